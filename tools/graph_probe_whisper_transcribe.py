"""test helper (GPU box): (1) one ops.timestamp_segments launch captured with torch.cuda.graph and replayed after its static token
and window buffers changed, against the eager op and the torch restatement on the new contents; (2) WhisperMoP.transcribe with
graph=True (every window's decoder step captured and replayed) against the eager run, greedy and with three beams, under bf16
autocast; prints whether the segments ran on the HIP kernel and whether everything is bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import LogitRules, WhisperConfig, WhisperMoP  # noqa: E402

TB, EOS, V = 101, 97, 131


def rows(R, T, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(R, T, generator=g)
    tok = torch.randint(0, EOS, (R, T), generator=g)
    tok = torch.where(u < 0.4, TB + torch.randint(0, 7, (R, T), generator=g), tok)
    return torch.where(u < 0.03, EOS, tok).to(torch.int32)


def same(x, y):
    return all(torch.equal(p, q) for p, q in zip(x, y))


# (1) the op
tok, win = rows(5, 70, 1).cuda(), torch.tensor([40, 33, 1, 64, 17], dtype=torch.int32).cuda()
ops.timestamp_segments(tok, 3, win, TB, EOS, 2)                  # warm-up outside the capture
fused = ops.LAST_PATH.get("timestamp_segments") == _lib.PATH_FUSED
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(g):
        out = ops.timestamp_segments(tok, 3, win, TB, EOS, 2)
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
ok = True
for seed in (2, 3):
    tok.copy_(rows(5, 70, seed))
    win.copy_(torch.tensor([seed, 64, 9, 40, 40], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    want = ops.timestamp_segments_torch(tok, 3, win, TB, EOS, 2)
    ok = ok and same(out, want) and same(out, ops.timestamp_segments(tok, 3, win, TB, EOS, 2))
print("FUSED", fused, flush=True)
print("OP_REPLAY_IDENTICAL", ok, flush=True)

# (2) the loop
torch.manual_seed(0)
cfg = WhisperConfig(n_mels=12, n_audio_ctx=64, vocab_size=V, n_text_ctx=64, n_embd=128, n_head=2, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
with torch.no_grad():
    m.dec_ln_f.weight.mul_(20.0)                 # peaked logits: text and timestamps both win steps
rules = LogitRules(V, suppress_tokens=[1, 2], suppress_at_begin=[5, EOS], timestamp_begin=TB, eos_token_id=EOS,
                   no_timestamps_token_id=100, max_initial_timestamp_index=4)
clips = [torch.randn(n, 12, device="cuda") for n in (150, 64, 37)]
prompt = torch.tensor([7, 8, 9], device="cuda")
ok = True
for beams in (1, 3):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        eager = m.transcribe(clips, prompt, rules, 12, num_beams=beams)
        try:
            graphed = m.transcribe(clips, prompt, rules, 12, num_beams=beams, graph=True)
        except RuntimeError as e:
            print("CAPTURE_UNSUPPORTED", beams, repr(e)[:300], flush=True)
            sys.exit(0)
    torch.cuda.synchronize()
    one = all(same(a, b) for a, b in zip(eager, graphed))
    print(f"num_beams={beams} segments {[int(t.starts.numel()) for t in eager]} identical {one}", flush=True)
    ok = ok and one
print("GRAPH_IDENTICAL", ok, flush=True)
