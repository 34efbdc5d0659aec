"""test helper (GPU box): WhisperMoP greedy decoding with statistics (with_logit_rules(...).generate(return_stats=True): every token
chosen by ops.greedy_pick) with graph=True -- one step with its logit_rules and greedy_pick launches captured with torch.cuda.graph
and replayed per token -- against the eager runs and against generate() without statistics, with and without logit rules, in fp32
and under bf16 autocast; prints whether the pick ran on the HIP kernel and whether tokens, step logits and all three statistics are
bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import LogitRules, WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=300, vocab_size=1000, n_text_ctx=96, n_embd=256, n_head=4, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
with torch.no_grad():
    m.dec_ln_f.weight.mul_(20.0)                 # peaked logits: text and timestamps both win steps
rules = LogitRules(1000, suppress_tokens=[1, 2, 500, 899], suppress_at_begin=[5, 800], timestamp_begin=900, eos_token_id=800,
                   no_timestamps_token_id=898, max_initial_timestamp_index=10)
mel = torch.randn(2, 300, 16, device="cuda")
prompt = torch.randint(0, 800, (2, 4), device="cuda")
ragged = [prompt[0], prompt[1, :2]]
kw = dict(return_logits=True, return_stats=True, no_speech_token_id=799, sot_index=1)
ok = True
for autocast in (False, True):
    for name, d, p in (("plain", m.with_logit_rules(None), prompt), ("rules", m.with_logit_rules(rules), prompt),
                       ("rules ragged", m.with_logit_rules(rules), ragged)):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            base = d.generate(mel, p, 40, eos_token_id=800)
            ops.LAST_PATH.pop("greedy_pick", None)
            toks, logits, st = d.generate(mel, p, 40, eos_token_id=800, **kw)
            fused = ops.LAST_PATH.get("greedy_pick") == _lib.PATH_FUSED and ops.LAST_PATH.get("token_logprob") == _lib.PATH_FUSED
            try:
                gtoks, glogits, gst = d.generate(mel, p, 40, eos_token_id=800, graph=True, **kw)
            except RuntimeError as e:
                print("CAPTURE_UNSUPPORTED", name, repr(e)[:300], flush=True)
                sys.exit(0)
        torch.cuda.synchronize()
        rows = lambda t: list(t) if isinstance(t, (list, tuple)) else [t]                                  # noqa: E731
        same = all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(rows(base), rows(toks), rows(gtoks)))
        same = same and torch.equal(logits, glogits) and all(torch.equal(a, b) for a, b in zip(st, gst))
        counted = bool((st.n_tokens >= 1).all()) and bool(torch.isfinite(st.sum_logprobs).all())
        print(f"autocast={autocast} {name} FUSED {fused} identical {same} n_tokens {st.n_tokens.tolist()}", flush=True)
        ok = ok and same and fused and counted
print("FUSED", ops.LAST_PATH.get("greedy_pick") == _lib.PATH_FUSED, flush=True)
print("GRAPH_IDENTICAL", ok, flush=True)
