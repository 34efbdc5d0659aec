"""test helper (GPU box): WhisperMoP.sample(graph=True) -- one sampling step (decoder step + sample_tokens + the eos / sum update)
captured with torch.cuda.graph on one stream and replayed per token -- against eager sample, in fp32 and under bf16 autocast; prints
whether the sampler ran on the HIP kernel and whether tokens and sum_logprobs are bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=300, vocab_size=1000, n_text_ctx=96, n_embd=256, n_head=4, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
mel = torch.randn(2, 300, 16, device="cuda")
prompt = torch.randint(0, 1000, (2, 4), device="cuda")
kw = dict(temperature=0.7, top_k=50, top_p=0.95, num_samples=3, eos_token_id=7, seed=21)
ok = True
for autocast in (False, True):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        eager, se = m.sample(mel, prompt, 40, **kw)
        fused = ops.LAST_PATH.get("sample") == _lib.PATH_FUSED and ops.LAST_PATH.get("decode_attn_rows") == _lib.PATH_FUSED
        try:
            graphed, sg = m.sample(mel, prompt, 40, graph=True, **kw)
        except RuntimeError as e:
            print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
            sys.exit(0)
    torch.cuda.synchronize()
    same = torch.equal(eager, graphed) and torch.equal(se, sg)
    print(f"autocast={autocast} FUSED {fused} identical {same}", flush=True)
    ok = ok and same and fused
print("FUSED", ops.LAST_PATH.get("sample") == _lib.PATH_FUSED, flush=True)
print("GRAPH_IDENTICAL", ok, flush=True)
