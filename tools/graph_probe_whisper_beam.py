"""test helper (GPU box): WhisperMoP.beam_search(graph=True) -- one beam step (decoder step + beam_step) captured with
torch.cuda.graph on one stream and replayed per token -- against eager beam_search, in fp32 and under bf16 autocast; prints whether
the row-indirect attention and the beam step ran on the HIP kernels and whether tokens and scores are bit-identical."""
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
ok = True
for autocast in (False, True):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        eager, se = m.beam_search(mel, prompt, 40, 5, eos_token_id=7)
        fused = ops.LAST_PATH.get("decode_attn_rows") == _lib.PATH_FUSED and ops.LAST_PATH.get("beam_step") == _lib.PATH_FUSED
        try:
            graphed, sg = m.beam_search(mel, prompt, 40, 5, eos_token_id=7, graph=True)
        except RuntimeError as e:
            print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
            sys.exit(0)
    torch.cuda.synchronize()
    same = torch.equal(eager, graphed) and torch.equal(se, sg)
    print(f"autocast={autocast} FUSED {fused} identical {same}", flush=True)
    ok = ok and same and fused
print("FUSED", ops.LAST_PATH.get("beam_step") == _lib.PATH_FUSED, flush=True)
print("GRAPH_IDENTICAL", ok, flush=True)
