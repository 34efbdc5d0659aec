"""test helper (GPU box): WhisperMoP.generate / beam_search / sample on a list of clips of different lengths (and a ragged prompt
list) with graph=True -- one step captured with torch.cuda.graph on one stream and replayed per token, the static audio_lens tensor
included -- against eager, in fp32 and under bf16 autocast; prints whether the length-aware kernels ran and whether every output
is bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=300, vocab_size=1000, n_text_ctx=96, n_embd=256, n_head=4, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
clips = [torch.randn(n, 16, device="cuda") for n in (300, 137, 64, 1)]
prompts = [torch.randint(0, 1000, (n,), device="cuda") for n in (1, 4, 17, 40)]
calls = {"generate": lambda g: (m.generate(clips, prompts, 30, eos_token_id=7, graph=g),),
         "beam_search": lambda g: m.beam_search(clips, prompts, 30, 3, eos_token_id=7, graph=g),
         "sample": lambda g: m.sample(clips, prompts, 30, temperature=0.7, top_k=50, top_p=0.95, num_samples=3, eos_token_id=7,
                                      seed=21, graph=g)}


def flat(out):
    return [t for o in out for t in (o if isinstance(o, list) else [o])]


ok = True
for autocast in (False, True):
    for name, call in calls.items():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            eager = flat(call(False))
            fused = ops.LAST_PATH.get("decode_attn_lens") == _lib.PATH_FUSED
            try:
                graphed = flat(call(True))
            except RuntimeError as e:
                print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
                sys.exit(0)
        torch.cuda.synchronize()
        same = len(eager) == len(graphed) and all(torch.equal(a, b) for a, b in zip(eager, graphed))
        print(f"{name} autocast={autocast} FUSED {fused} identical {same}", flush=True)
        ok = ok and same and fused
print("GRAPH_IDENTICAL", ok, flush=True)
