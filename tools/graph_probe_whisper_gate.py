"""test helper (GPU box): WhisperMoP.encode -- the taps fold, ops.mel_gate for all layers and ops.gated_residual per block -- and
ops.mel_gate with per-clip lengths, each captured with torch.cuda.graph on one stream (the warm-up outside the capture) and replayed
on new mel values, against eager, in fp32 and under bf16 autocast; prints whether the kernels ran and whether every output is
bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=150, vocab_size=200, n_text_ctx=32, n_embd=128, n_head=2, n_layer_enc=3, n_layer_dec=1)
m = WhisperMoP(cfg).cuda().eval()
with torch.no_grad():
    for blk in m.encoder:
        blk.mop.fuse.alpha.copy_(torch.rand(2) + 0.5)
lens = torch.tensor([150, 1, 77], dtype=torch.int32).cuda()
taps = ops.mel_gate_taps(*(torch.randn(s, device="cuda") for s in ((3, 5, 1, 1), (3, 3, 5, 5, 5), (3, 2, 8, 1, 1), (3, 2))), 16)
calls = {"encode": lambda mel: m.encode(mel), "mel_gate_lens": lambda mel: (ops.mel_gate(mel, taps, lens),)}

ok = True
for autocast in (False, True):
    for name, call in calls.items():
        static = torch.randn(3, 150, 16, device="cuda")
        fresh = torch.randn(3, 150, 16, device="cuda")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                             # warm-up: allocations and lazy initialisation
                call(static)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    out = call(static)
            except RuntimeError as e:
                print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
                sys.exit(0)
            fused = ops.LAST_PATH.get("mel_gate_fwd") == _lib.PATH_FUSED
            if name == "encode":
                fused = fused and ops.LAST_PATH.get("gated_residual_fwd") == _lib.PATH_FUSED
            static.copy_(fresh)
            graph.replay()
            torch.cuda.synchronize()
            eager = call(fresh)
        torch.cuda.synchronize()
        same = len(out) == len(eager) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(out, eager))
        print(f"{name} autocast={autocast} FUSED {fused} identical {same}", flush=True)
        ok = ok and same and fused
print("GRAPH_IDENTICAL", ok, flush=True)
