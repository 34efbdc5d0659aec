"""test helper (GPU box): one ops.log_mel call (the tile launch, then the clamp launch: a straight line) captured with
torch.cuda.graph and replayed after the audio and the lengths in its static buffers changed, against the eager op on the new
contents; prints whether the call ran on the HIP kernels and whether every replay is bit-identical to eager."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402

B, L = 4, 160 * 70 + 33
g = torch.Generator().manual_seed(0)
audio = (torch.randn(B, L, generator=g) * 0.1).cuda()
lens = torch.tensor([L, 201, 160 * 32 + 5, 160 * 33], dtype=torch.int32).cuda()
filt = ops.mel_filterbank(16000, 400, 80, device="cuda")
ops.log_mel(audio, filt, lens=lens)                              # warm-up outside the capture: tables, bands, the LDS limit
fused = ops.LAST_PATH.get("log_mel") == _lib.PATH_FUSED
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(graph):
        out = ops.log_mel(audio, filt, lens=lens)
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
ok = True
for seed in (1, 2):
    g = torch.Generator().manual_seed(seed)
    audio.copy_(torch.randn(B, L, generator=g) * (0.1 * seed))
    lens.copy_(torch.tensor([160 * seed + 300, L, 160 * 64, L - seed], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.log_mel(audio, filt, lens=lens)
    close = float((out - ops.log_mel_torch(audio, filt, lens=lens)).abs().max())
    ok = ok and torch.equal(out, eager) and close < 1e-4
print("FUSED", fused, flush=True)
print("REPLAY_IDENTICAL", ok, flush=True)
