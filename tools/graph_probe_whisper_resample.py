"""test helper (GPU box): one ops.resample call (a single launch) captured with torch.cuda.graph and replayed after the audio and
the lengths in its static buffers changed, against the eager op on the new contents; prints whether the call ran on the HIP kernel
and whether every replay, out_lens included, is bit-identical to eager."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402

B, C, L = 4, 2, 441 * 16 + 33
g = torch.Generator().manual_seed(0)
audio = (torch.randn(B, C, L, generator=g) * 0.1).cuda()
lens = torch.tensor([L, 1, 441 * 7 + 5, 2823], dtype=torch.int32).cuda()
ops.resample(audio, 44100, 16000, lens)                          # warm-up outside the capture: the tap table goes to the device
fused = ops.LAST_PATH.get("resample") == _lib.PATH_FUSED
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(graph):
        out, out_lens = ops.resample(audio, 44100, 16000, lens)
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
ok = True
for seed in (1, 2):
    g = torch.Generator().manual_seed(seed)
    audio.copy_(torch.randn(B, C, L, generator=g) * (0.1 * seed))
    lens.copy_(torch.tensor([441 * seed + 300, L, 0, L - seed], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager, eager_lens = ops.resample(audio, 44100, 16000, lens)
    close = float((out - ops.resample_torch(audio, 44100, 16000, lens)[0]).abs().max())
    ok = ok and torch.equal(out, eager) and torch.equal(out_lens, eager_lens) and close < 1e-5
print("FUSED", fused, flush=True)
print("REPLAY_IDENTICAL", ok, flush=True)
