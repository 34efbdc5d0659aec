"""test helper (GPU box): MoEMLP forward + backward (torch.autograd.grad: no AccumulateGrad) captured into one HIP graph on a single
stream with torch.cuda.graph and replayed twice; prints whether the kernels ran fused and whether both replays reproduce the eager
output and gradients bit for bit."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn.components import MoEMLP  # noqa: E402

torch.manual_seed(0)
m = MoEMLP(128, 4.0, 4).cuda().to(torch.bfloat16)
x = torch.randn(4, 200, 128, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
gout = torch.randn(4, 200, 128, device="cuda", dtype=torch.bfloat16)
res = torch.randn(4, 200, 128, device="cuda", dtype=torch.bfloat16)
ws = [l.weight for l in m.fc1] + [l.weight for l in m.fc2]


def step():
    y = m(x, residual=res)
    return (y,) + torch.autograd.grad(y, [x] + ws, gout)


eager = [t.detach().clone() for t in step()]
torch.cuda.synchronize()
print("FUSED", ops.LAST_PATH.get("moe_fwd") == _lib.PATH_FUSED and ops.LAST_PATH.get("moe_bwd") == _lib.PATH_FUSED, flush=True)
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    for _ in range(2):
        step()
torch.cuda.current_stream().wait_stream(s)
graph = torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(graph):
        static = step()
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
print("captured", flush=True)
ok = True
for _ in range(2):
    graph.replay()
    torch.cuda.synchronize()
    ok = ok and all(torch.equal(a, b) for a, b in zip(eager, static))
print("GRAPH_IDENTICAL", ok, flush=True)
