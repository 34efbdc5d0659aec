"""test helper (GPU box): forward + backward of ops.quartet_core and ops.token_gate_1d with per-row lengths (torch.autograd.grad: no
AccumulateGrad), captured once with torch.cuda.graph and replayed -- the static lens tensor included, rewritten between replays --
against eager; `bf16` (the fused kernels, default) or `fp32` (the generic path) as the argument.  Prints whether every output and
gradient is bit-identical.

The eager results are kept DETACHED.  A kept output that still carries its graph keeps the leaves' AccumulateGrad nodes alive on the
stream of the eager pass; the captured backward then hands its leaf gradients across streams, which pulls a second stream into the
capture (torch warns of an AccumulateGrad stream mismatch) and ends the capture with a segmentation fault -- see tools/graph_probe.py."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402

B, T, H, DK = 6, 200, 2, 64
LENS = [(200, 137, 128, 64, 2, 1), (1, 200, 0, 77, 129, 64)]


def step(ins, lens):
    q, k, v, q2, k2, mix, qs, x, u, dy = ins
    y = ops.quartet_core(q, k, v, q2, k2, mix, qs, None, 1e-5, True, lens=lens)
    out = ops.token_gate_1d(x, y.to(x.dtype), u, lens)
    grads = torch.autograd.grad(out, [q, k, v, q2, k2, mix, qs, x, u], dy)
    return [y, out, *grads]


ok = True
for dt in ((torch.float32,) if sys.argv[1:] == ["fp32"] else (torch.bfloat16,)):
    g = torch.Generator(device="cuda").manual_seed(0)
    ins = [torch.randn(B, T, H, DK, device="cuda", generator=g).to(dt).requires_grad_(True) for _ in range(5)]
    ins += [torch.tensor([0.3], device="cuda", requires_grad=True), torch.tensor([0.8], device="cuda", requires_grad=True)]
    ins += [torch.randn(B, T, H * DK, device="cuda", generator=g).to(dt).requires_grad_(True),
            (0.05 * torch.randn(3, H * DK, device="cuda", generator=g)).requires_grad_(True),
            torch.randn(B, T, H * DK, device="cuda", generator=g).to(dt)]
    lens = torch.tensor(LENS[0], dtype=torch.int32, device="cuda")
    eager = [[t.detach().clone() for t in step(ins, torch.tensor(v, dtype=torch.int32, device="cuda"))] for v in LENS]
    torch.cuda.synchronize()
    fused = ops.LAST_PATH["quartet_fwd"] == (_lib.PATH_FUSED if dt == torch.bfloat16 else _lib.PATH_GENERIC)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(ins, lens)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = step(ins, lens)
    except RuntimeError as e:
        print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
        sys.exit(0)
    print("captured", flush=True)
    for v, want in zip(LENS, eager):
        lens.copy_(torch.tensor(v, dtype=torch.int32, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(want, static))
        print(f"{dt} lens={v} PATH_AS_EXPECTED {fused} identical {same}", flush=True)
        ok = ok and same and fused
print("GRAPH_IDENTICAL", ok, flush=True)
