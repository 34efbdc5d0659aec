"""test helper (GPU box): ops.cross_entropy + backward and ops.linear_cross_entropy + backward, each captured with torch.cuda.graph on
one stream and replayed after the logits / activations and the targets in their static buffers changed.  The cross-entropy replay
must equal the eager op on the new contents bit for bit; the chunked head loss and its gradients are held, against float64, to twice
the error of the unchunked torch head plus 160 x 2^-24 of each result's largest entry (the kernels' own rounding at this V: 4 x the
summation depth of 31, 2 ln V, |lse| and |loss| stay under 160; a chunk's GEMM may run another hipBLASLt kernel than the whole one).  Prints whether the calls ran on the HIP kernels and the two verdicts."""
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402

R, V, M, D, CHUNK = 5, 8 * 1024 + 3, 37, 24, 8


def draw(seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (R,), generator=g)
    t[seed % R] = -100
    th = torch.randint(0, V, (M,), generator=g)
    th[(3 * seed) % M] = -100
    return (torch.randn(R, V, generator=g) * seed, t, torch.randn(M, D, generator=g), torch.randn(V, D, generator=g) * 0.3,
            torch.randn(V, generator=g) * 0.1, th)


def ce(x, t):
    loss = ops.cross_entropy(x, t)
    return loss, torch.autograd.grad(loss, x)[0]


def head(h, w, b, t):
    loss = ops.linear_cross_entropy(h, w, t, b, chunk_rows=CHUNK)
    return (loss,) + torch.autograd.grad(loss, (h, w, b))


def head_torch(h, w, b, t):
    loss = F.cross_entropy(F.linear(h, w, b), t)
    return (loss,) + torch.autograd.grad(loss, (h, w, b))


x, t, h, w, b, th = [v.cuda() for v in draw(1)]
x, h, w, b = [v.requires_grad_() for v in (x, h, w, b)]
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):                                    # warm-up outside the capture: the GEMMs' workspaces
    ce(x, t), head(h, w, b, th)
torch.cuda.current_stream().wait_stream(side)
fused = (ops.LAST_PATH.get("cross_entropy_fwd") == ops.LAST_PATH.get("cross_entropy_bwd")
         == ops.LAST_PATH.get("linear_cross_entropy") == _lib.PATH_FUSED)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(graph):
        out_ce = ce(x, t)
        out_head = head(h, w, b, th)
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
same, within = True, True
for seed in (2, 3):
    new = draw(seed)
    with torch.no_grad():
        for dst, src in zip((x, t, h, w, b, th), new):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    same = same and all(torch.equal(a, e) for a, e in zip(out_ce, ce(x, t)))
    whole = head_torch(h, w, b, th)
    h64, w64, b64 = [v.detach().double().cpu().requires_grad_() for v in (h, w, b)]
    want = head_torch(h64, w64, b64, th.cpu())
    for got, wh, wa in zip(out_head, whole, want):
        err, err_whole = float((got.double().cpu() - wa).abs().max()), float((wh.double().cpu() - wa).abs().max())
        within = within and err <= 2 * err_whole + 160 * 2.0 ** -24 * float(wa.abs().max())
print("FUSED", fused, flush=True)
print("CE_REPLAY_IDENTICAL", same, flush=True)
print("LINEAR_REPLAY_WITHIN_RULE", within, flush=True)
