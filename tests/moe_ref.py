"""float64 router reference, prescribed routes and gates that realise them, shared by the MoE route tests (test_moe_ref_cpu.py,
test_gpu_moe_routes.py).  Everything here runs on the CPU; the GPU tests move the tensors over."""
import math

import torch

MARGIN = 0.25               # least float64 top-1 - top-2 margin of a prescribed gate
UNDECIDED_CAP = 1e-3        # largest share of undecided tokens a router case may have: a condition on the inputs, not a tolerance

# the router cases: (M, D, E, x dtype, gate dtype, gate bias, seed).  The first six are the seeded draws of test_gpu_moe._case
# (x ~ N(0, 1), gate.weight ~ N(0, 1 / D), gate.bias ~ 0.1 N(0, 1)); then the dtype mixes, no bias, and M = 1, 3, 4, 5: partial
# four-wave workgroups of the logits kernel (one wave per token)
F32, BF16 = torch.float32, torch.bfloat16
ROUTER_CASES = [
    (4099, 384, 64, F32, F32, True, 0),
    (4099, 384, 64, BF16, BF16, True, 0),
    (3001, 72, 8, BF16, BF16, True, 1),
    (257, 8, 2, F32, F32, True, 2),
    (2049, 1024, 64, BF16, BF16, True, 3),
    (4099, 384, 4, BF16, BF16, True, 4),
    (3001, 72, 8, BF16, F32, True, 1),
    (4099, 384, 64, F32, BF16, True, 0),
    (2049, 1024, 64, BF16, BF16, False, 3),
    (257, 8, 2, F32, F32, False, 2),
    (1, 72, 8, F32, F32, True, 5),
    (3, 72, 8, BF16, BF16, True, 5),
    (4, 72, 8, F32, BF16, True, 5),
    (5, 72, 8, BF16, F32, True, 5),
]


def case_id(c):
    M, D, E, xdt, gdt, bias, seed = c
    n = {F32: "fp32", BF16: "bf16"}
    return f"M{M}-D{D}-E{E}-x{n[xdt]}-g{n[gdt]}-{'b' if bias else 'nob'}-s{seed}"


def router_case(M, D, E, xdt, gdt, bias, seed):
    """(x, gate.weight, gate.bias or None) of a router case, drawn on the CPU in fp32 and rounded to the case's dtypes"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g).to(xdt)
    gw = (torch.randn(E, D, generator=g) / D ** 0.5).to(gdt)
    gb = (0.1 * torch.randn(E, generator=g)).to(gdt)
    return x, gw, (gb if bias else None)


def route_ref64(x, gw, gb=None):
    """(logits, beta), both float64 (M, E) on the CPU: the gate logits x gw^T + gb of the operands as the kernel reads them (a bf16
    tensor widens to float64 exactly, so no input rounding enters) and the rounding bound of the kernel's fp32 evaluation,

        beta[t, e] = (ceil(D / 64) + 7) 2^-24 (sum_d |x[t, d] gw[e, d]| + |gb[e]|).

    The logits kernel gives a token one wave: lane l chains the ceil(D / 64) FMAs of d = l, l + 64, ...; a butterfly adds the 64
    partial sums in six steps; the bias adds once.  A product therefore passes through at most n = ceil(D / 64) + 6 + 1 fp32
    roundings, each of relative size u = 2^-24, on its way into the logit, and the bias through one.  The standard bound is
    gamma_n sum |terms| with gamma_n = n u / (1 - n u); beta is its first-order form n u sum |terms| (n u <= 23 * 2^-24 here, the
    second-order part is below 2e-6 of beta)."""
    x64 = x.detach().cpu().double().reshape(-1, x.shape[-1])
    w64 = gw.detach().cpu().double()
    logits = x64 @ w64.t()
    mag = x64.abs() @ w64.abs().t()
    if gb is not None:
        b64 = gb.detach().cpu().double()
        logits = logits + b64
        mag = mag + b64.abs()
    n = math.ceil(x64.shape[1] / 64) + 7
    return logits, n * 2.0 ** -24 * mag


def decide(logits, beta):
    """(top1, decided): the float64 argmax (lowest index among equals) and, per token, whether the top-1 - top-2 margin exceeds
    beta_top1 + beta_top2, i.e. whether every evaluation inside the bound picks the same expert"""
    i1 = logits.argmax(-1, keepdim=True)
    i2 = logits.scatter(1, i1, float("-inf")).argmax(-1, keepdim=True)
    margin = logits.gather(1, i1) - logits.gather(1, i2)
    return i1.squeeze(1), (margin > beta.gather(1, i1) + beta.gather(1, i2)).squeeze(1)


def admissible(logits, beta, got):
    """per token: may a router whose logits stay inside beta answer got[t]?  The float64 argmax always may; another expert e
    only when its logit is within beta_top1 + beta_e of the top"""
    top1 = logits.argmax(-1, keepdim=True)
    g = got.reshape(-1, 1).long()
    gap = logits.gather(1, top1) - logits.gather(1, g)
    return (gap <= beta.gather(1, top1) + beta.gather(1, g)).squeeze(1) | (g == top1).squeeze(1)


def counts_to_route(counts, order, seed=0):
    """int64 (sum(counts),) route with counts[e] tokens of expert e.  order "sorted": expert 0's tokens first, and so on;
    "reversed": the last expert's first; "shuffled": a seeded permutation of the sorted route"""
    r = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(list(counts), dtype=torch.int64))
    if order == "sorted":
        return r
    if order == "reversed":
        return r.flip(0)
    if order == "shuffled":
        return r[torch.randperm(r.numel(), generator=torch.Generator().manual_seed(seed))]
    raise ValueError(order)


def prescribed_gate(route, D, E, dtype):
    """(x_patch, gate.weight, gate.bias) that send token t to route[t] with a float64 margin of at least MARGIN, every value exact
    in bf16 and fp32 alike.  x_patch (M, P) replaces the first P columns of any x; the gate reads no other column.
      E <= D: gate.weight[e] = 8 unit(e), no offset in the bias, x_patch = 4 onehot(route): logit 32 for the routed expert and 0
              for the others.  Gate and x_patch in `dtype`.
      E > D:  a one-coordinate code, gate.weight[e, 0] = e, gate.bias[e] = -e^2 / 2, x_patch[t, 0] = route[t]: logit
              (r^2 - (e - r)^2) / 2, so the routed expert leads its neighbours by 1 / 2.  e^2 / 2 needs more than bf16's eight
              bits, so this gate is fp32 whatever `dtype`; x_patch (integers up to 63) is in `dtype`."""
    route = route.long()
    M = route.numel()
    if E <= D:
        gw = torch.zeros(E, D)
        gw[torch.arange(E), torch.arange(E)] = 8.0
        gb = torch.zeros(E)
        xp = torch.zeros(M, E)
        xp[torch.arange(M), route] = 4.0
        return xp.to(dtype), gw.to(dtype), gb.to(dtype)
    gw = torch.zeros(E, D)
    gw[:, 0] = torch.arange(E, dtype=torch.float32)
    gb = -0.5 * torch.arange(E, dtype=torch.float32) ** 2
    return route.reshape(M, 1).to(dtype), gw, gb


def patched(x, x_patch):
    """x with its first columns replaced by x_patch (cast to x's dtype: the patch values are exact in both)"""
    x = x.clone()
    x[:, :x_patch.shape[1]] = x_patch.to(x.dtype)
    return x
