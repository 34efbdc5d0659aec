"""The tensor lists of the FusedAdamW tests and the step-by-step comparison against optim_ref, shared by the CPU and the GPU tests
(the CPU suite checks torch's own AdamW on the very lists the GPU test uses)."""
import torch

import optim_ref as R
from mop_amd import _lib

C = _lib.ADAMW_CHUNK
SIZES = (0, 1, 7, C - 1, C, C + 1, 3 * C + 5)
F32, BF16 = torch.float32, torch.bfloat16
HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-2)


def view_at(values: torch.Tensor, offset: int) -> torch.Tensor:
    """a contiguous tensor holding `values` that starts `offset` elements into its storage"""
    buf = torch.zeros(values.numel() + offset, dtype=values.dtype, device=values.device)
    buf[offset:].copy_(values.reshape(-1))
    return buf[offset:].view(values.shape)


def mixed_list(device, seed=0):
    """every size as (fp32 p, fp32 g), (bf16 p, bf16 g) and (fp32 p, bf16 g), plus an fp32 and a bf16 parameter that are views
    starting one element into their storage -> (params, grad dtypes)"""
    gen = torch.Generator().manual_seed(seed)
    params, gdt = [], []
    for n in SIZES:
        for pd, gd in ((F32, F32), (BF16, BF16), (F32, BF16)):
            params.append(torch.randn(n, generator=gen).to(pd).to(device))
            gdt.append(gd)
    for pd in (F32, BF16):
        params.append(view_at(torch.randn(C + 9, generator=gen).to(pd).to(device), 1))
        gdt.append(pd)
    params = [torch.nn.Parameter(p) for p in params]
    for p, d in zip(params, gdt):
        if d != p.dtype:
            p.grad_dtype = d            # a bf16 gradient on an fp32 parameter
    return params, gdt


def grads_for(params, gdt, step, scale=1.0, seed=100):
    gen = torch.Generator().manual_seed(seed + step)
    return [(scale * torch.randn(p.shape, generator=gen)).to(d).to(p.device) for p, d in zip(params, gdt)]


def state_of(opt, p, ema):
    st = opt.state.get(p, {})
    z = torch.zeros(p.shape, dtype=F32, device=p.device)
    out = dict(p=p.detach().clone(), m=st["exp_avg"].clone() if "exp_avg" in st else z, v=st["exp_avg_sq"].clone() if "exp_avg_sq" in st else z,
               step=int(st["step"]) if "step" in st else 0)
    if ema:
        out["ema"] = st["ema"].clone() if "ema" in st else p.detach().clone()
    return out


def checked_step(opt, params, step_grads, *, hypers, max_grad_norm=None, ema_decay=None, norm=None, what=""):
    """give the parameters their gradients (None: no gradient), take one opt.step() and check every tensor against optim_ref from
    the state stored before the step.  hypers: one dict per parameter.  norm: the optimiser's norm when it takes one (checked
    here against float64).  Returns the largest share of a bound used, per output."""
    before = [state_of(opt, p, ema_decay is not None) for p in params]
    for p, g in zip(params, step_grads):
        p.grad = g
    kept = [g.clone() for g in step_grads if g is not None]
    opt.step()
    assert all(torch.equal(a, b) or (a != a).any() for a, b in zip(kept, [g for g in step_grads if g is not None])), "a gradient was modified"
    coef, eps_c = 1.0, 0.0
    shares = {}
    if norm is not None:
        ref, nb = R.ref_norm(kept), R.norm_bound(kept, C)
        got = float(norm())
        assert abs(got - ref) <= nb, f"{what}: norm {got!r} against {ref!r}, bound {nb:.3g}"
        shares["norm"] = abs(got - ref) / nb
        coef, eps_c = R.coef_and_eps(ref, max_grad_norm, nb / ref if ref > 0 else 0.0)
    for i, (p, g, b, h) in enumerate(zip(params, step_grads, before, hypers)):
        after = state_of(opt, p, ema_decay is not None)
        if g is None:
            assert after["step"] == b["step"] and all(torch.equal(after[k], b[k]) for k in b if k != "step"), f"{what}: tensor {i} has no gradient"
            continue
        assert after["step"] == b["step"] + 1, f"{what}: tensor {i} step {after['step']}"
        b["g"] = g
        s = R.check_step(b, after, b["step"], coef=coef, eps_c=eps_c, hyper=h, ema_decay=ema_decay, what=f"{what} tensor {i} n={p.numel()}")
        for k, x in s.items():
            shares[k] = max(shares.get(k, 0.0), x)
    return shares


def torch_reference_alone(params, gdt, steps, max_grad_norm):
    """torch.optim.AdamW in fp32 (and clip_grad_norm_ before it) on the list's values, checked against optim_ref's bounds"""
    ps = [torch.nn.Parameter(p.detach().to("cpu", F32).clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=HYPER["weight_decay"])
    shares = {}
    for s in range(steps):
        grads = [g.to("cpu", F32) for g in grads_for(params, gdt, s)]
        before = [dict(state_of(opt, p, False), g=g.clone()) for p, g in zip(ps, grads)]
        for p, g in zip(ps, grads):
            p.grad = g
        coef, eps_c = 1.0, 0.0
        if max_grad_norm is not None:
            ref, nb = R.ref_norm([b["g"] for b in before]), R.norm_bound([b["g"] for b in before], C)
            got = float(torch.nn.utils.clip_grad_norm_(ps, max_grad_norm))
            assert abs(got - ref) <= nb
            coef, eps_c = R.coef_and_eps(ref, max_grad_norm, nb / ref)
        opt.step()
        for i, (p, b) in enumerate(zip(ps, before)):
            if p.numel() == 0:
                continue
            sh = R.check_step(b, state_of(opt, p, False), b["step"], coef=coef, eps_c=eps_c, hyper=HYPER, what=f"torch step {s} tensor {i}")
            for k, x in sh.items():
                shares[k] = max(shares.get(k, 0.0), x)
    return shares
