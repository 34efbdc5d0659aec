"""Float64 statement of one fused AdamW step (include/mopk.h, "Fused AdamW step") and the error bounds of its fp32 evaluation.

`ref_step` takes the STORED inputs of a step (fp32 / bf16 tensors, widened exactly) and returns what the step would give in real
arithmetic, to float64 accuracy.  `bounds` returns, per element, how far an fp32 evaluation of the documented formulae may lie from
that; `check_step` compares.  A multi-step test calls them once per step on the state the code under test stored, so every bound is
a one-step bound.

The bounds count fp32 roundings, u = 2^-24 (round to nearest), gamma(k) = (1 + u)^k - 1; no constant is tuned.
  coef    exact 1 without clipping.  With clipping it carries the norm's relative error plus 3 roundings (the sum with 1e-6, the
          rounded max_norm, the division): eps_c.
  g'      fl(coef * g): relative (1 + eps_c)(1 + u) - 1.
  m       at most three roundings plus the rounded constant, each on a quantity no larger than |m| + |g'|:
          ((1 + u)^4 (1 + eps_c) - 1) (|m| + |g'|).  (torch's lerp form m + (1 - b1)(g' - m) stays inside it as well.)
  v       all terms are non-negative, so the bound is relative: the g' term sees the rounded constant, two products and the sum on
          a squared g':  rel_v = (1 + u)^4 ((1 + eps_c)(1 + u))^2 - 1.
  p       p * decay: rounded constant and product, gamma(2) |p decay|.  denom = sqrt(v) / sqrt(bc2) + eps: sqrt of a v that is off
          by rel_v, three roundings (sqrt, rounded sqrt(bc2), division), then the sum of two non-negative terms (eps rounded once):
          rel_d = sqrt(1 + rel_v) (1 + u)^4 - 1.  Quotient q = m / denom: E_m / (denom (1 - rel_d)) + |q| rel_d / (1 - rel_d), one
          rounding.  Update term step_size * q: rounded constant and product.  The final subtraction: one rounding of the result.
  bf16 p  half a bf16 ulp on top (one round-to-nearest-even from the fp32 result): 2^-9 times the power of two above |p|.  (As a
          multiple of |p| itself half an ulp reaches 2^-8 |p| just above a power of two -- bf16 keeps 8 significant bits -- so
          2^-9 |p| cannot be met by any rounding, torch's included; half an ulp is the format's own, tighter statement.)
  ema     fl(d) ema + fl(1 - d) p_stored: two roundings plus the rounded constants on |d ema| + |(1 - d) p|, plus (1 - d) times
          the bound of p (the reference averages its own p); a bf16 EMA adds half a bf16 ulp.
  norm    a thread squares (1 rounding) and adds its CHUNK / 256 vector elements and at most 2 head / tail elements serially, the
          wave tree adds 6 levels, the 4 waves 3 more: K roundings on non-negative terms, relative gamma(K) on the sum of squares.
          The partials are summed in double (2^-40 covers it), the square root is taken in double and rounded once.  A square
          below fp32's normal range may be flushed: sqrt(n 2^-126) absolute.
Every elementwise bound carries 2^-126 absolute for results in the subnormal range.
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
NORM_THREADS = 256          # threads of the sum-of-squares workgroup (include/mopk.h)
WAVE = 64


def gamma(k: int) -> float:
    return (1.0 + U) ** k - 1.0


def bf16_half_ulp(x):
    """half the spacing of the bf16 grid at |x| (8 significant bits): 2^-9 times the power of two above |x|"""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.full_like(x, 2.0 ** -9), e)


def f64(t):
    return t.detach().to("cpu", torch.float64)


def ref_norm(grads) -> float:
    return math.sqrt(sum(float((f64(g) ** 2).sum()) for g in grads))


def norm_bound(grads, chunk: int) -> float:
    """absolute bound on |norm_fp32 - ref_norm| for the documented summation order"""
    n = sum(g.numel() for g in grads)
    K = 1 + (chunk // NORM_THREADS + 2) + int(math.log2(WAVE)) + (NORM_THREADS // WAVE - 1)
    rel = math.sqrt(1.0 + gamma(K) + 2.0 ** -40) * (1.0 + U) - 1.0
    return rel * ref_norm(grads) + math.sqrt(n * TINY)


def coef_and_eps(norm: float, max_grad_norm, norm_rel: float):
    """(clip coefficient in real arithmetic, its relative error bound eps_c)"""
    if max_grad_norm is None:
        return 1.0, 0.0
    c = max_grad_norm / (norm + 1e-6)
    # below 1 by less than its own error: the fp32 evaluation may land on either side, both within eps_c of min(1, c)
    return min(1.0, c), (1.0 + norm_rel) * (1.0 + U) ** 3 - 1.0


def ref_step(p, g, m, v, ema, step: int, *, coef=1.0, lr, beta1, beta2, eps, weight_decay, ema_decay=None):
    """one tensor's step in float64 from the stored inputs -> dict(p, m, v, ema, gp)"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    k = step + 1
    bc1, bc2 = 1.0 - beta1 ** k, 1.0 - beta2 ** k
    gp = coef * g
    pd = p * (1.0 - lr * weight_decay)
    m2 = beta1 * m + (1.0 - beta1) * gp
    v2 = beta2 * v + (1.0 - beta2) * gp * gp
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    q = m2 / denom
    p2 = pd - (lr / bc1) * q
    out = dict(p=p2, m=m2, v=v2, gp=gp, pd=pd, q=q, denom=denom, m_in=m, step_size=lr / bc1)
    if ema_decay is not None:
        out["ema"] = ema_decay * f64(ema) + (1.0 - ema_decay) * p2
        out["ema_in"] = f64(ema)
    return out


def bounds(r: dict, *, eps_c=0.0, p_bf16=False, ema_decay=None):
    """per-element absolute bounds for the outputs of ref_step's dict r"""
    u1 = 1.0 + U
    E_m = (u1 ** 4 * (1.0 + eps_c) - 1.0) * (r["m_in"].abs() + r["gp"].abs()) + TINY
    rel_v = u1 ** 4 * ((1.0 + eps_c) * u1) ** 2 - 1.0
    E_v = rel_v * r["v"] + TINY
    rel_d = math.sqrt(1.0 + rel_v) * u1 ** 4 - 1.0
    E_q = (E_m / (r["denom"] * (1.0 - rel_d)) + r["q"].abs() * rel_d / (1.0 - rel_d)) * u1 + U * r["q"].abs()
    E_t = r["step_size"] * (E_q * u1 ** 2 + gamma(2) * r["q"].abs())
    E_p = (gamma(2) * r["pd"].abs() + E_t) * u1 + U * r["p"].abs() + TINY
    if p_bf16:
        E_p = E_p + bf16_half_ulp(r["p"].abs() + E_p)
    out = dict(m=E_m, v=E_v, p=E_p)
    if ema_decay is not None:
        E_e = gamma(3) * (ema_decay * r["ema_in"].abs() + (1.0 - ema_decay) * r["p"].abs()) * u1 + (1.0 - ema_decay) * E_p * u1 + TINY
        if p_bf16:
            E_e = E_e + bf16_half_ulp(r["ema"].abs() + E_e)
        out["ema"] = E_e
    return out


def check_step(before, after, step: int, *, coef=1.0, eps_c=0.0, hyper, ema_decay=None, what=""):
    """before / after: dicts p, g, m, v(, ema) of one tensor around a step; asserts every output inside its bound and returns the
    largest used share of a bound per output"""
    r = ref_step(before["p"], before["g"], before["m"], before["v"], before.get("ema"), step, coef=coef, ema_decay=ema_decay, **hyper)
    b = bounds(r, eps_c=eps_c, p_bf16=before["p"].dtype == torch.bfloat16, ema_decay=ema_decay)
    share = {}
    for k in b:
        err = (f64(after[k]) - r[k]).abs()
        bad = err > b[k]
        assert not bool(bad.any()), (f"{what} {k}: {int(bad.sum())} of {err.numel()} elements outside the bound; worst "
                                     f"err / bound = {float((err / b[k]).max()):.3g}")
        share[k] = float((err / b[k]).max()) if err.numel() else 0.0
    return share
