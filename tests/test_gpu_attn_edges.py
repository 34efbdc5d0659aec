"""-m gpu: the attention cores where trained models take them and N(0, 1) inputs do not.

Peaked logits: logit standard deviations 1 to 32 on every core (SDPA square / causal / rectangular / packed, MultiHop, the folded
CrossView core, Quartet, the decode kernels) against float64 on the operands the kernels read, with ONE bound at every scale.
Fully blocked rows: a mask that blocks whole rows (and rows open at a single key at either end, or past a blocked first tile) gives
y = 0 and dq = 0 on those rows and the reference's dk, dv; an additive -inf key-padding bias (Whisper cross-attention) likewise.
A bias that requires grad is refused rather than silently given no gradient."""
import numpy as np
import pytest
import torch

from attn_ref import bf16_exact, blocked_rows_mask, logit_qk, logit_std, sdpa_ref64
from gpu_util import max_abs

pytestmark = pytest.mark.gpu
SIGMAS = [1, 4, 8, 16, 32]
MODES = ["bf16-fused", "bf16-generic", "fp32-generic"]
YTOL, GTOL, GFLOOR = 1e-2, 1.5e-2, 1e-2       # y: max-abs / max|y_ref|; gradients: as _grad_errs, floor 1e-2 x the largest gradient


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _mode(mode):
    import mop_amd
    from mop_amd import ops
    prec, path = mode.split("-")
    mop_amd.set_precision(prec)
    ops.set_path(path)
    return prec, path


def _io(io):
    return torch.float32 if io == "fp32" else torch.bfloat16


def _yerr(y, yr):
    y, yr = np.asarray(y, np.float64), np.asarray(yr, np.float64)
    return max_abs(y, yr) / max(float(np.abs(yr).max()), 1e-30)


def _gerrs(got, ref, floor=GFLOOR):
    """{name: max-abs error / max(max|ref|, floor x the call's largest reference gradient)} (test_gpu_whisper._grad_errs)"""
    ref = {n: np.asarray(r, np.float64) for n, r in ref.items()}
    gscale = max(float(np.abs(r).max()) for r in ref.values())
    return {n: max_abs(np.asarray(got[n], np.float64), r) / max(float(np.abs(r).max()), floor * gscale, 1e-30) for n, r in ref.items()}


def _assert_close(y, yr, got, ref, what):
    assert np.isfinite(np.asarray(y, np.float64)).all() and all(np.isfinite(np.asarray(g, np.float64)).all() for g in got.values()), what
    ey = _yerr(y, yr)
    assert ey <= YTOL, f"{what}: y {ey:.3e}"
    for n, e in _gerrs(got, ref).items():
        assert e <= GTOL, f"{what}: {n} {e:.3e}"


def _np(t):
    return t.detach().double().cpu().numpy()


def _hp(t):
    """(B,N,H,dk) torch -> (B,H,N,dk) float64 numpy (the oracle layout)"""
    return np.transpose(_np(t), (0, 2, 1, 3))


# ---------------------------------------------------------------- logit-magnitude sweep
SDPA_SHAPES = [(130, 65, "rect"), (200, 1500, "rect"), (448, 1500, "rect"), (197, 197, "causal"), (197, 197, "packed")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("N,Nk,kind", SDPA_SHAPES)
def test_sdpa_logit_scale_sweep(N, Nk, kind, sigma, dk, io, mode):
    from mop_amd import _lib, ops
    prec, path = _mode(mode)
    dt = _io(io)
    B, H = 1, 2
    g = torch.Generator(device="cuda").manual_seed(1000 * sigma + N + dk)
    q, k = logit_qk((B, N, H, dk), (B, Nk, H, dk), sigma, g)
    v = torch.randn(B, Nk, H, dk, device="cuda", generator=g)
    q, k, v = (bf16_exact(t).to(dt) for t in (q, k, v))
    w = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g))   # dy as the kernels read it
    causal = kind == "causal"
    if kind == "packed":
        qkv = torch.stack([q, k, v], 2).requires_grad_(True)
        y = ops.sdpa_core(qkv)
        (y.float() * w).sum().backward()
        got = {n: qkv.grad[:, :, i].float().cpu().numpy() for i, n in enumerate(("dq", "dk", "dv"))}
    else:
        ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
        y = ops.sdpa_core(*ts, causal=causal)
        (y.float() * w).sum().backward()
        got = {n: t.grad.float().cpu().numpy() for n, t in zip(("dq", "dk", "dv"), ts)}
    want = _lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC
    assert ops.LAST_PATH["sdpa_fwd"] == want and ops.LAST_PATH["sdpa_bwd"] == want
    r = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    yr = sdpa_ref64(*r, causal=causal)
    (yr * w.double()).sum().backward()
    ref = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}
    _assert_close(y.detach().float().cpu().numpy(), yr.detach().cpu().numpy(), got, ref, f"logit std {logit_std(q, k):.2f}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("sigma", [1, 8, 32])
def test_sdpa_exact_ties_across_key_tiles(sigma, dk, mode):
    """rows 0-3: the row's largest-logit key copied into the second and third key tiles and the last, partial one (Nk = 200), so
    the online max meets the same, bit-identical score in four tiles"""
    from mop_amd import ops
    _mode(mode)
    B, N, Nk, H = 1, 130, 200, 2
    g = torch.Generator(device="cuda").manual_seed(sigma + dk)
    q, k = logit_qk((B, N, H, dk), (B, Nk, H, dk), sigma, g)
    q, k = bf16_exact(q), bf16_exact(k)
    tops = {(r, h): int((k[0, :, h] @ q[0, r, h]).argmax()) for r in range(4) for h in range(H)}
    free = [[j for j in range(a, b) if j not in tops.values()] for a, b in ((64, 128), (128, 192), (192, 200))]
    for (r, h), top in tops.items():
        for tile in free:                      # one copy per later tile; no copy overwrites another row's maximum
            k[0, tile[r], h] = k[0, top, h]
    v = bf16_exact(torch.randn(B, Nk, H, dk, device="cuda", generator=g))
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())[0, :, :4]
    assert all(int((s[h, r] == s[h, r].max()).sum()) >= 4 for h in range(H) for r in range(4))      # exact ties in the scores
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    w = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g))
    y = ops.sdpa_core(q, k, v)
    (y * w).sum().backward()
    r_ = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    yr = sdpa_ref64(*r_)
    (yr * w.double()).sum().backward()
    got = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), (q, k, v))}
    ref = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r_)}
    _assert_close(y.detach().cpu().numpy(), yr.detach().cpu().numpy(), got, ref, f"ties, logit std {logit_std(q, k):.2f}")


GATES = (0.8, 0.4, 0.3)        # and, or, not: the or-gate runs the lse2 mix of the two scores


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_dualpath_logit_scale_sweep(sigma, dk, io, mode):
    """MultiHop core (two scores mixed through lse, transport A1 A2 v2) at N = 197 against the float64 oracle"""
    from oracle import multihop as om
    from mop_amd import _lib, ops
    prec, path = _mode(mode)
    dt = _io(io)
    B, N, H, hops = 1, 197, 2, 2
    g = torch.Generator(device="cuda").manual_seed(2000 * sigma + dk)
    q1, k1 = logit_qk((B, N, H, dk), (B, N, H, dk), sigma, g)
    q2, k2 = logit_qk((B, N, H, dk), (B, N, H, dk), sigma, g)
    v1, v2 = (torch.randn(B, N, H, dk, device="cuda", generator=g) for _ in range(2))
    base = [bf16_exact(t).to(dt) for t in (q1, k1, v1, q2, k2, v2)]
    dy = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g)).to(dt)
    ts = [t.clone().requires_grad_(True) for t in base]
    lg = torch.tensor(-0.5, device="cuda", requires_grad=True)
    y = ops.dualpath_core(*ts, lg, *GATES, 0.0, 0.6, hops)
    y.backward(dy)
    assert ops.LAST_PATH["dualpath_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    yo, c = om.core_fwd(*(_hp(t) for t in base), dict(and_=GATES[0], or_=GATES[1], not_=GATES[2], chain=0.0), 0.6, hops, -0.5)
    go = om.core_bwd(_hp(dy.view(B, N, H, dk)), c)
    names = ("dq1", "dk1", "dv1", "dq2", "dk2", "dv2")
    got = {n: _hp(t.grad) for n, t in zip(names, ts)}
    _assert_close(_hp(y.view(B, N, H, dk)), yo, got, {n: go[n] for n in names}, f"logit std {logit_std(base[0], base[1]):.2f}")


@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_crossview_folded_logit_scale_sweep(sigma, dk, io):
    """the folded CrossView core (2x2 mix folded into two mixed key tensors + the fused two-score kernels) against the float64
    oracle.  The oracle gets the mixed keys as the kernel reads them (identity mix on k1', k2'); dk1, dk2 are the mix's adjoint of its
    dk1', dk2'."""
    from oracle import crossview as oc
    import mop_amd
    from mop_amd import ops
    mop_amd.set_precision("bf16")
    dt = _io(io)
    B, N, H = 1, 197, 2
    g = torch.Generator(device="cuda").manual_seed(3000 * sigma + dk)
    q1, k1 = logit_qk((B, N, H, dk), (B, N, H, dk), sigma, g)
    q2, k2 = logit_qk((B, N, H, dk), (B, N, H, dk), sigma, g)
    v1 = torch.randn(B, N, H, dk, device="cuda", generator=g)
    base = [bf16_exact(t).to(dt) for t in (q1, k1, v1, q2, k2)]
    mix = torch.tensor([[1.0, 0.5], [-0.25, 0.75]], device="cuda")
    dy = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g)).to(dt)
    ts = [t.clone().requires_grad_(True) for t in base]
    y = ops.crossview_core(*ts, mix)
    y.backward(dy)
    assert ops.LAST_PATH["crossview_fwd"] == mop_amd._lib.PATH_FUSED
    k1p, k2p = (bf16_exact(t) for t in ops._cv_mixed_keys(mix.to(dt), base[1], base[4]))
    yo, c = oc.core_fwd(_hp(base[0]), _hp(k1p), _hp(base[2]), _hp(base[3]), _hp(k2p), np.eye(2))
    go = oc.core_bwd(_hp(dy.view(B, N, H, dk)), c)
    m = mix.to(dt).double().cpu().numpy()
    ref = dict(dq1=go["dq1"], dv1=go["dv1"], dq2=go["dq2"], dk1=m[0, 0] * go["dk1"] + m[1, 0] * go["dk2"],
               dk2=m[0, 1] * go["dk1"] + m[1, 1] * go["dk2"])
    got = dict(dq1=_hp(ts[0].grad), dv1=_hp(ts[2].grad), dq2=_hp(ts[3].grad), dk1=_hp(ts[1].grad), dk2=_hp(ts[4].grad))
    _assert_close(_hp(y.view(B, N, H, dk)), yo, got, ref, f"logit std {logit_std(base[0], k1p):.2f}")


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("use_quartet", [False, True])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_quartet_logit_scale_sweep(sigma, dk, use_quartet, path):
    """Quartet core (z-normalised scores: the scale reaches the result through eps) at T = 197, bf16 io, against the float64 oracle"""
    from oracle import quartet as oq
    import mop_amd
    from mop_amd import _lib, ops
    mop_amd.set_precision("bf16")
    ops.set_path(path)
    B, T, H = 1, 197, 2
    g = torch.Generator(device="cuda").manual_seed(4000 * sigma + dk + use_quartet)
    q, k = logit_qk((B, T, H, dk), (B, T, H, dk), sigma, g)
    q2, k2 = logit_qk((B, T, H, dk), (B, T, H, dk), sigma, g)
    v = torch.randn(B, T, H, dk, device="cuda", generator=g)
    base = [t.to(torch.bfloat16) for t in (q, k, v, q2, k2)]
    dy = torch.randn(B, T, H * dk, device="cuda", generator=g).to(torch.bfloat16)
    ts = [t.clone().requires_grad_(True) for t in base]
    mix, qs = torch.tensor([0.3], device="cuda"), torch.tensor([0.8], device="cuda")
    if use_quartet:
        y = ops.quartet_core(*ts, mix, qs, None, 1e-5, True)
    else:
        y = ops.quartet_core(ts[0], ts[1], ts[2], None, None, None, None, None, 1e-5, False)
    y.backward(dy)
    assert ops.LAST_PATH["quartet_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    yo, c = oq.core_fwd(*(_hp(t) for t in base), 0.3, 0.8, 1e-5, use_quartet, True, None)
    go = oq.core_bwd(_hp(dy.view(B, T, H, dk)), c)
    names = ("dq", "dk", "dv", "dq2", "dk2") if use_quartet else ("dq", "dk", "dv")
    got = {n: _hp(t.grad) for n, t in zip(names, ts)}
    _assert_close(_hp(y.view(B, T, H, dk)), yo, got, {n: go[n] for n in names}, f"logit std {logit_std(base[0], base[1]):.2f}")


@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_decode_attention_logit_scale_sweep(sigma, dk, io):
    """the split-KV decode kernels (plain and row-gathered) at L = 1500 cached keys against float64"""
    from mop_amd import _lib, ops
    dt = _io(io)
    B, Tq, H, cap, L = 2, 4, 2, 1507, 1500
    g = torch.Generator(device="cuda").manual_seed(5000 * sigma + dk)
    q, k = logit_qk((B, Tq, H, dk), (B, cap, H, dk), sigma, g)
    v = torch.randn(B, cap, H, dk, device="cuda", generator=g)
    q, k, v = (t.to(dt) for t in (q, k, v))
    kv_len = torch.tensor([L], dtype=torch.int32, device="cuda")
    std = logit_std(q, k[:, :L])
    for causal in (False, True):
        y = ops.decode_attention(q, k, v, kv_len=kv_len, causal=causal)
        assert ops.LAST_PATH["decode_attn"] == _lib.PATH_FUSED
        yr = torch.stack([sdpa_ref64(q[:, i:i + 1], k[:, :L - (Tq - 1 - i if causal else 0)],
                                     v[:, :L - (Tq - 1 - i if causal else 0)]) for i in range(Tq)], 1).reshape(B, Tq, -1)
        assert _yerr(y.float().cpu().numpy(), yr.cpu().numpy()) <= YTOL, f"logit std {std:.2f} causal {causal}"
        rows = torch.tensor([[1] * cap, [0] * cap], dtype=torch.int32, device="cuda")      # row b reads cache row 1 - b
        yg = ops.decode_attention_rows(q, k, v, rows, kv_len=kv_len, causal=causal)
        kr, vr = k.flip(0), v.flip(0)
        yr = torch.stack([sdpa_ref64(q[:, i:i + 1], kr[:, :L - (Tq - 1 - i if causal else 0)],
                                     vr[:, :L - (Tq - 1 - i if causal else 0)]) for i in range(Tq)], 1).reshape(B, Tq, -1)
        assert _yerr(yg.float().cpu().numpy(), yr.cpu().numpy()) <= YTOL, f"rows, logit std {std:.2f} causal {causal}"


# ---------------------------------------------------------------- fully blocked rows
def _check_blocked(y, got, ref_y, ref, empty, what, dq_names=("dq",)):
    """y (B,N,H*dk) / grads (B,N,H,dk) as numpy; empty: (B,N) bool rows with no open key"""
    assert np.isfinite(y).all() and all(np.isfinite(g).all() for g in got.values()), f"{what}: non-finite"
    assert (y[empty] == 0).all(), f"{what}: blocked rows give y != 0 (max {np.abs(y[empty]).max():.3e})"
    for n in dq_names:
        assert (got[n][empty] == 0).all(), f"{what}: blocked rows give {n} != 0"
    assert _yerr(y, ref_y) <= YTOL, f"{what}: y {_yerr(y, ref_y):.3e}"
    for n, e in _gerrs(got, ref).items():
        assert e <= GTOL, f"{what}: {n} {e:.3e}"


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Nk,causal", [(197, 197, False), (130, 200, False), (200, 1500, False), (197, 197, True)])
def test_sdpa_fully_blocked_rows(N, Nk, causal, io, path):
    from mop_amd import _lib, ops
    _mode("bf16-" + path)
    B, H, dk = 2, 2, 64
    g = torch.Generator(device="cuda").manual_seed(N + Nk + causal)
    q, k, v = (bf16_exact(torch.randn(B, n, H, dk, device="cuda", generator=g)).to(_io(io)) for n in (N, Nk, Nk))
    keep = torch.stack([blocked_rows_mask(N, Nk, g) for _ in range(B)]).unsqueeze(1)      # (B,1,N,Nk)
    w = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g))   # dy as the kernels read it
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    y = ops.sdpa_core(*ts, attn_mask=keep, causal=causal)
    (y.float() * w).sum().backward()
    assert ops.LAST_PATH["sdpa_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    r = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    yr = sdpa_ref64(*r, mask=keep, causal=causal)
    (yr * w.double()).sum().backward()
    eff = keep[:, 0] & (torch.ones(N, Nk, dtype=torch.bool, device="cuda").tril() if causal else True)
    empty = (~eff.any(-1)).cpu().numpy()
    assert empty[:, 0].all() and empty[:, N - 2].all()
    got = {n: t.grad.float().cpu().numpy() for n, t in zip(("dq", "dk", "dv"), ts)}
    ref = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}
    _check_blocked(y.detach().float().cpu().numpy(), got, yr.detach().cpu().numpy(), ref, empty, f"{path} N {N} Nk {Nk}")


@pytest.mark.parametrize("mode", ["bf16-fused", "bf16-generic", "fp32-generic"])
def test_dualpath_fully_blocked_rows(mode):
    from oracle import multihop as om
    from mop_amd import _lib, ops
    prec, path = _mode(mode)
    B, N, H, dk, hops = 2, 197, 2, 64, 2
    g = torch.Generator(device="cuda").manual_seed(77)
    base = [bf16_exact(torch.randn(B, N, H, dk, device="cuda", generator=g)) for _ in range(6)]
    keep = torch.stack([blocked_rows_mask(N, N, g) for _ in range(B)]).unsqueeze(1)
    dy = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g))
    ts = [t.clone().requires_grad_(True) for t in base]
    lg = torch.tensor(-0.5, device="cuda", requires_grad=True)
    y = ops.dualpath_core(*ts, lg, *GATES, 0.0, 0.6, hops, keep)
    y.backward(dy)
    assert ops.LAST_PATH["dualpath_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    blocked = ~keep.cpu().numpy()
    yo, c = om.core_fwd(*(_hp(t) for t in base), dict(and_=GATES[0], or_=GATES[1], not_=GATES[2], chain=0.0), 0.6, hops, -0.5, blocked)
    go = om.core_bwd(_hp(dy.view(B, N, H, dk)), c)
    names = ("dq1", "dk1", "dv1", "dq2", "dk2", "dv2")
    got = {n: t.grad.float().cpu().numpy() for n, t in zip(names, ts)}
    ref = {n: np.transpose(go[n], (0, 2, 1, 3)) for n in names}
    empty = (~keep[:, 0].any(-1)).cpu().numpy()
    assert np.isfinite(float(lg.grad))
    _check_blocked(y.detach().float().cpu().numpy(), got, np.transpose(yo, (0, 2, 1, 3)).reshape(B, N, -1), ref, empty, mode,
                   dq_names=("dq1", "dq2"))


@pytest.mark.parametrize("variant", ["fused", "generic-cues"])
def test_crossview_fully_blocked_rows(variant):
    from oracle import crossview as oc
    import mop_amd
    from mop_amd import _lib, ops
    mop_amd.set_precision("bf16")
    t1, t2 = (0.0, 0.0) if variant == "fused" else (0.3, -0.2)
    B, N, H, dk = 2, 197, 2, 64
    g = torch.Generator(device="cuda").manual_seed(78)
    base = [bf16_exact(torch.randn(B, N, H, dk, device="cuda", generator=g)) for _ in range(5)]
    keep = torch.stack([blocked_rows_mask(N, N, g) for _ in range(B)]).unsqueeze(1)
    mix = torch.tensor([[1.0, 0.5], [-0.25, 0.75]], device="cuda")
    dy = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g))
    ts = [t.clone().requires_grad_(True) for t in base]
    y = ops.crossview_core(*ts, mix, t1=t1, t2=t2, attn_mask=keep)
    y.backward(dy)
    assert ops.LAST_PATH["crossview_fwd"] == (_lib.PATH_FUSED if variant == "fused" else _lib.PATH_GENERIC)
    blocked = ~keep.cpu().numpy()
    if variant == "fused":     # the kernel reads the mixed keys (test_crossview_folded_logit_scale_sweep)
        k1p, k2p = (bf16_exact(t) for t in ops._cv_mixed_keys(mix, base[1], base[4]))
        yo, c = oc.core_fwd(_hp(base[0]), _hp(k1p), _hp(base[2]), _hp(base[3]), _hp(k2p), np.eye(2), blocked=blocked)
        go = oc.core_bwd(_hp(dy.view(B, N, H, dk)), c)
        m = mix.double().cpu().numpy()
        go["dk1"], go["dk2"] = m[0, 0] * go["dk1"] + m[1, 0] * go["dk2"], m[0, 1] * go["dk1"] + m[1, 1] * go["dk2"]
    else:
        yo, c = oc.core_fwd(*(_hp(t) for t in base), mix.double().cpu().numpy(), t1, t2, blocked=blocked)
        go = oc.core_bwd(_hp(dy.view(B, N, H, dk)), c)
    names = ("dq1", "dk1", "dv1", "dq2", "dk2")
    got = {n: t.grad.float().cpu().numpy() for n, t in zip(names, ts)}
    ref = {n: np.transpose(go[n], (0, 2, 1, 3)) for n in names}
    empty = (~keep[:, 0].any(-1)).cpu().numpy()
    # with transpose cues a blocked row's q still reaches other rows' logits (S^T), so only the fused core's dq rows are 0
    _check_blocked(y.detach().float().cpu().numpy(), got, np.transpose(yo, (0, 2, 1, 3)).reshape(B, N, -1), ref, empty, variant,
                   dq_names=("dq1", "dq2") if variant == "fused" else ())


# ---------------------------------------------------------------- additive -inf bias (Whisper cross-attention key padding)
def _key_padding(B, Nk, lengths, dev="cuda"):
    """(B,1,1,Nk) additive bias: 0 on the first lengths[b] keys, -inf after"""
    j = torch.arange(Nk, device=dev)
    bias = torch.zeros(B, 1, 1, Nk, device=dev)
    for b, n in enumerate(lengths):
        bias[b, 0, 0, j >= n] = float("-inf")
    return bias


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("io", ["fp32", "bf16"])
def test_sdpa_minus_inf_key_padding(io, path):
    """key padding at Nk = 1500 with a different length per item (crossing tiles), one item padded at every key (a zero row), and
    +-1e4 finite biases over part of some rows; reference: torch's float64 SDPA"""
    import torch.nn.functional as F
    from mop_amd import _lib, ops
    _mode("bf16-" + path)
    B, N, Nk, H, dk = 4, 130, 1500, 2, 64
    g = torch.Generator(device="cuda").manual_seed(90)
    q, k, v = (bf16_exact(torch.randn(B, n, H, dk, device="cuda", generator=g)).to(_io(io)) for n in (N, Nk, Nk))
    bias = _key_padding(B, Nk, [1500, 1001, 0, 65]).expand(B, 1, N, Nk).clone()
    bias[3, 0, 5, :40] = 1e4                     # a few keys dominate row 5 of item 3
    bias[1, 0, 7, 100:700] = -1e4                # a finite wall in the middle of row 7 of item 1
    w = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g))   # dy as the kernels read it
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    y = ops.sdpa_core(*ts, bias=bias)
    (y.float() * w).sum().backward()
    assert ops.LAST_PATH["sdpa_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    r = [t.detach().double().cpu().requires_grad_(True) for t in (q, k, v)]       # torch's CPU SDPA: zero rows for all -inf
    yr = F.scaled_dot_product_attention(*(t.transpose(1, 2) for t in r), attn_mask=bias.double().cpu()).transpose(1, 2).reshape(B, N, -1)
    (yr * w.double().cpu()).sum().backward()
    empty = np.zeros((B, N), dtype=bool)
    empty[2] = True
    got = {n: t.grad.float().cpu().numpy() for n, t in zip(("dq", "dk", "dv"), ts)}
    ref = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}
    assert (yr.detach()[2] == 0).all()
    _check_blocked(y.detach().float().cpu().numpy(), got, yr.detach().cpu().numpy(), ref, empty, path)


def test_sdpa_finfo_min_bias_row_is_finite():
    """a row biased entirely by finfo(float32).min: torch averages it uniformly; the kernels' bias . log2(e) overflows to -inf there
    and the row is 0 (documented in INTEGRATION.md) -- finite either way"""
    from mop_amd import ops
    for path in ("fused", "generic"):
        _mode("bf16-" + path)
        q, k, v = (torch.randn(1, 70, 2, 64, device="cuda") for _ in range(3))
        bias = torch.zeros(1, 1, 70, 70, device="cuda")
        bias[0, 0, 3] = torch.finfo(torch.float32).min
        y = ops.sdpa_core(q, k, v, bias=bias)
        assert torch.isfinite(y).all(), path


@pytest.mark.parametrize("path", ["fused", "generic"])
def test_whisper_cross_attention_key_padding(path):
    """MultiheadCrossAttention with an additive -inf key-padding attn_mask against the same module computed in float64"""
    import torch.nn.functional as F
    from mop_amd.nn.whisper_mop import MultiheadCrossAttention
    _mode("fp32-generic" if path == "generic" else "bf16-fused")
    torch.manual_seed(3)
    B, Tq, Tk, D, H = 3, 37, 1500, 128, 2
    m = MultiheadCrossAttention(D, D, H, 0.0, True).cuda().eval()
    xq = torch.randn(B, Tq, D, device="cuda")
    xkv = torch.randn(B, Tk, D, device="cuda")
    mask = _key_padding(B, Tk, [1500, 700, 0])
    with torch.no_grad():
        y = m(xq, xkv, attn_mask=mask)
        lin = lambda p, x: F.linear(x.double().cpu(), p.weight.double().cpu(), p.bias.double().cpu())
        q, k, v = (lin(p, x).view(B, -1, H, D // H).transpose(1, 2) for p, x in ((m.q_proj, xq), (m.k_proj, xkv), (m.v_proj, xkv)))
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask.double().cpu()).transpose(1, 2).reshape(B, Tq, D)
        ref = lin(m.o_proj, a)
    assert torch.isfinite(y).all()
    assert torch.equal(a[2], torch.zeros_like(a[2]))
    tol = 1e-4 if path == "generic" else YTOL
    assert float((y.double().cpu() - ref).abs().max()) <= tol * float(ref.abs().max()), path


# ---------------------------------------------------------------- a bias that requires grad
def test_bias_that_requires_grad_is_refused():
    from mop_amd import ops
    from mop_amd.nn.whisper_mop import MultiheadCrossAttention, MultiheadSelfAttention
    B, N, H, dk = 1, 20, 2, 32
    q, k, v = (torch.randn(B, N, H, dk, device="cuda", requires_grad=True) for _ in range(3))
    bias = torch.randn(B, 1, N, N, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="bias"):
        ops.sdpa_core(q, k, v, bias=bias)
    with pytest.raises(NotImplementedError, match="add_mask"):
        ops.quartet_core(q, k, v, None, None, None, None, bias, 1e-5, False)
    sa = MultiheadSelfAttention(64, 2, 0.0, True, causal=False).cuda()
    ca = MultiheadCrossAttention(64, 64, 2, 0.0, True).cuda()
    x = torch.randn(B, N, 64, device="cuda")
    with pytest.raises(NotImplementedError):
        sa(x, attn_bias=bias)
    with pytest.raises(NotImplementedError):
        ca(x, x, attn_mask=bias)
    # as before under no_grad, and with a plain tensor (its gradient is not asked for)
    plain = bias.detach()
    ref = sdpa_ref64(q, k, v, bias=plain)
    for b_, ctx in ((bias, torch.no_grad()), (plain, torch.enable_grad())):
        with ctx:
            y = ops.sdpa_core(q, k, v, bias=b_)
            assert float((y.double() - ref).abs().max()) <= 1e-2 * float(ref.abs().max())
            ops.quartet_core(q, k, v, None, None, None, None, b_, 1e-5, False)
            sa(x, attn_bias=b_)
            ca(x, x, attn_mask=b_)
    y = ops.sdpa_core(q, k, v, bias=plain)
    y.sum().backward()
    assert q.grad is not None and bias.grad is None
