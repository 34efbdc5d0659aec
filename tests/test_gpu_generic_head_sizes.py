"""-m gpu: the generic multi-kernel paths (bgemm.h, attn_generic.hip, edgewise_generic.hip) at head sizes the fused kernels do not
take -- dk in {6, 12, 40, 80, 100, 128} -- against float64 on the operands the kernels read: forward and every gradient.

What each head size reaches (K = dk in the q k^T products, N = dk in the map x vector ones):
  6    rows of 24 / 12 bytes: the scalar loads of BgStage::load (no operand keeps 16-byte alignment), unaligned bf16 io rows
  12   16-byte loads, and the second 8-float chunk of a row crosses the K edge (scalar tail); 24-byte bf16 io rows
  40   a partial second K tile
  80   a partial third K tile; output tiles 64 + 16 wide (an n-edge inside dk); two d-chunks in scale_bwd_kernel, the second partial
  100  a partial fourth K tile; dk > 96: with N = 130 the N x dk outputs (P v, dS k, dS^T q, P^T dy) take the 128 x 128 tile with an
       n-edge at 100 and a partial second row of tiles; scale_bwd_kernel's second d-chunk has 36 live lanes
  128  exact K tiles and an exact 128-wide output tile; two full d-chunks
N = 50 is one partial 64-tile; N = 130 (> 96, > 128) puts the N x N products on the 128 x 128 tile with a partial second tile;
(N, Nk) = (130, 70) and (50, 150) are the rectangular cases.  B = H = 2 everywhere, so batch and head strides count.

The split: the plain call of each core runs the whole DKS x N x arithmetic x io sweep; the option variants (mask + bias, lengths,
dropout, hops = 3, explicit mask, transpose cues + prior, additive mask, the dense / 3x3 / lens-bank Edgewise heads) run at
dk in {12, 100} and N = 130.  One test per core also runs every dk under set_path("auto") and asserts the generic route was taken.

Bounds (none of them new): bf16 arithmetic or bf16 io -> YTOL / GTOL / GFLOOR of test_gpu_attn_edges.py through its _assert_close;
fp32 arithmetic with fp32 io -> max-abs(y) <= 1e-4 and max-abs(grad) / max|ref| <= 1e-3, as test_edgewise_vs_oracle_seeded asserts for
this path.  The longest fp32 FMA chain here has 150 terms (about 9e-6 of the sum of magnitudes at worst); a dropped or misplaced K
chunk of N(0, 1) operands moves a result by O(1 / sqrt(dk)) >= 0.09.  Each test prints its figures before it asserts.

Inputs: N(0, 1) draws from a seeded generator.  Two cores carry gradients that a random draw can leave ill-conditioned whatever the
head size.  MultiHop's d chain_logit and EdgewiseMSA's d chain_value_logit are sums of B N H dk signed terms: under a random
upstream gradient they cancel to 1e-4 of their magnitudes, so these two cores get the gradient of <r, y> + |y|^2 / (2 rms(y))
(_upstream), whose quadratic part gives the sum a definite term.  And the Edgewise gate-head gradients fall to 1e-7 of the module's
scale when a draw's mixed softmax saturates (a plain float32 evaluation of the float64 oracle is then 3.5e-2 off by itself).  No
bound can be asked of such a tensor, so for these two cores a draw is kept only if the REFERENCE resolves every gradient on it
(_well_conditioned: the oracle's own error under the rounding of the arithmetic, a factor 2 below the bound; the kernels' results
take no part), else the next seed is drawn."""
import copy
import functools

import numpy as np
import pytest
import torch

from attn_ref import bf16_exact, blocked_rows_mask, sdpa_ref64
from gpu_util import max_abs, rel_err
from test_gpu_attn_edges import GFLOOR, GTOL, YTOL, _assert_close, _gerrs, _yerr

pytestmark = pytest.mark.gpu
DKS = [6, 12, 40, 80, 100, 128]
OPT_DKS = [12, 100]                       # the option variants: a K-edge chunk, and the big tile with an n-edge
NS = [50, 130]
MODES = ["bf16-generic", "fp32-generic"]
IOS = ["fp32", "bf16"]
B, H = 2, 2
GATES = (0.8, 0.4, 0.3)                   # and, or, not
FP32_YTOL, FP32_GTOL = 1e-4, 1e-3         # test_edgewise_vs_oracle_seeded


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


def _dt(io):
    return torch.float32 if io == "fp32" else torch.bfloat16


def _exact(mode, io):
    """fp32 arithmetic on fp32 tensors: nothing on the way is rounded to bf16"""
    return mode == "fp32-generic" and io == "fp32"


def _rand(shape, g, mode, io):
    """N(0, 1) as the kernel reads it: bf16-exact values unless both the arithmetic and the tensors are fp32"""
    t = torch.randn(*shape, device="cuda", generator=g)
    return t if _exact(mode, io) else bf16_exact(t).to(_dt(io))


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _np(t):
    return t.detach().double().cpu().numpy()


def _hp(t):
    """(B,N,H,dk) torch -> (B,H,N,dk) float64 numpy (the oracle layout)"""
    return np.transpose(_np(t), (0, 2, 1, 3))


def _check(y, yr, got, ref, mode, io, what):
    """y and every gradient in `ref` against float64, under the bound of the arithmetic / io pair; prints the figures first"""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    y, yr = np.asarray(y, np.float64), np.asarray(yr, np.float64).reshape(np.shape(y))
    got = {n: np.asarray(got[n], np.float64).reshape(np.shape(ref[n])) for n in ref}
    if _exact(mode, io):
        ey, ge = max_abs(y, yr), {n: rel_err(got[n], ref[n]) for n in ref}
    else:
        ey, ge = _yerr(y, yr), _gerrs(got, ref)
    worst = max(ge, key=ge.get)
    print(f"\nFIG {what} {mode} io {io}: y {ey:.3e} grad {ge[worst]:.3e} ({worst})")
    if _exact(mode, io):
        assert np.isfinite(y).all() and all(np.isfinite(g).all() for g in got.values()), what
        assert ey <= FP32_YTOL, f"{what}: y {ey:.3e}"
        for n, e in ge.items():
            assert e <= FP32_GTOL, f"{what}: {n} {e:.3e}"
    else:
        _assert_close(y, yr, got, ref, what)


NOISE_FACTOR, MAX_DRAWS = 2.0, 32       # two samples of one rounding noise differ (test_gpu_edgewise.NOISE_FACTOR's default)


def _well_conditioned(ref_fn, operands, ref, exact):
    """does the reference itself resolve every gradient of this draw?  ref_fn(operands) -> {name: gradient} is evaluated once more
    under the rounding the arithmetic applies -- exact: wholly in float32; else: every operand moved by a relative 2^-9 x U(-1, 1),
    one bfloat16 rounding -- and has to stay NOISE_FACTOR below the bound the test asserts, in the metric the test asserts"""
    if exact:
        noisy = ref_fn([np.asarray(a, np.float32) for a in operands])
        errs, lim = {n: rel_err(np.asarray(noisy[n], np.float64), ref[n]) for n in ref}, FP32_GTOL
    else:
        rng = np.random.default_rng(2024)
        noisy = ref_fn([a * (1.0 + 2.0 ** -9 * rng.uniform(-1.0, 1.0, np.shape(a))) for a in operands])
        errs, lim = _gerrs(noisy, ref), GTOL
    return all(NOISE_FACTOR * e <= lim for e in errs.values())


def _upstream(r, y_ref, exact):
    """the gradient of the loss <r, y> + |y|^2 / (2 rms(y)) at the reference's y: r + y_ref / rms(y_ref), in r's shape and as the
    kernels read it.  Under <r, y> alone, d chain_logit = w (1 - w) sum(dy * y_chain) is a sum of signed terms with nothing to
    keep it from cancelling; the quadratic part adds w |y_chain|^2 to it"""
    y_ref = np.asarray(y_ref, np.float64)
    dy = r + torch.from_numpy(y_ref / np.sqrt((y_ref ** 2).mean())).to(r.device, r.dtype).reshape(r.shape)
    return dy if exact else bf16_exact(dy)


def _generic(*keys):
    from mop_amd import _lib, ops
    for k in keys:
        assert ops.LAST_PATH[k] == _lib.PATH_GENERIC, k


# ---------------------------------------------------------------- plain SDPA
def _sdpa_grads(ts, packed):
    if packed:
        return {n: ts[0].grad[:, :, i].float().cpu().numpy() for i, n in enumerate(("dq", "dk", "dv"))}
    return {n: t.grad.float().cpu().numpy() for n, t in zip(("dq", "dk", "dv"), ts)}


def _sdpa_case(N, Nk, dk, mode, io, g, packed=False, ref_mask=None, **kw):
    """one ops.sdpa_core forward + backward against sdpa_ref64; kw goes to the core, ref_mask (with kw's bias / causal) to the reference"""
    from mop_amd import ops
    q, k, v = (_rand((B, n, H, dk), g, mode, io) for n in (N, Nk, Nk))
    w = _rand((B, N, H * dk), g, mode, io)
    if packed:
        ts = [torch.stack([q, k, v], 2).requires_grad_(True)]
        y = ops.sdpa_core(ts[0], **kw)
    else:
        ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
        y = ops.sdpa_core(*ts, **kw)
    y.backward(w)
    _generic("sdpa_fwd", "sdpa_bwd")
    r = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
    yr = sdpa_ref64(*r, mask=ref_mask, bias=kw.get("bias"), causal=kw.get("causal", False))
    (yr * w.double()).sum().backward()
    ref = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}
    return y.detach().float().cpu().numpy(), yr.detach().cpu().numpy(), _sdpa_grads(ts, packed), ref


SDPA_SHAPES = [(50, 50, "square"), (130, 130, "square"), (130, 70, "rect"), (50, 150, "rect"), (130, 130, "causal"), (130, 130, "packed")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", DKS)
@pytest.mark.parametrize("N,Nk,kind", SDPA_SHAPES)
def test_sdpa_head_sizes(N, Nk, kind, dk, io, mode):
    _mode(mode)
    out = _sdpa_case(N, Nk, dk, mode, io, _gen(1, N, Nk, dk), packed=kind == "packed", causal=kind == "causal")
    _check(*out, mode, io, f"sdpa {kind} N {N} Nk {Nk} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", OPT_DKS)
@pytest.mark.parametrize("N,Nk", [(130, 130), (130, 70)])
def test_sdpa_mask_and_bias_head_sizes(N, Nk, dk, io, mode):
    """an explicit mask with fully blocked rows (blocked_rows_mask) plus an additive bias: y = 0 and dq = 0 on the blocked rows"""
    _mode(mode)
    g = _gen(2, N, Nk, dk)
    keep = torch.stack([blocked_rows_mask(N, Nk, g) for _ in range(B)]).unsqueeze(1)          # (B,1,N,Nk)
    bias = torch.randn(B, 1, N, Nk, device="cuda", generator=g)
    y, yr, got, ref = _sdpa_case(N, Nk, dk, mode, io, g, attn_mask=keep, bias=bias, ref_mask=keep)
    empty = (~keep[:, 0].any(-1)).cpu().numpy()
    assert empty[:, 0].all() and empty[:, N - 2].all()
    assert (y[empty] == 0).all() and (got["dq"][empty] == 0).all()
    _check(y, yr, got, ref, mode, io, f"sdpa mask+bias N {N} Nk {Nk} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", OPT_DKS)
@pytest.mark.parametrize("N,Nk", [(130, 130), (130, 70)])
def test_sdpa_lens_head_sizes(N, Nk, dk, io, mode):
    """q_lens / kv_lens over a right-padded batch whose padding rows hold NaN (q, k, v and the incoming gradient): the result is the
    reference on the rows inside the lengths, 0 on the padding rows, and finite everywhere"""
    from mop_amd import ops
    _mode(mode)
    g = _gen(3, N, Nk, dk)
    q, k, v = (_rand((B, n, H, dk), g, mode, io) for n in (N, Nk, Nk))
    w = _rand((B, N, H * dk), g, mode, io)
    ql = torch.tensor([N, 67], dtype=torch.int32, device="cuda")          # one full row; one ending inside the second 64-tile
    kl = torch.tensor([Nk - 5, 33], dtype=torch.int32, device="cuda")
    qpad = (torch.arange(N, device="cuda")[None] >= ql[:, None])            # (B,N)
    kpad = (torch.arange(Nk, device="cuda")[None] >= kl[:, None])
    nan = float("nan")
    ts = [t.masked_fill(p[:, :, None, None], nan).requires_grad_(True) for t, p in ((q, qpad), (k, kpad), (v, kpad))]
    y = ops.sdpa_core(*ts, q_lens=ql, kv_lens=kl)
    y.backward(w.masked_fill(qpad[:, :, None], nan))
    _generic("sdpa_fwd", "sdpa_bwd")
    r = [t.masked_fill(p[:, :, None, None], 0.0).double().requires_grad_(True) for t, p in ((q, qpad), (k, kpad), (v, kpad))]
    yr = sdpa_ref64(*r, mask=ops.sdpa_lens_mask(ql, kl, B, N, Nk, "cuda"))
    (yr * w.double()).sum().backward()
    got = {n: t.grad.float().cpu().numpy() for n, t in zip(("dq", "dk", "dv"), ts)}
    ref = {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}
    yn = y.detach().float().cpu().numpy()
    qp, kp = qpad.cpu().numpy(), kpad.cpu().numpy()
    assert (yn[qp] == 0).all() and (got["dq"][qp] == 0).all() and (got["dk"][kp] == 0).all() and (got["dv"][kp] == 0).all()
    _check(yn, yr.detach().cpu().numpy(), got, ref, mode, io, f"sdpa lens N {N} Nk {Nk} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", OPT_DKS)
@pytest.mark.parametrize("N,Nk", [(130, 130), (130, 70)])
def test_sdpa_dropout_head_sizes(N, Nk, dk, io, mode):
    """dropout_p = 0.25 with a fixed seed against the float64 oracle under ops.dropout_keep_mask"""
    from mop_amd import ops
    from oracle import sdpa as osd
    _mode(mode)
    p, seed = 0.25, 0x5EED0000 + 131 * N + dk
    g = _gen(4, N, Nk, dk)
    q, k, v = (_rand((B, n, H, dk), g, mode, io) for n in (N, Nk, Nk))
    w = _rand((B, N, H * dk), g, mode, io)
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    y = ops.sdpa_core(*ts, dropout_p=p, seed=seed)
    y.backward(w)
    _generic("sdpa_fwd", "sdpa_bwd")
    drop = ops.dropout_keep_mask(seed, p, B, H, N, Nk).numpy().astype(np.float64) / (1.0 - p)
    yo, c = osd.core_fwd(_hp(q), _hp(k), _hp(v), None, None, drop)
    go = osd.core_bwd(_hp(w.view(B, N, H, dk)), c)
    got = {n: _hp(t.grad) for n, t in zip(("dq", "dk", "dv"), ts)}
    _check(_hp(y.view(B, N, H, dk)), yo, got, {n: go[n] for n in got}, mode, io, f"sdpa dropout N {N} Nk {Nk} dk {dk}")


# ---------------------------------------------------------------- MultiHop (dual path)
DP_NAMES = ("dq1", "dk1", "dv1", "dq2", "dk2", "dv2")


@functools.lru_cache(maxsize=None)
def _dualpath_draw(N, dk, hops, mask_kind, exact, key):
    """the first well-conditioned draw of (six operands, dy, keep mask) with its float64 result, shared by the arithmetic / io pairs"""
    from oracle import multihop as om
    gates = dict(and_=GATES[0], or_=GATES[1], not_=GATES[2], chain=0.0)
    for draw in range(MAX_DRAWS):
        g = _gen(key, N, dk, hops, len(mask_kind), draw)
        base = [torch.randn(B, N, H, dk, device="cuda", generator=g) for _ in range(6)]
        dy = torch.randn(B, N, H * dk, device="cuda", generator=g)
        if not exact:
            base = [bf16_exact(t) for t in base]
        keep = torch.stack([blocked_rows_mask(N, N, g) for _ in range(B)]).unsqueeze(1) if mask_kind == "mask" else None
        blocked = None
        if mask_kind == "mask":
            blocked = ~keep.cpu().numpy()
        elif mask_kind == "causal":
            blocked = ~np.tril(np.ones((N, N), dtype=bool))[None, None]
        dy = _upstream(dy, om.core_fwd(*(_hp(t) for t in base), gates, 0.6, hops, -0.5, blocked)[0].transpose(0, 2, 1, 3), exact)

        def ref_fn(a, out=None):
            yo, c = om.core_fwd(*a[:6], gates, 0.6, hops, -0.5, blocked)
            go = om.core_bwd(a[6], c)
            if out is not None:
                out.append(yo)
            return {**{n: go[n] for n in DP_NAMES}, "dlogit": np.asarray(go["dlogit"])}
        operands, yo = [_hp(t) for t in base] + [_hp(dy.view(B, N, H, dk))], []
        ref = ref_fn(operands, yo)
        if _well_conditioned(ref_fn, operands, ref, exact):
            return base, dy, keep, yo[0], ref
    raise AssertionError(f"no well-conditioned draw in {MAX_DRAWS} (N {N} dk {dk} hops {hops} {mask_kind})")


def _dualpath_case(N, dk, mode, io, key, hops, mask_kind):
    from mop_amd import ops
    base, dy, keep, yo, ref = _dualpath_draw(N, dk, hops, mask_kind, _exact(mode, io), key)
    ts = [t.clone().to(_dt(io)).requires_grad_(True) for t in base]           # the draw is shared: never a view of it
    lg = torch.tensor(-0.5, device="cuda", requires_grad=True)
    y = ops.dualpath_core(*ts, lg, *GATES, 0.0, 0.6, hops, keep, causal=mask_kind == "causal")
    y.backward(dy.to(_dt(io)))
    _generic("dualpath_fwd", "dualpath_bwd")
    got = {n: _hp(t.grad) for n, t in zip(DP_NAMES, ts)}
    got["dlogit"] = _np(lg.grad)
    yn = _hp(y.view(B, N, H, dk))
    if mask_kind == "mask":
        empty = (~keep[:, 0].any(-1)).cpu().numpy()[:, None].repeat(H, 1)             # (B,H,N)
        assert (yn[empty] == 0).all() and (got["dq1"][empty] == 0).all() and (got["dq2"][empty] == 0).all()
    return yn, yo, got, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", DKS)
@pytest.mark.parametrize("N", NS)
def test_dualpath_head_sizes(N, dk, io, mode):
    _mode(mode)
    _check(*_dualpath_case(N, dk, mode, io, 5, 2, "none"), mode, io, f"dualpath N {N} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", OPT_DKS)
@pytest.mark.parametrize("hops,mask_kind", [(3, "none"), (2, "causal"), (3, "causal"), (2, "mask"), (3, "mask")])
def test_dualpath_options_head_sizes(hops, mask_kind, dk, io, mode):
    _mode(mode)
    _check(*_dualpath_case(130, dk, mode, io, 6, hops, mask_kind), mode, io,
           f"dualpath hops {hops} {mask_kind} dk {dk}")


# ---------------------------------------------------------------- Quartet
def _quartet_case(T, dk, mode, io, g, use_quartet, with_mask):
    from oracle import quartet as oq
    from mop_amd import ops
    base = [_rand((B, T, H, dk), g, mode, io) for _ in range(5)]
    dy = _rand((B, T, H * dk), g, mode, io)
    am = 2.0 * torch.randn(B, 1, T, T, device="cuda", generator=g) if with_mask else None
    ts = [t.clone().requires_grad_(True) for t in base]
    mix = torch.tensor([0.3], device="cuda", requires_grad=True)
    qs = torch.tensor([0.8], device="cuda", requires_grad=True)
    if use_quartet:
        y = ops.quartet_core(*ts, mix, qs, am, 1e-5, True)
    else:
        y = ops.quartet_core(ts[0], ts[1], ts[2], None, None, None, None, am, 1e-5, False)
    y.backward(dy)
    _generic("quartet_fwd")            # the backward runs the path the forward resolved (ctx.meta): there is no record of its own
    yo, c = oq.core_fwd(*(_hp(t) for t in base), 0.3, 0.8, 1e-5, use_quartet, True, None if am is None else _np(am))
    go = oq.core_bwd(_hp(dy.view(B, T, H, dk)), c)
    names = ("dq", "dk", "dv", "dq2", "dk2") if use_quartet else ("dq", "dk", "dv")
    got = {n: _hp(t.grad) for n, t in zip(names, ts)}
    ref = {n: go[n] for n in names}
    if use_quartet:
        got.update(dmixture=_np(mix.grad), dquartet_scale=_np(qs.grad))
        ref.update(dmixture=np.asarray([go["dmixture"]]), dquartet_scale=np.asarray([go["dquartet_scale"]]))
    return _hp(y.view(B, T, H, dk)), yo, got, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("use_quartet", [True, False])
@pytest.mark.parametrize("dk", DKS)
@pytest.mark.parametrize("T", NS)
def test_quartet_head_sizes(T, dk, use_quartet, io, mode):
    _mode(mode)
    _check(*_quartet_case(T, dk, mode, io, _gen(7, T, dk, use_quartet), use_quartet, False), mode, io,
           f"quartet use_quartet {use_quartet} T {T} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("use_quartet", [True, False])
@pytest.mark.parametrize("dk", OPT_DKS)
def test_quartet_additive_mask_head_sizes(dk, use_quartet, io, mode):
    _mode(mode)
    _check(*_quartet_case(130, dk, mode, io, _gen(8, dk, use_quartet), use_quartet, True), mode, io,
           f"quartet use_quartet {use_quartet} add_mask dk {dk}")


# ---------------------------------------------------------------- CrossView
CV_MIX = [[1.0, 0.5], [-0.25, 0.75]]


def _crossview_case(N, dk, mode, io, g, cues, causal):
    """cues: transpose cues and the per-key prior on (anchor rows by argmax_row_sum: the oracle is evaluated at the rows the device
    picked, as test_crossview_mixer does -- the argmax over row sums of a row-stochastic map is decided by rounding)"""
    from oracle import crossview as oc
    from mop_amd import ops
    base = [_rand((B, N, H, dk), g, mode, io) for _ in range(5)]
    dy = _rand((B, N, H * dk), g, mode, io)
    ts = [t.clone().requires_grad_(True) for t in base]
    mix = torch.tensor(CV_MIX, device="cuda", requires_grad=True)
    kw = dict(t1=0.3, t2=-0.2, prior_weight=0.4, anchor_mode="argmax_row_sum") if cues else {}
    y = ops.crossview_core(*ts, mix, causal=causal, **kw)
    y.backward(dy)
    _generic("crossview_fwd")          # _CrossViewFn is the generic route in both directions: there is no backward record
    blocked = ~np.tril(np.ones((N, N), dtype=bool))[None, None] if causal else None
    okw = {}
    if cues:
        okw = dict(t1=0.3, t2=-0.2, prior_weight=0.4, k_star=ops.LAST_PATH["crossview_k_star"].cpu().numpy().astype(np.int64))
    yo, c = oc.core_fwd(*(_hp(t) for t in base), np.asarray(CV_MIX), blocked=blocked, **okw)
    go = oc.core_bwd(_hp(dy.view(B, N, H, dk)), c)
    names = ("dq1", "dk1", "dv1", "dq2", "dk2")
    got = {n: _hp(t.grad) for n, t in zip(names, ts)}
    got["dmix"] = _np(mix.grad)
    ref = {n: go[n] for n in names}
    ref["dmix"] = go["dmix"]
    return _hp(y.view(B, N, H, dk)), yo, got, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", DKS)
@pytest.mark.parametrize("N", NS)
def test_crossview_head_sizes(N, dk, io, mode):
    _mode(mode)
    _check(*_crossview_case(N, dk, mode, io, _gen(9, N, dk), False, False), mode, io, f"crossview N {N} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", OPT_DKS)
@pytest.mark.parametrize("cues,causal", [(False, True), (True, False), (True, True)])
def test_crossview_options_head_sizes(cues, causal, dk, io, mode):
    _mode(mode)
    _check(*_crossview_case(130, dk, mode, io, _gen(10, cues, causal, dk), cues, causal), mode, io,
           f"crossview cues+prior {cues} causal {causal} dk {dk}")


# ---------------------------------------------------------------- EdgewiseMSA
EW_V, EW_R = 3, 2
SCALE_GRADS = ("q_scale", "k_scale", "v_scale")        # reduced over the tokens by scale_bwd_kernel, one d-chunk of 64 per block


def _edgewise_model(N, dk, variant, exact, draw):
    """a seeded EdgewiseMSA(dim = H dk, V = 3, r = 2) as test_edgewise_vs_oracle_seeded builds it, x, and the random part r of the
    upstream gradient (_upstream); bf16-exact parameters and x unless arithmetic and tensors are fp32"""
    from mop_amd.nn import EdgewiseMSA
    D = H * dk
    kw, dil = dict(n_views=EW_V, share_qkv=True), None
    if variant == "lowrank":
        kw.update(gate_mode="lowrank", gate_rank=EW_R, gate_init="mix5")
    elif variant == "lowrank_lens":
        dil = (1, 2)
        kw.update(gate_mode="lowrank", gate_rank=EW_R, gate_init="mix5", use_lens_bank=True, lens_dilations=dil)
    else:
        kw.update(gate_mode="dense", use_k3=variant == "dense_k3", gate_init="and")
    torch.manual_seed(1000 * N + dk + len(variant) + 7919 * draw)
    m = EdgewiseMSA(D, H, **kw)
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("_scale"):
                p.add_(0.1 * torch.randn_like(p))
            elif "proj.weight" in n_ and "edge_head" in n_:
                p.mul_(3.0)
            elif n_.endswith("conv2.bias"):
                p.copy_(0.5 * torch.randn_like(p))          # the -5 preset leaves every gate (and its gradient) ~0
        m.chain_value_logit.fill_(-0.5)
        x, w = torch.randn(B, N, D), torch.randn(B, N, D)
        if not exact:
            for p in m.parameters():
                p.copy_(bf16_exact(p))
            x = bf16_exact(x)
    return m, x, w, dil


@functools.lru_cache(maxsize=None)
def _edgewise_draw(N, dk, variant, exact):
    """the first well-conditioned draw of (module, x, w) with oracle.edgewise's float64 output and gradients (dx under 'dx'), shared
    by the arithmetic / io pairs"""
    from oracle import edgewise as oe
    for draw in range(MAX_DRAWS):
        m, x, w, dil = _edgewise_model(N, dk, variant, exact, draw)
        names = list(m.state_dict())

        def ref_fn(a, out=None):
            yo, cache = oe.module_fwd(a[0], dict(zip(names, a[2:])), H, EW_V, True, 0.5, lens_dilations=dil)
            dx, go = oe.module_bwd(a[1], cache)
            if out is not None:
                out.append(yo)
            return {**go, "dx": dx}
        pvals = [v.detach().double().numpy() for v in m.state_dict().values()]
        w = _upstream(w, oe.module_fwd(x.double().numpy(), dict(zip(names, pvals)), H, EW_V, True, 0.5, lens_dilations=dil)[0], exact)
        operands, yo = [x.double().numpy(), w.double().numpy()] + pvals, []
        ref = ref_fn(operands, yo)
        if _well_conditioned(ref_fn, operands, ref, exact):
            return m, x, w, yo[0], ref
    raise AssertionError(f"no well-conditioned draw in {MAX_DRAWS} (N {N} dk {dk} {variant})")


def _edgewise_case(N, dk, mode, io, variant):
    """EdgewiseMSA forward + backward against oracle.edgewise.module_fwd / module_bwd on the parameters and inputs the module holds"""
    m, x, w, out, g_ref = _edgewise_draw(N, dk, variant, _exact(mode, io))
    m = copy.deepcopy(m).cuda().to(_dt(io)).eval()
    xt = x.cuda().to(_dt(io)).requires_grad_(True)
    y = m(xt)
    y.backward(w.cuda().to(_dt(io)))
    _generic("edgewise_fwd", "edgewise_bwd")
    got = {k: p.grad.float().cpu().numpy() for k, p in m.named_parameters()}
    got["dx"] = xt.grad.float().cpu().numpy()
    assert set(got) == set(g_ref) and set(SCALE_GRADS) <= set(g_ref)
    return y.detach().float().cpu().numpy(), out, got, g_ref


def _check_edgewise(y, yr, got, ref, mode, io, what):
    ge = _gerrs({n: got[n].reshape(ref[n].shape) for n in ref}, ref) if not _exact(mode, io) else \
        {n: rel_err(got[n].reshape(ref[n].shape), ref[n]) for n in ref}
    print(f"\nFIG {what} {mode} io {io}: " + " ".join(f"{n} {ge[n]:.3e}" for n in SCALE_GRADS))
    _check(y, yr, got, ref, mode, io, what)
    lim = FP32_GTOL if _exact(mode, io) else GTOL
    for n in SCALE_GRADS:                 # by name: what scale_bwd_kernel reduces
        assert ge[n] <= lim, f"{what}: {n} {ge[n]:.3e}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", DKS)
@pytest.mark.parametrize("N", NS)
def test_edgewise_head_sizes(N, dk, io, mode):
    _mode(mode)
    _check_edgewise(*_edgewise_case(N, dk, mode, io, "lowrank"), mode, io, f"edgewise lowrank N {N} dk {dk}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", IOS)
@pytest.mark.parametrize("dk", OPT_DKS)
@pytest.mark.parametrize("variant", ["dense", "dense_k3", "lowrank_lens"])
def test_edgewise_variants_head_sizes(variant, dk, io, mode):
    _mode(mode)
    _check_edgewise(*_edgewise_case(130, dk, mode, io, variant), mode, io, f"edgewise {variant} dk {dk}")


# ---------------------------------------------------------------- routing under set_path("auto")
@pytest.mark.parametrize("dk", DKS)
def test_auto_path_takes_the_generic_route_at_these_head_sizes(dk):
    """bf16 tensors under the default settings (bf16 arithmetic, path auto: the fused kernels are candidates): every core lands on the
    generic route in both directions -- asserted inside each case -- and is still right there"""
    mode, io, N = "auto-auto", "bf16", 50
    _mode(mode)
    _check(*_sdpa_case(N, N, dk, mode, io, _gen(11, dk)), mode, io, f"auto sdpa dk {dk}")
    _check(*_dualpath_case(N, dk, mode, io, 12, 2, "none"), mode, io, f"auto dualpath dk {dk}")
    _check(*_quartet_case(N, dk, mode, io, _gen(13, dk), True, False), mode, io, f"auto quartet dk {dk}")
    _check(*_crossview_case(N, dk, mode, io, _gen(14, dk), False, False), mode, io, f"auto crossview dk {dk}")
    _check_edgewise(*_edgewise_case(N, dk, mode, io, "lowrank"), mode, io, f"auto edgewise dk {dk}")
