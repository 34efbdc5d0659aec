"""The Edgewise cores at peaked logits, token row by token row against the float64 oracle.

Inputs, oracle mapping, rounding model and bounds are tests/edgewise_peaks.py; tests/test_edgewise_peaks_cpu.py shows on the oracle alone
that they are fair.  The per-view logit standard deviation runs through 0.5, 2, 4 and 8 (the rest of the suite stays near 0.3): the
online maxima move, the gates saturate, the chain products underflow, |Smix| reaches several hundred.  Five ways through the kernels:
  1 fused training forward + backward on the exported record        4 generic path, bf16 arithmetic
  2 the same with set_save_chain_state(False): the backward recomputes   5 generic path, fp32 arithmetic
  3 fused inference forward (no_grad)
float32 and bfloat16 I/O for 1 and 3, float32 for the rest.  Every case asserts the path it ran.

bf16 arithmetic: every token row of y / dq / dk / dv within max(tol max|ref|, 4 x the row's own movement under the q sqk_v rounding),
tol = 1e-2 for y and 3e-2 for gradients as everywhere in the suite; small-parameter gradients through check_grads with the noise
record of all the documented rounding sites (edgewise_peaks.small_noise: dbc at N = 33, level 0.5 needs them, nothing else does).
fp32 arithmetic (mode 5): 1e-3 relative on every tensor, no allowance.  Planted rows (each attends to itself alone, in the first key,
at a tile edge, in the last partial tile): the plain tolerance, no allowance.  DESIGN.md 4.2b has the measured ratios."""
import numpy as np
import pytest
import torch

import edgewise_peaks as ep
from edgewise_peaks import GTOL_BF16, GTOL_FP32, LEVELS, ROW_TENSORS, SHAPES, TOL_BF16
from gpu_util import check_grads, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# (mode, I/O dtype)
RUNS = ((1, F32), (1, BF16), (2, F32), (3, F32), (3, BF16), (4, F32), (5, F32))
_run_id = lambda r: f"mode{r[0]}-{'bf16io' if r[1] == BF16 else 'f32io'}"
_shape_id = lambda s: "B%d-N%d-dk%d-V%d-r%d" % s


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    ops.set_save_chain_state(True)
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def run_core(case, mode, dtype, backward=True):
    """one call of the core as `mode` describes; returns float64 numpy results by the oracle's names (y alone for a forward-only run)"""
    from mop_amd import ops, _lib as L
    fused = mode in (1, 2, 3)
    path = L.PATH_FUSED if fused else L.PATH_GENERIC
    prec = L.PREC_FP32 if mode == 5 else L.PREC_BF16
    train = mode != 3
    ops.set_save_chain_state(mode != 2)
    ops.LAST_PATH.pop("edgewise_fwd", None), ops.LAST_PATH.pop("edgewise_bwd", None)
    qkv = case.qkv().cuda().to(dtype).requires_grad_(train)
    small = [t.cuda().requires_grad_(train) for t in (case.sqk, case.vs0, case.vsL, case.chain_logit)]
    head = [t.cuda().requires_grad_(train) for t in case.head]
    with torch.set_grad_enabled(train):
        if case.dense:
            y = ops.edgewise_general_core(qkv, *small, head, case.beta_not, case.V, ops.EdgewiseVariant(dense=True), precision=prec)
        else:
            y = ops.edgewise_lowrank_core(qkv, small[0], small[1], small[2], *head, small[3], case.beta_not, case.V, precision=prec, path=path)
    assert ops.LAST_PATH["edgewise_fwd"] == path, "the forward ran on the other path"
    B, N, H, dk = case.q.shape
    out = dict(y=y.detach().double().cpu().numpy().reshape(B, N, H, dk))
    if train and backward:
        y.backward(case.dy.cuda().to(dtype).reshape(B, N, H * dk))
        assert ops.LAST_PATH["edgewise_bwd"] == path, "the backward ran on the other path"
        g = qkv.grad.double().cpu().numpy()[:, :, 0]                         # (B,N,3,H,dk)
        out.update(dq=g[:, :, 0], dk=g[:, :, 1], dv=g[:, :, 2])
        for n_, t in zip(("dsqk", "dvs0", "dvsL", "dchain_logit") + case.head_names, small + head):
            out[n_] = t.grad.double().cpu().numpy()
    torch.cuda.synchronize()
    return out


def judge(case, res, mode, dtype, what, planted_tight=False):
    """the assertions of one run; prints the figures DESIGN.md records"""
    ref = ep.oracle_core(case)
    lo, hi = ep.realised_logit_std(case)
    tag = f"{_shape_id((case.B, case.N, case.dk, case.V, case.r))} L{case.level}{' plant' if case.plant else ''}{' dense' if case.dense else ''} " \
          f"{_run_id((mode, dtype))} [{what}] std {lo:.2f}-{hi:.2f}"
    for n_, t in res.items():
        assert np.isfinite(t).all(), f"{tag}: {n_} is not finite"
    fails = []
    if mode == 5:
        for n_, t in res.items():
            err = rel_err(t, ref[n_]) if n_ in ROW_TENSORS else None
            if err is not None:
                print(f"{tag} {n_}: rel {err:.2e}")
                if err > GTOL_FP32:
                    fails.append(f"{n_}: {err:.3e} > {GTOL_FP32}")
        small = {n_: res[n_] for n_ in res if n_ not in ROW_TENSORS}
        if small:
            check_grads(small, {n_: ref[n_] for n_ in small}, GTOL_FP32)
        assert not fails, f"{tag}: " + "; ".join(fails)
        return
    noise = ep.rounding_noise(case)
    for n_ in [n_ for n_ in ROW_TENSORS if n_ in res]:
        top = float(np.abs(ref[n_]).max())
        io = 2.0 ** -9 * top if dtype == BF16 else 0.0
        err = ep.row_errors(res[n_], ref[n_])
        bound = ep.row_bounds(ref[n_], noise[n_], ep.tol_of(n_), dtype == BF16)
        tight = ep.tol_of(n_) * top + io
        if planted_tight and n_ == "y":
            bound = bound.copy()
            bound[:, list(ep.planted_tokens(case.N))] = tight         # the reference's noise is zero there: no allowance
        ratio = err / bound
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{tag} {n_}: worst err/bound {ratio.max():.2f} at (b, n, h) = {tuple(int(i) for i in at)}; rows above the tight bound: "
              f"kernel {float((err > tight).mean()):.3f}, reference noise {float((ep.NOISE_FACTOR * noise[n_] > tight - io).mean()):.3f}; "
              f"max-norm err {err.max() / top:.2e}")
        if ratio.max() > 1.0:
            fails.append(f"{n_}: {int((ratio > 1).sum())} of {ratio.size} rows over their bound, worst {ratio.max():.2f} x at {at}")
    assert not fails, f"{tag}: " + "; ".join(fails)
    small = {n_: res[n_] for n_ in res if n_ not in ROW_TENSORS}
    if small:
        wide = ep.small_noise(case)
        for n_ in small:
            err = rel_err(small[n_].reshape(ref[n_].shape), ref[n_])
            lim_q, lim = (max(GTOL_BF16, ep.NOISE_FACTOR * d["bf16err:" + n_]) for d in (noise, wide))
            print(f"{tag} {n_}: rel {err:.2e}, err/limit {err / lim:.2f} (q sqk_v rounding alone: {err / lim_q:.2f})")
        check_grads(small, {n_: ref[n_] for n_ in small}, GTOL_BF16, d=wide)


@pytest.mark.parametrize("run", RUNS, ids=_run_id)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_lowrank_level_sweep(shape, level, run):
    """every output finite, every token row within its bound, small gradients within theirs; the last shape forward only.  Prints the
    realised logit std, the worst row error / row bound and where, and the share of rows above the tight bound (kernel | reference)."""
    mode, dtype = run
    case = ep.shape_case(shape, level)
    judge(case, run_core(case, mode, dtype, backward=shape not in ep.FWD_ONLY), mode, dtype, "sweep")


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=_shape_id)
def test_lowrank_planted_rows(shape):
    """level 2 with tokens 0, 31, 32 and N - 1 attending to themselves alone (k[j] = 8 q[j]): y[j] = v[j] vs0 + sigmoid(c) v[j] vsL in
    exact arithmetic, whatever the rounding of q sqk_v, so those rows are held to the plain tolerance in every mode; every other row
    and every gradient as in the sweep.  The suite nowhere asserts that the training and the inference forward agree bit for bit,
    so both are held to the bounds."""
    case = ep.shape_case(shape, 2, plant=True)
    rows = list(ep.planted_tokens(case.N))
    ident = ep.planted_identity(case)
    top = float(np.abs(ep.oracle_core(case)["y"]).max())
    failed = []
    for mode, dtype in RUNS:
        res = run_core(case, mode, dtype)
        lim = GTOL_FP32 * top if mode == 5 else TOL_BF16 * top + (2.0 ** -9 * top if dtype == BF16 else 0.0)
        err = float(np.abs(res["y"][:, rows] - ident).max())
        print(f"N={case.N} {_run_id((mode, dtype))}: planted rows off by {err:.2e} (limit {lim:.2e})")
        if not err <= lim:
            failed.append(f"{_run_id((mode, dtype))}: planted rows off by {err:.3e} > {lim:.3e}")
        try:
            judge(case, res, mode, dtype, "planted", planted_tight=True)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("level", (0.5, 4, 8))
def test_dense_head_level_sweep(level):
    """the dense gate head inside the fused kernels (HEAD = 1: shared qkv, no 3x3, bf16), forward + backward, by the sweep's scheme"""
    case = ep.shape_case(SHAPES[1], level, dense=True)
    for dtype in (F32, BF16):
        judge(case, run_core(case, 1, dtype), 1, dtype, "dense")


def test_extreme_level_stays_finite():
    """shape 3 at level 32 with the planted tokens: |S_v| in the thousands on the planted diagonal and about 150 off it, |Smix| beyond
    ten thousand.  Every output is finite and the planted rows are exact.  No row bound here: the reference itself moves by more
    than its own size under the q sqk_v rounding at this level, so no other assertion would mean anything."""
    case = ep.shape_case(SHAPES[2], 32, plant=True)
    rows = list(ep.planted_tokens(case.N))
    ident = ep.planted_identity(case)
    top = float(np.abs(ep.oracle_core(case)["y"]).max())
    failed = []
    for mode, dtype in ((1, F32), (1, BF16), (3, F32), (3, BF16), (4, F32)):
        res = run_core(case, mode, dtype)
        bad = [n_ for n_, t in res.items() if not np.isfinite(t).all()]
        err = float(np.abs(res["y"][:, rows] - ident).max())
        lim = TOL_BF16 * top + (2.0 ** -9 * top if dtype == BF16 else 0.0)
        print(f"level 32 {_run_id((mode, dtype))}: planted rows off by {err:.2e} (limit {lim:.2e}); non-finite: {bad}")
        if bad or not err <= lim:
            failed.append(f"{_run_id((mode, dtype))}: non-finite {bad}, planted rows off by {err:.3e} (limit {lim:.3e})")
    assert not failed, "\n".join(failed)


def test_peaked_run_is_bitwise_repeatable():
    """the determinism test of test_gpu_edgewise.py runs at flat logits only: shape 3 at level 8, fused training step, twice"""
    case = ep.shape_case(SHAPES[2], 8)
    a, b = run_core(case, 1, BF16), run_core(case, 1, BF16)
    assert set(a) == set(b) and len(a) == 12
    for n_ in a:
        assert np.array_equal(a[n_], b[n_]), n_
