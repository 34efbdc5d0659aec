"""-m gpu: the backward kernels that cap their grid and loop, held to their float64 references at sizes where a workgroup takes a
second, third, ... trip through its loop.

  kernel                                   cap                                   a workgroup's k-th trip
  ln_bwd_kernel (layernorm.hip)            LN_MAX_PARTS = 512 workgroups x 4     rows 2048 k + 4 blockIdx + wave
  tg_bwd_kernel (token_gate.hip)           TG_MAX_PARTS = 512                    the 16-token tile 512 k + blockIdx
  mg_bwd_kernel (mel_gate.hip)             MG_MAX_PARTS = 256                    the 32-frame tile 256 k + blockIdx
  fused Edgewise backward, launches A/B/C  bwd_grid(): 256 x per_cu              the (b,h) item grid k + blockIdx (B: two per (b,h))

What a workgroup carries from one trip to the next -- the dgamma / dbeta / du / dW accumulators and the Edgewise parameter partials,
LDS rewritten behind a barrier, registers of a trip whose rows were past the end, a tile of another batch item than the one before,
halo rows at a sequence start on a later trip, workspace rows indexed by blockIdx.x -- is compared with a reference only here; the
other test files stay at or below the caps wherever they compare with one.

References, bounds and helpers are those of the existing test of each kernel: test_gpu_layernorm._ref (ytol 1e-5 / 1.6e-2, gradients
2e-5 / 8e-3 of the reference's max), test_gpu_gpt._ref64 (1e-4, bf16 1e-2), float64 autograd of test_whisper_gate_cpu._conv_gates
(forward 1e-5, backward 1e-4), oracle/edgewise_torch.py in float64 (TOL_BF16, 3e-2, GTOL_BF16 over the oracle's own bf16 noise).
The "late" variants zero the upstream gradient on everything a workgroup handles on its first trip, so the parameter gradients come
from the later trips alone and a kernel that dropped them would return zeros.  The LayerNorm ops have no second route (a call the
kernels do not cover raises), so there ops.layernorm_supported stands in for the LAST_PATH assertion of the other three."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import check_grads, max_abs
from guarded_alloc import guarded_allocations
from test_gpu_bounds import _assert_guarded_equals_plain, _leaf
from test_gpu_edgewise import GTOL_BF16, TOL_BF16, _mk
from test_gpu_gpt import TILE, _DT, _inputs, _nerr, _ref64
from test_gpu_layernorm import _ref as _ln_ref
from test_gpu_whisper_gate import _mel, _rel
from test_whisper_gate_cpu import _conv_gates, _params

pytestmark = pytest.mark.gpu

LN_WAVES, LN_MAX_PARTS = 4, 512                 # mop_amd/csrc/layernorm.hip
LN_TRIP = LN_WAVES * LN_MAX_PARTS               # rows of one trip of the whole grid (2048)
TG_MAX_PARTS = 512                              # mop_amd/csrc/token_gate.hip (TILE = 16 tokens)
MG_TILE, MG_MAX_PARTS, MG_LC = 32, 256, 8       # mop_amd/csrc/mel_gate.hip (MG_LC: layers per launch)
FUSED = 2

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import _lib, ops
    assert FUSED == _lib.PATH_FUSED
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


# ---- 1. LayerNorm backward ---------------------------------------------------------------------------------------------------------
LN_DTYPES = [(torch.float32, torch.float32, torch.float32), (torch.float32, torch.bfloat16, torch.float32),
             (torch.bfloat16, torch.bfloat16, torch.bfloat16)]
LN_IDS = ["f32-f32-f32", "f32-bf16-f32", "bf16-bf16-bf16"]
# 2048: exactly the cap; 2049: one wave takes one more row; 4100: two full trips + 4 rows for workgroup 0; 6151 x 520: three trips
# and a remainder, 65 vectors = VPL 2 with one live lane in the second chunk; 2061 x 1152: VPL 3
LN_SHAPES = [(2048, 64), (2049, 8), (4100, 72), (6151, 520), (2061, 1152)]
LN_VPL_DIMS = [520, 1544, 2056, 2568, 3080, 3592]      # 64 k + 1 vectors: VPL 2, 4, 5, 6, 7, 8 with one lane in the last chunk


def _ln_case(rows, dim, xdt, ydt, pdt, late=False):
    """the inputs of test_layernorm_forward_backward_vs_torch (same generator, same scaling) and their float64 reference; late: dy
    is zero on the rows of the grid's first trip"""
    def make():
        gen = torch.Generator().manual_seed(rows * 131 + dim)
        x = (torch.randn(rows, dim, generator=gen) * 1.7 + 0.3).to(xdt)
        g = (1.0 + 0.2 * torch.randn(dim, generator=gen)).to(pdt)
        b = (0.1 * torch.randn(dim, generator=gen)).to(pdt)
        dy = torch.randn(rows, dim, generator=gen).to(ydt)
        dres = torch.randn(rows, dim, generator=gen).to(xdt)
        if late:
            dy[:LN_TRIP] = 0
        return (x, g, b, dy, dres), _ln_ref(x.float(), g.float(), b.float(), 1e-5, dy.float(), dres.float())
    return _cached(("ln", rows, dim, xdt, ydt, pdt, late), make)


def _ln_check(res, ref, xdt, ydt, what, names=("dx", "dgamma", "dbeta")):
    yr = ref[0]
    ytol = 1e-5 if ydt == torch.float32 else 1.6e-2
    e = (res["y"].float().cpu().double() - yr).abs().max().item() / max(1.0, yr.abs().max().item())
    print(f"layernorm {what} y: {e:.3e} (bound {ytol:.1e})")
    assert e <= ytol, f"y {e:.2e}"
    gt = 2e-5 if xdt == torch.float32 else 8e-3
    for name, r in zip(("dx", "dgamma", "dbeta"), ref[1:]):
        if name not in names:
            continue
        err = (res[name].float().cpu().double() - r).abs().max().item() / max(1e-6, r.abs().max().item())
        print(f"layernorm {what} {name}: {err:.3e} (bound {gt:.1e})")
        assert err <= gt, f"{name} {err:.2e}"


def _ln_run(t, ydt, residual=True):
    """t: x, g, b (or None), dy, dres on the GPU, the first three leaves"""
    from mop_amd import ops
    assert ops.layernorm_supported(t["x"], t["g"])
    if residual:
        xres, y = ops.layernorm_residual(t["x"], t["g"], t.get("b"), 1e-5, ydt)
        assert y.dtype == ydt and xres.data_ptr() == t["x"].data_ptr()
        torch.autograd.backward([xres, y], [t["dres"], t["dy"]])
    else:
        y = ops.layernorm(t["x"], t["g"], t.get("b"), 1e-5, ydt)
        y.backward(t["dy"])
    torch.cuda.synchronize()
    res = dict(y=y.detach(), dx=t["x"].grad, dgamma=t["g"].grad)
    if t.get("b") is not None:
        res["dbeta"] = t["b"].grad
    return res


def _ln_inputs(x, g, b, dy, dres):
    return dict(x=x.cuda().requires_grad_(True), g=g.cuda().requires_grad_(True), b=b.cuda().requires_grad_(True), dy=dy.cuda(),
                dres=dres.cuda())


@pytest.mark.parametrize("xdt,ydt,pdt", LN_DTYPES, ids=LN_IDS)
@pytest.mark.parametrize("rows,dim", LN_SHAPES, ids=lambda v: str(v))
def test_layernorm_backward_beyond_the_workgroup_cap(rows, dim, xdt, ydt, pdt):
    assert (rows + LN_WAVES - 1) // LN_WAVES >= LN_MAX_PARTS and (rows > LN_TRIP or (rows, dim) == (2048, 64))
    ins, ref = _ln_case(rows, dim, xdt, ydt, pdt)
    _ln_check(_ln_run(_ln_inputs(*ins), ydt), ref, xdt, ydt, f"{rows}x{dim}")


def test_layernorm_backward_beyond_the_cap_without_bias():
    """bias=None: no dbeta is asked for, the reduction launch writes dgamma alone; the reference has a zero bias"""
    rows, dim, (xdt, ydt, pdt) = 6151, 520, LN_DTYPES[1]
    (x, g, b, dy, dres), _ = _ln_case(rows, dim, xdt, ydt, pdt)
    ref = _cached(("ln-nobias", rows, dim), lambda: _ln_ref(x.float(), g.float(), torch.zeros(dim), 1e-5, dy.float(), dres.float()))
    t = _ln_inputs(x, g, b, dy, dres)
    del t["b"]
    res = _ln_run(t, ydt)
    assert "dbeta" not in res
    _ln_check(res, ref, xdt, ydt, f"{rows}x{dim} no bias", names=("dx", "dgamma"))


def test_layernorm_backward_beyond_the_cap_without_the_residual_branch():
    """ops.layernorm: dres is a null pointer in the kernel; the reference adds a zero residual gradient"""
    rows, dim, (xdt, ydt, pdt) = 4100, 72, LN_DTYPES[2]
    (x, g, b, dy, dres), _ = _ln_case(rows, dim, xdt, ydt, pdt)
    ref = _cached(("ln-nores", rows, dim), lambda: _ln_ref(x.float(), g.float(), b.float(), 1e-5, dy.float(), torch.zeros(rows, dim)))
    _ln_check(_ln_run(_ln_inputs(x, g, b, dy, dres), ydt, residual=False), ref, xdt, ydt, f"{rows}x{dim} no residual")


@pytest.mark.parametrize("xdt,ydt,pdt", [LN_DTYPES[0], LN_DTYPES[2]], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim", LN_VPL_DIMS)
def test_layernorm_every_vector_count_per_lane(dim, xdt, ydt, pdt):
    """rows = 5 (one workgroup of four rows, one of one row): the VPL instantiations the other tests do not reach"""
    assert (dim // 8) % 64 == 1 and (dim // 8 + 63) // 64 in (2, 4, 5, 6, 7, 8)
    ins, ref = _ln_case(5, dim, xdt, ydt, pdt)
    _ln_check(_ln_run(_ln_inputs(*ins), ydt), ref, xdt, ydt, f"5x{dim}")


def test_layernorm_parameter_gradients_from_later_trips_alone():
    """(4100, 72) fp32 with dy = 0 on rows < 2048: dgamma and dbeta are what the second and third trips add, held to their own max"""
    rows, dim, (xdt, ydt, pdt) = 4100, 72, LN_DTYPES[0]
    ins, ref = _ln_case(rows, dim, xdt, ydt, pdt, late=True)
    assert not bool(ins[3][:LN_TRIP].any()) and float(ref[2].abs().max()) > 1.0 and float(ref[3].abs().max()) > 1.0
    _ln_check(_ln_run(_ln_inputs(*ins), ydt), ref, xdt, ydt, f"{rows}x{dim} late rows only")


# ---- 2. token gate backward --------------------------------------------------------------------------------------------------------
# 513 tiles, the last of one token | 516 tiles: the second trip's belong to another batch item, one starts a sequence | 520 tiles,
# VPL 2 | 2050 tiles: four trips + 2, the batch item changes inside a workgroup's loop
TG_SHAPES = [(1, 8193, 64), (3, 2737, 96), (5, 1650, 1024), (2, 16400, 64)]


def _tg_tiles(B, T):
    return B * ((T + TILE - 1) // TILE)


def _tg_case(B, T, D, dt, with_a, strided=False, late=False):
    def make():
        xdt, adt = _DT[dt]
        x, a, u, dout = _inputs(B, T, D, xdt, adt if with_a else None, strided, seed=B * 10007 + T * 31 + D)
        odt = torch.bfloat16 if (xdt == torch.bfloat16 and (a is None or adt == torch.bfloat16)) else torch.float32
        dout = dout.to(odt)
        if late:                                   # zero on the first TG_MAX_PARTS tiles in launch order (tile = b tiles + t / 16)
            tile = torch.arange(B, device="cuda").unsqueeze(1) * ((T + TILE - 1) // TILE) + torch.arange(T, device="cuda").unsqueeze(0) // TILE
            dout = dout * (tile >= TG_MAX_PARTS).unsqueeze(-1).to(odt)
        return (x, a, u, dout, odt), _ref64(x, a, u, dout)
    return _cached(("tg", B, T, D, dt, with_a, strided, late), make)


def _tg_run(t):
    from mop_amd import ops
    for k in ("token_gate_fwd", "token_gate_bwd"):
        ops.LAST_PATH.pop(k, None)
    out = ops.token_gate_1d(t["x"], t.get("a"), t["u"])
    out.backward(t["dout"])
    torch.cuda.synchronize()
    assert ops.LAST_PATH["token_gate_fwd"] == FUSED and ops.LAST_PATH["token_gate_bwd"] == FUSED
    res = dict(out=out.detach(), dx=t["x"].grad, du=t["u"].grad)
    if t.get("a") is not None:
        res["da"] = t["a"].grad
    return res


def _tg_inputs(x, a, u, dout):
    t = dict(x=x.detach().requires_grad_(True), u=u.clone().requires_grad_(True), dout=dout)
    if a is not None:
        t["a"] = a.detach().requires_grad_(True)
    return t


def _tg_check(res, ref, dt, odt, adt, what):
    ro, rdx, rdu = ref
    tol = 1e-2 if dt == "bf16" else 1e-4
    assert res["out"].dtype == odt
    figures = [("out", _nerr(res["out"], ro), tol), ("dx", _nerr(res["dx"], rdx), tol), ("du", _nerr(res["du"], rdu), tol)]
    if "da" in res:
        assert res["da"].dtype == adt
        figures.append(("da", _nerr(res["da"], rdx), 1e-2 if adt == torch.bfloat16 else 1e-4))      # da: dr rounded to a's dtype
    for name, e, bound in figures:
        print(f"token gate {what} {name}: {e:.3e} (bound {bound:.1e})")
    for name, e, bound in figures:
        assert e <= bound, f"{what} {name} {e:.2e}"


@pytest.mark.parametrize("with_a", [True, False], ids=["a", "no-a"])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "mixed"])
@pytest.mark.parametrize("B,T,D", TG_SHAPES, ids=lambda v: str(v))
def test_token_gate_backward_beyond_the_workgroup_cap(B, T, D, dt, with_a):
    assert _tg_tiles(B, T) > TG_MAX_PARTS
    (x, a, u, dout, odt), ref = _tg_case(B, T, D, dt, with_a)
    _tg_check(_tg_run(_tg_inputs(x, a, u, dout)), ref, dt, odt, _DT[dt][1], f"B={B} T={T} D={D} {dt} a={with_a}")


def test_token_gate_backward_beyond_the_cap_on_strided_inputs():
    """x: the first half of 2D-wide rows, a: a (T,B,D) buffer seen as (B,T,D) -- the row pointers of every later trip use the strides"""
    B, T, D, dt = 3, 2737, 96, "fp32"
    (x, a, u, dout, odt), ref = _tg_case(B, T, D, dt, True, strided=True)
    assert not x.is_contiguous() and not a.is_contiguous()
    _tg_check(_tg_run(_tg_inputs(x, a, u, dout)), ref, dt, odt, _DT[dt][1], f"B={B} T={T} D={D} {dt} strided")


def test_token_gate_tap_gradients_from_later_trips_alone():
    """(2, 16400, 64) fp32 with dout = 0 on the first 512 tiles (tokens < 8192 of item 0): du is what trips two to five add (the
    first trip's tile 511 contributes the one term its halo token 8192 hands it)"""
    B, T, D, dt = 2, 16400, 64, "fp32"
    (x, a, u, dout, odt), ref = _tg_case(B, T, D, dt, True, late=True)
    assert not bool(dout[0, :TG_MAX_PARTS * TILE].any()) and bool(dout[0, TG_MAX_PARTS * TILE].any()) and float(ref[2].abs().max()) > 1.0
    _tg_check(_tg_run(_tg_inputs(x, a, u, dout)), ref, dt, odt, _DT[dt][1], f"B={B} T={T} D={D} {dt} late tiles only")


# ---- 3. mel gate backward ----------------------------------------------------------------------------------------------------------
# B,T,F,L,k,lens: 257 tiles | 282 tiles, Whisper's own map | 260 tiles, F = 10 takes the element-wise staging and L = 9 two launches
# that write disjoint columns of the same partial rows | lens: the `continue` for tiles behind a clip inside multi-trip loops -- with
# (3000, 1, 1500) the second-trip tiles (frames >= 2176 of clip 2) all lie behind their clip, with (1, 1500, 3000) they are all live
# and 25 of the 26 workgroups that take them have skipped their first tile
MG_CASES = [(1, 8200, 16, 2, 3, None), (3, 3000, 80, 6, 5, None), (5, 1650, 10, 9, 7, None), (3, 3000, 80, 6, 5, (3000, 1, 1500)),
            (3, 3000, 80, 6, 5, (1, 1500, 3000))]
MG_V, MG_K = 3, 2                               # views and kernels of the folded chain: they do not reach the kernels


def _mg_tiles(B, T):
    return B * ((T + MG_TILE - 1) // MG_TILE)


def _mg_case(B, T, Fm, L, k, lens, how, late=False):
    """inputs and the float64 references of test_mel_gate_backward_against_float64_autograd_of_the_convolutions, plus the gates"""
    def make():
        from mop_amd import ops
        prm = [p.cuda() for p in _params(L, MG_V, MG_K, k, seed=6, dtype=torch.float32)]
        mel = _mel(B, T, Fm, how, seed=7)
        dg = torch.randn(B, L, T, generator=torch.Generator().manual_seed(5)).cuda()
        if late:                                   # zero on the first MG_MAX_PARTS tiles in launch order (tile = b tiles + t / 32)
            tile = torch.arange(B, device="cuda").unsqueeze(1) * ((T + MG_TILE - 1) // MG_TILE) + torch.arange(T, device="cuda").unsqueeze(0) // MG_TILE
            dg = dg * (tile >= MG_MAX_PARTS).unsqueeze(1)
        dev_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
        # float64: the clips cut to their lengths are what lens means (zero rows behind, no gradient from the columns behind)
        mel64, dg64 = mel.double(), dg.double()
        if lens is not None:
            live = (torch.arange(T, device="cuda").unsqueeze(0) < dev_lens.unsqueeze(1))
            mel64, dg64 = mel64 * live.unsqueeze(-1), dg64 * live.unsqueeze(1)
        p64 = [p.double().requires_grad_() for p in prm]
        ref = list(torch.autograd.grad(_conv_gates(mel64, *p64), p64, dg64))
        W64 = ops.mel_gate_taps(*[p.double() for p in prm], Fm).requires_grad_()
        gates64 = ops.mel_gate_torch(mel.double(), W64, dev_lens)
        ref.insert(0, torch.autograd.grad(gates64, W64, dg.double())[0])
        return (mel, prm, dg, dev_lens), (gates64.detach(), ref)
    return _cached(("mg", B, T, Fm, L, k, lens, how, late), make)


def _mg_run(mel, prm, dg, lens):
    from mop_amd import ops
    for key in ("mel_gate_fwd", "mel_gate_bwd"):
        ops.LAST_PATH.pop(key, None)
    leaves = [p.detach().clone().requires_grad_() for p in prm]
    W = ops.mel_gate_taps(*leaves, mel.shape[2])
    W.retain_grad()
    gates = ops.mel_gate(mel, W, lens)
    (gates * dg).sum().backward()
    torch.cuda.synchronize()
    assert ops.LAST_PATH["mel_gate_fwd"] == FUSED and ops.LAST_PATH["mel_gate_bwd"] == FUSED
    return gates.detach(), [W.grad] + [p.grad for p in leaves]


def _mg_check(gates, got, ref, what):
    gates64, gref = ref
    e = _rel(gates, gates64)
    print(f"mel gate {what} gates: {e:.3e} (bound 1e-5)")
    assert e <= 1e-5, "gates"
    figures = [(name, _rel(g.reshape(r.shape), r)) for name, g, r in zip(("dW", "Wv", "Wk", "Wf", "alpha"), got, gref)]
    for name, e in figures:
        print(f"mel gate {what} {name}: {e:.3e} (bound 1e-4)")
    for name, e in figures:
        assert e <= 1e-4, name


@pytest.mark.parametrize("how", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,Fm,L,k,lens", MG_CASES, ids=lambda v: str(v))
def test_mel_gate_backward_beyond_the_workgroup_cap(B, T, Fm, L, k, lens, how):
    assert _mg_tiles(B, T) > MG_MAX_PARTS
    ins, ref = _mg_case(B, T, Fm, L, k, lens, how)
    gates, got = _mg_run(*ins)
    _mg_check(gates, got, ref, f"{how} B={B} T={T} F={Fm} L={L} k={k} lens={lens}")


def test_mel_gate_tap_gradients_from_later_trips_alone():
    """(3, 3000, 80, 6, 5) fp32 with dgates = 0 on the first 256 tiles (clips 0 and 1, frames < 2176 of clip 2): dW and the four
    parameter gradients are what the second trip adds"""
    B, T, Fm, L, k = 3, 3000, 80, 6, 5
    ins, ref = _mg_case(B, T, Fm, L, k, None, "fp32", late=True)
    dg, edge = ins[2], (MG_MAX_PARTS - 2 * 94) * MG_TILE
    assert not bool(dg[:2].any()) and not bool(dg[2, :, :edge].any()) and bool(dg[2, :, edge].any())
    assert float(ref[1][0].abs().max()) > 1.0
    gates, got = _mg_run(*ins)
    _mg_check(gates, got, ref, f"fp32 B={B} T={T} F={Fm} L={L} k={k} late tiles only")


# ---- 5. the caps as the library states them ------------------------------------------------------------------------------------------
def test_workspaces_stop_growing_at_the_caps():
    """mopk_*_workspace_bytes of every shape above equals its value at the cap (one partial row per workgroup, not per tile); a moved
    cap shows up here and in the tile counts asserted beside every case"""
    from mop_amd import _lib as L
    lib = L.lib()

    def ln(rows, dim):
        return lib.mopk_layernorm_workspace_bytes(C.byref(L.LayerNormArgs(rows=rows, dim=dim)))

    def tg(B, T, D):
        return lib.mopk_token_gate_workspace_bytes(C.byref(L.TokenGateArgs(B=B, T=T, D=D)))

    def mg(B, T, Fm, Ln, k):
        return lib.mopk_mel_gate_workspace_bytes(C.byref(L.MelGateArgs(B=B, T=T, F=Fm, L=Ln, k=k, mel_dtype=L.MOPK_F32, mel_sb=T * Fm, mel_st=Fm)))

    for rows, dim in LN_SHAPES:
        assert (rows + LN_WAVES - 1) // LN_WAVES >= LN_MAX_PARTS
        assert ln(rows, dim) == ln(LN_TRIP, dim) == LN_MAX_PARTS * 2 * dim * 4, (rows, dim)
    assert ln(LN_TRIP - LN_WAVES, 64) == (LN_MAX_PARTS - 1) * 2 * 64 * 4
    for B, T, D in TG_SHAPES:
        assert _tg_tiles(B, T) > TG_MAX_PARTS
        assert tg(B, T, D) == tg(1, TG_MAX_PARTS * TILE, D) == TG_MAX_PARTS * 3 * D * 4, (B, T, D)
    assert tg(1, (TG_MAX_PARTS - 1) * TILE, 64) == (TG_MAX_PARTS - 1) * 3 * 64 * 4
    for B, T, Fm, Ln, k, _ in MG_CASES:
        assert _mg_tiles(B, T) > MG_MAX_PARTS
        assert mg(B, T, Fm, Ln, k) == mg(1, MG_MAX_PARTS * MG_TILE, Fm, Ln, k) == MG_MAX_PARTS * Ln * k * Fm * 4, (B, T, Fm, Ln, k)
    assert mg(1, (MG_MAX_PARTS - 1) * MG_TILE, 16, 2, 3) == (MG_MAX_PARTS - 1) * 2 * 3 * 16 * 4


# ---- 6. guarded runs -----------------------------------------------------------------------------------------------------------------
def _plain_then_guarded(call, inputs, check_plain, paths, sizes, what):
    """call(dict of leaves) -> {name: tensor}: once on plain tensors (held to the reference), once with every input embedded in NaN
    and every buffer the op allocates -- the capped workspace among them -- between guard bands: guards intact, finite, bit-identical"""
    plain = call({k: _leaf(t, False) for k, t in inputs.items()})
    torch.cuda.synchronize()
    check_plain(plain)
    with guarded_allocations() as ledger:
        guarded = call({k: _leaf(t, True) for k, t in inputs.items()})
        torch.cuda.synchronize()
    _assert_guarded_equals_plain(ledger, plain, guarded, paths, FUSED if paths else None, sizes, what)


def test_layernorm_beyond_the_cap_stays_inside_its_buffers():
    rows, dim, (xdt, ydt, pdt) = 4100, 72, LN_DTYPES[0]
    ins, ref = _ln_case(rows, dim, xdt, ydt, pdt)
    # y, dx; mean, rstd; dgamma, dbeta; the workspace: one (2, dim) float32 row per workgroup of the capped grid
    sizes = 2 * [rows * dim * 4] + 2 * [rows * 4] + 2 * [dim * 4] + [LN_MAX_PARTS * 2 * dim * 4]
    _plain_then_guarded(lambda t: _ln_run(t, ydt), _ln_inputs(*ins), lambda res: _ln_check(res, ref, xdt, ydt, f"{rows}x{dim} plain"),
                        (), sizes, f"layernorm {rows}x{dim}")


def test_token_gate_beyond_the_cap_stays_inside_its_buffers():
    B, T, D, dt = 3, 2737, 96, "bf16"
    (x, a, u, dout, odt), ref = _tg_case(B, T, D, dt, True)
    sizes = 2 * [B * T * D * 2] + [B * T * 4, 3 * D * 4, TG_MAX_PARTS * 3 * D * 4]       # out and dr, the saved gate, du, the workspace
    _plain_then_guarded(_tg_run, _tg_inputs(x, a, u, dout), lambda res: _tg_check(res, ref, dt, odt, _DT[dt][1], f"B={B} T={T} D={D} plain"),
                        ("token_gate_fwd", "token_gate_bwd"), sizes, f"token gate B={B} T={T} D={D} {dt}")


@pytest.mark.parametrize("B,T,Fm,L,k,lens", MG_CASES[3:], ids=lambda v: str(v))
def test_mel_gate_beyond_the_cap_stays_inside_its_buffers(B, T, Fm, L, k, lens):
    from mop_amd import ops
    (mel, prm, dg, dev_lens), (gates64, gref) = _mg_case(B, T, Fm, L, k, lens, "fp32")
    W = ops.mel_gate_taps(*prm, Fm)

    def call(t):
        for key in ("mel_gate_fwd", "mel_gate_bwd"):
            ops.LAST_PATH.pop(key, None)
        gates = ops.mel_gate(t["mel"], t["W"], t["lens"])
        gates.backward(t["dg"])
        return dict(gates=gates.detach(), dW=t["W"].grad)

    def check(res):
        assert _rel(res["gates"], gates64) <= 1e-5 and _rel(res["dW"], gref[0]) <= 1e-4
    sizes = [B * L * T * 4, L * k * Fm * 4, MG_MAX_PARTS * L * k * Fm * 4]                   # gates, dW, the workspace
    _plain_then_guarded(call, dict(mel=mel, W=W.requires_grad_(True), lens=dev_lens, dg=dg), check, ("mel_gate_fwd", "mel_gate_bwd"), sizes,
                        f"mel gate B={B} T={T} F={Fm} L={L} k={k} lens={lens}")


# ---- 7. fused Edgewise backward ------------------------------------------------------------------------------------------------------
# bwd_grid() of mop_amd/csrc/edgewise_fused_bwd.hip: launches A and C run min(B H, 256 per_cu) workgroups, launch B min(2 B H, 256 per_cu);
# per_cu = 1 for N > 96 (NT >= 4) and min(8 / NT, 160 KiB / LDS bytes) below.
#   N = 197 (NT = 7), dk = 64: cap 256.  B H = 259 x 2 = 518 = 2 x 256 + 6: workgroups 0..5 of launches A and C take three trips, the
#     rest two; launch B has 1036 = 4 x 256 + 12 items.
#   N = 8 (NT = 1), dk = 16, V = 2: BwdCfg<1,16>::lds_bytes(2) = 17280 + 1536 + 4 x 752 = 21824, per_cu = min(8, 163840 / 21824) = 7,
#     cap 1792.  B H = 897 x 4 = 3588 = 2 x 1792 + 4: workgroups 0..3 take three trips, the rest two; launch B 7176 = 4 x 1792 + 8.
# V = 2 views and rank 1 are the smallest the fused path takes.  B, N, D, H, V, r, cap, images per oracle chunk
EW_CASES = {"n197": (259, 197, 128, 2, 2, 1, 256, 37), "n8": (897, 8, 64, 4, 2, 1, 1792, 897)}


def _ew_oracle(x, w, params, H, V, chunk):
    """oracle/edgewise_torch.py in float64 on the device, `chunk` images at a time (the N x N planes of 259 images need not be alive
    together); the parameter gradients add up over the chunks"""
    from oracle import edgewise_torch as oet
    p = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    ys, dxs = [], []
    for s in range(0, x.shape[0], chunk):
        xs = x[s:s + chunk].double().requires_grad_(True)
        y = oet.edgewise_layer(xs, p, H, V, 0.5)
        (y * w[s:s + chunk].double()).sum().backward()
        ys.append(y.detach())
        dxs.append(xs.grad)
    return torch.cat(ys), torch.cat(dxs), {k: v.grad.cpu().numpy() for k, v in p.items()}


def _bf16_draw(t, gen):
    """t rounded to bfloat16: to nearest even (gen None), or stochastically -- an independent sample of the same rounding noise"""
    if gen is None:
        return t.float().bfloat16().float()
    bits = t.float().contiguous().view(torch.int32)
    add = torch.randint(0, 1 << 16, t.shape, device=t.device, generator=gen, dtype=torch.int32)
    return ((bits + add) & -65536).view(torch.float32)


def _ew_oracle_bf16_noise(x, w, params, H, V, chunk, exact, samples=2):
    """gpu_util.oracle_bf16_noise on the torch oracle: how far the float64 gradients move when x, the upstream gradient and every
    parameter are rounded to bfloat16 (max-abs / max|exact| per tensor, the largest of `samples` draws), as check_grads reads it"""
    gen = torch.Generator(device="cuda").manual_seed(1234)
    noise = {}
    for i in range(samples):
        g = gen if i else None
        _, _, gb = _ew_oracle(_bf16_draw(x, g), _bf16_draw(w, g), {k: _bf16_draw(v, g) for k, v in params.items()}, H, V, chunk)
        for k in exact:
            e = max_abs(gb[k], exact[k]) / max(float(np.abs(exact[k]).max()), 1e-30)
            noise["bf16err:" + k] = max(e, noise.get("bf16err:" + k, 0.0))
    return noise


def _ew_edgewise_ws(B, N, H, dk, V, r):
    from mop_amd import _lib as L
    a = L.EdgewiseArgs(B=B, H=H, N=N, dk=dk, V=V, r=r, io_dtype=L.MOPK_F32, precision=L.PREC_BF16, path=L.PATH_FUSED, save_for_backward=1)
    return L.lib().mopk_edgewise_workspace_bytes(C.byref(a))


@pytest.mark.parametrize("late", [False, True], ids=["all", "late-only"])
@pytest.mark.parametrize("case", list(EW_CASES))
def test_fused_edgewise_backward_beyond_its_grid(case, late):
    """EdgewiseMSA (shared qkv, low-rank head) on the fused bf16 kernels with more (b,h) pairs than twice the persistent grid, against
    oracle/edgewise_torch.py in float64: y, dx of every image, every parameter gradient.  Caps the shapes were derived from: 256
    workgroups at N = 197 (per_cu = 1), 1792 = 256 x 7 at N = 8, dk = 16, V = 2 (see EW_CASES); the workspace query confirms them.
    late-only: the upstream gradient is zero for the images whose (b,h) pairs all fall in the first trip of launches A and C, so
    every parameter gradient is what the later trips add.
    Bounds of test_fused_lowrank_batch_of_three_at_full_size_vs_oracle: TOL_BF16 on y, 3e-2 on dx per image, GTOL_BF16 per parameter
    gradient or 4 x the oracle's own bf16 noise where that is larger."""
    import mop_amd
    from mop_amd import ops
    B, N, D, H, V, r, cap, chunk = EW_CASES[case]
    dk = D // H
    assert B * H > 2 * cap and B * H < 3 * cap
    # the cap as the library states it: one scratch region per workgroup of launch B's grid min(2 B H, cap) plus one hand-off region
    # per (b,h), so an image adds less workspace once 2 B H has passed the cap
    b_cap = cap // (2 * H)
    ws = lambda b: _ew_edgewise_ws(b, N, H, dk, V, r)
    below, above = ws(b_cap) - ws(b_cap - 1), ws(b_cap + 1) - ws(b_cap)
    assert ws(2) - ws(1) == below and ws(B) - ws(B - 1) == above and 0 < above < below, (below, above)
    first_trip = cap // H                           # images whose (b,h) pairs all lie below the cap
    mop_amd.set_precision("bf16")
    m = _mk(D, H, V, r, seed=B * 1000 + N).cuda().eval()
    params = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator(device="cuda").manual_seed(N + B)
    x = torch.randn(B, N, D, device="cuda", generator=g)
    w = torch.randn(B, N, D, device="cuda", generator=g)
    if late:
        w[:first_trip] = 0
    out, dx_ref, g_ref = _ew_oracle(x, w, params, H, V, chunk)

    for k in ("edgewise_fwd", "edgewise_bwd"):
        ops.LAST_PATH.pop(k, None)
    xt = x.clone().requires_grad_(True)
    y = m(xt)
    y.backward(w)
    torch.cuda.synchronize()
    assert ops.LAST_PATH["edgewise_fwd"] == FUSED and ops.LAST_PATH["edgewise_bwd"] == FUSED
    grads = {k: p.grad.detach().float().cpu().numpy() for k, p in m.named_parameters()}

    ey = float((y.detach().double() - out).abs().max())
    print(f"edgewise {case} late={late} y: {ey:.3e} (bound {TOL_BF16:.1e})")
    assert ey <= TOL_BF16
    # every image separately: a trip that used another item's record or hand-off region would hit some images and not others
    err = (xt.grad.double() - dx_ref).abs().amax(dim=(1, 2))
    own = dx_ref.abs().amax(dim=(1, 2))
    live = slice(first_trip, B) if late else slice(0, B)
    e_live = float((err[live] / own[live]).max())
    print(f"edgewise {case} late={late} dx, worst image: {e_live:.3e} (bound 3.0e-02)")
    assert e_live <= 3e-2, f"dx, image {int((err[live] / own[live]).argmax())}"
    if late:                                        # no gradient reaches the first-trip images: theirs is zero in the oracle
        assert float(own[:first_trip].max()) == 0.0
        assert float(err[:first_trip].max()) <= 3e-2 * float(own.max())
    # noise floor: how far the oracle's own float64 gradients move under bf16 rounding of its inputs, computed on the oracle here for
    # these very inputs (two draws) and never on the kernels; the bound per tensor is max(GTOL_BF16 = 3e-2, 4 x that value).  Largest
    # values seen: n197 chain_value_logit 1.5e-2 (late-only 6.0e-2), q_scale / k_scale 1.1e-2 (1.5e-2), row_proj 2.0e-2;
    # n8 col_proj 4.0e-2 (3.1e-2), row_proj 1.3e-2 (2.5e-2); every other tensor below 3e-2 / 4, i.e. held to GTOL_BF16 itself
    noise = _ew_oracle_bf16_noise(x, w, params, H, V, chunk, g_ref)
    print(f"edgewise {case} late={late} oracle bf16 noise: " + ", ".join(f"{k[8:]} {v:.2e}" for k, v in noise.items()))
    for k in g_ref:
        e = max_abs(grads[k].reshape(g_ref[k].shape), g_ref[k]) / max(float(np.abs(g_ref[k]).max()), 1e-30)
        print(f"edgewise {case} late={late} {k}: {e:.3e} (bound {max(GTOL_BF16, 4.0 * noise['bf16err:' + k]):.1e})")
    assert all(float(np.abs(v).max()) > 0 for v in g_ref.values())
    check_grads(grads, g_ref, GTOL_BF16, d=noise)
