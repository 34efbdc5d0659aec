"""-m gpu: the attention cores on strided and broadcast views (the stride arithmetic of sdpa_flash.hip, quartet_flash.hip,
attn_generic.hip, decode_attn.hip and the dual-path element-wise passes), and the mask / bias forms on the device.

Every core takes its operands as MopkView4 (pointer + batch, head and token strides).  The other GPU tests feed them a fresh
contiguous (B,N,H,dk) tensor or the slots of a packed (B,N,3,H,dk) projection; here each operand of a call gets one of the eight
layouts of tests/attn_layouts.py, whose storage is NaN outside the view.

Subjects: one small case per core and path (SUBJECTS).  B = 2 and H = 3 (no two extents or strides coincide), N = 131 (two 128-row
query blocks, the second partial), Nk = 70 where rectangular (two 64-key tiles, the second partial), dk 32 / 64 on the fused paths,
dk = 40 or fp32 arithmetic on the generic ones; the decode ops have cap = 130 (two or three key chunks), a device kv_len of 129,
Tq = 1 and Tq = 3 causal, dk = 64 bf16 and dk = 128 fp32.

  anchor     each subject once in the plain way, on contiguous tensors, against its float64 reference under the constants of the
             file that already tests the core (named at each check; nothing here has a tolerance of its own)
  rotations  r = 0 .. 7: operand j gets layout (j + r) mod 8 -- no two operands of a call share a layout, every operand meets
             every layout, so a kernel that reads one operand with another's strides cannot pass.  The run on the views (the
             leaves are the storages) and a run on contiguous copies of the same views, pinned to the path the view run took,
             must agree BIT FOR BIT in y, in the gradient the Function returned for every view (view.retain_grad(): a broadcast
             operand's gradient before autograd sums it), in the scalar gradients, the returned weights and crossview's k_star.
             Layout changes addresses only and every core is run-to-run deterministic, so no tolerance applies.  Everything must be
             finite: the NaN padding never leaks.
  uniform    all operands heads_first, and all operands window
  paths      the expected path of every run comes from the documented rule -- pointer and all three strides multiples of 16 bytes,
             plus the core's own dk / arithmetic conditions (_aligned and the subjects' `expect`) -- and is asserted against
             ops.LAST_PATH; it is never read off the run.  odd_rows is aligned for float32 and not for bfloat16: a bf16 call with
             such an operand must take the generic kernels, an fp32 one must stay fused.  The decode kernels read q by scalar
             loads, so only their K / V caches count; a bf16 odd_rows cache sends the call to torch's einsum composition, whose
             kernel choice may depend on strides: that one case is held to the float64 reference under
             test_gpu_whisper_decode.py's bound instead of the bitwise comparison.
  forms      every broadcast form of an attn_mask / bias / add_mask gives bitwise the result of the materialised (B,H,N,Nk) tensor,
             forward and backward; the forms broadcast along the keys close whole rows ((N,1) bias of -inf on two rows, (B,1,N,1)
             mask), which must come out as the zero rows of attn_ref.sdpa_ref64
  C ABI      mopk_sdpa_fwd / mopk_sdpa_bwd writing y, dq, dk, dv into heads_first and wide_rows buffers filled with a sentinel: the
             views hold bitwise the contiguous run's results and every byte outside them is still the sentinel

The anchors do not assert d chain_logit of the dual path (a sum of B N H dk signed terms that a random upstream gradient leaves
ill-conditioned, see test_gpu_generic_head_sizes.py); the bitwise comparisons cover it."""
import contextlib
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import attn_layouts as al
from attn_ref import bf16_exact, blocked_rows_mask, sdpa_ref64
from gpu_util import max_abs, rel_err
from test_gpu_attn_edges import GFLOOR, GTOL, YTOL, _assert_close, _gerrs, _yerr      # bf16 arithmetic or bf16 tensors
from test_gpu_generic_head_sizes import FP32_GTOL, FP32_YTOL, MAX_DRAWS, NOISE_FACTOR     # fp32 arithmetic on fp32 tensors; draws

pytestmark = pytest.mark.gpu

QT_SCALAR_TOL = 5e-2                    # test_gpu_bounds.test_quartet: |d mixture|, |d quartet_scale| errors / max(|want|, 1e-3)
DROP_YTOL, DROP_GTOL = 1e-2, 3e-2       # test_gpu_dropout.test_sdpa_dropout_matches_the_oracle_under_the_same_mask
DECODE_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}     # test_gpu_whisper_decode.test_op_sweep_vs_float64
FUSED, GENERIC = 2, 1
B, H, N, NK = 2, 3, 131, 70
CAP, KV_LEN = 130, 129
GATES = (0.8, 0.4, 0.3)                 # and, or, not
CV_MIX = [[1.0, 0.5], [-0.25, 0.75]]
CV_KW = dict(t1=0.3, t2=-0.2, prior_weight=0.4, anchor_mode="argmax_row_sum")


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    assert (FUSED, GENERIC) == (mop_amd._lib.PATH_FUSED, mop_amd._lib.PATH_GENERIC)
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _gen(name):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(name.encode()))


def _rand(shape, g, dt, exact=False):
    """N(0, 1) as the kernels read it: bf16-exact values unless arithmetic and tensors are fp32"""
    t = torch.randn(*shape, device="cuda", generator=g)
    return t if exact else bf16_exact(t).to(dt)


def _np(t):
    return t.detach().double().cpu().numpy()


def _hp(t):
    """(B,N,H,dk) torch -> (B,H,N,dk) float64 numpy (the oracle layout)"""
    return np.transpose(_np(t), (0, 2, 1, 3))


def _bnhd(a):
    """(B,H,N,dk) oracle array -> (B,N,H,dk)"""
    return np.transpose(np.asarray(a), (0, 2, 1, 3))


def _aligned(views):
    """the documented rule of the fused kernels' 16-byte loads, on every view given"""
    return all(al.aligned16(v) for v in views)


def _close(y, yr, got, ref, exact, what):
    """y and the gradients in `ref` against float64.  exact (fp32 arithmetic on fp32 tensors): FP32_YTOL on max-abs(y), FP32_GTOL on
    max-abs(grad) / max|ref|; else test_gpu_attn_edges._assert_close: YTOL, GTOL, GFLOOR.  Prints the figures first."""
    y, yr = np.asarray(y, np.float64), np.asarray(yr, np.float64).reshape(np.shape(y))
    got = {n: np.asarray(got[n], np.float64).reshape(np.shape(ref[n])) for n in ref}
    if exact:
        ey, ge = max_abs(y, yr), {n: rel_err(got[n], ref[n]) for n in ref}
    else:
        ey, ge = _yerr(y, yr), _gerrs(got, ref, GFLOOR)
    print(f"\nFIG {what}: y {ey:.3e} " + " ".join(f"{n} {e:.3e}" for n, e in ge.items()))
    if exact:
        assert np.isfinite(y).all() and all(np.isfinite(g).all() for g in got.values()), what
        assert ey <= FP32_YTOL, f"{what}: y {ey:.3e}"
        for n, e in ge.items():
            assert e <= FP32_GTOL, f"{what}: {n} {e:.3e}"
    else:
        _assert_close(y, yr, got, ref, what)          # YTOL, GTOL, GFLOOR


# ------------------------------------------------------------------------------------------------ subjects
class Subject:
    """names: the operands that vary in layout, vals: their (B,n,H,dk) values; scalars: further leaves (name -> tensor); dy: the
    incoming gradient (None: the op has no backward and runs under no_grad); prec: the arithmetic set before a run; call(t) -> the
    output(s), outs their names; keys: the LAST_PATH entries the call sets; expect(views) -> the path the documented rule gives for
    these operand views; check(res): the float64 reference under the core's own bounds"""

    def __init__(self, name, vals, call, keys, expect, check, prec, dy=None, scalars=None, outs=("y",), k_star=False, torch_fallback=False):
        self.name, self.vals, self.call, self.keys, self.expect, self.check, self.prec = name, vals, call, tuple(keys), expect, check, prec
        self.names, self.dy, self.scalars, self.outs, self.k_star = tuple(vals), dy, scalars or {}, tuple(outs), k_star
        self.torch_fallback = torch_fallback          # GENERIC is a torch composition (decode ops): no bitwise claim there

    @property
    def grad(self):
        return self.dy is not None


SUBJECTS = {}


def _subject(name):
    def deco(fn):
        SUBJECTS[name] = functools.lru_cache(maxsize=None)(lambda: fn(name))
        return fn
    return deco


def subject(name) -> Subject:
    return SUBJECTS[name]()


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def run(s: Subject, views: dict, pin="auto"):
    """one forward (and backward) of the subject on the given operand tensors -> ({name: tensor}, {LAST_PATH key: path})"""
    import mop_amd
    from mop_amd import ops
    mop_amd.set_precision(s.prec)
    ops.set_path(pin)
    for k in s.keys:
        ops.LAST_PATH.pop(k, None)
    sc = {k: v.detach().clone().requires_grad_(s.grad) for k, v in s.scalars.items()}
    for v in views.values():
        if v.requires_grad and not v.is_leaf:
            v.retain_grad()
    with contextlib.nullcontext() if s.grad else torch.no_grad():
        ys = _tuple(s.call({**views, **sc}))
    res = {n: y.detach() for n, y in zip(s.outs, ys)}
    if s.k_star:
        res["k_star"] = ops.LAST_PATH["crossview_k_star"].clone()
    if s.grad:
        ys[0].backward(s.dy)
        for k, v in {**views, **sc}.items():
            assert v.grad is not None, f"{s.name}: no gradient for {k}"
            res["d" + k] = v.grad.detach()
    torch.cuda.synchronize()
    return res, {k: ops.LAST_PATH.get(k) for k in s.keys}


def layout_views(s: Subject, layouts):
    return {n: al.build(lay, s.vals[n], requires_grad=s.grad)[1] for n, lay in zip(s.names, layouts)}


def contiguous_copies(s: Subject, views):
    return {n: v.detach().clone(memory_format=torch.contiguous_format).requires_grad_(s.grad) for n, v in views.items()}


def same(got, want, what):
    """bit for bit, dtype and shape included"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for n in sorted(want):
        g, w = got[n], want[n]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {n} is {g.dtype} {tuple(g.shape)}, the contiguous run's {w.dtype} {tuple(w.shape)}"
        assert torch.equal(g, w), (f"{what}: {n} differs from the contiguous run in {int((g != w).sum())} value(s), "
                                   f"max |diff| {float((g.double() - w.double()).abs().max()):.3e}")


def finite(res, what):
    for n, t in res.items():
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), f"{what}: {n} is not finite (NaN padding read?)"


def views_against_contiguous(s: Subject, layouts):
    what = f"{s.name} [{' '.join(f'{n}={lay}' for n, lay in zip(s.names, layouts))}]"
    views = layout_views(s, layouts)
    for n, lay in zip(s.names, layouts):
        assert al.view4(views[n]) == al.expected_strides(lay, *s.vals[n].shape), (what, n)
    want = s.expect(views)                                  # from the rule, before anything runs
    got, paths = run(s, views)
    assert paths == {k: want for k in s.keys}, f"{what}: took {paths}, the alignment rule gives {want}"
    finite(got, what)
    if s.torch_fallback and want == GENERIC:
        s.check(got, {n: v.detach() for n, v in views.items()})        # torch's einsum may pick another kernel for other strides
        return
    ref, rpaths = run(s, contiguous_copies(s, views), pin={FUSED: "fused", GENERIC: "generic"}[want])
    assert rpaths == paths, (what, rpaths)
    same(got, ref, what)


# ---- plain SDPA
def _sdpa(name, nk, dk, dt, prec, kind):
    from mop_amd import ops
    g = _gen(name)
    exact = prec == "fp32" and dt == torch.float32
    vals = {n: _rand((B, m, H, dk), g, dt, exact) for n, m in (("q", N), ("k", nk), ("v", nk))}
    dy = _rand((B, N, H * dk), g, dt, exact)
    kw, ref_mask, p, seed = {}, None, 0.2, 0x5EED0000 + dk
    if kind == "causal":
        kw = dict(causal=True)
    elif kind == "mask+bias":
        ref_mask = torch.stack([blocked_rows_mask(N, nk, g) for _ in range(B)]).unsqueeze(1)          # (B,1,N,Nk), rows 0 and N - 2 closed
        kw = dict(attn_mask=ref_mask, bias=torch.randn(1, H, N, nk, device="cuda", generator=g))
    elif kind == "lens":
        kw = dict(q_lens=torch.tensor([N, 67], dtype=torch.int32, device="cuda"),        # one full row; one ending inside a tile
                  kv_lens=torch.tensor([nk - 5, 33], dtype=torch.int32, device="cuda"))
        ref_mask = ops.sdpa_lens_mask(kw["q_lens"], kw["kv_lens"], B, N, nk, "cuda")
    elif kind == "dropout":
        kw = dict(dropout_p=p, seed=seed)

    def check(res):
        q, k, v = (vals[n] for n in "qkv")
        got = {n: _np(res[n]) for n in ("dq", "dk", "dv")}
        if kind == "dropout":
            from oracle import sdpa as osd
            drop = ops.dropout_keep_mask(seed, p, B, H, N, nk).numpy().astype(np.float64) / (1.0 - p)
            yo, c = osd.core_fwd(_hp(q), _hp(k), _hp(v), None, None, drop)
            go = osd.core_bwd(_hp(dy.view(B, N, H, dk)), c)
            yo = _bnhd(yo).reshape(B, N, H * dk)
            ey = max_abs(_np(res["y"]), yo)
            ge = {n: rel_err(got[n], _bnhd(go[n])) for n in got}
            print(f"\nFIG {name}: y {ey:.3e} " + " ".join(f"{n} {e:.3e}" for n, e in ge.items()))
            assert ey <= DROP_YTOL * max(1.0, float(np.abs(yo).max())), ey
            for n, e in ge.items():
                assert e <= DROP_GTOL, (n, e)
            return
        r = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
        yr = sdpa_ref64(*r, mask=ref_mask, bias=kw.get("bias"), causal=kw.get("causal", False))
        (yr * dy.double()).sum().backward()
        _close(_np(res["y"]), _np(yr), got, {n: _np(t.grad) for n, t in zip(("dq", "dk", "dv"), r)}, exact, name)
        if ref_mask is not None:
            empty = ~torch.broadcast_to(ref_mask, (B, 1, N, nk))[:, 0].any(-1)                         # (B,N): rows with no open key
            assert bool(empty.any())
            assert bool((res["y"][empty] == 0).all()) and bool((res["dq"][empty] == 0).all())

    def expect(views):
        return FUSED if prec == "bf16" and dk in (32, 64) and _aligned(views.values()) else GENERIC
    return Subject(name, vals, lambda t: ops.sdpa_core(t["q"], t["k"], t["v"], **kw), ("sdpa_fwd", "sdpa_bwd"), expect, check, prec, dy=dy)


for _name, _args in {
    "sdpa-fused-plain-bf16-dk64": (N, 64, torch.bfloat16, "bf16", "plain"),
    "sdpa-fused-causal-fp32io-dk32": (N, 32, torch.float32, "bf16", "causal"),
    "sdpa-fused-rect-bf16-dk32": (NK, 32, torch.bfloat16, "bf16", "plain"),
    "sdpa-fused-mask+bias-fp32io-dk64": (NK, 64, torch.float32, "bf16", "mask+bias"),
    "sdpa-fused-lens-bf16-dk64": (NK, 64, torch.bfloat16, "bf16", "lens"),
    "sdpa-fused-dropout-bf16-dk32": (N, 32, torch.bfloat16, "bf16", "dropout"),
    "sdpa-generic-rect-bf16-dk40": (NK, 40, torch.bfloat16, "bf16", "plain"),
    "sdpa-generic-fp32-dk32": (N, 32, torch.float32, "fp32", "causal"),
}.items():
    _subject(_name)(functools.partial(lambda name, args: _sdpa(name, *args), args=_args))


# ---- dual path (MultiHopMSA)
def _dualpath(name, dk, dt, chain, causal):
    from mop_amd import ops
    g = _gen(name)
    names = ("q1", "k1", "v1", "q2", "k2", "v2")
    vals = {n: _rand((B, N, H, dk), g, dt) for n in names}
    dy = _rand((B, N, H * dk), g, dt)
    hops, beta, lg = 2, 0.6, -0.5

    def check(res):
        from oracle import multihop as om
        blocked = np.broadcast_to(~np.tril(np.ones((N, N), dtype=bool)), (B, 1, N, N)) if causal else None
        yo, c = om.core_fwd(*(_hp(vals[n]) for n in names), dict(and_=GATES[0], or_=GATES[1], not_=GATES[2], chain=chain), beta, hops, lg, blocked)
        go = om.core_bwd(_hp(dy.view(B, N, H, dk)), c)
        _close(_np(res["y"]), _bnhd(yo).reshape(B, N, -1), {"d" + n: _np(res["d" + n]) for n in names},
               {"d" + n: _bnhd(go["d" + n]) for n in names}, False, name)

    def expect(views):
        return FUSED if chain == 0.0 and dk in (32, 64) and _aligned(views.values()) else GENERIC
    call = lambda t: ops.dualpath_core(*(t[n] for n in names), t["lg"], *GATES, chain, beta, hops, None, causal=causal)   # noqa: E731
    return Subject(name, vals, call, ("dualpath_fwd", "dualpath_bwd"), expect, check, "bf16", dy=dy,
                   scalars=dict(lg=torch.tensor(lg, device="cuda")))


_subject("dualpath-fused-bf16-dk64")(lambda name: _dualpath(name, 64, torch.bfloat16, 0.0, False))
_subject("dualpath-fused-causal-fp32io-dk32")(lambda name: _dualpath(name, 32, torch.float32, 0.0, True))
_subject("dualpath-generic-chain-bf16-dk40")(lambda name: _dualpath(name, 40, torch.bfloat16, 0.5, False))


# ---- Quartet
def _quartet(name, dk, dt, need_weights, with_mask):
    from mop_amd import ops
    from oracle import quartet as oq
    names = ("q", "k", "v", "q2", "k2")
    scalar_names = dict(dmix="dmixture", dqs="dquartet_scale")

    def oracle(operands, mask):
        yo, c = oq.core_fwd(*operands[:5], 0.3, 0.8, 1e-5, True, True, mask)
        return yo, oq.core_bwd(operands[5], c)

    def scalar_lim(want):
        return QT_SCALAR_TOL * max(abs(want), 1e-3)

    # d mixture and d quartet_scale are sums of B H N N signed terms, which a random draw can leave cancelling to far below their
    # terms' magnitude.  No bound can be asked of such a sum, so a draw is kept only if the REFERENCE resolves both under one bf16
    # rounding of its operands (a relative 2^-9 x U(-1, 1)), NOISE_FACTOR below the bound asserted -- the kernels take no part
    # (test_gpu_generic_head_sizes._well_conditioned)
    for draw in range(MAX_DRAWS):
        g = _gen(f"{name}/{draw}")
        vals = {n: _rand((B, N, H, dk), g, dt) for n in names}
        dy = _rand((B, N, H * dk), g, dt)
        am = 2.0 * torch.randn(B, 1, N, N, device="cuda", generator=g) if with_mask else None
        operands = [_hp(vals[n]) for n in names] + [_hp(dy.view(B, N, H, dk))]
        mask = None if am is None else _np(am)
        yo, go = oracle(operands, mask)
        rng = np.random.default_rng(2024)
        _, gn = oracle([a * (1.0 + 2.0 ** -9 * rng.uniform(-1.0, 1.0, a.shape)) for a in operands], mask)
        if all(NOISE_FACTOR * abs(float(gn[k]) - float(go[k])) <= scalar_lim(float(go[k])) for k in scalar_names.values()):
            break
    else:
        raise AssertionError(f"{name}: no well-conditioned draw in {MAX_DRAWS}")

    def check(res):
        """tensors under test_gpu_attn_edges' bound, the two scalar gradients as test_gpu_bounds.test_quartet asserts them"""
        _close(_np(res["y"]), _bnhd(yo).reshape(B, N, -1), {"d" + n: _np(res["d" + n]) for n in names},
               {"d" + n: _bnhd(go["d" + n]) for n in names}, False, name)
        for k, o in scalar_names.items():
            got, want = float(res[k]), float(go[o])
            print(f"FIG {name}: {o} {got:.6e} want {want:.6e} (limit {scalar_lim(want):.3e})")
            assert abs(got - want) <= scalar_lim(want), (o, got, want)          # QT_SCALAR_TOL

    def expect(views):
        return FUSED if not need_weights and dk in (32, 64) and _aligned(views.values()) else GENERIC
    call = lambda t: ops.quartet_core(*(t[n] for n in names), t["mix"], t["qs"], am, 1e-5, True, need_weights)   # noqa: E731
    return Subject(name, vals, call, ("quartet_fwd",), expect, check, "bf16", dy=dy, outs=("y", "attn") if need_weights else ("y",),
                   scalars=dict(mix=torch.tensor([0.3], device="cuda"), qs=torch.tensor([0.8], device="cuda")))


_subject("quartet-fused-bf16-dk64")(lambda name: _quartet(name, 64, torch.bfloat16, False, False))
_subject("quartet-fused-addmask-fp32io-dk32")(lambda name: _quartet(name, 32, torch.float32, False, True))
_subject("quartet-generic-weights-bf16-dk32")(lambda name: _quartet(name, 32, torch.bfloat16, True, False))


# ---- CrossView, unfolded (transpose cues and the per-key prior on)
@_subject("crossview-prior-bf16-dk40")
def _crossview(name):
    from mop_amd import ops
    g = _gen(name)
    dk, dt = 40, torch.bfloat16
    names = ("q1", "k1", "v1", "q2", "k2")
    vals = {n: _rand((B, N, H, dk), g, dt) for n in names}
    dy = _rand((B, N, H * dk), g, dt)

    def check(res):
        """the oracle at the anchor rows the device picked (the argmax over row sums of a row-stochastic map is decided by rounding)"""
        from oracle import crossview as oc
        yo, c = oc.core_fwd(*(_hp(vals[n]) for n in names), np.asarray(CV_MIX), t1=CV_KW["t1"], t2=CV_KW["t2"],
                            prior_weight=CV_KW["prior_weight"], k_star=res["k_star"].cpu().numpy().astype(np.int64))
        go = oc.core_bwd(_hp(dy.view(B, N, H, dk)), c)
        got = {"d" + n: _np(res["d" + n]) for n in names}
        ref = {"d" + n: _bnhd(go["d" + n]) for n in names}
        got["dmix"], ref["dmix"] = _np(res["dmix"]), go["dmix"]
        _close(_np(res["y"]), _bnhd(yo).reshape(B, N, -1), got, ref, False, name)
    call = lambda t: ops.crossview_core(*(t[n] for n in names), t["mix"], **CV_KW)       # noqa: E731
    return Subject(name, vals, call, ("crossview_fwd",), lambda views: GENERIC, check, "bf16", dy=dy, k_star=True,
                   scalars=dict(mix=torch.tensor(CV_MIX, device="cuda")))


# ---- the decode ops (no backward; only q and the K / V caches vary in layout)
def _decode_ref64(q, k, v, L, causal, rows=None, kv_start=None, kv_lens=None):
    """float64, one (row, query) at a time: key j of row b from cache row rows[b, j], open if kv_start[b] <= j < min(L, kv_lens[b])
    and, causal, j < L - Tq + i + 1; a query with no open key gives 0"""
    Bq, Tq, Hq, dk = q.shape
    y = torch.zeros(Bq, Tq, Hq, dk, dtype=torch.float64, device=q.device)
    j = torch.arange(k.shape[1], device=q.device)
    for b in range(Bq):
        kb, vb = (t[rows[b, :k.shape[1]].long(), j] if rows is not None else t[b] for t in (k, v))
        lo = int(kv_start[b]) if kv_start is not None else 0
        hi = min(L, int(kv_lens[b])) if kv_lens is not None else L
        for i in range(Tq):
            top = min(hi, L - Tq + i + 1) if causal else hi
            if top <= lo:
                continue
            s = torch.einsum("hd,jhd->hj", q[b, i].double(), kb[lo:top].double()) / dk ** 0.5
            y[b, i] = torch.einsum("hj,jhd->hd", s.softmax(-1), vb[lo:top].double())
    return y.reshape(Bq, Tq, Hq * dk)


def _decode(name, op, Bd, Tq, dk, dt, causal):
    from mop_amd import ops
    g = _gen(name)
    vals = {n: torch.randn(Bd, m, H, dk, device="cuda", generator=g).to(dt) for n, m in (("q", Tq), ("k", CAP), ("v", CAP))}
    kv_len = torch.tensor([KV_LEN], dtype=torch.int32, device="cuda")
    kw, rkw, L = dict(kv_len=kv_len, causal=causal), {}, KV_LEN
    if op == "decode_attention_rows":
        rkw = dict(rows=((torch.arange(Bd, device="cuda")[:, None] + 1 + torch.arange(CAP, device="cuda")[None]) % Bd).to(torch.int32))
    elif op == "decode_attention_ragged":
        rkw = dict(kv_start=torch.tensor([0, 70][:Bd], dtype=torch.int32, device="cuda"))
    elif op == "decode_attention_lens":
        kw, L = {}, CAP                                     # non-causal by definition, the row's own key count
        rkw = dict(kv_lens=torch.tensor([KV_LEN, 65][:Bd], dtype=torch.int32, device="cuda"))
    key = ops._DA_OPS[op][2]

    def check(res, seen=None):
        """seen: the operand tensors of the run (broadcast layouts hold the first batch row / head only); None: vals"""
        seen = seen or vals
        ref = _decode_ref64(seen["q"], seen["k"], seen["v"], L, causal, **rkw)
        e = float((res["y"].double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))        # test_gpu_whisper_decode._rel
        print(f"\nFIG {name}: y {e:.3e}")
        assert e <= DECODE_TOL[dt], f"{name}: y {e:.3e}"

    def expect(views):                                      # da_check: dk, Tq, and the K / V cache views; q is read by scalar loads
        return FUSED if dk in (32, 64, 128) and Tq <= 16 and _aligned((views["k"], views["v"])) else GENERIC
    call = lambda t: getattr(ops, op)(t["q"], t["k"], t["v"], **rkw, **kw)             # noqa: E731
    return Subject(name, vals, call, (key,), expect, check, "bf16" if dt == torch.bfloat16 else "fp32", torch_fallback=True)


for _name, _args in {
    "decode-bf16-dk64-tq1": ("decode_attention", B, 1, 64, torch.bfloat16, False),
    "decode-causal-fp32-dk128-tq3": ("decode_attention", B, 3, 128, torch.float32, True),
    "decode-rows-causal-bf16-dk64-tq3": ("decode_attention_rows", 3, 3, 64, torch.bfloat16, True),
    "decode-rows-fp32-dk128-tq1": ("decode_attention_rows", 3, 1, 128, torch.float32, False),
    "decode-ragged-causal-fp32-dk128-tq3": ("decode_attention_ragged", B, 3, 128, torch.float32, True),
    "decode-ragged-bf16-dk64-tq1": ("decode_attention_ragged", B, 1, 64, torch.bfloat16, False),
    "decode-lens-bf16-dk64-tq1": ("decode_attention_lens", B, 1, 64, torch.bfloat16, False),
    "decode-lens-fp32-dk128-tq3": ("decode_attention_lens", B, 3, 128, torch.float32, False),
}.items():
    _subject(_name)(functools.partial(lambda name, args: _decode(name, *args), args=_args))

NAMES = list(SUBJECTS)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", NAMES)
def test_anchor_contiguous_run_against_float64(name):
    s = subject(name)
    views = layout_views(s, ["contig"] * len(s.names))
    want = s.expect(views)
    assert want == (FUSED if "-fused-" in name or name.startswith("decode-") else GENERIC), name     # what the subject is here for
    res, paths = run(s, views)
    assert paths == {k: want for k in s.keys}, paths
    finite(res, name)
    s.check(res)


@pytest.mark.parametrize("r", range(8))
@pytest.mark.parametrize("name", NAMES)
def test_rotation(name, r):
    s = subject(name)
    views_against_contiguous(s, al.rotation(r, len(s.names)))


@pytest.mark.parametrize("layout", ["heads_first", "window"])
@pytest.mark.parametrize("name", NAMES)
def test_uniform_layout(name, layout):
    s = subject(name)
    views_against_contiguous(s, [layout] * len(s.names))


# ---- mask / bias forms on the device
FORMS = ["()", "(Nk,)", "(N,1)", "(N,Nk)", "(1,1,N,Nk)", "(B,1,1,Nk)", "(B,1,N,1)", "(B,H,1,Nk)", "(B,H,N,1)", "(1,H,N,Nk)", "(B,H,N,Nk)",
         "(N,Nk) transposed"]
CLOSED_ROWS = (0, N - 2)                 # one in each query block


def _form(full, form):
    """the `form` slice of a (B,H,N,Nk) tensor: mostly non-contiguous views, as a caller's own slicing gives them"""
    if form == "(N,Nk) transposed":
        t = full[0, 0].t().contiguous().t()
        assert not t.is_contiguous()
        return t
    return {"()": lambda: full[0, 0, 0, 0], "(Nk,)": lambda: full[0, 0, 0], "(N,1)": lambda: full[0, 0, :, :1], "(N,Nk)": lambda: full[0, 0],
            "(1,1,N,Nk)": lambda: full[:1, :1], "(B,1,1,Nk)": lambda: full[:, :1, :1], "(B,1,N,1)": lambda: full[:, :1, :, :1],
            "(B,H,1,Nk)": lambda: full[:, :, :1], "(B,H,N,1)": lambda: full[..., :1], "(1,H,N,Nk)": lambda: full[:1],
            "(B,H,N,Nk)": lambda: full}[form]()


def _closes_rows(form):
    return form in ("(N,1)", "(B,1,N,1)", "(B,H,N,1)")


@functools.lru_cache(maxsize=None)
def _form_inputs(kind, nk, form, finite_only):
    """(the form, its materialised (B,H,N,nk) twin).  A form broadcast along the keys closes whole rows (mask) / puts them at -inf
    (bias) unless finite_only"""
    g = _gen(f"{kind}{nk}")
    if kind == "mask":
        full = torch.rand(B, H, N, nk, device="cuda", generator=g) > 0.3
        full[..., 0] = True
        closed = False
    else:
        full = torch.randn(B, H, N, nk, device="cuda", generator=g)
        closed = float("-inf")
    if _closes_rows(form) and not finite_only:
        full[:, :, list(CLOSED_ROWS), 0] = closed         # key column 0 is the one these forms keep
    src = _form(full, form)
    return src, torch.broadcast_to(src, (B, H, N, nk)).contiguous()


def _form_runs(s, call, src, full):
    views = layout_views(s, ["contig"] * len(s.names))
    want = s.expect(views)
    out = []
    for m in (src, full):
        s.call = functools.partial(call, m)
        res, paths = run(s, contiguous_copies(s, views))
        assert paths == {k: want for k in s.keys}, paths
        out.append(res)
    return out


@pytest.mark.parametrize("kind", ["mask", "bias"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["sdpa-fused-rect-bf16-dk32", "sdpa-generic-rect-bf16-dk40"])
def test_sdpa_mask_and_bias_forms(name, form, kind):
    from mop_amd import ops
    if kind == "mask" and form == "()":                  # a 0-d mask can only be all open; it must work all the same
        src, full = torch.ones((), dtype=torch.bool, device="cuda"), torch.ones(B, H, N, NK, dtype=torch.bool, device="cuda")
    else:
        src, full = _form_inputs(kind, NK, form, False)
    base = subject(name)
    s = Subject(name, base.vals, None, base.keys, base.expect, None, base.prec, dy=base.dy)
    kwn = "attn_mask" if kind == "mask" else "bias"
    got, want = _form_runs(s, lambda m, t: ops.sdpa_core(t["q"], t["k"], t["v"], **{kwn: m}), src, full)
    finite(got, f"{name} {kind} {form}")
    same(got, want, f"{name} {kind} {form}")
    if _closes_rows(form):
        rows = list(CLOSED_ROWS)
        assert bool((got["y"][:, rows] == 0).all()) and bool((got["dq"][:, rows] == 0).all())
        r = [base.vals[n].detach().double().requires_grad_(True) for n in "qkv"]
        yr = sdpa_ref64(*r, **({"mask": full} if kind == "mask" else {"bias": full}))
        (yr * base.dy.double()).sum().backward()
        _close(_np(got["y"]), _np(yr), {n: _np(got[n]) for n in ("dq", "dk", "dv")},
               {n: _np(t.grad) for n, t in zip(("dq", "dk", "dv"), r)}, False, f"{name} {kind} {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["quartet-fused-bf16-dk64", "quartet-generic-weights-bf16-dk32"])
def test_quartet_add_mask_forms(name, form):
    """finite values throughout: Quartet documents no zero row for an all -inf add_mask row"""
    from mop_amd import ops
    src, full = _form_inputs("bias", N, form, True)
    base = subject(name)
    s = Subject(name, base.vals, None, base.keys, base.expect, None, base.prec, dy=base.dy, scalars=base.scalars, outs=base.outs)
    names, nw = base.names, "attn" in base.outs
    got, want = _form_runs(s, lambda m, t: ops.quartet_core(*(t[n] for n in names), t["mix"], t["qs"], m, 1e-5, True, nw), src, full)
    finite(got, f"{name} {form}")
    same(got, want, f"{name} {form}")


@pytest.mark.parametrize("form", ["(N,1)", "(B,1,N,1)", "(B,1,1,Nk)"])
@pytest.mark.parametrize("name", ["dualpath-fused-bf16-dk64", "dualpath-generic-chain-bf16-dk40", "crossview-prior-bf16-dk40"])
def test_other_mask_callers_take_the_key_broadcast_forms(name, form):
    """the dual-path and CrossView cores hand their attn_mask to the same ops._mask_u8: a per-query mask that closes rows, and the
    common key-padding form, against the materialised tensor"""
    from mop_amd import ops
    src, full = _form_inputs("mask", N, form, False)
    base = subject(name)
    s = Subject(name, base.vals, None, base.keys, base.expect, None, base.prec, dy=base.dy, scalars=base.scalars, k_star=base.k_star)
    names = base.names
    if name.startswith("dualpath"):
        chain = 0.5 if "chain" in name else 0.0
        call = lambda m, t: ops.dualpath_core(*(t[n] for n in names), t["lg"], *GATES, chain, 0.6, 2, m)       # noqa: E731
    else:
        call = lambda m, t: ops.crossview_core(*(t[n] for n in names), t["mix"], attn_mask=m, **CV_KW)         # noqa: E731
    got, want = _form_runs(s, call, src, full)
    finite(got, f"{name} {form}")
    same(got, want, f"{name} {form}")
    if _closes_rows(form) and name.startswith("dualpath"):       # test_dualpath_fully_blocked_rows: a row with no open key is 0
        assert bool((got["y"][:, list(CLOSED_ROWS)] == 0).all())


# ---- output views through the C ABI
def _abi_sdpa(s, outs=None):
    """mopk_sdpa_fwd and mopk_sdpa_bwd as _SdpaFn launches them (sized saved / workspace, the current stream), y, dq, dk, dv going
    into `outs` (name -> view) or into fresh contiguous tensors"""
    from mop_amd import _lib as L, ops
    lib = L.lib()
    q, k, v = (s.vals[n] for n in "qkv")
    Bq, Nq, Hq, dk = q.shape
    dy = s.dy.view(Bq, Nq, Hq, dk)
    prec = L.PREC_BF16 if s.prec == "bf16" else L.PREC_FP32
    path = s.expect({n: s.vals[n] for n in "qkv"})
    outs = outs or {n: torch.empty_like(s.vals[m]) for n, m in (("y", "q"), ("dq", "q"), ("dk", "k"), ("dv", "k"))}
    assert _aligned(outs.values())
    none = (None, (0, 0, 0))
    a = ops._sdpa_args(q, k, v, outs["y"], none, none, False, prec, path, (0.0, 0))
    assert bool(lib.mopk_sdpa_fused_supported(C.byref(a))) == (path == FUSED)
    saved = ops._bytes(lib.mopk_sdpa_saved_bytes(C.byref(a)), q.device)
    ws = ops._bytes(lib.mopk_sdpa_workspace_bytes(C.byref(a)), q.device)
    a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
    ops._launch("mopk_sdpa_fwd", a)
    a = ops._sdpa_args(q, k, v, outs["y"], none, none, False, prec, path, (0.0, 0))
    a.dy = ops._v4(dy)
    a.dq, a.dk_, a.dv = ops._v4(outs["dq"]), ops._v4(outs["dk"]), ops._v4(outs["dv"])
    ws = ops._bytes(lib.mopk_sdpa_workspace_bytes(C.byref(a)), q.device)
    a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
    ops._launch("mopk_sdpa_bwd", a)
    torch.cuda.synchronize()
    return outs


SENTINEL = 0xA5


@pytest.mark.parametrize("layout", ["heads_first", "wide_rows"])
@pytest.mark.parametrize("name", ["sdpa-fused-rect-bf16-dk32", "sdpa-generic-rect-bf16-dk40"])
def test_sdpa_output_views_through_the_c_abi(name, layout):
    s = subject(name)
    want = _abi_sdpa(s)
    plain, _ = run(s, contiguous_copies(s, s.vals))                  # the Function's own launch of the same call
    same({n: want[n].view(plain[n].shape) for n in want}, plain, f"{name}: C ABI against ops.sdpa_core")
    bufs = {}
    for n, m in (("y", "q"), ("dq", "q"), ("dk", "k"), ("dv", "k")):
        storage, view = al.build(layout, torch.zeros_like(s.vals[m]))
        storage.view(torch.uint8).fill_(SENTINEL)
        bufs[n] = (storage, view)
    got = _abi_sdpa(s, {n: v for n, (_, v) in bufs.items()})
    ints = torch.int16 if s.vals["q"].element_size() == 2 else torch.int32
    for n, (storage, view) in bufs.items():
        assert torch.equal(got[n], want[n]), f"{name} {layout}: {n} differs from the contiguous run"
        inside = torch.zeros(storage.shape, dtype=torch.bool, device="cuda")
        inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)        # these two layouts have no overlap
        assert int(inside.sum()) == view.numel()
        sent = torch.empty_like(storage)
        sent.view(torch.uint8).fill_(SENTINEL)
        assert torch.equal(storage.view(ints)[~inside], sent.view(ints)[~inside]), f"{name} {layout}: {n} was written outside its view"
