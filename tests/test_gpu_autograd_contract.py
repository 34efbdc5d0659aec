"""-m gpu: the autograd contract of every differentiable core (the torch.autograd.Functions of mop_amd/ops.py and mop_amd/nn/linear.py).

The other GPU tests call `.backward()` in one way: every leaf requires grad, one forward, one backward on the default stream, a
fresh contiguous aligned gradient, nothing else in flight.  A training loop also freezes parameters, accumulates gradients, keeps
two graphs alive, checkpoints activations, runs on side streams and hands a backward whatever tensor autograd has at hand.  Each
subject below (one small case per Function and path, shapes and float64 references of tests/test_gpu_bounds.py) is run once in the
plain way -- the anchor, held to the core's float64 reference under the tolerance constants its own tests use, named at each
check -- and every scenario is then compared with that plain run BIT FOR BIT (the cores are run-to-run deterministic), together
with the ops.LAST_PATH entries the plain run left.

Scenarios: a subsets of requires_grad, b a no_grad forward before a training one, c retain_graph (twice, another gradient,
accumulation), d two graphs alive (and a third forward in between), e forms of the incoming gradient (stride 0, sliced from a wider
buffer, off a 16-byte boundary) and an input leaf off that boundary, f create_graph (the kernels have no second derivative: it
must raise), g activation checkpointing with in-kernel dropout, h a side stream, i an in-place edit of the output.

Module-level subjects also put the odd gradient of e(ii) / e(iii) where it enters the core: a hook on the output projection's
input hands the core its gradient in that form (`_GradForm`).

The one documented exception to "a subset of requires_grad does not change y": the dense gate head of _EdgewiseGeneralFn takes the
fused kernels at V > 6 only when nothing requires grad (`wants_grad`, ops.edgewise_general_core); the dense subject here has V = 3,
where the path must not depend on it, and asserts that."""
import contextlib

import numpy as np
import pytest
import torch

from attn_ref import bf16_exact, sdpa_ref64
from gpu_util import check_grads, max_abs, rel_err

pytestmark = pytest.mark.gpu

TOL_BF16, GTOL_BF16 = 1e-2, 3e-2                # test_gpu_edgewise.py (bf16-MFMA arithmetic)
TOL_FP32, GTOL_FP32 = 1e-4, 1e-3                # test_gpu_bounds.test_edgewise_generic_path (exact fp32 arithmetic)
YTOL, GTOL, GFLOOR = 1e-2, 1.5e-2, 1e-2         # test_gpu_attn_edges.py
FUSED, GENERIC = 2, 1


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    assert (FUSED, GENERIC) == (mop_amd._lib.PATH_FUSED, mop_amd._lib.PATH_GENERIC)
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")
    ops.set_save_chain_state(True)


# ------------------------------------------------------------------------------------------------ a case and the ways to run it
class Case:
    """one set of inputs of a subject.  leaves: name -> GPU tensor (values only); acts: the names that are activations, the rest are
    parameters; fn(dict of leaves) -> output tensor(s); dys: one gradient per output; outs: the outputs' names in a result; gnames:
    leaf -> the name of its gradient in a result; proj: the module whose input is the core's output (module-level subjects)"""

    def __init__(self, leaves, acts, fn, dys, gnames, outs=("y",), proj=None):
        self.leaves, self.acts, self.fn, self.dys, self.gnames, self.outs, self.proj = leaves, tuple(acts), fn, tuple(dys), gnames, outs, proj


class Subject:
    """name; build(variant) -> Case ("A": the anchor, "B": other inputs with another N / T); setup(): precision, path and chain
    switches, called before every run; paths: the LAST_PATH keys the subject sets, want: the path the issue names for it (None: as
    the shape selects); check(res, y_only): the float64 reference at the core's own tolerance; function: the Function's name;
    kernel: backed by HIP kernels; inplace: what an in-place edit of y must give ("error": the backward reads y; "equal"); core_level:
    the leaves are the core's own inputs (an unaligned leaf then reaches the kernels' support check); unaligned: LAST_PATH after a
    run on unaligned input leaves (None: the plain run's)"""

    def __init__(self, name, build, setup, paths, want, check, function, kernel=True, inplace="equal", core_level=False, has_params=True,
                 unaligned=None, e4=None):
        self.name, self._build, self.setup, self.paths, self.want, self.check = name, build, setup, tuple(paths), want, check
        self.function, self.kernel, self.inplace, self.core_level, self.has_params = function, kernel, inplace, core_level, has_params
        self.unaligned, self.e4 = unaligned, e4
        self._cases, self._plain = {}, {}

    def case(self, variant="A") -> Case:
        if variant not in self._cases:
            self.setup()
            self._cases[variant] = self._build(variant)
        return self._cases[variant]

    def plain(self, variant="A", dys=None, key=None):
        """the plain run (all leaves require grad, one forward, one backward, fresh contiguous aligned gradients), made once"""
        k = (variant, key)
        if k not in self._plain:
            self._plain[k] = run(self, self.case(variant), dys=dys)[:2]
        return self._plain[k]

    def __repr__(self):
        return self.name


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def fresh(case, rg=None, remap=None):
    """new leaves with the case's values; rg: the names that require grad (None: all)"""
    t = {}
    for k, v in case.leaves.items():
        v = remap(k, v) if remap is not None else v.detach().clone()
        t[k] = v.requires_grad_(rg is None or k in rg)
    return t


def paths_now(subj, suffix=None):
    from mop_amd import ops
    return {k: ops.LAST_PATH.get(k) for k in subj.paths if suffix is None or k.endswith(suffix)}


def collect(case, ys, t):
    res = {n: y.detach() for n, y in zip(case.outs, ys)}
    res.update({case.gnames[k]: v.grad for k, v in t.items() if v.grad is not None})
    return res


def run(subj, case, rg=None, dys=None, remap=None):
    """forward and backward on fresh leaves -> (result {name: tensor}, LAST_PATH entries, leaves)"""
    subj.setup()
    t = fresh(case, rg, remap)
    ys = _tuple(case.fn(t))
    torch.autograd.backward(ys, case.dys if dys is None else dys)
    torch.cuda.synchronize()
    return collect(case, ys, t), paths_now(subj), t


def same(got, want, what, names=None):
    """bit for bit, dtype included"""
    names = set(want) if names is None else set(names)
    assert names <= set(got), f"{what}: missing {sorted(names - set(got))}"
    for n in sorted(names):
        g, w = got[n], want[n]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {n} is {g.dtype} {tuple(g.shape)}, the plain run's {w.dtype} {tuple(w.shape)}"
        assert torch.equal(g, w), (f"{what}: {n} differs from the plain run in {int((g != w).sum())} value(s), "
                                   f"max |diff| {float((g.double() - w.double()).abs().max()):.3e}")


def off_boundary(t):
    """t's values in a contiguous tensor whose first element is one element past a 16-byte boundary"""
    n = t.numel()
    u = torch.empty(n + 1, dtype=t.dtype, device=t.device)[1:1 + n].view(t.shape)
    u.copy_(t.detach())
    assert u.is_contiguous() and u.data_ptr() % 16 != 0
    return u


def sliced(t):
    """t's values as the first columns of a wider buffer: not contiguous"""
    u = torch.empty(*t.shape[:-1], t.shape[-1] + 8, dtype=t.dtype, device=t.device)[..., :t.shape[-1]]
    u.copy_(t.detach())
    assert not u.is_contiguous()
    return u


class _GradForm(torch.autograd.Function):
    """identity whose gradient goes on in the given form (the same values)"""

    @staticmethod
    def forward(ctx, t, form):
        ctx.form = form
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.form(g), None


@contextlib.contextmanager
def core_gradient_as(case, form):
    """module-level subjects: the gradient that enters the core (through the output projection's input) takes `form`"""
    if case.proj is None:
        yield
        return
    h = case.proj.register_forward_pre_hook(lambda mod, inp: (_GradForm.apply(inp[0], form),))
    try:
        yield
    finally:
        h.remove()


def graph_nodes(ys):
    seen, todo = set(), [y.grad_fn for y in ys if y.grad_fn is not None]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        todo.extend(f for f, _ in n.next_functions)
    return {type(n).__name__ for n in seen}


# ------------------------------------------------------------------------------------------------ references
_REF = {}


def _cached(key, fn):
    """float64 references are computed once per subject and never modified"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _f(t):
    return t.detach().float().cpu().numpy()


def _np(t):
    return t.detach().double().cpu().numpy()


def _hp(t):
    return np.transpose(_np(t), (0, 2, 1, 3))


def _rb(t):
    return torch.as_tensor(t).to(torch.bfloat16).double().numpy()


def _yerr(y, yr):
    return max_abs(y, yr) / max(float(np.abs(yr).max()), 1e-30)


def _attn_check(make, scalars_tol=None):
    """test_gpu_attn_edges._assert_close: y max-abs / max|y_ref| <= YTOL, gradients GTOL of max(max|ref|, GFLOOR x the largest)"""
    def check(res, y_only=False):
        from test_gpu_attn_edges import _assert_close
        yr, ref, scalars = make()
        if y_only:
            ey = _yerr(_np(res["y"]), yr)
            assert ey <= YTOL, f"y {ey:.3e}"
            return
        _assert_close(_np(res["y"]), yr, {n: _np(res[n]) for n in ref}, ref, "plain run")
        for n, want in scalars.items():       # test_quartet_dropout_matches_the_oracle_under_the_same_mask
            assert abs(float(res[n]) - want) <= 5e-2 * max(abs(want), 1e-3), (n, float(res[n]), want)
    return check


# ------------------------------------------------------------------------------------------------ module-level subjects
def _module_case(m, x, w, proj="proj", patch=None, **fk):
    """leaves: x and every parameter; the module is called functionally on them.  patch: (name, value) set on mop_amd.ops for the call"""
    from mop_amd import ops
    from torch.func import functional_call
    params = {k: p.detach() for k, p in m.named_parameters()}

    def fn(t):
        real = getattr(ops, patch[0]) if patch else None
        if patch:
            setattr(ops, *patch)
        try:
            return functional_call(m, {k: t[k] for k in params}, (t["x"],), fk)
        finally:
            if patch:
                setattr(ops, patch[0], real)
    return Case({"x": x, **params}, ("x",), fn, (w,), {"x": "dx", **{k: k for k in params}}, proj=getattr(m, proj))


def _prec(prec, path="auto", save_chain=True):
    def setup():
        import mop_amd
        from mop_amd import ops
        mop_amd.set_precision(prec)
        ops.set_path(path)
        ops.set_save_chain_state(save_chain)
    return setup


def _param_grads(res):
    return {k: _f(v) for k, v in res.items() if k not in ("y", "dx")}


def _check_param_grads(grads, gref, gtol, **kw):
    for k in set(grads) - set(gref):
        assert not grads[k].any(), f"{k}: no reference gradient, and the module's is not zero"
    check_grads({k: grads[k] for k in gref}, gref, gtol, **kw)


def _ew_ref(key, m, x, w, H, V, io_bf16, dil=None, noise=True):
    """oracle.edgewise in float64 on the inputs as given (out, dx, grads, bf16 noise per tensor) and on the inputs rounded to
    bfloat16 as the kernels read them (test_gpu_bounds._ew_oracle)"""
    from gpu_util import oracle_bf16_noise
    from oracle import edgewise as oe

    def make():
        params = {k: v.detach().cpu().double().numpy() for k, v in m.state_dict().items()}
        kw = dict(lens_dilations=dil) if dil is not None else {}
        fwd = lambda xx, pp, *a: oe.module_fwd(xx, pp, *a, **kw)     # noqa: E731
        x64, w64 = x.double().numpy(), w.double().numpy()
        out, cache = fwd(x64, params, H, V, True, 0.5)
        dx, g = oe.module_bwd(w64, cache)
        nz = oracle_bf16_noise(fwd, oe.module_bwd, x64, w64, params, H, V, True, 0.5) if noise else None
        rounded = None
        if io_bf16:
            yr, cb = fwd(_rb(x), {k: _rb(v) for k, v in params.items()}, H, V, True, 0.5)
            rounded = (yr, *oe.module_bwd(_rb(w), cb))
        return out, dx, g, nz, rounded
    return lambda: _cached(key, make)


def _ew_check_bf16(ref, io_bf16):
    """bf16-MFMA arithmetic (test_gpu_bounds._ew_check_bf16_arith): y TOL_BF16 of max(1, |y|max), dx GTOL_BF16; bfloat16 tensors
    against the oracle on the rounded inputs; parameter gradients GTOL_BF16 under the oracle's own bf16 noise"""
    def check(res, y_only=False):
        out, dx, g, nz, rounded = ref()
        yo, dxo = (rounded[0], rounded[1]) if io_bf16 else (out, dx)
        ey = max_abs(_f(res["y"]), yo)
        assert ey <= TOL_BF16 * max(1.0, float(np.abs(yo).max())), f"y {ey:.3e}"
        if y_only:
            return
        ed = rel_err(_f(res["dx"]), dxo)
        assert ed <= GTOL_BF16, f"dx {ed:.3e}"
        _check_param_grads(_param_grads(res), g, GTOL_BF16, d=nz)
    return check


def _ew_check_fp32(ref, dense):
    """exact fp32 arithmetic (test_edgewise_generic_path): y TOL_FP32, gradients GTOL_FP32"""
    def check(res, y_only=False):
        out, dx, g = ref()[:3]
        assert max_abs(_f(res["y"]), out) <= TOL_FP32, f"y {max_abs(_f(res['y']), out):.3e}"
        if y_only:
            return
        assert rel_err(_f(res["dx"]), dx) <= GTOL_FP32, f"dx {rel_err(_f(res['dx']), dx):.3e}"
        grads = _param_grads(res)
        if dense:
            return _check_param_grads(grads, g, GTOL_FP32, floor=1e-3)
        assert set(grads) == set(g)
        for k in g:
            assert rel_err(grads[k].reshape(g[k].shape), g[k]) <= GTOL_FP32, k
    return check


def _xw(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)


def _ew_lowrank(name, prec, path, save_chain, io, route, want, function):
    """EdgewiseMSA(share_qkv, low-rank head) at (2, 65, 96, 3, 4, 2) (test_edgewise_lowrank_fused); route "core": the layer's tensor
    expressions feed ops.edgewise_lowrank_core (_EdgewiseLowrankFn), "shared": ops.edgewise_lowrank_core_shared (_EdgewiseSharedFn)"""
    B, N, D, H, V, r = (2, 65, 96, 3, 4, 2) if route == "core" else (2, 33, 128, 2, 2, 3)
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    box = {}

    def module():
        if "m" not in box:
            from test_gpu_edgewise import _mk
            box["cpu"] = _mk(D, H, V, r, seed=B * 1000 + N)
            box["x"], box["w"] = _xw(B, N, D, N)
            import copy
            box["m"] = copy.deepcopy(box["cpu"]).cuda().to(dt).eval()
        return box["m"]

    def build(variant):
        m = module()
        x, w = (box["x"], box["w"]) if variant == "A" else _xw(B, 33 if N > 64 else 70, D, 5)
        patch = ("edgewise_shared_params_supported", lambda *a: False) if route == "core" else None
        return _module_case(m, x.cuda().to(dt), w.cuda().to(dt), patch=patch)

    def ref():
        module()
        return _ew_ref((name, "ref"), box["cpu"], box["x"], box["w"], H, V, io == "bf16", noise=prec == "bf16")()
    check = _ew_check_bf16(ref, io == "bf16") if prec == "bf16" else _ew_check_fp32(ref, False)
    return Subject(name, build, _prec(prec, path, save_chain), ("edgewise_fwd", "edgewise_bwd"), want, check, function)


def _ew_lens():
    """the (1, 8, 64, 4, 2, 1, (1, 9)) lens-bank case of test_edgewise_lowrank_lens_bank_fused: ops.edgewise_lowrank_core with the S lens
    bank as extra mean-feature channels.  The fused parameter gradients are bounded against the generic path's error, as there."""
    B, N, D, H, V, r, dil = 1, 8, 64, 4, 2, 1, (1, 9)
    box = {}

    def module():
        if "m" not in box:
            import copy
            from mop_amd.nn import EdgewiseMSA
            torch.manual_seed(N * 11 + V)
            m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="lowrank", gate_rank=r, gate_init="mix5", use_lens_bank=True, lens_dilations=dil)
            with torch.no_grad():
                for n_, p in m.named_parameters():
                    if n_.endswith("_scale"):
                        p.add_(0.1 * torch.randn_like(p))
                    if "proj.weight" in n_ and "edge_head" in n_:
                        p.mul_(3.0)
                m.chain_value_logit.fill_(-0.5)
            box["cpu"], box["x"], box["w"] = m, torch.randn(B, N, D), torch.randn(B, N, D)
            box["m"] = copy.deepcopy(m).cuda().to(torch.bfloat16).eval()
        return box["m"]

    def build(variant):
        m = module()
        x, w = (box["x"], box["w"]) if variant == "A" else _xw(B, 37, D, 5)
        return _module_case(m, x.cuda().to(torch.bfloat16), w.cuda().to(torch.bfloat16))

    def make():
        from oracle import edgewise as oe
        params = {k: _rb(v) for k, v in box["cpu"].state_dict().items()}
        out, cache = oe.module_fwd(_rb(box["x"]), params, H, V, True, 0.5, lens_dilations=dil)
        return (out, *oe.module_bwd(_rb(box["w"]), cache))

    def check(res, y_only=False):
        from mop_amd import ops
        module()
        out, dx_ref, g_ref = _cached(("ew-lens", "ref"), make)
        assert max_abs(_f(res["y"]), out) <= TOL_BF16, f"y {max_abs(_f(res['y']), out):.3e}"
        if y_only:
            return
        assert rel_err(_f(res["dx"]), dx_ref) <= GTOL_BF16, f"dx {rel_err(_f(res['dx']), dx_ref):.3e}"
        ops.set_path("generic")                     # the bound of the fused gradients is stated against the generic path's error
        try:
            gen, paths, _ = run(subj, subj.case("A"))
            assert paths["edgewise_bwd"] == GENERIC
        finally:
            ops.set_path("auto")
        grads, gg = _param_grads(res), _param_grads(gen)
        assert set(grads) == set(g_ref)
        for k in g_ref:
            e, eg = rel_err(grads[k].reshape(g_ref[k].shape), g_ref[k]), rel_err(gg[k].reshape(g_ref[k].shape), g_ref[k])
            assert e <= max(GTOL_BF16, 2.0 * eg), f"{k}: fused {e:.3e} generic {eg:.3e}"

    def setup():
        import mop_amd
        from mop_amd import ops
        mop_amd.set_precision("bf16")
        ops.set_save_chain_state(True)          # the path stays as the caller set it: check() switches to the generic one
    subj = Subject("ew-lowrank-lens-bank", build, setup, ("edgewise_fwd", "edgewise_bwd"), FUSED, check, "_EdgewiseLowrankFn")
    return subj


def _ew_dense(name, k3):
    """_EdgewiseGeneralFn: the dense head at (3, 50, 128, 2, 3) inside the fused kernels (test_edgewise_dense_head_fused), and with the
    3x3 mid convolution at (2, 33, 64, 1, 3) on the generic path in exact fp32 arithmetic (test_edgewise_generic_path dense_k3)"""
    B, N, D, H, V = (2, 33, 64, 1, 3) if k3 else (3, 50, 128, 2, 3)
    box = {}

    def module():
        if "m" not in box:
            import copy
            from mop_amd.nn import EdgewiseMSA
            torch.manual_seed(N if k3 else N * 11 + V)
            m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="dense", use_k3=k3, gate_init="and")
            with torch.no_grad():
                for n_, p in m.named_parameters():
                    if n_.endswith("_scale"):
                        p.add_(0.1 * torch.randn_like(p))
                    elif n_.endswith("conv2.bias"):
                        p.copy_((0.5 if k3 else 0.7) * torch.randn_like(p))
                    elif not k3 and ("conv1" in n_ or "conv2" in n_):
                        p.mul_(1.5)
                m.chain_value_logit.fill_(-0.5)
            box["cpu"] = m
            box["x"], box["w"] = (torch.randn(B, N, D), torch.randn(B, N, D)) if k3 else _xw(B, N, D, N)
            box["m"] = copy.deepcopy(m).cuda().eval()
        return box["m"]

    def build(variant):
        m = module()
        x, w = (box["x"], box["w"]) if variant == "A" else _xw(B, 17 if k3 else 70, D, 5)
        return _module_case(m, x.cuda(), w.cuda())

    def ref():
        module()
        return _ew_ref((name, "ref"), box["cpu"], box["x"], box["w"], H, V, False, noise=not k3)()
    if k3:
        return Subject(name, build, _prec("fp32", "generic"), ("edgewise_fwd", "edgewise_bwd"), GENERIC, _ew_check_fp32(ref, True), "_EdgewiseGeneralFn")
    return Subject(name, build, _prec("bf16"), ("edgewise_fwd", "edgewise_bwd"), FUSED, _ew_check_bf16(ref, False), "_EdgewiseGeneralFn")


def _crossview_module(name, cues):
    """CrossViewMixerMSA(128, 2), B = 2, N = 150 (test_crossview_mixer): with transpose cues the generic kernels (_CrossViewFn),
    without them the folded route on the fused two-score kernels from the packed projections (_CrossViewFoldedFn); bounds of
    test_gpu_siblings.test_crossview_mixer for bf16 arithmetic (y TOL_BF16, gradients GTOL_BF16 with a floor of 1e-2 x the largest)"""
    B, N, D, H = 2, 150, 128, 2
    box = {}

    def module():
        if "m" not in box:
            import copy
            from mop_amd.nn import CrossViewMixerMSA
            torch.manual_seed(5)
            m = CrossViewMixerMSA(D, H, use_transpose_cues=cues, t1=0.3, t2=-0.2)
            with torch.no_grad():
                m.mix.add_(0.3 * torch.randn(2, 2))
            box["cpu"], box["x"], box["w"] = m, torch.randn(B, N, D), torch.randn(B, N, D)
            box["m"] = copy.deepcopy(m).cuda().eval()
        return box["m"]

    def build(variant):
        m = module()
        x, w = (box["x"], box["w"]) if variant == "A" else _xw(B, 60, D, 5)
        return _module_case(m, x.cuda(), w.cuda())

    def make():
        from oracle import crossview as oc
        params = {k: v.detach().double().numpy() for k, v in box["cpu"].state_dict().items()}
        out, c = oc.module_fwd(box["x"].double().numpy(), params, H, None, cues, 0.3, -0.2)
        return (out, *oc.module_bwd(box["w"].double().numpy(), c))

    def check(res, y_only=False):
        module()
        out, dx_ref, g_ref = _cached((name, "ref"), make)
        assert max_abs(_f(res["y"]), out) <= TOL_BF16, f"y {max_abs(_f(res['y']), out):.3e}"
        if y_only:
            return
        assert rel_err(_f(res["dx"]), dx_ref) <= GTOL_BF16, f"dx {rel_err(_f(res['dx']), dx_ref):.3e}"
        _check_param_grads(_param_grads(res), g_ref, GTOL_BF16, floor=1e-2)
    return Subject(name, build, _prec("bf16"), ("crossview_fwd",), GENERIC if cues else FUSED, check,
                   "_CrossViewFn" if cues else "_CrossViewFoldedFn", inplace="equal")


# ------------------------------------------------------------------------------------------------ core-level subjects
def _bf(shape, g, dt):
    return bf16_exact(torch.randn(*shape, device="cuda", generator=g)).to(dt)


def _core_gnames(names, **special):
    return {n: special.get(n, "d" + n) for n in names}


def _sdpa(name, kind, N, Nk, dk, io, NB):
    """ops.sdpa_core in bf16 arithmetic against attn_ref.sdpa_ref64 (test_gpu_bounds.test_sdpa); kind: "packed-causal", "mask+bias"
    (a detached bias: the cores compute no gradient for it), "dropout" (p = 0.2 under an explicit seed, against oracle.sdpa under the
    kernels' own keep mask: test_sdpa_dropout_matches_the_oracle_under_the_same_mask, y TOL_BF16 of max(1, |y|max), gradients GTOL_BF16)"""
    B, H = 2, 2
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    seed, p = 0xC0FFEE1234567, 0.2

    def build(variant):
        from mop_amd import ops
        n, nk = (N, Nk) if variant == "A" else NB
        g = torch.Generator(device="cuda").manual_seed(7 * n + nk + dk)
        q, k, v = (_bf((B, m_, H, dk), g, dt) for m_ in (n, nk, nk))
        dy = _bf((B, n, H * dk), g, dt)
        if kind == "packed-causal":
            return Case({"qkv": torch.stack([q, k, v], 2)}, ("qkv",), lambda t: ops.sdpa_core(t["qkv"], causal=True), (dy,), {"qkv": "dqkv"})
        kw = {}
        if kind == "mask+bias":
            mask = torch.rand(B, 1, n, nk, device="cuda", generator=g) > 0.3
            mask[..., 0] = True                                               # no fully blocked row
            kw = dict(attn_mask=mask, bias=0.5 * torch.randn(1, H, n, nk, device="cuda", generator=g))
        if kind == "dropout":
            kw = dict(dropout_p=p, seed=seed)
        case = Case(dict(q=q, k=k, v=v), ("q", "k", "v"), lambda t: ops.sdpa_core(t["q"], t["k"], t["v"], **kw), (dy,), _core_gnames("qkv"))
        case.kw = kw
        return case

    def make():
        from mop_amd import ops
        from oracle import sdpa as osd
        c = subj.case("A")
        dy = c.dys[0]
        if kind == "packed-causal":
            q, k, v = c.leaves["qkv"].unbind(2)
        else:
            q, k, v = c.leaves["q"], c.leaves["k"], c.leaves["v"]
        if kind == "dropout":
            drop = ops.dropout_keep_mask(seed, p, B, H, N, Nk).numpy().astype(np.float64) / (1.0 - p)
            yr, cc = osd.core_fwd(_hp(q), _hp(k), _hp(v), None, None, drop)
            gr = osd.core_bwd(_hp(dy.view(B, N, H, dk)), cc)
            return np.transpose(yr, (0, 2, 1, 3)).reshape(B, N, H * dk), {n: np.transpose(gr[n], (0, 2, 1, 3)) for n in ("dq", "dk", "dv")}, {}
        r = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
        kw = getattr(c, "kw", {})
        yr = sdpa_ref64(*r, mask=kw.get("attn_mask"), bias=kw.get("bias"), causal=kind == "packed-causal")
        (yr * dy.double()).sum().backward()
        return yr.detach().cpu().numpy(), {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}, {}

    def split(res):
        if "dqkv" in res:
            d = res["dqkv"]
            return dict(res, dq=d[:, :, 0], dk=d[:, :, 1], dv=d[:, :, 2])
        return res
    ref = lambda: _cached((name, "ref"), make)     # noqa: E731
    inner = _attn_check(ref)

    def check(res, y_only=False):
        if kind != "dropout":
            return inner(split(res), y_only)
        yr, gref, _ = ref()
        ey = max_abs(_np(res["y"]), yr)
        assert ey <= TOL_BF16 * max(1.0, float(np.abs(yr).max())), ey
        if not y_only:
            for n in gref:
                assert rel_err(_np(res[n]), gref[n]) <= GTOL_BF16, (n, rel_err(_np(res[n]), gref[n]))
    subj = Subject(name, build, _prec("bf16"), ("sdpa_fwd", "sdpa_bwd"), FUSED if kind == "packed-causal" else None, check, "_SdpaFn",
                   inplace="error", core_level=True, has_params=False, unaligned=dict(sdpa_fwd=GENERIC, sdpa_bwd=GENERIC))
    return subj


def _sdpa_lens():
    """q_lens / kv_lens (test_sdpa_with_lengths: lengths 0, 1, inside a tile and full; naive_lens_attention in float64, 2e-2 of
    max(1, |ref|max) for bf16, the bound of test_sdpa_lens_matches_float64)"""
    H, dk, dt = 2, 64, torch.bfloat16

    def build(variant):
        from mop_amd import ops
        B, n, nk = (4, 130, 200) if variant == "A" else (4, 64, 100)
        g = torch.Generator(device="cuda").manual_seed(11 + n)
        q, k, v = (_bf((B, m_, H, dk), g, dt) for m_ in (n, nk, nk))
        dy = _bf((B, n, H * dk), g, dt)
        kl = torch.tensor([0, 1, 64, nk], dtype=torch.int32, device="cuda")
        ql = torch.tensor([n, 1, 0, 65 if n > 65 else 33], dtype=torch.int32, device="cuda")
        case = Case(dict(q=q, k=k, v=v), ("q", "k", "v"), lambda t: ops.sdpa_core(t["q"], t["k"], t["v"], q_lens=ql, kv_lens=kl), (dy,),
                    _core_gnames("qkv"))
        case.lens = (ql, kl)
        return case

    def make():
        from test_whisper_audio_lens_cpu import naive_lens_attention
        c = subj.case("A")
        q64, k64, v64 = (c.leaves[n].detach().cpu().double().requires_grad_(True) for n in "qkv")
        ref = naive_lens_attention(q64, k64, v64, c.lens[0].cpu(), c.lens[1].cpu(), False)
        rq, rk, rv = torch.autograd.grad(ref, (q64, k64, v64), c.dys[0].cpu().double().reshape(ref.shape))
        return dict(y=ref.detach(), dq=rq, dk=rk, dv=rv)

    def check(res, y_only=False):
        ref = _cached(("sdpa-lens", "ref"), make)
        for name in ("y",) if y_only else ("y", "dq", "dk", "dv"):
            want = ref[name]
            e = float((res[name].detach().cpu().double().reshape(want.shape) - want).abs().max() / max(1.0, float(want.abs().max())))
            assert e <= 2e-2, (name, e)
    subj = Subject("sdpa-lens", build, _prec("bf16"), ("sdpa_fwd", "sdpa_bwd"), None, check, "_SdpaLensFn", inplace="error", core_level=True,
                   has_params=False, unaligned=dict(sdpa_fwd=GENERIC, sdpa_bwd=GENERIC))
    return subj


def _dualpath(name, cfg, chain, want):
    """ops.dualpath_core (cases of test_gpu_bounds.test_dualpath) against oracle.multihop in float64 under test_gpu_attn_edges' bound;
    chain: the chain gate, which only the generic kernels take"""
    B, N, H, dk, hops, gates, causal, io = cfg
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    names = ("q1", "k1", "v1", "q2", "k2", "v2")

    def build(variant):
        from mop_amd import ops
        n = N if variant == "A" else (64 if N > 64 else 130)
        g = torch.Generator(device="cuda").manual_seed(n + hops)
        leaves = {k: _bf((B, n, H, dk), g, dt) for k in names}
        leaves["lg"] = torch.tensor(-0.5, device="cuda")
        dy = _bf((B, n, H * dk), g, dt)
        fn = lambda t: ops.dualpath_core(*(t[k] for k in names), t["lg"], *gates, chain, 0.6, hops, None, causal=causal)   # noqa: E731
        return Case(leaves, names, fn, (dy,), _core_gnames(names + ("lg",), lg="dlogit"))

    def make():
        from oracle import multihop as om
        c = subj.case("A")
        blocked = np.broadcast_to(~np.tril(np.ones((N, N), dtype=bool)), (B, 1, N, N)) if causal else None
        yo, cc = om.core_fwd(*(_hp(c.leaves[k]) for k in names), dict(and_=gates[0], or_=gates[1], not_=gates[2], chain=chain), 0.6, hops, -0.5, blocked)
        go = om.core_bwd(_hp(c.dys[0].view(B, N, H, dk)), cc)
        return np.transpose(yo, (0, 2, 1, 3)).reshape(B, N, -1), {"d" + k: np.transpose(go["d" + k], (0, 2, 1, 3)) for k in names}, {}
    subj = Subject(name, build, _prec("bf16"), ("dualpath_fwd", "dualpath_bwd"), want, _attn_check(lambda: _cached((name, "ref"), make)),
                   "_DualPathFn", inplace="error", core_level=True, unaligned=dict(dualpath_fwd=GENERIC, dualpath_bwd=GENERIC))
    return subj


def _crossview_core():
    """ops.crossview_core without cues or prior: the 2x2 mix folded into two mixed key tensors by torch ops, the core the fused
    two-score kernels (_DualPathFn, hops = 0); oracle.crossview's core in float64 under the bounds of the module-level subjects"""
    B, H, dk = 2, 2, 64
    names = ("q1", "k1", "v1", "q2", "k2")

    def build(variant):
        from mop_amd import ops
        n = 70 if variant == "A" else 33
        g = torch.Generator(device="cuda").manual_seed(n)
        leaves = {k: _bf((B, n, H, dk), g, torch.float32) for k in names}
        leaves["mix"] = torch.eye(2, device="cuda") + 0.3 * torch.randn(2, 2, device="cuda", generator=g)
        dy = _bf((B, n, H * dk), g, torch.float32)
        return Case(leaves, names, lambda t: ops.crossview_core(*(t[k] for k in names), t["mix"]), (dy,), _core_gnames(names + ("mix",)))

    def make():
        from oracle import crossview as oc
        c = subj.case("A")
        n = c.leaves["q1"].shape[1]
        yo, cc = oc.core_fwd(*(_hp(c.leaves[k]) for k in names), _np(c.leaves["mix"]))
        go = oc.core_bwd(_hp(c.dys[0].view(B, n, H, dk)), cc)
        ref = {"d" + k: np.transpose(go["d" + k], (0, 2, 1, 3)) for k in names}
        ref["dmix"] = go["dmix"]
        return np.transpose(yo, (0, 2, 1, 3)).reshape(B, n, -1), ref

    def check(res, y_only=False):
        yr, ref = _cached(("crossview-core", "ref"), make)
        assert max_abs(_f(res["y"]), yr) <= TOL_BF16, f"y {max_abs(_f(res['y']), yr):.3e}"
        if not y_only:
            check_grads({k: _f(res[k]) for k in ref}, ref, GTOL_BF16, floor=1e-2)
    subj = Subject("crossview-core-fold", build, _prec("bf16"), ("crossview_fwd", "dualpath_fwd", "dualpath_bwd"), FUSED, check, "_DualPathFn",
                   inplace="error", core_level=True, unaligned=dict(crossview_fwd=GENERIC))
    return subj


def _quartet(name, cfg, path, want):
    """ops.quartet_core (test_gpu_bounds.test_quartet) against oracle.quartet in float64 under test_gpu_attn_edges' bound"""
    B, T, H, dh, uq, io = cfg
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    names = ("q", "k", "v", "q2", "k2")[:5 if uq else 3]

    def build(variant):
        from mop_amd import ops
        n = T if variant == "A" else 64
        g = torch.Generator(device="cuda").manual_seed(n)
        leaves = {k: _bf((B, n, H, dh), g, dt) for k in names}
        if uq:
            leaves.update(mix=torch.tensor([0.3], device="cuda"), qs=torch.tensor([0.8], device="cuda"))
        dy = _bf((B, n, H * dh), g, dt)
        fn = lambda t: ops.quartet_core(t["q"], t["k"], t["v"], t.get("q2"), t.get("k2"), t.get("mix"), t.get("qs"), None, 1e-5, uq)   # noqa: E731
        return Case(leaves, names, fn, (dy,), _core_gnames(tuple(leaves), mix="dmixture", qs="dquartet_scale"))

    def make():
        from oracle import quartet as oq
        c = subj.case("A")
        base = [_hp(c.leaves[k]) for k in names] + ([] if uq else [None, None])
        yo, cc = oq.core_fwd(*base, 0.3, 0.8, 1e-5, uq, True, None)
        go = oq.core_bwd(_hp(c.dys[0].view(B, T, H, dh)), cc)
        return (np.transpose(yo, (0, 2, 1, 3)).reshape(B, T, -1), {"d" + k: np.transpose(go["d" + k], (0, 2, 1, 3)) for k in names},
                {k: float(go[k]) for k in ("dmixture", "dquartet_scale")} if uq else {})
    subj = Subject(name, build, _prec("bf16", path), ("quartet_fwd",), want, _attn_check(lambda: _cached((name, "ref"), make)), "_QuartetFn",
                   inplace="error", core_level=True, has_params=uq, unaligned=dict(quartet_fwd=GENERIC))
    return subj


def _layernorm(name, rows, dim, dt, residual):
    """ops.layernorm / ops.layernorm_residual; reference and bounds of test_layernorm_forward_backward_vs_torch"""
    def build(variant):
        from mop_amd import ops
        n = rows if variant == "A" else rows + 40
        gen = torch.Generator().manual_seed(n * 131 + dim)
        x = (torch.randn(n, dim, generator=gen) * 1.7 + 0.3).to(dt).cuda()
        g = (1.0 + 0.2 * torch.randn(dim, generator=gen)).to(dt).cuda()
        b = (0.1 * torch.randn(dim, generator=gen)).to(dt).cuda()
        dy, dres = torch.randn(n, dim, generator=gen).to(dt).cuda(), torch.randn(n, dim, generator=gen).to(dt).cuda()
        gn = dict(x="dx", g="dgamma", b="dbeta")
        if residual:
            return Case(dict(x=x, g=g, b=b), ("x",), lambda t: ops.layernorm_residual(t["x"], t["g"], t["b"], 1e-5, dt), (dres, dy), gn, outs=("xres", "y"))
        return Case(dict(x=x, g=g, b=b), ("x",), lambda t: ops.layernorm(t["x"], t["g"], t["b"], 1e-5, dt), (dy,), gn)

    def check(res, y_only=False):
        from test_gpu_layernorm import _ref
        c = subj.case("A")
        dy = c.dys[-1]
        dres = c.dys[0] if residual else torch.zeros_like(dy)
        yr, dxr, dgr, dbr = _cached((name, "ref"), lambda: _ref(*(c.leaves[k].float().cpu() for k in "xgb"), 1e-5, dy.float().cpu(), dres.float().cpu()))
        ytol = 1e-5 if dt == torch.float32 else 1.6e-2
        assert (res["y"].float().cpu().double() - yr).abs().max().item() <= ytol * max(1.0, yr.abs().max().item())
        if y_only:
            return
        gt = 2e-5 if dt == torch.float32 else 8e-3
        for n, ref in (("dx", dxr), ("dgamma", dgr), ("dbeta", dbr)):
            err = (res[n].float().cpu().double() - ref).abs().max().item() / max(1e-6, ref.abs().max().item())
            assert err <= gt, f"{n} {err:.2e}"

    def e4(case):
        """an x off the 16-byte boundary is outside what the kernels take: the predicate says so (the caller then keeps torch's
        LayerNorm, mop_amd/nn), and a direct call is refused on the host, before any launch"""
        from mop_amd import ops
        x = off_boundary(case.leaves["x"])
        assert ops.layernorm_supported(case.leaves["x"], case.leaves["g"]) and not ops.layernorm_supported(x, case.leaves["g"])
        with pytest.raises(RuntimeError, match="mopk_layernorm_fwd"):
            case.fn(dict(case.leaves, x=x))
    subj = Subject(name, build, _prec("auto"), (), None, check, "_LayerNormFn", core_level=True, e4=e4)
    return subj


def _token_gate():
    """ops.token_gate_1d, B = 3, T = 17, D = 96, float32 x with a bfloat16 a; reference and bounds of test_token_gate_op_against_float64"""
    B, D = 3, 96

    def build(variant):
        from mop_amd import ops
        from test_gpu_gpt import _inputs
        T = 17 if variant == "A" else 40
        x, a, u, dout = _inputs(B, T, D, torch.float32, torch.bfloat16, False, seed=B * 10007 + T * 31 + D)
        return Case(dict(x=x, a=a, u=u), ("x", "a"), lambda t: ops.token_gate_1d(t["x"], t["a"], t["u"]), (dout,), dict(x="dx", a="da", u="du"),
                    outs=("out",))

    def check(res, y_only=False):
        from test_gpu_gpt import _nerr, _ref64
        c = subj.case("A")
        ro, rdx, rdu = _cached(("token-gate", "ref"), lambda: _ref64(c.leaves["x"], c.leaves["a"], c.leaves["u"], c.dys[0]))
        assert res["out"].dtype == torch.float32 and _nerr(res["out"], ro) <= 1e-4
        if not y_only:
            assert _nerr(res["dx"], rdx) <= 1e-4 and _nerr(res["du"], rdu) <= 1e-4
            assert res["da"].dtype == torch.bfloat16 and _nerr(res["da"], rdx) <= 1e-2

    def e4(case):
        """token_gate_supported is the library's own query and sees the pointer: the call runs the same formula in torch ops"""
        from mop_amd import ops
        x = off_boundary(case.leaves["x"])
        assert ops.token_gate_supported(case.leaves["x"], case.leaves["a"]) and not ops.token_gate_supported(x, case.leaves["a"])
        res, _, _ = run(subj, case, remap=lambda k, v: off_boundary(v) if k == "x" else v.detach().clone())
        assert ops.LAST_PATH["token_gate_fwd"] == GENERIC
        check(res)
    subj = Subject("token-gate", build, _prec("auto"), ("token_gate_fwd", "token_gate_bwd"), FUSED, check, "_TokenGateFn", core_level=True, e4=e4)
    return subj


def _moe():
    """ops.moe_mlp at (65, 8, 32, 8) bf16 with the residual folded in (test_gpu_moe.SWEEP); reference and bounds of
    test_moe_op_sweep_vs_float64"""
    D, F_, E = 8, 32, 8
    dt = torch.bfloat16

    def build(variant):
        from mop_amd import ops
        from test_gpu_moe import _case
        M = 65 if variant == "A" else 130
        x, gw, gb, w1s, w2s, dy, res_ = _case(M, D, F_, E, False, 0 if variant == "A" else 1, dtype=dt)
        leaves = dict(x=x, res=res_.to(dt))
        leaves.update({f"w1.{e}": w.detach() for e, w in enumerate(w1s)})
        leaves.update({f"w2.{e}": w.detach() for e, w in enumerate(w2s)})
        fn = lambda t: ops.moe_mlp(t["x"], gw, gb, [t[f"w1.{e}"] for e in range(E)], [t[f"w2.{e}"] for e in range(E)], residual=t["res"])   # noqa: E731
        case = Case(leaves, ("x", "res"), fn, (dy.to(dt),), {k: {"x": "dx", "res": "dres"}.get(k, k) for k in leaves})
        case.gate = (gw, gb)
        return case

    def check(res, y_only=False, route=None):
        from mop_amd import ops
        from test_gpu_moe import _ref64
        c = subj.case("A")
        x, (gw, gb) = c.leaves["x"], c.gate
        route = ops.moe_route(x, gw, gb) if route is None else route
        y64, dx64, dw1, dw2 = _ref64(x, gw, gb, [c.leaves[f"w1.{e}"] for e in range(E)], [c.leaves[f"w2.{e}"] for e in range(E)], route,
                                     c.dys[0], c.leaves["res"])
        yv = res["y"].double().reshape(y64.shape)
        assert float((yv - y64).abs().max()) <= 2e-2 * max(1.0, float(y64.abs().max())), f"y {float((yv - y64).abs().max()):.3e}"
        if y_only:
            return
        got, ref = {"dx": res["dx"].double().reshape(dx64.shape)}, {"dx": dx64}
        for e in range(E):
            got[f"w1.{e}"], ref[f"w1.{e}"] = res[f"w1.{e}"].double(), dw1[e]
            got[f"w2.{e}"], ref[f"w2.{e}"] = res[f"w2.{e}"].double(), dw2[e]
        check_grads({k: v.cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in ref.items()}, 3e-2)
        assert torch.equal(res["dres"], c.dys[0])

    def e4(case):
        """moe_supported hands the library's query x's pointer: the call runs the reference's dense composition in torch ops, which
        routes by its own logits -- the float64 reference takes that route"""
        import torch.nn.functional as F
        from mop_amd import ops
        gw, gb = case.gate
        w1s, w2s = [case.leaves[f"w1.{e}"] for e in range(E)], [case.leaves[f"w2.{e}"] for e in range(E)]
        x = off_boundary(case.leaves["x"])
        assert ops.moe_supported(case.leaves["x"], gw, gb, w1s, w2s) and not ops.moe_supported(x, gw, gb, w1s, w2s)
        res, _, _ = run(subj, case, remap=lambda k, v: off_boundary(v) if k == "x" else v.detach().clone())
        assert ops.LAST_PATH["moe_fwd"] == GENERIC and ops.LAST_PATH["moe_bwd"] == GENERIC
        check(res, route=F.linear(case.leaves["x"], gw, gb).argmax(-1))
    subj = Subject("moe-bf16-residual", build, _prec("auto"), ("moe_fwd", "moe_bwd"), FUSED, check, "_MoeFn", inplace="error", core_level=True, e4=e4)
    return subj


def _linear(name, which):
    """mop_amd.nn.linear: residual_linear and TokenLinear (4096 rows: the batched weight-gradient GEMM) in float32 against F.linear
    in float64, rtol = atol = 1e-4, the bound of test_token_linear_matches_nn_linear_forward_and_gradients for the weight gradient"""
    n_in, n_out = 32, 24

    def build(variant):
        from mop_amd.nn.linear import TokenLinear, residual_linear
        rows = 2048 if variant == "A" else 4096
        g = torch.Generator(device="cuda").manual_seed(rows)
        x = torch.randn(2, rows, n_in, device="cuda", generator=g)
        w = torch.randn(n_out, n_in, device="cuda", generator=g) / n_in ** 0.5
        dy = torch.randn(2, rows, n_out, device="cuda", generator=g)
        if which == "residual":
            res = torch.randn(2, rows, n_out, device="cuda", generator=g)
            return Case(dict(res=res, x=x, weight=w), ("res", "x"), lambda t: residual_linear(t["res"], t["x"], t["weight"]), (dy,),
                        dict(res="dres", x="dx", weight="dweight"))
        b = torch.randn(n_out, device="cuda", generator=g)
        lin = TokenLinear(n_in, n_out, bias=True).cuda()
        fn = lambda t: torch.func.functional_call(lin, dict(weight=t["weight"], bias=t["bias"]), (t["x"],))   # noqa: E731
        return Case(dict(x=x, weight=w, bias=b), ("x",), fn, (dy,), dict(x="dx", weight="dweight", bias="dbias"))

    def check(res, y_only=False):
        import torch.nn.functional as F
        c = subj.case("A")
        t = {k: v.detach().double().requires_grad_(True) for k, v in c.leaves.items()}
        y = F.linear(t["x"], t["weight"], t.get("bias"))
        if which == "residual":
            y = y + t["res"]
        y.backward(c.dys[0].double())
        assert torch.allclose(res["y"].double(), y.detach(), rtol=1e-4, atol=1e-4)
        if not y_only:
            for k, v in t.items():
                assert torch.allclose(res[c.gnames[k]].double(), v.grad, rtol=1e-4, atol=1e-4), k
    subj = Subject(name, build, _prec("auto"), (), None, check, "_ResidualLinearFn" if which == "residual" else "_TokenLinearFn", kernel=False,
                   inplace="error", core_level=True)
    return subj


def _subjects():
    dp = [(1, 130, 3, 32, 2, (0.7, 0.4, 0.3), True, "bf16"), (2, 64, 2, 64, 4, (0.9, 0.5, 0.0), False, "fp32")]      # test_gpu_bounds.DUALPATH
    return [
        _ew_lowrank("ew-lowrank-fused", "bf16", "auto", True, "bf16", "core", FUSED, "_EdgewiseLowrankFn"),
        _ew_lowrank("ew-lowrank-fused-recomputed-chain", "bf16", "auto", False, "bf16", "core", FUSED, "_EdgewiseLowrankFn"),
        _ew_lowrank("ew-lowrank-generic-fp32", "fp32", "generic", True, "fp32", "core", GENERIC, "_EdgewiseLowrankFn"),
        _ew_lens(),
        _ew_lowrank("ew-shared", "bf16", "auto", True, "bf16", "shared", None, "_EdgewiseSharedFn"),
        _ew_dense("ew-dense-fused", False),
        _ew_dense("ew-dense-k3-generic", True),
        _sdpa("sdpa-packed-causal", "packed-causal", 130, 130, 32, "bf16", (64, 64)),
        _sdpa("sdpa-rect-mask-bias", "mask+bias", 37, 150, 64, "fp32", (70, 100)),
        _sdpa("sdpa-rect-dropout", "dropout", 130, 200, 32, "bf16", (64, 100)),
        _sdpa_lens(),
        _dualpath("dualpath-hops2", dp[0], 0.0, FUSED),
        _dualpath("dualpath-chain-gate", dp[1], 0.3, GENERIC),
        _crossview_module("crossview-generic-cues", True),
        _crossview_module("crossview-folded-packed", False),
        _crossview_core(),
        _quartet("quartet-fused", (1, 130, 3, 32, True, "fp32"), "auto", FUSED),
        _quartet("quartet-plain-generic", (2, 130, 2, 64, False, "bf16"), "generic", GENERIC),
        _layernorm("layernorm-129x72-f32-residual", 129, 72, torch.float32, True),
        _layernorm("layernorm-129x72-f32", 129, 72, torch.float32, False),
        _layernorm("layernorm-33x1152-bf16-residual", 33, 1152, torch.bfloat16, True),
        _layernorm("layernorm-33x1152-bf16", 33, 1152, torch.bfloat16, False),
        _token_gate(),
        _moe(),
        _linear("residual-linear", "residual"),
        _linear("token-linear", "token"),
    ]


SUBJECTS = _subjects()
KERNEL_SUBJECTS = [s for s in SUBJECTS if s.kernel]
each_subject = pytest.mark.parametrize("subj", SUBJECTS, ids=repr)


# ------------------------------------------------------------------------------------------------ the anchor
@each_subject
def test_plain_run_matches_float64(subj):
    """all leaves require grad, one forward, one backward, a fresh contiguous aligned gradient: held to the core's float64 reference
    at the tolerance constants of the core's own tests, on the path the subject names, through the Function it names"""
    res, paths = subj.plain()
    subj.check(res)
    for k, p in paths.items():
        assert p in (FUSED, GENERIC) and (subj.want is None or p == subj.want), f"{k} took path {p}, the subject names {subj.want}"
    case = subj.case()
    subj.setup()
    assert subj.function + "Backward" in graph_nodes(_tuple(case.fn(fresh(case))))
    again = run(subj, case)[0]
    same(again, res, "a second plain run")


# ------------------------------------------------------------------------------------------------ a. subsets of requires_grad
SUBSETS = [(s, p) for s in SUBJECTS for p in ("activations", "parameters", "alternate") if p != "parameters" or s.has_params]


@pytest.mark.parametrize("subj,pattern", SUBSETS, ids=lambda v: str(v))
def test_subsets_of_requires_grad(subj, pattern):
    """activations only (every parameter frozen), parameters only, every second leaf: y and every gradient that is asked for are the
    plain run's, a leaf that does not require grad has no .grad.  (ew-dense-fused: V = 3 <= 6, so the path the dense head takes does
    not depend on what requires grad -- the LAST_PATH assertion below is the one its exception keeps.)"""
    case = subj.case()
    plain, paths = subj.plain()
    names = list(case.leaves)
    rg = {"activations": set(case.acts), "parameters": set(names) - set(case.acts), "alternate": set(names[::2])}[pattern]
    assert rg
    res, got_paths, t = run(subj, case, rg=rg)
    for k, v in t.items():
        assert (v.grad is not None) == (k in rg), f"{k}: requires_grad={k in rg}, .grad is {'set' if v.grad is not None else 'None'}"
    same(res, plain, f"{pattern} require grad", set(case.outs) | {case.gnames[k] for k in rg})
    assert got_paths == paths


# ------------------------------------------------------------------------------------------------ b. no_grad forward
@each_subject
def test_no_grad_forward_then_training_forward(subj):
    """y under torch.no_grad() is within the core's y tolerance of float64, and the training run that follows is the plain run: the
    inference call leaves nothing behind"""
    case = subj.case()
    plain, paths = subj.plain()
    subj.setup()
    with torch.no_grad():
        ys = _tuple(case.fn(fresh(case, rg=set())))
    assert all(not y.requires_grad for y in ys)
    subj.check({n: y for n, y in zip(case.outs, ys)}, y_only=True)
    res, got_paths, _ = run(subj, case)
    same(res, plain, "training run after a no_grad forward")
    assert got_paths == paths


# ------------------------------------------------------------------------------------------------ c. retain_graph
def _grads(case, t):
    return {case.gnames[k]: v.grad for k, v in t.items() if v.grad is not None}


@each_subject
def test_retain_graph(subj):
    """backward twice through one graph gives the same gradients twice; a different gradient through the same graph gives what a
    fresh forward and backward give; without clearing, .grad is the sum torch forms in the gradient's dtype"""
    case = subj.case()
    plain, paths = subj.plain()
    dys2 = tuple((d.flip(0) * 0.5).contiguous() for d in case.dys)
    fresh2, _ = subj.plain(dys=dys2, key="dy2")
    gn = set(case.gnames.values())
    subj.setup()
    t = fresh(case)
    ys = _tuple(case.fn(t))
    for what in ("first", "second"):
        for v in t.values():
            v.grad = None
        torch.autograd.backward(ys, case.dys, retain_graph=True)
        same(_grads(case, t), plain, f"{what} backward through the graph", gn)
        assert paths_now(subj) == paths
    for v in t.values():
        v.grad = None
    torch.autograd.backward(ys, dys2, retain_graph=True)
    same(_grads(case, t), fresh2, "backward with another gradient through the same graph", gn)
    torch.autograd.backward(ys, case.dys)
    same(_grads(case, t), {n: fresh2[n] + plain[n] for n in gn}, "accumulated gradients", gn)


# ------------------------------------------------------------------------------------------------ d. two graphs alive
@each_subject
def test_two_graphs_alive(subj):
    """forward A, forward B (another N / T: another tile count), backward B, backward A: each is what it is alone; again with a
    third forward between forward A and backward A.  State kept outside ctx would show."""
    A, B = subj.case("A"), subj.case("B")
    (pa, paths_a), (pb, paths_b) = subj.plain("A"), subj.plain("B")
    subj.setup()
    ta, tb = fresh(A), fresh(B)
    ya = _tuple(A.fn(ta))
    assert paths_now(subj, "_fwd") == {k: v for k, v in paths_a.items() if k.endswith("_fwd")}
    yb = _tuple(B.fn(tb))
    torch.autograd.backward(yb, B.dys)
    assert paths_now(subj) == paths_b
    torch.autograd.backward(ya, A.dys)
    assert paths_now(subj, "_bwd") == {k: v for k, v in paths_a.items() if k.endswith("_bwd")}
    same(collect(B, yb, tb), pb, "B, run between A's forward and backward")
    same(collect(A, ya, ta), pa, "A, with B run in between")
    ta, tc = fresh(A), fresh(B)
    ya = _tuple(A.fn(ta))
    yc = _tuple(B.fn(tc))                       # a third forward, never differentiated
    torch.autograd.backward(ya, A.dys)
    same(collect(A, ya, ta), pa, "A, with another forward before its backward")
    same(collect(B, yc, tc), pb, "the forward in between", B.outs)


# ------------------------------------------------------------------------------------------------ e. forms of dy
@each_subject
def test_expanded_gradient(subj):
    """(i) y.sum().backward(): a stride-0 gradient, against the plain run with an explicit tensor of ones"""
    import torch.nn.functional as F
    case = subj.case()
    ones, paths = subj.plain(dys=tuple(torch.ones_like(d) for d in case.dys), key="ones")
    subj.setup()
    t = fresh(case)
    core_out = []
    h = case.proj.register_forward_pre_hook(lambda mod, inp: core_out.append(inp[0].detach())) if case.proj is not None else None
    try:
        ys = _tuple(case.fn(t))
    finally:
        if h is not None:
            h.remove()
    sum(y.sum() for y in ys).backward()
    res = collect(case, ys, t)
    assert paths_now(subj) == paths
    if case.proj is None:
        return same(res, ones, "y.sum().backward()")
    # module-level subjects: the expanded tensor is the gradient of torch's own output projection (F.linear; no bias), whose weight
    # gradient torch then forms with other GEMM kernels than from a contiguous tensor (float32: a few units in the last place).
    # Everything the core computes is the plain run's; proj.weight's gradient is what torch's linear gives for the core's output.
    same(res, ones, "y.sum().backward()", set(ones) - {"proj.weight"})
    w = t["proj.weight"].detach().requires_grad_(True)
    (gw,) = torch.autograd.grad(F.linear(core_out[0], w).sum(), w)
    same({"proj.weight": res["proj.weight"]}, {"proj.weight": gw}, "y.sum().backward(), against torch's linear on the core's output")


@pytest.mark.parametrize("form", [sliced, off_boundary], ids=["sliced-from-a-wider-buffer", "off-a-16-byte-boundary"])
@each_subject
def test_gradient_form(subj, form):
    """(ii) a gradient that is not contiguous, (iii) a contiguous one whose first element is off a 16-byte boundary (`.contiguous()`
    returns that one as it is): both the gradient given to backward() and, for module-level subjects, the one entering the core"""
    case = subj.case()
    plain, paths = subj.plain()
    dys = tuple(form(d) for d in case.dys)
    with core_gradient_as(case, form):
        res, got_paths, _ = run(subj, case, dys=dys)
    same(res, plain, f"gradient {form.__name__}")
    assert got_paths == paths


@each_subject
def test_input_leaf_off_a_16_byte_boundary(subj):
    """(iv) the activations off the boundary: a result within the core's tolerance of float64, on the path the core has for them --
    the generic kernels (element loads: attn_generic.hip gather / scatter, edgewise_generic.hip) for the attention cores, which
    ask their `*_fused_supported` query under PATH_AUTO; the torch composition for the token gate and the MoE MLP; a host-side
    refusal for LayerNorm, whose callers ask ops.layernorm_supported first.  Module-level subjects hand their core the aligned output
    of a projection: the plain run's path."""
    case = subj.case()
    if subj.e4 is not None:
        return subj.e4(case)
    _, paths = subj.plain()
    res, got_paths, _ = run(subj, case, remap=lambda k, v: off_boundary(v) if k in case.acts else v.detach().clone())
    subj.check(res)
    want = subj.unaligned if subj.unaligned else paths       # only the entries the documented path sets
    assert {k: got_paths[k] for k in want} == want, f"unaligned inputs took {got_paths}, documented {want}"


# ------------------------------------------------------------------------------------------------ f. create_graph
@pytest.mark.parametrize("subj", KERNEL_SUBJECTS, ids=repr)
def test_create_graph_raises(subj):
    """the kernels have no second derivative: differentiating a gradient taken with create_graph=True raises, it does not
    contribute nothing (or a partial graph, as the folded CrossView backward's torch ops would record)"""
    case = subj.case()
    subj.setup()
    t = fresh(case)
    ys = _tuple(case.fn(t))
    (g,) = torch.autograd.grad(sum(y.sum() for y in ys), t[case.acts[0]], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        (g.float() ** 2).sum().backward()


# ------------------------------------------------------------------------------------------------ g. activation checkpointing
@pytest.mark.parametrize("kind", ["EdgewiseMSA", "BaselineMSA", "MultiHopMSA"])
def test_activation_checkpointing_with_attention_dropout(kind):
    """checkpoint(module, x, use_reentrant=False) with attention dropout 0.1 inside the kernels: y, dx and every parameter gradient
    are those of the run without the checkpoint under the same torch.manual_seed -- the dropout seed comes from torch's CPU
    generator, whose state the checkpoint restores for the recomputation"""
    import mop_amd
    from mop_amd import nn as mnn, ops
    from torch.utils.checkpoint import checkpoint
    mop_amd.set_precision("bf16")
    torch.manual_seed(3)
    B, N, D, H = 2, 65, 96, 3
    if kind == "EdgewiseMSA":
        m, keys = mnn.EdgewiseMSA(D, H, attn_drop=0.1, n_views=4, share_qkv=True, gate_mode="lowrank", gate_rank=2, gate_init="mix5"), ("edgewise_fwd", "edgewise_bwd")
    elif kind == "BaselineMSA":
        m, keys = mnn.BaselineMSA(D, H, attn_drop=0.1), ("sdpa_fwd", "sdpa_bwd")
    else:
        m, keys = mnn.MultiHopMSA(D, H, attn_drop=0.1, hops=2), ("dualpath_fwd", "dualpath_bwd")
    m = m.cuda().to(torch.bfloat16).train()
    x, w = (t.cuda().to(torch.bfloat16) for t in _xw(B, N, D, 9))

    def go(ckpt):
        m.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        torch.manual_seed(1234)
        y = checkpoint(m, xi, use_reentrant=False) if ckpt else m(xi)
        y.backward(w)
        torch.cuda.synchronize()
        res = {"y": y.detach(), "dx": xi.grad}
        res.update({k: p.grad for k, p in m.named_parameters() if p.grad is not None})
        return res, {k: ops.LAST_PATH[k] for k in keys}
    plain, paths = go(False)
    assert len(plain) > 3 and set(paths.values()) == {FUSED}
    other = m(x)                                        # another seed gives another mask: the dropout is on
    assert not torch.equal(other, plain["y"])
    res, got_paths = go(True)
    assert set(res) == set(plain)
    same(res, plain, "checkpointed run")
    assert got_paths == paths


# ------------------------------------------------------------------------------------------------ h. side stream
@each_subject
def test_side_stream(subj):
    """forward and backward inside torch.cuda.stream(s): the kernels are launched on s (ops._stream() is torch's current stream) and
    give the plain run's results"""
    from mop_amd import ops
    case = subj.case()
    plain, paths = subj.plain()
    torch.cuda.synchronize()
    s, cur = torch.cuda.Stream(), torch.cuda.current_stream()
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream() == s and ops._stream().value == torch.cuda.current_stream().cuda_stream
        res, got_paths, _ = run(subj, case)
    cur.wait_stream(s)
    torch.cuda.synchronize()
    same(res, plain, "run on a side stream")
    assert got_paths == paths


# ------------------------------------------------------------------------------------------------ i. in-place edit of the output
@each_subject
def test_inplace_edit_of_the_output(subj):
    """y.add_(1) before backward: an error from autograd where the backward reads y (the flash cores: SDPA, dual-path, folded
    CrossView and Quartet save it: "modified by an inplace operation") and where the Function hands out a view of its output buffer
    (MoE, the linear Functions: "is a view and is being modified inplace"), the plain run's gradients everywhere else (LayerNorm,
    token gate; the module-level subjects, whose y is the output projection's) -- never other gradients"""
    case = subj.case()
    plain, paths = subj.plain()
    subj.setup()
    t = fresh(case)
    ys = _tuple(case.fn(t))
    assert paths_now(subj, "_fwd") == {k: v for k, v in paths.items() if k.endswith("_fwd")}
    try:
        ys[-1].add_(1)
        torch.autograd.backward(ys, case.dys)
        outcome = "equal"
    except RuntimeError as e:
        assert "inplace" in str(e) or "in-place" in str(e), str(e)
        outcome = "error"
    if outcome == "equal":
        same(_grads(case, t), plain, "gradients after y.add_(1)", set(case.gnames.values()))
        assert paths_now(subj) == paths
    assert outcome == subj.inplace, f"y.add_(1) gave {outcome}, expected {subj.inplace}"
