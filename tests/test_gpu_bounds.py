"""-m gpu: every core's kernels stay inside the tensors they are given (tests/guarded_alloc.py).

Each case runs its core twice.  The plain run, on ordinary tensors, is checked against the float64 reference and under the tolerance
that core's own tests use (named at each check).  The guarded run repeats the call with every input embedded in NaN (0xFF bytes for
integer tensors) and with torch.empty / empty_like / zeros / zeros_like handing out poisoned buffers between guard bands.  It must
leave every guard byte alone, give finite results, and give the plain run's results BIT FOR BIT -- every core here is run-to-run
deterministic (fixed reduction orders), so none is compared under a tolerance --, on the path the case names, through buffers the
ledger saw.  A kernel that writes past an output, a saved buffer or a workspace damages a guard; one that reads past an input and
weights the stray values by zero, or reads a workspace nobody wrote, turns a result into NaN.

Module-level cases (EdgewiseMSA, CrossViewMixerMSA) also embed what crosses the core's boundary inside the module: the output of
each qkv projection (the unshared EdgewiseMSA builds its qkv with F.linear inline: there the core's entry point is wrapped for the
guarded run and embeds its first argument) and the gradient that reaches the core from the output projection.

Kernel-read or kernel-written buffers that do NOT come from the four patched functions and are therefore unguarded here:
  * the uint8 mask the cores read: _mask_u8 builds it with `(attn_mask != 0).to(torch.uint8)`, also from an embedded mask;
  * a bias / additive mask that is not float32 or not contiguous (`.to(float32).contiguous()` in _bias_f32);
  * the float32 copies of bfloat16 small parameters (_f32_pack: torch.cat + .to; _f32c: .to) read by the Edgewise, dual-path and
    Quartet cores, and `uc` of the token gate for a non-float32 u;
  * `x.contiguous()` of a row-strided LayerNorm input (ops.layernorm_residual cannot pass a row stride: the kernels' x_ld / y_ld
    are covered through the C ABI in test_layernorm_kernels_with_a_row_stride), `reshape(-1, D).contiguous()` of a strided MoE input, `q.contiguous()` of
    a packed projection that is not contiguous (an incoming gradient that is not contiguous, aligned and of the core's dtype is
    copied by ops._grad_in into a torch.empty buffer, a guarded one here: tests/test_gpu_autograd_contract.py runs those forms);
  * the mixed keys k1', k2' of the folded CrossView core (`_cv_mixed_keys`: arithmetic + .contiguous()) and the zero chain logit
    of ops.crossview_core (`new_zeros`);
  * what autograd itself allocates (accumulated .grad tensors are the guarded tensors the Functions return, but sums such as
    `dlg.sum()` or `dmix.sum((0, 1))` are new tensors written by torch, not by the kernels).
The graph-capture paths are not run under the context manager."""
import numpy as np
import pytest
import torch

from attn_ref import bf16_exact, sdpa_ref64
from gpu_util import check_grads, max_abs, oracle_bf16_noise, rel_err
from guarded_alloc import embedded, guarded_allocations

pytestmark = pytest.mark.gpu

TOL_BF16, GTOL_BF16 = 1e-2, 3e-2        # test_gpu_edgewise.py
YTOL, GTOL, GFLOOR = 1e-2, 1.5e-2, 1e-2   # test_gpu_attn_edges.py
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


# ------------------------------------------------------------------------------------------------ the two runs and what they must share
def _nbytes(t):
    return t.numel() * t.element_size()


def _assert_guarded_equals_plain(ledger, plain, guarded, paths, want_path, sizes, what):
    """the five assertions of a case; plain / guarded: {name: tensor} of the two runs; paths: LAST_PATH keys; sizes: payload sizes
    (bytes) of the buffers the call must have obtained from the ledger, one entry per buffer: a size listed n times must have been
    handed out at least n times"""
    from collections import Counter
    from mop_amd import ops
    torch.cuda.synchronize()
    assert ledger.intact(), f"{what}: {ledger.describe_damage()}"
    assert set(guarded) == set(plain), what
    for n, g in guarded.items():
        p = plain[n]
        ok = torch.isfinite(g) | ((p == float("-inf")) & (g == float("-inf"))) if g.dtype.is_floating_point else torch.ones_like(g, dtype=torch.bool)
        assert bool(ok.all()), f"{what}: {n} has {int((~ok).sum())} non-finite value(s) in the guarded run"
        assert g.dtype == p.dtype and torch.equal(g, p), \
            f"{what}: {n} differs from the plain run in {int((g != p).sum())} value(s), max |diff| {float((g.double() - p.double()).abs().max()):.3e}"
    for k in paths:
        assert ops.LAST_PATH[k] == want_path, f"{what}: {k} took path {ops.LAST_PATH[k]}, the case names {want_path}"
    assert ledger.count() > 0, f"{what}: nothing was allocated through the patched functions"
    for s, n in Counter(sizes).items():
        assert ledger.count(s) >= n, f"{what}: {ledger.count(s)} buffer(s) of {s} bytes handed out, {n} expected ({ledger.count()} buffers in all)"


def _leaf(t, embed):
    """an input of a run: a fresh leaf with t's values and requires_grad, embedded in poison for the guarded run"""
    if t is None:
        return None
    return embedded(t) if embed else t.detach().clone().requires_grad_(t.requires_grad)


def _two_runs(call, inputs, check_plain, paths, want_path, sizes, what, poison=None):
    """call(dict of leaves) -> {name: result}.  check_plain(results) holds the plain run to the core's float64 reference.
    poison(dict of leaves): optional extra poison written into the guarded run's inputs (values the core must not use)."""
    plain = call({k: _leaf(t, False) for k, t in inputs.items()})
    torch.cuda.synchronize()
    check_plain(plain)
    with guarded_allocations() as ledger:
        ins = {k: _leaf(t, True) for k, t in inputs.items()}
        if poison is not None:
            with torch.no_grad():
                poison(ins)
        guarded = call(ins)
        torch.cuda.synchronize()
    _assert_guarded_equals_plain(ledger, plain, guarded, paths, want_path, sizes(plain) if callable(sizes) else sizes, what)


class _Embed(torch.autograd.Function):
    """identity whose output, and whose gradient on the way back, sit in NaN"""

    @staticmethod
    def forward(ctx, t):
        return embedded(t, requires_grad=False)

    @staticmethod
    def backward(ctx, g):
        return embedded(g, requires_grad=False)


def _module_runs(m, x, w, check_plain, paths, want_path, sizes, what, qkv=("qkv",), seed=None, core=None, **fk):
    """_two_runs for an attention module: results are y, dx and every parameter gradient.  Guarded run: x, w and every parameter
    embedded, the qkv projections' outputs and the gradient that enters the core embedded by hooks.  core: name of an ops entry
    point whose first argument is embedded on the guarded run (a qkv no module hook can reach)."""
    from mop_amd import ops
    def run(xi, wi):
        m.zero_grad(set_to_none=True)
        if seed is not None:
            torch.manual_seed(seed)              # the module draws its dropout seed from torch's CPU generator
        y = m(xi, **fk)
        y.backward(wi)
        torch.cuda.synchronize()
        res = {"y": y.detach(), "dx": xi.grad}
        res.update({k: p.grad for k, p in m.named_parameters() if p.grad is not None})
        return res

    plain = run(x.detach().clone().requires_grad_(True), w)
    check_plain(plain)
    hooks = []
    with guarded_allocations() as ledger:
        for p in m.parameters():
            p.data = embedded(p.data, requires_grad=False)
        for name in qkv:
            hooks.append(getattr(m, name).register_forward_hook(lambda mod, inp, out: _Embed.apply(out)))
        hooks.append(m.proj.register_forward_pre_hook(lambda mod, inp: (_Embed.apply(inp[0]),)))
        real = getattr(ops, core) if core else None
        seen = []
        if core:
            def wrapped(first, *a, **k):
                seen.append(first.shape)
                return real(_Embed.apply(first), *a, **k)
            setattr(ops, core, wrapped)
        try:
            guarded = run(embedded(x, requires_grad=True), embedded(w))
        finally:
            for h in hooks:
                h.remove()
            if core:
                setattr(ops, core, real)
        assert not core or len(seen) == 1, f"{what}: ops.{core} was called {len(seen)} time(s)"
    _assert_guarded_equals_plain(ledger, plain, guarded, paths, want_path, sizes, what)


_REF = {}


def _cached(key, fn):
    """float64 references are computed once per distinct case and never modified"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _f(t):
    return t.detach().float().cpu().numpy()


def _param_grads(res):
    return {k: _f(v) for k, v in res.items() if k not in ("y", "dx")}


def _check_param_grads(grads, gref, gtol, **kw):
    """check_grads over the reference's tensors; a gradient the module returns beyond them must be exactly zero"""
    for k in set(grads) - set(gref):
        assert not grads[k].any(), f"{k}: no reference gradient, and the module's is not zero"
    check_grads({k: grads[k] for k in gref}, gref, gtol, **kw)


# ------------------------------------------------------------------------------------------------ Edgewise
def _rb(t):
    return torch.as_tensor(t).to(torch.bfloat16).double().numpy()


def _perturb(m, head_scale=3.0):
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("_scale"):
                p.add_(0.1 * torch.randn_like(p))
            elif "edge_head" in n_ and n_.endswith("weight"):
                p.mul_(head_scale)
        m.chain_value_logit.fill_(-0.5)
    return m


def _ew_oracle(key, m, x, w, H, V, share, io_bf16, dil=None, drop=None, noise=True):
    """the float64 oracle on the inputs as given (-> out, dx, grads, bf16 noise per tensor) and, for bf16 tensors, on the inputs
    rounded to bfloat16 as the kernels read them (-> out, dx)"""
    from oracle import edgewise as oe

    params = {k: v.detach().cpu().double().numpy() for k, v in m.state_dict().items()}
    kw = dict(lens_dilations=dil) if dil is not None else {}
    fwd = lambda xx, pp, *a: oe.module_fwd(xx, pp, *a, drop=drop, **kw)     # noqa: E731

    def exact():
        x64, w64 = x.double().numpy(), w.double().numpy()
        out, cache = fwd(x64, params, H, V, share, 0.5)
        dx, g = oe.module_bwd(w64, cache)
        nz = oracle_bf16_noise(fwd, oe.module_bwd, x64, w64, params, H, V, share, 0.5) if noise else None
        return out, dx, g, nz

    def rounded():
        yr, cb = fwd(_rb(x), {k: _rb(v) for k, v in params.items()}, H, V, share, 0.5)
        dxr, gr = oe.module_bwd(_rb(w), cb)
        return yr, dxr, gr
    return (*_cached((key, "exact"), exact), _cached((key, "rounded"), rounded) if io_bf16 else None)


def _ew_check_bf16_arith(ref, io_bf16):
    """bf16-MFMA arithmetic: test_fused_vs_oracle_shape_sweep / test_fused_dense_head_backward_vs_oracle for float32 tensors,
    test_edgewise_dropout_matches_the_oracle_under_the_same_mask for bfloat16 tensors (y and dx against the oracle on the rounded
    inputs, parameter gradients against the exact ones under the oracle's own bf16 noise)"""
    out, dx, g, nz, rounded = ref

    def check(res):
        yo, dxo = (rounded[0], rounded[1]) if io_bf16 else (out, dx)
        ey, ed = max_abs(_f(res["y"]), yo), rel_err(_f(res["dx"]), dxo)
        print(f"y {ey:.3e} (bound {TOL_BF16 * max(1.0, float(np.abs(yo).max())):.1e}), dx {ed:.3e} (bound {GTOL_BF16:.0e})")
        assert ey <= TOL_BF16 * max(1.0, float(np.abs(yo).max())), f"y {ey:.3e}"
        assert ed <= GTOL_BF16, f"dx {ed:.3e}"
        _check_param_grads(_param_grads(res), g, GTOL_BF16, d=nz)
    return check


def _ew_sizes(B, N, D, Vq, es):
    """the core's output (B,N,H,dk) and its input gradient dqkv (B,N,Vq,3,H,dk)"""
    return [B * N * D * es, B * N * Vq * 3 * D * es]


LOWRANK = [(2, 1, 32, 2, 2, 1), (2, 33, 128, 2, 2, 3), (2, 65, 96, 3, 4, 2), (2, 197, 128, 2, 5, 4)]
LOWRANK_CASES = [(s, io, True) for s in LOWRANK for io in ("bf16", "fp32")] + [(LOWRANK[2], io, False) for io in ("bf16", "fp32")]


@pytest.mark.parametrize("shape,io,save_chain", LOWRANK_CASES,
                         ids=["x".join(map(str, s)) + f"-{io}-" + ("saved-chain" if sc else "recomputed-chain") for s, io, sc in LOWRANK_CASES])
def test_edgewise_lowrank_fused(shape, io, save_chain):
    """EdgewiseMSA(share_qkv, low-rank head) on the fused forward and its three-launch backward, through
    edgewise_lowrank_core_shared (mopk_edgewise_params_fwd / _bwd around the core); N = 65 also without the saved chain state"""
    import mop_amd
    from mop_amd import ops
    from test_gpu_edgewise import _mk
    B, N, D, H, V, r = shape
    mop_amd.set_precision("bf16")
    ops.set_save_chain_state(save_chain)
    m = _mk(D, H, V, r, seed=B * 1000 + N)
    g = torch.Generator().manual_seed(N)
    x, w = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    bf = io == "bf16"
    ref = _ew_oracle(("lowrank", shape), m, x, w, H, V, True, bf)
    dt = torch.bfloat16 if bf else torch.float32
    _module_runs(m.cuda().to(dt).eval(), x.cuda().to(dt), w.cuda().to(dt), _ew_check_bf16_arith(ref, bf),
                 ("edgewise_fwd", "edgewise_bwd"), FUSED, _ew_sizes(B, N, D, 1, 2 if bf else 4), f"lowrank fused {shape} {io}")


def test_edgewise_lowrank_unshared_views():
    """share_qkv=False: V projections, a (B,N,V,3,H,dk) qkv whose gradient the backward zero-fills except v of views 0 and V - 1.
    The fused kernels take shared views only, so this is the generic path in bf16 arithmetic."""
    import mop_amd
    from mop_amd.nn import EdgewiseMSA
    B, N, D, H, V, r = 2, 33, 64, 2, 3, 2
    mop_amd.set_precision("bf16")
    torch.manual_seed(B * 1000 + N)
    m = _perturb(EdgewiseMSA(D, H, n_views=V, share_qkv=False, gate_mode="lowrank", gate_rank=r, gate_init="mix5"))
    g = torch.Generator().manual_seed(N)
    x, w = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    ref = _ew_oracle(("unshared",), m, x, w, H, V, False, False)
    _module_runs(m.cuda().eval(), x.cuda(), w.cuda(), _ew_check_bf16_arith(ref, False), ("edgewise_fwd", "edgewise_bwd"), GENERIC,
                 _ew_sizes(B, N, D, V, 4), "lowrank unshared", qkv=(), core="edgewise_lowrank_core")


def test_edgewise_lowrank_fused_with_attention_dropout():
    """p = 0.2 inside the fused kernels, fixed seed: the backward redraws the forward's mask"""
    import mop_amd
    from mop_amd import ops
    from mop_amd.nn import EdgewiseMSA
    B, N, D, H, V, r, p = 2, 65, 96, 3, 4, 2, 0.2
    mop_amd.set_precision("bf16")
    torch.manual_seed(B * 1000 + N)
    m = _perturb(EdgewiseMSA(D, H, attn_drop=p, n_views=V, share_qkv=True, gate_mode="lowrank", gate_rank=r, gate_init="mix5"))
    g = torch.Generator().manual_seed(N)
    x, w = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    torch.manual_seed(77)
    seed = ops.dropout_seed()
    drop = ops.dropout_keep_mask(seed, p, B, H, N).numpy().astype(np.float64) / (1.0 - p)
    ref = _ew_oracle(("dropout",), m, x, w, H, V, True, True, drop=drop)
    dt = torch.bfloat16
    _module_runs(m.cuda().to(dt).train(), x.cuda().to(dt), w.cuda().to(dt), _ew_check_bf16_arith(ref, True),
                 ("edgewise_fwd", "edgewise_bwd"), FUSED, _ew_sizes(B, N, D, 1, 2), "lowrank fused dropout", seed=77)


@pytest.mark.parametrize("shape", [(3, 50, 128, 2, 3), (2, 129, 64, 1, 4)], ids=lambda s: "x".join(map(str, s)))
def test_edgewise_dense_head_fused(shape):
    """as test_fused_dense_head_backward_vs_oracle: the dense gate head inside the fused forward and backward"""
    import mop_amd
    from mop_amd.nn import EdgewiseMSA
    B, N, D, H, V = shape
    torch.manual_seed(N * 11 + V)
    m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="dense", use_k3=False, gate_init="and")
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("_scale"):
                p.add_(0.1 * torch.randn_like(p))
            elif n_.endswith("conv2.bias"):
                p.copy_(0.7 * torch.randn_like(p))
            elif "conv1" in n_ or "conv2" in n_:
                p.mul_(1.5)
        m.chain_value_logit.fill_(-0.5)
    g = torch.Generator().manual_seed(N)
    x, w = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    ref = _ew_oracle(("dense", shape), m, x, w, H, V, True, False)
    mop_amd.set_precision("bf16")
    _module_runs(m.cuda().eval(), x.cuda(), w.cuda(), _ew_check_bf16_arith(ref, False), ("edgewise_fwd", "edgewise_bwd"), FUSED,
                 _ew_sizes(B, N, D, 1, 4), f"dense head fused {shape}")


@pytest.mark.parametrize("shape", [(1, 8, 64, 4, 2, 1, (1, 9)), (3, 50, 128, 2, 3, 4, (1, 2, 3))], ids=lambda s: "x".join(map(str, s[:6])))
def test_edgewise_lowrank_lens_bank_fused(shape):
    """as test_fused_lowrank_lens_bank_vs_oracle_and_generic: the S lens bank as extra mean-feature channels of the fused kernels,
    with lens_means_hip / lens_means_bwd_hip around them"""
    import mop_amd
    from mop_amd import ops
    from mop_amd.nn import EdgewiseMSA
    from oracle import edgewise as oe
    B, N, D, H, V, r, dil = shape
    torch.manual_seed(N * 11 + V)
    m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="lowrank", gate_rank=r, gate_init="mix5", use_lens_bank=True, lens_dilations=dil)
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("_scale"):
                p.add_(0.1 * torch.randn_like(p))
            if "proj.weight" in n_ and "edge_head" in n_:
                p.mul_(3.0)
        m.chain_value_logit.fill_(-0.5)
    x, w = torch.randn(B, N, D), torch.randn(B, N, D)

    def make():
        params = {k: _rb(v) for k, v in m.state_dict().items()}
        out, cache = oe.module_fwd(_rb(x), params, H, V, True, 0.5, lens_dilations=dil)
        return (out, *oe.module_bwd(_rb(w), cache))
    out, dx_ref, g_ref = _cached(("lens", shape), make)
    mop_amd.set_precision("bf16")
    dt = torch.bfloat16
    mg, xg, wg = m.cuda().to(dt).eval(), x.cuda().to(dt), w.cuda().to(dt)

    def check(res):
        ops.set_path("generic")                     # the bound of the fused gradients is stated against the generic path's error
        try:
            mg.zero_grad(set_to_none=True)
            xi = xg.detach().clone().requires_grad_(True)
            mg(xi).backward(wg)
            assert ops.LAST_PATH["edgewise_bwd"] == GENERIC
            gg = {k: _f(p.grad) for k, p in mg.named_parameters() if p.grad is not None}
        finally:
            ops.set_path("auto")
        assert max_abs(_f(res["y"]), out) <= TOL_BF16, f"y {max_abs(_f(res['y']), out):.3e}"
        assert rel_err(_f(res["dx"]), dx_ref) <= GTOL_BF16, f"dx {rel_err(_f(res['dx']), dx_ref):.3e}"
        grads = _param_grads(res)
        assert set(grads) == set(g_ref)
        for k in g_ref:
            e, eg = rel_err(grads[k].reshape(g_ref[k].shape), g_ref[k]), rel_err(gg[k].reshape(g_ref[k].shape), g_ref[k])
            assert e <= max(GTOL_BF16, 2.0 * eg), f"{k}: fused {e:.3e} generic {eg:.3e}"
    E = len(dil) * V
    sizes = _ew_sizes(B, N, D, 1, 2) + 4 * [B * H * E * N * 4]       # and the lens means (B,H,E,N) float32: row, col, their gradients
    _module_runs(mg, xg, wg, check, ("edgewise_fwd", "edgewise_bwd"), FUSED, sizes, f"lowrank + lens bank fused {shape}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["lowrank", "dense_k3"])
def test_edgewise_generic_path(variant, prec):
    """ops.set_path("generic"): the multi-kernel path with its N x N workspace; low-rank (3, 17, 64, 4, 3, 2) as
    test_edgewise_vs_oracle_seeded, dense head with the 3x3 mid convolution at N = 33 as test_variants_vs_oracle_at_full_sequence_length"""
    import mop_amd
    from mop_amd import ops
    from mop_amd.nn import EdgewiseMSA
    mop_amd.set_precision(prec)
    ops.set_path("generic")
    if variant == "lowrank":
        B, N, D, H, V, r = 3, 17, 64, 4, 3, 2
        torch.manual_seed(B * 1000 + N)
        m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="lowrank", gate_rank=r, gate_init="mix5")
        with torch.no_grad():
            for n_, p in m.named_parameters():
                if n_.endswith("_scale"):
                    p.add_(0.1 * torch.randn_like(p))
                if "proj.weight" in n_ and "edge_head" in n_:
                    p.mul_(3.0)
    else:
        B, N, D, H, V = 2, 33, 64, 1, 3
        torch.manual_seed(N)
        m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="dense", use_k3=True, gate_init="and")
        with torch.no_grad():
            for n_, p in m.named_parameters():
                if n_.endswith("_scale"):
                    p.add_(0.1 * torch.randn_like(p))
                elif n_.endswith("conv2.bias"):
                    p.copy_(0.5 * torch.randn_like(p))
            m.chain_value_logit.fill_(-0.5)
    x, w = torch.randn(B, N, D), torch.randn(B, N, D)
    ref = _ew_oracle(("generic", variant, prec), m, x, w, H, V, True, False, noise=prec == "bf16")
    out, dx_ref, g_ref = ref[:3]

    def check_fp32(res):
        assert max_abs(_f(res["y"]), out) <= 1e-4, f"y {max_abs(_f(res['y']), out):.3e}"
        assert rel_err(_f(res["dx"]), dx_ref) <= 1e-3, f"dx {rel_err(_f(res['dx']), dx_ref):.3e}"
        grads = _param_grads(res)
        if variant == "dense_k3":
            return _check_param_grads(grads, g_ref, 1e-3, floor=1e-3)
        assert set(grads) == set(g_ref)
        for k in g_ref:
            assert rel_err(grads[k].reshape(g_ref[k].shape), g_ref[k]) <= 1e-3, k
    _module_runs(m.cuda().eval(), x.cuda(), w.cuda(), check_fp32 if prec == "fp32" else _ew_check_bf16_arith(ref, False),
                 ("edgewise_fwd", "edgewise_bwd"), GENERIC, _ew_sizes(B, N, D, 1, 4), f"generic {variant} {prec}")


# ------------------------------------------------------------------------------------------------ SDPA
def _np(t):
    return t.detach().double().cpu().numpy()


def _hp(t):
    return np.transpose(_np(t), (0, 2, 1, 3))


def _attn_close(res, yr, ref, what):
    """test_gpu_attn_edges._assert_close: y max-abs / max|y_ref| <= 1e-2, gradients 1.5e-2 of max(max|ref|, 1e-2 x the largest)"""
    from test_gpu_attn_edges import _assert_close
    _assert_close(_np(res["y"]), yr, {n: _np(res[n]) for n in ref}, ref, what)


def _sdpa_inputs(B, N, Nk, H, dk, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = (bf16_exact(torch.randn(B, n, H, dk, device="cuda", generator=g)).to(dt).requires_grad_(True) for n in (N, Nk, Nk))
    dy = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g)).to(dt)
    return q, k, v, dy, g


SDPA_CASES = [
    # B, N, Nk, kind
    (2, 197, 197, "causal"), (2, 130, 200, "rect"), (3, 1, 1, "rect"), (2, 65, 65, "packed"), (2, 130, 200, "mask+bias"),
    (2, 130, 200, "dropout")]


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("io", ["bf16", "fp32"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("B,N,Nk,kind", SDPA_CASES, ids=lambda v: str(v))
def test_sdpa(B, N, Nk, kind, dk, io, path):
    """ops.sdpa_core in bf16 arithmetic against attn_ref.sdpa_ref64 (dropout: oracle.sdpa under the kernels' own keep mask, as
    test_sdpa_dropout_matches_the_oracle_under_the_same_mask)"""
    import mop_amd
    from mop_amd import ops
    from oracle import sdpa as osd
    mop_amd.set_precision("bf16")
    ops.set_path(path)
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    H, es = 2, 2 if io == "bf16" else 4
    q, k, v, dy, g = _sdpa_inputs(B, N, Nk, H, dk, dt, 7 * N + Nk + dk)
    inputs, kw = dict(q=q, k=k, v=v, dy=dy), {}
    mask = bias = None
    if kind == "mask+bias":
        mask = torch.rand(B, 1, N, Nk, device="cuda", generator=g) > 0.3
        mask[..., 0] = True                                               # no fully blocked row
        bias = 0.5 * torch.randn(1, H, N, Nk, device="cuda", generator=g)
        inputs.update(mask=mask, bias=bias)
    if kind == "dropout":
        kw = dict(dropout_p=0.2, seed=0xC0FFEE1234567)
    if kind == "packed":
        inputs = dict(qkv=torch.stack([q, k, v], 2).detach().requires_grad_(True), dy=dy)

    def call(t):
        if kind == "packed":
            y = ops.sdpa_core(t["qkv"])
            y.backward(t["dy"])
            d = t["qkv"].grad
            return dict(y=y.detach(), dq=d[:, :, 0], dk=d[:, :, 1], dv=d[:, :, 2])
        y = ops.sdpa_core(t["q"], t["k"], t["v"], attn_mask=t.get("mask"), bias=t.get("bias"), causal=kind == "causal", **kw)
        y.backward(t["dy"])
        return dict(y=y.detach(), dq=t["q"].grad, dk=t["k"].grad, dv=t["v"].grad)

    def make():
        if kind == "dropout":
            drop = ops.dropout_keep_mask(kw["seed"], 0.2, B, H, N, Nk).numpy().astype(np.float64) / 0.8
            yr, c = osd.core_fwd(_hp(q), _hp(k), _hp(v), None, None, drop)
            gr = osd.core_bwd(_hp(dy.view(B, N, H, dk)), c)
            return np.transpose(yr, (0, 2, 1, 3)).reshape(B, N, H * dk), {n: np.transpose(gr[n], (0, 2, 1, 3)) for n in ("dq", "dk", "dv")}
        r = [t.detach().double().requires_grad_(True) for t in (q, k, v)]
        yr = sdpa_ref64(*r, mask=mask, bias=bias, causal=kind == "causal")
        (yr * dy.double()).sum().backward()
        return yr.detach().cpu().numpy(), {n: t.grad.cpu().numpy() for n, t in zip(("dq", "dk", "dv"), r)}
    yr, ref = _cached(("sdpa", B, N, Nk, kind, dk, io), make)
    want = FUSED if path == "fused" else GENERIC
    sizes = [B * N * H * dk * es] + ([3 * B * N * H * dk * es] if kind == "packed" else [B * N * H * dk * es] + 2 * [B * Nk * H * dk * es])   # y; dqkv | dq, dk, dv

    def check(res):
        if kind != "dropout":
            return _attn_close(res, yr, ref, f"sdpa {kind}")
        ey = max_abs(_np(res["y"]), yr)                      # test_sdpa_dropout_matches_the_oracle_under_the_same_mask
        assert ey <= 1e-2 * max(1.0, float(np.abs(yr).max())), ey
        for n in ref:
            assert rel_err(_np(res[n]), ref[n]) <= 3e-2, (n, rel_err(_np(res[n]), ref[n]))
    _two_runs(call, inputs, check, ("sdpa_fwd", "sdpa_bwd"), want, sizes,
              f"sdpa {kind} B={B} N={N} Nk={Nk} dk={dk} {io} {path}")


def test_sdpa_with_lengths():
    """q_lens / kv_lens on the fused length-aware kernels: lengths 0, 1, inside a tile and full; in the guarded run q, k, v and dy
    are NaN beyond each row's length as well (test_nothing_beyond_a_length_is_used).  Reference and bound:
    test_sdpa_lens_matches_float64 (naive_lens_attention, 2e-2 of max(1, |ref|max) for bf16)."""
    from mop_amd import ops
    from test_whisper_audio_lens_cpu import naive_lens_attention
    B, N, Nk, H, dk, dt = 4, 130, 200, 2, 64, torch.bfloat16
    q, k, v, dy, _ = _sdpa_inputs(B, N, Nk, H, dk, dt, 11)
    kl = torch.tensor([0, 1, 64, 200], dtype=torch.int32, device="cuda")
    ql = torch.tensor([130, 1, 0, 65], dtype=torch.int32, device="cuda")

    def call(t):
        y = ops.sdpa_core(t["q"], t["k"], t["v"], q_lens=t["ql"], kv_lens=t["kl"])
        y.backward(t["dy"])
        return dict(y=y.detach(), dq=t["q"].grad, dk=t["k"].grad, dv=t["v"].grad)

    def poison(t):
        for b in range(B):
            t["k"][b, int(kl[b]):] = float("nan")
            t["v"][b, int(kl[b]):] = float("nan")
            t["q"][b, int(ql[b]):] = float("nan")
            t["dy"][b, int(ql[b]):] = float("nan")

    def check(res):
        q64, k64, v64 = (t.detach().cpu().double().requires_grad_(True) for t in (q, k, v))
        ref = naive_lens_attention(q64, k64, v64, ql.cpu(), kl.cpu(), False)
        rq, rk, rv = torch.autograd.grad(ref, (q64, k64, v64), dy.cpu().double())
        for name, want in (("y", ref.detach()), ("dq", rq), ("dk", rk), ("dv", rv)):
            e = float((res[name].detach().cpu().double().reshape(want.shape) - want).abs().max() / max(1.0, float(want.abs().max())))
            assert e <= 2e-2, (name, e)
    es = 2
    _two_runs(call, dict(q=q, k=k, v=v, dy=dy, ql=ql, kl=kl), check, ("sdpa_fwd", "sdpa_bwd"), FUSED,
              2 * [B * N * H * dk * es] + 2 * [B * Nk * H * dk * es], "sdpa with lengths", poison=poison)


# ------------------------------------------------------------------------------------------------ dual-path, CrossView, Quartet
DUALPATH = [
    # B, N, H, dk, hops, (and, or, not), causal, io
    (1, 130, 3, 32, 2, (0.7, 0.4, 0.3), True, "bf16"), (2, 64, 2, 64, 4, (0.9, 0.5, 0.0), False, "fp32"),
    (2, 150, 2, 64, 3, (1.0, 0.3, 0.0), "mask", "bf16")]


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("cfg", DUALPATH, ids=lambda c: f"N{c[1]}-dk{c[3]}-hops{c[4]}-{c[6]}-{c[7]}")
def test_dualpath(cfg, path):
    """ops.dualpath_core (cases of test_dualpath_fused_matches_generic) against oracle.multihop in float64 under
    test_gpu_attn_edges' bound (test_dualpath_logit_scale_sweep, test_dualpath_fully_blocked_rows for the mask)"""
    import mop_amd
    from mop_amd import ops
    from oracle import multihop as om
    B, N, H, dk, hops, gates, causal, io = cfg
    mop_amd.set_precision("bf16")
    ops.set_path(path)
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(N + hops)
    base = [bf16_exact(torch.randn(B, N, H, dk, device="cuda", generator=g)).to(dt).requires_grad_(True) for _ in range(6)]
    dy = bf16_exact(torch.randn(B, N, H * dk, device="cuda", generator=g)).to(dt)
    names = ("q1", "k1", "v1", "q2", "k2", "v2")
    inputs = dict(zip(names, base), dy=dy, lg=torch.tensor(-0.5, device="cuda", requires_grad=True))
    mask = None
    if causal == "mask":
        mask = torch.rand(B, 1, N, N, device="cuda", generator=g) > 0.35
        mask |= torch.eye(N, dtype=torch.bool, device="cuda")
        inputs["mask"] = mask

    def call(t):
        y = ops.dualpath_core(*(t[n] for n in names), t["lg"], *gates, 0.0, 0.6, hops, t.get("mask"), causal=causal is True)
        y.backward(t["dy"])
        return dict(y=y.detach(), dlogit=t["lg"].grad, **{"d" + n: t[n].grad for n in names})

    def make():
        blocked = None
        if mask is not None:
            blocked = ~mask.cpu().numpy()
        elif causal is True:
            blocked = np.broadcast_to(~np.tril(np.ones((N, N), dtype=bool)), (B, 1, N, N))
        yo, c = om.core_fwd(*(_hp(t) for t in base), dict(and_=gates[0], or_=gates[1], not_=gates[2], chain=0.0), 0.6, hops, -0.5, blocked)
        go = om.core_bwd(_hp(dy.view(B, N, H, dk)), c)
        return np.transpose(yo, (0, 2, 1, 3)).reshape(B, N, -1), {"d" + n: np.transpose(go["d" + n], (0, 2, 1, 3)) for n in names}
    yr, ref = _cached(("dualpath", cfg), make)
    es = 2 if io == "bf16" else 4
    _two_runs(call, inputs, lambda res: _attn_close(res, yr, ref, "dualpath"), ("dualpath_fwd", "dualpath_bwd"),
              FUSED if path == "fused" else GENERIC, 7 * [B * N * H * dk * es] + [B * H * 4], f"dualpath {cfg} {path}")     # y, six gradients, d logit


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("variant", ["folded-fused", "generic-cues"])
def test_crossview_mixer(variant, with_mask):
    """CrossViewMixerMSA(128, 2), B = 2, N = 150: the folded route on the fused two-score kernels, and the generic kernels with
    transpose cues; float32 tensors in bf16 arithmetic against oracle.crossview's module in float64 under the bounds of
    test_gpu_siblings.test_crossview_mixer for that arithmetic (y 1e-2, gradients 3e-2 with a floor of 1e-2 x the largest)"""
    import mop_amd
    from mop_amd.nn import CrossViewMixerMSA
    from oracle import crossview as oc
    mop_amd.set_precision("bf16")
    B, N, D, H = 2, 150, 128, 2
    cues = variant == "generic-cues"
    torch.manual_seed(5)
    m = CrossViewMixerMSA(D, H, use_transpose_cues=cues, t1=0.3, t2=-0.2)
    with torch.no_grad():
        m.mix.add_(0.3 * torch.randn(2, 2))
    x, w = torch.randn(B, N, D), torch.randn(B, N, D)
    mask = None
    if with_mask:
        mask = ((torch.rand(B, 1, N, N) > 0.3) | torch.eye(N, dtype=torch.bool)).float()

    def make():
        params = {k: v.detach().double().numpy() for k, v in m.state_dict().items()}
        out, c = oc.module_fwd(x.double().numpy(), params, H, None if mask is None else mask.numpy(), cues, 0.3, -0.2)
        return (out, *oc.module_bwd(w.double().numpy(), c))
    out, dx_ref, g_ref = _cached(("crossview", variant, with_mask), make)

    def check(res):
        assert max_abs(_f(res["y"]), out) <= 1e-2, f"y {max_abs(_f(res['y']), out):.3e}"
        assert rel_err(_f(res["dx"]), dx_ref) <= 3e-2, f"dx {rel_err(_f(res['dx']), dx_ref):.3e}"
        _check_param_grads(_param_grads(res), g_ref, 3e-2, floor=1e-2)
    fk = {} if mask is None else dict(attn_mask=embedded(mask.cuda()))
    es = 4
    # folded: y, dk1', dk2', dv2 and the two packed gradients; generic: y, five gradients and the d mix partials
    sizes = 4 * [B * N * D * es] + 2 * [3 * B * N * D * es] if not cues else 6 * [B * N * D * es] + [B * H * 4 * 4]
    _module_runs(m.cuda().eval(), x.cuda(), w.cuda(), check, ("crossview_fwd",), GENERIC if cues else FUSED,
                 sizes, f"crossview {variant} mask={with_mask}", qkv=("qkv1", "qkv2"), **fk)


QUARTET = [(2, 130, 2, 64, False, "bf16"), (1, 200, 3, 32, True, "fp32"), (1, 1, 2, 32, True, "fp32")]


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("cfg", QUARTET, ids=lambda c: f"T{c[1]}-dh{c[3]}-{'quartet' if c[4] else 'plain'}-{c[5]}")
def test_quartet(cfg, path):
    """ops.quartet_core (cases of test_quartet_fused_matches_generic) against oracle.quartet in float64 under test_gpu_attn_edges'
    bound (test_quartet_logit_scale_sweep); the scalar gradients as test_quartet_dropout_matches_the_oracle_under_the_same_mask"""
    import mop_amd
    from mop_amd import ops
    from oracle import quartet as oq
    B, T, H, dh, uq, io = cfg
    mop_amd.set_precision("bf16")
    ops.set_path(path)
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(T)
    base = [bf16_exact(torch.randn(B, T, H, dh, device="cuda", generator=g)).to(dt).requires_grad_(True) for _ in range(5)]
    dy = bf16_exact(torch.randn(B, T, H * dh, device="cuda", generator=g)).to(dt)
    names = ("q", "k", "v", "q2", "k2")[:5 if uq else 3]
    inputs = dict(zip(names, base), dy=dy)
    if uq:
        inputs.update(mix=torch.tensor([0.3], device="cuda", requires_grad=True), qs=torch.tensor([0.8], device="cuda", requires_grad=True))

    def call(t):
        y = ops.quartet_core(t["q"], t["k"], t["v"], t.get("q2"), t.get("k2"), t.get("mix"), t.get("qs"), None, 1e-5, uq)
        y.backward(t["dy"])
        res = dict(y=y.detach(), **{"d" + n: t[n].grad for n in names})
        if uq:
            res.update(dmixture=t["mix"].grad, dquartet_scale=t["qs"].grad)
        return res

    def make():
        yo, c = oq.core_fwd(*(_hp(t) for t in base), 0.3, 0.8, 1e-5, uq, True, None)
        go = oq.core_bwd(_hp(dy.view(B, T, H, dh)), c)
        return (np.transpose(yo, (0, 2, 1, 3)).reshape(B, T, -1), {"d" + n: np.transpose(go["d" + n], (0, 2, 1, 3)) for n in names},
                {n: float(go[n]) for n in ("dmixture", "dquartet_scale")} if uq else {})
    yr, ref, scalars = _cached(("quartet", cfg), make)

    def check(res):
        _attn_close(res, yr, ref, "quartet")
        for n, want in scalars.items():
            assert abs(float(res[n]) - want) <= 5e-2 * max(abs(want), 1e-3), (n, float(res[n]), want)
    es = 2 if io == "bf16" else 4
    _two_runs(call, inputs, check, ("quartet_fwd",), FUSED if path == "fused" else GENERIC,
              (1 + len(names)) * [B * T * H * dh * es] + (2 * [B * H * 4] if uq else []), f"quartet {cfg} {path}")


# ------------------------------------------------------------------------------------------------ LayerNorm, token gate, MoE
LN_DTYPES = [(torch.float32, torch.float32, torch.float32), (torch.float32, torch.bfloat16, torch.float32),
             (torch.bfloat16, torch.bfloat16, torch.bfloat16)]


@pytest.mark.parametrize("xdt,ydt,pdt", LN_DTYPES, ids=["f32-f32-f32", "f32-bf16-f32", "bf16-bf16-bf16"])
@pytest.mark.parametrize("rows,dim", [(7, 64), (129, 72), (33, 1152), (5, 4096)], ids=lambda v: str(v))
def test_layernorm_residual(rows, dim, xdt, ydt, pdt):
    """ops.layernorm_residual forward and backward; reference and bounds of test_layernorm_forward_backward_vs_torch"""
    from mop_amd import ops
    from test_gpu_layernorm import _ref
    gen = torch.Generator().manual_seed(rows * 131 + dim)
    x = (torch.randn(rows, dim, generator=gen) * 1.7 + 0.3).to(xdt)
    g = (1.0 + 0.2 * torch.randn(dim, generator=gen)).to(pdt)
    b = (0.1 * torch.randn(dim, generator=gen)).to(pdt)
    dy = torch.randn(rows, dim, generator=gen).to(ydt)
    dres = torch.randn(rows, dim, generator=gen).to(xdt)
    yr, dxr, dgr, dbr = _cached(("ln", rows, dim, xdt, ydt, pdt), lambda: _ref(x.float(), g.float(), b.float(), 1e-5, dy.float(), dres.float()))

    def call(t):
        xi = t["x"]
        xres, y = ops.layernorm_residual(xi, t["g"], t["b"], 1e-5, ydt)
        torch.autograd.backward([xres, y], [t["dres"], t["dy"]])
        return dict(y=y.detach(), dx=xi.grad, dgamma=t["g"].grad, dbeta=t["b"].grad)

    def check(res):
        ytol = 1e-5 if ydt == torch.float32 else 1.6e-2
        assert (res["y"].float().cpu().double() - yr).abs().max().item() <= ytol * max(1.0, yr.abs().max().item())
        gt = 2e-5 if xdt == torch.float32 else 8e-3
        for name, ref in (("dx", dxr), ("dgamma", dgr), ("dbeta", dbr)):
            err = (res[name].float().cpu().double() - ref).abs().max().item() / max(1e-6, ref.abs().max().item())
            assert err <= gt, f"{name} {err:.2e}"
    inputs = dict(x=x.cuda().requires_grad_(True), g=g.cuda().requires_grad_(True), b=b.cuda().requires_grad_(True), dy=dy.cuda(),
                  dres=dres.cuda())
    plain = call({k: _leaf(t, False) for k, t in inputs.items()})
    torch.cuda.synchronize()
    check(plain)
    with guarded_allocations() as ledger:
        ins = {k: _leaf(t, True) for k, t in inputs.items()}
        guarded = call(ins)
        torch.cuda.synchronize()
    sizes = [_nbytes(plain["y"]), _nbytes(plain["dx"])] + 2 * [rows * 4] + 2 * [dim * 4]      # y, dx; mean, rstd; dgamma, dbeta (float32)
    _assert_guarded_equals_plain(ledger, plain, guarded, (), None, sizes, f"layernorm {rows}x{dim}")


@pytest.mark.parametrize("xdt,ydt,pdt", LN_DTYPES, ids=["f32-f32-f32", "f32-bf16-f32", "bf16-bf16-bf16"])
def test_layernorm_kernels_with_a_row_stride(xdt, ydt, pdt):
    """mopk_layernorm_fwd / _bwd with x_ld > dim and y_ld > dim, (rows, dim) = (129, 72).  ops.layernorm_residual makes x contiguous
    and always passes x_ld = y_ld = dim, so a row stride reaches the kernels through the C ABI only (as
    test_layernorm_rejects_what_the_kernel_does_not_cover builds its arguments).  x, dres and dx are the first 72 columns of
    80-wide rows, y and dy of 88-wide rows; the gaps of the inputs are NaN, those of the guarded outputs must stay unwritten.
    Reference and bounds of test_layernorm_forward_backward_vs_torch (dgamma, dbeta are the kernels' float32 values)."""
    import ctypes as C
    from mop_amd import _lib as L, ops
    from test_gpu_layernorm import _ref
    rows, dim, xld, yld = 129, 72, 80, 88
    gen = torch.Generator().manual_seed(rows * 131 + dim)
    x = (torch.randn(rows, dim, generator=gen) * 1.7 + 0.3).to(xdt)
    g = (1.0 + 0.2 * torch.randn(dim, generator=gen)).to(pdt)
    b = (0.1 * torch.randn(dim, generator=gen)).to(pdt)
    dy = torch.randn(rows, dim, generator=gen).to(ydt)
    dres = torch.randn(rows, dim, generator=gen).to(xdt)
    yr, dxr, dgr, dbr = _cached(("ln", rows, dim, xdt, ydt, pdt), lambda: _ref(x.float(), g.float(), b.float(), 1e-5, dy.float(), dres.float()))

    def run(embed):
        def wide(t, ld):
            wd = torch.full((rows, ld), float("nan"), dtype=t.dtype, device="cuda")
            wd[:, :dim] = t.cuda()
            return embedded(wd) if embed else wd
        xw, drw, dyw = wide(x, xld), wide(dres, xld), wide(dy, yld)
        gg, bb = (embedded(t.cuda()) if embed else t.cuda() for t in (g, b))
        f32 = dict(dtype=torch.float32, device="cuda")
        yw, dxw = torch.empty(rows, yld, dtype=ydt, device="cuda"), torch.empty(rows, xld, dtype=xdt, device="cuda")
        mean, rstd, dg, db = torch.empty(rows, **f32), torch.empty(rows, **f32), torch.empty(dim, **f32), torch.empty(dim, **f32)
        a = L.LayerNormArgs(rows=rows, dim=dim, x_dtype=ops._io_dtype(xw), y_dtype=ops._io_dtype(yw), p_dtype=ops._io_dtype(gg), eps=1e-5,
                            x_ld=xld, y_ld=yld, x=xw.data_ptr(), gamma=gg.data_ptr(), beta=bb.data_ptr(), y=yw.data_ptr(),
                            mean=mean.data_ptr(), rstd=rstd.data_ptr())
        ops._launch("mopk_layernorm_fwd", a)
        a.dy, a.dres, a.dx, a.dgamma, a.dbeta = dyw.data_ptr(), drw.data_ptr(), dxw.data_ptr(), dg.data_ptr(), db.data_ptr()
        ws = torch.empty(max(1, L.lib().mopk_layernorm_workspace_bytes(C.byref(a))), dtype=torch.uint8, device="cuda")
        a.workspace = ws.data_ptr()
        ops._launch("mopk_layernorm_bwd", a)
        torch.cuda.synchronize()
        return dict(y=yw[:, :dim], dx=dxw[:, :dim], dgamma=dg, dbeta=db, mean=mean, rstd=rstd), (yw[:, dim:], dxw[:, dim:])

    plain, _ = run(False)
    ytol = 1e-5 if ydt == torch.float32 else 1.6e-2
    assert (plain["y"].float().cpu().double() - yr).abs().max().item() <= ytol * max(1.0, yr.abs().max().item())
    gt = 2e-5 if xdt == torch.float32 else 8e-3
    for name, ref in (("dx", dxr), ("dgamma", dgr), ("dbeta", dbr)):
        err = (plain[name].float().cpu().double() - ref).abs().max().item() / max(1e-6, ref.abs().max().item())
        assert err <= gt, f"{name} {err:.2e}"
    with guarded_allocations() as ledger:
        guarded, gaps = run(True)
    for name, gap in zip(("y", "dx"), gaps):
        assert bool((gap.contiguous().view(torch.uint8) == 0xFF).all()), f"{name}: the kernel wrote between the rows"
    sizes = [rows * yld * _es(ydt), rows * xld * _es(xdt)] + 2 * [rows * 4] + 2 * [dim * 4]
    _assert_guarded_equals_plain(ledger, plain, guarded, (), None, sizes, "layernorm kernels, row stride")


def _es(dt):
    return 2 if dt == torch.bfloat16 else 4


TG_TILE = 16
TG_DT = {"fp32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "mixed": (torch.float32, torch.bfloat16)}


@pytest.mark.parametrize("dt,with_a", [("fp32", True), ("fp32", False), ("bf16", True), ("bf16", False), ("mixed", True)],
                         ids=["fp32-a", "fp32-no-a", "bf16-a", "bf16-no-a", "mixed-a"])      # mixed without a is fp32 without a
@pytest.mark.parametrize("D", [64, 96])
@pytest.mark.parametrize("T", [1, TG_TILE + 1, 2 * TG_TILE])
def test_token_gate(T, D, dt, with_a):
    """ops.token_gate_1d, B = 3; reference and bounds of test_token_gate_op_against_float64.  The guarded run gives the kernels x as
    rows 1..T of a (B, T + 2, D) buffer whose rows 0 and T + 1 are NaN: the taps at t - 1 and t + 1 must stop at the sequence's ends"""
    from mop_amd import ops
    from test_gpu_gpt import TILE, _inputs, _nerr, _ref64
    assert TILE == TG_TILE
    B = 3
    xdt, adt = TG_DT[dt]
    x, a, u, dout = _inputs(B, T, D, xdt, adt if with_a else None, False, seed=B * 10007 + T * 31 + D)
    odt = torch.bfloat16 if (xdt == torch.bfloat16 and (a is None or adt == torch.bfloat16)) else torch.float32
    dout = dout.to(odt)

    def call(t):
        out = ops.token_gate_1d(t["x"], t.get("a"), t["u"])
        out.backward(t["dout"])
        res = dict(out=out.detach(), dx=t["x"].grad, du=t["u"].grad)
        if with_a:
            res["da"] = t["a"].grad
        return res

    def check(res):
        ro, rdx, rdu = _ref64(x, a, u, dout)
        tol = 1e-2 if dt == "bf16" else 1e-4
        assert res["out"].dtype == odt
        assert _nerr(res["out"], ro) <= tol and _nerr(res["dx"], rdx) <= tol and _nerr(res["du"], rdu) <= tol
        if with_a:
            assert res["da"].dtype == adt and _nerr(res["da"], rdx) <= (1e-2 if adt == torch.bfloat16 else 1e-4)
    inputs = dict(x=x.requires_grad_(True), u=u.requires_grad_(True), dout=dout)
    if with_a:
        inputs["a"] = a.requires_grad_(True)
    plain = call({k: _leaf(t, False) for k, t in inputs.items()})
    torch.cuda.synchronize()
    check(plain)
    with guarded_allocations() as ledger:
        ins = {k: _leaf(t, True) for k, t in inputs.items()}
        rows = torch.full((B, T + 2, D), float("nan"), dtype=xdt, device="cuda")
        rows[:, 1:T + 1] = x.detach()
        ins["x"] = embedded(rows)[:, 1:T + 1].detach().requires_grad_(True)
        assert T == 1 or ins["x"].stride(0) == (T + 2) * D
        guarded = call(ins)
        torch.cuda.synchronize()
    es = 2 if odt == torch.bfloat16 else 4
    sizes = 2 * [B * T * D * es] + [B * T * 4, 3 * D * 4]           # out and dr, the saved gate, du
    _assert_guarded_equals_plain(ledger, plain, guarded, ("token_gate_fwd", "token_gate_bwd"), FUSED, sizes,
                                 f"token gate T={T} D={D} {dt} a={with_a}")


MOE = [(1, 72, 288, 4, False, "fp32", False), (63, 72, 288, 4, True, "bf16", True), (65, 8, 32, 8, False, "bf16", True),
       (129, 384, 1536, 2, True, "fp32", False), (128, 8, 64, 64, False, "fp32", True)]


@pytest.mark.parametrize("M,D,F_,E,skew,mode,with_res", MOE, ids=lambda v: str(v))
def test_moe_mlp(M, D, F_, E, skew, mode, with_res):
    """ops.moe_mlp on rows of test_gpu_moe.SWEEP (experts without a token, every token in one expert, M on and off the 64- and
    128-row tile edges); reference and bounds of test_moe_op_sweep_vs_float64"""
    from mop_amd import ops
    from test_gpu_moe import SWEEP, _case, _ref64
    assert (M, D, F_, E, skew, mode, with_res) in SWEEP
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, gw, gb, w1s, w2s, dy, res_ = _case(M, D, F_, E, skew, 0, dtype=dt)
    inputs = dict(x=x.requires_grad_(True), gw=gw, gb=gb, dy=dy.to(dt))
    inputs.update({f"w1.{e}": w for e, w in enumerate(w1s)})
    inputs.update({f"w2.{e}": w for e, w in enumerate(w2s)})
    if with_res:
        inputs["res"] = res_.to(dt).requires_grad_(True)

    def call(t):
        y = ops.moe_mlp(t["x"], t["gw"], t["gb"], [t[f"w1.{e}"] for e in range(E)], [t[f"w2.{e}"] for e in range(E)], residual=t.get("res"))
        y.backward(t["dy"])
        out = dict(y=y.detach(), dx=t["x"].grad)
        out.update({f"w1.{e}": t[f"w1.{e}"].grad for e in range(E)})
        out.update({f"w2.{e}": t[f"w2.{e}"].grad for e in range(E)})
        if with_res:
            out["dres"] = t["res"].grad
        return out

    def check(out):
        route = ops.moe_route(x, gw, gb)
        if skew:
            assert bool((route == E - 1).all())
        y64, dx64, dw1, dw2 = _ref64(x.detach(), gw, gb, [w.detach() for w in w1s], [w.detach() for w in w2s], route, dy.to(dt),
                                     res_.to(dt) if with_res else None)
        tol = 2e-5 if mode == "fp32" else 2e-2
        yv = out["y"].double().reshape(y64.shape)
        assert float((yv - y64).abs().max()) <= tol * max(1.0, float(y64.abs().max())), f"y {float((yv - y64).abs().max()):.3e}"
        got, ref = {"dx": out["dx"].double().reshape(dx64.shape)}, {"dx": dx64}
        for e in range(E):
            got[f"w1.{e}"], ref[f"w1.{e}"] = out[f"w1.{e}"].double(), dw1[e]
            got[f"w2.{e}"], ref[f"w2.{e}"] = out[f"w2.{e}"].double(), dw2[e]
        check_grads({k: v.cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in ref.items()},
                    1e-4 if mode == "fp32" else 3e-2)
        if with_res:
            assert torch.equal(out["dres"], dy.to(dt))
        for e in set(range(E)) - set(route.tolist()):
            assert not bool(out[f"w1.{e}"].any()) and not bool(out[f"w2.{e}"].any())
    es = 2 if mode == "bf16" else 4
    sizes = 2 * [M * D * es] + 2 * [M * F_ * es] + 2 * E * [F_ * D * es] + [(2 * M + E + 1) * 4]     # y, dx; u, h; dW1_e, dW2_e; route
    _two_runs(call, inputs, check, ("moe_fwd", "moe_bwd"), FUSED, sizes, f"moe M={M} D={D} F={F_} E={E} skew={skew} {mode}")


# ------------------------------------------------------------------------------------------------ decode attention (forward only)
@pytest.mark.parametrize("op", ["decode_attention", "decode_attention_rows", "decode_attention_ragged", "decode_attention_lens"])
@pytest.mark.parametrize("io", ["bf16", "fp32"])
@pytest.mark.parametrize("dk", [32, 64, 128])
def test_decode_attention(dk, io, op):
    """the split-KV kernels (partials in a workspace), B = 3, H = 2, a cache of 300 rows of which 261 are filled, Tq = 5; in the guarded
    run every cache entry beyond the fill, beyond a row's kv_lens, before its kv_start or never named by the row table is NaN; the per-row
    values (kv_lens, kv_start) are 1, one inside a split and one on a split's edge, as in test_decode_attention_lens_matches_float64.
    References and bounds: the float64 loops of test_whisper_ragged_cpu / test_whisper_audio_lens_cpu; max-abs / max|ref| <= 1e-5 /
    1e-2 for decode_attention and _rows (test_op_sweep_vs_float64, test_rows_attention_vs_float64_gather), max-abs <= 2e-5 / 2e-2
    for _ragged and _lens (test_attention_matches_float64, test_decode_attention_lens_matches_float64)"""
    from mop_amd import ops
    from test_whisper_audio_lens_cpu import naive_lens_attention
    from test_whisper_ragged_cpu import naive_ragged_attention
    dt = torch.float32 if io == "fp32" else torch.bfloat16
    B, H, cap, nk, Tq = 3, 2, 300, 261, 5
    chunk = min(32768 // (dk * (4 if io == "fp32" else 2)), 128)
    g = torch.Generator(device="cuda").manual_seed(dk)
    k = torch.randn(B, cap, H, dk, device="cuda", generator=g).to(dt)
    v = torch.randn(B, cap, H, dk, device="cuda", generator=g).to(dt)
    q = torch.randn(B, Tq, H, dk, device="cuda", generator=g).to(dt)
    per_row = torch.tensor([1, 37, chunk], dtype=torch.int32, device="cuda")
    j = torch.arange(cap, device="cuda").unsqueeze(0)

    def reached(start):
        """(B, cap) bool: cache entries (row, position) some query row reads through the table, positions start[b] <= j < nk"""
        vis = torch.zeros(B, cap, dtype=torch.bool, device="cuda")
        m = (j >= start.view(B, 1)) & (j < nk)
        vis[rows[:, :cap].long()[m], j.expand(B, cap)[m]] = True
        return vis
    kv_len = torch.tensor([nk], dtype=torch.int32, device="cuda")
    rows = torch.randint(0, B, (B, cap + 7), device="cuda", generator=g, dtype=torch.int32)
    inputs = dict(q=q, k=k, v=v)
    key = {"decode_attention": "decode_attn", "decode_attention_rows": "decode_attn_rows", "decode_attention_ragged": "decode_attn_ragged",
           "decode_attention_lens": "decode_attn_lens"}[op]
    cpu = lambda t: t.cpu().float()       # noqa: E731
    zero = torch.zeros(B, dtype=torch.int32)
    if op == "decode_attention":
        visible = (j < nk).expand(B, cap)
        inputs.update(kv_len=kv_len)
        call = lambda t: dict(y=ops.decode_attention(t["q"], t["k"], t["v"], kv_len=t["kv_len"], causal=True))          # noqa: E731
        ref = lambda: naive_ragged_attention(cpu(q), cpu(k), cpu(v), zero, None, nk, True)                             # noqa: E731
    elif op == "decode_attention_rows":
        visible = reached(torch.zeros_like(per_row))
        inputs.update(kv_len=kv_len, rows=rows)
        call = lambda t: dict(y=ops.decode_attention_rows(t["q"], t["k"], t["v"], t["rows"], kv_len=t["kv_len"], causal=True))   # noqa: E731
        ref = lambda: naive_ragged_attention(cpu(q), cpu(k), cpu(v), zero, rows.cpu(), nk, True)                       # noqa: E731
    elif op == "decode_attention_ragged":
        visible = reached(per_row)
        inputs.update(kv_len=kv_len, rows=rows, kv_start=per_row)
        call = lambda t: dict(y=ops.decode_attention_ragged(t["q"], t["k"], t["v"], t["kv_start"], rows=t["rows"], kv_len=t["kv_len"],   # noqa: E731
                                                            causal=True))
        ref = lambda: naive_ragged_attention(cpu(q), cpu(k), cpu(v), per_row.cpu(), rows.cpu(), nk, True)              # noqa: E731
    else:
        visible = j < per_row.view(B, 1)
        inputs.update(kv_lens=per_row)
        call = lambda t: dict(y=ops.decode_attention_lens(t["q"], t["k"], t["v"], t["kv_lens"], nk=nk))                # noqa: E731
        ref = lambda: naive_lens_attention(cpu(q), cpu(k)[:, :nk], cpu(v)[:, :nk], None, per_row.cpu())                # noqa: E731
    yr = _cached((op, dk, io), ref)

    def check(res):
        err = float((res["y"].cpu().double() - yr).abs().max())
        if op in ("decode_attention", "decode_attention_rows"):
            assert err / float(yr.abs().max()) <= (1e-5 if io == "fp32" else 1e-2), err
        else:
            assert err <= (2e-5 if io == "fp32" else 2e-2), err

    def poison(t):                       # the guarded run's cache is NaN wherever no query may look
        assert 0 < int(visible.sum()) < B * cap
        t["k"][~visible] = float("nan")
        t["v"][~visible] = float("nan")
    _two_runs(call, inputs, check, (key,), FUSED, [B * Tq * H * dk * (4 if io == "fp32" else 2)], f"{op} dk={dk} {io}", poison=poison)
