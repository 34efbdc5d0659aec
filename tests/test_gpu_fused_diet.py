"""The fused Edgewise kernels at the shapes where their vector-instruction diet could go wrong: the NT = 7 / dk = 64 code at N = 193 (one
valid query and key in the last tile), 197, 208 (the ctrim / klast boundary) and 224 (no padding), float32 and bfloat16 I/O, against the
float64 oracle and against the generic path; the separate-tensor epilogue of launch A and strided q / k / v / dy views through the C ABI;
one small instantiation; and a forward whose chain product underflows to exactly 0, so that log(C + eps) is taken at eps itself.

Bounds are the suite's own (test_gpu_edgewise.py): 1e-2 max-abs on y and 3e-2 relative on gradients for bf16 arithmetic, a gradient tensor
that bf16 cannot resolve being held to 4 x the amount the exact gradient moves when the inputs are rounded to bf16 (gpu_util).  With
bfloat16 I/O the output itself is rounded once more: half a bf16 ulp of the largest |y| is added to the bound on y."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_util import check_grads, max_abs, oracle_bf16_noise, rel_err, run_fwd_bwd

pytestmark = pytest.mark.gpu

TOL_BF16, GTOL_BF16 = 1e-2, 3e-2
TOL_GENERIC = 1e-4                # the generic path (fp32 arithmetic) against the oracle, as test_edgewise_vs_oracle_seeded holds it
B, H, V, R = 2, 2, 5, 4


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _module(D, heads, share, seed):
    from mop_amd.nn import EdgewiseMSA
    torch.manual_seed(seed)
    m = EdgewiseMSA(D, heads, n_views=V, share_qkv=share, gate_mode="lowrank", gate_rank=R, gate_init="mix5")
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("_scale"):
                p.add_(0.1 * torch.randn_like(p))
            elif "edge_head" in n_ and n_.endswith("weight"):
                p.mul_(3.0)
        m.chain_value_logit.fill_(-0.5)
    return m


@functools.lru_cache(maxsize=None)
def _case(N, dk, share):
    """module, inputs, the oracle's outputs and its bf16 noise floor, the generic path's outputs: computed once per (N, dk, share)"""
    from oracle import edgewise as oe
    import mop_amd
    from mop_amd import ops, _lib
    D = H * dk
    m = _module(D, H, share, seed=1000 * N + dk)
    params = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, N, D, generator=g).numpy()
    w = torch.randn(B, N, D, generator=g).numpy()
    out, cache = oe.module_fwd(x.astype(np.float64), params, H, V, share, 0.5)
    dx_ref, g_ref = oe.module_bwd(w.astype(np.float64), cache)
    noise = oracle_bf16_noise(oe.module_fwd, oe.module_bwd, x, w, params, H, V, share, 0.5, samples=2)
    mop_amd.set_precision("fp32")
    ops.set_path("generic")
    generic = run_fwd_bwd(m.cuda().eval(), x, w)
    assert ops.LAST_PATH["edgewise_fwd"] == _lib.PATH_GENERIC
    m.zero_grad()
    mop_amd.set_precision("auto")
    ops.set_path("auto")
    return m, x, w, out, dx_ref, g_ref, noise, generic


def _check(N, dk, share, dtype, fused):
    import mop_amd
    from mop_amd import ops, _lib
    m, x, w, out, dx_ref, g_ref, noise, (y_g, dx_g, grads_g) = _case(N, dk, share)
    # the generic path first: it is the second reference, so it has to stand on the oracle itself
    assert max_abs(y_g, out) <= TOL_GENERIC and rel_err(dx_g, dx_ref) <= 1e-3
    mop_amd.set_precision("bf16")
    y, dx, grads = run_fwd_bwd(copy.deepcopy(m), x, w, dtype=dtype)      # a copy: a bfloat16 run rounds the module's parameters in place
    path = _lib.PATH_FUSED if fused else _lib.PATH_GENERIC
    assert ops.LAST_PATH["edgewise_fwd"] == path and ops.LAST_PATH["edgewise_bwd"] == path
    ytol = TOL_BF16 + (2.0 ** -9 * float(np.abs(out).max()) if dtype == torch.bfloat16 else 0.0)
    print(f"N={N} dk={dk} share={share} {dtype}: y {max_abs(y, out):.3e} (generic {max_abs(y, y_g):.3e}) dx {rel_err(dx, dx_ref):.3e} "
          f"(generic {rel_err(dx, dx_g):.3e})")
    assert max_abs(y, out) <= ytol
    assert max_abs(y, y_g) <= ytol + TOL_GENERIC
    assert rel_err(dx, dx_ref) <= GTOL_BF16
    assert rel_err(dx, dx_g) <= GTOL_BF16 + 1e-3
    check_grads(grads, g_ref, GTOL_BF16, d=noise)
    check_grads(grads, {k: np.asarray(v, np.float64).reshape(g_ref[k].shape) for k, v in grads_g.items()}, GTOL_BF16 + 1e-3, d=noise)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [193, 197, 208, 224])
def test_fused_nt7_dk64_vs_oracle_and_generic(N, dtype):
    """share_qkv layer: v0 and vL are one tensor, launch A's epilogue writes dv0 + dvL to one place (its `same` path)"""
    _check(N, 64, True, dtype, fused=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_small_instantiation_vs_oracle_and_generic(dtype):
    """N = 33, dk = 16 (NT = 2): the helpers are shared by every instantiation"""
    _check(33, 16, True, dtype, fused=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unshared_layer_vs_oracle(dtype):
    """share_qkv=False: per-view q / k, which the fused kernels do not take -- the layer runs on the generic path (the fused kernels'
    separate dv0 / dvL epilogue is reached through the C ABI below)"""
    _check(197, 64, False, dtype, fused=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the core through the C ABI: v0 / vL and dv0 / dvL as separate tensors, q / k / v / dy / dq / dk / dv as padded (strided) views
# ---------------------------------------------------------------------------------------------------------------------------------
def _core_abi(q, k, v0, vL, dy, small, head, dtype, pad, same):
    """One forward + backward of the fused low-rank core on (B,N,H,dk) tensors.  pad: every tensor lives in a larger allocation, so batch,
    token and head strides all differ from the packed ones.  same: v0 and vL (dv0 and dvL) are ONE tensor.  Returns y, dq, dk, dv0, dvL
    and the per-(b,h) partial sums of the value-scale gradients as float32 numpy arrays."""
    from mop_amd import _lib as L, ops
    lib = L.lib()
    Bq, N, Hh, dk = q.shape

    def place(t):
        t = t.to(dtype)
        if not pad:
            return t.contiguous()
        big = torch.zeros(Bq + 1, N + 3, Hh + 1, dk + 8, dtype=dtype, device="cuda")
        view = big[:Bq, 1:N + 1, :Hh, 8:]
        view.copy_(t)
        return view

    def v4(t):
        return L.View4(t.data_ptr(), t.stride(0), t.stride(2), t.stride(1))

    def v5(t):
        return L.View5(t.data_ptr(), 0, t.stride(0), t.stride(2), t.stride(1))
    tq, tk, tv0, tdy = place(q), place(k), place(v0), place(dy)
    tvL = tv0 if same else place(vL)
    y, dq, dk_, dv0 = (place(torch.zeros_like(q)) for _ in range(4))
    dvL = dv0 if same else place(torch.zeros_like(q))
    a = L.EdgewiseArgs()
    a.B, a.H, a.N, a.dk, a.V, a.r = Bq, Hh, N, dk, V, R
    a.io_dtype, a.precision, a.path, a.beta_not = ops._io_dtype(tq), L.PREC_BF16, L.PATH_FUSED, 0.5
    a.q, a.k, a.v0, a.vL, a.y = v5(tq), v5(tk), v4(tv0), v4(tvL), v4(y)
    a.sqk, a.vs0, a.vsL, a.chain_logit = (t.data_ptr() for t in small)
    a.Wr, a.br, a.Wc, a.bc = (t.data_ptr() for t in head)
    a.save_for_backward = 1
    assert lib.mopk_edgewise_fused_supported(C.byref(a))
    saved = ops._bytes(lib.mopk_edgewise_saved_bytes(C.byref(a)), "cuda")
    ws = ops._bytes(256, "cuda")
    a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
    ops._launch("mopk_edgewise_lowrank_fwd", a)
    a.dy, a.dq, a.dk_, a.dv0, a.dvL = v4(tdy), v5(dq), v5(dk_), v4(dv0), v4(dvL)
    n_sqk, n_vs, n_w = V * Hh * dk, Hh * dk, 4 * R * (2 * V + 2)
    parts = torch.zeros(Bq * (n_sqk + 2 * n_vs + Hh), dtype=torch.float32, device="cuda")
    p_sqk, p_vs0, p_vsL, p_lg = torch.split(parts, [Bq * n_sqk, Bq * n_vs, Bq * n_vs, Bq * Hh])
    hg = torch.zeros(2 * n_w + 8 * R, dtype=torch.float32, device="cuda")
    g_wr, g_br, g_wc, g_bc = torch.split(hg, [n_w, 4 * R, n_w, 4 * R])
    a.dsqk_part, a.dvs0_part, a.dvsL_part, a.dlogit_part = (t.data_ptr() for t in (p_sqk, p_vs0, p_vsL, p_lg))
    a.dWr, a.dbr, a.dWc, a.dbc = (t.data_ptr() for t in (g_wr, g_br, g_wc, g_bc))
    ws2 = ops._bytes(lib.mopk_edgewise_workspace_bytes(C.byref(a)), "cuda")
    a.workspace = ws2.data_ptr()
    ops._launch("mopk_edgewise_lowrank_bwd", a)
    torch.cuda.synchronize()
    return tuple(t.detach().float().cpu().numpy() for t in (y, dq, dk_, dv0, dvL, p_vs0.view(Bq, Hh, dk), p_vsL.view(Bq, Hh, dk)))


@functools.lru_cache(maxsize=None)
def _abi_inputs(N, dk):
    g = torch.Generator().manual_seed(7 * N + dk)
    rb = lambda *s: torch.randn(*s, generator=g).bfloat16().float()      # bf16-representable: both I/O types read the same numbers
    q, k, v0, vL, dy = (rb(B, N, H, dk) for _ in range(5))
    C_ = 2 * V + 2
    small = (torch.full((V, H, dk), dk ** -0.5) * (1 + 0.1 * torch.randn(V, H, dk, generator=g)), 1 + 0.1 * torch.randn(H, dk, generator=g),
             1 + 0.1 * torch.randn(H, dk, generator=g), torch.tensor([-0.5]))
    head = (0.3 * torch.randn(4 * R, C_, generator=g), 0.1 * torch.randn(4 * R, generator=g),
            0.3 * torch.randn(4 * R, C_, generator=g), 0.1 * torch.randn(4 * R, generator=g))
    return q, k, v0, vL, dy, small, head


@functools.lru_cache(maxsize=None)
def _abi_oracle(N, dk, same):
    from edgewise_peaks import core_oracle                               # the oracle in the core's layouts, stated once
    q, k, v0, vL, dy, small, head = _abi_inputs(N, dk)
    f = lambda t: t.numpy().astype(np.float64)
    sqk, vs0, vsL, lg = map(f, small)
    o = core_oracle(f(q), f(k), f(v0), f(v0 if same else vL), f(dy), sqk, vs0, vsL, float(lg[0]), tuple(map(f, head)), 0.5)
    return o["y"], o["dq"], o["dk"], o["dv0"], o["dvL"], o["dvs0_bh"], o["dvsL_bh"]   # the last two per (b,h): d/d vs0, d/d vsL


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("N", [193, 208])
def test_core_abi_strided_views_and_separate_value_tensors(N, same, dtype):
    """packed and padded layouts give the same bits; both agree with the oracle.  same=False is launch A's separate dv0 / dvL epilogue."""
    ins = _abi_inputs(N, 64)
    packed = _core_abi(*[t.cuda() for t in ins[:5]], [t.cuda().contiguous() for t in ins[5]], [t.cuda().contiguous() for t in ins[6]],
                       dtype, pad=False, same=same)
    padded = _core_abi(*[t.cuda() for t in ins[:5]], [t.cuda().contiguous() for t in ins[5]], [t.cuda().contiguous() for t in ins[6]],
                       dtype, pad=True, same=same)
    names = ("y", "dq", "dk", "dv0", "dvL", "dvs0_part", "dvsL_part")
    for n_, a_, b_ in zip(names, packed, padded):
        assert np.array_equal(a_, b_), f"{n_}: the padded layout changes the result"
    ref = _abi_oracle(N, 64, same)
    for n_, got, want in zip(names, packed, ref):
        if n_ == "dv0" and same:
            want = want + ref[4]                                         # one tensor receives both value gradients
        if n_ == "dvL" and same:
            continue
        # every tensor relative to its largest magnitude, y included: the core's raw output is O(1) here (standard-normal values, no
        # output projection), where the suite's absolute 1e-2 -- set for module outputs of about 0.1 -- would be a third of the relative
        # bound the gradients are held to; bfloat16 I/O rounds each result once more (half an ulp = 2^-9 relative)
        err = rel_err(got, want)
        lim = GTOL_BF16 + (2.0 ** -9 if dtype == torch.bfloat16 else 0.0)
        print(f"N={N} same={same} {dtype} {n_}: {err:.3e} (max |ref| {float(np.abs(want).max()):.3e})")
        assert err <= lim, f"{n_}: {err:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# chain product that underflows to exactly 0: log(C + eps) at eps itself
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False])
def test_forward_where_the_chain_product_underflows_to_zero(train):
    """Tokens fall into 64 classes; q and k are 40 x the class's unit vector, so every view's score is 200 inside a class and 0 across
    classes: the per-view softmax weights across classes are e^-200 (0 in float32 and in bf16) and C->[i, j] is EXACTLY 0 for every
    cross-class pair -- log(C + eps) = log(1e-6) there, in the chain epilogue's row means and in the mix loop.  The gates are set so
    that the logarithms decide the output: G_and = G_or = 0 and G_not = 1 with beta_not = 1 cancel the scores (all views score alike), which
    leaves Smix = G_chain log(C + eps) with G_chain = sigmoid(0.25 + 0.1 rowmean(log C->)), about 0.25: most of the probability mass
    sits on cross-class keys, whose weight is e^(G_chain log eps).
    train: the record-exporting forward of a training step (the benchmark's instantiation) or the inference forward."""
    from oracle import edgewise as oe
    import mop_amd
    from mop_amd import ops, _lib
    from mop_amd.nn import EdgewiseMSA
    N, D = 197, 64
    g = torch.Generator().manual_seed(3)
    m = EdgewiseMSA(D, 1, n_views=V, share_qkv=True, gate_mode="lowrank", gate_rank=R, beta_not=1.0)
    with torch.no_grad():
        # every view scores alike (q_scale = k_scale = 1), so O = (V - 1) S_0 and S_0 - G_not nb O = 0 at G_not = 1, nb = beta_not / (V - 1)
        m.q_scale.fill_(1.0); m.k_scale.fill_(1.0); m.v_scale.fill_(1.0)
        eye = torch.eye(D)
        vmat = (2 * torch.rand(D, D, generator=g) - 1).bfloat16().float()
        m.qkv.weight.copy_(torch.cat([40.0 * eye, 40.0 * eye, vmat]))
        m.proj.weight.copy_(eye)
        for proj, bias in ((m.edge_head.row_proj, (-20.0, -20.0, 20.0, 0.25)), (m.edge_head.col_proj, (1.0, 1.0, 1.0, 1.0))):
            proj.weight.zero_(); proj.bias.zero_()
            for gate, b_ in enumerate(bias):
                proj.bias[gate * R] = b_                       # Z_g = a_g0 b_g0: a constant per gate ...
        m.edge_head.row_proj.weight[3 * R, 2 * V, 0] = 0.1     # ... but the chain gate, which reads the row mean of log C->
        m.chain_value_logit.fill_(-0.5)
    x = torch.zeros(1, N, D)
    x[0, torch.arange(N), torch.arange(N) % D] = 1.0
    params = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    out, cache = oe.module_fwd(x.numpy().astype(np.float64), params, 1, V, True, 1.0)
    cross = (np.arange(N)[:, None] % D) != (np.arange(N)[None, :] % D)
    assert np.abs(cache["Cr"][0, 0][cross] - np.log(1e-6)).max() < 1e-9      # the oracle's log(C + eps) is log(eps) there
    assert 0.5 < (cache["P"][0, 0] * cross).sum(-1).min()                     # ... and those entries carry most of the attention
    mop_amd.set_precision("bf16")
    m = m.cuda().eval()
    xt = x.cuda().requires_grad_(train)
    with torch.set_grad_enabled(train):
        y = m(xt).detach().float().cpu().numpy()
    assert ops.LAST_PATH["edgewise_fwd"] == _lib.PATH_FUSED
    print(f"train={train}: y {max_abs(y, out):.3e} of max |y| {np.abs(out).max():.3e}")
    assert np.isfinite(y).all()
    assert max_abs(y, out) <= TOL_BF16
