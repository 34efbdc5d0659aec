"""The small-parameter prologue / epilogue kernels of a share_qkv EdgewiseMSA layer (mopk_edgewise_params_fwd / _bwd, reached
through ops.edgewise_lowrank_core_shared) against the tensor expressions they replace: `edgewise_lowrank_core` fed with
`(q_scale * k_scale).squeeze(2) / sqrt(dk)`, `v_scale[0, :, 0]`, `v_scale[V - 1, :, 0]` and the head's parameters, with autograd
doing the chain rule.  The kernels restate the same roundings and the same summation order, so the comparison is torch.equal:
no tolerance."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, R, B = 64, 2, 4, 19           # dk = 32; B = 19: the 16 batch slices of the reduction hold one or two rows each
SMALL = ("q_scale", "k_scale", "v_scale", "edge_head.row_proj.weight", "edge_head.row_proj.bias", "edge_head.col_proj.weight",
         "edge_head.col_proj.bias", "chain_value_logit")


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _layer(V, dtype):
    from mop_amd.nn import EdgewiseMSA
    torch.manual_seed(7)
    m = EdgewiseMSA(D, H, n_views=V, share_qkv=True, gate_mode="lowrank", gate_rank=R, gate_init="mix5")
    with torch.no_grad():           # distinct views, live gates, a chain logit that is not a round number
        for n, p in m.named_parameters():
            if n.endswith("_scale"):
                p.add_(0.1 * torch.randn_like(p))
            elif "edge_head" in n:
                p.add_(0.3 * torch.randn_like(p))
        m.chain_value_logit.add_(0.37)
    return m.cuda().to(dtype)


def _forward_by_expressions(m, x):
    """EdgewiseMSA.forward of the plain share_qkv low-rank layer written with tensor expressions around edgewise_lowrank_core"""
    from mop_amd import ops
    Bx, N, _ = x.shape
    V, dk, eh = m.n_views, m.dk, m.edge_head
    qkv = m.qkv(x).view(Bx, N, 1, 3, m.h, dk)
    sqk = (m.q_scale * m.k_scale).squeeze(2) * (1.0 / math.sqrt(dk))
    vs0, vsL = m.v_scale[0, :, 0], m.v_scale[V - 1, :, 0]
    y = ops.edgewise_lowrank_core(qkv, sqk, vs0, vsL, eh.row_proj.weight.squeeze(-1), eh.row_proj.bias,
                                  eh.col_proj.weight.squeeze(-1), eh.col_proj.bias, m.chain_value_logit, float(m.beta_not), V)
    return m._project(y, None)


def _run(m, fwd, x0, w):
    for p in m.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    y = fwd(x)
    y.backward(w)
    torch.cuda.synchronize()
    return y.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("N", [6, 65, 197])
@pytest.mark.parametrize("V", [2, 3, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_shared_parameter_kernels_match_the_tensor_expressions_bitwise(dtype, V, N, path, monkeypatch):
    import mop_amd
    from mop_amd import _lib, ops
    ops.set_path(path)
    if path == "fused":             # the fused kernels are the bf16-MFMA arithmetic, for float32 tensors too
        mop_amd.set_precision("bf16")
    m = _layer(V, dtype)
    g = torch.Generator(device="cuda").manual_seed(11)
    x0 = torch.randn(B, N, D, device="cuda", dtype=dtype, generator=g)
    w = torch.randn(B, N, D, device="cuda", dtype=dtype, generator=g)

    calls = []
    real = ops.edgewise_lowrank_core_shared
    monkeypatch.setattr(ops, "edgewise_lowrank_core_shared", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    y, dx, grads = _run(m, m, x0, w)
    assert calls == [1], "EdgewiseMSA.forward did not take edgewise_lowrank_core_shared"
    want = _lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC
    assert ops.LAST_PATH["edgewise_fwd"] == want and ops.LAST_PATH["edgewise_bwd"] == want
    y_ref, dx_ref, grads_ref = _run(m, lambda x: _forward_by_expressions(m, x), x0, w)
    assert calls == [1]

    assert torch.equal(y, y_ref)
    assert torch.equal(dx, dx_ref)
    assert set(grads) == set(grads_ref)
    for n in grads_ref:
        assert grads[n] is not None and grads[n].dtype == dtype and grads[n].shape == grads_ref[n].shape, n
        assert torch.equal(grads[n], grads_ref[n]), f"{n}: max-abs difference {(grads[n].float() - grads_ref[n].float()).abs().max().item():.3e}"
    assert not bool(grads["v_scale"][1:V - 1].any()), "rows 1 .. V-2 of v_scale.grad must be zero"
    assert bool(grads["q_scale"].float().abs().max() > 0) and bool(grads["edge_head.row_proj.weight"].float().abs().max() > 0)
    for n in SMALL:                 # each gradient is a tensor of its own, so autograd kept it without a copy
        t = grads[n]
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size(), f"{n}.grad does not own its storage"
