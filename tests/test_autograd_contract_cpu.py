"""The parts of the autograd contract (tests/test_gpu_autograd_contract.py) that need no GPU: the gradient-intake helper every
kernel-backed backward takes its incoming gradients through, the once_differentiable mark on those backwards, and the two linear
Functions of mop_amd/nn/linear.py, which are plain torch and must keep a correct second derivative."""
import inspect

import pytest
import torch
import torch.nn.functional as F


def _off_boundary(t):
    n = t.numel()
    u = torch.empty(n + 1, dtype=t.dtype)[1:1 + n].view(t.shape)
    u.copy_(t)
    return u


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_grad_in_passes_a_good_gradient_on_and_copies_the_rest(dtype):
    """contiguous, of the core's dtype and on a 16-byte boundary: the same object (viewed as the kernels' shape without a copy);
    stride 0, sliced from a wider buffer, another dtype, one element off the boundary: a contiguous aligned copy of the same values"""
    from mop_amd.ops import _grad_in
    g = torch.Generator().manual_seed(0)
    good = torch.randn(3, 10, 8, generator=g).to(dtype)
    assert good.data_ptr() % 16 == 0
    assert _grad_in(good, dtype) is good and _grad_in(good, dtype, good.shape) is good
    v = _grad_in(good, dtype, (3, 10, 2, 4))
    assert v.data_ptr() == good.data_ptr() and v.shape == (3, 10, 2, 4)
    wide = torch.randn(3, 10, 16, generator=g).to(dtype)
    other = torch.float32 if dtype == torch.bfloat16 else torch.float64
    odd = {"stride 0": torch.ones((), dtype=dtype).expand(3, 10, 8),
           "sliced": wide[..., :8],
           "another dtype": good.to(other),
           "off the boundary": _off_boundary(good)}
    assert odd["off the boundary"].is_contiguous() and odd["off the boundary"].data_ptr() % 16 != 0
    assert odd["off the boundary"].contiguous() is odd["off the boundary"]          # what every backward used to rely on
    assert not odd["sliced"].is_contiguous() and odd["stride 0"].stride() == (0, 0, 0)
    for what, t in odd.items():
        for shape in (None, (30, 8), (-1, 8)):
            out = _grad_in(t, dtype, shape)
            assert out.dtype == dtype and out.is_contiguous() and out.data_ptr() % 16 == 0, what
            assert out.shape == (t.shape if shape is None else (30, 8)), what
            assert torch.equal(out.reshape(t.shape), t.to(dtype)), what
            assert out.data_ptr() != t.data_ptr(), what


def test_every_kernel_backed_backward_is_once_differentiable_and_uses_grad_in():
    """the Functions of mop_amd/ops.py launch kernels whose outputs carry no graph: each backward is marked once_differentiable (a
    second differentiation raises instead of contributing nothing) and takes its gradients through _grad_in, none through a
    `.contiguous()` of its own"""
    from mop_amd import ops
    fns = [v for v in vars(ops).values() if inspect.isclass(v) and issubclass(v, torch.autograd.Function) and v.__module__ == ops.__name__]
    assert len(fns) == 12, sorted(f.__name__ for f in fns)
    plain = torch.autograd.Function.backward
    for fn in fns:
        src = inspect.getsource(fn.backward)
        assert fn.backward is not plain and "once_differentiable" in src.split("def backward")[0], fn.__name__
        body = src + (inspect.getsource(ops._ew_lowrank_bwd) if "_ew_lowrank_bwd" in src else "")
        assert "_grad_in(" in body, fn.__name__
        assert "dy.contiguous()" not in body and "dout.to(" not in body and "dy.reshape(" not in body, fn.__name__


def test_once_differentiable_raises_for_a_gradient_of_ones_too():
    """torch's once_differentiable hangs its error on the outputs only when an incoming gradient requires grad; y.sum() hands the
    backward a constant, and the kernels' gradient still depends on the saved inputs: ops._once_differentiable raises there as well,
    and changes nothing without create_graph"""
    from mop_amd.ops import _once_differentiable

    class Square(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            y = torch.empty_like(x)                 # as the kernels' outputs: no graph
            torch.mul(x, x, out=y)
            return y

        @staticmethod
        @_once_differentiable
        def backward(ctx, dy):
            assert not torch.is_grad_enabled()
            (x,) = ctx.saved_tensors
            return 2 * x * dy

    x = torch.arange(4.0, requires_grad=True)
    (g,) = torch.autograd.grad(Square.apply(x).sum(), x)
    assert torch.equal(g, 2 * x.detach()) and not g.requires_grad
    for loss in (lambda y: y.sum(), lambda y: (y ** 2).sum()):
        (g,) = torch.autograd.grad(loss(Square.apply(x)), x, create_graph=True)
        assert g.requires_grad
        with pytest.raises(RuntimeError, match="once_differentiable"):
            (g ** 2).sum().backward()


def _second_order(fn, ref, leaves):
    """d/d(leaves) of sum(|grad of sum(y^2) wrt leaves|^2) through fn and through ref, float64"""
    out = []
    for f in (fn, ref):
        t = [v.detach().clone().requires_grad_(True) for v in leaves]
        y = f(*t)
        g = torch.autograd.grad((y ** 2).sum(), t, create_graph=True)
        assert all(x.requires_grad for x in g)
        out.append((y.detach(), [x.detach() for x in g], torch.autograd.grad(sum((x ** 2).sum() for x in g), t)))
    return out


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("rows", [6, 4096], ids=["one-gemm", "sliced-weight-gradient"])
def test_linear_functions_first_and_second_derivatives(rows):
    """_ResidualLinearFn and _TokenLinearFn are torch ops on saved tensors: gradients of gradients must be those of F.linear, in
    float64 to 1e-10 relative (4096 rows: the weight gradient as a batched GEMM over row slices)"""
    from mop_amd.nn.linear import _ResidualLinearFn, _TokenLinearFn, weight_grad_splits
    assert weight_grad_splits(rows, 5) == (32 if rows == 4096 else 1)
    g = torch.Generator().manual_seed(rows)
    x, w, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((2, rows // 2, 7), (5, 7), (5,)))
    res = torch.randn(2, rows // 2, 5, generator=g, dtype=torch.float64)
    cases = [("token", lambda x_, w_, b_: _TokenLinearFn.apply(x_, w_, b_), lambda x_, w_, b_: F.linear(x_, w_, b_), (x, w, b)),
             ("token, no bias", lambda x_, w_: _TokenLinearFn.apply(x_, w_, None), lambda x_, w_: F.linear(x_, w_), (x, w)),
             ("residual", lambda r_, x_, w_: _ResidualLinearFn.apply(r_, x_, w_), lambda r_, x_, w_: r_ + F.linear(x_, w_), (res, x, w))]
    for what, fn, ref, leaves in cases:
        (y, g1, g2), (yr, r1, r2) = _second_order(fn, ref, leaves)
        assert _rel(y, yr) <= 1e-10, what
        for i, (a, r) in enumerate(zip(g1, r1)):
            assert _rel(a, r) <= 1e-10, f"{what}: first derivative of leaf {i}: {_rel(a, r):.2e}"
        for i, (a, r) in enumerate(zip(g2, r2)):
            assert _rel(a, r) <= 1e-10, f"{what}: second derivative of leaf {i}: {_rel(a, r):.2e}"


def test_linear_functions_with_frozen_leaves():
    """a leaf that does not require grad gets none, the others are unchanged, bit for bit (CPU float64)"""
    from mop_amd.nn.linear import _ResidualLinearFn, _TokenLinearFn
    g = torch.Generator().manual_seed(1)
    x, w, b, res = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((4, 6, 7), (5, 7), (5,), (4, 6, 5)))
    dy = torch.randn(4, 6, 5, generator=g, dtype=torch.float64)

    def grads(fn, leaves, rg):
        t = [v.clone().requires_grad_(i in rg) for i, v in enumerate(leaves)]
        fn(*t).backward(dy)
        return [v.grad for v in t]
    for fn, leaves in ((_TokenLinearFn.apply, (x, w, b)), (_ResidualLinearFn.apply, (res, x, w))):
        full = grads(fn, leaves, {0, 1, 2})
        for rg in ({0}, {1}, {2}, {0, 2}, {1, 2}):
            got = grads(fn, leaves, rg)
            for i in range(3):
                assert (got[i] is None) == (i not in rg)
                assert i not in rg or torch.equal(got[i], full[i])
