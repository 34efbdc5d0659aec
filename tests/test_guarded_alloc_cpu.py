"""tests/guarded_alloc.py on CPU tensors: faults planted in plain Python "ops" are detected, a correct op passes, and torch is
left as it was.  The GPU bounds tests (test_gpu_bounds.py) rely on exactly these detections."""
import pytest
import torch

from guarded_alloc import BAND, embedded, guarded_allocations

REAL = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like)


def _op_ok(x, w):
    """y = x @ w through an `empty` output and an `empty` workspace it fills before reading"""
    y = torch.empty(x.shape[0], w.shape[1], dtype=x.dtype)
    ws = torch.empty_like(y)
    torch.matmul(x, w, out=ws)
    y.copy_(ws)
    return y


def _op_writes_past_the_end(x, w):
    y = _op_ok(x, w)
    n = y.numel()
    torch.as_strided(y, (n + 1,), (1,))[n] = 1.0
    return y


def _op_writes_before_the_start(x, w):
    y = _op_ok(x, w)
    torch.as_strided(y, (1,), (1,), y.storage_offset() - 1)[0] = 1.0
    return y


def _op_sums_an_unwritten_workspace(x, w):
    y = _op_ok(x, w)
    ws = torch.empty(8, dtype=x.dtype)
    return y + ws.sum()


def _op_weights_a_row_out_of_range_by_zero(x, w):
    """reads row M of an (M, K) input and multiplies it by 0.0 where a select was due"""
    y = _op_ok(x, w)
    M, K = x.shape
    stray = torch.as_strided(x, (1, K), (K, 1), x.storage_offset() + M * K)
    return y + (stray * 0.0) @ w


def _inputs(dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    return torch.randn(5, 7, generator=g).to(dtype), torch.randn(7, 3, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_correct_op_passes_every_check(dtype):
    x, w = _inputs(dtype)
    plain = _op_ok(x, w)
    with guarded_allocations() as ledger:
        y = _op_ok(embedded(x), embedded(w))
    assert ledger.intact(), ledger.describe_damage()
    assert torch.isfinite(y).all() and torch.equal(y, plain)
    assert ledger.count() == 2 and ledger.count(y.numel() * y.element_size()) == 2 and ledger.count(12345) == 0
    assert ledger.describe_damage() == "no guard byte changed"


@pytest.mark.parametrize("op,side", [(_op_writes_past_the_end, "after"), (_op_writes_before_the_start, "before")])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_write_of_one_element_outside_the_output_is_reported(op, side, dtype):
    x, w = _inputs(dtype)
    with guarded_allocations() as ledger:
        y = op(embedded(x), embedded(w))
    assert torch.equal(y, _op_ok(x, w))          # the values alone do not show it
    assert not ledger.intact()
    msg = ledger.describe_damage()
    assert f"guard {side} the payload" in msg and "(5, 3)" in msg and str(dtype) in msg, msg
    # every byte of 1.0 (00 00 80 3f / 80 3f) differs from 0xFF: the element touches the payload on either side
    where = "past the end of" if side == "after" else "before the start of"
    assert where in msg and "the nearest with 0 intact byte(s)" in msg and f"{y.element_size()} byte(s) changed" in msg, msg


def test_a_single_damaged_byte_is_reported():
    with guarded_allocations() as ledger:
        y = torch.empty(3, 5)
        u8 = torch.as_strided(y.view(torch.uint8), (256 + BAND,), (1,))
        u8[-1] = 0                              # the last guard byte of the buffer (the 60-byte payload is rounded up to 256)
    assert not ledger.intact()
    assert f"1 byte(s) changed, the nearest with {256 + BAND - 1 - 60} intact byte(s)" in ledger.describe_damage()


def test_an_unwritten_workspace_reads_as_nan():
    x, w = _inputs()
    with guarded_allocations() as ledger:
        y = _op_sums_an_unwritten_workspace(embedded(x), embedded(w))
    assert ledger.intact()
    assert torch.isnan(y).all()
    with guarded_allocations():
        assert torch.isnan(torch.empty(4, dtype=torch.bfloat16)).all()
        assert (torch.empty(4, dtype=torch.int32) == -1).all()
        assert (torch.empty_like(torch.ones(2, 3)).isnan()).all()


def test_an_out_of_range_row_times_zero_is_nan():
    x, w = _inputs()
    with guarded_allocations() as ledger:
        y = _op_weights_a_row_out_of_range_by_zero(embedded(x), embedded(w))
    assert ledger.intact()
    assert torch.isnan(y).all()
    # with finite bytes behind the input the same op is silently right: that is the gap the poison closes
    y0 = _op_weights_a_row_out_of_range_by_zero(embedded(x, poison=3.0), embedded(w))
    assert torch.equal(y0, _op_ok(x, w))


def test_embedded_keeps_values_grad_flag_and_poison():
    x = torch.arange(12, dtype=torch.float32).view(3, 4).t()           # non-contiguous source
    e = embedded(x.requires_grad_(True))
    assert e.is_contiguous() and e.requires_grad and e.is_leaf and torch.equal(e.detach(), x.detach())
    assert e.contiguous().data_ptr() == e.data_ptr() and e.data_ptr() % 16 == 0
    assert not embedded(x, requires_grad=False).requires_grad
    store = torch.as_strided(e.detach(), (e.storage_offset() + e.numel() + BAND // 4,), (1,), 0)
    assert e.storage_offset() * 4 >= BAND
    assert store[:e.storage_offset()].isnan().all() and store[e.storage_offset() + e.numel():].isnan().all()
    (e * 2).sum().backward()
    assert torch.equal(e.grad, torch.full((4, 3), 2.0))
    for t in (torch.tensor([3, 1, 4], dtype=torch.int32), torch.tensor([[1, 0, 1]], dtype=torch.uint8), torch.tensor([True, False])):
        i = embedded(t)
        assert torch.equal(i, t) and i.dtype == t.dtype
        around = torch.as_strided(i.view(torch.uint8), (BAND,), (1,), i.view(torch.uint8).storage_offset() - BAND)
        assert (around == 0xFF).all()
    assert (embedded(torch.tensor([3, 1], dtype=torch.int32)).untyped_storage().nbytes()) >= 2 * BAND + 8


def test_torch_is_restored_after_the_block_also_when_it_raises():
    with guarded_allocations():
        assert torch.empty is not REAL[0] and torch.zeros_like is not REAL[3]
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) == REAL
    with pytest.raises(RuntimeError, match="planted"):
        with guarded_allocations():
            raise RuntimeError("planted")
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like) == REAL


def test_every_pointer_is_16_byte_aligned_and_zeros_are_zero():
    with guarded_allocations() as ledger:
        ts = [torch.empty(n, dtype=dt) for n in (1, 3, 17, 255, 4097) for dt in (torch.uint8, torch.bfloat16, torch.float32, torch.int64)]
        z = torch.zeros(3, 5, dtype=torch.bfloat16)
        zl = torch.zeros_like(torch.ones(7, dtype=torch.int32))
        el = torch.empty_like(z, dtype=torch.float32)
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in ts + [z, zl, el])
    assert (z == 0).all() and z.shape == (3, 5) and (zl == 0).all() and zl.dtype == torch.int32
    assert el.shape == (3, 5) and el.dtype == torch.float32
    assert ledger.count() == len(ts) + 3 and ledger.intact()


def test_shapes_as_varargs_tuple_size_and_keyword():
    with guarded_allocations() as ledger:
        a = torch.empty(2, 3, 4)
        b = torch.empty((2, 3, 4), dtype=torch.bfloat16)
        c = torch.zeros(torch.Size([2, 3, 4]), dtype=torch.float32, device="cpu")
        d = torch.empty([2, 3, 4], requires_grad=True)
        e = torch.empty(size=(2, 3, 4))
        s = torch.zeros((), dtype=torch.float32)
    assert all(t.shape == (2, 3, 4) for t in (a, b, c, d, e)) and s.shape == () and float(s) == 0.0
    assert b.dtype == torch.bfloat16 and d.requires_grad and not a.requires_grad
    assert ledger.count() == 6 and ledger.count(96) == 4 and ledger.count(48) == 1


def test_calls_the_wrapper_cannot_serve_go_to_the_real_function():
    nc = torch.ones(4, 6).t()
    out = torch.ones(5)
    with guarded_allocations() as ledger:
        e0 = torch.empty(0, 3)
        e1 = torch.zeros(0)
        like_nc = torch.empty_like(nc)
        z_nc = torch.zeros_like(nc)
        fmt = torch.empty_like(torch.ones(2, 3), memory_format=torch.contiguous_format)
        pin = torch.empty(3, pin_memory=False)
        got = torch.zeros(5, out=out)
        like_empty = torch.zeros_like(torch.ones(0, 2))
    assert ledger.count() == 0
    assert e0.shape == (0, 3) and e1.numel() == 0 and like_empty.shape == (0, 2)
    assert like_nc.shape == nc.shape and like_nc.stride() == nc.stride() and (z_nc == 0).all()
    assert fmt.shape == (2, 3) and pin.shape == (3,) and got is out and (out == 0).all()


class _Fn(torch.autograd.Function):
    """the pattern of mop_amd/ops.py: forward returns a view of an `empty` output and saves an `empty` workspace"""

    @staticmethod
    def forward(ctx, x):
        y = torch.empty(x.shape[0], 2, x.shape[1] // 2, dtype=x.dtype)
        saved = torch.empty(x.shape[0], dtype=torch.float32)
        y.view(x.shape).copy_(x * 2)
        saved.copy_(x.float().sum(1))
        ctx.save_for_backward(saved)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        (saved,) = ctx.saved_tensors
        dx = torch.empty_like(dy)
        dx.copy_(dy * 2 + (saved * 0)[:, None].to(dy.dtype))
        return dx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_an_autograd_function_in_the_style_of_ops_py_runs_unchanged(dtype):
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(1)).to(dtype)
    with guarded_allocations() as ledger:
        xe = embedded(x, requires_grad=True)
        y = _Fn.apply(xe)
        y.backward(embedded(torch.ones_like(x)))
    assert ledger.intact(), ledger.describe_damage()
    assert torch.equal(y.detach(), x * 2) and torch.equal(xe.grad, torch.full_like(x, 2.0))
    assert ledger.count(x.numel() * x.element_size()) >= 2 and ledger.count(16) == 1
