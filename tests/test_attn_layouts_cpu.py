"""No GPU: the layout builders of tests/attn_layouts.py, and the mask / bias side of the attention cores' stride contract.

The kernels read a mask or a bias at `ptr + b*sb + h*sh + i*si + j`: the key axis has stride 1 by construction, B, H and N may be
broadcast by stride 0.  ops._mask_u8 / ops._bias_f32 turn anything that broadcasts to (B,H,N,Nk) into such a tensor and its (sb, sh,
si); the table test below walks the flat storage the way the kernels do.  N = 5 and Nk = 7 differ, so a confusion of the two
extents shows."""
import pytest
import torch

import attn_layouts as al

B, N, H, DK = 2, 5, 3, 8        # odd N and H: odd_rows then has all three strides = 4 (mod 8)
NK = 7


def _values(dtype, n=N):
    g = torch.Generator().manual_seed(11)
    return torch.randn(B, n, H, DK, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", al.LAYOUTS)
def test_builder(name, dtype):
    """strides as tabled, the view holds the input, everything outside it is NaN, alignment as claimed"""
    vals = _values(dtype)
    storage, view = al.build(name, vals)
    assert view.shape == (B, N, H, DK) and view.stride(3) == 1 and view.dtype == dtype
    assert al.view4(view) == al.expected_strides(name, B, N, H, DK)
    expect = vals
    if name == "batch_bcast":
        expect = vals[:1].expand(B, N, H, DK)
    elif name == "head_bcast":
        expect = vals[:, :, :1].expand(B, N, H, DK)
    assert torch.equal(view, expect)
    assert view.untyped_storage().data_ptr() == storage.untyped_storage().data_ptr()
    # outside the view: mark the view's elements in a copy of the storage, everything left unmarked must be NaN
    inside = torch.zeros(storage.shape, dtype=torch.bool)
    idx = view.storage_offset() + sum(torch.arange(n).view([-1 if e == d else 1 for e in range(4)]) * view.stride(d)
                                      for d, n in enumerate(view.shape))
    inside.view(-1)[idx.reshape(-1)] = True
    assert inside.sum() == (view.numel() if "bcast" not in name else view.numel() // (B if name == "batch_bcast" else H))
    assert torch.isnan(storage[~inside]).all() and not torch.isnan(storage[inside]).any()
    assert (~inside).sum() == storage.numel() - inside.sum()
    # alignment: the allocation itself is on a 16-byte boundary, so the pointer's residue is the offset's
    assert storage.data_ptr() % 16 == 0
    off, strides = al.view4(view)
    assert view.data_ptr() % 16 == (off * view.element_size()) % 16 == 0
    if name == "odd_rows":
        assert all(s % 8 == 4 for s in strides)
        assert al.aligned16(view) == (view.element_size() == 4)          # misaligned exactly for 2-byte elements
    else:
        assert al.aligned16(view)


@pytest.mark.parametrize("slot", [0, 1, 2])
def test_packed_slot_builder_takes_every_slot(slot):
    vals = _values(torch.bfloat16)
    storage, view = al.packed_slot(vals, slot=slot)
    assert al.view4(view) == (slot * H * DK, (3 * N * H * DK, DK, 3 * H * DK)) and al.aligned16(view)
    assert torch.equal(view, vals) and torch.equal(storage[:, :, slot], vals)
    assert torch.isnan(storage[:, :, [s for s in range(3) if s != slot]]).all()


def test_builder_leaf_is_the_storage():
    """with requires_grad the storage is the leaf, and the view's retained gradient is what came in for the view: for a broadcast
    operand it is seen before autograd sums it into the storage"""
    for name in al.LAYOUTS:
        storage, view = al.build(name, _values(torch.float32), requires_grad=True)
        assert storage.is_leaf and storage.requires_grad
        view.retain_grad()
        w = torch.arange(view.numel(), dtype=torch.float32).view(view.shape)
        (view * w).sum().backward()
        assert torch.equal(view.grad, w), name
        assert storage.grad.shape == storage.shape
        if name == "batch_bcast":
            assert torch.equal(storage.grad, w.sum(0, keepdim=True))
        if name == "head_bcast":
            assert torch.equal(storage.grad, w.sum(2, keepdim=True))


def test_rotation_covers_every_pair_once():
    for n in (3, 5, 6, 8):
        seen = set()
        for r in range(8):
            names = al.rotation(r, n)
            assert len(set(names)) == n
            seen.update((j, nm) for j, nm in enumerate(names))
        assert len(seen) == n * 8


# ---------------------------------------------------------------- ops._mask_u8 / ops._bias_f32
def _forms():
    """every broadcast form of a (B,H,N,Nk) mask / bias: name -> shape"""
    return {
        "(Nk,)": (NK,), "(N,1)": (N, 1), "(N,Nk)": (N, NK), "(1,1,N,Nk)": (1, 1, N, NK), "(B,1,1,Nk)": (B, 1, 1, NK),
        "(B,1,N,1)": (B, 1, N, 1), "(B,H,1,Nk)": (B, H, 1, NK), "(B,H,N,1)": (B, H, N, 1), "(1,H,N,Nk)": (1, H, N, NK),
        "(B,H,N,Nk)": (B, H, N, NK),
    }


def _inputs(kind):
    g = torch.Generator().manual_seed(5)

    def draw(shape):
        t = torch.randn(tuple(shape), generator=g)
        return (t > 0.3) if kind == "mask" else t
    out = {name: draw(shape) for name, shape in _forms().items()}
    out["(N,Nk) transposed"] = draw((NK, N)).t()
    assert not out["(N,Nk) transposed"].is_contiguous()
    if kind == "bias":
        out["()"] = draw(())
    return out


def _helper(kind):
    from mop_amd import ops
    return ops._mask_u8 if kind == "mask" else ops._bias_f32


def _check_form(kind, src):
    out, strides = _helper(kind)(src, B, H, N, torch.device("cpu"), NK)
    want = torch.broadcast_to((src != 0).to(torch.uint8) if kind == "mask" else src.to(torch.float32), (B, H, N, NK))
    assert out.dtype == want.dtype and out.shape == (B, H, N, NK)
    assert torch.equal(out, want)
    assert out.stride(3) == 1
    assert strides == (out.stride(0), out.stride(1), out.stride(2))
    # the kernels' own indexing over the flat storage, from the pointer they are handed
    es = out.element_size()
    base = (out.data_ptr() - out.untyped_storage().data_ptr()) // es
    flat = torch.empty(0, dtype=out.dtype).set_(out.untyped_storage())
    sb, sh, si = strides
    idx = (base + torch.arange(B).view(B, 1, 1, 1) * sb + torch.arange(H).view(1, H, 1, 1) * sh
           + torch.arange(N).view(1, 1, N, 1) * si + torch.arange(NK).view(1, 1, 1, NK))
    assert int(idx.max()) < flat.numel(), "the kernels would read past the end of the buffer"
    assert torch.equal(flat[idx], want)
    return out


@pytest.mark.parametrize("kind", ["mask", "bias"])
@pytest.mark.parametrize("form", list(_forms()) + ["(N,Nk) transposed", "()"])
def test_mask_and_bias_forms(form, kind):
    """On the parent of this change the (N,1) and (B,1,N,1) rows fail (and (B,H,N,1) with them: every form whose key axis has
    extent 1 while Nk > 1): the expand left a zero stride on the key axis, which the kernels cannot express -- they read
    bias[i + j] -- and the mask twin stopped at a bare assert."""
    ins = _inputs(kind)
    if form not in ins:
        assert kind == "mask" and form == "()"
        ins[form] = torch.tensor(True)          # a 0-d mask is no documented form, but it broadcasts: it must work all the same
    src = ins[form]
    out = _check_form(kind, src)
    # storage: B, H and N stay broadcast; a key axis of extent 1 is the only thing that is written out
    shape4 = (1,) * (4 - src.dim()) + tuple(src.shape)
    numel = shape4[0] * shape4[1] * shape4[2] * NK
    assert out.untyped_storage().nbytes() == numel * out.element_size(), (form, shape4)
    for d in range(3):
        assert (out.stride(d) == 0) == (shape4[d] == 1), (form, d, out.stride())


def test_forms_that_need_no_copy_keep_their_storage():
    """a float32 bias whose key axis is already there goes to the kernels as it is"""
    from mop_amd import ops
    for form, src in _inputs("bias").items():
        if src.dim() == 0 or src.shape[-1] == 1 or not src.is_contiguous():
            continue
        out, _ = ops._bias_f32(src, B, H, N, torch.device("cpu"), NK)
        assert out.data_ptr() == src.data_ptr(), form


def test_key_axis_of_extent_one_with_one_key():
    """Nk = 1: there is no key stride to speak of, nothing is copied"""
    from mop_amd import ops
    src = torch.randn(N, 1)
    out, strides = ops._bias_f32(src, B, H, N, torch.device("cpu"), 1)
    assert out.shape == (B, H, N, 1) and out.data_ptr() == src.data_ptr() and strides == (0, 0, 1)


def test_square_default_and_none():
    from mop_amd import ops
    assert ops._mask_u8(None, B, H, N, torch.device("cpu")) == (None, (0, 0, 0))
    assert ops._bias_f32(None, B, H, N, torch.device("cpu"), NK) == (None, (0, 0, 0))
    out, _ = ops._bias_f32(torch.randn(1, N), B, H, N, torch.device("cpu"))          # Nk defaults to N
    assert out.shape == (B, H, N, N) and out.stride() == (0, 0, 0, 1)


@pytest.mark.parametrize("kind", ["mask", "bias"])
@pytest.mark.parametrize("shape", [(N + 1, NK), (NK, N), (B, H, N, NK + 1), (2, B, H, N, NK), (3,)])
def test_shapes_that_do_not_broadcast_raise_torchs_error(shape, kind):
    with pytest.raises(RuntimeError):
        _helper(kind)(torch.ones(*shape), B, H, N, torch.device("cpu"), NK)
