"""Guard bands and poison around the buffers an op allocates and the tensors it is given.

guarded_allocations() replaces torch.empty, torch.empty_like, torch.zeros and torch.zeros_like -- the allocation entry points of
mop_amd/ops.py and mop_amd/nn -- while its block is open.  A replaced call that asks for a contiguous tensor gets a view into the
middle of a larger uint8 buffer:

    [ BAND bytes 0xFF | payload, rounded up to ALIGN bytes | BAND bytes 0xFF ]

The whole buffer, payload included, starts as the byte 0xFF: a NaN when read as float32 or bfloat16, -1 as int32.  A kernel that
writes past either end of the payload changes a guard byte (Ledger.intact() turns false); one that reads an `empty` buffer before
anything wrote it computes on NaNs.  zeros / zeros_like then zero the payload.  Calls the wrapper cannot serve (empty_like of a
non-contiguous tensor, keywords such as pin_memory, memory_format or out=) go to the real function unchanged, and an empty shape
returns a real empty tensor.

embedded(t) is the same idea for the inputs of a call: a contiguous copy of t in the middle of a buffer of poison (NaN; the byte
0xFF for integer / bool tensors), so a lane that reads past the tensor and multiplies by a zero weight instead of selecting shows up
as a NaN in the result.
"""
import contextlib
import math

import torch

BAND = 4096   # guard bytes on each side of a payload
ALIGN = 256   # a payload is rounded up to this many bytes; BAND and ALIGN keep every data_ptr() 16-byte aligned
FILL = 0xFF

_REAL = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like")}
_SERVED_KW = {"dtype", "device", "requires_grad", "layout"}


def _round_up(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _carve(shape, dtype, device):
    """(buffer, view, nbytes): a uint8 buffer of FILL bytes and the contiguous `shape` / `dtype` view of its payload"""
    nbytes = math.prod(shape) * _REAL["empty"]((), dtype=dtype).element_size()
    buf = _REAL["empty"](2 * BAND + _round_up(nbytes), dtype=torch.uint8, device=device)
    buf.fill_(FILL)
    view = buf[BAND:BAND + nbytes].view(dtype).view(shape)
    return buf, view, nbytes


class Ledger:
    """every buffer handed out while guarded_allocations() is open: (uint8 buffer, payload bytes, shape, dtype).  The ledger keeps
    the buffers alive, so no two payloads share memory and a guard can be read after the op has dropped its tensor."""

    def __init__(self):
        self.entries = []

    def _guards(self):
        for buf, nbytes, shape, dtype in self.entries:
            yield buf[:BAND], "before", shape, dtype
            yield buf[BAND + nbytes:], "after", shape, dtype

    def _damage(self):
        for g, side, shape, dtype in self._guards():
            bad = (g != FILL)
            if bool(bad.any()):
                near = int(bad.nonzero()[0 if side == "after" else -1])
                gap = near if side == "after" else BAND - 1 - near      # undamaged bytes between the payload and the damage
                return shape, dtype, side, gap, int(bad.sum())
        return None

    def intact(self) -> bool:
        """every guard byte of every buffer is still FILL (reads the buffers: synchronise first when kernels may be in flight)"""
        ok = None
        for g, *_ in self._guards():
            cur = (g == FILL).all()
            ok = cur if ok is None else ok.to(cur.device) & cur
        return True if ok is None else bool(ok)

    def describe_damage(self) -> str:
        d = self._damage()
        if d is None:
            return "no guard byte changed"
        shape, dtype, side, gap, n = d
        where = "past the end of" if side == "after" else "before the start of"
        return (f"guard {side} the payload damaged: {n} byte(s) changed, the nearest with {gap} intact byte(s) between it and the "
                f"payload ({where} a buffer of shape {tuple(shape)}, dtype {dtype}; 0 = the byte next to the payload, on either "
                f"side; the guard after it begins at the payload's true end, inside the padding that rounds it up to {ALIGN} bytes)")

    def count(self, nbytes=None) -> int:
        """buffers handed out, optionally only those whose payload is `nbytes` bytes"""
        return sum(1 for e in self.entries if nbytes is None or e[1] == nbytes)


def _size_of(args, kwargs):
    """the shape of an empty / zeros call given as varargs, one sequence or size=; None when it is neither"""
    if "size" in kwargs:
        if args:
            return None
        args = (kwargs["size"],)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if not all(isinstance(s, int) and not isinstance(s, bool) for s in args):
        return None
    return tuple(int(s) for s in args)


def _servable(kwargs) -> bool:
    return set(kwargs) <= _SERVED_KW and kwargs.get("layout", torch.strided) is torch.strided


def _hand_out(ledger, shape, dtype, device, requires_grad, zero):
    buf, view, nbytes = _carve(shape, dtype, device)
    if zero:
        view.zero_()
    ledger.entries.append((buf, nbytes, torch.Size(shape), dtype))
    return view.requires_grad_(True) if requires_grad else view


def _new(ledger, name, zero):
    real = _REAL[name]

    def replaced(*args, **kwargs):
        kw = {k: v for k, v in kwargs.items() if k != "size"}
        shape = _size_of(args, kwargs)
        if shape is None or not _servable(kw) or math.prod(shape) == 0 or any(s < 0 for s in shape):
            return real(*args, **kwargs)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = torch.device(kw["device"]) if kw.get("device") is not None else torch.get_default_device()
        return _hand_out(ledger, shape, dtype, device, bool(kw.get("requires_grad", False)), zero)
    return replaced


def _new_like(ledger, name, zero):
    real = _REAL[name]

    def replaced(t, *args, **kwargs):
        if (args or not isinstance(t, torch.Tensor) or not _servable(kwargs) or t.layout is not torch.strided
                or not t.is_contiguous() or t.numel() == 0):
            return real(t, *args, **kwargs)
        dtype = kwargs.get("dtype") or t.dtype
        device = torch.device(kwargs["device"]) if kwargs.get("device") is not None else t.device
        return _hand_out(ledger, tuple(t.shape), dtype, device, bool(kwargs.get("requires_grad", False)), zero)
    return replaced


@contextlib.contextmanager
def guarded_allocations():
    """with guarded_allocations() as ledger: torch.empty / empty_like / zeros / zeros_like hand out guarded, poisoned buffers"""
    ledger = Ledger()
    try:
        torch.empty = _new(ledger, "empty", False)
        torch.zeros = _new(ledger, "zeros", True)
        torch.empty_like = _new_like(ledger, "empty_like", False)
        torch.zeros_like = _new_like(ledger, "zeros_like", True)
        yield ledger
    finally:
        for n, f in _REAL.items():
            setattr(torch, n, f)


def embedded(t: torch.Tensor, poison=float("nan"), requires_grad=None) -> torch.Tensor:
    """a contiguous copy of t (requires_grad as asked; t's own by default) in the middle of a buffer whose other bytes are the
    poison, BAND bytes at least on each side; integer, uint8 and bool tensors are surrounded by the byte 0xFF.  .contiguous() on
    the result copies nothing, so a kernel is given the embedded pointer."""
    src = t.detach()
    buf, view, _ = _carve(tuple(src.shape), src.dtype, src.device)
    if src.dtype.is_floating_point:
        buf.view(src.dtype).fill_(poison)
    view.copy_(src)
    return view.requires_grad_(t.requires_grad if requires_grad is None else bool(requires_grad))
