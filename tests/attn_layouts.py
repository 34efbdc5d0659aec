"""Layouts of a logical (B,N,H,dk) attention operand (plain torch, importable without a GPU).

The attention cores take every operand as a MopkView4: a pointer and three element strides (batch, head, token), inner stride 1.
A builder takes the values of a logical (B,N,H,dk) tensor and returns (storage, view): `view` has those values, that shape and a
unit inner stride, and every element of `storage` outside the view is NaN, so a kernel that reads with the wrong stride reads NaN
(or another operand's layout) instead of a plausible number.

  name         how                                               View4 strides (sb, sh, sn)
  contig       fresh                                             (N H dk, dk, H dk)
  heads_first  contiguous (B,H,N,dk), .transpose(1, 2)           (H N dk, N dk, dk)
  packed_slot  slot s of (B,N,3,H,dk), passed unpacked           (3 N H dk, dk, 3 H dk), offset s H dk
  wide_rows    [..., 8:8+dk] of (B,N,H,dk+16)                    (N H (dk+16), dk+16, H (dk+16)), offset 8
  window       rows [3:3+N] of (B,N+5,H,dk)                      ((N+5) H dk, dk, H dk), offset 3 H dk
  batch_bcast  (1,N,H,dk).expand(B, ...)                         sb = 0
  head_bcast   (B,N,1,dk).expand(..., H, ...)                    sh = 0, sn = dk
  odd_rows     [..., :dk] of (B,N,H,dk+4)                        (N H (dk+4), dk+4, H (dk+4))

The two broadcast layouts hold the values of the first batch row / head.  With dk a multiple of 8, every layout but odd_rows keeps
the pointer and the three strides on 16-byte multiples for 2- and 4-byte elements alike.  odd_rows has a head stride of dk + 4
= 4 (mod 8) elements (and, for odd N and H, all three strides = 4 (mod 8)): 16-byte multiples for float32, not for bfloat16.
"""
import torch

LAYOUTS = ("contig", "heads_first", "packed_slot", "wide_rows", "window", "batch_bcast", "head_bcast", "odd_rows")
PACKED_SLOT = 1                 # the slot build() uses for "packed_slot": a non-zero offset
WIDE_PAD, WIDE_OFF = 16, 8      # wide_rows: dk + 16 elements per row, the view from element 8
WINDOW_PAD, WINDOW_OFF = 5, 3   # window: N + 5 rows, the view from row 3
ODD_PAD = 4                     # odd_rows: dk + 4 elements per row


def _nan(values: torch.Tensor, *shape) -> torch.Tensor:
    return torch.full(shape, float("nan"), dtype=values.dtype, device=values.device)


# every builder: (values, requires_grad) -> (storage, view).  With requires_grad the storage is the leaf and the view hangs on it in
# the autograd graph (view.retain_grad() then shows the gradient a Function returned for it, before autograd sums a broadcast)
def contig(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, B, N, H, dk)
    s.copy_(values)
    s.requires_grad_(requires_grad)
    return s, s


def heads_first(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, B, H, N, dk)
    s.copy_(values.transpose(1, 2))
    s.requires_grad_(requires_grad)
    return s, s.transpose(1, 2)


def packed_slot(values, requires_grad=False, slot=PACKED_SLOT):
    B, N, H, dk = values.shape
    s = _nan(values, B, N, 3, H, dk)
    s[:, :, slot].copy_(values)
    s.requires_grad_(requires_grad)
    return s, s[:, :, slot]


def wide_rows(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, B, N, H, dk + WIDE_PAD)
    s[..., WIDE_OFF:WIDE_OFF + dk].copy_(values)
    s.requires_grad_(requires_grad)
    return s, s[..., WIDE_OFF:WIDE_OFF + dk]


def window(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, B, N + WINDOW_PAD, H, dk)
    s[:, WINDOW_OFF:WINDOW_OFF + N].copy_(values)
    s.requires_grad_(requires_grad)
    return s, s[:, WINDOW_OFF:WINDOW_OFF + N]


def batch_bcast(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, 1, N, H, dk)
    s.copy_(values[:1])
    s.requires_grad_(requires_grad)
    return s, s.expand(B, N, H, dk)


def head_bcast(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, B, N, 1, dk)
    s.copy_(values[:, :, :1])
    s.requires_grad_(requires_grad)
    return s, s.expand(B, N, H, dk)


def odd_rows(values, requires_grad=False):
    B, N, H, dk = values.shape
    s = _nan(values, B, N, H, dk + ODD_PAD)
    s[..., :dk].copy_(values)
    s.requires_grad_(requires_grad)
    return s, s[..., :dk]


BUILDERS = {"contig": contig, "heads_first": heads_first, "packed_slot": packed_slot, "wide_rows": wide_rows, "window": window,
            "batch_bcast": batch_bcast, "head_bcast": head_bcast, "odd_rows": odd_rows}
assert tuple(BUILDERS) == LAYOUTS


def build(name_or_index, values, requires_grad=False):
    """(storage, view) of `values` in the named layout (or LAYOUTS[index])"""
    name = LAYOUTS[name_or_index] if isinstance(name_or_index, int) else name_or_index
    return BUILDERS[name](values, requires_grad)


def rotation(r: int, n_operands: int):
    """the layouts of rotation r: operand j gets LAYOUTS[(j + r) mod 8] -- no two operands of a call (at most 8) share one, and over
    r = 0 .. 7 every operand meets every layout"""
    return [LAYOUTS[(j + r) % len(LAYOUTS)] for j in range(n_operands)]


def view4(view: torch.Tensor):
    """(element offset into the storage, (sb, sh, sn)) of a (B,N,H,dk) view: what ops._v4 hands the kernels"""
    assert view.dim() == 4 and view.stride(3) == 1
    return view.storage_offset(), (view.stride(0), view.stride(2), view.stride(1))


def expected_strides(name: str, B: int, N: int, H: int, dk: int):
    """(element offset, (sb, sh, sn)) as the table above states them"""
    return {
        "contig": (0, (N * H * dk, dk, H * dk)),
        "heads_first": (0, (H * N * dk, N * dk, dk)),
        "packed_slot": (PACKED_SLOT * H * dk, (3 * N * H * dk, dk, 3 * H * dk)),
        "wide_rows": (WIDE_OFF, (N * H * (dk + WIDE_PAD), dk + WIDE_PAD, H * (dk + WIDE_PAD))),
        "window": (WINDOW_OFF * H * dk, ((N + WINDOW_PAD) * H * dk, dk, H * dk)),
        "batch_bcast": (0, (0, dk, H * dk)),
        "head_bcast": (0, (N * dk, 0, dk)),
        "odd_rows": (0, (N * H * (dk + ODD_PAD), dk + ODD_PAD, H * (dk + ODD_PAD))),
    }[name]


def aligned16(view: torch.Tensor) -> bool:
    """the documented rule of the 16-byte loads: the pointer and all three strides (batch, head, token) are multiples of 16 bytes"""
    es = view.element_size()
    return view.data_ptr() % 16 == 0 and all((view.stride(d) * es) % 16 == 0 for d in (0, 1, 2))
