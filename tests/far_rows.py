"""Operands whose rows lie more than 2^32 bytes apart: one large device buffer of a sentinel byte, from which a test is handed
`torch.as_strided` views with a leading (batch or row) stride of FAR_STRIDE = 2^31 + 2^16 elements.

    byte 0                                                                                          8 GiB + 64 MiB
    | guard | row 0 of A | guard | row 0 of B | ...      | guard | row 1 of A | ...      | guard | row 2 of A | ... |
            ^ cursor               ^ cursor'              ^ cursor + FAR_STRIDE * itemsize        ^ cursor + 2 * FAR_STRIDE * itemsize

Row b of a view starts FAR_STRIDE * itemsize * b bytes after row 0.  With two-byte elements (bf16) row 1 lies past 2^31 elements
and 2^32 bytes and row 2 past 2^32 elements (3 rows fit); with four-byte elements (fp32, int32) row 1 lies past 2^31 elements and
past 8 GiB (2 rows fit).  Inner strides are those of a compact tensor, and every row starts on an ALIGN = 256-byte boundary, so a
row keeps the 16-byte phase of the same row in a compact tensor.  Several operands of one call are handed out one after the
other: row 0 of each sits at the cursor, which then moves past the row and a guard.

Every row handed out is recorded (`live` while a test holds it; `handed_out` keeps all of them, for reports).  check_guards() asserts that the GUARD bytes on either side of each live row still hold the
sentinel; release() gives the rows back (they are filled with the sentinel again, and the cursor returns to the start);
scan_untouched() asserts the sentinel everywhere outside the live rows, one pass over the whole buffer.  The sentinel is the
byte 0xFF: a NaN when read as float32 or bfloat16, -1 as int32, so a read outside a row shows in a result.

Nothing here touches a device at import time; the geometry is tested on a small CPU buffer with a small stride.
"""
import math

import torch

SENTINEL = 0xFF
FAR_STRIDE = 2 ** 31 + 2 ** 16            # elements between the rows of a far view
BUFFER_BYTES = 8 * 2 ** 30 + 64 * 2 ** 20
GUARD = 2 ** 20                           # bytes checked on either side of a row
ALIGN = 256                               # every row starts on this boundary
MIN_FREE_BYTES = 12 * 2 ** 30             # the buffer, the float64 references and the ops' own allocations
_SCAN_CHUNK = 2 ** 30


def far_rows(dtype) -> int:
    """how many rows of a FAR_STRIDE view fit in the buffer: 3 of a two-byte dtype, 2 of a four-byte one"""
    return {2: 3, 4: 2}[torch.empty((), dtype=dtype).element_size()]


class FarBuffer:
    """the sentinel buffer and the ledger of the rows handed out of it"""

    def __init__(self, device, nbytes=BUFFER_BYTES, stride=FAR_STRIDE, guard=GUARD):
        assert nbytes % 8 == 0 and guard % ALIGN == 0
        self.stride, self.guard, self.nbytes = stride, guard, nbytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.buf.fill_(SENTINEL)
        self.live = []          # (first byte, one past the last byte) of every row now handed out
        self.handed_out = []    # every row ever handed out: a record for reports only (how many rows the tests placed); the
                                # scan needs no such list, since release() refills a row before it leaves `live`
        self.cursor = guard

    @classmethod
    def on_device(cls, device="cuda"):
        """the full-size buffer; fails (it does not skip) where the device has too little free memory for the far tests"""
        free = torch.cuda.mem_get_info()[0]
        assert free >= MIN_FREE_BYTES, (f"the far-row tests need {MIN_FREE_BYTES / 2 ** 30:.0f} GiB of free device memory for their "
                                        f"{BUFFER_BYTES / 2 ** 30:.2f} GiB buffer and references; {free / 2 ** 30:.1f} GiB are free")
        return cls(device)

    def far(self, shape, dtype, batch_stride=None) -> torch.Tensor:
        """a `shape` / `dtype` view of the buffer: stride(0) = batch_stride (the buffer's far stride by default) elements, the inner
        strides compact, every row on an ALIGN-byte boundary, GUARD sentinel bytes at least between it and any other row"""
        shape = tuple(int(s) for s in shape)
        stride = self.stride if batch_stride is None else int(batch_stride)
        isz = torch.empty((), dtype=dtype).element_size()
        row_elems = math.prod(shape[1:])
        assert shape[0] >= 1 and row_elems >= 1 and (shape[0] == 1 or stride >= row_elems)
        assert (stride * isz) % ALIGN == 0, "the batch stride must keep every row on the alignment boundary"
        rows = [(self.cursor + b * stride * isz, self.cursor + b * stride * isz + row_elems * isz) for b in range(shape[0])]
        assert rows[-1][1] + self.guard <= self.nbytes, (
            f"a {shape} {dtype} view with batch stride {stride} ends at byte {rows[-1][1]}: past the buffer's {self.nbytes} less a guard")
        for lo, hi in rows:
            for lo2, hi2 in self.live + [r for r in rows if r != (lo, hi)]:
                assert hi + self.guard <= lo2 or hi2 + self.guard <= lo, f"rows [{lo}, {hi}) and [{lo2}, {hi2}) lie within a guard"
        inner = [1] * (len(shape) - 1)
        for i in range(len(shape) - 3, -1, -1):
            inner[i] = inner[i + 1] * shape[i + 2]
        view = torch.as_strided(self.buf.view(dtype), shape, (stride, *inner), self.cursor // isz)
        self.live += rows
        self.handed_out += rows
        self.cursor = (rows[0][1] + ALIGN - 1) // ALIGN * ALIGN + self.guard
        return view

    def far_like(self, t: torch.Tensor) -> torch.Tensor:
        """a far view of t's shape and dtype that holds t's values"""
        v = self.far(t.shape, t.dtype)
        v.copy_(t.detach())
        return v

    def _bad_bytes(self, lo, hi):
        """how many bytes of [lo, hi) differ from the sentinel, as a 0-d device tensor (no synchronisation)"""
        total = torch.zeros((), dtype=torch.int64, device=self.buf.device)
        a, b = min(hi, (lo + 7) // 8 * 8), max(lo, hi // 8 * 8)
        if a >= b:
            return total + (self.buf[lo:hi] != SENTINEL).sum()
        total += (self.buf[lo:a] != SENTINEL).sum() + (self.buf[b:hi] != SENTINEL).sum()
        for c in range(a, b, _SCAN_CHUNK):          # eight bytes at a time: a word that is not all-sentinel counts as one
            total += (self.buf[c:min(b, c + _SCAN_CHUNK)].view(torch.int64) != -1).sum()
        return total

    def _first_bad(self, lo, hi) -> int:
        for c in range(lo, hi, _SCAN_CHUNK):
            bad = (self.buf[c:min(hi, c + _SCAN_CHUNK)] != SENTINEL).nonzero()
            if bad.numel():
                return c + int(bad[0])
        return -1

    def guards(self):
        """[(first, one past last, which row, side)]: the guard intervals around every live row"""
        out = []
        for lo, hi in self.live:
            out.append((lo - self.guard, lo, (lo, hi), "before"))
            out.append((hi, hi + self.guard, (lo, hi), "after"))
        return out

    def check_guards(self) -> None:
        """the GUARD bytes on either side of every live row still hold the sentinel"""
        gs = self.guards()
        if not gs:
            return
        bad = torch.stack([self._bad_bytes(lo, hi) for lo, hi, _, _ in gs]).cpu().tolist()
        for n, (lo, hi, row, side) in zip(bad, gs):
            assert n == 0, (f"the guard {side} the row at bytes [{row[0]}, {row[1]}) was written: {n} word(s) changed, the first at "
                            f"byte {self._first_bad(lo, hi)}")

    def release(self) -> None:
        """give every live row back: it holds the sentinel again, and the next view starts at the front of the buffer"""
        for lo, hi in self.live:
            self.buf[lo:hi].fill_(SENTINEL)
        self.live = []
        self.cursor = self.guard

    def scan_untouched(self) -> None:
        """every byte outside the live rows holds the sentinel (one pass over the buffer)"""
        edges, at = [], 0
        for lo, hi in sorted(self.live):
            edges.append((at, lo))
            at = hi
        edges.append((at, self.nbytes))
        edges = [(lo, hi) for lo, hi in edges if hi > lo]
        bad = torch.stack([self._bad_bytes(lo, hi) for lo, hi in edges]).cpu().tolist()
        for n, (lo, hi) in zip(bad, edges):
            assert n == 0, (f"{n} word(s) outside every row handed out were written; the first at byte {self._first_bad(lo, hi)} "
                            f"(rows handed out so far: {len(self.handed_out)})")
