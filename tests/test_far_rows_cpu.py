"""The far-row helper's geometry on a small CPU buffer, and every `*_workspace_bytes` / `*_saved_bytes` export in 64 bits.  No device.

Geometry: tests/far_rows.py with the stride passed in.  The rows of a view and of several views do not overlap, start on 256-byte
boundaries and are surrounded by guards; check_guards() and scan_untouched() catch one byte written outside a row and accept
writes inside one.  A captured stride truncated to 32 bits does not equal the far stride (the comparison the GPU file makes).

Sizes: for a fill the support query accepts, B is doubled through the values at which the size crosses 2^31 and 2^32 bytes.  A size
that grows with B is affine in it (past any per-row-count cap), so f(4B) - f(2B) == 2 (f(2B) - f(B)) and f(2B) > f(B): a product
formed in 32 bits breaks both.  A size that is bounded (a capped number of partial-sum rows) is constant past its cap and stays
under 2^31.  Where the support query refuses the shape, the size query returns 0.
"""
import ctypes as C

import pytest
import torch

import far_rows as FR
from test_entry_refusals_cpu import ROWS, _filled, _set

STRIDE, NBYTES, GUARD = 2 ** 16 + 2 ** 8, 5 * 2 ** 18, 4096


def _buf():
    return FR.FarBuffer("cpu", nbytes=NBYTES, stride=STRIDE, guard=GUARD)


def _byte0(buf, t):
    return t.data_ptr() - buf.buf.data_ptr()


# ---------------------------------------------------------------------------------------------- geometry
def test_the_full_size_layout_puts_the_rows_where_the_far_tests_need_them():
    s = FR.FAR_STRIDE
    assert FR.far_rows(torch.bfloat16) == 3 and FR.far_rows(torch.float32) == 2 and FR.far_rows(torch.int32) == 2
    assert 1 * s > 2 ** 31                                                 # row 1 (any dtype) lies past 2^31 elements
    assert 1 * s * 2 > 2 ** 32                                             # bf16: row 1 lies past 2^32 bytes
    assert 2 * s > 2 ** 32                                                 # bf16: row 2 lies past 2^32 elements
    assert 1 * s * 4 > 8 * 2 ** 30                                         # fp32 / int32: row 1 lies past 8 GiB
    assert 2 * s * 2 + 63 * 2 ** 20 <= FR.BUFFER_BYTES                     # 63 MiB of rows and guards behind the last far row
    assert 1 * s * 4 + 63 * 2 ** 20 <= FR.BUFFER_BYTES
    assert (2 * s) % FR.ALIGN == 0 and (4 * s) % FR.ALIGN == 0
    assert s > 2 ** 31 - 1 and (2 * s) >> 32 != 0                          # the stride fits no int, a row-1 byte offset no unsigned


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.int32])
def test_rows_are_aligned_compact_inside_and_apart(dtype):
    buf = _buf()
    isz = torch.empty((), dtype=dtype).element_size()
    rows = NBYTES // (STRIDE * isz)
    assert rows >= 2
    views = [buf.far((rows, 5, 3, 8), dtype), buf.far((rows, 1003), dtype), buf.far((rows,), dtype)]
    for v in views:
        assert v.stride(0) == STRIDE and tuple(v.stride()[1:]) == tuple(torch.empty(v.shape[1:]).stride())
        for b in range(rows):
            assert _byte0(buf, v[b]) % FR.ALIGN == 0
    spans = sorted(buf.live)
    assert len(spans) == 3 * rows == len(buf.handed_out)
    assert spans[0][0] >= GUARD and spans[-1][1] + GUARD <= NBYTES
    for (lo, hi), (lo2, hi2) in zip(spans, spans[1:]):
        assert hi + GUARD <= lo2, "two rows lie within a guard of each other"
    for lo, hi, row, side in buf.guards():
        assert hi - lo == GUARD and (hi == row[0] if side == "before" else lo == row[1])
    # a view holds what was written through it and nothing else moved
    ref = torch.arange(rows * 1003, dtype=torch.float32).view(rows, 1003).to(dtype)
    views[1].copy_(ref)
    assert torch.equal(views[1], ref)
    buf.check_guards()
    buf.scan_untouched()


def test_far_like_copies_values_and_a_too_large_view_is_refused():
    buf = _buf()
    t = torch.randn(2, 7, 16)
    v = buf.far_like(t)
    assert torch.equal(v, t) and v.stride(0) == STRIDE
    with pytest.raises(AssertionError, match="past the buffer"):
        buf.far((NBYTES // (STRIDE * 4) + 2, 4), torch.float32)
    with pytest.raises(AssertionError, match="alignment"):
        buf.far((2, 4), torch.float32, batch_stride=STRIDE + 1)


@pytest.mark.parametrize("where", ["before", "after", "far"])
def test_one_byte_outside_a_row_is_caught_and_writes_inside_are_accepted(where):
    buf = _buf()
    v = buf.far((2, 1000), torch.float32)
    w = buf.far((2, 33), torch.int32)
    v.fill_(1.0)
    w.fill_(7)
    buf.check_guards()
    buf.scan_untouched()
    lo, hi = sorted(buf.live)[2]                       # row 1 of v
    at = {"before": lo - 1, "after": hi, "far": NBYTES - 100}[where]
    if where == "far":
        assert all(not (g[0] <= at < g[1]) for g in buf.guards()) and all(not (r[0] <= at < r[1]) for r in buf.live)
    buf.buf[at] = 0
    if where == "far":
        buf.check_guards()                             # outside every guard: only the scan sees it
    else:
        with pytest.raises(AssertionError, match=f"first at byte {at}"):
            buf.check_guards()
    with pytest.raises(AssertionError, match=f"first at byte {at}"):
        buf.scan_untouched()
    buf.buf[at] = FR.SENTINEL
    buf.release()
    assert not buf.live and buf.cursor == GUARD
    buf.scan_untouched()                               # released rows hold the sentinel again
    assert _byte0(buf, buf.far((2, 8), torch.float32)) == GUARD


def test_a_stride_truncated_to_32_bits_is_not_the_far_stride():
    s = FR.FAR_STRIDE
    assert C.c_int64(s).value == s
    assert C.c_int32(s).value != s and C.c_uint32(2 * s).value != 2 * s       # an int stride; an unsigned row-2 / byte offset
    assert C.c_int32(-s).value != -s


# ---------------------------------------------------------------------------------------------- sizes
@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


GENERIC, FUSED = 1, 2
_BY_QUERY = {r[1]: r for r in ROWS}
_EW_GENERIC = dict(path=GENERIC, N=64, dk=32, V=3, r=2, precision=0)

# (id, the row of test_entry_refusals_cpu whose fill is used, its support query or None for a path that takes every shape,
#  ("struct:<name>": a bare struct), whether the query is asked, size exports, fill overrides, the extent that is doubled, its first value, "affine" | "bounded")
SIZES = [
    ("sdpa_fused", "mopk_sdpa_fused_supported", True, ("mopk_sdpa_saved_bytes", "mopk_sdpa_workspace_bytes"), dict(N=4096), "B", 64, "affine"),
    ("sdpa_generic", "mopk_sdpa_fused_supported", False, ("mopk_sdpa_saved_bytes", "mopk_sdpa_workspace_bytes"),
     dict(path=GENERIC, N=64), "B", 64, "affine"),
    ("sdpa_lens_fused", "mopk_sdpa_lens_supported", True, ("mopk_sdpa_lens_saved_bytes", "mopk_sdpa_lens_workspace_bytes"),
     {"base.N": 4096}, "base.B", 64, "affine"),
    ("sdpa_lens_generic", "mopk_sdpa_lens_supported", False, ("mopk_sdpa_lens_saved_bytes", "mopk_sdpa_lens_workspace_bytes"),
     {"base.path": GENERIC, "base.N": 64}, "base.B", 64, "affine"),
    ("dualpath_fused", "mopk_dualpath_fused_supported", True, ("mopk_dualpath_saved_bytes", "mopk_dualpath_workspace_bytes"),
     dict(N=1024), "B", 64, "affine"),
    ("dualpath_generic", "mopk_dualpath_fused_supported", False, ("mopk_dualpath_saved_bytes", "mopk_dualpath_workspace_bytes"),
     dict(path=GENERIC, N=64), "B", 64, "affine"),
    ("quartet_fused", "mopk_quartet_fused_supported", True, ("mopk_quartet_saved_bytes", "mopk_quartet_workspace_bytes"),
     dict(T=1024), "B", 64, "affine"),
    ("quartet_generic", "mopk_quartet_fused_supported", False, ("mopk_quartet_saved_bytes", "mopk_quartet_workspace_bytes"),
     dict(path=GENERIC, T=64), "B", 64, "affine"),
    ("edgewise_fused", "mopk_edgewise_fused_supported", True, ("mopk_edgewise_saved_bytes", "mopk_edgewise_workspace_bytes"),
     dict(path=FUSED), "B", 4096, "affine"),          # past the persistent grid's cap: one hand-off slab per (b, h) from there on
    ("edgewise_generic", "mopk_edgewise_fused_supported", False, ("mopk_edgewise_saved_bytes", "mopk_edgewise_workspace_bytes"),
     _EW_GENERIC, "B", 64, "affine"),
    ("decode_attn", "mopk_decode_attn_supported", True, ("mopk_decode_attn_workspace_bytes",), dict(Tq=16, dk=128), "B", 64, "affine"),
    ("decode_attn_rows", "mopk_decode_attn_rows_supported", True, ("mopk_decode_attn_rows_workspace_bytes",),
     {"base.Tq": 16, "base.dk": 128}, "base.B", 64, "affine"),
    ("decode_attn_ragged", "mopk_decode_attn_ragged_supported", True, ("mopk_decode_attn_ragged_workspace_bytes",),
     {"base.Tq": 16, "base.dk": 128}, "base.B", 64, "affine"),
    ("decode_attn_lens", "mopk_decode_attn_lens_supported", True, ("mopk_decode_attn_lens_workspace_bytes",),
     {"base.Tq": 16, "base.dk": 128}, "base.B", 64, "affine"),
    ("beam", "mopk_beam_supported", True, ("mopk_beam_workspace_bytes",), dict(K=8), "B", 4096, "affine"),   # past BS_TARGET_WG rows: one slice each
    ("dtw", "mopk_dtw_align_supported", True, ("mopk_dtw_workspace_bytes",), dict(N=64, M=1024, cost_ld=1024), "B", 64, "affine"),
    ("log_mel", "mopk_log_mel_supported", True, ("mopk_log_mel_workspace_bytes",), dict(L=1600000, audio_ld=1600000, out_dtype=1), "B", 64, "affine"),
    ("crossview", "struct:CrossViewArgs", False, ("mopk_crossview_saved_bytes", "mopk_crossview_workspace_bytes"),
     dict(H=1, N=64, dk=32, use_prior=1), "B", 64, "affine"),
    ("layernorm", "struct:LayerNormArgs", False, ("mopk_layernorm_workspace_bytes",), dict(dim=8192), "rows", 2 ** 16, "bounded"),
    ("token_gate", "mopk_token_gate_supported", True, ("mopk_token_gate_workspace_bytes",), dict(D=1024, x_st=1024, a_st=1024), "B", 2 ** 16, "bounded"),
    ("mel_gate", "mopk_mel_gate_supported", True, ("mopk_mel_gate_workspace_bytes",), dict(F=128, mel_st=128, L=8), "B", 2 ** 16, "bounded"),
]


def _size_row(lib, spec):
    from mop_amd import _lib
    name, query, _, exports, over, extent, first, kind = spec
    if query.startswith("struct:"):                    # no row in the refusal table: a bare struct
        a, keep = getattr(_lib, query[7:])(), None
    else:
        a, _, keep = _filled(_BY_QUERY[query])
    for k, v in over.items():
        _set(a, k, v)
    return a, keep


@pytest.mark.parametrize("spec", SIZES, ids=[s[0] for s in SIZES])
def test_size_exports_are_exact_in_64_bits(lib, spec):
    name, query, asks, exports, over, extent, first, kind = spec
    a, keep = _size_row(lib, spec)

    def f(export, n):
        _set(a, extent, n)
        ok = bool(getattr(lib, query)(C.byref(a))) if asks else True
        return ok, int(getattr(lib, export)(C.byref(a)))

    for export in exports:
        crossed, n = set(), first
        while 4 * n <= 2 ** 31 - 1:
            (ok1, f1), (ok2, f2), (ok4, f4) = f(export, n), f(export, 2 * n), f(export, 4 * n)
            for ok, size, m in ((ok1, f1, n), (ok2, f2, 2 * n), (ok4, f4, 4 * n)):
                if asks and not ok:
                    assert size == 0, f"{export}: {extent} = {m} is refused by {query}, yet the size is {size}"
            if ok1 and ok2 and ok4:
                if kind == "affine":
                    assert f1 > 0 and f2 > f1 and f4 > f2, f"{export}: not increasing at {extent} = {n}: {f1}, {f2}, {f4}"
                    assert f4 - f2 == 2 * (f2 - f1), f"{export}: not affine at {extent} = {n}: {f1}, {f2}, {f4}"
                    crossed |= {e for e in (31, 32) if f1 < 2 ** e <= f4}
                else:
                    assert 0 < f1 == f2 == f4 < 2 ** 31, f"{export}: not constant under 2^31 at {extent} = {n}: {f1}, {f2}, {f4}"
            n *= 2
        if kind == "affine":
            assert crossed == {31, 32}, f"{export}: the sweep of {extent} never took the size across 2^31 and 2^32 bytes ({crossed})"
