"""-m gpu: the two-launch beam step (mopk_beam_step) on the logits, states and layouts of tests/beam_rows.py, one launch per case
(two where a second call is the point), against the float64 reference of the documented step: the nine state tensors, integers bit
for bit, infinities equal, finite scores within the derived rounding bound (stored hypotheses' scores within bound / norm plus
rtol = 1e-5 for the powf normalisation), poisoned hist / rows columns untouched.  Families: beam counts K = 1 .. 8, 2K candidates in
one thread's registers, row edges and degenerate geometries, ties, the walk, the lse, the reorder beyond one column block.  One
guarded run per family (workspace, logits and state between guard bands) and one alignment-independence check.
test_beam_rows_cpu shows without a GPU that every case is decided under the bound."""
import dataclasses

import pytest
import torch

import beam_rows as R
from guarded_alloc import BAND, embedded, guarded_allocations

pytestmark = pytest.mark.gpu
INTS = [n for n in R.FIELDS if n not in ("scores", "fin_scores")]


def _buffer(t):
    """the whole uint8 buffer that an embedded() tensor lies in"""
    buf = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    assert t.data_ptr() - buf.data_ptr() == BAND
    return buf


def _steps(c, x, st):
    from mop_amd import _lib, ops
    pos = torch.tensor([c.pos], dtype=torch.int32, device="cuda")
    for _ in range(c.calls):
        ops.beam_step(x, st, pos)
        assert ops.LAST_PATH["beam_step"] == _lib.PATH_FUSED, c.name
        pos += 1


def _run(c, contiguous=False):
    st, wide = c.state("cuda", contiguous)
    _steps(c, c.logits("cuda", contiguous), st)
    return R.state_dict(st), wide


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_family(family):
    frac = 0.0
    for c in R.cases(family):
        got, wide = _run(c)
        frac = max(frac, R.compare(c, R.reference(c), got, wide))
    print(f"{family}: {len(R.cases(family))} cases, the kernel uses {frac:.3f} of the bound at most")
    assert frac <= 1.0


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_guarded_run(family):
    """the workspace from guarded_allocations(), the logits and every state tensor embedded in poison: no byte outside them changes
    and the results are those of the plain run, bit for bit"""
    c = R.case(family, R.GUARDED[family])
    plain, _ = _run(c, contiguous=True)
    st, _ = c.state("cuda", contiguous=True)
    x = embedded(c.logits("cuda", contiguous=True))
    for n in R.FIELDS:
        setattr(st, n, embedded(getattr(st, n)))
    held = [x] + [getattr(st, n) for n in R.FIELDS]
    before = [_buffer(t).clone() for t in held]
    with guarded_allocations() as ledger:
        _steps(c, x, st)
        torch.cuda.synchronize()
    assert ledger.count() >= c.calls and ledger.intact(), ledger.describe_damage()
    for t, b in zip(held, before):
        n = t.numel() * t.element_size()
        assert torch.equal(_buffer(t)[:BAND], b[:BAND]) and torch.equal(_buffer(t)[BAND + n:], b[BAND + n:]), c.name
    assert torch.equal(_buffer(x), before[0])             # the logits are read only
    got = R.state_dict(st)
    for n in R.FIELDS:
        assert torch.equal(got[n].view(torch.int32), plain[n].view(torch.int32)), (c.name, n)
    R.compare(c, R.reference(c, contiguous=True), got)


def test_integer_outputs_do_not_depend_on_the_alignment():
    """one (B * K, V) content at two base alignments: other heads, tails, slice edges and addition orders, the same integers"""
    for name in ("counts-K5-B3-f32", "counts-K8-B3-bf16"):
        c = R.case("beam_counts", name)
        a, _ = _run(c)
        for off in (1, 3):
            d = dataclasses.replace(c, offset=off)
            b, _ = _run(d)
            R.compare(d, R.reference(d), b)
            for n in INTS:
                assert torch.equal(a[n], b[n]), (name, off, n)
