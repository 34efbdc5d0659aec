"""CPU checks of the sampling filters' test rows (no GPU; tests/sample_rows.py).  For every case ops.sample_tokens_torch equals the
exact reference draw by draw outside the near ties, and the reference alone proves what keeps the GPU test from hiding a failure:
few near ties, both deciding tie groups winning at least 16 draws (or the case named in UNWITNESSED), a top-p margin of at least
1e-4, the rows exercising the radix levels they were built for.  kept_exact against the plain-Python restatement on the hand-built
rows of test_whisper_sample_cpu; and the teeth of the comparison: a threshold one tie group off in either direction fails it."""
import functools

import pytest
import torch

import sample_rows as S
from test_whisper_sample_cpu import ROWS, f32, py_sample

CASES = S.all_cases()
NAMES = [c.name for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
SHIFTS = [(c.name, s) for c in CASES if c.name not in S.UNWITNESSED for s in (1, -1) if c.kept(s) is not None]


@functools.lru_cache(maxsize=None)
def _reference(name):
    return S.reference(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _torch_tokens(name):
    from mop_amd import ops
    c = BY_NAME[name]
    x, toks = c.logits("cpu"), []
    for p in range(c.P):
        out = (torch.zeros(c.R, dtype=torch.int32), torch.zeros(c.R))
        ops.sample_tokens_torch(x, torch.tensor([S.POS0 + p], dtype=torch.int32), c.temperature, c.top_k, c.top_p, S.SEED, out=out)
        toks.append(out[0])
    return toks


def test_every_family_is_there():
    assert len(set(NAMES)) == len(NAMES)
    assert {c.x.shape[0] for c in S.cases("stride_edges")} == {2, 3, 1023, 1024, 1025, 16385}
    assert all(c.x.shape[0] <= 1025 and c.R * c.P == 16384 for c in CASES if c.x.shape[0] != 16385)
    assert all(c.R * c.x.shape[0] * 8 <= 200e6 for c in CASES)                  # the widest reference array (int64 hashes)
    assert {c.x.dtype for c in S.cases("bf16_storage")} == {torch.float32, torch.bfloat16}
    assert sum(c.offset != 0 for c in CASES) == 2
    for c in CASES:
        assert not torch.isnan(c.x.float()).any() and not torch.isposinf(c.x.float()).any()


@pytest.mark.parametrize("name", NAMES)
def test_torch_path_matches_the_reference(name):
    ref, toks = _reference(name), _torch_tokens(name)
    wrong, off = S.compare_draws(toks, ref)
    assert wrong == 0 and off == 0, S.describe(BY_NAME[name], ref, toks)
    seen = torch.unique(torch.cat(toks).long())
    assert bool(ref.kept.keep[seen].all()), S.describe(BY_NAME[name], ref, toks)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_witnesses_the_threshold(name):
    ref = _reference(name)
    assert ref.near <= 0.01 * ref.n
    if BY_NAME[name].top_p < 1:
        assert ref.kept.margin >= 1e-4
    if name in S.UNWITNESSED:
        return
    assert ref.low_wins >= 16                              # a threshold too tight loses these draws
    if bool(ref.kept.excl.any()):                         # a threshold too loose hands these draws to the excluded group
        assert ref.excl_wins >= 16
    else:                                                 # nothing finite is excluded: nothing can be added
        assert ref.excl_wins == 0


def test_unwitnessed_names_only_what_cannot_be_witnessed():
    assert set(S.UNWITNESSED) <= set(NAMES)
    for name in S.UNWITNESSED:
        ref = _reference(name)
        assert ref.low_wins < 16 or (bool(ref.kept.excl.any()) and ref.excl_wins < 16), name
        assert name.startswith(("peaked-", "masked-all"))


@pytest.mark.parametrize("name,shift", SHIFTS)
def test_a_threshold_one_tie_group_off_fails_the_comparison(name, shift):
    c = BY_NAME[name]
    right, moved = c.kept(), c.kept(shift)
    group = right.low if shift == 1 else right.excl      # the finite entries that change sides are exactly that tie group
    assert torch.equal((moved.keep ^ right.keep) & torch.isfinite(c.x.float()), group) and bool(group.any())
    wrong, _ = S.compare_draws(_torch_tokens(name), S.reference(c, shift=shift))
    assert wrong >= 16


def test_every_witnessed_case_with_a_neighbouring_group_has_teeth():
    shifted = {n for n, _ in SHIFTS}
    for c in CASES:
        if c.name in S.UNWITNESSED or c.name in shifted:
            continue
        k = c.kept()                                      # one finite tie group only: there is no other threshold to confuse it with
        assert not bool(k.excl.any()) and k.keep[torch.isfinite(c.x.float())].all(), c.name
        assert c.name.startswith(("all-equal", "masked-1")), c.name


@pytest.mark.parametrize("name", sorted(ROWS))
@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 1.0), (0.5, 3, 1.0), (2.0, 0, 0.6), (1.0, 4, 0.7), (0.25, 2, 0.9),
                                                     (1.0, 100, 1.0), (1.0, 1, 1.0), (4.0, 5, 0.3)])
def test_kept_exact_matches_the_python_restatement(name, temperature, top_k, top_p):
    x = [f32(v) for v in ROWS[name]]
    kept = py_sample(x, 0, 0, temperature, top_k, top_p, 0)[2]
    got = S.kept_exact(torch.tensor(x), temperature, top_k, top_p)
    assert set(got.keep.nonzero().flatten().tolist()) == kept and got.count == len(kept)


def _levels(name):
    c = BY_NAME[name]
    return S.radix_walk(c.x, c.temperature, c.top_k, c.top_p)


def test_rows_exercise_the_radix_levels_they_were_built_for():
    assert [lv[:2] for lv in _levels("depth-one-f32-k")] == [("top_k", 0)]
    assert [lv[:2] for lv in _levels("depth-one-f32-p")] == [("top_p", 0)]
    for f in ("k", "p"):
        lv = _levels("depth-mid-f32-" + f)                 # a window of about 2^16 keys: 512 keys per bin, then single keys
        assert len(lv) in (2, 3) and lv[0][1] == 9 and (lv[-1][1] == 0 or lv[-1][2]), lv
    for tag in ("f32", "bf16"):
        lv = _levels(f"depth-four-{tag}-kp")
        k_sh, p_sh = ([s for n, s, _ in lv if n == flt] for flt in ("top_k", "top_p"))
        # top-k from the widest shift: all four levels in fp32; bf16 values are 2^16 keys apart, so the walk ends early at shift 16
        assert k_sh == ([24, 16, 8, 0] if tag == "f32" else [24, 16]) and (tag == "f32" or lv[1][2]), lv
        assert 1 <= len(p_sh) <= 3 and p_sh[0] < 24 and p_sh[-1] == 0, lv          # top-p starts inside top-k's window
        assert [s for n, s, _ in _levels(f"depth-four-{tag}-p")][0] == 24
        lv = _levels(f"tie-ends-at-k-{tag}")
        assert lv[-1][2] and lv[-1][1] > 0, lv            # the early return, at a level of more than one key per bin
        assert not any(e for _, _, e in _levels(f"tie-straddles-k-{tag}"))
    c = BY_NAME["depth-four-f32-k"]
    z = c.x.float()
    assert bool((z == float("-inf")).any()) and float(z[torch.isfinite(z)].min()) <= -1e28 and bool((z > 0).any())


@pytest.mark.parametrize("name", [c.name for c in S.ragged_cases()])
def test_ragged_torch_path_matches_the_reference(name):
    from mop_amd import ops
    c = BY_NAME[name]
    off = S.pos_offsets(c.R, "cpu")
    ref = S.reference(c, pos_off=off)
    x, toks, plain = c.logits("cpu"), [], []
    for p in range(c.P):
        pos = torch.tensor([S.POS0 + p], dtype=torch.int32)
        out = (torch.zeros(c.R, dtype=torch.int32), torch.zeros(c.R))
        ops.sample_tokens_ragged_torch(x, pos, off, c.temperature, c.top_k, c.top_p, S.SEED, out=out)
        toks.append(out[0])
        out = (torch.zeros(c.R, dtype=torch.int32), torch.zeros(c.R))
        ops.sample_tokens_ragged_torch(x, pos, torch.zeros_like(off), c.temperature, c.top_k, c.top_p, S.SEED, out=out)
        plain.append(out[0])
    assert S.compare_draws(toks, ref) == (0, 0), S.describe(c, ref, toks)
    assert all(torch.equal(a, b) for a, b in zip(plain, _torch_tokens(name)))
    assert not all(torch.equal(a, b) for a, b in zip(toks, plain)) or c.kept().count == 1
