"""CPU checks of tests/beam_rows.py (no GPU): the model's slice count against mopk_beam_workspace_bytes, every case of every family
fit to judge a kernel (decided(), none excluded), planned cases walking their plan, ops.beam_step_torch on the CPU reproducing the
float64 reference inside the derived bound, the reference against the all-candidates oracle of test_whisper_beam_cpu, the two
rounding-collapse cases, the index limit of mopk_beam_supported, and the ownership the one_thread and edges cases claim."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import beam_rows as R
from test_whisper_beam_cpu import _oracle_step

FAMILIES = list(R.FAMILIES)


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _args(B, K, V, dtype, T=12):
    from mop_amd import _lib
    a = _lib.BeamArgs()
    a.B, a.K, a.V, a.T, a.eos, a.prompt_len, a.length_penalty = B, K, V, T, -1, 1, 1.0
    a.logits_dtype = _lib.MOPK_BF16 if dtype == torch.bfloat16 else _lib.MOPK_F32
    a.logits_sb, a.logits_sk, a.hist_ld, a.rows_ld = K * V, V, T, T
    return a


def test_model_slice_count_is_the_librarys(lib):
    shapes = {(c.B, c.K, c.V, c.dtype) for f in FAMILIES for c in R.cases(f)}
    shapes |= {(B, K, V, d) for B in (1, 2, 3, 8, 64, 600) for K in range(1, 9) for V in (2, 511, 512, 1023, 1024, 4099, 51865)
               for d in R.DTYPES}
    for B, K, V, d in shapes:
        n = lib.mopk_beam_workspace_bytes(C.byref(_args(B, K, V, d)))
        assert n == B * K * (2 + 4 * K) * 4 * R.nslice(B, K, V, d), (B, K, V, d)
        assert R.partition(V, d, 0, B, K).nslice == R.nslice(B, K, V, d)


def test_partition_covers_every_element_once():
    for V, d, mod, B, K in ((4099, torch.float32, 4, 1, 8), (4099, torch.bfloat16, 6, 1, 2), (1024, torch.float32, 4, 1, 2),
                            (3, torch.float32, 4, 2, 1), (2, torch.bfloat16, 14, 2, 8), (8192, torch.float32, 0, 37, 8)):
        p, E = R.partition(V, d, mod, B, K), R.epv(d)
        assert p.head + p.nvec * E == p.tail0 <= V and V - p.tail0 < E and (p.head < E or p.head == V)
        assert p.slices[0][0] == 0 and p.slices[-1][1] == p.nvec and all(a[1] == b[0] for a, b in zip(p.slices, p.slices[1:]))
        assert (mod + p.head * (16 // E)) % 16 == 0 or p.head == V
        for s, (u0, u1) in enumerate(p.slices):
            own = (p.slice == s) & (p.kind == R.VEC)
            assert int(own.sum()) == (u1 - u0) * E
            if u1 > u0:
                assert own[p.head + u0 * E] and own[p.head + u1 * E - 1]
        assert bool((p.slice[p.kind == R.HEAD] == 0).all()) and bool((p.slice[p.kind == R.TAIL] == p.nslice - 1).all())


@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_is_decided(family):
    for c in R.cases(family):
        assert R.decided(c) is None
        if c.name == R.GUARDED[family]:
            assert R.decided(c, contiguous=True) is None
    if family == "beam_counts":                               # the alignment check of the GPU file moves these two
        for name in ("counts-K5-B3-f32", "counts-K8-B3-bf16"):
            assert all(R.decided(dataclasses.replace(R.case(family, name), offset=off)) is None for off in (1, 3))


@pytest.mark.parametrize("family", FAMILIES)
def test_planned_cases_walk_their_plan(family):
    n = 0
    for c in R.cases(family):
        if c.plans is None:
            continue
        in_range = c.Tp <= c.pos < c.T
        for b, (plan, w) in enumerate(zip(c.plans, R.reference(c).calls[0])):
            if plan is None or not in_range:
                assert w is None
                continue
            assert [(q.k, q.flat - q.k * c.V) for q in w.cands[:w.n_read]] == R.expected_walk(plan, c.K, c.eos), (c.name, b)
            n += 1
        if in_range:
            assert R.min_gap(c) >= 1.0, c.name                # the builder's gaps between deciding candidates
    assert n > 0 or family in ("ties", "lse")


def _run_torch(c):
    from mop_amd import ops
    st, wide = c.state("cpu")
    x = c.logits("cpu")
    for i in range(c.calls):
        ops.beam_step_torch(x, st, torch.tensor([c.pos + i], dtype=torch.int32))
    return R.state_dict(st), wide


@pytest.mark.parametrize("family", FAMILIES)
def test_torch_composition_reproduces_the_reference(family):
    """an independent fp32 implementation decides every case: integers bit for bit, scores inside the bound"""
    frac = 0.0
    for c in R.cases(family):
        got, wide = _run_torch(c)
        frac = max(frac, R.compare(c, R.reference(c), got, wide))
    print(f"{family}: beam_step_torch on the CPU uses {frac:.3f} of the bound at most")
    assert frac <= 1.0


def _py_state(c):
    s = c.state0()
    fin = [[(float(s["fin_scores"][b, j]), s["fin_tokens"][b, j].tolist()) for j in range(int(s["fin_count"][b]))]
           for b in range(c.B)]
    return s["scores"].tolist(), s["hist"].tolist(), s["rows"].tolist(), fin, [bool(d) for d in s["done"]]


def test_reference_against_the_all_candidates_oracle():
    """on the inputs of test_beam_step_torch_matches_the_python_oracle (ties, a -inf row, eos finishing, a done item), where no two
    different logits of a beam round to one score and the per-beam cut therefore changes nothing"""
    torch.manual_seed(3)
    B, K, V, eos = 3, 3, 7, 5
    for step in range(4):
        lg = torch.randn(B * K, V) * 2
        lg[0:K, eos] += 3.0
        lg[K + 1, :] = R.NEG
        lg[2 * K:, eos] = torch.tensor([8.0, 7.0, 6.5])
        lg[2 * K, 0] = lg[2 * K, 4]
        sc = -torch.rand(B * K) * 3
        sc[4] = R.NEG
        c = R.Case(f"oracle-{step}", "oracle", B, K, lg, sc, eos=eos, lp=0.7, T=9, Tp=2, pos=3 + step, fin_count=[0, 2, 1],
                   done=[0, step % 2, 0])
        assert R.decided(c) is None
        full = R.reference(c)
        ref = full.state
        w_sc, w_hi, w_ro, w_fi, w_dn, w_par, w_nxt = _oracle_step(lg, *_py_state(c), c.pos, K, c.Tp, eos, c.lp)
        assert [bool(d) for d in ref["done"]] == w_dn
        for b in range(B):
            assert int(ref["fin_count"][b]) == len(w_fi[b])
            for j, (s, t) in enumerate(w_fi[b]):
                assert abs(float(ref["fin_scores"][b, j]) - s) <= full.tol_fin[b, j] + 1e-6 * abs(s)      # the oracle's lse is fp32
                assert ref["fin_tokens"][b, j, :len(t)].tolist() == t[:c.T]
            for r in range(b * K, (b + 1) * K):
                assert ref["hist"][r].tolist() == w_hi[r] and ref["rows"][r].tolist() == w_ro[r]
                if w_par[r] is not None:
                    assert (int(ref["parents"][r]), int(ref["next_ids"][r])) == (w_par[r], w_nxt[r])
                assert (ref["scores"][r] == w_sc[r] if full.tol_scores[r] == 0 else
                        abs(float(ref["scores"][r]) - w_sc[r]) <= full.tol_scores[r]), r


def test_the_per_beam_cut_decides_a_rounding_collapse():
    """K = 1: x[5] = 3.0 and x[2] = the fp32 below it round to one score.  The definition cuts each beam to its 2K largest logits
    first (eos and v = 5), so v = 5 becomes the live beam; ranking all K * V candidates by score would keep v = 2."""
    c = R.case("ties", "tie-collapse-cut-f32")
    x, info = c.x64()[0], R.row_info(c, 0)
    assert R.score32(c.scores[0].numpy(), x[5], info.lse) == R.score32(c.scores[0].numpy(), x[2], info.lse) and x[5] > x[2]
    assert float(R.score32(c.scores[0].numpy(), x[5], info.lse)) == -36.00495147705078
    ref = R.reference(c).state
    got, _ = _run_torch(c)
    assert int(ref["next_ids"][0]) == 5 and int(got["next_ids"][0]) == 5 and int(ref["fin_count"][0]) == 1


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_collapse_far_from_a_rounding_boundary_ties_to_the_smaller_index(dtype):
    """sc = -1e6: the logits 3 (v = 5) and 2.99 (v = 2) fall into one fp32 cell of the score, 8 beta_lse or more from its edges, so
    every evaluation ties them and the smaller flat index wins"""
    c = R.case("ties", f"tie-collapse-large-{dtype}")
    x, info, sc = c.x64()[0], R.row_info(c, 0), float(c.scores[0])
    s = R.score32(np.float32(sc), x[5], info.lse)
    assert s == R.score32(np.float32(sc), x[2], info.lse)
    lo = (float(s) + float(np.nextafter(s, np.float32(-np.inf)))) / 2
    hi = (float(s) + float(np.nextafter(s, np.float32(np.inf)))) / 2
    for v in (2, 5):
        real = sc + (x[v] - info.lse)
        assert min(real - lo, hi - real) >= 8 * info.beta_lse + 2 * R.U * abs(x[v] - info.lse), (v, real, lo, hi)
    got, _ = _run_torch(c)
    assert int(R.reference(c).state["next_ids"][0]) == 2 and int(got["next_ids"][0]) == 2


def test_support_query_at_the_index_limit(lib):
    """a support query allocates nothing: K * V must stay below the sentinel index 2^31 - 1"""
    ok = lambda K, V: lib.mopk_beam_supported(C.byref(_args(1, K, V, torch.bfloat16)))
    assert ok(7, 2 ** 28) == 1 and ok(8, 2 ** 28) == 0
    assert ok(1, 2 ** 31 - 2) == 1 and ok(1, 2 ** 31 - 1) == 0
    assert ok(8, 2 ** 28 - 1) == 1


def test_one_thread_cases_own_what_they_claim():
    for c in R.cases("one_thread"):
        assert c.B * c.K >= 256 and c.claims
        for r, mode, s, t in c.claims:
            p, top = c.part(r), R.row_info(c, r).top
            assert len(top) == 2 * c.K and p.chain >= 2 * c.K + R.epv(c.dtype)
            assert bool((p.slice[top] == s).all()) and bool((p.kind[top] == R.VEC).all()), (c.name, r)
            if mode == "thread":
                assert bool((p.thread[top] == t).all()), (c.name, r)
            else:
                assert len(set(p.thread[top].tolist())) > c.K, (c.name, r)
        assert {(m, s) for _, m, s, _ in c.claims} == {("thread", 0), ("slice", 0), ("slice", 1)} and c.part(0).nslice == 2


def test_edge_cases_own_what_they_claim():
    for dtype in R.DTYPES:
        E, seen = R.epv(dtype), {}
        for c in R.cases("edges"):
            if c.dtype != dtype or not c.claims:
                continue
            names = seen.setdefault(c.name, set())
            for (r, _, v, _), w in zip(c.claims, R.reference(c).calls[0]):
                sp = c.part(r).specials(E)
                assert w.cands[0].flat == v and w.cands[0].k == 0 and v in sp, (c.name, r)      # the item's best candidate
                names.add(sp[v])
                for k in range(c.K):                          # and every beam's 2K largest logits are special elements
                    assert set(R.row_info(c, r + k).top.tolist()) <= set(c.part(r + k).specials(E)), (c.name, r, k)
        assert len(seen) == E + 1
        for name, names in seen.items():
            p = R.case("edges", name).part(0)
            assert names == set(p.specials(E).values()), name
            assert {f"first{s}" for s in range(p.nslice)} | {f"last{s}" for s in range(p.nslice)} <= names
            assert ("head" in names) == (p.head > 0) and ("tail" in names) == (p.tail0 < p.kind.shape[0])
        assert any("head" in n and "tail" in n for n in seen.values())
        short = R.case("edges", f"edge-short-slices-{R.tag(dtype)}").part(0)
        assert [u1 - u0 for u0, u1 in short.slices] == [127, 128]
    small = [c for c in R.cases("edges") if c.V <= 9]
    assert {(c.V, c.offset, c.K, c.dtype) for c in small} == {(V, o, K, d) for d in R.DTYPES for V in range(2, 10)
                                                               for o in range(R.epv(d)) for K in (1, 8)}
    assert any(c.part(0).nvec == 0 for c in small) and any(c.part(0).head == c.V < R.epv(c.dtype) - 1 for c in small)
    gap = R.case("edges", "edge-row-gap-f32")
    assert gap.sk > gap.V and bool(torch.isnan(gap.logits("cpu").as_strided((gap.sk,), (1,))[gap.V:]).all())
    assert R.case("edges", "edge-shared-rows-bf16").shared
