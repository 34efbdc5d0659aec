"""-m gpu: the top-k / top-p thresholds of the sampling kernel (mopk_sample_*, mopk_sample_ragged_*), draw by draw against the exact
kept set and Gumbel-max of tests/sample_rows.py.  One logit row shared by 4096 output rows at 4 positions (fewer rows at V = 16385):
the kernel's token is the reference winner in every draw outside the near ties and one of its top two inside them, so the smallest
kept tie group is drawn wherever the reference draws it and the largest excluded one never is; test_whisper_sample_filters_cpu
proves on the reference alone that both groups win at least 16 draws of every case outside UNWITNESSED.  Row families: radix depth,
ties at the threshold, masked rows, mass underflow, geometric masses, thread-stride edges, bf16 storage; each once through the
ragged op."""
import pytest
import torch

import sample_rows as S

pytestmark = pytest.mark.gpu


def _names(family):
    return [c.name for c in S.cases(family)]


def _case(family, name):
    return next(c for c in S.cases(family) if c.name == name)


def _check_logprobs(c, x, toks, lps):
    """within 1e-5 of the float64 log_softmax of the unscaled row; infinities equal; the -inf-only row has none (NaN on both sides)"""
    ref = torch.log_softmax(x[0].double(), -1)
    for tok, lp in zip(toks, lps):
        want = ref[tok.long()]
        fin, inf = torch.isfinite(want), torch.isinf(want)
        assert bool(((lp[fin].double() - want[fin]).abs() <= 1e-5).all()), c.name
        assert torch.equal(lp[inf].double(), want[inf]) and bool(torch.isnan(lp[torch.isnan(want)]).all()), c.name


def _run(c, ragged=False):
    from mop_amd import _lib, ops
    x = c.logits("cuda")
    assert x.data_ptr() % 16 == (c.offset * x.element_size()) % 16
    off = S.pos_offsets(c.R, "cuda") if ragged else None
    ref = S.reference(c, "cuda", pos_off=off)
    out = (torch.empty(c.R, dtype=torch.int32, device="cuda"), torch.empty(c.R, device="cuda"))
    toks, lps = [], []
    for p in range(c.P):
        pos = torch.tensor([S.POS0 + p], dtype=torch.int32, device="cuda")
        if ragged:
            ops.sample_tokens_ragged(x, pos, off, c.temperature, c.top_k, c.top_p, S.SEED, out=out)
            assert ops.LAST_PATH["sample_ragged"] == _lib.PATH_FUSED
            zero = ops.sample_tokens_ragged(x, pos, torch.zeros_like(off), c.temperature, c.top_k, c.top_p, S.SEED,
                                            out=(torch.empty_like(out[0]), torch.empty_like(out[1])))
            plain = ops.sample_tokens(x, pos, c.temperature, c.top_k, c.top_p, S.SEED,
                                      out=(torch.empty_like(out[0]), torch.empty_like(out[1])))
            assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1].view(torch.int32), plain[1].view(torch.int32)), c.name
        else:
            ops.sample_tokens(x, pos, c.temperature, c.top_k, c.top_p, S.SEED, out=out)
            assert ops.LAST_PATH["sample"] == _lib.PATH_FUSED
        toks.append(out[0].clone())
        lps.append(out[1].clone())
    what = S.describe(c, ref, toks)
    wrong, off2 = S.compare_draws(toks, ref)
    print(f"{c.name}: draws={ref.n} near={ref.near} low_wins={ref.low_wins} excl_wins={ref.excl_wins} kept={ref.kept.count} "
          f"wrong={wrong} near_off={off2}")
    assert wrong == 0, what                               # the reference winner in every draw that is no near tie
    assert off2 == 0, what                                # one of the reference's top two in the near ties
    seen = torch.zeros(c.x.shape[0], dtype=torch.bool)
    seen[torch.unique(torch.cat(toks).long()).cpu()] = True
    assert int(torch.cat(toks).min()) >= 0 and int(torch.cat(toks).max()) < c.x.shape[0], what
    assert not bool((seen & ~ref.kept.keep).any()), what   # inside the exact kept set ...
    assert not bool((seen & ref.kept.excl).any()), what    # ... so never from the largest excluded tie group
    if c.name not in S.UNWITNESSED:
        assert bool((seen & ref.kept.low).any()) and ref.low_wins >= 16, what     # the smallest kept tie group is drawn
    _check_logprobs(c, x, toks, lps)
    if not ragged and not bool(torch.isfinite(c.x.float()).any()):               # the -inf-only row: the torch path's token
        tt, _ = ops.sample_tokens_torch(x, pos, c.temperature, c.top_k, c.top_p, S.SEED,
                                        out=(torch.empty_like(out[0]), torch.empty_like(out[1])))
        assert torch.equal(toks[-1], tt), what


@pytest.mark.parametrize("name", _names("radix_depth"))
def test_radix_depth(name):
    _run(_case("radix_depth", name))


@pytest.mark.parametrize("name", _names("threshold_ties"))
def test_ties_at_the_threshold(name):
    _run(_case("threshold_ties", name))


@pytest.mark.parametrize("name", _names("masked_rows"))
def test_masked_rows(name):
    _run(_case("masked_rows", name))


@pytest.mark.parametrize("name", _names("mass_underflow"))
def test_mass_underflow(name):
    _run(_case("mass_underflow", name))


@pytest.mark.parametrize("name", _names("geometric"))
def test_geometric_masses(name):
    _run(_case("geometric", name))


@pytest.mark.parametrize("name", _names("stride_edges"))
def test_thread_stride_edges(name):
    _run(_case("stride_edges", name))


@pytest.mark.parametrize("name", _names("bf16_storage"))
def test_bf16_storage(name):
    _run(_case("bf16_storage", name))


@pytest.mark.parametrize("name", [c.name for c in S.ragged_cases()])
def test_ragged(name):
    _run(next(c for c in S.ragged_cases() if c.name == name), ragged=True)
