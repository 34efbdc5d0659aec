"""CPU checks of tests/moe_ref.py (no GPU): the prescribed gates give the prescribed argmax in float64 with the promised margin and
dtype-exact values; counts_to_route gives the counts in each order; and every router case of test_gpu_moe_routes.py is fit to
judge a router: at most 0.1 % of its tokens are undecided under the rounding bound, and an fp32 torch evaluation of the same
operands stays inside that bound."""
import pytest
import torch
import torch.nn.functional as F

import moe_ref as R

ORDERS = ["sorted", "reversed", "shuffled"]


def _counts(E):
    c = [(7 * e) % 5 for e in range(E)]          # zeros included (e = 0, 5, ...)
    c[-1] += 3
    return c


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("D", [8, 72])
@pytest.mark.parametrize("E", [2, 10, 64])
def test_prescribed_gate_gives_the_prescribed_argmax(E, D, order, dtype):
    route = R.counts_to_route(_counts(E), order, seed=E + D)
    M = route.numel()
    xp, gw, gb = R.prescribed_gate(route, D, E, dtype)
    if E <= D:
        assert gw.dtype == gb.dtype == dtype
    else:
        assert gw.dtype == gb.dtype == torch.float32
    assert xp.dtype == dtype and gw.shape == (E, D) and gb.shape == (E,) and xp.shape[0] == M
    for t in (xp, gw) + ((gb,) if E <= D else ()):                  # exact in both dtypes
        assert torch.equal(t.to(torch.bfloat16).double(), t.double())
    x = R.patched(torch.randn(M, D, generator=torch.Generator().manual_seed(1)).to(dtype), xp)
    assert x.dtype == dtype and torch.equal(x[:, :xp.shape[1]].double(), xp.double())
    logits, beta = R.route_ref64(x, gw, gb)
    assert torch.equal(logits.argmax(-1), route)
    top2 = logits.topk(2, dim=-1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) >= R.MARGIN
    top1, decided = R.decide(logits, beta)
    assert torch.equal(top1, route) and bool(decided.all())


@pytest.mark.parametrize("counts", [(3, 0, 2), (0, 0, 5), (1,) * 64, (0, 70, 0, 0, 58, 0)])
def test_counts_to_route(counts):
    E, M = len(counts), sum(counts)
    s = R.counts_to_route(counts, "sorted")
    assert s.dtype == torch.int64 and s.numel() == M
    assert torch.equal(torch.bincount(s, minlength=E), torch.tensor(counts))
    assert bool((s[1:] >= s[:-1]).all())
    assert torch.equal(R.counts_to_route(counts, "reversed"), s.flip(0))
    a, b = R.counts_to_route(counts, "shuffled", seed=3), R.counts_to_route(counts, "shuffled", seed=3)
    assert torch.equal(a, b) and torch.equal(torch.bincount(a, minlength=E), torch.tensor(counts))
    if M > 8 and sum(c > 0 for c in counts) > 1:
        assert not torch.equal(a, s)
    with pytest.raises(ValueError):
        R.counts_to_route(counts, "random")


def test_decide_and_admissible_on_a_hand_made_case():
    logits = torch.tensor([[1.0, 1.0, 0.0], [0.0, 2.0, 1.0], [0.5, 0.0, 0.5 - 1e-9]], dtype=torch.float64)
    beta = torch.full_like(logits, 1e-8)
    top1, decided = R.decide(logits, beta)
    assert top1.tolist() == [0, 1, 0] and decided.tolist() == [False, True, False]
    assert R.admissible(logits, beta, torch.tensor([1, 1, 2])).tolist() == [True, True, True]
    assert R.admissible(logits, beta, torch.tensor([2, 2, 1])).tolist() == [False, False, False]


def test_route_ref64_widens_bf16_exactly_and_counts_the_bias():
    x = torch.tensor([[1.0, -2.0] + [0.0] * 6]).to(torch.bfloat16)
    gw = torch.tensor([[0.5, 0.25] + [0.0] * 6, [-1.0, 1.0] + [0.0] * 6])
    logits, beta = R.route_ref64(x, gw, torch.tensor([0.125, -3.0]))
    assert logits.dtype == beta.dtype == torch.float64
    assert logits.tolist() == [[0.125, -6.0]]
    assert beta.tolist() == [[8 * 2.0 ** -24 * 1.125, 8 * 2.0 ** -24 * 6.0]]
    assert R.route_ref64(x, gw)[1].tolist() == [[8 * 2.0 ** -24 * 1.0, 8 * 2.0 ** -24 * 3.0]]
    assert R.route_ref64(torch.zeros(1, 136), torch.zeros(2, 136))[1].tolist() == [[0.0, 0.0]]


@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=R.case_id)
def test_router_case_is_fit_to_judge_a_router(case):
    x, gw, gb = R.router_case(*case)
    logits, beta = R.route_ref64(x, gw, gb)
    top1, decided = R.decide(logits, beta)
    share = 1.0 - float(decided.double().mean())
    got = F.linear(x.float(), gw.float(), None if gb is None else gb.float()).double()
    ratio = float(((got - logits).abs() / beta).max())
    print(f"{R.case_id(case)}: undecided share {share:.4%}, fp32 torch error {ratio:.3f} beta")
    assert share <= R.UNDECIDED_CAP
    assert ratio <= 1.0
    assert bool(R.admissible(logits, beta, got.argmax(-1)).all())
