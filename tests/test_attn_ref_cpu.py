"""no GPU: the float64 attention references the edge-case tests rely on (tests/attn_ref.py, the oracles' empty-row convention)
against torch's own float64 SDPA, the logit-scale generator, and the refusal of a bias that requires grad (raised before any
kernel runs)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attn_ref import blocked_rows_mask, logit_qk, logit_std, sdpa_ref64


def _torch_sdpa(q, k, v, mask):
    """(B,N,H,dk) layout around F.scaled_dot_product_attention"""
    y = F.scaled_dot_product_attention(*(t.transpose(1, 2) for t in (q, k, v)), attn_mask=mask)
    return y.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


@pytest.mark.parametrize("kind", ["bool", "minus_inf_bias"])
def test_sdpa_ref64_matches_torch_sdpa_with_blocked_rows(kind):
    g = torch.Generator().manual_seed(0)
    B, N, Nk, H, dk = 2, 70, 130, 2, 16
    q, k, v = (torch.randn(B, n, H, dk, generator=g, dtype=torch.float64, requires_grad=True) for n in (N, Nk, Nk))
    keep = torch.stack([blocked_rows_mask(N, Nk, g, "cpu") for _ in range(B)]).unsqueeze(1)
    w = torch.randn(B, N, H * dk, generator=g, dtype=torch.float64)
    if kind == "bool":
        y = sdpa_ref64(q, k, v, mask=keep)
        mask = keep
    else:
        bias = torch.zeros(keep.shape, dtype=torch.float64).masked_fill(~keep, float("-inf"))
        y = sdpa_ref64(q, k, v, bias=bias)
        mask = bias
    grads = torch.autograd.grad((y * w).sum(), (q, k, v))
    yt = _torch_sdpa(q, k, v, mask)
    gt = torch.autograd.grad((yt * w).sum(), (q, k, v))
    empty = ~keep[:, 0].any(-1)
    assert empty[:, 0].all() and empty[:, N - 2].all() and not empty[:, 1].any() and not empty[:, N - 1].any()
    assert (y.detach()[empty] == 0).all() and (yt.detach()[empty] == 0).all()
    assert torch.allclose(y, yt, rtol=0, atol=1e-12)
    for a, b in zip(grads, gt):
        assert torch.isfinite(a).all() and torch.allclose(a, b, rtol=0, atol=1e-12)
    assert (grads[0][empty] == 0).all()


def test_sdpa_ref64_causal_matches_torch():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(1, 65, 2, 8, generator=g, dtype=torch.float64) for _ in range(3))
    y = sdpa_ref64(q, k, v, causal=True)
    yt = F.scaled_dot_product_attention(*(t.transpose(1, 2) for t in (q, k, v)), is_causal=True).transpose(1, 2).reshape(1, 65, -1)
    assert torch.allclose(y, yt, rtol=0, atol=1e-12)


def test_blocked_rows_mask_holds_every_hard_row():
    keep = blocked_rows_mask(197, 200, torch.Generator().manual_seed(2), "cpu")
    assert not keep[0].any() and not keep[195].any()
    assert keep[1].nonzero().flatten().tolist() == [0]
    assert keep[196].nonzero().flatten().tolist() == [199]
    assert not keep[2, :64].any() and keep[2, 64:].any()
    rest = keep[3:195].float().mean()
    assert 0.65 < float(rest) < 0.75


@pytest.mark.parametrize("sigma", [1, 4, 8, 16, 32])
def test_logit_scale_generator_reaches_its_target(sigma):
    q, k = logit_qk((1, 200, 2, 64), (1, 300, 2, 64), sigma, torch.Generator().manual_seed(sigma), "cpu")
    assert abs(logit_std(q, k) / sigma - 1.0) < 0.05


def test_oracle_masked_softmax_gives_an_empty_row_zero():
    from oracle.multihop import _masked_softmax
    S = np.random.default_rng(0).standard_normal((2, 4, 5))
    blocked = np.zeros(S.shape, dtype=bool)
    blocked[0, 1] = True                     # every key of one row
    blocked[1, 2, :4] = True                 # one open key
    with np.errstate(all="raise"):           # no -inf - -inf, no 0 / 0
        P = _masked_softmax(S, blocked)
    assert (P[0, 1] == 0).all()
    assert P[1, 2, 4] == 1.0 and (P[1, 2, :4] == 0).all()
    keep = ~blocked[0, 0]
    assert np.allclose(P[0, 0], np.exp(S[0, 0]) / np.exp(S[0, 0]).sum()) and keep.all()


def test_oracle_multihop_with_a_fully_blocked_row_is_finite_and_zero_there():
    from oracle import multihop as om
    rng = np.random.default_rng(3)
    B, H, N, dk = 1, 2, 9, 4
    ts = [rng.standard_normal((B, H, N, dk)) for _ in range(6)]
    blocked = rng.random((B, 1, N, N)) < 0.3
    blocked[..., np.arange(N), np.arange(N)] = False
    blocked[..., 4, :] = True
    gates = dict(and_=0.8, or_=0.4, not_=0.3, chain=0.2)
    y, c = om.core_fwd(*ts, gates, 0.6, 3, -0.5, blocked)
    g = om.core_bwd(rng.standard_normal(y.shape), c)
    assert np.isfinite(y).all() and all(np.isfinite(np.asarray(x)).all() for x in g.values())
    assert (y[:, :, 4] == 0).all() and (g["dq1"][:, :, 4] == 0).all() and (g["dq2"][:, :, 4] == 0).all()
    # the blocked row takes no part: the other rows are what the oracle gives with that row's queries changed
    ts2 = [t.copy() for t in ts]
    ts2[0][:, :, 4] += 1.0
    ts2[3][:, :, 4] -= 1.0
    y2, _ = om.core_fwd(*ts2, gates, 0.6, 3, -0.5, blocked)
    assert np.allclose(np.delete(y, 4, 2), np.delete(y2, 4, 2), rtol=0, atol=1e-12)


def test_a_bias_that_requires_grad_is_refused():
    """the cores compute no gradient for an additive bias: the refusal comes before any kernel (CPU tensors reach it)"""
    from mop_amd import ops
    q = torch.randn(1, 8, 2, 16)
    bias = torch.zeros(1, 1, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="sdpa_core: bias requires grad"):
        ops.sdpa_core(q, q, q, bias=bias)
    with pytest.raises(NotImplementedError, match="quartet_core: add_mask requires grad"):
        ops.quartet_core(q, q, q, None, None, None, None, bias, 1e-5, False)
