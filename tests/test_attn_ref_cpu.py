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


# ---------------------------------------------------------------- the numpy oracles at head sizes outside 16 / 32 / 64
# tests/test_gpu_generic_head_sizes.py judges the generic kernels by these oracles at dk = 6 ... 128: here they are held, without a GPU,
# to float64 torch autograd of the plain formula at dk = 6, 12, 100, so a head-size assumption in a reference would show first
HEAD_SIZES = [6, 12, 100]
_OB, _OH, _ON = 2, 2, 20


def _oracle_inputs(n, dk, seed):
    g = torch.Generator().manual_seed(seed + dk)
    ts = [torch.randn(_OB, _ON, _OH, dk, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(n)]
    dy = torch.randn(_OB, _ON, _OH * dk, generator=g, dtype=torch.float64)
    return ts, dy


def _bhnd(t):
    """(B,N,H,dk) torch -> (B,H,N,dk) numpy, the oracle layout"""
    return t.detach().numpy().transpose(0, 2, 1, 3)


def _scores(q, k):
    """(B,N,H,dk) x (B,N,H,dk) -> (B,H,N,N) q k^T / sqrt(dk)"""
    return torch.einsum("bihd,bjhd->bhij", q, k) / q.shape[-1] ** 0.5


def _agree(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref, np.float64)
    assert got.shape == ref.shape or got.size == ref.size == 1, (what, got.shape, ref.shape)
    assert float(np.abs(got.reshape(ref.shape) - ref).max()) <= 1e-10, (what, float(np.abs(got.reshape(ref.shape) - ref).max()))


@pytest.mark.parametrize("dk", HEAD_SIZES)
def test_oracle_multihop_default_gates_is_sdpa_plus_transport_at_any_head_size(dk):
    """default gates: y = softmax(S1 + S2) v1 + sigmoid(w) A1 A2^(hops-1) v2 -- the first term through sdpa_ref64 on concatenated heads"""
    from oracle import multihop as om
    (q1, k1, v1, q2, k2, v2), dy = _oracle_inputs(6, dk, 10)
    hops, lg = 3, torch.tensor(-0.5, dtype=torch.float64, requires_grad=True)
    base = sdpa_ref64(torch.cat([q1, q2], -1), torch.cat([k1, k2], -1) * 2 ** 0.5, torch.cat([v1, v1], -1))    # (S1 + S2) at 1 / sqrt(2 dk)
    base = base.view(_OB, _ON, _OH, 2 * dk)[..., :dk].reshape(_OB, _ON, _OH * dk)
    A1, A2 = _scores(q1, k1).softmax(-1), _scores(q2, k2).softmax(-1)
    tr = v2.transpose(1, 2)
    for _ in range(hops - 1):
        tr = A2 @ tr
    y = base + torch.sigmoid(lg) * (A1 @ tr).transpose(1, 2).reshape(_OB, _ON, _OH * dk)
    ts = (q1, k1, v1, q2, k2, v2)
    grads = torch.autograd.grad((y * dy).sum(), (*ts, lg))
    yo, c = om.core_fwd(*(_bhnd(t) for t in ts), om.DEFAULT_GATES, 0.6, hops, -0.5)
    go = om.core_bwd(_bhnd(dy.view(_OB, _ON, _OH, dk)), c)
    _agree(yo, y.view(_OB, _ON, _OH, dk).transpose(1, 2), "y")
    for n, gr in zip(("dq1", "dk1", "dv1", "dq2", "dk2", "dv2"), grads):
        _agree(go[n], gr.transpose(1, 2), n)
    _agree(go["dlogit"], grads[-1], "dlogit")


@pytest.mark.parametrize("hops", [2, 3])
@pytest.mark.parametrize("dk", HEAD_SIZES)
def test_oracle_multihop_matches_autograd_at_any_head_size(dk, hops):
    """every gate on (and, or, not, chain), under a mask: the hand-derived backward against autograd of the stated formula"""
    from oracle import multihop as om
    (q1, k1, v1, q2, k2, v2), dy = _oracle_inputs(6, dk, 20 + hops)
    g_and, g_or, g_not, g_ch, beta = 0.8, 0.4, 0.3, 0.2, 0.6
    lg = torch.tensor(-0.5, dtype=torch.float64, requires_grad=True)
    blocked = ~torch.ones(_ON, _ON, dtype=torch.bool).tril()
    ninf = lambda s: s.masked_fill(blocked, float("-inf"))
    S1, S2 = _scores(q1, k1), _scores(q2, k2)
    A1, A2 = ninf(S1).softmax(-1), ninf(S2).softmax(-1)
    C, tr = A1, v2.transpose(1, 2)
    for _ in range(hops - 1):
        C, tr = C @ A2, A2 @ tr
    Smix = S1 + g_and * S2 + g_or * (torch.logaddexp(S1, S2) - S1) - g_not * beta * S2 + g_ch * torch.log(C + 1e-6)
    y = ninf(Smix).softmax(-1) @ v1.transpose(1, 2) + torch.sigmoid(lg) * (A1 @ tr)              # (B,H,N,dk)
    ts = (q1, k1, v1, q2, k2, v2)
    dyh = dy.view(_OB, _ON, _OH, dk).transpose(1, 2)
    grads = torch.autograd.grad((y * dyh).sum(), (*ts, lg))
    yo, c = om.core_fwd(*(_bhnd(t) for t in ts), dict(and_=g_and, or_=g_or, not_=g_not, chain=g_ch), beta, hops, -0.5,
                        blocked.numpy()[None, None])
    go = om.core_bwd(dyh.numpy(), c)
    _agree(yo, y, "y")
    for n, gr in zip(("dq1", "dk1", "dv1", "dq2", "dk2", "dv2"), grads):
        _agree(go[n], gr.transpose(1, 2), n)
    _agree(go["dlogit"], grads[-1], "dlogit")


@pytest.mark.parametrize("use_quartet", [True, False])
@pytest.mark.parametrize("dk", HEAD_SIZES)
def test_oracle_quartet_matches_autograd_at_any_head_size(dk, use_quartet):
    from oracle import quartet as oq
    (q, k, v, q2, k2), dy = _oracle_inputs(5, dk, 30 + use_quartet)
    eps = 1e-5
    mix = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    qs = torch.tensor(0.8, dtype=torch.float64, requires_grad=True)
    am = torch.randn(_OB, 1, _ON, _ON, generator=torch.Generator().manual_seed(dk), dtype=torch.float64)
    zn = lambda s: (s - s.mean(-1, keepdim=True)) / (s.std(-1, keepdim=True) + eps)                 # torch.std: unbiased
    z1 = zn(_scores(q, k))
    sc = (1 - torch.sigmoid(mix)) * z1 + torch.sigmoid(mix) * (z1 * zn(_scores(q2, k2))) * qs if use_quartet else z1
    sc = (sc + am).masked_fill(~torch.ones(_ON, _ON, dtype=torch.bool).tril(), float("-inf"))
    y = sc.softmax(-1) @ v.transpose(1, 2)
    dyh = dy.view(_OB, _ON, _OH, dk).transpose(1, 2)
    ins = (q, k, v, q2, k2, mix, qs) if use_quartet else (q, k, v)
    grads = torch.autograd.grad((y * dyh).sum(), ins)
    yo, c = oq.core_fwd(*(_bhnd(t) for t in (q, k, v, q2, k2)), 0.3, 0.8, eps, use_quartet, True, am.numpy())
    go = oq.core_bwd(dyh.numpy(), c)
    _agree(yo, y, "y")
    for n, gr in zip(("dq", "dk", "dv", "dq2", "dk2"), grads[:5]):
        _agree(go[n], gr.transpose(1, 2), n)
    if use_quartet:
        _agree(go["dmixture"], grads[5], "dmixture")
        _agree(go["dquartet_scale"], grads[6], "dquartet_scale")


@pytest.mark.parametrize("cues", [False, True])
@pytest.mark.parametrize("dk", HEAD_SIZES)
def test_oracle_crossview_matches_autograd_at_any_head_size(dk, cues):
    """cues: transpose cues and the per-key prior at fixed anchor rows; off: the mixed scores alone, which sdpa_ref64 states too"""
    from oracle import crossview as oc
    (q1, k1, v1, q2, k2), dy = _oracle_inputs(5, dk, 40 + cues)
    mix = torch.tensor([[1.0, 0.5], [-0.25, 0.75]], dtype=torch.float64, requires_grad=True)
    t1, t2, pw = (0.3, -0.2, 0.4) if cues else (0.0, 0.0, 0.0)
    k_star = np.array([[3, 0], [_ON - 1, 7]], dtype=np.int64)
    blocked = ~torch.ones(_ON, _ON, dtype=torch.bool).tril()
    ninf = lambda s: s.masked_fill(blocked, float("-inf"))
    S1, S2 = _scores(q1, k1), _scores(q2, k2)
    S = mix[0, 0] * S1 + mix[0, 1] * _scores(q1, k2) + mix[1, 0] * _scores(q2, k1) + mix[1, 1] * S2
    S = S + t1 * S1.transpose(-1, -2) + t2 * S2.transpose(-1, -2)
    A = ninf(S).softmax(-1)
    if cues:
        A1, A2 = ninf(S1).softmax(-1), ninf(S2).softmax(-1)
        anc = torch.stack([torch.stack([A2[b, h, int(k_star[b, h])] for h in range(_OH)]) for b in range(_OB)]).unsqueeze(2)
        u = A1 * anc
        A = (1 - pw) * A + pw * u / (u.sum(-1, keepdim=True) + 1e-9)
    y = A @ v1.transpose(1, 2)
    dyh = dy.view(_OB, _ON, _OH, dk).transpose(1, 2)
    grads = torch.autograd.grad((y * dyh).sum(), (q1, k1, v1, q2, k2, mix))
    yo, c = oc.core_fwd(*(_bhnd(t) for t in (q1, k1, v1, q2, k2)), mix.detach().numpy(), t1, t2, blocked.numpy()[None, None], pw,
                        "fixed", 0, k_star if cues else None)
    go = oc.core_bwd(dyh.numpy(), c)
    _agree(yo, y, "y")
    for n, gr in zip(("dq1", "dk1", "dv1", "dq2", "dk2"), grads[:5]):
        _agree(go[n], gr.transpose(1, 2), n)
    _agree(go["dmix"], grads[5], "dmix")
    if not cues:          # the folded statement: S = q1 (m11 k1 + m12 k2)^T + q2 (m21 k1 + m22 k2)^T, one SDPA over concatenated heads
        m = mix.detach()
        kk = torch.cat([m[0, 0] * k1 + m[0, 1] * k2, m[1, 0] * k1 + m[1, 1] * k2], -1) * 2 ** 0.5
        ys = sdpa_ref64(torch.cat([q1, q2], -1), kk, torch.cat([v1, v1], -1), causal=True)
        _agree(yo, ys.view(_OB, _ON, _OH, 2 * dk)[..., :dk].transpose(1, 2), "y through sdpa_ref64")
