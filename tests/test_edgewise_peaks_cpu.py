"""The peaked-logit reference of tests/edgewise_peaks.py stands on its own: the oracle's hand-derived backward agrees with float64
autograd where the logits are peaked, the planted rows obey their closed form, the generators are deterministic and hit the logit
level they name, and -- on the oracle alone -- the per-row bounds the GPU tests apply are not vacuous at any (shape, level) they use."""
import numpy as np
import pytest
import torch

import edgewise_peaks as ep
from edgewise_peaks import LEVELS, ROW_TENSORS, SHAPES

DENSE_SHAPE, DENSE_LEVELS = SHAPES[1], (0.5, 4, 8)
PLANT_SHAPES, PLANT_LEVEL = (SHAPES[1], SHAPES[2]), 2
EXTREME = (SHAPES[2], 32)


def gpu_cases():
    """every case tests/test_gpu_edgewise_peaks.py runs: (shape, level, plant, dense)"""
    out = [(s, l, False, False) for s in SHAPES for l in LEVELS]
    out += [(s, PLANT_LEVEL, True, False) for s in PLANT_SHAPES]
    out += [(DENSE_SHAPE, l, False, True) for l in DENSE_LEVELS]
    return out + [(EXTREME[0], EXTREME[1], True, False)]


def _id(c):
    (B, N, dk, V, r), level, plant, dense = c
    return f"B{B}-N{N}-dk{dk}-V{V}-r{r}-L{level}" + ("-plant" if plant else "") + ("-dense" if dense else "")


# ---------------------------------------------------------------------------------------------------------------------------------
# core_bwd against autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_core(case):
    """the core's algebra (oracle/edgewise_torch.py, plus the dense head) on the case's operands in float64; every operand a leaf"""
    d = lambda t: t.double().clone().requires_grad_(True)
    q, k, v, sqk, vs0, vsL, lg = map(d, (case.q, case.k, case.v, case.sqk, case.vs0, case.vsL, case.chain_logit))
    head = tuple(map(d, case.head))
    B, N, H, dk = case.q.shape
    V = case.V
    hv = lambda t: t.transpose(1, 2)
    S = torch.stack([(hv(q) * sqk[i][None, :, None, :]) @ hv(k).transpose(-1, -2) for i in range(V)])        # (V,B,H,N,N)
    A = torch.softmax(S, -1)
    Cf, Cb = A[0], A[V - 1]
    for i in range(1, V):
        Cf = Cf @ A[i]
    for i in range(V - 2, -1, -1):
        Cb = Cb @ A[i]
    Cr, Cl = torch.log(Cf + 1e-6), torch.log(Cb + 1e-6)
    if case.dense:
        W1, b1, W2, b2 = head
        feat = torch.stack([S[i] for i in range(V)] + [S[i].transpose(-1, -2) for i in range(V)] + [Cr, Cl], 2)      # (B,H,C,N,N)
        h = torch.nn.functional.gelu(torch.einsum("oc,bhcij->bhoij", W1, feat) + b1[None, None, :, None, None], approximate="tanh")
        G = torch.sigmoid(torch.einsum("go,bhoij->bhgij", W2, h) + b2[None, None, :, None, None])
    else:
        Wr, br, Wc, bc = head
        rS, cS = S.mean(-1).permute(1, 2, 0, 3), S.mean(-2).permute(1, 2, 0, 3)
        row = torch.cat([rS, cS, Cr.mean(-1)[:, :, None], Cl.mean(-1)[:, :, None]], 2)
        col = torch.cat([cS, rS, Cr.mean(-2)[:, :, None], Cl.mean(-2)[:, :, None]], 2)
        a = torch.einsum("oc,bhcn->bhon", Wr, row) + br[None, None, :, None]
        b = torch.einsum("oc,bhcn->bhon", Wc, col) + bc[None, None, :, None]
        G = torch.sigmoid(torch.einsum("bhgkn,bhgkm->bhgnm", a.view(B, H, 4, case.r, N), b.view(B, H, 4, case.r, N)))
    S0, O = S[0], S.sum(0) - S[0]
    Smix = S0 + G[:, :, 0] * O + G[:, :, 1] * (torch.logsumexp(S, 0) - S0) - G[:, :, 2] * (case.beta_not / max(1, V - 1) * O) + G[:, :, 3] * Cr
    y = torch.softmax(Smix, -1) @ (hv(v) * vs0[None, :, None])
    t = hv(v) * vsL[None, :, None]
    for i in range(V - 1, -1, -1):
        t = A[i] @ t
    y = hv(y + torch.sigmoid(lg) * t)
    (y * case.dy.double()).sum().backward()
    names = ("dq", "dk", "dv", "dsqk", "dvs0", "dvsL", "dchain_logit") + case.head_names
    grads = dict(zip(names, (t_.grad.numpy() for t_ in (q, k, v, sqk, vs0, vsL, lg) + head)))
    return y.detach().numpy(), grads


@pytest.mark.parametrize("dense", [False, True], ids=["lowrank", "dense"])
@pytest.mark.parametrize("plant", [False, True], ids=["plain", "planted"])
@pytest.mark.parametrize("level", [4, 8])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=lambda s: "N%d-dk%d-V%d-r%d" % s[1:])
def test_core_bwd_matches_float64_autograd_at_peaked_logits(shape, level, plant, dense):
    """nothing else checks the hand-derived backward above flat logits, and the GPU tests rest on it.  1e-9 relative per tensor."""
    case = ep.shape_case(shape, level, plant, dense)
    ref = ep.oracle_core(case)
    y, grads = _torch_core(case)
    for n_, got in dict(grads, y=y).items():
        err = float(np.abs(got - ref[n_].reshape(got.shape)).max()) / max(float(np.abs(got).max()), 1e-300)
        assert err <= 1e-9, f"{n_}: {err:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the planted rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in gpu_cases() if c[2]], ids=_id)
def test_planted_rows_obey_their_closed_form_and_do_not_move(c):
    """y[j] = v[j] vs0 + sigmoid(chain_logit) v[j] vsL to 1e-9 in the oracle, and not a bit of it depends on how q sqk_v is rounded:
    the GPU tests hold those rows to the plain tolerance with no noise allowance"""
    case = ep.shape_case(*c)
    rows = list(ep.planted_tokens(case.N))
    ref = ep.oracle_core(case)
    assert float(np.abs(ref["y"][:, rows] - ep.planted_identity(case)).max()) <= 1e-9
    assert float(ep.rounding_noise(case)["y"][:, rows].max()) <= 1e-9
    cache = ref["cache"]
    print(f"{_id(c)}: max |S_v| {np.abs(cache['S']).max():.0f}, max |Smix| {np.abs(cache['Smix']).max():.0f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the caps: conditions on the inputs, checked on the reference alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in gpu_cases() if c[1] <= max(LEVELS)], ids=_id)
def test_row_bounds_are_not_vacuous(c):
    """At most 10 % of the rows of y, dq, dk, dv may have a bound above ten times the tight one (4 noise > 10 tol max|ref|), and at
    levels 0.5 and 2 the median row bound is at most twice the tight one.  A seed that broke this would be replaced (case_seed), or
    the level dropped for that shape and said so here -- the caps are not widened.  One was: the dense head at level 8 (see
    edgewise_peaks.case_seed); no level is dropped."""
    case = ep.shape_case(*c)
    ref, noise = ep.oracle_core(case), ep.rounding_noise(case)
    line = []
    for n_ in ROW_TENSORS:
        tight = ep.tol_of(n_) * float(np.abs(ref[n_]).max())
        bound = ep.row_bounds(ref[n_], noise[n_], ep.tol_of(n_))
        loose = float((bound > 10 * tight).mean())
        med = float(np.median(bound)) / tight
        line.append(f"{n_}: loose {loose:.3f} median {med:.2f} worst row {noise[n_].max() / np.abs(ref[n_]).max():.3f} "
                    f"above tight {float((bound > tight).mean()):.3f}")
        assert loose <= 0.10, f"{n_}: {loose:.3f} of the rows have a bound above 10 x the tight one"
        if c[1] <= 2:
            assert med <= 2.0, f"{n_}: median row bound {med:.2f} x the tight one"
    print(_id(c) + " | " + " | ".join(line))


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------
def test_case_and_noise_are_deterministic():
    args = (65, 32, 3, 2, 4, 77)
    a, b = ep._peaked_case(*args, B=2, plant=True), ep._peaked_case(*args, B=2, plant=True)
    for n_ in ("q", "k", "v", "dy", "sqk", "vs0", "vsL", "chain_logit"):
        assert torch.equal(getattr(a, n_), getattr(b, n_)), n_
    assert all(torch.equal(x, y) for x, y in zip(a.head, b.head))
    for n_ in ("q", "k", "v", "dy"):
        assert torch.equal(getattr(a, n_), ep.bf16_exact(getattr(a, n_))), f"{n_} is not bf16-exact"
    na, nb = ep._rounding_noise(a, draws=3), ep._rounding_noise(b, draws=3)
    assert set(na) == set(nb)
    for n_ in na:
        assert np.array_equal(na[n_], nb[n_]), n_


@pytest.mark.parametrize("c", [c for c in gpu_cases() if not c[2]], ids=_id)
def test_realised_logit_std_is_the_level(c):
    """every view's logit standard deviation within 15 % of `level` (the planted cases add four outliers per head on purpose)"""
    lo, hi = ep.realised_logit_std(ep.shape_case(*c))
    assert 0.85 * c[1] <= lo and hi <= 1.15 * c[1], (lo, hi)


def test_gates_saturate_from_level_2_up():
    """the un-shrunk head scale is there to saturate the gate sigmoids: 40 - 80 % of the gate values within 0.01 of 0 or 1"""
    for level in (2, 4, 8):
        G = ep.oracle_core(ep.shape_case(SHAPES[2], level))["cache"]["G"]
        sat = float(((G < 0.01) | (G > 0.99)).mean())
        print(f"level {level}: {sat:.2f} of the gate values saturated")
        assert 0.4 <= sat
