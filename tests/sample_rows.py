"""Exact references and hand-built logit rows for the top-k / top-p thresholds of ops.sample_tokens (test_whisper_sample_filters_cpu,
test_gpu_whisper_sample_filters).  The op's noise is a pure function of (seed, row, pos, v), so its kept set {v : z_v >= thr} can be
observed draw by draw: the threshold is right if and only if the smallest kept tie group is drawn whenever the reference draws it
and the largest excluded tie group never is.  kept_exact states the documented rule on one row in float64 / integers, draw_reference
the Gumbel-max over a kept set, and the builders below give rows on which both deciding groups win a healthy share of the draws.
Entries of z = -inf have probability 0 whatever the threshold is, so the deciding groups are taken among the finite z only."""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

NEG = float("-inf")
SEED = 0x5EED5A3F1E
POS0 = 11                                                 # the draws of a case are at positions POS0 .. POS0 + P - 1
LN2 = math.log(2.0)


def _z(x, temperature):
    from mop_amd import ops
    return x.float() * torch.tensor(ops._f32(1.0 / temperature), device=x.device)


def gumbel(R, V, pos, seed, device, pos_off=None):
    """the op's noise G of every (row, v) at one position, fp32 (R, V); pos_off (R,): row r is at pos - pos_off[r]"""
    from mop_amd import ops
    s = seed & 0xFFFFFFFFFFFFFFFF
    r = torch.arange(R, device=device, dtype=torch.int64).unsqueeze(1)
    p = torch.full((1, 1), pos, dtype=torch.int64, device=device)
    if pos_off is not None:
        p = (p - pos_off.reshape(R, 1).to(device=device, dtype=torch.int64)) & ops._M32
    rh = ops._hash32(ops._hash32((s & ops._M32) ^ ops._mul32(r, 0x9E3779B1)) ^ (s >> 32) ^ ops._mul32(p, 0x85EBCA77))
    h = ops._hash32(rh ^ ops._mul32(torch.arange(V, device=device, dtype=torch.int64).unsqueeze(0), 0xC2B2AE3D))
    u = ((h >> 9).to(torch.float32) + 0.5) * 2.0 ** -23
    return -torch.log(-torch.log(u))


@functools.lru_cache(maxsize=8)
def _gumbel_cached(R, V, pos, seed, device):
    return gumbel(R, V, pos, seed, torch.device(device))


def _perturbed(x, pos, temperature, seed):
    """z + G of every (row, v), the torch path's own noise"""
    return _z(x, temperature) + gumbel(x.shape[0], x.shape[1], pos, seed, x.device)


# ---- the kept set of one row ----
@dataclass
class Kept:
    keep: torch.Tensor                                    # (V,) bool, CPU
    thr: float                                            # the threshold: kept <=> z >= thr
    count: int
    margin: Optional[float]                               # top-p only: distance of P from the cumulative masses beside it, / Q
    low: torch.Tensor                                     # (V,) bool: the smallest kept tie group of finite z (may be empty)
    excl: torch.Tensor                                    # (V,) bool: the largest excluded tie group of finite z (may be empty)


def _groups(x, temperature):
    """the row's tie groups -> (z fp32 numpy (V,), distinct z descending, group index of every entry)"""
    z = _z(x.detach().cpu().reshape(-1), temperature).numpy() + np.float32(0.0)        # -0 -> +0
    assert not np.isnan(z).any() and not np.isposinf(z).any()
    u, inv = np.unique(-z.astype(np.float64), return_inverse=True)                      # ascending in -z: descending in z
    return z, -u, inv.reshape(-1)


def _entry_mass(z):
    """the fixed-point mass int(exp(z - max z) * 2^40) of every entry, int64: the difference taken in fp32 as the op takes it, the
    exponential in float64"""
    d = (z - z.max()).astype(np.float64)                  # fp32 subtraction, widened
    with np.errstate(invalid="ignore"):
        q = np.floor(np.exp(d) * 2.0 ** 40)
    return np.where(np.isfinite(q), q, 0.0).astype(np.int64)


def _masses(z, uz, inv):
    """the mass of every tie group, summed in integers"""
    m = np.zeros(len(uz), dtype=np.int64)
    np.add.at(m, inv, _entry_mass(z))
    return [int(v) for v in m]


def _threshold_group(x, temperature, top_k, top_p):
    """-> (z, uz, inv, g, margin): the kept set is the tie groups 0 .. g"""
    from mop_amd import ops
    z, uz, inv = _groups(x, temperature)
    V, G = len(z), len(uz)
    cnt = np.cumsum(np.bincount(inv, minlength=G))
    g = G - 1
    if 0 < top_k < V:
        g = int(np.argmax(cnt >= top_k))                  # tie-inclusive: the group that holds the k-th largest z
    margin = None
    tp = ops._f32(float(top_p))
    if tp < 1:
        margin = math.inf
        if uz[0] != NEG:                                  # a row of -inf only keeps everything
            m = _masses(z, uz, inv)
            Q = sum(m[:g + 1])
            P = math.ceil(tp * float(Q))
            cum, gp = 0, None
            for j in range(g + 1):
                below = cum
                cum += m[j]
                if cum >= P:
                    gp = j
                    break
            assert gp is not None
            # the side above P counts only if mass is left beyond it: cum == Q >= P holds however the terms are rounded
            margin = min(P - below, cum - P if cum < Q else math.inf) / Q
            g = gp
    return z, uz, inv, g, margin


def kept_exact(x, temperature, top_k, top_p, shift=0):
    """the kept set of one logit row (V,) by the rule in the sample_tokens docstring: z in fp32 as the op forms it, tie-inclusive
    top-k, top-p on fixed-point masses summed as integers against ceil(top_p * Q) in float64.  The margin is min |cum - P| / Q over
    the cumulative masses on either side of the threshold (the side above P only where kept mass lies beyond it: the last group's
    cumulative mass is Q itself and reaches P under any rounding of the terms).
    shift: +1 drops the smallest kept finite tie group, -1 adds the largest excluded one (a threshold one tie group off); None is
    returned where the row has no such group."""
    z, uz, inv, g, margin = _threshold_group(x, temperature, top_k, top_p)
    fin = int(np.isfinite(uz).sum())                      # the groups 0 .. fin - 1 are finite
    lo = min(g, fin - 1)                                  # the smallest kept finite group (-1: none)
    ex = g + 1 if g + 1 < fin else -1                     # the largest excluded finite group
    if shift == 1:
        if lo < 1:
            return None
        g = lo - 1
        lo, ex = g, g + 1
    elif shift == -1:
        if ex < 0:
            return None
        g = ex
        lo, ex = g, (g + 1 if g + 1 < fin else -1)
    keep = torch.from_numpy(inv <= g)
    return Kept(keep, float(uz[g]), int(keep.sum()), margin, torch.from_numpy(inv == lo), torch.from_numpy(inv == ex))


def p_mid(x, temperature, top_k, g):
    """the top_p that puts ceil(top_p * Q) halfway between the cumulative masses of the tie groups 0 .. g - 1 and 0 .. g of the row
    under this top_k: the nucleus is then the tie groups 0 .. g"""
    z, uz, inv, gk, _ = _threshold_group(x, temperature, top_k, 1.0)
    m = _masses(z, uz, inv)
    assert g <= gk and m[g] > 0
    return float(np.float32((sum(m[:g]) + 0.5 * m[g]) / sum(m[:gk + 1])))


def radix_walk(x, temperature, top_k, top_p):
    """a model of the documented threshold search on the order-preserving uint32 keys of z (<= 256 power-of-two bins per level, the
    window shrinking to the bin that reaches the target; a top-k level whose bin ends exactly at k returns at once; top-p starts at
    top-k's threshold) -> [(filter, shift, exact)] per level.  It certifies that a row exercises the levels it was built for; the
    kept set is never taken from it."""
    from mop_amd import ops
    z, uz, inv = _groups(x, temperature)
    u = z.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    mass = [int(m) for m in _entry_mass(z)] if uz[0] != NEG else None
    lo0, hi0, levels = int(key.min()), int(key.max()), []

    def select(name, w, lo, hi, target):
        above = 0
        while True:
            span = hi - lo
            sh = max(span.bit_length() - 8, 0)
            hist = [0] * 256
            for k, wk in zip(key, w):
                if lo <= k <= hi:
                    hist[(int(k) - lo) >> sh] += int(wk)
            cum = above
            for b in range(255, -1, -1):
                if cum < target <= cum + hist[b]:
                    break
                cum += hist[b]
            exact = name == "top_k" and cum + hist[b] == target
            levels.append((name, sh, exact))
            above = cum
            lo, hi = lo + (b << sh), min(hi, lo + (b << sh) + (1 << sh) - 1)
            if sh == 0 or exact:
                return lo

    thr = lo0
    if 0 < top_k < len(z):
        thr = select("top_k", [1] * len(z), lo0, hi0, int(top_k))
    tp = ops._f32(float(top_p))
    if tp < 1 and mass is not None:
        Q = sum(int(m) for k, m in zip(key, mass) if k >= thr)
        select("top_p", mass, thr, hi0, math.ceil(tp * float(Q)))
    return levels


# ---- the draws over a kept set ----
@dataclass
class Draws:
    winner: torch.Tensor                                  # (R,) int64: argmax over kept of z + G, ties to the smaller index
    second: torch.Tensor                                  # (R,) int64: the runner-up
    near: torch.Tensor                                    # (R,) bool: top-2 gap <= 1e-5 * max(1, |top|)
    excl_wins: int                                        # draws the largest excluded tie group would win if it were kept


def draw_reference(x, kept, pos, temperature, seed, R, pos_off=None):
    """the fp32 perturbed scores z + G of R draws of one row x (V,) at one position, and their Gumbel-max over kept (a Kept)"""
    x = x.reshape(-1)
    V, dev = x.shape[0], x.device
    if pos_off is None:
        G = _gumbel_cached(R, V, pos, seed, str(dev))
    else:
        G = gumbel(R, V, pos, seed, dev, pos_off)
    sc = _z(x, temperature).unsqueeze(0) + G
    ninf = torch.tensor(NEG, device=dev)
    ks = torch.where(kept.keep.to(dev).unsqueeze(0), sc, ninf)
    winner = ks.argmax(-1)                                # the first maximum: ties to the smaller index
    top = ks.gather(1, winner.unsqueeze(1)).squeeze(1)
    rest = ks.scatter(1, winner.unsqueeze(1), NEG)
    second = rest.argmax(-1)
    sec = rest.gather(1, second.unsqueeze(1)).squeeze(1)
    near = (top - sec).abs() <= 1e-5 * top.abs().clamp_min(1.0)
    excl_wins = 0
    if bool(kept.excl.any()):
        es = torch.where(kept.excl.to(dev).unsqueeze(0), sc, ninf).max(-1).values
        excl_wins = int((es > top).sum())
    return Draws(winner, second, near, excl_wins)


# ---- cases ----
@dataclass(frozen=True)
class Case:
    name: str
    x: torch.Tensor = field(compare=False)                # (V,) CPU, fp32 or bf16
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    R: int = 4096                                         # output rows sharing the one logit row
    P: int = 4                                            # positions
    offset: int = 0                                       # elements between the buffer's start and the row view's

    def logits(self, device):
        """the (1, V) logit row on device, as a view `offset` elements into its buffer"""
        V = self.x.shape[0]
        buf = torch.zeros(V + 3, dtype=self.x.dtype, device=device)
        buf[self.offset:self.offset + V] = self.x.to(device)
        return buf[self.offset:self.offset + V].unsqueeze(0)

    def kept(self, shift=0):
        return kept_exact(self.x, self.temperature, self.top_k, self.top_p, shift)


@dataclass
class Reference:
    kept: Kept
    draws: list                                           # one Draws per position
    low_wins: int                                         # draws the smallest kept finite tie group wins
    excl_wins: int                                        # draws the largest excluded finite tie group would win
    near: int
    n: int


def reference(case, device="cpu", shift=0, pos_off=None):
    kept = case.kept(shift)
    x = case.x.to(device)
    draws = [draw_reference(x, kept, POS0 + p, case.temperature, SEED, case.R, pos_off) for p in range(case.P)]
    low = kept.low.to(device)
    return Reference(kept, draws, sum(int(low[d.winner].sum()) for d in draws), sum(d.excl_wins for d in draws),
                     sum(int(d.near.sum()) for d in draws), case.R * case.P)


def pos_offsets(R, device):
    """a non-constant pos_off for the ragged op"""
    return (torch.arange(R, dtype=torch.int32, device=device) * 7) % 5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _scatter(V, vals, rest, gen, idx=None):
    """a row of V entries: vals at idx (default: random distinct places), rest (V - len(vals) values) elsewhere in random order"""
    vals = torch.as_tensor(vals, dtype=torch.float32)
    rest = torch.as_tensor(rest, dtype=torch.float32)
    assert len(vals) + len(rest) == V
    perm = torch.randperm(V, generator=gen)
    if idx is not None:
        idx = torch.as_tensor(idx)
        free = torch.ones(V, dtype=torch.bool)
        free[idx] = False
        perm = torch.cat([idx, torch.arange(V)[free][torch.randperm(V - len(idx), generator=gen)]])
    x = torch.empty(V)
    x[perm[:len(vals)]] = vals
    x[perm[len(vals):]] = rest[torch.randperm(len(rest), generator=gen)]
    return x


def _cluster(n, step, top=3.75, ties=(), gap_after=None, gap=0.0):
    """n values top - j * step; ties: (first, last) runs of j that take the value at `first`; the values after index gap_after are
    lowered by gap"""
    j = torch.arange(n, dtype=torch.float64)
    for a, b in ties:
        j[a:b + 1] = a
    v = top - j * step
    if gap_after is not None:
        v[gap_after + 1:] -= gap
    return v.float()


def _wide_rest(n, gen):
    """n values below the cluster that span the whole finite key range: most in [-20, -10], some as low as -1e30, some -inf, some
    around zero of either sign, and both zeros"""
    u = torch.rand(n, generator=gen)
    r = -10.0 - 10.0 * u
    r[:20] = -1e30 * (0.01 + u[:20])
    r[20:50] = NEG
    r[50:60] = 1e-3 * (u[50:60] - 0.5)
    r[60], r[61] = 0.0, -0.0
    return r


def _filters(name, x, T, k, g_p, g_kp, dtype, **kw):
    """a row under top_k alone, top_p alone (the nucleus ends at tie group g_p) and both (at g_kp inside the top-k set)"""
    x = x.to(dtype)
    return [Case(f"{name}-k", x, T, k, 1.0, **kw), Case(f"{name}-p", x, T, 0, p_mid(x, T, 0, g_p), **kw),
            Case(f"{name}-kp", x, T, k, p_mid(x, T, k, g_kp), **kw)]


def _step(dtype):
    return 2.0 ** -20 if dtype == torch.float32 else 2.0 ** -6        # cluster spacing: distinct in the row's storage type


def radix_depth(dtype=torch.float32):
    """a cluster of 40 candidates spaced one step apart on top of a row whose key window takes (a) one level, (b) about 2^16 keys
    (levels of 512 keys per bin, then one), (c) all four (the whole finite range and -inf, keys on both sides of the sign)"""
    tag, st, out = ("f32" if dtype == torch.float32 else "bf16"), _step(dtype), []
    if dtype == torch.float32:
        out += _filters(f"depth-one-{tag}", _scatter(64, _cluster(64, st), [], _gen(1)), 1.0, 29, 31, 20, dtype)
        g = _gen(2)
        rest = 3.75 - 2.0 ** -7 - 2.0 ** -6 * torch.rand(160, generator=g)
        out += _filters(f"depth-mid-{tag}", _scatter(200, _cluster(40, st), rest, g), 1.0, 29, 31, 20, dtype)
    else:                                                 # bf16: 200 values on a 128-point grid, so most are tied
        g = _gen(3)
        rest = 3.75 - 2.0 ** -6 * torch.randint(40, 128, (160,), generator=g)
        out += _filters(f"depth-grid-{tag}", _scatter(200, _cluster(40, st), rest, g), 1.0, 29, 31, 20, dtype)
    g = _gen(4)
    x = _scatter(1025, _cluster(40, st), _wide_rest(985, g), g)
    out += _filters(f"depth-four-{tag}", x, 1.0, 29, 31, 20, dtype)
    out += _filters(f"depth-four-T0.7-{tag}", x, 0.7, 29, 31, 20, dtype)[2:]
    return out


def threshold_ties(dtype=torch.float32):
    tag, st, out = ("f32" if dtype == torch.float32 else "bf16"), _step(dtype), []
    g = _gen(5)
    x = _scatter(1025, _cluster(40, st, ties=[(28, 30)]), _wide_rest(985, g), g).to(dtype)
    out.append(Case(f"tie-straddles-k-{tag}", x, 1.0, 29, 1.0))                   # kept: 31
    out.append(Case(f"tie-straddles-p-{tag}", x, 1.0, 0, p_mid(x, 1.0, 0, 28)))   # the nucleus ends inside the 3-way tie
    out.append(Case(f"tie-straddles-kp-{tag}", x, 1.0, 35, p_mid(x, 1.0, 35, 28)))
    g = _gen(6)
    gap = 2.0 ** -10 if dtype == torch.float32 else 0.25
    x = _scatter(1025, _cluster(40, st, ties=[(27, 28)], gap_after=28, gap=gap), _wide_rest(985, g), g).to(dtype)
    out.append(Case(f"tie-ends-at-k-{tag}", x, 1.0, 29, 1.0))                     # kept: exactly 29, the early return
    x = torch.full((257,), 0.5).to(dtype)
    out.append(Case(f"all-equal-k-{tag}", x, 0.7, 5, 1.0))
    out.append(Case(f"all-equal-p-{tag}", x, 0.7, 0, 0.5))
    g = _gen(7)
    x = _scatter(257, [0.0] * 10, [-3.0] * 247, g).to(dtype)
    out += [Case(f"two-valued-k5-{tag}", x, 1.0, 5, 1.0), Case(f"two-valued-k11-{tag}", x, 1.0, 11, 1.0),
            Case(f"two-valued-p0.1-{tag}", x, 1.0, 0, 0.1), Case(f"two-valued-p0.5-{tag}", x, 1.0, 0, 0.5)]
    g = _gen(8)
    pos = [0.0625 * (j + 1) for j in range(16)]
    x = _scatter(64, pos + [0.0, -0.0] * 3, [-0.125 * (j + 1) for j in range(42)], g).to(dtype)
    for T in (1.0, 0.7):
        out.append(Case(f"zero-threshold-k-T{T}-{tag}", x, T, 19, 1.0))           # kept: 16 positives and all six zeros
        out.append(Case(f"zero-threshold-p-T{T}-{tag}", x, T, 0, p_mid(x, T, 0, 16)))
    g = _gen(9)
    x = _scatter(257, [2.0] * 3, 1.0 - 4.0 * torch.rand(254, generator=g), g).to(dtype)
    out.append(Case(f"tied-max-p-{tag}", x, 1.0, 0, 0.05))                        # kept: the tied maximum only
    return out


def masked_rows():
    """rows as the logit-rule kernels leave them: nearly everything -inf"""
    x3 = torch.full((1025,), NEG)
    x3[5], x3[600], x3[1024] = 1.0, 0.5, -0.5
    x1 = torch.full((1025,), NEG)
    x1[333] = -2.5
    x0 = torch.full((1025,), NEG)
    return [Case("masked-3-k2", x3, 1.0, 2, 1.0), Case("masked-3-k5", x3, 1.0, 5, 1.0), Case("masked-3-p0.5", x3, 1.0, 0, 0.5),
            Case("masked-3-p0.7", x3, 1.0, 0, 0.7), Case("masked-3-k5-p0.7", x3, 0.8, 5, 0.7),
            Case("masked-1-k1", x1, 1.0, 1, 1.0), Case("masked-1-k3", x1, 1.0, 3, 1.0), Case("masked-1-p0.5", x1, 1.0, 0, 0.5),
            Case("masked-all", x0, 1.0, 0, 1.0), Case("masked-all-k3-p0.5", x0, 1.0, 3, 0.5)]


def mass_underflow():
    """a peaked row: one maximum, three entries 5 below it, and a tail 40 to 45 below, whose fixed-point mass is 0 at temperature 1"""
    g = _gen(10)
    x = _scatter(300, [3.0, -2.0, -2.0, -2.0], 3.0 - 40.0 - 5.0 * torch.rand(296, generator=g), g)
    return [Case(f"peaked-T{T}-p{p}", x, T, 0, p) for T in (1.0, 0.05, 50.0) for p in (0.9, 0.999999)]


def geometric(dtype=torch.float32):
    """z_j = -j ln 2: the cumulative masses are 1 - 2^-(j+1) of the whole"""
    tag = "f32" if dtype == torch.float32 else "bf16"
    x = (-LN2 * torch.arange(64, dtype=torch.float64)).float()
    x = x[torch.randperm(64, generator=_gen(11))].to(dtype)
    out = [Case(f"geometric-p{p}-{tag}", x, 1.0, 0, p) for p in (0.45, 0.55, 0.72, 0.78, 0.85, 0.9, 0.95, 0.98)]
    return out + [Case(f"geometric-k6-p{p}-{tag}", x, 1.0, 6, p) for p in (0.45, 0.55, 0.85, 0.93, 0.97, 0.995)]


def stride_edges():
    """the deciding groups at the ends of the 1024-thread stride: six near-equal candidates on a low background, the fifth (the
    smallest kept under top_k = 5) and the sixth (the largest excluded) at the row's last two indices; at V = 16385 also as 16-way
    tie groups at the indices 1024 i - 1 (kept) and 1024 i (excluded)"""
    out = []
    out += [Case("edge-V2-k1", torch.tensor([-1.0, 0.0]), 1.0, 1, 1.0), Case("edge-V2-p0.6", torch.tensor([-1.0, 0.0]), 1.0, 0, 0.6),
            Case("edge-V3-k2", torch.tensor([0.5, -0.3, 0.0]), 1.0, 2, 1.0), Case("edge-V3-p0.7", torch.tensor([0.5, -0.3, 0.0]), 1.0, 0, 0.7)]
    for V in (1023, 1024, 1025, 16385):
        g = _gen(100 + V % 97)
        R = 4096 if V < 16385 else 256
        idx = [3, V // 2, V // 3, 700, V - 1, V - 2]
        vals = [2.0, 1.9, 1.8, 1.7, 1.6, 1.5]              # the fifth (1.6) at V - 1, the sixth (1.5) at V - 2
        x = _scatter(V, vals, 2.0 - 25.0 - torch.rand(V - 6, generator=g), g, idx)
        out.append(Case(f"edge-V{V}-k5", x, 1.0, 5, 1.0, R=R))
        out.append(Case(f"edge-V{V}-p", x, 1.0, 0, p_mid(x, 1.0, 0, 4), R=R))
    V, g = 16385, _gen(12)
    hi = [1024 * i - 1 for i in range(1, 17)]
    lo = [1024 * i for i in range(1, 17)]
    x = _scatter(V, [2.0, 1.9, 1.8, 1.7] + [0.5] * 16 + [0.4] * 16, 2.0 - 25.0 - torch.rand(V - 36, generator=g), g, [3, 8000, 5001, 700] + hi + lo)
    out.append(Case("edge-V16385-stride-k12", x, 1.0, 12, 1.0, R=256))            # kept: 4 + the 16-way tie
    out.append(Case("edge-V16385-stride-p", x, 1.0, 0, p_mid(x, 1.0, 0, 4), R=256))
    return out


def bf16_storage():
    """the radix-depth, tie and geometric rows stored in bf16, and one case per dtype read through a view off a 16-byte boundary"""
    out = radix_depth(torch.bfloat16) + threshold_ties(torch.bfloat16) + geometric(torch.bfloat16)
    for c in (radix_depth()[-1], radix_depth(torch.bfloat16)[-1]):                 # the four-level row under top_k and top_p
        out.append(Case(c.name + "-offset", c.x, c.temperature, c.top_k, c.top_p, offset=1))
    return out


FAMILIES = {"radix_depth": radix_depth, "threshold_ties": threshold_ties, "masked_rows": masked_rows, "mass_underflow": mass_underflow,
            "geometric": geometric, "stride_edges": stride_edges, "bf16_storage": bf16_storage}


@functools.lru_cache(maxsize=None)
def cases(family):
    out = FAMILIES[family]()
    assert len({c.name for c in out}) == len(out)
    return out


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


# cases in which a deciding group cannot win 16 draws, whatever the row: held to per-draw equality only
UNWITNESSED = {
    "peaked-T1.0-p0.999999": "the largest excluded entry is 40 below the maximum (mass 0 is what excludes it): it wins no draw",
    "peaked-T0.05-p0.9": "at temperature 0.05 everything but the maximum is 100 or more below it: no other entry wins a draw",
    "peaked-T0.05-p0.999999": "at temperature 0.05 everything but the maximum is 100 or more below it: no other entry wins a draw",
    "masked-all": "a row of -inf only has no finite entry: every score is -inf and the draw is index 0",
    "masked-all-k3-p0.5": "a row of -inf only has no finite entry: every score is -inf and the draw is index 0",
}


RAGGED = {"radix_depth": "depth-four-f32-kp", "threshold_ties": "tie-straddles-kp-f32", "masked_rows": "masked-3-k5-p0.7",
          "mass_underflow": "peaked-T50.0-p0.9", "geometric": "geometric-k6-p0.93-f32", "stride_edges": "edge-V16385-stride-p",
          "bf16_storage": "depth-four-T0.7-bf16-kp-offset"}


def ragged_cases():
    """one case of every family for the ragged op"""
    return [next(c for c in cases(f) if c.name == RAGGED[f]) for f in FAMILIES]


def compare_draws(tokens, ref):
    """tokens: one (R,) tensor per position -> (draws outside the near ties whose token is not the reference winner, near-tie draws
    whose token is neither of the reference's top two)"""
    wrong = off = 0
    for tok, d in zip(tokens, ref.draws):
        tok = tok.long()
        wrong += int(((tok != d.winner) & ~d.near).sum())
        off += int(((tok != d.winner) & (tok != d.second) & d.near).sum())
    return wrong, off


def describe(case, ref, tokens):
    """what a failing case prints: the expected threshold and kept count against the smallest z drawn and the tokens seen"""
    z = _z(case.x, case.temperature)
    seen = torch.unique(torch.cat([t.long().cpu() for t in tokens]))
    return (f"{case.name}: T={case.temperature} top_k={case.top_k} top_p={case.top_p}: expected thr z={ref.kept.thr!r} "
            f"kept={ref.kept.count}; smallest z drawn={float(z[seen].min())!r}, {len(seen)} distinct tokens drawn, "
            f"{int((~ref.kept.keep[seen]).sum())} of them outside the kept set")
