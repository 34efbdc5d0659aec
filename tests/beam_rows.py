"""A float64 reference, a model of the row partition and hand-built cases for ops.beam_step (test_beam_rows_cpu,
test_gpu_beam_rows).

partition() restates how launch A of mopk_beam_step walks one logit row: the scalar head before the row's first 16-byte boundary,
the 16-byte vectors dealt to `nslice` slices of 128 threads, the scalar tail.  It is used to place logits (a candidate on the head,
on a slice edge, 2K candidates in one thread's registers) and to bound the row's longest addition chain; the CPU test ties its slice
count to the library's own workspace query.

reference() is one step by the definition in the ops.beam_step docstring: each beam contributes its 2K largest stored logits (ties
to the smaller v), lse in float64, score = fp32(sc + fp32(x - lse)) (-inf where x or sc is -inf), rank by score with ties to the
smaller k * V + v, then the walk and the in-place updates.

The rounding bound.  The kernel's lse of a row is fp32(M + logf(l)), l the sum of expf(x - m) built by online (max, sum) pairs: per
thread over its elements, through 7 LDS tree levels, then over the slices.  A term of l passes at most
    n_link = chain + 7 + (nslice - 1) + 1
links (chain: the most elements one thread adds, scalars included, from partition(); + 1 for the term's own expf), and a link costs
at most one expf, one multiply and one add: (4 + 1 + 1) u relative, u = 2^-24, with expf and logf taken as 2 ulp = 4 u relative (the
HIP documentation at hand states no ulp figures for them, so 2 ulp is an assumption).  The subtractions x - m round their result,
which moves the exponent of term i by at most u (M - x_i) in total (the running maxima only rise, so the pieces add up to M - x_i):
weighted by the term's share p_i of l this is u * t, t = sum_i p_i (M - x_i).  logf adds 4 u |log l| and the last addition u |lse|:
    beta_lse = 1.01 * u * (6 n_link + t + 4 (lse - M) + |lse|)
The score then takes two roundings on each side of the comparison (the reference is rounded to fp32 as well):
    beta = 1.01 * (beta_lse + 2 u (|x - lse| + |s|))
A row with one finite logit c has l = 1 and lse = c + logf(1) = c exactly: its beta_lse is 0.
decided() moves every beam's lse by +-beta_lse and requires that nothing the walk observes can change."""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

NEG = float("-inf")
U = 2.0 ** -24
A_THREADS, MIN_VEC, TARGET_WG = 128, 128, 512             # launch-A workgroup, vectors per slice at least, workgroups aimed for
POISON = -77
FIELDS = ("scores", "next_ids", "parents", "hist", "rows", "fin_tokens", "fin_scores", "fin_count", "done")
VEC, HEAD, TAIL = 0, 1, 2


def epv(dtype):
    return 4 if dtype == torch.float32 else 8


def tag(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


# ---- the model of launch A's row partition ----
def nslice(B, K, V, dtype):
    want = -(-TARGET_WG // (B * K))
    return max(1, min(want, V // epv(dtype) // MIN_VEC))


@dataclass
class Partition:
    head: int
    nvec: int
    tail0: int
    nslice: int
    slices: list                                          # [u0, u1) of every slice, in vectors
    slice: np.ndarray                                     # (V,) the slice that reads element v
    thread: np.ndarray                                    # (V,) its thread
    kind: np.ndarray                                      # (V,) VEC / HEAD / TAIL
    chain: int                                            # the most elements one thread of one slice adds up

    def specials(self, E):
        """the scalar head and tail elements and the first and last element of every slice -> {v: name}"""
        out = {v: "head" for v in range(self.head)}
        out.update({v: "tail" for v in range(self.tail0, len(self.kind))})
        for s, (u0, u1) in enumerate(self.slices):
            if u1 > u0:
                out[self.head + u0 * E] = f"first{s}"
                out[self.head + u1 * E - 1] = f"last{s}"
        return out


@functools.lru_cache(maxsize=None)
def partition(V, dtype, base_mod16, B, K):
    """who reads which element of a row that starts base_mod16 bytes behind a 16-byte boundary: head / nvec / tail0 restate
    RowSpan of csrc/row_helpers.h (the one split every row kernel uses), the rest is bs_rows_kernel's deal of the vectors to slices
    and threads"""
    es, E = 16 // epv(dtype), epv(dtype)
    head = min(((16 - base_mod16) & 15) // es, V)
    nvec = (V - head) // E
    tail0 = head + nvec * E
    ns = nslice(B, K, V, dtype)
    slices = [(nvec * s // ns, nvec * (s + 1) // ns) for s in range(ns)]
    v = np.arange(V)
    u = (v - head) // E
    sl = np.searchsorted(np.array([u1 for _, u1 in slices]), u, side="right").clip(0, ns - 1)
    th = (u - np.array([u0 for u0, _ in slices])[sl]) % A_THREADS
    kind = np.full(V, VEC)
    kind[:head], kind[tail0:] = HEAD, TAIL
    sl[:head], th[:head] = 0, v[:head] % A_THREADS
    nh_last = head if ns == 1 else 0                      # the last slice's scalar loop starts with its head elements, if it has any
    sl[tail0:], th[tail0:] = ns - 1, (nh_last + v[tail0:] - tail0) % A_THREADS
    chain = int(np.bincount(sl * A_THREADS + th, minlength=ns * A_THREADS).max())
    return Partition(head, nvec, tail0, ns, slices, sl, th, kind, chain)


# ---- cases ----
@dataclass
class Case:
    name: str
    family: str
    B: int
    K: int
    x: torch.Tensor = field(repr=False)                   # (B * K, V) or (B, V) CPU logits in their storage type
    scores: torch.Tensor = field(repr=False)              # (B * K,) fp32
    eos: Optional[int] = None
    lp: float = 0.9
    T: int = 12
    Tp: int = 3
    pos: int = 5
    fin_count: Optional[list] = None
    done: Optional[list] = None
    offset: int = 0                                       # elements between a 16-byte boundary and row 0
    sk: Optional[int] = None                              # elements between rows (>= V; the gap holds NaN)
    ld_pad: int = 0                                       # poisoned columns on either side of hist / rows
    calls: int = 1                                        # the second call is at pos + 1 on the same logits
    plans: Optional[list] = None                          # per item: the (parent, token) the walk reads, in rank order
    claims: list = field(default_factory=list)            # ownership the case was built for, checked through partition()

    def __post_init__(self):
        self.V, self.dtype = self.x.shape[1], self.x.dtype
        self.shared = self.x.shape[0] != self.B * self.K
        self.sk = self.sk or self.V
        self._x64, self._rows = None, {}

    def row(self, b, k):
        return b if self.shared else b * self.K + k

    def row_mod16(self, r, contiguous=False):
        off, sk = (0, self.V) if contiguous else (self.offset, self.sk)
        return (off + r * sk) * (16 // epv(self.dtype)) % 16

    def part(self, r, contiguous=False):
        return partition(self.V, self.dtype, self.row_mod16(r, contiguous), self.B, self.K)

    def x64(self):
        if self._x64 is None:
            self._x64 = self.x.float().numpy().astype(np.float64)
        return self._x64

    def state0(self):
        """the state before the call, CPU tensors: hist / rows / fin_tokens hold a value that names their row and column"""
        B, K, T = self.B, self.K, self.T
        r = torch.arange(B * K, dtype=torch.int32).unsqueeze(1) * 1000 + torch.arange(T, dtype=torch.int32)
        fc = torch.tensor(self.fin_count or [0] * B, dtype=torch.int32)
        fs = torch.full((B, K), NEG)
        for b in range(B):
            fs[b, :int(fc[b])] = -0.25 * torch.arange(1, int(fc[b]) + 1)
        return dict(scores=self.scores.clone().float(), next_ids=torch.full((B * K,), -3, dtype=torch.int32),
                    parents=torch.full((B * K,), -3, dtype=torch.int32), hist=r.clone(), rows=r + 1000000,
                    fin_tokens=(r + 2000000).view(B, K, T).clone(), fin_scores=fs, fin_count=fc,
                    done=torch.tensor(self.done or [0] * B, dtype=torch.int32))

    def logits(self, device, contiguous=False):
        """the logit rows on device, as a strided view into a buffer of NaN"""
        R, V = self.x.shape
        off, sk = (0, V) if contiguous else (self.offset, self.sk)
        buf = torch.full((off + R * sk + 8,), float("nan"), dtype=self.dtype, device=device)
        view = buf.as_strided((R, V), (sk, 1), off)
        view.copy_(self.x)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off * view.element_size() % 16
        return view

    def state(self, device, contiguous=False):
        """(BeamState, {name: the wider tensor that hist / rows are column views of})"""
        from mop_amd import ops
        st = ops.BeamState(torch.zeros(self.B, self.Tp, dtype=torch.long, device=device), self.K, self.T, self.eos, self.lp)
        wide, pad = {}, 0 if contiguous else self.ld_pad
        for name, t in self.state0().items():
            t = t.to(device)
            if name in ("hist", "rows") and pad:
                wide[name] = torch.full((t.shape[0], self.T + 2 * pad), POISON, dtype=torch.int32, device=device)
                wide[name][:, pad:pad + self.T] = t
                t = wide[name][:, pad:pad + self.T]
            setattr(st, name, t.view(-1, 1) if name == "next_ids" else t)
        return st, wide


def state_dict(st):
    return {n: getattr(st, n).detach().cpu().clone() for n in FIELDS}


# ---- the float64 reference ----
@dataclass
class RowInfo:
    top: np.ndarray                                       # the row's min(2K, V) largest logits' indices, ties to the smaller v
    lse: float
    M: float
    beta_lse: float
    exact: Optional[tuple]                                # (c, n): every finite logit equals c and their count n is a power of two


def row_info(case, r, contiguous=False):
    key = (r, contiguous)
    if key not in case._rows:
        x = case.x64()[r]
        top = np.argsort(-x, kind="stable")[:min(2 * case.K, case.V)]
        M = float(x.max())
        if M == NEG:
            case._rows[key] = RowInfo(top, NEG, NEG, 0.0, None)
        else:
            e = np.exp(x - M)
            l = float(e.sum())
            lse = M + math.log(l)
            d = np.where(e > 0, M - x, 0.0)
            t = float((e * d).sum() / l)
            p = case.part(r, contiguous)
            n_link = p.chain + 7 + (p.nslice - 1) + 1
            beta = 1.01 * U * (6 * n_link + t + 4 * (lse - M) + abs(lse))
            fin = x[np.isfinite(x)]
            n = len(fin)
            exact = (float(fin[0]), n) if bool((fin == fin[0]).all()) and n & (n - 1) == 0 and n <= 2 ** 24 else None
            if n == 1:                                    # l = 1 in any order and logf(1) = 0: the lse is the logit itself
                beta = 0.0
            case._rows[key] = RowInfo(top, lse, M, beta, exact)
    return case._rows[key]


def score32(sc, x, lse):
    """fp32(sc + fp32(x - lse)); -inf where x or sc is -inf"""
    if x == NEG or sc == NEG:
        return np.float32(NEG)
    return np.float32(sc) + np.float32(x - lse)


def score_beta(info, x, s):
    return 0.0 if s == NEG else 1.01 * (info.beta_lse + 2 * U * (abs(x - info.lse) + abs(float(s))))


@dataclass
class Cand:
    s: np.float32
    flat: int
    k: int
    x: float
    r: int                                                # the logit row
    sc: np.float32                                        # the beam's score on entry
    sc_beta: float                                        # the bound carried by that score (second calls)


@dataclass
class ItemWalk:
    cands: list                                           # every candidate of the item in rank order
    n_read: int
    live: list                                            # (score, parent, token)
    fins: list                                            # (slot, parent, score)


@dataclass
class Reference:
    state: dict                                           # the nine tensors after the call(s), numpy
    tol_scores: np.ndarray                                # (B * K,) the bound on each live score (0: must be bit-identical)
    tol_fin: np.ndarray                                   # (B, K) the bound on each stored score before the powf tolerance
    calls: list                                           # per call, per item: ItemWalk or None (nothing changed)


def _ref_step(case, st, pos, tol_s, tol_f, contiguous):
    B, K, V, T, Tp, eos = case.B, case.K, case.V, case.T, case.Tp, case.eos
    X, out = case.x64(), []
    for b in range(B):
        if st["done"][b] or pos < Tp or pos >= T:
            out.append(None)
            continue
        cands = []
        for k in range(K):
            r = case.row(b, k)
            info, sc = row_info(case, r, contiguous), st["scores"][b * K + k]
            for v in info.top:
                xv = float(X[r, v])
                cands.append(Cand(score32(sc, xv, info.lse), k * V + int(v), k, xv, r, sc, float(tol_s[b * K + k])))
        cands.sort(key=lambda c: (-float(c.s), c.flat))
        nf, live, fins, n_read = int(st["fin_count"][b]), [], [], 0
        norm = np.float32(pos - Tp + 1) ** np.float32(case.lp)
        for c in cands[:2 * K]:
            if len(live) >= K:
                break
            n_read += 1
            v = c.flat - c.k * V
            if eos is not None and v == eos and np.isfinite(c.s):
                if nf < K:
                    fins.append((nf, c.k, c.s, c))
                    nf += 1
            else:
                live.append((c.s, c.k, v, c))
        assert len(live) == K
        h0, r0, ts0 = st["hist"][b * K:(b + 1) * K].copy(), st["rows"][b * K:(b + 1) * K].copy(), tol_s[b * K:(b + 1) * K].copy()
        for slot, k, s, c in fins:
            st["fin_scores"][b, slot] = np.float32(s) / norm
            tol_f[b, slot] = (score_beta(row_info(case, c.r, contiguous), c.x, s) + ts0[k]) / float(norm)
            st["fin_tokens"][b, slot, :pos] = h0[k, :pos]
            st["fin_tokens"][b, slot, pos] = eos
        for i, (s, k, v, c) in enumerate(live):
            r = b * K + i
            st["scores"][r], st["parents"][r], st["next_ids"][r] = s, k, v
            tol_s[r] = 0.0 if s == NEG else score_beta(row_info(case, c.r, contiguous), c.x, s) + ts0[k]
            st["hist"][r, :pos], st["hist"][r, pos] = h0[k, :pos], v
            st["rows"][r, :pos], st["rows"][r, pos] = r0[k, :pos], r
        st["fin_count"][b], st["done"][b] = nf, int(nf >= K)
        out.append(ItemWalk(cands, n_read, [l[:3] for l in live], [f[:3] for f in fins]))
    return out


def _reference(case, contiguous):
    st = {n: t.numpy().copy() for n, t in case.state0().items()}
    tol_s, tol_f = np.zeros(case.B * case.K), np.zeros((case.B, case.K))
    calls = [_ref_step(case, st, case.pos + c, tol_s, tol_f, contiguous) for c in range(case.calls)]
    return Reference(st, tol_s, tol_f, calls)


def reference(case, contiguous=False):
    """the state after the case's call(s) by the documented definition, with the bounds of its scores (contiguous: for logits
    laid out without offset or gaps, whose rows have other addition chains)"""
    key = ("ref", contiguous)
    if key not in case._rows:
        case._rows[key] = _reference(case, contiguous)
    return case._rows[key]


def compare(case, ref, got, wide=None):
    """got: {name: CPU tensor} after the call(s).  Integers bit for bit, infinities equal, finite scores within their bound, stored
    scores within bound / norm + 1e-5 relative; poisoned columns untouched -> the largest |score - reference| / bound"""
    frac = 0.0
    for name in FIELDS:
        g, w = got[name].numpy().reshape(ref.state[name].shape), ref.state[name]
        if name not in ("scores", "fin_scores"):
            assert np.array_equal(g, w), (case.name, name, np.argwhere(g != w)[:4].tolist())
            continue
        tol = ref.tol_scores if name == "scores" else ref.tol_fin + 1e-5 * np.abs(np.where(np.isfinite(w), w, 0.0)) * (ref.tol_fin > 0)
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin) and np.array_equal(g[~fin], w[~fin]), (case.name, name)
        err = np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float64))
        same = tol[fin] == 0
        assert np.array_equal(g[fin][same], w[fin][same]), (case.name, name, "an entry the call must not change")
        if (~same).any():
            f = float((err[~same] / tol[fin][~same]).max())
            assert f <= 1.0, (case.name, name, f)
            frac = max(frac, f)
    for name, t in (wide or {}).items():
        t = t.cpu()
        assert bool((t[:, :case.ld_pad] == POISON).all()) and bool((t[:, case.ld_pad + case.T:] == POISON).all()), (case.name, name)
    return frac


def _span(c, info):
    """the fp32 scores of a candidate with its beam's lse moved by +-beta_lse (and its entry score by the bound it carries)"""
    if c.s == NEG:
        return NEG, NEG
    lo = float(score32(c.sc, c.x, info.lse + info.beta_lse)) - c.sc_beta
    hi = float(score32(c.sc, c.x, info.lse - info.beta_lse)) + c.sc_beta
    return lo, hi


def _collapse_holds(a, b, info):
    """two candidates of one beam whose different logits round to one score: the same for every fp32 lse within beta_lse"""
    l, hi, n = np.float32(info.lse - info.beta_lse), np.float32(info.lse + info.beta_lse), 0
    while l <= hi and n < 4096:
        if score32(a.sc, a.x, float(l)) != score32(b.sc, b.x, float(l)):
            return False
        l, n = np.nextafter(l, np.float32(np.inf)), n + 1
    return n < 4096


def decided(case, contiguous=False):
    """None if no fp32 evaluation whose lse lies within beta_lse of the true one can change what the walk observes: the order and
    tie status of adjacent candidates among the ranks read and the first rank not read.  Which logits fall inside a beam's 2K is a
    comparison of stored values and cannot move.  Ties are robust between equal logits of one beam, between -inf scores, and across
    beams only between exact rows with the same (c, n) and the same entry score.  Otherwise the reason the case is unfit."""
    for call in reference(case, contiguous).calls:
        for b, w in enumerate(call):
            if w is None:
                continue
            for i in range(min(w.n_read, len(w.cands) - 1)):
                p, q = w.cands[i], w.cands[i + 1]
                ip, iq = row_info(case, p.r, contiguous), row_info(case, q.r, contiguous)
                (plo, phi), (qlo, qhi) = _span(p, ip), _span(q, iq)
                where = f"{case.name}: item {b} ranks {i}, {i + 1}"
                if phi == NEG and qhi == NEG:
                    continue
                if p.k == q.k:
                    if p.x == q.x or (p.x > q.x and p.flat < q.flat) or plo > qhi:
                        continue
                    if p.x < q.x and p.sc_beta == 0 and _collapse_holds(p, q, ip):
                        continue
                    return where + " (one beam): the tie status can change"
                elif plo > qhi:
                    continue
                elif (ip.exact is not None and ip.exact == iq.exact and p.sc == q.sc and p.x == q.x and p.sc_beta == 0
                      and q.sc_beta == 0):
                    continue
                return where + f": scores {float(p.s)!r} [{plo!r}, {phi!r}] and {float(q.s)!r} [{qlo!r}, {qhi!r}] can swap or tie"
    return None


def min_gap(case):
    """the smallest score difference between adjacent candidates among the ranks read and the first not read (inf: none finite)"""
    g = math.inf
    for call in reference(case).calls:
        for w in call:
            if w is not None:
                for i in range(min(w.n_read, len(w.cands) - 1)):
                    a, b = float(w.cands[i].s), float(w.cands[i + 1].s)
                    if b != NEG:
                        g = min(g, a - b)
    return g


# ---- builders ----
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tokens(gen, V, n, exclude=()):
    ex = set(int(e) for e in exclude if e is not None)
    return [int(v) for v in torch.randperm(V, generator=gen).tolist() if v not in ex][:n]


def logits_from_targets(targets, V, dtype, gen, bg=40.0):
    """targets[k]: (token, target score) of beam k.  With sc[k] = logsumexp of the beam's targets and x[k, token] = target - sc[k]
    the beam's lse is 0 and each planted candidate scores its target (up to the rounding of x to its storage type and a background
    `bg` or more below the beam's smallest planted logit).  A beam with no target gets a score 30 below every target.
    -> (x (K, V) in dtype, sc (K,) fp32)"""
    K = len(targets)
    x, sc = torch.empty(K, V, dtype=torch.float64), torch.empty(K)
    lowest = min((s for t in targets for _, s in t), default=0.0)
    for k, t in enumerate(targets):
        assert len({v for v, _ in t}) == len(t) <= 2 * K
        S = torch.tensor([s for _, s in t], dtype=torch.float64)
        sc[k] = float(torch.logsumexp(S, 0)) if t else lowest - 30.0
        vals = S - float(sc[k])
        x[k] = (float(vals.min()) if t else 0.0) - bg - torch.rand(V, generator=gen, dtype=torch.float64)
        if t:
            x[k, [v for v, _ in t]] = vals
    return x.float().to(dtype), sc


def logits_for_walk(plan, K, V, dtype, gen, top=-1.0, gap=1.5, fill=None):
    """plan: the (parent, token) of the item's candidates in rank order (token == eos: an eos candidate); rank r is given the target
    score top - gap * r.  fill: {k: tokens} further candidates of beam k, gap apart, 5 or more below the plan's last rank.
    -> (x (K, V), sc (K,))"""
    targets = [[] for _ in range(K)]
    for r, (k, v) in enumerate(plan):
        targets[k].append((int(v), top - gap * r))
    low = top - gap * len(plan) - 5.0
    for k, toks in (fill or {}).items():
        targets[k] += [(int(v), low - gap * j) for j, v in enumerate(toks)]
    return logits_from_targets(targets, V, dtype, gen)


def expected_walk(plan, K, eos):
    """the prefix of a plan that the walk reads: up to its K-th live candidate"""
    out, nl = [], 0
    for k, v in plan:
        if nl == K:
            break
        out.append((k, v))
        nl += v != eos
    return out


def _planned(name, family, plans, K, V, dtype, gen, eos=None, fills=None, **kw):
    """a case of one planned item per plan"""
    xs, scs = zip(*[logits_for_walk(p, K, V, dtype, gen, fill=(fills or [None] * len(plans))[i]) for i, p in enumerate(plans)])
    return Case(name, family, len(plans), K, torch.cat(xs), torch.cat(scs), eos=eos, plans=list(plans), **kw)


def _dense(gen, K, V, dtype, scale=3.0, eos=None, lift=6.0, avoid=()):
    """K random rows whose 2K + 1 largest logits are 1.5 apart (at none of the indices `avoid`), with entry scores 4 apart in a
    random beam order"""
    x = torch.randn(K, V, generator=gen) * scale
    for k in range(K):
        toks = _tokens(gen, V, 2 * K + 1, (eos, *avoid))
        x[k, toks] = float(x[k].max()) + 1.5 * torch.arange(2 * K + 1, 0, -1) + torch.rand(1, generator=gen)
        if eos is not None:
            x[k, eos] = float(x[k].max()) - lift * float(torch.rand(1, generator=gen))
    sc = -4.0 * torch.randperm(K, generator=gen).float() - torch.rand(K, generator=gen)
    return x.to(dtype), sc


DTYPES = (torch.float32, torch.bfloat16)


# ---- the families ----
def beam_counts():
    """K = 1 .. 8 at B = 1 (random rows) and B = 3 (the item's 2K from one beam, from all beams, from the last beam only), V = 4099:
    several slices, and a row stride that gives every beam row another alignment"""
    out, V, eos = [], 4099, 4000
    for dtype in DTYPES:
        for K in range(1, 9):
            g = _gen(100 + K)
            x, sc = _dense(g, K, V, dtype, eos=eos)
            out.append(Case(f"counts-K{K}-B1-{tag(dtype)}", "beam_counts", 1, K, x, sc, eos=eos))
            plans = []
            for beams in ([K // 2], list(range(K)), [K - 1]):
                toks = {k: _tokens(g, V, 2 * K, (eos,)) for k in beams}
                plan = [(beams[r % len(beams)], toks[beams[r % len(beams)]][r // len(beams)]) for r in range(2 * K)]
                if K > 1:
                    plan[1] = (plan[1][0], eos)
                plans.append(plan)
            out.append(_planned(f"counts-K{K}-B3-{tag(dtype)}", "beam_counts", plans, K, V, dtype, g, eos=eos))
    return out


def one_thread():
    """B * K >= 256 rows of V = 8192 (two slices of 8 (fp32) / 4 (bf16) vectors per thread): the 2K largest logits of every beam row
    of item 0 in one thread's registers, of item 1 spread over one slice, of item 2 over the last slice.  Every rank of item b comes
    from its beam b + 1, so the walk reads K + 1 entries (eos among them, items 0 and 1) of one per-thread or per-slice list.  The
    other items are done."""
    out, V, B = [], 8192, 37
    for dtype in DTYPES:
        for K in (7, 8):
            g, p = _gen(200 + K), partition(V, dtype, 0, B, K)            # V * es is a multiple of 16: one alignment for all rows
            plans, fills, claims, eos = [], [], [], None
            for b, (mode, s) in enumerate((("thread", 0), ("slice", 0), ("slice", 1))):
                toks = {}
                for k in range(K):
                    own = (p.slice == s) & (p.kind == VEC)
                    if mode == "thread":
                        own &= p.thread == 5 + 17 * k
                    idx = np.nonzero(own)[0]
                    idx = idx[-2 * K:] if mode == "thread" else idx[torch.randperm(len(idx), generator=g)[:2 * K].numpy()]
                    toks[k] = [int(v) for v in idx if int(v) != eos or k == b + 1][:2 * K]
                    claims.append((b * K + k, mode, s, 5 + 17 * k))
                if b == 0:
                    eos = toks[1][1]
                elif b == 1 and eos not in toks[2]:
                    toks[2][1] = eos
                plans.append([(b + 1, v) for v in toks[b + 1]])
                fills.append({k: toks[k] for k in range(K) if k != b + 1})
            xs, scs = zip(*[logits_for_walk(pl, K, V, dtype, g, fill=f) for pl, f in zip(plans, fills)])
            x = torch.cat(list(xs) + [torch.zeros((B - 3) * K, V, dtype=dtype)])
            sc = torch.cat(list(scs) + [torch.zeros((B - 3) * K)])
            out.append(Case(f"one-thread-K{K}-{tag(dtype)}", "one_thread", B, K, x, sc, eos=eos, plans=plans + [None] * (B - 3),
                            fin_count=[0, 0, 0] + [K] * (B - 3), done=[0, 0, 0] + [1] * (B - 3), claims=claims))
    return out


def _rotation(name, dtype, V, offset, B=24, K=2):
    """item b's rank-r candidate is beam r % K's special element number b + r // K (the scalar head and tail elements, the first
    and last element of every slice, in index order, cyclically): every special element of beam 0 holds the item's best candidate
    in one item, and each beam's 2K largest logits are special elements"""
    g, plans, fills, claims = _gen(300 + offset), [], [], []
    assert V * (16 // epv(dtype)) % 16 == 0               # every row has the alignment of row 0
    sp = [sorted(partition(V, dtype, (offset + k * V) * (16 // epv(dtype)) % 16, B, K).specials(epv(dtype))) for k in range(K)]
    assert all(len(s) <= B for s in sp)
    for b in range(B):
        plans.append([(r % K, sp[r % K][(b + r // K) % len(sp[r % K])]) for r in range(2 * K)])
        fills.append({k: [sp[k][(b + 2 + j) % len(sp[k])] for j in range(2 * K - 2)] for k in range(K)})
        claims.append((b * K, "special", plans[-1][0][1], None))
    c = _planned(name, "edges", plans, K, V, dtype, g, fills=fills, offset=offset)
    c.claims = claims
    return c


def edges():
    out = []
    for dtype in DTYPES:
        E, t = epv(dtype), tag(dtype)
        for off in range(E):                              # four slices; V a multiple of 8 elements keeps one alignment per beam
            out.append(_rotation(f"edge-rotation-off{off}-{t}", dtype, 2056 if dtype == torch.float32 else 4104, off))
        out.append(_rotation(f"edge-short-slices-{t}", dtype, 256 * E, 1))       # 255 vectors in two slices: 127 and 128
        for V in range(2, 10):
            for off in range(E):
                for K in (1, 8):
                    g = _gen(1000 * V + 10 * off + K)
                    x = torch.stack([torch.randperm(V, generator=g).float() for _ in range(2 * K)])
                    sc = -0.13 * torch.randperm(2 * K, generator=g).float()     # no difference of two is a whole number
                    out.append(Case(f"edge-V{V}-off{off}-K{K}-{t}", "edges", 2, K, x.to(dtype), sc, eos=V - 1, offset=off))
        g = _gen(77)
        x, sc = zip(*[_dense(g, 4, 2051, dtype, eos=9) for _ in range(2)])
        out.append(Case(f"edge-row-gap-{t}", "edges", 2, 4, torch.cat(x), torch.cat(sc), eos=9, offset=1, sk=2051 + 5))
        x = [_dense(g, 4, 2051, dtype, eos=9)[0][:1] for _ in range(2)]
        sc = -3.0 * torch.randperm(8, generator=g).float() - torch.rand(8, generator=g)
        out.append(Case(f"edge-shared-rows-{t}", "edges", 2, 4, torch.cat(x), sc, eos=9, offset=3, sk=2051 + 2))
    return out


def ties():
    out = []
    for dtype in DTYPES:
        t, E = tag(dtype), epv(dtype)
        for name, sc in (("equal-scores", torch.full((8,), -1.0)), ("own-scores", -1.0 - torch.tensor([3., 1, 0, 2, 7, 5, 4, 6]))):
            out.append(Case(f"tie-all-equal-{name}-{t}", "ties", 1, 8, torch.full((8, 4096), 0.5).to(dtype), sc, eos=3, offset=1,
                            sk=4097))
        g = _gen(400)                                     # one value at 15 places of every beam: head, tail, slice edges, elsewhere
        x = (-40.0 - torch.rand(4, 4099, generator=g))
        for k in range(4):
            p = partition(4099, dtype, (1 + k * 4099) * (16 // E) % 16, 1, 4)
            sp = sorted(p.specials(E))
            x[k, sp[:12] + _tokens(g, 4099, 15 - len(sp[:12]), sp)] = 2.0    # 15 equal logits: specials first, then anywhere
        out.append(Case(f"tie-spread-{t}", "ties", 1, 4, x.to(dtype), torch.tensor([-3.0, -1.0, -4.0, -2.0]), eos=0, offset=1))
        x = torch.full((4, 4096), NEG)                    # exact rows: 1024 entries of 1.25, elsewhere -inf, other places per beam
        for k in range(4):
            x[k, _tokens(g, 4096, 1024)] = 1.25
        out.append(Case(f"tie-exact-rows-{t}", "ties", 1, 4, x.to(dtype), torch.full((4,), -2.0), eos=None, offset=2, sk=4097))
        x = torch.full((4, 4099), NEG)                    # a -inf tie group: two finite candidates, then -inf by flat index
        x[0, 4098], x[2, 0], x[3, 2048] = 1.0, 0.0, -1.0
        out.append(Case(f"tie-neg-inf-{t}", "ties", 1, 4, x.to(dtype), torch.tensor([-1.0, -9.0, -5.0, NEG]), eos=1, offset=1))
        x = torch.full((1, 8), -5.0)                      # the large-score twin: 3 and 2.99 fall into one fp32 cell at -1e6
        x[0, 5], x[0, 2] = 3.0, 2.99
        out.append(Case(f"tie-collapse-large-{t}", "ties", 1, 1, x.to(dtype), torch.tensor([-1e6]), eos=7))
    x = torch.full((1, 8), -5.0)                          # the per-beam cut is by logit: x[5] is in the beam's two best, x[2] is not
    x[0, 5], x[0, 2], x[0, 7] = 3.0, float(np.nextafter(np.float32(3.0), np.float32(0.0))), 9.0
    out.append(Case("tie-collapse-cut-f32", "ties", 1, 1, x, torch.tensor([-30.0]), eos=7))
    return out


def _walk_grid(K, dtype, V=300):
    """item (f, e): fin_count f on entry and e eos candidates ahead of the K-th live one, eos and live ranks alternating"""
    g, eos, plans, fc = _gen(500 + K), 11, [], []
    for f in range(K):
        for e in range(K + 1):
            toks = _tokens(g, V, 2 * K, (eos,))
            plan, ne, nl = [], 0, 0
            while nl < K:
                if ne < e and (ne <= nl or nl == K - 1):
                    plan.append((ne, eos))                   # one eos candidate per beam
                    ne += 1
                else:
                    plan.append(((nl * 5 + e) % K, toks[nl]))
                    nl += 1
            if len(plan) < 2 * K:
                plan.append(((e + f) % K, toks[K]))       # the first rank the walk does not read
            plans.append(plan)
            fc.append(f)
    return _planned(f"walk-grid-K{K}-{tag(dtype)}", "walk", plans, K, V, dtype, g, eos=eos, fin_count=fc)


def walk():
    out = []
    for dtype in DTYPES:
        t = tag(dtype)
        out += [_walk_grid(K, dtype) for K in (1, 4, 8)]
        g, K, V, eos = _gen(600), 4, 300, 11
        tk = _tokens(g, V, 40, (eos,))
        # item 0 stores its K-th hypothesis and is done, the second call must leave it alone; item 1 advances twice
        plans = [[(2, eos), (0, tk[0]), (1, tk[1]), (0, tk[2]), (3, tk[3])], [(1, tk[4]), (0, eos), (0, tk[5]), (2, tk[6]), (1, tk[7])]]
        out.append(_planned(f"walk-done-second-call-{t}", "walk", plans, K, V, dtype, g, eos=eos, fin_count=[K - 1, 0], calls=2))
        x = torch.full((4 * K, V), NEG)                   # items with 0, 1 and K - 1 finite candidates; an eos whose logit is -inf
        x[K, 40] = 0.5
        x[2 * K, 5], x[2 * K, 9], x[2 * K + 1, eos] = 1.0, -1.0, 0.0
        x[3 * K, 200] = 2.0
        sc = torch.tensor([-1.0, -2, -3, -4] + [-1.0, NEG, -3, -4] + [-1.0, -6, NEG, NEG] + [-1.0, NEG, NEG, NEG])
        out.append(Case(f"walk-few-finite-{t}", "walk", 4, K, x.to(dtype), sc, eos=eos))
        out.append(Case(f"walk-eos-neg-inf-{t}", "walk", 4, K, x.to(dtype), sc, eos=0))     # eos = 0 leads every -inf tie group
        plan = [(k % K, tk[8 + k]) for k in range(2 * K)]
        out.append(_planned(f"walk-no-eos-{t}", "walk", [plan], K, V, dtype, g, eos=None))
        plan = [(1, eos), (0, tk[20]), (3, eos), (1, tk[21]), (2, tk[22]), (0, tk[23]), (2, tk[24])]
        for lp in (0.0, 0.9, 1.0, 2.0):
            out.append(_planned(f"walk-length-penalty-{lp}-{t}", "walk", [plan], K, V, dtype, g, eos=eos, lp=lp, fin_count=[1]))
        for pos in (2, 12):
            out.append(_planned(f"walk-pos-{pos}-out-of-range-{t}", "walk", [plan], K, V, dtype, g, eos=eos, pos=pos))
    return out


def lse():
    out = []
    for dtype in DTYPES:
        t, E, g = tag(dtype), epv(dtype), _gen(700)
        V, K = 512 * E + 5, 2                             # four slices, and a scalar tail at offset 1
        p = partition(V, dtype, 16 // E, 1, K)            # beam 0's row, one element past a 16-byte boundary
        dead = np.nonzero((p.slice == 1) & (p.kind == VEC))[0]
        x, sc = _dense(g, K, V, dtype, eos=5, avoid=dead.tolist())
        x[0, torch.from_numpy(dead)] = NEG                # a slice of -inf only
        out.append(Case(f"lse-dead-slice-{t}", "lse", 1, K, x, sc, eos=5, offset=1))
        x = torch.full((K, V), NEG)                       # the only finite logit in the scalar tail
        x[0, V - 1], x[1, V - 1] = 2.5, -1e30
        assert p.kind[V - 1] == TAIL
        out.append(Case(f"lse-tail-only-{t}", "lse", 1, K, x.to(dtype), torch.tensor([-1.0, -2.0]), eos=5, offset=1))
        x, sc = _dense(g, K, V, dtype, eos=5)             # one logit 100 above the rest: every other term underflows
        x[0, 1000] = float(x[0].float().max()) + 100.0
        x[1, V - 2] = float(x[1].float().max()) + 100.0
        out.append(Case(f"lse-peak-{t}", "lse", 1, K, x, sc, eos=5, offset=1))
        low = torch.randperm(V, generator=g)[:V // 2].tolist()
        x, sc = _dense(g, K, V, dtype, eos=5, avoid=low)  # finite logits at -1e30 beside ordinary ones
        x[:, [v for v in low if v != 5]] = -1e30
        out.append(Case(f"lse-huge-negative-{t}", "lse", 1, K, x, sc, eos=5, offset=1))
        out.append(Case(f"lse-equal-16384-{t}", "lse", 1, 1, torch.full((1, 2 ** 14), -0.75).to(dtype), torch.tensor([-2.0]), eos=1,
                        offset=3))
    even = list(range(0, 4099, 2))
    x, sc = _dense(_gen(701), 2, 4099, torch.bfloat16, eos=5, avoid=even)         # bf16 groups: half the row on 16 values of [8, 9)
    x[:, ::2] = (8.0 + torch.randint(0, 16, (2, 2050), generator=_gen(702)) / 16.0).to(torch.bfloat16)
    out.append(Case("lse-bf16-groups-bf16", "lse", 1, 2, x, sc, eos=5, offset=1))
    return out


def _perms(K):
    return {"identity": list(range(K)), "reversed": list(range(K - 1, -1, -1)), "from-last": [K - 1] * K, "from-first": [0] * K,
            "cyclic": [(k + 1) % K for k in range(K)], "repeats": [(k // 2 * 3 + 1) % K for k in range(K)]}


def reorder():
    """T = 600: the reorder of 1 .. 3 column blocks by six parent permutations (one item each), two hypotheses finished from
    parents in the same blocks, hist / rows as column views of wider poisoned tensors"""
    out, V, eos = [], 300, 11
    for dtype in DTYPES:
        for K in (2, 7, 8):
            for pos in (1, 255, 256, 257, 511, 512, 513, 599):
                g, plans = _gen(800 + K), []
                for par in _perms(K).values():
                    toks = _tokens(g, V, K, (eos,))
                    plan = [(par[0], eos), (par[0], toks[0]), ((par[0] + 1) % K, eos)] + [(par[i], toks[i]) for i in range(1, K)]
                    plans.append(plan)
                out.append(_planned(f"reorder-K{K}-pos{pos}-{tag(dtype)}", "reorder", plans, K, V, dtype, g, eos=eos, T=600, Tp=1,
                                    pos=pos, ld_pad=3))
    return out


FAMILIES = {"beam_counts": beam_counts, "one_thread": one_thread, "edges": edges, "ties": ties, "walk": walk, "lse": lse,
            "reorder": reorder}
GUARDED = {"beam_counts": "counts-K7-B3-f32", "one_thread": "one-thread-K7-bf16", "edges": "edge-V3-off0-K8-f32",
           "ties": "tie-spread-bf16", "walk": "walk-grid-K8-f32", "lse": "lse-dead-slice-f32", "reorder": "reorder-K8-pos599-bf16"}


@functools.lru_cache(maxsize=None)
def cases(family):
    out = FAMILIES[family]()
    assert len({c.name for c in out}) == len(out) and all(c.family == family for c in out)
    return out


def case(family, name):
    return next(c for c in cases(family) if c.name == name)
