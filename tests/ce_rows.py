"""Cases, a float64 reference and derived rounding bounds for the cross-entropy kernels (mopk_cross_entropy_*), shared by
test_cross_entropy_cpu.py and test_gpu_cross_entropy.py.

The reference works on the logits AS STORED (a bf16 case is rounded to bf16 first, then widened exactly), so the bounds below hold
the arithmetic alone to account, never the storage format.

The bounds, with u = 2^-24 (half an ulp of fp32, relative) and the kernel's shape: THREADS = 1024 threads per row, WAVES = 16,
16-byte vectors of EPV = 4 (fp32) / 8 (bf16) elements.

Row loss.  A thread folds its elements into (m, l) one by one: at most chain(V) = EPV * ceil(floor(V / EPV) / THREADS) + 1 steps
(its strided vectors, one head or tail element).  A step is l * expf(m - f) + 1 or l + expf(f - m): expf within 1 ulp (2 u), its
argument's rounding u |f - m| weighs u |d| e^-|d| <= 0.37 u against l >= 1, one product, one sum: under 4 u of l.  A merge of two
pairs (6 xor levels in the wave, then WAVES - 1 in wave order) is two such products and a sum: again under 4 u.  So l is off by at
most 4 u depth relatively, depth(V) = chain(V) + 6 + WAVES, and so is log l absolutely.  0 <= log l <= ln V, so logf (1 ulp) adds
at most 2 u ln V; the sum m + log l rounds to within u |lse|, the difference lse - x_t to within u |loss|:

    lse_bound = u (4 depth(V) + 2 ln V + |lse|),    loss_bound = lse_bound + u |loss|.

(The trial bound this replaces, u (4 (ceil(V / threads) + 6 + waves) + 2 |lse| + |x_t| + |loss|), charged the logarithm's rounding
to |lse| and |x_t|; log l is bounded by ln V whatever the row's offset, which is what is charged here.)

Sum / mean.  The reduce accumulates the fp32 row losses in double (error ~ 2^-53 R, nothing here) and rounds once:
sum_bound = sum of the rows' loss_bound + u |sum|;  mean_bound = sum_bound / n + u |mean|.

Gradient d_j = g (p_j - [j == t]), p_j = expf(x_j - lse).  The exponent's argument carries lse's absolute error and its own
rounding u |x_j - lse|; expf adds 2 u: p_j is off by p_j (lse_bound + u |x_j - lse| + 2 u).  g = grad * scale is one product of
a scale 1 / n rounded once against the exact g / n (3 u), the difference p_j - [.] and the product with g round once each, and the
result is rounded to the output dtype (fp32: u; bf16: 2^-8, its 8 significant bits; relative), with fp32's smallest normal as the floor:

    grad_bound_j = |g| (p_j (lse_bound + u |x_j - lse| + 2 u) + 5 u |p_j - [j == t]|) + r_out |d_j| + 2^-126.
"""
import math

import torch

THREADS = 1024
WAVES = 16
U = 2.0 ** -24


def epv(dtype) -> int:
    return 8 if dtype == torch.bfloat16 else 4


def chain(V: int, dtype) -> int:
    e = epv(dtype)
    return e * math.ceil((V // e) / THREADS) + 1


def depth(V: int, dtype) -> int:
    return chain(V, dtype) + 6 + WAVES


def span(start: int, V: int, dtype):
    """(head, nvec, tail0) of a row of V elements that starts `start` elements behind a 16-byte boundary: RowSpan of row_helpers.h"""
    e = epv(dtype)
    head = min((-start) % e, V)
    nvec = (V - head) // e
    return head, nvec, head + nvec * e


def positions(start: int, V: int, dtype):
    """name -> element index of the places a row walk can lose or double: the ends of the head, of the first vector, of a thread's
    first sweep, the start of its second, the last vector element, the first tail element, the row's last.  Places a row does not
    have (no head, one sweep only, no tail) are left out."""
    e = epv(dtype)
    head, nvec, tail0 = span(start, V, dtype)
    pos = {"first": 0, "last": V - 1}
    if head:
        pos["head_last"] = head - 1
    if nvec:
        pos["vec0_first"], pos["vec0_last"], pos["vec_last"] = head, head + e - 1, tail0 - 1
    if nvec > THREADS:
        pos["sweep0_last"], pos["sweep1_first"] = head + THREADS * e - 1, head + THREADS * e
    if tail0 < V:
        pos["tail_first"] = tail0
    return pos


def stored(x: torch.Tensor, dtype) -> torch.Tensor:
    """x rounded to the case's dtype (what the kernel is given)"""
    return x.to(dtype)


def counted(targets: torch.Tensor, V: int, ignore_index: int) -> torch.Tensor:
    return (targets != ignore_index) & (targets >= 0) & (targets < V)


class Ref:
    """float64 loss, lse and softmax of stored logits (R, V) against targets, with the bounds of the module docstring"""

    def __init__(self, logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100):
        x = logits.detach().cpu().to(torch.float64)
        t = targets.detach().cpu()
        R, V = x.shape
        self.R, self.V, self.dtype = R, V, logits.dtype
        self.valid = counted(t, V, ignore_index)
        self.t = torch.where(self.valid, t, torch.zeros_like(t))
        self.x = x
        self.lse = torch.logsumexp(x, 1)
        self.x_t = x.gather(1, self.t[:, None])[:, 0]
        self.loss = torch.where(self.valid, self.lse - self.x_t, torch.zeros(R, dtype=torch.float64))
        self.n = int(self.valid.sum())
        d = depth(V, logits.dtype)
        self.lse_bound = U * (4 * d + 2 * math.log(V) + self.lse.abs())
        self.loss_bound = torch.where(self.valid, self.lse_bound + U * self.loss.abs(), torch.zeros(R, dtype=torch.float64))

    def reduced(self, reduction: str):
        """(value, bound) of the reduction in float64"""
        if reduction == "none":
            return self.loss, self.loss_bound
        s = self.loss.sum()
        sb = self.loss_bound.sum() + U * s.abs()
        if reduction == "sum":
            return s, sb
        if self.n == 0:
            return torch.tensor(float("nan"), dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)
        return s / self.n, sb / self.n + U * (s / self.n).abs()

    def grad(self, reduction: str, upstream):
        """(gradient (R, V), bound (R, V)) for an upstream scalar or per-row vector (float64)"""
        g = torch.as_tensor(upstream, dtype=torch.float64).reshape(-1 if reduction == "none" else 1)
        g = g.expand(self.R) if g.numel() == 1 else g
        if reduction == "mean":
            g = g / max(self.n, 1)
        g = torch.where(self.valid, g, torch.zeros_like(g))[:, None]
        arg = self.x - self.lse[:, None]
        p = torch.exp(arg)
        hot = torch.zeros_like(p)
        hot[torch.arange(self.R), self.t] = 1.0
        d = g * (p - hot)
        arg_abs = torch.where(torch.isinf(arg), torch.zeros_like(arg), arg.abs())
        r_out = 2.0 ** -8 if self.dtype == torch.bfloat16 else U
        bound = g.abs() * (p * (self.lse_bound[:, None] + U * arg_abs + 2 * U) + 5 * U * (p - hot).abs()) + r_out * d.abs() + 2.0 ** -126
        return d, torch.where(self.valid[:, None], bound, torch.zeros_like(bound))


def worst(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """the largest |got - want| / bound (0 / 0 counts as 0; a NaN or a miss of a zero bound as inf)"""
    err = (got.detach().cpu().to(torch.float64) - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    frac = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(frac.max()) if frac.numel() else 0.0


def dropped_and_doubled(x_row: torch.Tensor, t: int, j: int):
    """the float64 loss of a stored row with element j left out of the sum, and with it counted twice"""
    x = x_row.detach().cpu().to(torch.float64)
    keep = torch.ones_like(x, dtype=torch.bool)
    keep[j] = False
    lse_drop = torch.logsumexp(x[keep], 0)
    lse_twice = torch.logsumexp(torch.cat([x, x[j:j + 1]]), 0)
    return float(lse_drop - x[t]), float(lse_twice - x[t])


# ---- case builders (CPU fp32 tensors; the tests round them with stored() and lay them out) ----
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def normal(R: int, V: int, seed: int = 0, scale: float = 1.0):
    g = _gen(seed)
    return torch.randn(R, V, generator=g) * scale, torch.randint(0, V, (R,), generator=g)


def lengths(dtype):
    e = epv(dtype)
    return sorted({2, 3, e - 1, e, e + 1, 2 * e + 1, 1000, THREADS * e - 1, THREADS * e, THREADS * e + 1, 2 * THREADS * e + e + 3})


def position_shape(dtype):
    """(V, ld, start): V = T EPV + EPV + 3, an odd row stride (every row at another phase), row 0 two elements before a boundary"""
    e = epv(dtype)
    V = THREADS * e + e + 3
    return V, V + 2, e - 2                                      # V is odd, and so is V + 2


def position_cases(dtype, R: int = 3, seed: int = 7):
    """[(name, row, element, logits (R, V), targets_elsewhere (R,), targets_on_it (R,))]: one logit of +12 over N(0, 1) noise on each
    place of positions(), row by row (every row of the odd-stride layout sits at another phase)"""
    V, ld, start = position_shape(dtype)
    out = []
    for r in range(R):
        for name, j in sorted(positions(start + r * ld, V, dtype).items()):
            x, t = normal(R, V, seed + 31 * r + j % 97)
            x[r, j] = 12.0
            t[r] = (j + V // 2) % V
            t_on = t.clone()
            t_on[r] = j
            out.append((f"{name}-row{r}", r, j, x, t, t_on))
    return out


def value_cases(dtype, V: int = 1000, seed: int = 11):
    """name -> (logits (3, V), targets): peaked, offset, -inf and flat rows (-inf is never at the target)"""
    cases = {}
    x, t = normal(3, V, seed)
    hi = x.clone()
    hi[torch.arange(3), t] += 60.0
    cases["target_60_above"] = (hi, t)
    lo = x.clone()
    lo[torch.arange(3), t] -= 60.0
    cases["target_60_below"] = (lo, t)
    if dtype == torch.float32:
        cases["offset_3e4"] = (x + 3.0e4, t)
    t5 = torch.full((3,), 5, dtype=torch.long)
    a = x.clone()
    a[:, 0] = -math.inf
    cases["ninf_at_0"] = (a, t5)
    b = x.clone()
    b[:, 16:16 + epv(dtype)] = -math.inf
    cases["ninf_vector"] = (b, t5)
    c = torch.full((3, V), -math.inf)
    c[:, 5], c[:, V - 2] = x[:, 5], x[:, V - 2]
    cases["ninf_all_but_two"] = (c, t5)
    cases["flat"] = (torch.full((3, V), 0.25), t)
    return cases


def layout(x: torch.Tensor, dtype, ld: int = None, start: int = 0, pad=float("nan"), device="cpu") -> torch.Tensor:
    """the stored case as an (R, V) view with row stride ld of a 16-byte-aligned buffer, `start` elements in; the elements around
    the rows hold `pad`"""
    R, V = x.shape
    ld = V if ld is None else ld
    buf = torch.full((start + R * ld + 16,), pad, dtype=dtype, device=device)
    view = buf.as_strided((R, V), (ld, 1), buf.storage_offset() + start)
    view.copy_(stored(x, dtype))
    return view
