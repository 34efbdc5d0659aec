"""Peaked-logit inputs for the Edgewise cores, their float64 oracle in the cores' own layouts, and a model of the roundings the design
admits -- first of all the one every bf16-MFMA implementation of the operation shares: the per-view, per-dimension scale sqk_v is
folded into the bf16 query fragment, so the scores are built from bf16(q * sqk_v).  No GPU code here (tests/attn_ref.py and
tests/moe_ref.py are the models).

Why rows and not tensors: at a per-view logit standard deviation of 4 the exact result of a third of the token rows moves by more than
0.25 % of max|y| under that rounding alone, and single rows by several per cent, so no max-norm bound on a whole tensor
is both true and meaningful there.  Each token row is judged against its own conditioning, measured on the oracle (`rounding_noise`),
never on the code under test: bound = max(tol * max|ref|, 4 * the row's largest movement)."""
import functools
import math

import numpy as np
import torch

from attn_ref import bf16_exact

TOL_BF16, GTOL_BF16, GTOL_FP32 = 1e-2, 3e-2, 1e-3       # the suite's own (test_gpu_edgewise.py, test_gpu_fused_diet.py)
NOISE_FACTOR = 4.0                                      # check_grads / oracle_bf16_noise: one sample of rounding noise against another
LEVELS = (0.5, 2, 4, 8)
# (B, N, dk, V, r), H = 2: dk = 16 with two tiles, the last holding one valid key | the same tail at dk = 32, and B = 2 so that the
# per-batch partials of the small gradients are reduced | the benchmark's (b, h) problem | klast: no padding anywhere (forward only)
SHAPES = ((1, 33, 16, 2, 1), (2, 65, 32, 3, 2), (1, 197, 64, 5, 4), (1, 224, 64, 5, 4))
FWD_ONLY = (SHAPES[3],)
ROW_TENSORS = ("y", "dq", "dk", "dv")
PLANT_FACTOR = 8.0                                      # 4 is not enough at dk = 32: the identity fails by 3.4 there


def planted_tokens(N):
    """first key | the two sides of a 32-key tile edge | the last key of the last partial tile = the last query of the last block"""
    return (0, 31, 32, N - 1)


def case_seed(shape, level, plant=False, dense=False):
    """one seed per (shape, level, kind); tests/test_edgewise_peaks_cpu.py checks on the oracle alone that each of them gives inputs
    whose row bounds are not vacuous and whose planted rows obey their closed form.  (The planted offset was 500 at first: at
    (2, 65, 32, 3, 2) one planted token of 16 then had so short a q that another planted key outscored its own in the mixed logits --
    the closed form was off by 3.5 in the oracle itself.  The dense offset was 250: at level 8, 11.5 % of the rows of y then had a
    bound above ten times the tight one, over the cap of 10 %.  Conditions on the inputs, so the seeds moved, not the checks.)"""
    B, N, dk, V, r = shape
    return 1000 * N + 10 * dk + int(round(2 * level)) + (503 if plant else 0) + (253 if dense else 0)


class Case:
    """operands of one core call; float32 torch tensors, q / k / v / dy bf16-exact.  Hashable by identity: `peaked_case` is cached, so
    equal arguments give the same object and the caches of `oracle_core` / `rounding_noise` key on it."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def head_names(self):
        return ("dW1", "db1", "dW2", "db2") if self.dense else ("dWr", "dbr", "dWc", "dbc")

    def qkv(self):
        """(B,N,1,3,H,dk): the share_qkv layout both cores take"""
        return torch.stack([self.q, self.k, self.v], 2).unsqueeze(2).contiguous()


def _peaked_case(N, dk, V, r, level, seed, B=1, H=2, plant=False, dense=False):
    g = torch.Generator().manual_seed(int(seed))
    rn = lambda *s: torch.randn(*s, generator=g)
    s = math.sqrt(float(level))
    q, k = bf16_exact(rn(B, N, H, dk) * s), bf16_exact(rn(B, N, H, dk) * s)
    v, dy = bf16_exact(rn(B, N, H, dk)), bf16_exact(rn(B, N, H, dk))
    sqk = dk ** -0.5 * (1 + 0.1 * rn(V, H, dk))                  # float32, not rounded: the kernels read it as it is
    vs0, vsL = 1 + 0.1 * rn(H, dk), 1 + 0.1 * rn(H, dk)
    C = 2 * V + 2
    # un-shrunk head scale on purpose: 40 - 80 % of the gate values sit within 0.01 of 0 or 1 from level 2 up
    if dense:
        head = (rn(16, C) / math.sqrt(C), 0.1 * rn(16), rn(4, 16) / 4.0, 0.1 * rn(4))          # each weight by its fan-in, likewise
    else:
        head = (rn(4 * r, C) / math.sqrt(C), 0.1 * rn(4 * r), rn(4 * r, C) / math.sqrt(C), 0.1 * rn(4 * r))
    if plant:
        for j in planted_tokens(N):
            k[:, j] = PLANT_FACTOR * q[:, j]                     # a power of two: still bf16-exact
    return Case(N=N, dk=dk, V=V, r=r, level=level, seed=seed, B=B, H=H, plant=plant, dense=dense, q=q, k=k, v=v, dy=dy, sqk=sqk,
                vs0=vs0, vsL=vsL, chain_logit=torch.tensor(-0.5), head=head, beta_not=0.5)


peaked_case = functools.lru_cache(maxsize=None)(_peaked_case)


def shape_case(shape, level, plant=False, dense=False):
    B, N, dk, V, r = shape
    return peaked_case(N, dk, V, r, level, case_seed(shape, level, plant, dense), B=B, plant=plant, dense=dense)


def realised_logit_std(case):
    """largest and smallest per-view standard deviation of the logits (q sqk_v sqrt(dk)) . k / sqrt(dk)"""
    from attn_ref import logit_std
    stds = [logit_std(case.q * (case.sqk[v_] * case.dk ** 0.5), case.k) for v_ in range(case.V)]
    return min(stds), max(stds)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle in the cores' layouts
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_round(a, rng=None):
    """float64 array rounded to bfloat16: to nearest even, or stochastically with `rng` (gpu_util.oracle_bf16_noise)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    add = rng.integers(0, 1 << 16, size=a.shape, dtype=np.uint64) if rng is not None else (((u >> 16) & 1) + 0x7fff)
    return ((u + add) & 0xffff0000).astype(np.uint32).view(np.float32).astype(np.float64)


def fp16_round(a, rng=None):
    """float64 array rounded to float16: to nearest even, or stochastically (to either neighbour, in proportion) with `rng`"""
    a = np.asarray(a, dtype=np.float64)
    h = a.astype(np.float16)
    if rng is None:
        return h.astype(np.float64)
    err = a - h.astype(np.float64)
    other = np.nextafter(h, np.where(err >= 0, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float64)
    gap = np.abs(other - h.astype(np.float64))
    take = rng.random(a.shape) * np.where(gap > 0, gap, 1.0) < np.abs(err)
    return np.where(take, other, h.astype(np.float64))


def core_oracle(q, k, v0, vL, dy, sqk, vs0, vsL, chain_logit, head, beta_not=0.5, dense=False, rnd=None):
    """oracle/edgewise.py core_fwd / core_bwd on the operands of ops.edgewise_lowrank_core / edgewise_general_core, results in the
    layouts those return.  q, k, v0, vL, dy (B,N,H,dk); sqk (V,H,dk); vs0, vsL (H,dk); float64 numpy.  head: (Wr, br, Wc, bc), or the
    dense head's (W1, b1, W2, b2) with dense=True.  rnd: None, or rnd(site, array) -> array, the rounding model: applied to the scaled queries q * sqk_v ('q') and
    the scaled values v * vs0, v * vsL ('v') here, and handed on to core_fwd for the sites inside it.
    Returns y, dq, dk, dv0, dvL (B,N,H,dk), the per-(b,h) sums dvs0_bh, dvsL_bh (B,H,dk), dsqk (V,H,dk), dchain_logit and the head's
    gradients by name, and the forward cache under 'cache'."""
    from oracle import edgewise as oe
    hv = lambda t: np.transpose(t, (0, 2, 1, 3))                         # (B,N,H,dk) <-> (B,H,N,dk)
    dk_ = q.shape[-1]
    qs = hv(q)[None] * sqk[:, None, :, None, :]                          # (V,B,H,N,dk)
    if rnd is None:
        rnd = lambda site, x: x
    qs = rnd("q", qs)
    qv = qs * dk_ ** 0.5                                                 # core_fwd scales the scores by 1 / sqrt(dk) itself
    kv = np.broadcast_to(hv(k)[None], qv.shape)
    hd = dict(zip(("W1", "b1", "W2", "b2"), head)) if dense else None
    lr = (None,) * 4 if dense else head
    y, cache = oe.core_fwd(qv, kv, rnd("v", hv(v0) * vs0[None, :, None]), rnd("v", hv(vL) * vsL[None, :, None]), *lr, beta_not,
                           float(chain_logit), dense=hd, rnd=rnd)
    o = oe.core_bwd(hv(dy), cache)
    sc = (sqk * dk_ ** 0.5)[:, None, :, None, :]
    out = dict(y=hv(y), dq=hv((o["dqv"] * sc).sum(0)), dk=hv(o["dkv"].sum(0)),
               dv0=hv(o["dv0"] * vs0[None, :, None]), dvL=hv(o["dvL"] * vsL[None, :, None]),
               dvs0_bh=(o["dv0"] * hv(v0)).sum(2), dvsL_bh=(o["dvL"] * hv(vL)).sum(2),
               dsqk=(o["dqv"] * hv(q)[None]).sum((1, 3)) * dk_ ** 0.5, dchain_logit=np.asarray(o["dlogit"]), cache=cache)
    for n_ in (("dW1", "db1", "dW2", "db2") if dense else ("dWr", "dbr", "dWc", "dbc")):
        out[n_] = o[n_]
    return out


def _case_oracle(case, rnd=None):
    f = lambda t: t.numpy().astype(np.float64)
    o = core_oracle(f(case.q), f(case.k), f(case.v), f(case.v), f(case.dy), f(case.sqk), f(case.vs0), f(case.vsL), float(case.chain_logit),
                    tuple(map(f, case.head)), case.beta_not, case.dense, rnd)
    o["dv"] = o.pop("dv0") + o.pop("dvL")                                # share_qkv: one v tensor receives both value gradients
    o["dvs0"], o["dvsL"] = o.pop("dvs0_bh").sum(0), o.pop("dvsL_bh").sum(0)
    return o


def small_names(case):
    return ("dsqk", "dvs0", "dvsL", "dchain_logit") + case.head_names


@functools.lru_cache(maxsize=None)
def oracle_core(case):
    """float64 y and every gradient the core returns, by name: y, dq, dk, dv (B,N,H,dk); dsqk, dvs0, dvsL, dchain_logit and the head's;
    'cache' holds the oracle's intermediates (S, Smix, G, ...) for the tests that look at the inputs' conditioning"""
    return _case_oracle(case)


ROW_SITES = ("q",)
SMALL_SITES = ("q", "v", "A", "chain", "P", "logC")


def _rounding_noise(case, draws=8, sites=ROW_SITES):
    """The oracle re-run `draws` times with the intermediates named in `sites` rounded (draw 0: to nearest even; the others: stochastic
    rounding from a fixed generator).  Sites, each one the fused kernels' headers and DESIGN.md state: 'q' the scaled queries q * sqk_v
    and 'v' the scaled values v * vs0, v * vsL -- the per-dimension scales any bf16-MFMA implementation has to fold into an operand --
    'A' the per-view softmax pieces, 'chain' the chain products, 'P' the mixed softmax, all packed to bf16 as MFMA operands, and
    'logC' the chain logarithms, kept in fp16.
    Returns, for y / dq / dk / dv, the largest movement of each token row over the draws (max over dk; (B,N,H)), and for the small
    tensors the largest max-norm movement relative to max|exact| under 'bf16err:<name>', the form gpu_util.check_grads reads."""
    ref = oracle_core(case)
    rng = np.random.default_rng(1234)
    rows = {n_: np.zeros(ref[n_].shape[:3]) for n_ in ROW_TENSORS}
    small = {"bf16err:" + n_: 0.0 for n_ in small_names(case)}
    for i in range(draws):
        def rnd(site, a):
            if site not in sites:
                return a
            return (fp16_round if site == "logC" else bf16_round)(a, rng if i else None)
        o = _case_oracle(case, rnd)
        for n_ in ROW_TENSORS:
            rows[n_] = np.maximum(rows[n_], np.abs(o[n_] - ref[n_]).max(-1))
        for n_ in small_names(case):
            rel = float(np.abs(o[n_] - ref[n_]).max()) / max(float(np.abs(ref[n_]).max()), 1e-30)
            small["bf16err:" + n_] = max(small["bf16err:" + n_], rel)
    return dict(rows, **small)


rounding_noise = functools.lru_cache(maxsize=None)(_rounding_noise)


def small_noise(case, sites=SMALL_SITES):
    """the 'bf16err:<name>' record of the small-parameter gradients under all the rounding sites.  The rows of y / dq / dk / dv are
    judged on the 'q' site alone (the narrower model, so the harder bound; the kernels keep it).  The small gradients are sums of
    10^3 - 10^5 signed per-edge terms and move with every site: at (1, 33, 16, 2, 1), level 0.5, the exact dbc moves by 1 % under
    'q' alone and by several per cent once P and the chain products are rounded (DESIGN.md has the table)."""
    narrow, wide = rounding_noise(case), rounding_noise(case, 8, sites)
    return {k_: max(v_, narrow[k_]) for k_, v_ in wide.items() if k_.startswith("bf16err:")}        # more sites never narrow a limit


def row_bounds(ref, noise_rows, tol, bf16_io=False):
    """per token row: max(tol * max|ref|, 4 * the row's own movement), + half a bf16 ulp of max|ref| when the result is stored as bf16"""
    top = float(np.abs(ref).max())
    return np.maximum(tol * top, NOISE_FACTOR * noise_rows) + (2.0 ** -9 * top if bf16_io else 0.0)


def row_errors(got, ref):
    """largest |got - ref| of each token row: (B,N,H,dk) -> (B,N,H)"""
    return np.abs(np.asarray(got, np.float64) - ref).max(-1)


def tol_of(name):
    return TOL_BF16 if name == "y" else GTOL_BF16


def planted_identity(case):
    """y of the planted rows in exact arithmetic: each attends to itself alone in every view, so
    y[j] = v[j] vs0 + sigmoid(chain_logit) v[j] vsL.  (B, len(planted), H, dk) float64."""
    v = case.v.numpy().astype(np.float64)[:, list(planted_tokens(case.N))]
    w = 1.0 / (1.0 + math.exp(-float(case.chain_logit)))
    return v * case.vs0.numpy().astype(np.float64) + w * v * case.vsL.numpy().astype(np.float64)
