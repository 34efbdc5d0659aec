"""CPU checks of token-level timestamps (no GPU): ops.dtw_align_torch against a per-item double loop written here (Whisper's dtw_cpu
rules in numpy float32, no call into ops; starts / ends must be equal) and on a planted staircase whose optimum is unique;
ops.alignment_cost_torch against a float64 per-item restatement written here (numpy.median over an explicitly reflect-padded row);
every ValueError; the support and workspace queries without a GPU; and
WhisperMoP.align_tokens with every core on its torch composition."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _tiny_model

NAN = float("nan")
DTW_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 5), (7, 3), (65, 130)]          # (N, M); (7, 3): more tokens than frames


# ---------------------------------------------------------------- the restatements
def ref_dtw(x):
    """Whisper's dtw_cpu and backtrace on one (R, C) float32 array -> (starts, ends) per row"""
    x = np.asarray(x, dtype=np.float32)
    R, Cn = x.shape
    D = np.full((R + 1, Cn + 1), np.inf, dtype=np.float32)
    tr = -np.ones((R + 1, Cn + 1), dtype=np.int64)
    D[0, 0] = 0
    for j in range(1, Cn + 1):
        for i in range(1, R + 1):
            c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            D[i, j] = np.float32(x[i - 1, j - 1] + c)
            tr[i, j] = t
    i, j = R, Cn
    tr[0, :] = 2
    tr[:, 0] = 1
    cells = []
    while i > 0 or j > 0:
        cells.append((i - 1, j - 1))
        if tr[i, j] == 0:
            i, j = i - 1, j - 1
        elif tr[i, j] == 1:
            i -= 1
        else:
            j -= 1
    starts, ends = np.full(R, 10 ** 9), np.full(R, -1)
    for i, j in cells:
        assert i >= 0 and j >= 0
        starts[i], ends[i] = min(starts[i], j), max(ends[i], j)
    return starts, ends


def ref_dtw_batch(cost, n_rows, n_cols, row0):
    B, N, M = cost.shape
    S, E = -np.ones((B, N), dtype=np.int64), -np.ones((B, N), dtype=np.int64)
    for b in range(B):
        r1, c1 = min(max(int(n_rows[b]), 0), N), min(max(int(n_cols[b]), 0), M)
        if r1 > row0 and c1 > 0:
            S[b, row0:r1], E[b, row0:r1] = ref_dtw(cost[b, row0:r1, :c1].numpy())
    return S, E


def ref_cost64(probs, n_tokens, n_frames, width):
    """the issue's semantics in float64, item by item -> (B, N, M) float64, NaN outside the windows"""
    B, S, N, M = probs.shape
    out = np.full((B, N, M), np.nan)
    h = width // 2
    for b in range(B):
        nt, nf = min(max(int(n_tokens[b]), 0), N), min(max(int(n_frames[b]), 0), M)
        if nt == 0 or nf == 0:
            continue
        total = np.zeros((nt, nf))
        for s in range(S):
            p = probs[b, s, :nt, :nf].double().numpy()
            z = (p - p.mean(0, keepdims=True)) / p.std(0, keepdims=True)           # population: numpy's ddof = 0
            if nf > h and h > 0:
                f = np.empty_like(z)
                for i in range(nt):
                    row = np.concatenate([z[i, 1:h + 1][::-1], z[i], z[i, nf - 1 - h:nf - 1][::-1]])    # reflect, edge not repeated
                    for j in range(nf):
                        f[i, j] = np.median(row[j:j + width])
                z = f
            total += z
        out[b, :nt, :nf] = -(total / S)
    return out


def cost_scale(probs, n_tokens, n_frames):
    """what an fp32 rounding error is multiplied by on its way into z = (p - mu) / sd, in float64: the largest |mu| / sd of a
    column (the error of mu, relative to sd) plus the largest |z| (the relative errors of the subtraction, of sd and of the
    division)"""
    B, S, N, M = probs.shape
    worst = 0.0
    for b in range(B):
        nt, nf = min(max(int(n_tokens[b]), 0), N), min(max(int(n_frames[b]), 0), M)
        if nt and nf:
            p = probs[b, :, :nt, :nf].double().numpy()
            mu, sd = p.mean(1, keepdims=True), p.std(1, keepdims=True)
            worst = max(worst, float((np.abs(mu) / sd).max() + np.abs((p - mu) / sd).max()))
    return worst


def window_mask(B, N, M, n_rows, n_cols, row0=0):
    m = torch.zeros(B, N, M, dtype=torch.bool)
    for b in range(B):
        m[b, row0:min(max(int(n_rows[b]), 0), N), :min(max(int(n_cols[b]), 0), M)] = True
    return m


def dtw_case(N, M, seed, B=1, n_rows=None, n_cols=None, row0=0):
    """random costs, NaN outside every item's window -> (cost, n_rows, n_cols)"""
    g = torch.Generator().manual_seed(seed)
    cost = torch.randn(B, N, M, generator=g)
    n_rows = torch.tensor([N] * B if n_rows is None else n_rows, dtype=torch.int32)
    n_cols = torch.tensor([M] * B if n_cols is None else n_cols, dtype=torch.int32)
    cost[~window_mask(B, N, M, n_rows, n_cols, row0)] = NAN
    return cost, n_rows, n_cols


def staircase(N, M, seed):
    """cost 1 everywhere, 0 on a monotone staircase from (0, 0) to (N - 1, M - 1) with diagonal, vertical and horizontal steps
    -> (cost (1, N, M), starts, ends).  A vertical step never touches a horizontal one (a diagonal would cut that corner at the same
    cost), so the staircase is the only path of cost 0: the unique optimum, whatever the tie rules are"""
    rng = np.random.default_rng(seed)
    while True:
        i = j = 0
        cells, kinds, last = [(0, 0)], set(), None
        while (i, j) != (N - 1, M - 1):
            moves = [m for m in ((1, 1), (1, 0), (0, 1)) if i + m[0] < N and j + m[1] < M and {m, last} != {(1, 0), (0, 1)}]
            if not moves:
                break
            last = moves[rng.integers(len(moves))]
            kinds.add(last)
            i, j = i + last[0], j + last[1]
            cells.append((i, j))
        if (i, j) == (N - 1, M - 1) and {(1, 1), (1, 0)} <= kinds:
            break
    cost = torch.ones(1, N, M)
    starts, ends = np.full(N, 10 ** 9), np.full(N, -1)
    for i, j in cells:
        cost[0, i, j] = 0.0
        starts[i], ends[i] = min(starts[i], j), max(ends[i], j)
    return cost, starts, ends


def cost_case(S, N, M, n_tokens, n_frames, seed, device="cpu"):
    """softmax rows as probabilities, NaN outside every item's window -> (probs (B, S, N, M), n_tokens, n_frames)"""
    B = len(n_tokens)
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(2.0 * torch.randn(B, S, N, M, generator=g), dim=-1)
    nt, nf = torch.tensor(n_tokens, dtype=torch.int32), torch.tensor(n_frames, dtype=torch.int32)
    probs[~window_mask(B, N, M, nt, nf).unsqueeze(1).expand(B, S, N, M)] = NAN
    return probs.to(device), nt.to(device), nf.to(device)


COST_CASES = [(S, w, nt, nf) for S in (1, 3) for w in (1, 3, 7) for nt in (2, 5, 65) for nf in (2, 3, 4, 63, 64, 65)]


def max_err(got, ref64):
    """largest absolute error inside the windows (where ref64 is not NaN); every value there must be finite"""
    inside = ~np.isnan(ref64)
    g = got.double().cpu().numpy()[inside]
    assert np.isfinite(g).all()
    return float(np.abs(g - ref64[inside]).max()) if inside.any() else 0.0


# ---------------------------------------------------------------- dtw_align_torch
@pytest.mark.parametrize("N,M", DTW_SHAPES)
def test_dtw_torch_equals_the_double_loop(N, M):
    from mop_amd import ops
    for seed in range(3):
        cost, nr, nc = dtw_case(N, M, seed)
        s, e = ops.dtw_align_torch(cost, nr, nc)
        rs, re = ref_dtw_batch(cost, nr, nc, 0)
        assert s.dtype == e.dtype == torch.int32 and s.shape == e.shape == (1, N)
        assert np.array_equal(s.numpy(), rs) and np.array_equal(e.numpy(), re)
        assert rs[0, 0] == 0 and re[0, -1] == M - 1


@pytest.mark.parametrize("row0", [0, 2])
def test_dtw_torch_batch_with_per_item_lengths(row0):
    from mop_amd import ops
    N, M = 12, 17
    cost, nr, nc = dtw_case(N, M, 7, B=3, n_rows=[12, 5, 9], n_cols=[17, 4, 11], row0=row0)
    s, e = ops.dtw_align_torch(cost, nr, nc, row0)
    rs, re = ref_dtw_batch(cost, nr, nc, row0)
    assert np.array_equal(s.numpy(), rs) and np.array_equal(e.numpy(), re)
    assert (s[:, :row0] == -1).all() and (s[1, 5:] == -1).all() and (e[2, 9:] == -1).all()
    # empty items, lengths past the shape (clamped) and negative ones
    cost, nr, nc = dtw_case(N, M, 8, B=4, n_rows=[row0, 12, 99, -3], n_cols=[5, 0, 99, 4], row0=row0)
    s, e = ops.dtw_align_torch(cost, nr, nc, row0)
    rs, re = ref_dtw_batch(cost, nr, nc, row0)
    assert np.array_equal(s.numpy(), rs) and np.array_equal(e.numpy(), re)
    assert (s[0] == -1).all() and (s[1] == -1).all() and (s[3] == -1).all() and s[2, row0] == 0 and e[2, N - 1] == M - 1


@pytest.mark.parametrize("N,M", [(6, 9), (9, 6), (40, 70)])
def test_dtw_torch_finds_the_planted_staircase(N, M):
    from mop_amd import ops
    cost, starts, ends = staircase(N, M, N + M)
    full = lambda v: torch.tensor([v], dtype=torch.int32)                  # noqa: E731
    s, e = ops.dtw_align_torch(cost, full(N), full(M))
    assert np.array_equal(s[0].numpy(), starts) and np.array_equal(e[0].numpy(), ends)


# ---------------------------------------------------------------- alignment_cost_torch
@pytest.mark.parametrize("S,width,nt,nf", COST_CASES)
def test_cost_torch_against_float64(S, width, nt, nf):
    from mop_amd import ops
    # three items: the case's window, a smaller one and the whole padded map
    N, M = nt + 3, nf + 5
    probs, n_tokens, n_frames = cost_case(S, N, M, [nt, max(nt - 1, 2), N], [nf, max(nf - 1, 1), M], 100 * nt + nf)
    got = ops.alignment_cost_torch(probs, n_tokens, n_frames, width)
    ref = ref_cost64(probs, n_tokens, n_frames, width)
    assert got.shape == (3, N, M) and got.dtype == torch.float32
    # fp32 against float64: mu and sd are sums of nt <= 68 terms, each within log2(68) + 2 < 8 roundings of 2^-24 whatever the
    # summation order is pairwise or within 68 / 2 on average when it is sequential; cost_scale carries them into z, and the
    # median, the mean over S <= 3 heads and the negation add at most 4 roundings of |z|: 8 * 2^-23 * cost_scale covers both
    assert max_err(got, ref) <= 8 * 2.0 ** -23 * cost_scale(probs, n_tokens, n_frames)


def test_cost_torch_skips_the_filter_on_narrow_maps():
    from mop_amd import ops
    probs, nt, nf = cost_case(2, 5, 9, [5, 5], [3, 4], 3)
    w7, w1 = ops.alignment_cost_torch(probs, nt, nf, 7), ops.alignment_cost_torch(probs, nt, nf, 1)
    assert torch.equal(w7[0, :, :3], w1[0, :, :3])                          # 3 <= 7 // 2: no filter
    assert not torch.equal(w7[1, :, :4], w1[1, :, :4])


# ---------------------------------------------------------------- errors, layouts, queries
def test_value_errors():
    from mop_amd import ops
    p, i32 = torch.rand(2, 3, 4, 5), lambda *v: torch.tensor(v, dtype=torch.int32)       # noqa: E731
    nt, nf = i32(4, 4), i32(5, 5)
    for f in (ops.alignment_cost, ops.alignment_cost_torch, ops.alignment_cost_supported):
        for bad in (lambda: f(p[0], nt, nf), lambda: f(p.double(), nt, nf), lambda: f(p.transpose(2, 3), nt, nf),
                    lambda: f(p, nt, nf, 4), lambda: f(p, nt, nf, 0), lambda: f(p, nt, nf, 3.5), lambda: f(p, i32(4), nf),
                    lambda: f(p, nt, nf.float()), lambda: f(p, nt, [5, 5]), lambda: f(p[:, :0], nt, nf)):
            with pytest.raises(ValueError):
                bad()
    c = torch.rand(2, 4, 5)
    for f in (ops.dtw_align, ops.dtw_align_torch, ops.dtw_align_supported):
        for bad in (lambda: f(c[0], nt, nf), lambda: f(c.double(), nt, nf), lambda: f(c.transpose(1, 2), nf, nt),
                    lambda: f(c, nt, nf, 4), lambda: f(c, nt, nf, -1), lambda: f(c, nt, nf, 1.5), lambda: f(c, i32(4, 4, 4), nf),
                    lambda: f(c, nt.float(), nf), lambda: f(c, nt, None)):
            with pytest.raises(ValueError):
                bad()


def test_support_and_workspace_queries_need_no_gpu():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib, ops
    lib = _lib.lib()
    assert lib.mopk_version() == 118
    a = _lib.AlignCostArgs()
    a.B, a.S, a.N, a.M, a.width = 2, 3, 448, 1500, 7
    a.probs_sb, a.probs_ss, a.probs_sn, a.cost_sb, a.cost_ld = 3 * 448 * 1500, 448 * 1500, 1500, 448 * 1500, 1500
    assert lib.mopk_alignment_cost_supported(C.byref(a)) == 1
    for field, v in (("N", 1025), ("width", 11), ("width", 4), ("width", 0), ("S", 0), ("cost_ld", 1499), ("probs", 2)):
        keep = getattr(a, field)
        setattr(a, field, v)
        assert lib.mopk_alignment_cost_supported(C.byref(a)) == 0, field
        assert lib.mopk_alignment_cost(C.byref(a), None) < 0, field
        setattr(a, field, keep)
    a.N, a.width = 1024, 9
    assert lib.mopk_alignment_cost_supported(C.byref(a)) == 1
    assert lib.mopk_alignment_cost(C.byref(a), None) == -2                  # null pointers: refused before any launch
    d = _lib.DtwArgs()
    d.B, d.N, d.M, d.row0, d.cost_sb, d.cost_ld = 3, 448, 1500, 4, 448 * 1500, 1500
    assert lib.mopk_dtw_align_supported(C.byref(d)) == 1
    assert lib.mopk_dtw_workspace_bytes(C.byref(d)) == 3 * 444 * 1500 == ops.dtw_workspace_bytes(3, 448, 1500, 4)
    for field, v in (("N", 1029), ("row0", -1), ("row0", 448), ("cost_ld", 1499), ("M", 0), ("n_rows", 2)):
        keep = getattr(d, field)
        setattr(d, field, v)
        assert lib.mopk_dtw_align_supported(C.byref(d)) == 0, field
        assert lib.mopk_dtw_align(C.byref(d), None) < 0, field
        setattr(d, field, keep)
    d.N = 1028                                                              # 1024 rows from row0 on
    assert lib.mopk_dtw_align_supported(C.byref(d)) == 1
    assert lib.mopk_dtw_align(C.byref(d), None) == -2
    # CPU tensors take the torch path
    p, nt, nf = cost_case(1, 4, 6, [4], [6], 0)
    assert not ops.alignment_cost_supported(p, nt, nf) and not ops.dtw_align_supported(p[0], nt, nf)
    cost = ops.alignment_cost(p, nt, nf, 3)
    assert ops.LAST_PATH["alignment_cost"] == _lib.PATH_GENERIC
    ops.dtw_align(cost, nt, nf)
    assert ops.LAST_PATH["dtw_align"] == _lib.PATH_GENERIC


# ---------------------------------------------------------------- the model
def check_boundaries(starts, ends, r0, r1, n_frames, what=None):
    """rows [r0, r1) hold a monotone, contiguous path over the frames [0, n_frames); every other row holds -1"""
    s, e = np.asarray(starts), np.asarray(ends)
    assert (s[:r0] == -1).all() and (e[:r0] == -1).all() and (s[r1:] == -1).all() and (e[r1:] == -1).all(), what
    assert s[r0] == 0 and e[r1 - 1] == n_frames - 1, what
    assert (s[r0:r1] <= e[r0:r1]).all(), what
    step = s[r0 + 1:r1] - e[r0:r1 - 1]
    assert ((step == 0) | (step == 1)).all(), what


def test_align_tokens_on_the_torch_path(torch_cores):                       # noqa: F811
    from mop_amd.nn import TokenAlignment
    m = _tiny_model()
    torch.manual_seed(3)
    mel = torch.randn(2, 40, 10)
    tokens = torch.randint(0, 100, (2, 12))
    a = m.align_tokens(mel, tokens, 3)
    assert isinstance(a, TokenAlignment) and a.starts.shape == a.ends.shape == (2, 12) and a.starts.dtype == torch.int32
    assert a.n_tokens.tolist() == [12, 12]
    for b in range(2):
        check_boundaries(a.starts[b], a.ends[b], 3, 11, 40, b)
    # lists: clips and token sequences of different lengths; each item as it is alone
    clips, seqs = [mel[0], mel[1, :23]], [tokens[0], tokens[1, :7]]
    r, cost = m.align_tokens(clips, seqs, 3, alignment_heads=[(1, 0), (0, 1)], medfilt_width=3, return_cost=True)
    assert r.n_tokens.tolist() == [12, 7] and cost.shape == (2, 12, 40)
    check_boundaries(r.starts[0], r.ends[0], 3, 11, 40)
    check_boundaries(r.starts[1], r.ends[1], 3, 6, 23)
    for b in range(2):
        alone = m.align_tokens(clips[b].unsqueeze(0), seqs[b].unsqueeze(0), 3, alignment_heads=[(1, 0), (0, 1)], medfilt_width=3)
        n = len(seqs[b])
        assert torch.equal(alone.starts[0], r.starts[b, :n]) and torch.equal(alone.ends[0], r.ends[b, :n])


def test_align_tokens_value_errors(torch_cores):                            # noqa: F811
    m = _tiny_model()
    mel, tokens = torch.randn(2, 40, 10), torch.randint(0, 100, (2, 12))
    for bad in (lambda: m.align_tokens(mel, tokens[:1], 3), lambda: m.align_tokens(mel, tokens.float(), 3),
                lambda: m.align_tokens(mel, tokens, -1), lambda: m.align_tokens(mel, tokens, 11), lambda: m.align_tokens(mel, tokens, 2.0),
                lambda: m.align_tokens(mel, [tokens[0], tokens[1, :4]], 3), lambda: m.align_tokens(mel, tokens, 3, medfilt_width=4),
                lambda: m.align_tokens(mel, tokens, 3, alignment_heads=[]), lambda: m.align_tokens(mel, tokens, 3, alignment_heads=[(2, 0)]),
                lambda: m.align_tokens(mel, tokens, 3, alignment_heads=[(0, 2)]), lambda: m.align_tokens(mel, torch.zeros(2, 65, dtype=torch.long), 3),
                lambda: m.align_tokens([mel[0]], tokens, 3)):
        with pytest.raises(ValueError):
            bad()
