"""-m gpu: token-level timestamps on the HIP kernels (mopk_dtw_align, mopk_alignment_cost).  ops.dtw_align against
ops.dtw_align_torch on the same cost (equal: one identical fp32 add per cell) over the shapes of tests/test_whisper_align_cpu.py, the
wave boundary, one Whisper-sized map, a padded row stride, per-item lengths, row0 > 0, empty items, the planted staircase, NaN outside
the windows and two runs bit for bit; ops.alignment_cost against the float64 restatement of the CPU test with the fp32 torch
restatement's own error as the yardstick; and WhisperMoP.align_tokens: a valid path whose cost is the float64 optimum, a ragged batch
against each item alone, no host sync, the decoders untouched."""
import numpy as np
import pytest
import torch

from test_whisper_align_cpu import (COST_CASES, DTW_SHAPES, check_boundaries, cost_case, dtw_case, max_err, ref_cost64, ref_dtw_batch,
                                    staircase, window_mask)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the DTW kernel
def _dtw_both(cost, nr, nc, row0=0, what=None):
    """the kernel's result on device tensors, checked against the torch path on the same tensors -> (starts, ends)"""
    from mop_amd import _lib, ops
    rs, re = ops.dtw_align_torch(cost, nr, nc, row0)
    s, e = ops.dtw_align(cost, nr, nc, row0)
    assert ops.LAST_PATH["dtw_align"] == _lib.PATH_FUSED, what
    assert s.dtype == e.dtype == torch.int32 and s.shape == e.shape == cost.shape[:2]
    assert torch.equal(s, rs) and torch.equal(e, re), what
    return s, e


@pytest.mark.parametrize("N,M", DTW_SHAPES + [(63, 40), (64, 40), (65, 40)])
def test_dtw_kernel_equals_the_torch_path(N, M):
    for seed in range(2):
        cost, nr, nc = dtw_case(N, M, seed)
        s, e = _dtw_both(cost.cuda(), nr.cuda(), nc.cuda(), what=(N, M, seed))
        rs, re = ref_dtw_batch(cost, nr, nc, 0)                              # and the double loop of the CPU test
        assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(e.cpu().numpy(), re)


def test_dtw_kernel_at_whisper_size():
    cost, nr, nc = dtw_case(448, 1500, 5, B=2, n_rows=[448, 447], n_cols=[1500, 1333], row0=3)
    s, e = _dtw_both(cost.cuda(), nr.cuda(), nc.cuda(), 3)
    for b, (r1, c1) in enumerate(((448, 1500), (447, 1333))):
        check_boundaries(s[b].cpu(), e[b].cpu(), 3, r1, c1, b)


@pytest.mark.parametrize("row0", [0, 2])
def test_dtw_kernel_strides_lengths_and_empty_items(row0):
    from mop_amd import _lib, ops
    N, M = 70, 93
    n_rows, n_cols = [70, 5, 66, row0, 70, 99, -3], [93, 4, 64, 5, 0, 99, 4]
    cost, nr, nc = dtw_case(N, M, 7, B=7, n_rows=n_rows, n_cols=n_cols, row0=row0)
    s, e = _dtw_both(cost.cuda(), nr.cuda(), nc.cuda(), row0, "plain")
    rs, re = ref_dtw_batch(cost, nr, nc, row0)
    assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(e.cpu().numpy(), re)
    assert bool((s[3] == -1).all()) and bool((s[4] == -1).all()) and bool((e[6] == -1).all()) and bool((s[:, :row0] == -1).all())
    # a padded row stride and a padded item stride, NaN in the padding
    wide = torch.full((7, N + 2, M + 5), float("nan"), device="cuda")
    wide[:, :N, :M] = cost.cuda()
    view = wide[:, :N, :M]
    assert view.stride() == ((N + 2) * (M + 5), M + 5, 1)
    s2, e2 = _dtw_both(view, nr.cuda(), nc.cuda(), row0, "strided")
    assert torch.equal(s2, s) and torch.equal(e2, e)
    # two runs bit for bit
    s3, e3 = ops.dtw_align(view, nr.cuda(), nc.cuda(), row0)
    assert ops.LAST_PATH["dtw_align"] == _lib.PATH_FUSED and torch.equal(s3, s) and torch.equal(e3, e)


def test_dtw_kernel_single_row_and_single_item_strides():
    """N == 1: the row stride is never used, B == 1: the item stride is never used; values the kernel would refuse (a row stride
    below M) or misread (an item stride of 0) for more rows / items pass"""
    from mop_amd import ops
    cost, nr, nc = dtw_case(1, 7, 3, B=2, n_cols=[7, 5])
    view = cost.cuda().as_strided((2, 1, 7), (7, 1, 1))
    s, e = _dtw_both(view, nr.cuda(), nc.cuda(), what="N == 1, row stride 1")
    print(f"dtw N == 1, row stride 1: path {ops.LAST_PATH['dtw_align']}")
    assert s.tolist() == [[0], [0]] and e.tolist() == [[6], [4]]
    cost, nr, nc = dtw_case(3, 7, 4, n_rows=[3], n_cols=[6])
    view = cost.cuda().as_strided((1, 3, 7), (0, 7, 1))
    s, e = _dtw_both(view, nr.cuda(), nc.cuda(), what="B == 1, item stride 0")
    print(f"dtw B == 1, item stride 0: path {ops.LAST_PATH['dtw_align']}")
    check_boundaries(s[0].cpu(), e[0].cpu(), 0, 3, 6)


@pytest.mark.parametrize("N,M", [(6, 9), (9, 6), (40, 70), (130, 200)])
def test_dtw_kernel_finds_the_planted_staircase(N, M):
    cost, starts, ends = staircase(N, M, N + M)
    full = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")      # noqa: E731
    s, e = _dtw_both(cost.cuda(), full(N), full(M))
    assert np.array_equal(s[0].cpu().numpy(), starts) and np.array_equal(e[0].cpu().numpy(), ends)


def test_dtw_above_the_kernel_limit_takes_the_torch_path():
    from mop_amd import _lib, ops
    cost, nr, nc = dtw_case(1030, 3, 1)
    assert not ops.dtw_align_supported(cost.cuda(), nr.cuda(), nc.cuda(), 5)
    assert ops.dtw_align_supported(cost.cuda(), nr.cuda(), nc.cuda(), 6)      # 1024 rows from row0 on
    s, e = _dtw_both(cost.cuda(), nr.cuda(), nc.cuda(), 6)
    check_boundaries(s[0].cpu(), e[0].cpu(), 6, 1030, 3)
    ops.dtw_align(cost.cuda(), nr.cuda(), nc.cuda(), 5)
    assert ops.LAST_PATH["dtw_align"] == _lib.PATH_GENERIC


# ---------------------------------------------------------------- the filter kernel
def _cost_both(probs, nt, nf, width, what):
    """the kernel against float64 with the torch restatement's own error as the yardstick -> (cost, E32, the kernel's error)"""
    from mop_amd import _lib, ops
    ref = ref_cost64(probs.cpu(), nt.cpu(), nf.cpu(), width)
    e32 = max_err(ops.alignment_cost_torch(probs, nt, nf, width), ref)
    got = ops.alignment_cost(probs, nt, nf, width)
    assert ops.LAST_PATH["alignment_cost"] == _lib.PATH_FUSED, what
    assert got.shape == (probs.shape[0],) + probs.shape[2:] and got.dtype == torch.float32
    err = max_err(got, ref)
    bound = 4 * e32 + 8 * 2.0 ** -23 * float(np.nanmax(np.abs(ref)))
    print(f"alignment_cost {what}: E32 = {e32:.3e}, kernel error = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound, what
    return got, e32, err


def _inside(got, nt, nf):
    B, N, M = got.shape
    return got.view(torch.int32)[window_mask(B, N, M, nt.cpu(), nf.cpu()).cuda()]


@pytest.mark.parametrize("S,width", [(S, w) for S in (1, 3) for w in (1, 3, 7)])
def test_cost_kernel_over_the_cpu_sweep(S, width):
    for s_, w_, nt, nf in COST_CASES:
        if (s_, w_) == (S, width):
            N, M = nt + 3, nf + 5
            probs, n_tokens, n_frames = cost_case(S, N, M, [nt, max(nt - 1, 2), N], [nf, max(nf - 1, 1), M], 100 * nt + nf, "cuda")
            _cost_both(probs, n_tokens, n_frames, width, (S, width, nt, nf))


@pytest.mark.parametrize("N,M,width", [(5, 127, 7), (5, 128, 7), (5, 129, 7), (7, 193, 5), (7, 131, 9), (450, 33, 7), (449, 31, 7),
                                       (897, 17, 7), (1024, 15, 9)])
def test_cost_kernel_tiles_widths_and_row_counts(N, M, width):
    """the column tile is 64 wide up to 448 rows, 32 up to 896 and 16 up to 1024: M straddles it by one, and N every threshold"""
    tile = 64 if N <= 448 else 32 if N <= 896 else 16
    probs, nt, nf = cost_case(2, N, M, [N, N - 1, 3], [M, tile + 1, tile - 1], N + M, "cuda")
    got, _, _ = _cost_both(probs, nt, nf, width, (N, M, width))
    from mop_amd import ops
    again = ops.alignment_cost(probs, nt, nf, width)                         # two runs bit for bit
    assert torch.equal(_inside(got, nt, nf), _inside(again, nt, nf))


def test_cost_kernel_strided_probs():
    from mop_amd import _lib, ops
    S, N, M = 3, 40, 150
    probs, nt, nf = cost_case(S, N, M, [40, 17], [150, 65], 9, "cuda")
    plain, _, _ = _cost_both(probs, nt, nf, 7, "plain")
    big = torch.full((2, S + 1, N + 2, M + 3), float("nan"), device="cuda")  # padded in every dimension
    big[:, :S, :N, :M] = probs
    got, _, _ = _cost_both(big[:, :S, :N, :M], nt, nf, 7, "padded")
    assert torch.equal(_inside(got, nt, nf), _inside(plain, nt, nf))
    heads_first = probs.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)  # (S, B, N, M) memory
    assert not heads_first.is_contiguous()
    got, _, _ = _cost_both(heads_first, nt, nf, 7, "heads first")
    assert torch.equal(_inside(got, nt, nf), _inside(plain, nt, nf))
    # above the kernel's limits: the torch path
    ops.alignment_cost(probs, nt, nf, 11)
    assert ops.LAST_PATH["alignment_cost"] == _lib.PATH_GENERIC


# ---------------------------------------------------------------- the model
def _model(d=128, H=2, Ta=200, vocab=300, ctx=64, L=2):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=Ta, vocab_size=vocab, n_text_ctx=ctx, n_embd=d, n_head=H, n_layer_enc=1, n_layer_dec=L)
    m = WhisperMoP(cfg)
    with torch.no_grad():
        # at the default init the cross-attention logits have a deviation of ~0.05: every map is flat, a column's mean is hundreds
        # of times its deviation, and z = (p - mu) / sd multiplies the fp32 noise of everything upstream by that ratio.  A trained
        # model's maps are peaked; widen the logits 64-fold (deviation ~3) so that the maps under test are, too
        for blk in m.decoder:
            blk.cross_attn.q_proj.weight.mul_(8.0)
            blk.cross_attn.k_proj.weight.mul_(8.0)
    return m.cuda().eval()


def _optimum64(x):
    """the least cost of a monotone path from the first to the last cell, in float64"""
    R, Cn = x.shape
    D = np.full((R + 1, Cn + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(1, R + 1):
        for j in range(1, Cn + 1):
            D[i, j] = x[i - 1, j - 1] + min(D[i - 1, j - 1], D[i - 1, j], D[i, j - 1])
    return D[R, Cn]


def _path_cost(cost, starts, ends, r0, r1):
    x = cost.double().cpu().numpy()
    return sum(x[i, starts[i]:ends[i] + 1].sum() for i in range(r0, r1))


def _check_item(cost, starts, ends, P, n_tok, n_frames, what):
    """a valid path over rows [P, n_tok - 1) whose cost is the float64 optimum within (N + M) 2^-23 max|cost| -> (its cost, that
    tolerance).  N and M are the dimensions of the item's returned cost matrix, as the formula is stated for `cost (B, N, M)`, and
    max|cost| is taken over the warped window.  Observed on an MI355X: every path cost equals the float64 optimum to the printed
    six decimals.  The batch-against-alone differences come from upstream of the two ops (the padded batch runs the encoder's
    length-aware attention and GEMMs of other row counts, which round in another order): 1.1e-5, 4e-6 and 8.7e-6 for the three
    items, against 2.5e-5, 2.4e-5 and 1.8e-5 allowed; with the window's own row and column counts in place of N + M the third
    item's allowance would be 4.8e-6 and it would miss it."""
    s, e = starts.cpu().numpy(), ends.cpu().numpy()
    check_boundaries(s, e, P, n_tok - 1, n_frames, what)
    window = cost[P:n_tok - 1, :n_frames].double().cpu().numpy()
    got, best = _path_cost(cost, s, e, P, n_tok - 1), _optimum64(window)
    tol = (cost.shape[0] + cost.shape[1]) * 2.0 ** -23 * np.abs(window).max()
    print(f"align_tokens {what}: path cost {got:.6f}, float64 optimum {best:.6f}, tolerance {tol:.2e}")
    assert abs(got - best) <= tol, what
    return got, tol


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])
def test_align_tokens_path_is_valid_and_optimal(mode):
    from mop_amd import _lib, ops
    m = _model()
    torch.manual_seed(4)
    mel = torch.randn(2, 200, 12, device="cuda")
    tokens = torch.randint(0, 300, (2, 30), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
        a, cost = m.align_tokens(mel, tokens, 4, return_cost=True)
    assert ops.LAST_PATH["alignment_cost"] == _lib.PATH_FUSED and ops.LAST_PATH["dtw_align"] == _lib.PATH_FUSED
    assert a.n_tokens.tolist() == [30, 30] and cost.shape == (2, 30, 200)
    for b in range(2):
        _check_item(cost[b], a.starts[b], a.ends[b], 4, 30, 200, (mode, b))


def test_align_tokens_ragged_batch_against_each_item_alone():
    m = _model()
    torch.manual_seed(5)
    mel = torch.randn(3, 200, 12, device="cuda")
    tokens = torch.randint(0, 300, (3, 30), device="cuda")
    clips, seqs = [mel[0], mel[1, :131], mel[2, :57]], [tokens[0, :19], tokens[1], tokens[2, :8]]
    heads = [(1, 1), (0, 0), (1, 0)]
    a, cost = m.align_tokens(clips, seqs, 3, alignment_heads=heads, return_cost=True)
    for b in range(3):
        n, nf = len(seqs[b]), clips[b].shape[0]
        got, tol = _check_item(cost[b], a.starts[b], a.ends[b], 3, n, nf, ("batch", b))
        one, cost1 = m.align_tokens(clips[b].unsqueeze(0), seqs[b].unsqueeze(0), 3, alignment_heads=heads, return_cost=True)
        alone, tol1 = _check_item(cost1[0], one.starts[0], one.ends[0], 3, n, nf, ("alone", b))
        assert abs(got - alone) <= max(tol, tol1), b


def test_align_tokens_makes_no_host_sync_and_leaves_the_decoders_alone():
    m = _model()
    torch.manual_seed(6)
    mel = torch.randn(2, 200, 12, device="cuda")
    tokens = torch.randint(0, 300, (2, 30), device="cuda")
    prompt = tokens[:, :4].contiguous()
    before = (m.generate(mel, prompt, 12), m.beam_search(mel, prompt, 12, 3), m.sample(mel, prompt, 12, 0.8, 10, seed=4))
    clips, seqs = [mel[0], mel[1, :131]], [tokens[0], tokens[1, :11]]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            a = m.align_tokens(mel, tokens, 4)
            r = m.align_tokens(clips, seqs, 4, medfilt_width=5)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert a.starts.shape == (2, 30) and r.n_tokens.tolist() == [30, 11]
    check_boundaries(r.starts[1].cpu(), r.ends[1].cpu(), 4, 10, 131)
    after = (m.generate(mel, prompt, 12), m.beam_search(mel, prompt, 12, 3), m.sample(mel, prompt, 12, 0.8, 10, seed=4))
    assert torch.equal(before[0], after[0])
    for x, y in zip(before[1] + before[2], after[1] + after[2]):
        assert torch.equal(x, y)
