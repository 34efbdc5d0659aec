"""GPU checks of word timestamps: the mopk_alignment_rows and mopk_word_spans kernels against the torch path on the same device
tensors and against the Python-list restatements of tests/test_whisper_words_cpu.py (the hand-built rows and the sweep over N,
n_text, padded row strides and ids outside the table; sentinels around the outputs; what the kernels do not take; bitwise
repeatability; no host sync; graph capture in a process of its own), WhisperMoP.align_words against align_tokens plus the
restatement, and transcribe(word_timestamps=True) on the device against the naive host loop: greedy, a fallback run with a
skipped window, and condition_on_previous_text=True."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_whisper_align import _model as _align_model
from test_gpu_whisper_fallback import _model
from test_whisper_transcribe_cpu import EOS, RULES, V
from test_whisper_words_cpu import (NOTS, SWEEP_N, check_align_words, check_greedy_word_case, check_policy_word_cases, check_rows,
                                    check_spans, decoded_rows, hand_cases, random_rows, table_rules,
                                    word_rules_by_residue)

pytestmark = pytest.mark.gpu


def _fused(ops, key, what):
    from mop_amd import _lib
    assert ops.LAST_PATH.pop(key) == _lib.PATH_FUSED, (key, what)


def _same(x, y):
    return all(torch.equal(p, q) for p, q in zip(x, y))


def _spans_both(ops, tokens, times, probs, n_text, rules, cap, what, pad=0):
    """the kernel against the restatement, the torch path on device tensors against it, the integers of the two equal, and a
    second run of the kernel bit for bit"""
    ops.LAST_PATH.pop("word_spans", None)
    got = check_spans(ops.word_spans, tokens, times, probs, n_text, rules, cap, what, device="cuda", pad=pad)
    _fused(ops, "word_spans", what)
    ref = check_spans(ops.word_spans_torch, tokens, times, probs, n_text, rules, cap, what, device="cuda", pad=pad)
    assert all(torch.equal(getattr(got, f), getattr(ref, f)) for f in ("starts", "ends", "tok_begin", "tok_end", "n_words")), what
    again = check_spans(ops.word_spans, tokens, times, probs, n_text, rules, cap, what, device="cuda", pad=pad)
    assert _same(got, again), what
    return got


def _rows_both(ops, rows, t0, take, sot, dtype, what, **kw):
    ops.LAST_PATH.pop("alignment_rows", None)
    got = check_rows(ops.alignment_rows, rows, t0, take, sot, NOTS, EOS, dtype, what, device="cuda", **kw)
    _fused(ops, "alignment_rows", what)
    ref = check_rows(ops.alignment_rows_torch, rows, t0, take, sot, NOTS, EOS, dtype, what, device="cuda", **kw)
    again = check_rows(ops.alignment_rows, rows, t0, take, sot, NOTS, EOS, dtype, what, device="cuda", **kw)
    assert _same(got, ref) and _same(got, again), what
    return got


def test_hand_built_rows():
    from mop_amd import ops
    rules = table_rules(device="cuda")
    for name, tokens, times, n, cap, want in hand_cases():
        probs = [((7 * i + 3) % 10) / 10 for i in range(len(tokens))]
        for pad in (0, 3):
            got = _spans_both(ops, [tokens], [times], [probs], [n], rules, cap, name, pad=pad)
        if want is not None:
            k = int(got.n_words[0])
            assert list(zip(got.starts[0, :k].tolist(), got.ends[0, :k].tolist(), got.tok_begin[0, :k].tolist(),
                            got.tok_end[0, :k].tolist())) == want, name
    rows = [[7, 8, 9, 101, 5, 6, 103, 103, 11, EOS, EOS], [7, 8, 9, 101, 102, EOS, 4, 4, 4, 4, 4], [7, 8, 9, 1, 2, 3, 4, 5, 6, 7, 8]]
    for dt in (torch.int64, torch.int32):
        got = _rows_both(ops, rows, 3, [6, 2, 8], [7, 8, 9], dt, "by hand")
        assert got.n_tokens.tolist() == [8, 5, 13]


@pytest.mark.parametrize("N", SWEEP_N)
def test_kernels_match_the_torch_path_and_the_restatement(N):
    from mop_amd import ops
    rules = table_rules(device="cuda")
    R = 6 if N >= 448 else 24
    for seed, cap, pad in ((0, None, 0), (1, 1, 3), (2, 70, 0)):
        tokens, times, probs, n_text = random_rows(N, R, 1000 * N + seed)
        _spans_both(ops, tokens, times, probs, n_text, rules, cap, (N, seed), pad=pad)
    for t0, R, pad, dt in ((0, 3, 0, torch.int32), (3, 5, 2, torch.int64)):
        rows, take = decoded_rows(R, t0 + N, t0, N + t0)
        sot = [7, 8, 9] if t0 else [[r, r + 1] for r in range(R)]
        _rows_both(ops, rows, t0, take, sot, dt, (N, t0), pad=pad, sot_dtype=(torch.int64, torch.int32)[N % 2])


def test_sentinels_around_the_outputs():
    """both kernels launched through the library on output buffers with guard words on both sides"""
    from mop_amd import _lib, ops
    R, N = 5, 130
    rules = table_rules(device="cuda")
    tokens, times, probs, n_text = random_rows(N, R, 77)
    dev = dict(device="cuda")
    tk, tm = torch.tensor(tokens, dtype=torch.int32, **dev), torch.tensor(times, dtype=torch.int32, **dev)
    pr, nt = torch.tensor(probs, **dev), torch.tensor(n_text, dtype=torch.int32, **dev)
    a = ops._ws_accept(tk, tm, pr, nt, rules, 3)
    assert a is not None
    G = 8
    ints = torch.full((4, R * N + 2 * G), -77, dtype=torch.int32, **dev)
    fp = torch.full((R * N + 2 * G,), -77.0, **dev)
    nw = torch.full((R + 2 * G,), -77, dtype=torch.int32, **dev)
    a.starts, a.ends, a.tok_begin, a.tok_end = (ints[k, G:].data_ptr() for k in range(4))
    a.out_probs, a.n_words = fp[G:].data_ptr(), nw[G:].data_ptr()
    _lib.check(_lib.lib().mopk_word_spans(C.byref(a), torch.cuda.current_stream().cuda_stream), "mopk_word_spans")
    torch.cuda.synchronize()
    assert bool((ints[:, :G] == -77).all()) and bool((ints[:, G + R * N:] == -77).all())
    assert bool((fp[:G] == -77).all()) and bool((fp[G + R * N:] == -77).all()) and bool((nw[:G] == -77).all()) and bool((nw[G + R:] == -77).all())
    want = ops.word_spans(tk, tm, pr, nt, rules, 3)
    got = ops.WordSpans(ints[0, G:G + R * N].view(R, N), ints[1, G:G + R * N].view(R, N), fp[G:G + R * N].view(R, N),
                        ints[2, G:G + R * N].view(R, N), ints[3, G:G + R * N].view(R, N), nw[G:G + R])
    assert _same(got, want) and int(got.n_words.sum()) > 0
    T, t0, Tp = 133, 3, 3
    rows, take = decoded_rows(R, T, t0, 5)
    tok, tk_ = torch.tensor(rows, dtype=torch.int32, **dev), torch.tensor(take, dtype=torch.int32, **dev)
    sot = torch.tensor([7, 8, 9], **dev)
    b = ops._ar_accept(tok, t0, tk_, sot, NOTS, EOS, torch.int32)
    assert b is not None
    W = Tp + 2 + T - t0
    two = torch.full((2, R * W + 2 * G), -77, dtype=torch.int32, **dev)
    nk = torch.full((R + 2 * G,), -77, dtype=torch.int32, **dev)
    b.ids, b.col, b.n_tokens = two[0, G:].data_ptr(), two[1, G:].data_ptr(), nk[G:].data_ptr()
    _lib.check(_lib.lib().mopk_alignment_rows(C.byref(b), torch.cuda.current_stream().cuda_stream), "mopk_alignment_rows")
    torch.cuda.synchronize()
    assert bool((two[:, :G] == -77).all()) and bool((two[:, G + R * W:] == -77).all())
    assert bool((nk[:G] == -77).all()) and bool((nk[G + R:] == -77).all())
    want = ops.alignment_rows(tok, t0, tk_, sot, NOTS, EOS, torch.int32)
    assert torch.equal(two[0, G:G + R * W].view(R, W), want.ids) and torch.equal(two[1, G:G + R * W].view(R, W), want.col)
    assert torch.equal(nk[G:G + R], want.n_tokens)


def test_what_the_kernels_do_not_take():
    from mop_amd import _lib, ops
    rules = table_rules(device="cuda")
    # N = 1025 and 1025 generated columns: the torch path, with the same results
    tokens, times, probs, n_text = random_rows(1025, 3, 9)
    check_spans(ops.word_spans, tokens, times, probs, n_text, rules, 3, "N = 1025", device="cuda")
    assert ops.LAST_PATH["word_spans"] == _lib.PATH_GENERIC
    rows, take = decoded_rows(3, 3 + 1025, 3, 11)
    check_rows(ops.alignment_rows, rows, 3, take, [7, 8, 9], NOTS, EOS, torch.int64, "S = 1025", device="cuda")
    assert ops.LAST_PATH["alignment_rows"] == _lib.PATH_GENERIC
    dev = dict(device="cuda")
    tk, tm = torch.ones(4, 8, dtype=torch.int32, **dev), torch.zeros(4, 9, dtype=torch.int32, **dev)
    pr, nt = torch.rand(4, 8, **dev), torch.full((4,), 8, dtype=torch.int32, **dev)
    assert ops.word_spans_supported(tk, tm, pr, nt, rules)
    t_ = lambda x: x.t().contiguous().t()                                  # noqa: E731  transposed: the inner stride is the row count
    assert not ops.word_spans_supported(t_(tk), tm, pr, nt, rules) and not ops.word_spans_supported(tk, t_(tm), pr, nt, rules)
    assert not ops.word_spans_supported(tk, tm, t_(pr), nt, rules)
    assert not ops.word_spans_supported(tk.long(), tm, pr, nt, rules) and not ops.word_spans_supported(tk, tm.long(), pr, nt, rules)
    assert not ops.word_spans_supported(tk, tm, pr, nt.long(), rules)
    assert not ops.word_spans_supported(tk, tm, pr, torch.zeros(8, dtype=torch.int32, **dev)[::2], rules)
    half = torch.rand(4, 9, dtype=torch.float64, **dev).view(torch.float32)[:, 1:9]     # fp32 rows that start 4 bytes off: still aligned
    assert ops.word_spans_supported(tk, tm, half, nt, rules)
    sot = torch.tensor([7, 8, 9], **dev)
    assert ops.alignment_rows_supported(tk, 3, nt, sot, NOTS, EOS)
    assert not ops.alignment_rows_supported(t_(tk), 3, nt, sot, NOTS, EOS) and not ops.alignment_rows_supported(tk.long(), 3, nt, sot, NOTS, EOS)
    assert not ops.alignment_rows_supported(tk, 3, nt.long(), sot, NOTS, EOS)
    assert not ops.alignment_rows_supported(tk, 3, nt, torch.tensor([7, 0, 8, 0, 9, 0], **dev)[::2], NOTS, EOS)


def test_no_host_sync():
    from mop_amd import _lib, ops
    rules = table_rules(device="cuda")
    tokens, times, probs, n_text = random_rows(448, 8, 3)
    dev = dict(device="cuda")
    tk, tm = torch.tensor(tokens, dtype=torch.int32, **dev), torch.tensor(times, dtype=torch.int32, **dev)
    pr, nt = torch.tensor(probs, **dev), torch.tensor(n_text, dtype=torch.int32, **dev)
    rows, take = decoded_rows(8, 448, 3, 4)
    tok, tk_ = torch.tensor(rows, dtype=torch.int32, **dev), torch.tensor(take, dtype=torch.int32, **dev)
    sot = torch.tensor([7, 8, 9], **dev)
    m = _align_model()
    mel = torch.randn(2, 200, 12, **dev)
    seqs = torch.randint(0, 290, (2, 30), **dev)
    wr = word_rules_by_residue(300, "cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.word_spans(tk, tm, pr, nt, rules, 70)
        a = ops.LAST_PATH["word_spans"]
        ar = ops.alignment_rows(tok, 3, tk_, sot, NOTS, EOS)
        b = ops.LAST_PATH["alignment_rows"]
        ops.word_spans_torch(tk, tm, pr, nt, rules, 70)
        ops.alignment_rows_torch(tok, 3, tk_, sot, NOTS, EOS)
        w = m.align_words(mel, seqs, 4, wr, median_word_frames=70, eot_token_id=295)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert a == b == _lib.PATH_FUSED and out.starts.shape == (8, 448) and ar.ids.shape == (8, 3 + 2 + 445) and w.starts.shape == (2, 24)


def test_graph_replay_reproduces_eager():
    """each op captured once and replayed on changed inputs, in a process of its own (tools/graph_probe_whisper_words.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_words.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "OP_REPLAY_IDENTICAL True" in r.stdout, r.stdout[-800:]


# ------------------------------------------------------------------ the model
def test_align_words_equals_align_tokens_plus_the_restatement():
    """the widened-logits model of test_gpu_whisper_align.py (its docstring says why the maps must be peaked), one ragged batch"""
    from mop_amd import _lib, ops
    m = _align_model()
    torch.manual_seed(5)
    mel = torch.randn(3, 200, 12, device="cuda")
    tokens = torch.randint(0, 290, (3, 30), device="cuda")
    clips, seqs = [mel[0], mel[1, :131], mel[2, :57]], [tokens[0, :19], tokens[1], tokens[2, :8]]
    rules = word_rules_by_residue(300, "cuda")
    ops.LAST_PATH.pop("word_spans", None)
    got, want = check_align_words(m, clips, seqs, 3, rules, 4, 295, "ragged")
    _fused(ops, "word_spans", "align_words")
    assert ops.LAST_PATH["token_logprob"] == _lib.PATH_FUSED and ops.LAST_PATH["dtw_align"] == _lib.PATH_FUSED
    print("align_words: words per item", got.n_words.tolist())
    assert any(len(w) >= 3 for w in want)


def _words_setup():
    from mop_amd import ops
    m = _model()
    torch.manual_seed(4)                       # CPU clips moved over: the residues of word_rules_by_residue were chosen on them
    clips = [torch.randn(n, 12).cuda() for n in (200, 150, 140)]          # four, three and three windows of 64 frames
    return m, clips, torch.tensor([7, 8, 9], device="cuda"), ops.LogitRules(V, **RULES, device="cuda"), word_rules_by_residue(V, "cuda")


def test_transcribe_words_equal_the_naive_loop_greedy():
    from mop_amd import _lib, ops
    m, clips, prompt, rules, wrules = _words_setup()
    ops.LAST_PATH.clear()
    words, trace = check_greedy_word_case(m, clips, prompt, rules, wrules, window=64)
    print("greedy:", trace, "words per clip", [int(w.starts.numel()) for w in words])
    assert ops.LAST_PATH["word_spans"] == ops.LAST_PATH["alignment_rows"] == _lib.PATH_FUSED
    assert all(t.is_cuda for w in words for t in w)
    ops.LAST_PATH.clear()
    m.with_logit_rules(rules).transcribe(clips, prompt, 12, window=64, word_rules=wrules)
    assert "word_spans" not in ops.LAST_PATH and "alignment_rows" not in ops.LAST_PATH


def test_transcribe_words_equal_the_naive_loop_fallback_skip_and_conditioning():
    m, clips, prompt, rules, wrules = _words_setup()
    check_policy_word_cases(m, clips, prompt, rules, wrules, window=64)
