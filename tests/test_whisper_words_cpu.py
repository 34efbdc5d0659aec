"""CPU checks of word timestamps (no GPU): ops.WordRules and from_pieces, ops.word_spans_torch and ops.alignment_rows_torch
against plain Python-list restatements written from Whisper's algorithm (word records, the two while loops of
merge_punctuations over records whose "text" is the tuple of their tokens' classes, numpy.median), hand-built rows for every
rule and a random sweep of shapes, every ValueError, and
WhisperMoP.align_words and transcribe(word_timestamps=True) with every core routed through its torch composition against
align_tokens plus the restatement and against a naive host loop."""
import ctypes as C
import inspect
import random

import numpy as np
import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _params, _tiny_model
from test_whisper_transcribe_cpu import EOS, RULES, TB, V, ref_row, transcribe_model

BEGIN, PRE, APP, END = 1, 2, 4, 8
NOTS = RULES["no_timestamps_token_id"]
SWEEP_N = (1, 2, 63, 64, 65, 130, 448, 1024)
EPS = 2.0 ** -24


# ------------------------------------------------------------------ the restatements
def ref_word_spans(tokens, times, probs, n_text, table, cap=None, trace=None):
    """one row, the way Whisper does it -> a list of (start, end, prob (float64 mean), tok_begin, tok_end, count of own tokens).
    trace: a dict that counts what happened ("words" is the largest count of one row).
    find_alignment: split the tokens into words, a word ends where the next one starts, its probability is the mean of its
    tokens'.  add_word_timestamps: the duration bound from the median, the truncation at sentence ends, merge_punctuations."""
    N, Vt = len(tokens), len(table)
    n = min(max(n_text, 0), N)
    cls = [table[min(max(t, 0), Vt - 1)] for t in tokens[:n]]
    words = []                                                             # split_tokens_on_spaces: a record per word
    for i in range(n):
        if i == 0 or cls[i] & BEGIN:
            words.append(dict(text=(), tokens=[]))
        words[-1]["text"] += (cls[i],)
        words[-1]["tokens"].append(i)
    bounds = [w["tokens"][0] for w in words] + [n]
    for k, w in enumerate(words):
        w["start"], w["end"] = times[bounds[k]], times[bounds[k + 1]]
        w["prob"] = float(np.mean(np.asarray([probs[i] for i in w["tokens"]], dtype=np.float64)))
        w["count"] = len(w["tokens"])
    if not words:
        return []
    trace = {} if trace is None else trace
    count = lambda key: trace.__setitem__(key, trace.get(key, 0) + 1)      # noqa: E731
    single = lambda w, bit: len(w["text"]) == 1 and bool(w["text"][0] & bit)   # noqa: E731  "the word is this punctuation mark"
    dur = np.asarray([w["end"] - w["start"] for w in words], dtype=np.int64)
    nz = dur[dur.nonzero()[0]]
    m2 = int(round(2 * float(np.median(nz)))) if len(nz) else 0            # twice the median: an integer
    max_dur = m2 if cap is None else min(m2, 2 * cap)
    ends_sentence = [single(w, END) for w in words]
    for k in range(1, len(words)):                                         # truncate long words at sentence boundaries
        if dur[k] > max_dur:
            if ends_sentence[k]:
                words[k]["end"] = words[k]["start"] + max_dur
                count("truncated")
            elif ends_sentence[k - 1]:
                words[k]["start"] = words[k]["end"] - max_dur
                count("truncated")
    i, j = len(words) - 2, len(words) - 1                                  # merge_punctuations: prepended marks, right to left
    while i >= 0:
        previous, following = words[i], words[j]
        if single(previous, PRE):
            following["text"] = previous["text"] + following["text"]
            following["tokens"] = previous["tokens"] + following["tokens"]
            previous["text"], previous["tokens"] = (), []
            count("prepended")
        else:
            j = i
        i -= 1
    i, j = 0, 1                                                            # appended marks, left to right
    while j < len(words):
        previous, following = words[i], words[j]
        if single(following, APP) and previous["tokens"]:                  # (Whisper's endswith(" ") test is dropped; an emptied
            previous["text"] = previous["text"] + following["text"]        # record takes nothing: the mark then stays a word)
            previous["tokens"] = previous["tokens"] + following["tokens"]
            following["text"], following["tokens"] = (), []
            count("appended")
        else:
            i = j
        j += 1
    out = []
    for w in words:
        if w["tokens"]:
            assert w["tokens"] == list(range(w["tokens"][0], w["tokens"][-1] + 1))
            out.append((int(w["start"]), int(w["end"]), w["prob"], w["tokens"][0], w["tokens"][-1] + 1, w["count"]))
    trace["words"] = max(trace.get("words", 0), len(out))
    return out


def ref_alignment_rows(row, t0, n_take, sot, nots, eos):
    """one row -> (ids, n_tokens, col), W = T_p + 2 + (T - t0) entries each"""
    S = len(row) - t0
    W = len(sot) + 2 + S
    m = min(max(n_take, 0), S)
    text = [(row[t0 + j], t0 + j) for j in range(m) if row[t0 + j] < eos]
    ids = list(sot) + [nots] + [t for t, _ in text] + [eos]
    return ids + [eos] * (W - len(ids)), len(sot) + 2 + len(text), [c for _, c in text] + [-1] * (W - len(text))


# ------------------------------------------------------------------ comparing
def guarded(shape, dtype, device, row_pad=0):
    """a (R, N) view with `row_pad` spare columns per row inside a buffer with 8 guard words on both sides"""
    R, N = shape
    flat = torch.full((16 + R * (N + row_pad),), -77, dtype=dtype, device=device)
    return flat, flat[8:8 + R * (N + row_pad)].view(R, N + row_pad)[:, :N]


def check_spans(fn, tokens, times, probs, n_text, rules, cap, what, device="cpu", pad=0):
    """fn on these rows (lists) against the restatement: integers equal, probs within (count + 1) * 2^-24 of the float64 mean"""
    R, N = len(tokens), len(tokens[0])
    _, tk = guarded((R, N), torch.int32, device, pad)
    _, tm = guarded((R, N + 1), torch.int32, device, pad)
    _, pr = guarded((R, N), torch.float32, device, pad)
    tk.copy_(torch.tensor(tokens, dtype=torch.int32))
    tm.copy_(torch.tensor(times, dtype=torch.int32))
    pr.copy_(torch.tensor(probs, dtype=torch.float32))
    nt = torch.tensor(n_text, dtype=torch.int32, device=device)
    got = fn(tk, tm, pr, nt, rules, cap)
    compare_spans(got, tokens, times, pr.cpu().tolist(), n_text, rules, cap, what)
    return got


def compare_spans(got, tokens, times, probs, n_text, rules, cap, what):
    R, N = len(tokens), len(tokens[0])
    table = rules.on("cpu").tolist()
    for name in ("starts", "ends", "tok_begin", "tok_end", "n_words"):
        assert getattr(got, name).dtype == torch.int32, (what, name)
    assert got.probs.dtype == torch.float32 and got.probs.shape == (R, N) and got.n_words.shape == (R,), what
    st, en, pb, tb_, te, nw = (t.cpu().tolist() for t in got)
    refs = []
    for r in range(R):
        ref = ref_word_spans(tokens[r], times[r], probs[r], n_text[r], table, cap)
        refs.append(ref)
        k = len(ref)
        assert nw[r] == k, (what, r, nw[r], k)
        assert st[r][:k] == [w[0] for w in ref] and en[r][:k] == [w[1] for w in ref], (what, r, st[r][:k], en[r][:k], ref)
        assert tb_[r][:k] == [w[3] for w in ref] and te[r][:k] == [w[4] for w in ref], (what, r, tb_[r][:k], te[r][:k], ref)
        for j, w in enumerate(ref):
            assert abs(pb[r][j] - w[2]) <= (w[5] + 1) * EPS, (what, r, j, pb[r][j], w[2])
        assert all(x == -1 for row in (st, en, tb_, te) for x in row[r][k:]) and all(x == 0 for x in pb[r][k:]), (what, r)
    return refs


def check_rows(fn, rows, t0, n_take, sot, nots, eos, dtype, what, device="cpu", pad=0, sot_dtype=torch.int64):
    R, T = len(rows), len(rows[0])
    _, tk = guarded((R, T), torch.int32, device, pad)
    tk.copy_(torch.tensor(rows, dtype=torch.int32))
    per_row = isinstance(sot[0], list)
    got = fn(tk, t0, torch.tensor(n_take, dtype=torch.int32, device=device), torch.tensor(sot, dtype=sot_dtype, device=device), nots, eos,
             dtype)
    assert got.ids.dtype == dtype and got.n_tokens.dtype == got.col.dtype == torch.int32, what
    W = len(sot[0] if per_row else sot) + 2 + T - t0
    assert got.ids.shape == got.col.shape == (R, W) and got.n_tokens.shape == (R,), what
    for r in range(R):
        ids, n, col = ref_alignment_rows(rows[r], t0, n_take[r], sot[r] if per_row else sot, nots, eos)
        assert got.ids[r].tolist() == ids and int(got.n_tokens[r]) == n and got.col[r].tolist() == col, (what, r)
    return got


# ------------------------------------------------------------------ cases
def table_rules(Vt=16, device=None):
    """ids: 0-3 continue a word, 4-7 begin one, 8 prepend (and begin, as " (" does), 9 append (no begin, as "," does), 10 append
    and begin (as a lone "." piece of string.punctuation does) and sentence end, 11 prepend and append and begin (as ' "' is
    not, but a table may say so), 12 sentence end that continues, 13 begin and sentence end, 14-15 begin"""
    from mop_amd import ops
    return ops.WordRules(Vt, [4, 5, 6, 7, 8, 10, 11, 13, 14, 15], [8, 11], [9, 10, 11], [10, 12, 13], device=device)


def hand_cases():
    """(name, tokens, times, n_text, cap, expected (start, end, tok_begin, tok_end) list or None)"""
    ramp = lambda n, step=2: [step * i for i in range(n + 1)]              # noqa: E731
    return [
        ("every token a begin", [4, 5, 6, 7], ramp(4), 4, None, [(0, 2, 0, 1), (2, 4, 1, 2), (4, 6, 2, 3), (6, 8, 3, 4)]),
        ("no begin at all: one word", [0, 1, 2, 3], ramp(4), 4, None, [(0, 8, 0, 4)]),
        ("a run of prepends joins the next word", [4, 8, 8, 5, 1], ramp(5), 5, None, [(0, 2, 0, 1), (6, 10, 1, 5)]),
        ("a prepend as the last word stays", [4, 1, 8], ramp(3), 3, None, [(0, 4, 0, 2), (4, 6, 2, 3)]),
        ("an append as word 0 stays", [10, 4, 10], ramp(3), 3, None, [(0, 2, 0, 1), (2, 4, 1, 3)]),
        ("an append after a prepend-run host stays: it follows a merged word", [4, 8, 10, 5], ramp(4), 4, None,
         [(0, 2, 0, 1), (4, 6, 1, 3), (6, 8, 3, 4)]),
        ("a begin-append after a plain word joins it", [4, 10, 5], ramp(3), 3, None, [(0, 2, 0, 2), (4, 6, 2, 3)]),
        ("appends in a row all join", [4, 10, 10, 10, 5], ramp(5), 5, None, [(0, 2, 0, 4), (8, 10, 4, 5)]),
        ("a token with both bits: dies forward in pass 1", [4, 11, 5], ramp(3), 3, None, [(0, 2, 0, 1), (4, 6, 1, 3)]),
        ("a token with both bits as the last word: joins backward", [4, 11], ramp(2), 2, None, [(0, 2, 0, 2)]),
        ("prepends before an append: the append takes them and stays", [8, 8, 10], ramp(3), 3, None, [(4, 6, 0, 3)]),
        ("every earlier word died: the append stays", [8, 10, 4], ramp(3), 3, None, [(2, 4, 0, 2), (4, 6, 2, 3)]),
        ("all durations zero", [4, 5, 6], [3, 3, 3, 3], 3, None, [(3, 3, 0, 1), (3, 3, 1, 2), (3, 3, 2, 3)]),
        ("an odd count of nonzero durations: median 4, a long sentence end is cut", [4, 5, 6, 10], [0, 2, 6, 6, 40], 4, None,
         [(0, 2, 0, 1), (2, 6, 1, 2), (6, 6, 2, 4)]),
        ("an even count: median (2 + 4) / 2, max_dur 6", [4, 5, 10, 6], [0, 2, 6, 30, 30], 4, None,
         [(0, 2, 0, 1), (2, 6, 1, 3), (30, 30, 3, 4)]),
        ("a long word after a sentence end starts late", [4, 13, 5, 6], [0, 2, 4, 40, 42], 4, None,
         [(0, 2, 0, 1), (2, 4, 1, 2), (36, 40, 2, 3), (40, 42, 3, 4)]),
        ("a sentence end inside a longer word is none", [4, 12, 5, 6], [0, 2, 4, 40, 42], 4, None,
         [(0, 4, 0, 2), (4, 40, 2, 3), (40, 42, 3, 4)]),
        ("the cap acts", [4, 5, 13, 6], [0, 10, 20, 30, 90], 4, 3, None),
        ("the cap does not act", [4, 5, 13, 6], [0, 10, 20, 30, 90], 4, 70, None),
        ("cap 0", [4, 5, 13, 6], [0, 10, 20, 30, 90], 4, 0, None),
        ("n_text cuts the row", [4, 5, 10, 6, 7], ramp(5), 3, None, [(0, 2, 0, 1), (2, 4, 1, 3)]),
        ("n_text 0", [4, 5], ramp(2), 0, None, []),
        ("n_text below 0 and ids outside the table", [-5, 99], ramp(2), -3, None, []),
        ("ids outside the table are clamped", [-5, 99, 99], ramp(3), 7, None, [(0, 2, 0, 1), (2, 4, 1, 2), (4, 6, 2, 3)]),
    ]


def random_rows(N, R, seed, Vt=16):
    rng = random.Random(seed)
    tokens, times, probs, n_text = [], [], [], []
    for r in range(R):
        style = rng.randrange(4)
        pool = {0: list(range(Vt)), 1: [0, 1, 4, 8, 9, 10], 2: [8, 9, 10, 11, 12, 4], 3: list(range(-3, Vt + 3))}[style]
        tokens.append([rng.choice(pool) for _ in range(N)])
        t, row = rng.randrange(5), []
        for _ in range(N + 1):
            row.append(t)
            t += rng.choice([0, 0, 1, 2, 3, 40]) if rng.random() < 0.9 else rng.choice([0, 500])
        times.append(row)
        probs.append([rng.random() for _ in range(N)])
        n_text.append(rng.choice([0, N, N, rng.randrange(N + 1), rng.randrange(N + 1), -2, N + 5]))
    return tokens, times, probs, n_text


def decoded_rows(R, T, t0, seed):
    """rows over {text, timestamps, eos} and an n_take for each"""
    rng = random.Random(seed)
    rows, take = [], []
    for r in range(R):
        rows.append([rng.choice([rng.randrange(EOS), rng.randrange(EOS), TB + rng.randrange(20), EOS]) for _ in range(T)])
        take.append(rng.choice([0, T - t0, rng.randrange(T - t0 + 1), -3, T]))
    return rows, take


# ------------------------------------------------------------------ WordRules
def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import TranscriptWords, WhisperMoP, WordAlignment
    from mop_amd.nn.whisper_mop import RuledDecoding
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    sig = dict(tokens=(e, P), t0=(e, P), n_take=(e, P), sot=(e, P), no_timestamps_token_id=(e, P), eos_token_id=(e, P),
               dtype=(torch.int64, P))
    for fn in (ops.alignment_rows, ops.alignment_rows_torch, ops.alignment_rows_supported):
        assert _params(fn) == sig, fn.__name__
    sig = dict(tokens=(e, P), times=(e, P), probs=(e, P), n_text=(e, P), word_rules=(e, P), median_cap=(None, P))
    for fn in (ops.word_spans, ops.word_spans_torch, ops.word_spans_supported):
        assert _params(fn) == sig, fn.__name__
    assert ops.AlignmentRows._fields == ("ids", "n_tokens", "col")
    fields = ("starts", "ends", "probs", "tok_begin", "tok_end")
    assert ops.WordSpans._fields == WordAlignment._fields == fields + ("n_words",) and TranscriptWords._fields == fields + ("segment",)
    assert _params(WhisperMoP.align_words) == dict(
        mel=(e, P), tokens=(e, P), prompt_len=(e, P), word_rules=(e, P), alignment_heads=(None, P), medfilt_width=(7, P),
        median_word_frames=(None, P), eot_token_id=(None, K))
    new = dict(word_timestamps=(False, K), word_rules=(None, K), alignment_heads=(None, K), medfilt_width=(7, K),
               median_word_frames=(None, K))
    for fn in (RuledDecoding.transcribe, WhisperMoP._transcribe):
        got = _params(fn)
        assert {k: got.get(k) for k in new} == new, fn.__name__
    assert not any(k in _params(WhisperMoP.transcribe) for k in new)       # the public signature stays


def test_word_rules_from_pieces():
    from mop_amd import ops
    pieces = [" the", "re", ".", " (", ",", " -", None, "", " ", "?", ")", " \"", "\"", " 。", "。", " a.", "!!", "-"]
    want = [BEGIN, 0, BEGIN | APP | END, BEGIN | PRE, BEGIN | APP, BEGIN | PRE, 0, 0, BEGIN | PRE, BEGIN | APP | END, BEGIN | APP,
            BEGIN | PRE, BEGIN | APP, BEGIN, APP | END, BEGIN, 0, BEGIN]
    r = ops.WordRules.from_pieces(pieces)
    assert r.vocab_size == len(pieces) and r.table.dtype == torch.uint8 and r.table.tolist() == want
    # " " strips to "", which every str contains: Whisper's own test makes a lone space a prepended mark
    r = ops.WordRules.from_pieces(pieces, prepend="(", append=",", sentence_end=",")
    assert r.table.tolist()[:6] == [BEGIN, 0, BEGIN, BEGIN | PRE, BEGIN | APP | END, BEGIN]
    for bad in ([1, " a"], [" a", b"b"]):
        with pytest.raises(ValueError):
            ops.WordRules.from_pieces(bad)
    with pytest.raises(ValueError):
        ops.WordRules.from_pieces([" a"], prepend=None)


def test_word_rules_table_and_value_errors():
    from mop_amd import ops
    r = ops.WordRules(6, [0, 1], prepend_punct=(1,), append_punct=iter([2, 2]), sentence_end=torch.tensor([0, 0, 1, 0, 0, 1], dtype=torch.bool))
    assert r.table.tolist() == [1, 3, 4 | 8, 0, 0, 8] and r.table.device.type == "cpu" and r.on("cpu") is r.table
    assert ops.WordRules(3, ()).table.tolist() == [0, 0, 0]
    for args in ((0, []), (True, []), (2.0, []), (None, []), (4, [4]), (4, [-1]), (4, [0], [9]), (4, [0], (), [4]), (4, [0], (), (), [-2]),
                 (4, [1.0]), (4, [True]), (4, 3), (4, None), (4, "01"), (4, torch.ones(3, dtype=torch.bool)),
                 (4, torch.ones(4, dtype=torch.int64)), (4, [0], torch.ones(4, 1, dtype=torch.bool))):
        with pytest.raises(ValueError):
            ops.WordRules(*args)


# ------------------------------------------------------------------ the torch twins
def test_word_spans_torch_hand_rows():
    from mop_amd import _lib, ops
    rules = table_rules()
    for name, tokens, times, n, cap, want in hand_cases():
        probs = [((7 * i + 3) % 10) / 10 for i in range(len(tokens))]
        for fn in (ops.word_spans_torch, ops.word_spans):
            got = check_spans(fn, [tokens], [times], [probs], [n], rules, cap, name)
        if want is not None:
            k = int(got.n_words[0])
            assert list(zip(got.starts[0, :k].tolist(), got.ends[0, :k].tolist(), got.tok_begin[0, :k].tolist(),
                            got.tok_end[0, :k].tolist())) == want, name
    assert ops.LAST_PATH["word_spans"] == _lib.PATH_GENERIC
    # the truncations, by value: median 2 -> max_dur 4
    got = check_spans(ops.word_spans_torch, [[4, 5, 13, 6]], [[0, 10, 20, 30, 90]], [[.5] * 4], [4], rules, 3, "the cap acts")
    assert got.starts[0].tolist() == [0, 10, 20, 84] and got.ends[0].tolist() == [10, 20, 26, 90]            # max_dur 6, not 20
    got = check_spans(ops.word_spans_torch, [[4, 5, 13, 6]], [[0, 10, 20, 30, 90]], [[.5] * 4], [4], rules, 70, "the cap idles")
    assert got.starts[0].tolist() == [0, 10, 20, 70] and got.ends[0].tolist() == [10, 20, 30, 90]            # max_dur 20
    got = check_spans(ops.word_spans_torch, [[4, 5, 13, 6]], [[0, 10, 20, 30, 90]], [[.5] * 4], [4], rules, 0, "cap 0")
    assert got.starts[0].tolist() == [0, 10, 20, 90] and got.ends[0].tolist() == [10, 20, 20, 90]
    # a word's probability is the mean of its OWN tokens: what it absorbs does not count
    got = check_spans(ops.word_spans_torch, [[8, 4, 0, 10]], [[0, 1, 2, 3, 4]], [[.1, .2, .4, .9]], [4], rules, None, "own probability")
    assert int(got.n_words[0]) == 1 and abs(float(got.probs[0, 0]) - 0.3) < 1e-6 and got.tok_begin[0, 0] == 0 and got.tok_end[0, 0] == 4


@pytest.mark.parametrize("N", SWEEP_N)
def test_word_spans_torch_sweep(N):
    from mop_amd import ops
    rules = table_rules()
    R = 6 if N >= 448 else 24
    for seed, cap, pad in ((0, None, 0), (1, 1, 3), (2, 70, 0)):
        tokens, times, probs, n_text = random_rows(N, R, 1000 * N + seed)
        check_spans(ops.word_spans_torch, tokens, times, probs, n_text, rules, cap, (N, seed), pad=pad)
    tokens, times, probs, n_text = random_rows(N, 2, N)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)                     # noqa: E731  int64 inputs pass the torch path too
    got = ops.word_spans_torch(i64(tokens), i64(times), torch.tensor(probs), i64(n_text), rules)
    compare_spans(got, tokens, times, torch.tensor(probs).tolist(), n_text, rules, None, ("int64", N))
    assert not ops.word_spans_supported(i64(tokens), i64(times), torch.tensor(probs), i64(n_text), rules)


def test_alignment_rows_torch_matches_the_restatement():
    from mop_amd import _lib, ops
    sot = [7, 8, 9]
    rows = [[7, 8, 9, TB, 5, 6, TB + 2, TB + 2, 11, EOS, EOS],             # text between timestamps, an eos inside n_take
            [7, 8, 9, TB, TB + 1, EOS, 4, 4, 4, 4, 4],                     # no text at all inside n_take
            [7, 8, 9, 1, 2, 3, 4, 5, 6, 7, 8]]                             # text only
    got = check_rows(ops.alignment_rows_torch, rows, 3, [6, 2, 8], sot, NOTS, EOS, torch.int64, "by hand")
    assert got.ids[0].tolist() == [7, 8, 9, NOTS, 5, 6, 11] + [EOS] * 6 and got.col[0, :4].tolist() == [4, 5, 8, -1]
    assert got.n_tokens.tolist() == [8, 5, 13] and got.ids[2, -1] == EOS
    for S in (1, 2, 63, 64, 65, 130, 448, 1024):
        for t0, R, pad, dt in ((0, 3, 0, torch.int32), (3, 5, 2, torch.int64)):
            rows, take = decoded_rows(R, t0 + S, t0, S + t0)
            per_row = [[r, r + 1] for r in range(R)]
            check_rows(ops.alignment_rows_torch, rows, t0, take, sot if t0 else per_row, NOTS, EOS, dt, (S, t0), pad=pad,
                       sot_dtype=(torch.int64, torch.int32)[S % 2])
    check_rows(ops.alignment_rows, rows, 3, take, sot, NOTS, EOS, torch.int64, "public")
    assert ops.LAST_PATH["alignment_rows"] == _lib.PATH_GENERIC


def test_op_value_errors():
    from mop_amd import ops
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)                     # noqa: E731
    rules = table_rules()
    tok, tm, pr, n = torch.ones(2, 4, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32), torch.rand(2, 4), i32([4, 2])
    good = [tok, tm, pr, n, rules, None]
    for fn in (ops.word_spans, ops.word_spans_torch, ops.word_spans_supported):
        fn(*good)
        fn(tok, tm, pr, n, rules, 0)
        for i, v in ((0, tok.float()), (0, tok[0]), (0, tok[:, :0]), (0, tok.bool()), (0, None), (0, tok.to("meta")),
                     (1, tm[:, :4]), (1, tm.float()), (1, None), (1, tm.to("meta")),
                     (2, pr.double()), (2, pr[:, :3]), (2, tok), (2, None), (2, pr.to("meta")),
                     (3, n.float()), (3, i32([1, 2, 3])), (3, n.view(2, 1)), (3, None), (3, n.to("meta")),
                     (4, None), (4, rules.table), (5, -1), (5, 1.0), (5, True), (5, 2 ** 30)):
            args = list(good)
            args[i] = v
            with pytest.raises(ValueError):
                fn(*args)
    sot = torch.tensor([7, 8, 9])
    good = [tok, 1, n, sot, NOTS, EOS, torch.int64]
    for fn in (ops.alignment_rows, ops.alignment_rows_torch, ops.alignment_rows_supported):
        fn(*good)
        for i, v in ((0, tok.float()), (0, tok[0]), (0, tok[:, :0]), (0, None), (0, tok.to("meta")),
                     (1, -1), (1, 4), (1, 1.0), (1, True),
                     (2, n.float()), (2, i32([1])), (2, None), (2, n.to("meta")),
                     (3, sot.float()), (3, sot.to(torch.int16)), (3, sot[:0]), (3, sot.view(1, 1, 3)), (3, sot.view(1, 3).expand(3, 3)),
                     (3, None), (3, sot.to("meta")),
                     (4, None), (4, -1), (4, 2 ** 31), (4, True), (5, None), (5, -1), (5, 1.5),
                     (6, torch.int16), (6, torch.float32), (6, None)):
            args = list(good)
            args[i] = v
            with pytest.raises(ValueError):
                fn(*args)


# ------------------------------------------------------------------ ABI
def test_support_queries_and_bad_arguments_need_no_gpu():
    from mop_amd import _lib, build
    build.build_lib()
    lib = _lib.lib()

    def rows(**kw):
        a = _lib.AlignmentRowsArgs()
        a.R, a.T, a.T0, a.Tp, a.nots, a.eos, a.tokens_ld = 4, 448, 3, 3, 100, 97, 448
        for f in ("tokens", "n_take", "sot", "ids", "n_tokens", "col"):
            setattr(a, f, 64)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def spans(**kw):
        a = _lib.WordSpansArgs()
        a.R, a.N, a.V, a.median_cap, a.tokens_ld, a.times_ld, a.probs_ld = 4, 445, 131, -1, 445, 446, 445
        for f in ("tokens", "times", "probs", "n_text", "table", "starts", "ends", "out_probs", "tok_begin", "tok_end", "n_words"):
            setattr(a, f, 64)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    q = lambda a: lib.mopk_alignment_rows_supported(C.byref(a))            # noqa: E731
    assert q(rows()) and q(rows(T=1027, tokens_ld=1027)) and q(rows(out_i64=1, sot_i64=1, sot_ld=3)) and q(rows(ids=68, sot=68))
    for kw in (dict(T=1028, tokens_ld=1028), dict(T0=448), dict(T0=-1), dict(R=0), dict(Tp=0), dict(tokens_ld=447), dict(sot_ld=2),
               dict(out_i64=2), dict(sot_i64=-1), dict(tokens=66), dict(n_take=65), dict(col=66), dict(n_tokens=66),
               dict(out_i64=1, ids=68), dict(sot_i64=1, sot=68)):
        assert not q(rows(**kw)), kw
        assert lib.mopk_alignment_rows(C.byref(rows(**kw)), None) != 0, kw                 # refused before any launch
    assert lib.mopk_alignment_rows(C.byref(rows(col=0)), None) != 0 and lib.mopk_alignment_rows(None, None) != 0
    q = lambda a: lib.mopk_word_spans_supported(C.byref(a))                # noqa: E731
    assert q(spans()) and q(spans(N=1024, tokens_ld=1024, times_ld=1025, probs_ld=1030)) and q(spans(median_cap=0)) and q(spans(table=65))
    for kw in (dict(N=1025, tokens_ld=1025, times_ld=1026, probs_ld=1025), dict(N=0), dict(R=0), dict(V=0), dict(median_cap=-2),
               dict(tokens_ld=444), dict(times_ld=445), dict(probs_ld=444), dict(tokens=66), dict(times=65), dict(probs=66),
               dict(n_text=66), dict(starts=66), dict(ends=66), dict(out_probs=66), dict(tok_begin=66), dict(tok_end=66),
               dict(n_words=66)):
        assert not q(spans(**kw)), kw
        assert lib.mopk_word_spans(C.byref(spans(**kw)), None) != 0, kw                    # refused before any launch
    assert lib.mopk_word_spans(C.byref(spans(table=0)), None) != 0 and lib.mopk_word_spans(None, None) != 0
    assert lib.mopk_version() == 118


# ------------------------------------------------------------------ the model on the torch cores
def word_rules_by_residue(vocab, device="cpu"):
    """a WordRules over token-id residues (the text tokens of these tests are whatever the random models emit): mod 5 == 0 is a
    prepended mark, mod 5 == 1 an appended one, an even id or a prepended mark begins a word, an odd id is a sentence end.
    Chosen on the CPU path so that the greedy cases of both transcribe models (this file's and the GPU file's) show every rule
    at work; check_greedy_word_case asserts that they do"""
    from mop_amd import ops
    ids = range(vocab)
    return ops.WordRules(vocab, [v for v in ids if v % 2 == 0 or v % 5 == 0], [v for v in ids if v % 5 == 0],
                         [v for v in ids if v % 5 == 1], [v for v in ids if v % 2 == 1], device=device)


SOFTMAX64_TOL = 2e-5   # the sanity check of reference_token_probs only: an fp32 log-softmax of <= 300 fp32 logits against the
#                        float64 one (|error| of the lse <~ 1e-6, a few ulps of logits of size ~10 ~ 4e-6; d exp = p * d <= d)


def reference_token_probs(m, mel, seqs, eot):
    """the reference's own teacher-forced pass over the right-padded sequences -> fp32 (B, T - 1) on the CPU: column p holds
    exp(ops.token_logprob(logits[:, p, :eot], tokens[:, p + 1])), one call of the op per position, as align_words states it
    (a token at or above eot is read as eot - 1, as there).  As a sanity check every value is within SOFTMAX64_TOL of the
    float64 softmax of the same logits."""
    from mop_amd import ops
    T = max(len(s) for s in seqs)
    ids = torch.zeros(len(seqs), T, dtype=torch.long, device=seqs[0].device)
    for b, s in enumerate(seqs):
        ids[b, :len(s)] = s
    with torch.no_grad():
        logits = m.decode(m.encode(mel)[0], ids)
    Vr = logits.shape[-1] if eot is None else eot
    nxt = ids[:, 1:].clamp(0, Vr - 1)
    probs = torch.stack([ops.token_logprob(logits[:, p, :Vr], nxt[:, p].to(torch.int32).contiguous()).exp() for p in range(T - 1)], 1)
    assert probs.dtype == torch.float32
    p64 = torch.log_softmax(logits[:, :T - 1, :Vr].double(), -1).gather(2, nxt.unsqueeze(2)).squeeze(2).exp()
    assert float((probs.double() - p64).abs().max()) <= SOFTMAX64_TOL
    return probs.cpu()


def align_words_reference(m, mel, seqs, P, rules, cap, eot, heads=None, width=7):
    """align_tokens on the same batch, the fp32 token probabilities of reference_token_probs, and the restatement (its mean
    in float64) -> per item the list of (start, end, prob, tok_begin, tok_end, count), token indices of the full sequence"""
    al = m.align_tokens(mel, seqs, P, heads, width)
    tp = reference_token_probs(m, mel, list(seqs), eot)
    table = rules.on("cpu").tolist()
    out = []
    for b, s in enumerate(seqs):
        n_text = len(s) - P - 2
        text = s[P + 1:P + 1 + n_text].tolist()
        times = al.starts[b, P:P + n_text + 1].tolist()
        probs = tp[b, P:P + n_text].tolist()
        out.append([(a, e, p, tb_ + P + 1, te + P + 1, c) for a, e, p, tb_, te, c in
                    ref_word_spans(text, times, probs, n_text, table, cap)] if n_text > 0 else [])
    return out


def assert_words_equal(got_row, want, what):
    """one item's (starts, ends, probs, tok_begin, tok_end) lists against the reference records: integers equal, probs within
    (count + 1) * 2^-24 of the float64 mean of the reference's fp32 token probabilities"""
    st, en, pb, tb_, te = got_row
    assert st == [w[0] for w in want] and en == [w[1] for w in want], (what, st, en, want)
    assert tb_ == [w[3] for w in want] and te == [w[4] for w in want], (what, tb_, te, want)
    for j, w in enumerate(want):
        assert abs(pb[j] - w[2]) <= (w[5] + 1) * EPS, (what, j, pb[j], w[2])


def check_align_words(m, mel, seqs, P, rules, cap, eot, what):
    want = align_words_reference(m, mel, seqs, P, rules, cap, eot)
    got = m.align_words(mel, seqs, P, rules, median_word_frames=cap, eot_token_id=eot)
    N = max(len(s) for s in seqs) - P - 2
    assert all(t.shape == (len(seqs), N) for t in got[:5]) and got.n_words.shape == (len(seqs),), what
    for b, w in enumerate(want):
        k = int(got.n_words[b])
        assert k == len(w), (what, b, k, len(w))
        assert_words_equal([t[b, :k].tolist() for t in got[:5]], w, (what, b))
        assert all(bool((t[b, k:] == -1).all()) for t in (got.starts, got.ends, got.tok_begin, got.tok_end)), (what, b)
    return got, want


def test_align_words_equals_align_tokens_plus_the_restatement(torch_cores):               # noqa: F811
    m = _tiny_model()
    rules = word_rules_by_residue(100)
    torch.manual_seed(3)
    mel = [torch.randn(n, 10) for n in (40, 23, 31)]
    seqs = [torch.randint(0, 90, (n,)) for n in (30, 9, 6)]                # prompt_len 3: 25, 4 and 1 text tokens
    got, want = check_align_words(m, mel, seqs, 3, rules, 4, 95, "ragged")
    assert any(len(w) >= 3 for w in want)
    check_align_words(m, torch.randn(2, 40, 10), torch.randint(0, 90, (2, 12)), 0, rules, None, None, "tensor")


def window_words_reference(m, wins, rows, T_p, prompt_of, nots, eos, tb, f, wrules, cap, seeks, bases, trace=None):
    """one set of windows: rows are the decoded rows (the sot sequence and the generated tokens, lists), wins their clips ->
    per row the list of words in clip frames and Transcript token indices, or [] for a row without text"""
    table = wrules.on("cpu").tolist()
    seqs, cols, keep = [], [], []
    for a, row in enumerate(rows):
        segs, _ = ref_row(row, T_p, wins[a].shape[0], tb, eos, f)
        m_take = segs[-1][3] - T_p if segs else 0
        text = [(row[T_p + j], T_p + j) for j in range(m_take) if row[T_p + j] < eos]
        if text:
            keep.append(a)
            seqs.append(torch.tensor(list(prompt_of(a)) + [nots] + [t for t, _ in text] + [eos], device=wins[a].device))
            cols.append([c for _, c in text])
    out = [[] for _ in rows]
    if not keep:
        return out
    sub = [wins[a] for a in keep]
    al = m.align_tokens(sub, seqs, T_p)
    tp = reference_token_probs(m, sub, seqs, eos)
    for i, a in enumerate(keep):
        n_text = len(cols[i])
        text = seqs[i][T_p + 1:T_p + 1 + n_text].tolist()
        times = al.starts[i, T_p:T_p + n_text + 1].tolist()
        probs = tp[i, T_p:T_p + n_text].tolist()
        for s, e, p, b0, b1, c in ref_word_spans(text, times, probs, n_text, table, cap, trace):
            out[a].append((s + seeks[a], e + seeks[a], p, cols[i][b0] - T_p + bases[a], cols[i][b1 - 1] + 1 - T_p + bases[a], c))
    return out


def naive_word_transcribe(m, clips, prompt, rules, wrules, n_new, window, cap, decode_rows, f=1):
    """the word loop on the host: `decode_rows(act, wins)` gives the kept rows (lists, from the sot sequence on) and the skip
    flags of one set of windows; everything else is lists -> per clip the words, and what the restatement counted (the most
    words of one window, absorbed prepended and appended marks, truncations, windows)"""
    B, T_p, eos, tb = len(clips), prompt.shape[-1], rules.eos_token_id, rules.timestamp_begin
    seek, n_tok = [0] * B, [0] * B
    words, trace = [[] for _ in range(B)], dict(windows=0, skipped=0)
    while any(seek[b] < clips[b].shape[0] for b in range(B)):
        act = [b for b in range(B) if seek[b] < clips[b].shape[0]]
        wins = [clips[b][seek[b]:seek[b] + window] for b in act]
        rows, skipped = decode_rows(act, wins)
        live = [a for a in range(len(act)) if not skipped[a]]
        sot = lambda a: (prompt if prompt.dim() == 1 else prompt[act[live[a]]]).tolist()   # noqa: E731
        got = window_words_reference(m, [wins[a] for a in live], [rows[a] for a in live], T_p, sot, rules.no_timestamps_token_id, eos,
                                     tb, f, wrules, cap, [seek[act[a]] for a in live], [n_tok[act[a]] for a in live], trace)
        for a, b in enumerate(act):
            trace["windows"] += 1
            if skipped[a]:
                seek[b] += wins[a].shape[0]
                trace["skipped"] += 1
                continue
            words[b].extend(got[live.index(a)])
            segs, adv = ref_row(rows[a], T_p, wins[a].shape[0], tb, eos, f)
            seek[b] += adv
            n_tok[b] += segs[-1][3] - T_p if segs else 0
    return words, trace


def assert_transcript_words(got_words, transcripts, want, what):
    from mop_amd.nn import TranscriptWords
    assert len(got_words) == len(want)
    for b, (g, w) in enumerate(zip(got_words, want)):
        assert isinstance(g, TranscriptWords) and g.probs.dtype == torch.float32 and g.segment.dtype == torch.int64, (what, b)
        assert all(t.dtype == torch.int32 for t in (g.starts, g.ends, g.tok_begin, g.tok_end)), (what, b)
        assert_words_equal([t.tolist() for t in g[:5]], w, (what, b))
        off = transcripts[b].offsets.tolist()
        for j, x in enumerate(w):                                          # the word begins inside the segment it names
            s = int(g.segment[j])
            assert off[s] <= x[3] < off[s + 1] and x[3] < x[4] <= off[-1], (what, b, j, x, off)


def words_setup(device="cpu"):
    from mop_amd import ops
    m = transcribe_model().to(device)
    torch.manual_seed(1)
    clips = [torch.randn(n, 10).to(device) for n in (100, 40, 17)]
    return m, clips, torch.tensor([7, 8, 9], device=device), ops.LogitRules(V, **RULES, device=device), word_rules_by_residue(V, device)


WORD_CAP = 2       # median_word_frames of the transcribe cases: max_dur <= 4 frames, so rule 3 has long words to cut
PREV = 98          # the sot_prev token of the conditioned case (test_whisper_condition_cpu's)


def greedy_rows(m, rules, prompt, n_new):
    """decode_rows of naive_word_transcribe: the public greedy decoder on each set of windows"""
    dec = m.with_logit_rules(rules)

    def decode(act, wins):
        pr = prompt.unsqueeze(0).expand(len(act), -1) if prompt.dim() == 1 else torch.stack([prompt[b] for b in act])
        return dec.generate(wins, pr, n_new, rules.eos_token_id).tolist(), [False] * len(act)
    return decode


def recorded_rows(call):
    """decode_rows of naive_word_transcribe for the policies the existing suites pin against their own naive loops (fallback,
    skip, conditioning): `call` runs transcribe WITHOUT word timestamps and with return_log=True; the rows every set of windows
    hands to ops.timestamp_segments (the kept rows, from the sot sequence on) are recorded and replayed -> (decode, transcripts,
    logs)"""
    from mop_amd import ops
    real, sets = ops.timestamp_segments, []
    ops.timestamp_segments = lambda rows, *a, **k: sets.append(rows.tolist()) or real(rows, *a, **k)
    try:
        out, logs = call()
    finally:
        ops.timestamp_segments = real
    it, seen = iter(sets), [0] * len(logs)

    def decode(act, wins):
        skipped = [logs[b].skipped[seen[b]] for b in act]
        for b in act:
            seen[b] += 1
        return next(it), skipped
    return decode, out, logs


def check_word_case(m, clips, prompt, rules, wrules, what, n_new=12, window=40, cap=WORD_CAP, decode=None, **kw):
    """transcribe(word_timestamps=True, **kw) against the naive host loop: every integer equal, probs within the bound, the
    Transcripts those of the same call without word timestamps -> (words, what the naive loop counted)"""
    d = m.with_logit_rules(rules)
    bare = d.transcribe(clips, prompt, n_new, window=window, **kw)
    if decode is None:
        decode, _, logs = recorded_rows(lambda: d.transcribe(clips, prompt, n_new, window=window, return_log=True, **kw))
    want, trace = naive_word_transcribe(m, clips, prompt, rules, wrules, n_new, window, cap, decode)
    got, words = d.transcribe(clips, prompt, n_new, window=window, word_timestamps=True, word_rules=wrules, median_word_frames=cap, **kw)
    for g, b in zip(got, bare):
        assert all(torch.equal(x, y) for x, y in zip(g, b)), what
    assert_transcript_words(words, got, want, what)
    return words, trace


def check_greedy_word_case(m, clips, prompt, rules, wrules, n_new=12, window=40):
    """the greedy case; the naive result must show a window of >= 3 words, an absorbed prepended and appended mark and a
    truncation, or the comparison proves little"""
    words, trace = check_word_case(m, clips, prompt, rules, wrules, "greedy", n_new, window, decode=greedy_rows(m, rules, prompt, n_new))
    assert trace.get("words", 0) >= 3 and trace.get("prepended", 0) >= 1 and trace.get("appended", 0) >= 1, trace
    assert trace.get("truncated", 0) >= 1 and trace["windows"] >= 5, trace
    return words, trace


def check_policy_word_cases(m, clips, prompt, rules, wrules, window=40):
    """one fallback run with a skipped window, and condition_on_previous_text=True"""
    from test_whisper_fallback_cpu import NO_SPEECH
    from statistics import median
    d = m.with_logit_rules(rules)
    _, base = d.transcribe(clips, prompt, 12, window=window, return_log=True, no_speech_token_id=NO_SPEECH)
    ns, lp = median([p for g in base for p in g.no_speech_prob]), median([a for g in base for a in g.avg_logprob])
    kw = dict(temperatures=(0.0, 0.5), logprob_threshold=lp, no_speech_threshold=ns, no_speech_token_id=NO_SPEECH, seed=3)
    d_kw = dict(kw, return_log=True)
    _, logs = d.transcribe(clips, prompt, 12, window=window, **d_kw)
    assert any(t > 0 for g in logs for t in g.temperature) and any(s for g in logs for s in g.skipped), logs
    _, trace = check_word_case(m, clips, prompt, rules, wrules, "fallback and skip", window=window, **kw)
    assert trace["skipped"] >= 1 and trace.get("words", 0) >= 1, trace
    _, trace = check_word_case(m, clips, prompt, rules, wrules, "conditioned", window=window, condition_on_previous_text=True,
                               sot_prev_token_id=PREV, max_prompt_tokens=6)
    assert trace.get("words", 0) >= 1, trace


def test_transcribe_words_equal_the_naive_loop(torch_cores):                               # noqa: F811
    m, clips, prompt, rules, wrules = words_setup()
    words, trace = check_greedy_word_case(m, clips, prompt, rules, wrules)
    print("greedy:", trace, [len(w.starts) for w in words])
    check_policy_word_cases(m, clips, prompt, rules, wrules)
    # with the log, per-item prompts in int32, two frames per timestamp step, no cap
    d = m.with_logit_rules(rules)
    mel = torch.randn(2, 90, 10)
    prompts = torch.tensor([[7, 8, 9], [9, 8, 7]], dtype=torch.int32)
    want, _ = naive_word_transcribe(m, list(mel), prompts, rules, wrules, 9, 24, None, greedy_rows(m, rules, prompts, 9), f=2)
    got, logs, words = d.transcribe(mel, prompts, 9, window=24, frames_per_timestamp=2, return_log=True, word_timestamps=True,
                                    word_rules=wrules)
    assert len(logs) == 2
    assert_transcript_words(words, got, want, "per-item prompts")


def test_defaults_run_todays_path(torch_cores, monkeypatch):               # noqa: F811
    from mop_amd import ops
    m, clips, prompt, rules, wrules = words_setup()
    calls, shapes = [], []
    monkeypatch.setattr(ops, "alignment_rows", lambda *a, **k: calls.append("alignment_rows") or ops.alignment_rows_torch(*a, **k))
    monkeypatch.setattr(ops, "word_spans", lambda *a, **k: calls.append("word_spans") or ops.word_spans_torch(*a, **k))
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (shapes.append(tuple(t.shape)) if t.dim() == 2 and t.dtype == torch.int32
                                                          else None) or real(t))
    ops.LAST_PATH.pop("word_spans", None)
    ops.LAST_PATH.pop("alignment_rows", None)
    d = m.with_logit_rules(rules)
    out = d.transcribe(clips, prompt, 12, window=40, word_rules=wrules, median_word_frames=3)       # word_timestamps stays False
    assert isinstance(out, list) and not calls and "word_spans" not in ops.LAST_PATH and "alignment_rows" not in ops.LAST_PATH
    assert shapes and all(s[1] == 3 for s in shapes), shapes               # the download stays (A, 3)
    shapes.clear()
    d.transcribe(clips, prompt, 12, window=40, word_timestamps=True, word_rules=wrules)
    assert "alignment_rows" in calls and "word_spans" in calls and shapes and all(s[1] == 4 for s in shapes), (calls, shapes)


def test_word_value_errors(torch_cores):                                   # noqa: F811
    from mop_amd import ops
    from mop_amd.nn import LogMelFrontend
    m, clips, prompt, rules, wrules = words_setup()
    d = m.with_logit_rules(rules)
    no_nots = ops.LogitRules(V, **{**RULES, "no_timestamps_token_id": None})
    ok = dict(window=40, word_timestamps=True, word_rules=wrules)
    for kw, rl in ((dict(ok, word_rules=None), rules), (dict(ok, word_rules=word_rules_by_residue(V + 1)), rules),
                   (dict(ok, word_rules=wrules.table), rules), (ok, no_nots), (dict(ok, word_timestamps=1), rules),
                   (dict(ok, alignment_heads=[]), rules), (dict(ok, alignment_heads=[(2, 0)]), rules),
                   (dict(ok, alignment_heads=[(0, 0, 0)]), rules), (dict(ok, medfilt_width=4), rules),
                   (dict(ok, medfilt_width=0), rules), (dict(ok, median_word_frames=-1), rules),
                   (dict(ok, median_word_frames=1.5), rules), (dict(ok, median_word_frames=True), rules)):
        with pytest.raises(ValueError):
            m.with_logit_rules(rl).transcribe(clips, prompt, 12, **kw)
    with pytest.raises(ValueError, match="n_text_ctx"):                    # 3 + 60 + 2 > 64, while 3 + 60 fits the decoders
        d.transcribe(clips, prompt, 60, **ok)
    mel, seqs = torch.randn(2, 40, 10), torch.randint(0, 90, (2, 12))
    small = word_rules_by_residue(100)
    m2 = _tiny_model()
    m2.align_words(mel, seqs, 3, small)
    for args, kw in (((mel, seqs, 3, None), {}), ((mel, seqs, 3, wrules), {}), ((mel, seqs, 10, small), {}), ((mel, seqs[:, :5], 3, small), {}),
                     ((mel, seqs, 3, small, [(5, 0)]), {}), ((mel, seqs, 3, small, None, 2), {}),
                     ((mel, seqs, 3, small, None, 7, -1), {}), ((mel, seqs, 3, small, None, 7, 2.0), {}),
                     ((mel, seqs, 3, small), dict(eot_token_id=1)), ((mel, seqs, 3, small), dict(eot_token_id=101)),
                     ((mel, seqs, 3, small), dict(eot_token_id=True)), ((mel, seqs.float(), 3, small), {})):
        with pytest.raises(ValueError):
            m2.align_words(*args, **kw)
    # transcribe_audio fills Whisper's 0.7 s in
    fe = LogMelFrontend(n_mels=10)
    seen = {}
    orig = m._transcribe
    m._transcribe = lambda *a, **k: seen.update(k) or orig(*a, **k)
    audio = torch.randn(2, 160 * 50)
    m.transcribe_audio(audio, fe, prompt, rules, 8, window=40, word_timestamps=True, word_rules=wrules)
    assert seen["median_word_frames"] == round(0.7 / fe.frame_seconds) == 70
    m.transcribe_audio(audio, fe, prompt, rules, 8, window=40, word_timestamps=True, word_rules=wrules, median_word_frames=5)
    assert seen["median_word_frames"] == 5
    seen.clear()
    m.transcribe_audio(audio, fe, prompt, rules, 8, window=40)
    assert "median_word_frames" not in seen
