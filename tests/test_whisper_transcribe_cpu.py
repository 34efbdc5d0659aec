"""CPU checks of long-form transcription (no GPU): ops.timestamp_segments_torch against a per-row Python restatement of the
segment and seek rules (hand-built rows for every branch, random rows over {text, a few timestamps, eos}, a sweep of shapes, a
padded row stride), every ValueError of the op and of WhisperMoP.transcribe, the support
query and bad-argument returns of mopk_timestamp_segments (no launch), and transcribe with every core routed through its torch
composition against a naive loop over the same public decoders parsed by the restatement."""
import ctypes as C
import inspect
import random

import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _params, _tiny_model

TB, EOS, V = 101, 97, 131
SWEEP_S, SWEEP_T0, SWEEP_R, SWEEP_F = (1, 2, 5, 63, 64, 65, 445), (0, 3), (1, 3, 16), (1, 2)
PROMPT = [EOS, TB + 5, 3]                      # columns before t0 are never looked at: an eos and a timestamp sit there


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ the restatement
def ref_row(row, t0, w, tb, eos, f):
    """one row, in the order of the rules -> (list of (start, end, tok_begin, tok_end), advance)"""
    T, w = len(row), max(w, 1)
    e = T
    for c in range(t0, T):
        if row[c] == eos:
            e = c
            break
    g = row[t0:e]
    n = len(g)
    ts = [x >= tb for x in g]
    segs = []
    if n == 0:                                                             # rule 1
        adv = w
    else:
        single_end = n >= 2 and not ts[n - 2] and ts[n - 1]                # rule 2
        cs = [i for i in range(1, n) if ts[i - 1] and ts[i]]               # rule 3
        if cs:                                                             # rule 4
            p = 0
            for c in cs + ([n] if single_end else []):
                segs.append(((g[p] - tb) * f if ts[p] else 0, (g[c - 1] - tb) * f, t0 + p, t0 + c))
                p = c
            adv = w if single_end else (g[cs[-1] - 1] - tb) * f
        else:                                                              # rule 5
            end = w
            stamps = [x for x in g if x >= tb]
            if stamps and stamps[-1] != tb:
                end = (stamps[-1] - tb) * f
            segs.append((0, end, t0, t0 + n))
            adv = w
    return segs, min(max(adv, 1), w)                                       # rule 6


def ref_segments(rows, t0, window, tb, eos, f=1):
    """rows: list of R lists of T ints; window: list of R ints -> (starts, ends, tok_begin, tok_end (R, T - t0), n_segments,
    advance (R,)) as int32 tensors"""
    S = len(rows[0]) - t0
    cols, ns, advs = [[], [], [], []], [], []
    for row, w in zip(rows, window):
        segs, adv = ref_row(row, t0, w, tb, eos, f)
        for k in range(4):
            cols[k].append([s[k] for s in segs] + [-1] * (S - len(segs)))
        ns.append(len(segs))
        advs.append(adv)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)                     # noqa: E731
    return tuple(i32(c) for c in cols) + (i32(ns), i32(advs))


def assert_segments_equal(got, want, what=None):
    for name, g, w in zip(("starts", "ends", "tok_begin", "tok_end", "n_segments", "advance"), got, want):
        assert g.dtype == torch.int32 and g.shape == w.shape, (what, name, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.cpu(), w), (what, name, g.cpu().tolist(), w.tolist())


# ------------------------------------------------------------------ rows
t, a, b, c, d = 5, TB, TB + 3, TB + 7, TB + 11                              # a text token and four timestamps
HAND = [                                                                   # (name, generated columns, window)
    ("n = 0", [EOS, EOS, EOS], 40),
    ("eos in the first generated column, tokens behind it", [EOS, t, b, b], 40),
    ("n = 1 text", [t, EOS], 40),
    ("n = 1 timestamp", [b, EOS], 40),
    ("n = 1 timestamp tb", [a, EOS], 40),
    ("a lone final timestamp after text, no pair", [t, t, c, EOS], 40),
    ("no timestamp at all", [t, t, t, EOS], 40),
    ("timestamps, no pair, the last one tb", [a, t, t, EOS], 40),
    ("timestamps, no pair, the last one not tb", [b, t, t, EOS], 40),
    ("timestamps, no pair, two of them", [a, t, b, t, EOS], 40),
    ("one pair", [a, t, t, c, c, EOS], 40),
    ("several pairs, trailing text dropped", [a, t, b, b, t, t, c, c, t, t, EOS], 40),
    ("pairs and single_end", [a, t, b, b, t, t, d, EOS], 40),
    ("a pair that closes the row, no single_end", [a, t, b, b, EOS], 40),
    ("degenerate a a b b", [b, b, c, c, EOS], 40),
    ("g[0] text, then a pair", [t, t, b, b, t, EOS], 40),
    ("the last pair at tb: advance clamps to 1", [a, a, t, EOS], 40),
    ("a timestamp beyond the window: advance clamps to it", [a, t, TB + 50, TB + 50, EOS], 40),
    ("no eos, pairs", [a, t, b, b, t], 40),
    ("no eos, no pair", [t, t, t], 40),
    ("no eos, single_end", [a, b, b, t, c], 40),
    ("window 0 counts as 1", [t, EOS], 0),
    ("window 1", [a, t, b, b, EOS], 1),
    ("a negative id is text", [-4, b, b, EOS], 40),
]


def hand_cases():
    """-> (name, rows (1, T) list, t0, window list)"""
    for name, g, w in HAND:
        for t0 in (0, 3):
            yield f"{name}, t0 = {t0}", [PROMPT[:t0] + g], t0, [w]


def random_rows(R, S, t0, seed):
    """R rows over {text, seven timestamps, eos}; the eos rate differs per row, so short and full rows both occur"""
    rng = random.Random(seed)
    rows = []
    for _ in range(R):
        p_eos = rng.choice((0.0, 0.01, 0.1, 0.4))
        p_ts = rng.choice((0.15, 0.4, 0.7))
        row = list(PROMPT[:t0])
        for _ in range(S):
            u = rng.random()
            row.append(EOS if u < p_eos else (TB + rng.randrange(7) if u < p_eos + p_ts else rng.randrange(EOS)))
        rows.append(row)
    return rows, [rng.randrange(1, 50) for _ in range(R)]


def sweep_cases(S):
    """the shapes of the sweep at T - t0 = S -> (name, rows, t0, window, f)"""
    for t0 in SWEEP_T0:
        for R in SWEEP_R:
            for f in SWEEP_F:
                rows, window = random_rows(R, S, t0, seed=1000 * S + 100 * t0 + 10 * R + f)
                yield f"S = {S}, t0 = {t0}, R = {R}, f = {f}", rows, t0, window, f


def tensors(rows, window, device="cpu", pad=0):
    """(tokens (R, T) int32 with a row stride of T + pad, window (R,) int32)"""
    tok = torch.tensor(rows, dtype=torch.int32)
    if pad:
        big = torch.full((tok.shape[0], tok.shape[1] + pad), TB + 1, dtype=torch.int32)
        big[:, :tok.shape[1]] = tok
        tok = big.to(device)[:, :tok.shape[1]]
    return tok.to(device), torch.tensor(window, dtype=torch.int32, device=device)


# ------------------------------------------------------------------ the op on the torch path
def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import Transcript, WhisperMoP
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    sig = dict(tokens=(e, P), t0=(e, P), window=(e, P), timestamp_begin=(e, P), eos_token_id=(e, P), frames_per_timestamp=(1, P))
    for fn in (ops.timestamp_segments, ops.timestamp_segments_torch, ops.timestamp_segments_supported):
        assert _params(fn) == sig, fn.__name__
    assert ops.TimestampSegments._fields == ("starts", "ends", "tok_begin", "tok_end", "n_segments", "advance")
    assert _params(WhisperMoP.transcribe) == dict(mel=(e, P), prompt_ids=(e, P), logit_rules=(e, P), max_new_tokens=(e, P),
                                                  window=(None, K), frames_per_timestamp=(1, K), num_beams=(1, K),
                                                  length_penalty=(1.0, K), graph=(False, K))
    assert Transcript._fields == ("starts", "ends", "tokens", "offsets")


def test_restatement_on_hand_built_rows():
    from mop_amd import ops
    for name, rows, t0, window in hand_cases():
        for f in (1, 2):
            tok, win = tensors(rows, window)
            assert_segments_equal(ops.timestamp_segments_torch(tok, t0, win, TB, EOS, f), ref_segments(rows, t0, window, TB, EOS, f),
                                  f"{name}, f = {f}")


def test_hand_built_rows_mean_what_their_names_say():
    """the restatement itself, on the rows whose answer is easy to state"""
    by = {name: ref_row(g, 0, w, TB, EOS, 1) for name, g, w in HAND}
    assert by["n = 0"] == ([], 40) and by["n = 1 text"] == ([(0, 40, 0, 1)], 40)
    assert by["n = 1 timestamp"] == ([(0, 3, 0, 1)], 40) and by["n = 1 timestamp tb"] == ([(0, 40, 0, 1)], 40)
    assert by["one pair"] == ([(0, 7, 0, 4)], 7)
    assert by["several pairs, trailing text dropped"] == ([(0, 3, 0, 3), (3, 7, 3, 7)], 7)
    assert by["pairs and single_end"] == ([(0, 3, 0, 3), (3, 11, 3, 7)], 40)
    assert by["degenerate a a b b"] == ([(3, 3, 0, 1), (3, 3, 1, 2), (7, 7, 2, 3)], 7)
    assert by["g[0] text, then a pair"] == ([(0, 3, 0, 3)], 3)
    assert by["the last pair at tb: advance clamps to 1"] == ([(0, 0, 0, 1)], 1)
    assert by["a timestamp beyond the window: advance clamps to it"] == ([(0, 50, 0, 3)], 40)
    assert by["window 0 counts as 1"] == ([(0, 1, 0, 1)], 1)


@pytest.mark.parametrize("S", SWEEP_S)
def test_restatement_on_random_rows(S):
    from mop_amd import ops
    for name, rows, t0, window, f in sweep_cases(S):
        tok, win = tensors(rows, window)
        assert_segments_equal(ops.timestamp_segments_torch(tok, t0, win, TB, EOS, f), ref_segments(rows, t0, window, TB, EOS, f), name)


def test_padded_row_stride_other_dtypes_and_the_public_op_on_cpu():
    from mop_amd import _lib, ops
    rows, window = random_rows(5, 37, 3, seed=7)
    want = ref_segments(rows, 3, window, TB, EOS, 2)
    tok, win = tensors(rows, window, pad=6)
    assert tok.stride(0) == 46
    assert_segments_equal(ops.timestamp_segments_torch(tok, 3, win, TB, EOS, 2), want, "padded")
    assert_segments_equal(ops.timestamp_segments_torch(tok.long(), 3, win.long(), TB, EOS, 2), want, "int64")
    assert not ops.timestamp_segments_supported(tok, 3, win, TB, EOS, 2)                   # CPU tensors take the torch path
    assert_segments_equal(ops.timestamp_segments(tok, 3, win, TB, EOS, 2), want, "public")
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_GENERIC


def test_op_value_errors():
    from mop_amd import ops
    tok, win = tensors([[1, 2, 3, 4]] * 2, [40, 40])
    ok = (tok, 1, win, TB, EOS, 1)
    bad = [(0, tok.float()), (0, tok[0]), (0, tok[:, :0]), (0, [[1, 2]]), (0, tok.bool()), (1, -1), (1, 4), (1, 1.0), (1, True),
           (2, win[:1]), (2, win.float()), (2, [40, 40]), (2, win.view(2, 1)), (3, EOS), (3, 2 ** 31), (3, 101.0), (4, -1), (4, TB),
           (4, None), (5, 0), (5, 1.5), (5, True), (5, 2 ** 31)]
    for fn in (ops.timestamp_segments, ops.timestamp_segments_torch, ops.timestamp_segments_supported):
        fn(*ok)
        for i, v in bad:
            args = list(ok)
            args[i] = v
            with pytest.raises(ValueError):
                fn(*args)


# ------------------------------------------------------------------ ABI
FIELDS = ["R", "T", "T0", "tb", "eos", "f", "tokens", "tokens_ld", "window", "starts", "ends", "tok_begin", "tok_end", "n_segments",
          "advance"]


def _args(S=445, T0=3, R=4):
    from mop_amd import _lib
    assert FIELDS == [f for f, _ in _lib.TimestampSegmentsArgs._fields_]
    a = _lib.TimestampSegmentsArgs()
    a.R, a.T, a.T0, a.tb, a.eos, a.f, a.tokens_ld = R, T0 + S, T0, TB, EOS, 1, T0 + S
    for f in FIELDS[6:]:
        if f != "tokens_ld":
            setattr(a, f, 4096)                                            # aligned stand-ins: the queries never dereference them
    return a


def test_support_query_and_bad_arguments_need_no_gpu(lib):
    a = _args()
    assert lib.mopk_timestamp_segments_supported(C.byref(a)) == 1
    for field, v in (("R", 0), ("T", 0), ("T0", -1), ("T0", 448), ("tokens_ld", 447), ("eos", -1), ("eos", TB), ("f", 0),
                     ("T", 3 + 1025), ("tokens", 2), ("window", 2), ("starts", 2), ("ends", 2), ("tok_begin", 2), ("tok_end", 2),
                     ("n_segments", 2), ("advance", 2)):
        keep = getattr(a, field)
        setattr(a, field, v)
        if field == "T":
            a.tokens_ld = max(v, 1)
        assert lib.mopk_timestamp_segments_supported(C.byref(a)) == 0, field
        assert lib.mopk_timestamp_segments(C.byref(a), None) < 0, field
        setattr(a, field, keep)
        a.tokens_ld = a.T
    a = _args(S=1024)
    assert lib.mopk_timestamp_segments_supported(C.byref(a)) == 1
    a.window = None
    assert lib.mopk_timestamp_segments(C.byref(a), None) == -2            # null pointers: refused before any launch
    assert lib.mopk_timestamp_segments_supported(None) == 0 and lib.mopk_timestamp_segments(None, None) < 0


# ------------------------------------------------------------------ the model
CLIPS = (100, 40, 17)                          # several windows, exactly one window, shorter than one
RULES = dict(suppress_tokens=[1, 2], suppress_at_begin=[5, EOS], timestamp_begin=TB, eos_token_id=EOS, no_timestamps_token_id=100,
             max_initial_timestamp_index=4)


def transcribe_model(seed=0):
    m = _tiny_model(vocab_size=V)
    torch.manual_seed(seed)
    with torch.no_grad():                      # at the default init every logit gap is ~1e-2: widen them
        m.dec_ln_f.weight.mul_(20.0)
        for p in m.decoder.parameters():
            if p.dim() == 2:
                p.add_(torch.randn_like(p) * 0.05)
    return m


def naive_transcribe(m, clips, prompt, rules, n_new, window, f, num_beams, graph=False):
    """the loop written out: the same public decoders on the same windows and active sets, each row parsed on the host by
    ref_segments -> (per item (starts, ends, tokens, offsets) as lists, per item list of (advance, window length), seeks)"""
    B, T_p = len(clips), prompt.shape[-1]
    dec = m.with_logit_rules(rules)
    seek, out, log = [0] * B, [([], [], [], [0]) for _ in range(B)], [[] for _ in range(B)]
    while any(seek[b] < clips[b].shape[0] for b in range(B)):
        act = [b for b in range(B) if seek[b] < clips[b].shape[0]]
        wins = [clips[b][seek[b]:seek[b] + window] for b in act]
        pr = prompt.unsqueeze(0).expand(len(act), -1) if prompt.dim() == 1 else torch.stack([prompt[b] for b in act])
        if num_beams > 1:
            rows = dec.beam_search(wins, pr, n_new, num_beams, rules.eos_token_id, 1.0, graph)[0]
        else:
            rows = dec.generate(wins, pr, n_new, rules.eos_token_id, graph)
        rows = rows.tolist()
        for k, b in enumerate(act):
            segs, adv = ref_row(rows[k], T_p, wins[k].shape[0], rules.timestamp_begin, rules.eos_token_id, f)
            st, en, tk, off = out[b]
            for s, e, tb_, te in segs:
                st.append(s + seek[b])
                en.append(e + seek[b])
                tk.extend(rows[k][tb_:te])
                off.append(len(tk))
            log[b].append((adv, wins[k].shape[0]))
            seek[b] += adv
    return out, log, seek


def assert_transcripts_equal(got, want, dtype, what=None):
    from mop_amd.nn import Transcript
    assert len(got) == len(want)
    for b, (g, (st, en, tk, off)) in enumerate(zip(got, want)):
        assert isinstance(g, Transcript), (what, b)
        assert g.starts.dtype == g.ends.dtype == g.offsets.dtype == torch.int32 and g.tokens.dtype == dtype, (what, b)
        assert g.starts.tolist() == st and g.ends.tolist() == en, (what, b, g.starts.tolist(), st, g.ends.tolist(), en)
        assert g.tokens.tolist() == tk and g.offsets.tolist() == off, (what, b, g.tokens.tolist(), tk, g.offsets.tolist(), off)


def check_transcript_shape(g, ordered=True):
    """starts <= ends, offsets consistent and, with `ordered`, segments in the order of their starts (a timestamp past the end of a
    short last window can break that order across windows, so a caller whose run is not pinned leaves it out)"""
    st, en, off = g.starts.tolist(), g.ends.tolist(), g.offsets.tolist()
    assert len(st) == len(en) == len(off) - 1
    assert off[0] == 0 and off[-1] == g.tokens.numel() and all(x < y for x, y in zip(off, off[1:]))
    assert all(0 <= s <= e for s, e in zip(st, en))
    assert not ordered or all(x <= y for x, y in zip(st, st[1:]))


@pytest.mark.parametrize("num_beams", [1, 3])
def test_transcribe_equals_the_naive_loop_with_torch_cores(torch_cores, num_beams):     # noqa: F811
    from mop_amd import ops
    m = transcribe_model()
    torch.manual_seed(11)
    clips = [torch.randn(n, 10) for n in CLIPS]
    prompt = torch.tensor([7, 8, 9])
    rules = ops.LogitRules(V, **RULES)
    want, log, seek = naive_transcribe(m, clips, prompt, rules, 12, 40, 1, num_beams)
    got = m.transcribe(clips, prompt, rules, 12, num_beams=num_beams)
    assert_transcripts_equal(got, want, torch.int64, num_beams)
    for g in got:
        check_transcript_shape(g)
    assert all(s >= n for s, n in zip(seek, CLIPS))
    # the run takes both ways out of a window: a change that loses one fails here
    assert len(log[0]) >= 3, log[0]
    assert any(adv < w for adv, w in log[0]), log[0]                        # a pair cut inside the window
    assert any(adv == w for item in log for adv, w in item), log            # a full-window advance
    # a (B, T, n_mels) tensor, per-item prompts, a shorter window, two frames per timestamp step
    mel = torch.randn(2, 50, 10)
    prompts = torch.tensor([[7, 8, 9], [9, 8, 7]], dtype=torch.int32)
    want, _, seek = naive_transcribe(m, list(mel), prompts, rules, 9, 24, 2, num_beams)
    got = m.transcribe(mel, prompts, rules, 9, window=24, frames_per_timestamp=2, num_beams=num_beams)
    assert_transcripts_equal(got, want, torch.int32, "tensor")
    assert all(s >= 50 for s in seek)


def test_transcribe_value_errors(torch_cores):                             # noqa: F811
    from mop_amd import ops
    m = _tiny_model(vocab_size=V)
    rules = ops.LogitRules(V, **RULES)
    clips, prompt = [torch.randn(100, 10), torch.randn(17, 10)], torch.tensor([7, 8, 9])
    m.transcribe([clips[1]], prompt, rules, 2)
    no_tb = ops.LogitRules(V, suppress_tokens=[1])
    other_v = ops.LogitRules(V + 1, timestamp_begin=TB, eos_token_id=EOS)
    for bad in (lambda: m.transcribe([], prompt, rules, 4), lambda: m.transcribe(None, prompt, rules, 4),
                lambda: m.transcribe(torch.randn(100, 10), prompt, rules, 4), lambda: m.transcribe(torch.randn(2, 0, 10), prompt, rules, 4),
                lambda: m.transcribe([clips[0], torch.randn(0, 10)], prompt, rules, 4),
                lambda: m.transcribe([clips[0], torch.randn(5, 11)], prompt, rules, 4),
                lambda: m.transcribe([clips[0], clips[1].double()], prompt, rules, 4),
                lambda: m.transcribe([clips[0], clips[1].long()], prompt, rules, 4),
                lambda: m.transcribe(clips, prompt.float(), rules, 4), lambda: m.transcribe(clips, prompt[:0], rules, 4),
                lambda: m.transcribe(clips, prompt.view(1, 1, 3), rules, 4), lambda: m.transcribe(clips, prompt.view(1, 3), rules, 4),
                lambda: m.transcribe(clips, [prompt, prompt], rules, 4),
                lambda: m.transcribe(clips, prompt, None, 4), lambda: m.transcribe(clips, prompt, no_tb, 4),
                lambda: m.transcribe(clips, prompt, other_v, 4),
                lambda: m.transcribe(clips, prompt, rules, 0), lambda: m.transcribe(clips, prompt, rules, 62),
                lambda: m.transcribe(clips, prompt, rules, 4.0),
                lambda: m.transcribe(clips, prompt, rules, 4, window=0), lambda: m.transcribe(clips, prompt, rules, 4, window=41),
                lambda: m.transcribe(clips, prompt, rules, 4, window=8.0),
                lambda: m.transcribe(clips, prompt, rules, 4, frames_per_timestamp=0),
                lambda: m.transcribe(clips, prompt, rules, 4, frames_per_timestamp=1.0),
                lambda: m.transcribe(clips, prompt, rules, 4, num_beams=0), lambda: m.transcribe(clips, prompt, rules, 4, num_beams=9),
                lambda: m.transcribe(clips, prompt, rules, 4, num_beams=2.0),
                lambda: m.transcribe(clips, prompt, rules, 4, num_beams=2, length_penalty="1"),
                lambda: m.transcribe(clips, prompt, rules, 4, length_penalty=None),
                lambda: m.transcribe(clips, prompt.to("meta"), rules, 4)):
        with pytest.raises(ValueError):
            bad()
