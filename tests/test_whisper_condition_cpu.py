"""CPU checks of transcribe's conditioning on the previous text (no GPU): ops.prompt_history_update_torch and
ops.window_prompts_torch against a per-row Python-list restatement of their rules (hand-built rows for every branch, a random
sweep), every ValueError of both ops and of the new keywords, the support queries and bad-argument returns of both entry points
(no launch; tests/test_abi.py compares the two structs with the header), and transcribe with every core routed through its torch
composition against a naive host loop that keeps Python lists of history and calls the public decoders with list prompts."""
import ctypes as C
import inspect
import random

import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _params, _tiny_model
from test_whisper_fallback_cpu import NO_SPEECH, same
from test_whisper_transcribe_cpu import EOS, RULES, V, assert_transcripts_equal, ref_row, transcribe_model

PREV = 98                                      # the sot_prev token: below the timestamps, not the eos, never produced under RULES' grammar
SWEEP_N, SWEEP_A, SWEEP_TS, SWEEP_T0 = (1, 6, 64, 223, 1024), (1, 3, 16), (1, 3, 4), (0, 3)
NSP_RTOL = 1e-4                                # no_speech_prob of a row alone against the row in a batch, relative: the tolerance of
#                                                tests/test_gpu_whisper_fallback.py for the same probability (1e-5 in its logarithm, with room)


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ the restatement
def ref_history_update(hist, hist_len, rows, t0, n_take, item, mode):
    """hist: B lists of n ints, hist_len: B ints, both changed in place, one row after the other (distinct items)"""
    B, n = len(hist), len(hist[0])
    for a, row in enumerate(rows):
        b = item[a]
        if not 0 <= b < B:
            continue
        if mode[a] == 1:
            hist_len[b] = 0
        elif mode[a] == 0:
            L = min(max(hist_len[b], 0), n)
            m = min(max(n_take[a], 0), len(row) - t0)
            c = hist[b][:L] + row[t0:t0 + m]
            keep = min(n, L + m)
            hist[b][:keep] = c[len(c) - keep:]
            hist_len[b] = keep


def ref_window_prompts(hist, hist_len, item, sot, prev, width):
    """-> (ids: A lists of width ints, kv_start: A ints); sot: a list of ints, or B lists"""
    B, n = len(hist), len(hist[0])
    ids, ks = [], []
    for b in item:
        inside = 0 <= b < B
        bc = min(max(b, 0), B - 1)
        s = sot[bc] if isinstance(sot[0], list) else sot
        L = min(max(hist_len[bc], 0), n) if inside else 0
        room = width - len(s)
        h = min(L, room - 1) if L > 0 and room >= 2 else 0
        own = ([prev] + hist[bc][L - h:L] if h > 0 else []) + s
        ids.append([0] * (width - len(own)) + own)
        ks.append(width - len(own))
    return ids, ks


def state(B, n, lens, seed, device="cpu"):
    """(hist lists, hist_len list, hist tensor, hist_len tensor): every word of hist distinct and negative, so a word that moved
    or stayed is told from a token"""
    hist = [[-(1 + b * n + j) for j in range(n)] for b in range(B)]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=device)      # noqa: E731
    return hist, list(lens), i32(hist), i32(lens)


GUARD, GUARD_FILL = 64, -77


def guarded(t):
    """t's contents in the middle of a buffer of its own with GUARD sentinel words on either side -> (the view, the buffer)"""
    flat = torch.full((t.numel() + 2 * GUARD,), GUARD_FILL, dtype=t.dtype, device=t.device)
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return flat[GUARD:GUARD + t.numel()].view(t.shape), flat


def guards_intact(flat):
    return bool((flat[:GUARD] == GUARD_FILL).all()) and bool((flat[-GUARD:] == GUARD_FILL).all())


def token_rows(A, T, seed):
    rng = random.Random(seed)
    return [[rng.randrange(1, 1 << 20) for _ in range(T)] for _ in range(A)]


def padded(rows, pad, device="cpu"):
    """(A, T) int32 tokens with a row stride of T + pad; the padding holds -5"""
    tok = torch.tensor(rows, dtype=torch.int32)
    if not pad:
        return tok.to(device), None
    big = torch.full((tok.shape[0], tok.shape[1] + pad), -5, dtype=torch.int32)
    big[:, :tok.shape[1]] = tok
    big = big.to(device)
    return big[:, :tok.shape[1]], big


def check_update(fn, B, n, lens, rows, t0, n_take, item, mode, what, device="cpu", pad=0):
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=device)      # noqa: E731
    hist, hl, hist_t, hl_t = state(B, n, lens, 0, device)
    (hist_t, hist_buf), (hl_t, hl_buf) = guarded(hist_t), guarded(hl_t)   # sentinels on either side of the state
    tok, big = padded(rows, pad, device)
    args = (i32(n_take), i32(item), i32(mode))
    keep = [x.clone() for x in args] + [tok.clone()]
    assert fn(hist_t, hl_t, tok, t0, *args) is None, what
    assert guards_intact(hist_buf) and guards_intact(hl_buf), what
    ref_history_update(hist, hl, rows, t0, n_take, item, mode)
    assert hist_t.cpu().tolist() == hist, (what, hist_t.cpu().tolist(), hist)
    assert hl_t.cpu().tolist() == hl, (what, hl_t.cpu().tolist(), hl)
    assert all(torch.equal(x, y) for x, y in zip(keep, args + (tok,))), what          # the inputs are read only
    assert big is None or bool((big[:, tok.shape[1]:] == -5).all()), what
    return hist_t, hl_t


def check_prompts(fn, B, n, lens, item, sot, prev, width, out_dtype, what, device="cpu", sot_dtype=torch.int64):
    hist, hl, hist_t, hl_t = state(B, n, lens, 0, device)
    item_t = torch.tensor(item, dtype=torch.int32, device=device)
    sot_t = torch.tensor(sot, dtype=sot_dtype, device=device)
    before = (hist_t.clone(), hl_t.clone())
    got = fn(hist_t, hl_t, item_t, sot_t, prev, width, out_dtype)
    ids, ks = ref_window_prompts(hist, hl, item, sot, prev, width)
    assert got.ids.dtype == out_dtype and got.ids.shape == (len(item), width) and got.ids.is_contiguous(), what
    assert got.kv_start.dtype == torch.int32 and got.kv_start.shape == (len(item),), what
    assert got.ids.cpu().tolist() == ids, (what, got.ids.cpu().tolist(), ids)
    assert got.kv_start.cpu().tolist() == ks, (what, got.kv_start.cpu().tolist(), ks)
    assert torch.equal(hist_t, before[0]) and torch.equal(hl_t, before[1]), what
    return got


def update_hand_cases():
    """-> (name, B, n, hist_len, rows, t0, n_take, item, mode): every branch of the update's rules"""
    for t0 in SWEEP_T0:
        rows = token_rows(3, t0 + 8, 5 + t0)
        for name, n, lens, take, item, mode in (
                ("append into an empty history", 6, [0, 0, 0, 0], [2, 3, 1], [1, 2, 0], [0, 0, 0]),
                ("append without reaching the cap", 6, [2, 1, 3, 0], [2, 3, 3], [0, 1, 2], [0, 0, 0]),
                ("append exactly to the cap", 6, [2, 1, 3, 0], [4, 5, 3], [0, 1, 2], [0, 0, 0]),
                ("append past the cap: the shift", 6, [5, 6, 3, 6], [4, 1, 8], [0, 1, 3], [0, 0, 0]),
                ("more tokens than the cap: the history leaves entirely", 6, [6, 2, 0, 0], [7, 8, 6], [0, 1, 2], [0, 0, 0]),
                ("n_take 0 and negative: nothing joins", 6, [3, 4, 6, 0], [0, -3, 0], [0, 1, 2], [0, 0, 0]),
                ("n_take beyond the row: clamped to T - t0", 6, [0, 6, 2, 0], [9, 100, 2 ** 31 - 1], [0, 1, 2], [0, 0, 0]),
                ("reset", 6, [3, 6, 0, 2], [4, 4, 4], [0, 1, 2], [1, 1, 1]),
                ("leave", 6, [3, 6, 0, 2], [4, 4, 4], [0, 1, 2], [2, 2, -1]),
                ("the three modes side by side, a shuffled subset", 6, [3, 6, 4, 2], [4, 4, 4], [3, 0, 2], [0, 1, 2]),
                ("items out of range are skipped", 6, [3, 6, 4, 2], [4, 4, 4], [-1, 4, 1], [0, 1, 0]),
                ("hist_len outside [0, n] is clamped", 6, [-2, 9, 4, 2], [2, 2, 2], [0, 1, 3], [0, 0, 0]),
                ("n = 1", 1, [0, 1, 1, 0], [1, 3, 0], [0, 1, 2], [0, 0, 0]),
        ):
            yield f"{name}, t0 = {t0}", 4, n, lens, rows, t0, take, item, mode


def update_sweep_cases(n):
    """the shapes of the sweep at cap n -> (name, B, n, hist_len, rows, t0, n_take, item, mode, pad): hist_len over {0, partial,
    n}, n_take over {negative, 0, 1, n - 1, n, n + 1, beyond T - t0}, the three modes, one item out of range when A > 1"""
    for A in SWEEP_A:
        for t0 in SWEEP_T0:
            rng = random.Random(100 * n + 10 * A + t0)
            B, S = A + 2, min(n + 3, 1024)
            lens = [rng.choice((0, n // 2, n, rng.randrange(n + 1))) for _ in range(B)]
            take = [rng.choice((-2, 0, 1, n - 1, n, n + 1, S + 5)) for _ in range(A)]
            item = rng.sample(range(B), A)
            mode = [rng.choice((0, 0, 0, 1, 2)) for _ in range(A)]
            if A > 1:
                item[rng.randrange(A)] = rng.choice((-1, B, B + 7))
            mode[0] = 0
            yield f"n = {n}, A = {A}, t0 = {t0}", B, n, lens, token_rows(A, t0 + S, n + A), t0, take, item, mode, (0, 5)[A % 2]


def prompt_cases(n):
    """-> (name, B, n, hist_len, item, sot, width): T_s over SWEEP_TS, a shared and a per-item sot, the width exactly needed,
    wider, and narrower down to T_s + 1 and T_s (no history fits)"""
    for A in SWEEP_A:
        for T_s in SWEEP_TS:
            rng = random.Random(100 * n + 10 * A + T_s)
            B = A + 2
            lens = [rng.choice((0, n // 2, n, rng.randrange(n + 1))) for _ in range(B)]
            item = rng.sample(range(B), A)
            lens[item[0]] = n                                              # one full history in the call
            if A > 1:
                lens[item[1]] = 0                                          # and one bare row
                item[-1] = rng.choice((-1, B))
            shared = [900 + k for k in range(T_s)]
            per_item = [[1000 * (b + 1) + k for k in range(T_s)] for b in range(B)]
            need = T_s + 1 + n
            for width in sorted({need, need + 3, max(need - 1, T_s + 1), T_s + 2, T_s + 1, T_s}):
                if width <= 2048:
                    yield f"n = {n}, A = {A}, T_s = {T_s}, width = {width}", B, n, lens, item, (shared, per_item)[width % 2], width


# ------------------------------------------------------------------ the ops on the torch path
def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import WhisperMoP
    from mop_amd.nn.whisper_mop import RuledDecoding
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    sig = dict(hist=(e, P), hist_len=(e, P), tokens=(e, P), t0=(e, P), n_take=(e, P), item=(e, P), mode=(e, P))
    for fn in (ops.prompt_history_update, ops.prompt_history_update_torch, ops.prompt_history_update_supported):
        assert _params(fn) == sig, fn.__name__
    sig = dict(hist=(e, P), hist_len=(e, P), item=(e, P), sot=(e, P), sot_prev_token_id=(e, P), width=(e, P),
               out_dtype=(torch.int64, P))
    for fn in (ops.window_prompts, ops.window_prompts_torch, ops.window_prompts_supported):
        assert _params(fn) == sig, fn.__name__
    assert ops.WindowPrompts._fields == ("ids", "kv_start")
    new = [("condition_on_previous_text", (False, K)), ("initial_prompt", (None, K)), ("sot_prev_token_id", (None, K)),
           ("max_prompt_tokens", (None, K)), ("prompt_reset_temperature", (0.5, K))]
    for fn in (RuledDecoding.transcribe, WhisperMoP._transcribe):
        assert list(_params(fn).items())[-5:] == new, fn.__name__         # the new keywords come last
    assert not any(k in _params(WhisperMoP.transcribe) for k, _ in new)    # the public signature stays


def test_history_update_torch_matches_the_restatement():
    from mop_amd import _lib, ops
    for name, B, n, lens, rows, t0, take, item, mode in update_hand_cases():
        check_update(ops.prompt_history_update_torch, B, n, lens, rows, t0, take, item, mode, name)
    for n in SWEEP_N:
        for name, B, n_, lens, rows, t0, take, item, mode, pad in update_sweep_cases(n):
            check_update(ops.prompt_history_update_torch, B, n_, lens, rows, t0, take, item, mode, name, pad=pad)
    # the public op on CPU tensors takes the torch path; int64 rows and index tensors pass the torch path too
    name, B, n, lens, rows, t0, take, item, mode = next(update_hand_cases())
    check_update(ops.prompt_history_update, B, n, lens, rows, t0, take, item, mode, "public")
    assert ops.LAST_PATH["prompt_history_update"] == _lib.PATH_GENERIC
    hist, hl, hist_t, hl_t = state(B, n, lens, 0)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)                     # noqa: E731
    assert not ops.prompt_history_update_supported(hist_t, hl_t, i64(rows), t0, i64(take), i64(item), i64(mode))
    ops.prompt_history_update_torch(hist_t, hl_t, i64(rows), t0, i64(take), i64(item), i64(mode))
    ref_history_update(hist, hl, rows, t0, take, item, mode)
    assert hist_t.tolist() == hist and hl_t.tolist() == hl


def test_window_prompts_torch_matches_the_restatement():
    from mop_amd import _lib, ops
    # by hand: T_s = 3, n = 6
    sot = [7, 8, 9]
    for name, lens, item, width in (
            ("no history at all: the bare sot", [0, 0, 0], [0, 1, 2], 3),
            ("no history, a wider matrix", [0, 0, 0], [0, 1, 2], 6),
            ("unequal lengths", [6, 2, 0], [0, 1, 2], 10),
            ("equal lengths", [4, 4, 4], [2, 0, 1], 8),
            ("a narrower width keeps the newest tokens", [6, 2, 0], [0, 1, 2], 7),
            ("room for sot_prev and one token", [6, 2, 0], [0, 1, 2], 5),
            ("room for sot_prev alone: the history is dropped", [6, 2, 0], [0, 1, 2], 4),
            ("no room", [6, 2, 0], [0, 1, 2], 3),
            ("a subset, out of order, with an item out of range", [6, 2, 3], [2, -1, 0, 3], 10),
            ("hist_len outside [0, n]", [9, -1, 3], [0, 1, 2], 10),
    ):
        for dt in (torch.int64, torch.int32):
            check_prompts(ops.window_prompts_torch, 3, 6, lens, item, sot, PREV, width, dt, name)
    got = check_prompts(ops.window_prompts_torch, 3, 6, [6, 2, 0], [0, 1, 2], sot, PREV, 10, torch.int64, "example")
    assert got.ids.tolist() == [[PREV, -1, -2, -3, -4, -5, -6, 7, 8, 9], [0, 0, 0, 0, PREV, -7, -8, 7, 8, 9], [0] * 7 + [7, 8, 9]]
    assert got.kv_start.tolist() == [0, 4, 7]
    for n in SWEEP_N:
        for name, B, n_, lens, item, s, width in prompt_cases(n):
            check_prompts(ops.window_prompts_torch, B, n_, lens, item, s, PREV, width, (torch.int64, torch.int32)[width % 2], name,
                          sot_dtype=(torch.int64, torch.int32)[n % 2])
    check_prompts(ops.window_prompts, 3, 6, [6, 2, 0], [0, 1, 2], sot, PREV, 10, torch.int64, "public")
    assert ops.LAST_PATH["window_prompts"] == _lib.PATH_GENERIC


def test_op_value_errors():
    from mop_amd import ops
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)                     # noqa: E731
    hist, hl = torch.zeros(3, 6, dtype=torch.int32), i32([0, 1, 2])
    tok, three = torch.ones(2, 8, dtype=torch.int32), i32([1, 2])
    good = [hist, hl, tok, 3, three, three, three]
    for fn in (ops.prompt_history_update, ops.prompt_history_update_torch, ops.prompt_history_update_supported):
        assert fn(*good) in (None, False)
        for i, v in ((0, hist.long()), (0, hist[:, :5]), (0, hist[0]), (0, hist[:0]), (0, None), (0, hist.to("meta")),
                     (1, hl.long()), (1, hl[:2]), (1, hl.view(3, 1)), (1, None), (1, hl.to("meta")),
                     (2, tok.float()), (2, tok[0]), (2, tok[:, :0]), (2, tok.bool()), (2, None), (2, tok.to("meta")),
                     (3, -1), (3, 8), (3, 1.0), (3, True),
                     (4, three.float()), (4, i32([1, 2, 3])), (4, None), (5, three.view(2, 1)), (5, three.to("meta")),
                     (6, three.bool()), (6, 0)):
            args = list(good)
            args[i] = v
            with pytest.raises(ValueError):
                fn(*args)
    sot = torch.tensor([7, 8, 9])
    good = [hist, hl, three, sot, PREV, 10, torch.int64]
    for fn in (ops.window_prompts, ops.window_prompts_torch, ops.window_prompts_supported):
        fn(*good)
        fn(hist, hl, three, sot, PREV, 3)                                  # width == T_s: allowed
        for i, v in ((0, hist.long()), (0, hist.t()), (0, None), (1, hl[:2]), (1, hl.float()),
                     (2, three.float()), (2, three.view(1, 2)), (2, three[:0]), (2, None), (2, three.to("meta")),
                     (3, sot.float()), (3, sot[:0]), (3, sot.view(1, 1, 3)), (3, sot.view(1, 3).expand(2, 3)), (3, None),
                     (3, sot.to("meta")),
                     (4, None), (4, -1), (4, 2 ** 31), (4, 1.0), (4, True),
                     (5, 2), (5, 10.0), (5, None), (5, True),
                     (6, torch.int16), (6, torch.float32), (6, None)):
            args = list(good)
            args[i] = v
            with pytest.raises(ValueError):
                fn(*args)


# ------------------------------------------------------------------ ABI
UPDATE_FIELDS = ["A", "B", "n", "T", "T0", "reserved", "hist", "hist_len", "tokens", "tokens_ld", "n_take", "item", "mode"]
PROMPT_FIELDS = ["A", "B", "n", "width", "Ts", "prev", "out_i64", "sot_i64", "hist", "hist_len", "item", "sot", "sot_ld", "ids",
                 "kv_start"]


def update_args(n=223, S=445, T0=3, A=4):
    from mop_amd import _lib
    assert UPDATE_FIELDS == [f for f, _ in _lib.PromptHistoryArgs._fields_]
    a = _lib.PromptHistoryArgs()
    a.A, a.B, a.n, a.T, a.T0, a.tokens_ld = A, A + 1, n, T0 + S, T0, T0 + S
    for f in UPDATE_FIELDS[6:]:
        if f != "tokens_ld":
            setattr(a, f, 4096)                                            # aligned stand-ins: the queries never dereference them
    return a


def prompt_args(n=223, width=228, Ts=4, A=4):
    from mop_amd import _lib
    assert PROMPT_FIELDS == [f for f, _ in _lib.WindowPromptsArgs._fields_]
    a = _lib.WindowPromptsArgs()
    a.A, a.B, a.n, a.width, a.Ts, a.prev, a.out_i64, a.sot_i64, a.sot_ld = A, A + 1, n, width, Ts, PREV, 1, 1, 0
    for f in PROMPT_FIELDS[8:]:
        if f != "sot_ld":
            setattr(a, f, 4096)
    return a


def test_support_queries_and_bad_arguments_need_no_gpu(lib):
    a = update_args()
    assert lib.mopk_prompt_history_update_supported(C.byref(a)) == 1
    for field, v in (("A", 0), ("B", 0), ("n", 0), ("n", 1025), ("T", 0), ("T0", -1), ("T0", 448), ("tokens_ld", 447),
                     ("T", 3 + 1025), ("hist", 2), ("hist_len", 2), ("tokens", 2), ("n_take", 2), ("item", 2), ("mode", 2)):
        keep = getattr(a, field)
        setattr(a, field, v)
        if field == "T":
            a.tokens_ld = max(v, 1)
        assert lib.mopk_prompt_history_update_supported(C.byref(a)) == 0, field
        assert lib.mopk_prompt_history_update(C.byref(a), None) < 0, field
        setattr(a, field, keep)
        a.tokens_ld = a.T
    a = update_args(n=1024, S=1024)
    assert lib.mopk_prompt_history_update_supported(C.byref(a)) == 1
    a.mode = None
    assert lib.mopk_prompt_history_update(C.byref(a), None) == -2         # null pointers: refused before any launch
    assert lib.mopk_prompt_history_update_supported(None) == 0 and lib.mopk_prompt_history_update(None, None) < 0

    a = prompt_args()
    assert lib.mopk_window_prompts_supported(C.byref(a)) == 1
    for field, v in (("A", 0), ("B", 0), ("n", 0), ("Ts", 0), ("width", 3), ("width", 2049), ("out_i64", 2), ("sot_i64", -1),
                     ("sot_ld", -1), ("sot_ld", 3), ("hist", 2), ("hist_len", 2), ("item", 2), ("sot", 4), ("ids", 4), ("kv_start", 2)):
        keep = getattr(a, field)
        setattr(a, field, v)
        assert lib.mopk_window_prompts_supported(C.byref(a)) == 0, field
        assert lib.mopk_window_prompts(C.byref(a), None) < 0, field
        setattr(a, field, keep)
    a = prompt_args(width=2048)
    a.out_i64 = a.sot_i64 = 0
    a.sot = a.ids = 4                                                      # 4-byte alignment is enough for int32
    a.sot_ld = 4
    assert lib.mopk_window_prompts_supported(C.byref(a)) == 1
    a.kv_start = None
    assert lib.mopk_window_prompts(C.byref(a), None) == -2
    assert lib.mopk_window_prompts_supported(None) == 0 and lib.mopk_window_prompts(None, None) < 0


# ------------------------------------------------------------------ the model
CLIPS = (100, 40, 17)                          # several windows, exactly one window, shorter than one
N_HIST = 6


def naive_conditioned(m, clips, prompt, rules, n_new, window, *, n, prev=PREV, condition=True, initial_prompt=None, reset_temperature=0.5,
                      temperatures=(0.0,), logprob_threshold=None, no_speech_threshold=None, no_speech_token_id=None, sot_index=0,
                      num_samples=1, seed=0, num_beams=1, length_penalty=1.0, graph=False, stats=False, f=1):
    """transcribe with conditioning written out on the host: Python lists of history, the public decoders with LIST prompts
    ([prev] + history + sot for a clip that has history, sot for one that has none), every row parsed by ref_row -> (per item
    (starts, ends, tokens, offsets) lists, per item a list of (seek, temperature, avg_logprob, no_speech_prob, skipped, the
    clip's prompt length at this window), the prompt lengths of every decoder call, the clips whose history was cut at n).
    stats: decode with return_stats (transcribe does whenever a policy keyword or return_log is set).  The public decoders read
    no_speech_prob at sot_index of each row's OWN prompt, which the history shifts by a different amount per row: the batched
    calls run without a no-speech token and a one-token generate per row reads it at len - T_s + sot_index."""
    B, T_s, eos, nan = len(clips), prompt.shape[-1], rules.eos_token_id, float("nan")
    dec = m.with_logit_rules(rules)
    stats = stats or temperatures != (0.0,) or logprob_threshold is not None or no_speech_token_id is not None
    kw = dict(return_stats=True) if stats else {}
    hist = [[] for _ in range(B)]
    for b in range(B):
        if initial_prompt is not None:
            p = initial_prompt if isinstance(initial_prompt, torch.Tensor) else initial_prompt[b]
            hist[b] = p.tolist()[-n:]
    seek, n_calls = [0] * B, 0
    out, log, widths, cut = [([], [], [], [0]) for _ in range(B)], [[] for _ in range(B)], [], set()

    def prompts_of(todo):
        sot = lambda b: prompt if prompt.dim() == 1 else prompt[b]         # noqa: E731
        pr = [torch.cat([torch.tensor([prev] + hist[b], dtype=prompt.dtype, device=prompt.device), sot(b)]) if hist[b] else sot(b)
              for b in todo]
        widths.append([int(p.shape[0]) for p in pr])
        return pr

    while any(seek[b] < clips[b].shape[0] for b in range(B)):
        act = [b for b in range(B) if seek[b] < clips[b].shape[0]]
        wins = {b: clips[b][seek[b]:seek[b] + window] for b in act}
        final, todo = {}, list(act)
        for ti, t in enumerate(temperatures):
            pr, sub = prompts_of(todo), [wins[b] for b in todo]
            if t == 0 and num_beams > 1:
                res = dec.beam_search(sub, pr, n_new, num_beams, eos, length_penalty, graph, **kw)
                rows = [r.tolist() for r in res[0]]
            elif t == 0:
                res = dec.generate(sub, pr, n_new, eos, graph, **kw)
                rows = [r.tolist() for r in (res[0] if stats else res)]
            else:
                res = dec.sample(sub, pr, n_new, temperature=t, num_samples=num_samples, eos_token_id=eos, seed=seed + n_calls,
                                 graph=graph, **kw)
                n_calls += 1
                every = (res[-1].sum_logprobs / res[-1].n_tokens).tolist()
                best = [e.index(max(e)) for e in every]                    # ties to the smaller index
                rows = [res[0][k][s].tolist() for k, s in enumerate(best)]
            if not stats:
                avg = [nan] * len(todo)
            elif t == 0:
                avg = (res[-1].sum_logprobs / res[-1].n_tokens).tolist()
            else:
                avg = [e[s] for e, s in zip(every, best)]
            again = []
            for k, b in enumerate(todo):
                nsp = nan
                if no_speech_token_id is not None:
                    one = dec.generate([wins[b]], [pr[k]], 1, eos, return_stats=True, no_speech_token_id=no_speech_token_id,
                                       sot_index=int(pr[k].shape[0]) - T_s + sot_index)
                    nsp = float(one[-1].no_speech_prob[0])
                final[b] = (rows[k][len(rows[k]) - n_new - T_s:], t, avg[k], nsp, int(pr[k].shape[0]))
                need = logprob_threshold is not None and avg[k] < logprob_threshold
                if no_speech_threshold is not None and logprob_threshold is not None and nsp > no_speech_threshold and need:
                    need = False
                if need:
                    again.append(b)
            todo = again
            if not todo or ti + 1 == len(temperatures):
                break
        for b in act:
            row, t, avg_b, nsp_b, plen = final[b]                          # row: the sot sequence and the generated tokens
            wlen = wins[b].shape[0]
            skip = no_speech_threshold is not None and nsp_b > no_speech_threshold
            if skip and logprob_threshold is not None and avg_b > logprob_threshold:
                skip = False
            log[b].append((seek[b], t, avg_b, nsp_b, skip, plen))
            if skip:                                                       # neither extended nor cleared
                seek[b] += wlen
                continue
            segs, adv = ref_row(row, T_s, wlen, rules.timestamp_begin, eos, f)
            st_, en, tk, off = out[b]
            for s, e, tb_, te in segs:
                st_.append(s + seek[b])
                en.append(e + seek[b])
                tk.extend(row[tb_:te])
                off.append(len(tk))
            seek[b] += adv
            if not condition or t > reset_temperature:
                hist[b] = []
            else:
                joined = hist[b] + (row[T_s:segs[-1][3]] if segs else [])
                if len(joined) > n:
                    cut.add(b)
                hist[b] = joined[-n:]
    return out, log, widths, cut


def condition_setup(device="cpu"):
    from mop_amd import ops
    m = transcribe_model().to(device)
    torch.manual_seed(1)                       # clips on which the greedy and the 3-beam run both meet a ragged call
    clips = [torch.randn(n, 10).to(device) for n in CLIPS]
    return m, clips, torch.tensor([7, 8, 9], device=device), ops.LogitRules(V, **RULES, device=device)


def check_conditioned_case(m, clips, prompt, rules, window=40, n_new=12, n=N_HIST, dtype=torch.int64, expect_effect=True,
                           run=None, **kw):
    """transcribe(condition_on_previous_text=True, max_prompt_tokens=n) against the naive loop, exactly; the naive run must
    show a call with unequal prompt lengths and a history cut at n, and, with expect_effect, a transcript the unconditioned
    run does not give"""
    want, log, widths, cut = naive_conditioned(m, clips, prompt, rules, n_new, window, n=n, **kw)
    d = m.with_logit_rules(rules)
    call = lambda: d.transcribe(clips, prompt, n_new, window=window, condition_on_previous_text=True,      # noqa: E731
                                sot_prev_token_id=PREV, max_prompt_tokens=n, **kw)
    got = call() if run is None else run(call)                             # run: a caller's wrapper around the one call
    assert_transcripts_equal(got, want, dtype, kw)
    assert any(len(set(w)) > 1 for w in widths), widths                    # a ragged call
    assert cut, widths                                                     # a history cut at n
    assert max(max(w) for w in widths) == prompt.shape[-1] + 1 + n, widths
    if expect_effect:
        bare = d.transcribe(clips, prompt, n_new, window=window, **kw)
        assert any(g.tokens.tolist() != b.tokens.tolist() for g, b in zip(got, bare)), "conditioning changed no transcript"
    return got, log, widths


@pytest.mark.parametrize("num_beams", [1, 3])
def test_conditioned_transcribe_equals_the_naive_loop(torch_cores, num_beams):          # noqa: F811
    m, clips, prompt, rules = condition_setup()
    got, log, widths = check_conditioned_case(m, clips, prompt, rules, num_beams=num_beams)
    assert len(log[0]) >= 3
    # per-item sot sequences in int32, a tensor of clips, two frames per timestamp step, the default cap n_text_ctx // 2 - 1 = 31
    mel = torch.randn(2, 90, 10)
    prompts = torch.tensor([[7, 8, 9], [9, 8, 7]], dtype=torch.int32)
    want, _, widths, _ = naive_conditioned(m, list(mel), prompts, rules, 9, 24, n=31, num_beams=num_beams, f=2)
    got = m.with_logit_rules(rules).transcribe(mel, prompts, 9, window=24, frames_per_timestamp=2, num_beams=num_beams,
                                               condition_on_previous_text=True, sot_prev_token_id=PREV)
    assert_transcripts_equal(got, want, torch.int32, "per-item sot")
    assert max(max(w) for w in widths) > 3 + 1 + N_HIST                    # longer histories than the capped runs keep


def test_initial_prompt(torch_cores):                                      # noqa: F811
    m, clips, prompt, rules = condition_setup()
    d = m.with_logit_rules(rules)
    hint = torch.tensor([11, 12, 13, 14, 15, 16, 17, 18, 19])              # longer than the cap: its last 6 tokens seed the history
    kw = dict(condition_on_previous_text=True, sot_prev_token_id=PREV, max_prompt_tokens=N_HIST)
    want, log, widths, _ = naive_conditioned(m, clips, prompt, rules, 12, 40, n=N_HIST, initial_prompt=hint)
    got = d.transcribe(clips, prompt, 12, initial_prompt=hint, **kw)
    assert_transcripts_equal(got, want, torch.int64, "initial_prompt")
    assert widths[0] == [3 + 1 + N_HIST] * 3                               # the first call: every clip under the hint, a uniform batch
    # one per clip, an empty one among them, one on the prompt's dtype and one not
    hints = [hint[:2], hint[:0], hint.to(torch.int32)]
    want, _, widths, _ = naive_conditioned(m, clips, prompt, rules, 12, 40, n=N_HIST, initial_prompt=hints)
    got = d.transcribe(clips, prompt, 12, initial_prompt=hints, **kw)
    assert_transcripts_equal(got, want, torch.int64, "initial_prompt per clip")
    assert widths[0] == [6, 3, 10]
    # without condition_on_previous_text the hint conditions each clip's first window only
    want, log, widths, _ = naive_conditioned(m, clips, prompt, rules, 12, 40, n=N_HIST, initial_prompt=hint, condition=False)
    got = d.transcribe(clips, prompt, 12, initial_prompt=hint, sot_prev_token_id=PREV, max_prompt_tokens=N_HIST)
    assert_transcripts_equal(got, want, torch.int64, "initial_prompt alone")
    assert widths[0] == [10, 10, 10] and all(w == [3] * len(w) for w in widths[1:]) and len(widths) >= 3
    bare = d.transcribe(clips, prompt, 12)
    assert any(g.tokens.tolist() != b.tokens.tolist() for g, b in zip(got, bare))


def assert_condition_logs_equal(glog, wlog, what=None):
    for b, (g, w) in enumerate(zip(glog, wlog)):
        rows = list(zip(g.seek, g.temperature, g.avg_logprob, g.no_speech_prob, g.skipped))
        assert len(rows) == len(w), (what, b, rows, w)
        for x, y in zip(rows, w):
            assert x[0] == y[0] and x[1] == y[1] and same(x[2], y[2]) and x[4] == y[4], (what, b, x, y)
            assert same(x[3], y[3]) or abs(x[3] - y[3]) <= NSP_RTOL * y[3], (what, b, x, y)       # read in a batch / on the row alone


def run_condition_policy_case(m, clips, prompt, rules, window=40, **kw):
    want, wlog, widths, _ = naive_conditioned(m, clips, prompt, rules, 12, window, n=N_HIST, stats=True, **kw)
    got, glog = m.with_logit_rules(rules).transcribe(clips, prompt, 12, window=window, return_log=True, condition_on_previous_text=True,
                                                     sot_prev_token_id=PREV, max_prompt_tokens=N_HIST, **kw)
    assert_transcripts_equal(got, want, torch.int64, kw)
    assert_condition_logs_equal(glog, wlog, kw)
    return got, wlog, widths


def fallback_threshold(m, clips, prompt, rules, window=40):
    """a logprob threshold that sends some windows up the temperatures and keeps others at 0: the median avg_logprob of the
    clips' first windows at temperature 0, as in tests/test_whisper_fallback_cpu.py (the first windows have no history, as every
    window after a reset has: a median over all windows sits above what a bare prompt reaches, and every window would fall back)"""
    _, log, _ = run_condition_policy_case(m, clips, prompt, rules, window)
    avgs = sorted(g[0][2] for g in log)
    return avgs[len(avgs) // 2]


def check_reset_case(m, clips, prompt, rules, window=40, temperatures=(0.0, 0.4, 0.8), seed=3):
    """the fallback under conditioning: a window kept above 0.5 clears its clip's history (the next prompt is bare), one kept
    at or below 0.5 extends it"""
    thr = fallback_threshold(m, clips, prompt, rules, window)
    _, log, widths = run_condition_policy_case(m, clips, prompt, rules, window, temperatures=temperatures, logprob_threshold=thr,
                                               seed=seed)
    T_s = prompt.shape[-1]
    reset = [(b, i) for b, g in enumerate(log) for i in range(len(g) - 1) if g[i][1] > 0.5]
    grown = [(b, i) for b, g in enumerate(log) for i in range(len(g) - 1) if g[i][1] <= 0.5 and g[i + 1][5] > max(g[i][5], T_s)]
    assert reset and all(log[b][i + 1][5] == T_s for b, i in reset), log   # kept above 0.5: the clip's next prompt is bare
    assert grown, log                                                      # kept at or below 0.5: the history grows
    assert any(len(w) < 3 for w in widths), widths                         # an attempt on some of the rows
    return log


def test_fallback_resets_the_history(torch_cores):                        # noqa: F811
    m, clips, prompt, rules = condition_setup()
    torch.manual_seed(11)
    clips = [torch.randn(n, 10) for n in (130, 100, 90)]                  # four, three and three windows of 40 frames
    check_reset_case(m, clips, prompt, rules)


def test_skipped_window_leaves_the_history(torch_cores):                  # noqa: F811
    m, clips, prompt, rules = condition_setup()
    torch.manual_seed(11)
    clips = [torch.randn(n, 10) for n in (130, 100, 90)]
    _, base, _ = run_condition_policy_case(m, clips, prompt, rules, no_speech_token_id=NO_SPEECH, sot_index=1)
    probs = sorted(p for g in base for _, _, _, p, _, _ in g)
    k = max(range(2, len(probs) - 1), key=lambda i: probs[i] / probs[i - 1])           # the widest gap with two windows on each side
    assert probs[k] / probs[k - 1] > 1 + 100 * NSP_RTOL, probs             # a threshold no rounding moves a window across
    thr = (probs[k] * probs[k - 1]) ** 0.5
    _, log, _ = run_condition_policy_case(m, clips, prompt, rules, no_speech_threshold=thr, no_speech_token_id=NO_SPEECH, sot_index=1)
    skipped = [(b, i) for b, g in enumerate(log) for i in range(len(g) - 1) if g[i][4]]
    assert skipped and not all(w[4] for g in log for w in g), log
    assert all(log[b][i + 1][5] == log[b][i][5] for b, i in skipped), log  # skipped: the next prompt has the same length
    assert any(log[b][i][5] > 3 for b, i in skipped), log                  # ... and one of them had history to lose


def test_defaults_run_todays_path(torch_cores, monkeypatch):              # noqa: F811
    from mop_amd import ops
    m, clips, prompt, rules = condition_setup()
    calls = []
    monkeypatch.setattr(ops, "window_prompts", lambda *a, **k: calls.append("window_prompts") or ops.window_prompts_torch(*a, **k))
    monkeypatch.setattr(ops, "prompt_history_update",
                        lambda *a, **k: calls.append("prompt_history_update") or ops.prompt_history_update_torch(*a, **k))
    d = m.with_logit_rules(rules)
    plain = d.transcribe(clips, prompt, 12)
    spelled = d.transcribe(clips, prompt, 12, condition_on_previous_text=False, initial_prompt=None, sot_prev_token_id=None,
                           max_prompt_tokens=None, prompt_reset_temperature=0.5)
    assert not calls                                                       # no history, no new launch
    for a, b in zip(plain, spelled):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and torch.equal(x, y)
    d.transcribe(clips, prompt, 12, condition_on_previous_text=True, sot_prev_token_id=PREV, max_prompt_tokens=N_HIST)
    n_sets = calls.count("prompt_history_update")
    assert n_sets >= 3 and calls.count("window_prompts") == n_sets         # one of each per set of windows


def test_condition_value_errors(torch_cores):                             # noqa: F811
    m, clips, prompt, rules = condition_setup()
    d = m.with_logit_rules(rules)
    on = dict(condition_on_previous_text=True, sot_prev_token_id=PREV)
    d.transcribe([clips[2]], prompt, 2, **on)
    d.transcribe([clips[2]], prompt, 2, initial_prompt=[prompt[:0]], sot_prev_token_id=PREV)
    d.transcribe([clips[2]], prompt, 28, max_prompt_tokens=32, **on)       # 3 + 1 + 32 + 28 = 64 = n_text_ctx: the last that fits
    with pytest.raises(ValueError, match=r"3 \+ 1 \+ 32 \+ 29 = 65 exceeds n_text_ctx = 64"):
        d.transcribe([clips[2]], prompt, 29, max_prompt_tokens=32, **on)
    with pytest.raises(ValueError, match=r"3 \+ 1 \+ 31 \+ 30 = 65"):    # the default cap, n_text_ctx // 2 - 1
        d.transcribe([clips[2]], prompt, 30, **on)
    hint = torch.tensor([11, 12])
    for kw in (dict(condition_on_previous_text=True), dict(initial_prompt=hint),
               dict(condition_on_previous_text=True, sot_prev_token_id=V), dict(condition_on_previous_text=True, sot_prev_token_id=-1),
               dict(condition_on_previous_text=True, sot_prev_token_id=1.0), dict(condition_on_previous_text=True, sot_prev_token_id=True),
               dict(sot_prev_token_id=V), dict(condition_on_previous_text=1, sot_prev_token_id=PREV),
               dict(max_prompt_tokens=0, **on), dict(max_prompt_tokens=-3, **on), dict(max_prompt_tokens=6.0, **on),
               dict(max_prompt_tokens=True, **on), dict(max_prompt_tokens=0),
               dict(initial_prompt=hint.float(), **on), dict(initial_prompt=hint.view(1, 2), **on), dict(initial_prompt=[hint], **on),
               dict(initial_prompt=[hint, hint, None], **on), dict(initial_prompt=[hint, hint, hint.bool()], **on),
               dict(initial_prompt="a hint", **on), dict(initial_prompt=[11, 12], **on), dict(initial_prompt=[], **on),
               dict(prompt_reset_temperature=None, **on), dict(prompt_reset_temperature="0.5", **on),
               dict(prompt_reset_temperature=float("nan"), **on), dict(prompt_reset_temperature=True, **on),
               dict(prompt_reset_temperature=None)):
        with pytest.raises(ValueError):
            d.transcribe(clips, prompt, 4, **kw)
    tiny = _tiny_model(vocab_size=V, n_text_ctx=3)                         # n_text_ctx // 2 - 1 = 0: no room for previous text
    with pytest.raises(ValueError):
        tiny.with_logit_rules(rules).transcribe([clips[2]], prompt[:1], 1, **on)
