"""CPU checks of the repetition rules (no GPU): ops.repeat_rules_torch against a restatement written here (plain loops and sets
over Python floats, no call into ops) on hand-built rows with stated answers and over a sweep of vocabularies, row counts, dtypes,
n-gram sizes, penalties and histories, bit for bit on every row (nothing here is a near tie); every ValueError; the signatures;
the library's support query; and generate / beam_search / sample / transcribe under the rules
with every core on its torch composition: no repeated bigram, the timestamp grammar intact, and nothing changed without rules."""
import ctypes as C
import inspect
import itertools
import math
import struct

import pytest
import torch

from test_whisper_beam_cpu import _tiny_model
from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_rules_cpu import MODEL_RULES, _peaked_tiny_model, bits, check_grammar

NEG = float("-inf")
T0 = 3                                                       # prompt columns in front of the generated tokens
CAP = T0 + 34                                                # columns of the sweep's histories
NGRAMS, PENALTIES = (0, 1, 2, 3, 5), (1.0, 1.3, 0.8)


def f32(x: float) -> float:
    """x rounded to fp32 (to nearest even), as a Python float"""
    return struct.unpack("f", struct.pack("f", x))[0]


def bf16(x: float) -> float:
    """an fp32 value rounded to bf16 (to nearest even), as a Python float"""
    if x != x or math.isinf(x):
        return x
    u = struct.unpack("I", struct.pack("f", x))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("f", struct.pack("I", u))[0]


def ref_repeat(row, g, V, p, inv_p, s, exempt, to_bf16=False):
    """the rules as the issue states them, for one row: row, the logits as Python floats (each one a value of the logits' dtype);
    g, the generated tokens (raw ints); p and inv_p, the two fp32 constants; exempt, a set of ids -> (the new row, the penalised
    ids, the banned ids).  The product of two fp32 values is exact in a double, so f32() rounds it once, as an fp32 multiply does."""
    out, n = list(row), len(g)
    ok = lambda v: 0 <= v < V and v not in exempt            # noqa: E731
    penalised, banned = set(), set()
    if p != 1.0:
        for v in set(g):
            if ok(v):
                x = row[v]
                y = f32(x * p) if x < 0 else f32(x * inv_p)
                out[v] = bf16(y) if to_bf16 else y
                penalised.add(v)
    if s >= 1 and n >= s - 1:
        ctx = g[n - s + 1:]
        for i in range(0, n - s + 1):
            if g[i:i + s - 1] == ctx and ok(g[i + s - 1]):
                banned.add(g[i + s - 1])
        for v in banned:
            out[v] = NEG
    return out, penalised, banned


def rules_of(V, p, s, device=None):
    from mop_amd import ops
    return ops.RepeatRules(V, p, s, exempt_tokens=(ALPHABET(V)[0],), exempt_from=V - 10, device=device)


def ALPHABET(V):                                             # noqa: N802  the few ids the histories draw from: repeats are common
    return [5, 9, 17, 30, V - 12, V - 3]                     # the first is on the exempt list, the last is exempt by exempt_from


def build_case(V, R, dtype, n, s, seed, device="cpu", cap=CAP, pos=None):
    """(x (R, V) with zeros and -inf planted on tokens of the history, hist (R, cap) int32 drawn from ALPHABET(V) with, per row, a
    planted repeat of the last s - 1 tokens, an id < 0 and an id >= V among the generated tokens, pos (1,) int32 = T0 + n unless
    given).  Every column of hist is filled: a pos past the end reads the tail."""
    gen = torch.Generator().manual_seed(seed)
    al = torch.tensor(ALPHABET(V))
    x = torch.randn(R, V, generator=gen) * 3
    hist = al[torch.randint(0, len(al), (R, cap), generator=gen)].to(torch.int32)
    for r in range(R):
        g = hist[r, T0:]
        if n >= 8:
            g[1] = -5                                        # never a vocabulary entry, still part of the n-grams
            if r % 3 == 1:
                g[3] = V + 3
            if s >= 2 and n >= s + 3:                        # the last s - 1 tokens repeat g[2 : s + 1]: g[s + 1] is banned
                g[n - s + 1:n] = g[2:s + 1].clone()
        x[r, int(al[1 + r % 4])] = (0.0, NEG, -0.0)[r % 3]
    p = T0 + n if pos is None else pos
    return x.to(dtype).to(device), hist.to(device), torch.tensor([p], dtype=torch.int32, device=device)


def sweep_cases():
    """(n-gram size, penalty, generated length or None, pos or None): lengths 0, s - 2, s - 1, s and 30, then both clamps of pos"""
    for s, p in itertools.product(NGRAMS, PENALTIES):
        for n in sorted({0, max(s - 2, 0), max(s - 1, 0), s, 30}):
            yield s, p, n, None
        yield s, p, 30, T0 - 2                               # pos < t0: n = 0
        yield s, p, CAP - T0, CAP + 5                        # pos > T: n = T - t0


def expected(x, hist, pos, rules, t0=T0):
    """the restatement on every row of a case -> (the wanted tensor, per row (penalised, banned) sets)"""
    V, T = x.shape[1], hist.shape[1]
    n = min(max(int(pos) - t0, 0), T - t0)
    ex = set(rules.table("cpu").nonzero().flatten().tolist())
    rows, kinds = [], []
    for r in range(x.shape[0]):
        g = [int(t) for t in hist[r, t0:t0 + n]]
        out, pen, ban = ref_repeat(x[r].float().tolist(), g, V, rules.repetition_penalty, rules.inv_penalty,
                                   rules.no_repeat_ngram_size, ex, x.dtype == torch.bfloat16)
        rows.append(out)
        kinds.append((pen, ban))
    return torch.tensor(rows, dtype=torch.float32).to(x.dtype), kinds


def assert_bits_equal(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = (bits(got) != bits(want)).nonzero()
    assert bad.numel() == 0, (what, bad[:5].tolist())


def sweep(fn, V, R, dtype, device="cpu"):
    """fn(x, hist, pos, T0, rules) against the restatement over sweep_cases() -> how many rows were (banned only, penalised only,
    both, neither)"""
    seen = [0, 0, 0, 0]
    for ci, (s, p, n, pos) in enumerate(sweep_cases()):
        rules = rules_of(V, p, s)
        x, hist, pos_t = build_case(V, R, dtype, n, s, 100 * ci + R, pos=pos)
        want, kinds = expected(x, hist, pos_t, rules)
        got = fn(x.to(device), hist.to(device), pos_t.to(device), T0, rules)
        assert_bits_equal(got, want, (V, R, dtype, s, p, n, pos))
        for pen, ban in kinds:
            seen[3 if not (pen or ban) else 2 if pen and ban else 1 if pen else 0] += 1
    return seen


# ------------------------------------------------------------------ hand-built rows
@pytest.mark.parametrize("g,s,banned", [([1, 2, 3, 1, 2], 3, {3}), ([1, 2, 3, 1, 2], 2, {3}), ([1, 2, 3, 1, 2], 1, {1, 2, 3}),
                                        ([1, 2, 3, 1, 2], 6, set()), ([7, 7, 7], 2, {7}), ([], 1, set()), ([], 2, set()), ([], 4, set())])
def test_ngram_cases_by_hand(g, s, banned):
    from mop_amd import ops
    V = 16
    row = [0.5 * v - 3 for v in range(V)]
    assert ref_repeat(row, g, V, 1.0, 1.0, s, set())[2] == banned
    hist = torch.full((1, 12), 9, dtype=torch.int32)         # the prompt and the tail hold a token of their own: never counted
    hist[0, T0:T0 + len(g)] = torch.tensor(g, dtype=torch.int32)
    x, pos = torch.tensor([row]), torch.tensor([T0 + len(g)], dtype=torch.int32)
    out = ops.repeat_rules_torch(x, hist, pos, T0, ops.RepeatRules(V, 1.0, s))
    assert set(torch.isneginf(out[0]).nonzero().flatten().tolist()) == banned
    keep = ~torch.isneginf(out[0])
    assert torch.equal(bits(out[0][keep]), bits(x[0][keep]))


def test_penalty_exemption_and_ban_by_hand():
    from mop_amd import ops
    V, p = 16, 1.5
    r = ops.RepeatRules(V, p, 2, exempt_tokens=(4,), exempt_from=14)
    assert r.inv_penalty == f32(1 / 1.5) and r.repetition_penalty == 1.5 and not r.neutral
    x = torch.zeros(1, V)
    x[0, :8] = torch.tensor([3.0, -3.0, 0.0, NEG, 6.0, 9.0, -1.5, float("nan")])
    x[0, 14] = 2.0
    #    token: 0 positive, 1 negative, 2 zero, 3 -inf, 4 exempt by list, 14 exempt by range, 5 twice, 7 NaN; 6 follows 5 twice
    g = [0, 1, 2, 3, 4, 14, 5, 6, 7, 5]
    hist = torch.zeros(1, 20, dtype=torch.int32)
    hist[0, T0:T0 + len(g)] = torch.tensor(g, dtype=torch.int32)
    out = ops.repeat_rules_torch(x, hist, torch.tensor([T0 + len(g)], dtype=torch.int32), T0, r)[0]
    assert out[0] == f32(3.0 * r.inv_penalty) and out[1] == -4.5 and out[2] == 0.0 and out[3] == NEG
    assert out[4] == 6.0 and out[14] == 2.0                  # exempt: never penalised
    assert out[5] == f32(9.0 * r.inv_penalty)                # twice in g, penalised once (twice would be 4.0)
    assert out[6] == NEG                                     # ban beats the penalty (-2.25)
    assert math.isnan(out[7]) and torch.equal(out[8:14], x[0, 8:14]) and out[15] == 0.0
    # an exempt token is never banned either: 4 follows 3, and the history ends in 3
    g = [3, 4, 3]
    hist[0, T0:T0 + 3] = torch.tensor(g, dtype=torch.int32)
    out = ops.repeat_rules_torch(x, hist, torch.tensor([T0 + 3], dtype=torch.int32), T0, r)[0]
    assert out[4] == 6.0
    want, pen, ban = ref_repeat(x[0].tolist(), g, V, r.repetition_penalty, r.inv_penalty, 2, {4, 14, 15})
    assert pen == {3} and ban == set() and want[4] == 6.0
    # neutral rules are a valid call: the result is the input
    same = ops.repeat_rules(x, hist, torch.tensor([T0 + 3], dtype=torch.int32), T0, ops.RepeatRules(V))
    assert torch.equal(bits(same[:, :7]), bits(x[:, :7])) and same.data_ptr() != x.data_ptr() and ops.RepeatRules(V).neutral


# ------------------------------------------------------------------ the torch path against the restatement
SEEN = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,R", [(64, 1), (64, 3), (64, 16), (131, 1), (131, 3), (131, 16)])
def test_torch_path_matches_the_restatement(V, R, dtype):
    from mop_amd import ops
    SEEN[V, R, dtype] = sweep(ops.repeat_rules_torch, V, R, dtype)


def test_the_sweep_reaches_every_branch():
    from mop_amd import ops
    seen = SEEN.get((131, 16, torch.float32)) or sweep(ops.repeat_rules_torch, 131, 16, torch.float32)
    print(f"rows banned only / penalised only / both / neither: {seen}")
    assert all(k >= 16 for k in seen), seen
    # and inside one row: a token both penalised and banned, one only penalised, an id outside the vocabulary among the n-grams
    x, hist, pos = build_case(131, 3, torch.float32, 30, 3, 7)
    _, kinds = expected(x, hist, pos, rules_of(131, 1.3, 3))
    assert all(ban <= pen for pen, ban in kinds) and any(ban and pen - ban for pen, ban in kinds)     # a banned token was penalised first
    assert int(hist[1, T0 + 3]) == 134 and int(hist[0, T0 + 1]) == -5


def test_out_buffer_aliasing_and_strides_on_the_torch_path():
    from mop_amd import ops
    V = 131
    rules = rules_of(V, 1.3, 3)
    x, hist, pos = build_case(V, 4, torch.float32, 30, 3, 3)
    want = ops.repeat_rules_torch(x, hist, pos, T0, rules)
    assert_bits_equal(want, expected(x, hist, pos, rules)[0], "plain")
    assert bool((bits(want) != bits(x)).any())
    wide = torch.full((4, V + 5), 7.0)
    wide[:, :V] = x
    big = hist.repeat_interleave(3, 0)
    got = ops.repeat_rules_torch(wide[:, :V], big[::3], pos, T0, rules, out=wide[:, :V])
    assert got.data_ptr() == wide.data_ptr() and torch.equal(bits(wide[:, :V]), bits(want)) and bool((wide[:, V:] == 7.0).all())
    other = torch.empty(4, V)
    assert ops.repeat_rules_torch(x, hist, pos, T0, rules, out=other) is other and torch.equal(bits(other), bits(want))
    assert torch.equal(bits(ops.repeat_rules(x, hist, pos, T0, rules)), bits(want))
    assert ops.LAST_PATH["repeat_rules"] == 1                # CPU: the torch path
    one = ops.repeat_rules_torch(x[2:3].expand(1, V), hist[2:3], pos, T0, rules)
    assert torch.equal(bits(one), bits(want[2:3]))


# ------------------------------------------------------------------ arguments, signatures, the struct
def test_argument_errors():
    from mop_amd import ops
    from mop_amd.nn import RepeatRules
    assert RepeatRules is ops.RepeatRules
    V = 100
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.2), dict(repetition_penalty=float("inf")),
               dict(repetition_penalty=float("nan")), dict(repetition_penalty=None), dict(repetition_penalty=1e-60),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(no_repeat_ngram_size=True),
               dict(exempt_tokens=[100]), dict(exempt_tokens=[-1]), dict(exempt_tokens=[2.5]), dict(exempt_from=101),
               dict(exempt_from=-1), dict(exempt_from=3.5)):
        with pytest.raises(ValueError):
            RepeatRules(V, **kw)
    with pytest.raises(ValueError):
        RepeatRules(1)
    with pytest.raises(ValueError):
        RepeatRules.for_whisper("rules")
    r = RepeatRules(V, 1.2, 3, exempt_tokens=(3, 4), exempt_from=98)
    t = r.table("cpu")
    assert t.dtype == torch.uint8 and t.shape == (V,) and t.nonzero().flatten().tolist() == [3, 4, 98, 99] and r.table("cpu") is t
    assert r.inv_penalty == f32(1 / f32(1.2)) and r.repetition_penalty == f32(1.2) and r.no_repeat_ngram_size == 3
    assert RepeatRules(V, exempt_from=V).table("cpu").sum() == 0 and RepeatRules(V, exempt_from=0).table("cpu").sum() == V
    lr = ops.LogitRules(V, **MODEL_RULES)
    w = RepeatRules.for_whisper(lr, 1.1, 2, extra_exempt=(6,))
    assert w.table("cpu").nonzero().flatten().tolist() == [6, 70] + list(range(80, 100)) and w.no_repeat_ngram_size == 2
    assert RepeatRules.for_whisper(ops.LogitRules(V)).table("cpu").sum() == 0 and RepeatRules.for_whisper(lr).neutral
    x, hist, pos = torch.zeros(2, V), torch.zeros(2, 8, dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    for f in (ops.repeat_rules, ops.repeat_rules_torch, ops.repeat_rules_supported):
        for args in ((x[:, :50], hist, pos, 3, r), (x, hist[:1], pos, 3, r), (x, hist.float(), pos, 3, r), (x, hist, pos, 9, r),
                     (x, hist, pos, -1, r), (x, hist, torch.zeros(2, dtype=torch.int32), 3, r), (x, hist, pos, 3, None),
                     (x, hist, pos, 3, lr), (x, hist, pos, 3, r, torch.zeros(2, V, dtype=torch.bfloat16))):
            with pytest.raises(ValueError):
                f(*args)
    assert ops.repeat_rules_supported(x, hist, pos, 3, r) is False                # CPU tensors: the torch path
    m = _tiny_model()
    for bad in (RepeatRules(99, 1.2), "rules", lr):
        with pytest.raises(ValueError):
            m.with_logit_rules(None, bad)
    mel, ids = torch.randn(2, 40, 10), torch.randint(0, 100, (2, 4))
    with pytest.raises(ValueError):                          # before any device work: a CPU encode would raise RuntimeError
        m._generate(mel, ids, 5, None, False, False, None, repeat_rules=RepeatRules(99, 1.2))


def _params(f):
    return {k: (v.default, v.kind) for k, v in inspect.signature(f).parameters.items() if k != "self"}


def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import WhisperMoP
    from mop_amd.nn.whisper_mop import RuledDecoding
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    sig = dict(logits=(e, P), hist=(e, P), pos=(e, P), t0=(e, P), rules=(e, P), out=(None, P))
    for fn in (ops.repeat_rules, ops.repeat_rules_torch, ops.repeat_rules_supported, ops.logit_rules, ops.logit_rules_torch,
               ops.logit_rules_supported):
        assert _params(fn) == sig, fn.__name__
    assert _params(ops.RepeatRules.__init__) == dict(vocab_size=(e, P), repetition_penalty=(1.0, P), no_repeat_ngram_size=(0, P),
                                                     exempt_tokens=((), P), exempt_from=(None, P), device=(None, P))
    assert _params(ops.RepeatRules.for_whisper) == dict(logit_rules=(e, P), repetition_penalty=(1.0, P),
                                                        no_repeat_ngram_size=(0, P), extra_exempt=((), P))
    assert _params(WhisperMoP.with_logit_rules) == dict(logit_rules=(e, P), repeat_rules=(None, P))
    assert _params(RuledDecoding.__init__) == dict(model=(e, P), logit_rules=(e, P), repeat_rules=(None, P))
    assert _params(WhisperMoP._transcribe)["repeat_rules"] == (None, K) and "repeat_rules" not in _params(RuledDecoding.transcribe)
    for fn in (WhisperMoP.generate, WhisperMoP.beam_search, WhisperMoP.sample, WhisperMoP.transcribe):
        assert "repeat_rules" not in _params(fn), fn.__name__                     # the public signatures stay


def test_support_query_and_bad_arguments_need_no_gpu():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    lib = _lib.lib()
    assert lib.mopk_version() == 118
    a = _lib.RepeatRulesArgs()
    a.R, a.V, a.dtype, a.T, a.T0, a.ngram, a.penalty, a.inv_penalty = 2, 100, _lib.MOPK_F32, 16, 3, 3, 1.25, 0.8
    a.logits_ld = a.out_ld = 100
    a.hist_ld = 16
    assert lib.mopk_repeat_rules_supported(C.byref(a)) == 1
    assert lib.mopk_repeat_rules(C.byref(a), None) != 0      # null pointers: refused before any launch
    for field, bad in (("V", 1), ("R", 0), ("dtype", 7), ("T0", 17), ("T0", -1), ("ngram", -1), ("penalty", 0.0), ("penalty", -1.0),
                       ("penalty", float("inf")), ("penalty", float("nan")), ("inv_penalty", 0.0), ("inv_penalty", float("nan")),
                       ("logits_ld", 99), ("out_ld", 99), ("hist_ld", 15), ("T", -1)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.mopk_repeat_rules_supported(C.byref(a)) == 0, (field, bad)
        assert lib.mopk_repeat_rules(C.byref(a), None) != 0, (field, bad)
        setattr(a, field, keep)
    a.T, a.hist_ld = 3 + 4096, 5000                          # the history that still fits in LDS ...
    assert lib.mopk_repeat_rules_supported(C.byref(a)) == 1
    a.T = 3 + 4097                                           # ... and the first that does not: the op takes the torch path
    assert lib.mopk_repeat_rules_supported(C.byref(a)) == 0
    a.T, a.ngram, a.penalty, a.inv_penalty = 16, 0, 1.0, 1.0  # neutral rules are a valid call
    assert lib.mopk_repeat_rules_supported(C.byref(a)) == 1


# ------------------------------------------------------------------ the decoders
def repeated_bigrams(tokens, exempt):
    """the bigrams (a, b), b not exempt, that one row's generated tokens hold more than once"""
    g = [int(t) for t in tokens]
    seen, twice = set(), set()
    for a, b in zip(g, g[1:]):
        if b in exempt:
            continue
        (twice if (a, b) in seen else seen).add((a, b))
    return twice


WHISPER_EXEMPT = {MODEL_RULES["eos_token_id"]} | set(range(MODEL_RULES["timestamp_begin"], 100))
N_NEW = 28


def decoder_inputs():
    torch.manual_seed(3)
    return torch.randn(3, 40, 10), torch.randint(0, 70, (3, 3))


def test_decoders_emit_no_repeated_bigram_with_torch_cores(torch_cores):     # noqa: F811
    from mop_amd import ops
    m = _peaked_tiny_model()
    mel, prompt = decoder_inputs()
    lr = ops.LogitRules(100, **MODEL_RULES)
    plain = m.with_logit_rules(lr).generate(mel, prompt, N_NEW)
    loops = [repeated_bigrams(row[3:], WHISPER_EXEMPT) for row in plain]
    print("repeated bigrams without repeat rules:", loops)
    assert all(loops)                                        # the test bites: every row of the un-ruled output repeats a bigram
    d = m.with_logit_rules(lr, ops.RepeatRules.for_whisper(lr, no_repeat_ngram_size=2))
    ops.LAST_PATH.pop("repeat_rules", None)
    out, steps = d.generate(mel, prompt, N_NEW, return_logits=True)
    assert ops.LAST_PATH["repeat_rules"] == 1
    assert torch.equal(steps.argmax(-1), out[:, 3:])         # the returned logits are those after both filters
    assert not torch.equal(out, plain)
    runs = {"generate": out[:, 3:], "generate-eos": d.generate(mel, prompt, N_NEW, eos_token_id=70)[:, 3:],
            "generate-stats": d.generate(mel, prompt, N_NEW, eos_token_id=70, return_stats=True)[0][:, 3:],
            "beam": d.beam_search(mel, prompt, N_NEW, 3, eos_token_id=70)[0][:, 3:],
            "beam-no-eos": d.beam_search(mel, prompt, N_NEW, 3)[0][:, 3:],
            "sample": d.sample(mel, prompt, N_NEW, temperature=0.9, top_k=30, num_samples=2, eos_token_id=70, seed=5)[0][:, :, 3:]}
    assert torch.equal(runs["generate-eos"], runs["generate-stats"])
    for name, toks in runs.items():
        for i, row in enumerate(toks.reshape(-1, N_NEW)):
            check_grammar(row.tolist(), MODEL_RULES, (name, i))
            assert not repeated_bigrams(row, WHISPER_EXEMPT), (name, i, row.tolist())
    ragged = d.generate(mel, [prompt[0], prompt[1, :2], prompt[2, :1]], N_NEW)
    for i, row in enumerate(ragged):
        check_grammar(row[3 - i:].tolist(), MODEL_RULES, ("ragged", i))
        assert not repeated_bigrams(row[3 - i:], WHISPER_EXEMPT), ("ragged", i)
    # without logit rules: the history is kept for the repeat rules alone
    bare = m.with_logit_rules(None, ops.RepeatRules(100, no_repeat_ngram_size=2)).generate(mel, prompt, N_NEW)
    assert all(repeated_bigrams(row[3:], set()) for row in m.generate(mel, prompt, N_NEW))
    assert not any(repeated_bigrams(row[3:], set()) for row in bare)


def test_a_penalty_changes_the_log_probabilities_it_should(torch_cores):     # noqa: F811
    """sample's sum_logprobs is the log-softmax of the row after BOTH filters, the repeat rules first"""
    from mop_amd import ops
    from test_whisper_rules_cpu import ref_rules
    m = _peaked_tiny_model()
    torch.manual_seed(4)
    mel, prompt = torch.randn(2, 40, 10), torch.randint(0, 70, (2, 3))
    lr = ops.LogitRules(100, **MODEL_RULES)
    rr = ops.RepeatRules.for_whisper(lr, 1.3, 3)
    tok, lp = m.with_logit_rules(lr, rr).sample(mel, prompt, 8, temperature=0.8, num_samples=2, seed=9)
    enc, _ = m.encode(mel)
    for b in range(2):
        for s in range(2):
            total = 0.0
            for t in range(8):
                ids = tok[b, s, :3 + t].unsqueeze(0)
                raw = m.decode(enc[b:b + 1], ids)[:, -1]
                row = ref_repeat(raw[0].tolist(), ids[0, 3:].tolist(), 100, rr.repetition_penalty, rr.inv_penalty, 3, WHISPER_EXEMPT)[0]
                row = torch.tensor([row], dtype=torch.float32)
                blocked, _ = ref_rules(row, ids.to(torch.int32), 3 + t, 3, 100, **MODEL_RULES)
                x = row.double().masked_fill(torch.from_numpy(blocked), NEG)
                total += float(torch.log_softmax(x, -1)[0, tok[b, s, 3 + t]])
            assert math.isfinite(total) and abs(total - float(lp[b, s])) <= 1e-3, (b, s, total, float(lp[b, s]))


def test_no_rules_and_neutral_rules_change_nothing(torch_cores):             # noqa: F811
    from mop_amd import ops
    m = _peaked_tiny_model()
    mel, prompt = decoder_inputs()
    lr = ops.LogitRules(100, **MODEL_RULES)
    for rules in (None, lr):
        today = m.with_logit_rules(rules)
        for rr in (None, ops.RepeatRules(100), ops.RepeatRules.for_whisper(lr)):
            ops.LAST_PATH.pop("repeat_rules", None)
            d = m.with_logit_rules(rules, rr)
            a, b = d.generate(mel, prompt, 10, return_logits=True), today.generate(mel, prompt, 10, return_logits=True)
            assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))
            a, b = d.beam_search(mel, prompt, 8, 3, eos_token_id=70), today.beam_search(mel, prompt, 8, 3, eos_token_id=70)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            a, b = d.sample(mel, prompt, 8, temperature=0.7, num_samples=2, seed=3), today.sample(mel, prompt, 8, temperature=0.7,
                                                                                                num_samples=2, seed=3)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert "repeat_rules" not in ops.LAST_PATH
    assert torch.equal(m.with_logit_rules(None, ops.RepeatRules(100)).generate(mel, prompt, 10), m.generate(mel, prompt, 10))


def test_transcribe_under_repeat_rules(torch_cores):                         # noqa: F811
    from mop_amd import ops
    from test_whisper_transcribe_cpu import CLIPS, RULES, V, check_transcript_shape, transcribe_model
    m = transcribe_model()
    torch.manual_seed(11)
    clips = [torch.randn(n, 10) for n in CLIPS]
    prompt = torch.tensor([7, 8, 9])
    lr = ops.LogitRules(V, **RULES)
    rr = ops.RepeatRules.for_whisper(lr, 1.2, 2)
    ex = set(rr.table("cpu").nonzero().flatten().tolist())
    ops.LAST_PATH.pop("repeat_rules", None)
    got = m.with_logit_rules(lr, rr).transcribe(clips, prompt, 12)
    assert ops.LAST_PATH["repeat_rules"] == 1
    plain = m.with_logit_rules(lr).transcribe(clips, prompt, 12)
    assert any(not torch.equal(a.tokens, b.tokens) for a, b in zip(got, plain))
    tb = RULES["timestamp_begin"]
    for g in got:
        check_transcript_shape(g, ordered=False)
        toks, off = g.tokens.tolist(), g.offsets.tolist()
        for i in range(len(off) - 1):                        # a segment: a timestamp, text, and a timestamp unless the window cut it
            seg = toks[off[i]:off[i + 1]]
            assert seg[0] >= tb and all(t < tb for t in seg[1:-1]) and RULES["eos_token_id"] not in seg, seg
            assert not repeated_bigrams(seg, ex), seg        # a segment lies inside one window's generated tokens
    with_fallback = m.with_logit_rules(lr, rr).transcribe(clips, prompt, 12, temperatures=(0.0, 0.6), logprob_threshold=-0.5,
                                                         num_samples=2, seed=1)
    for g in with_fallback:
        check_transcript_shape(g, ordered=False)
    via_kw = m._transcribe(clips, prompt, lr, 12, repeat_rules=rr)
    assert all(torch.equal(a.tokens, b.tokens) for a, b in zip(got, via_kw))
