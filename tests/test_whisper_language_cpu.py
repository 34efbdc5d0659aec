"""CPU checks of language detection (no GPU): ops.language_probs_torch against a float64 restatement written here (numpy: plain
rows, rows with -inf at some language entries, an exact tie between two language tokens listed in descending id order), the
signatures and exports, the library's support query and bad-argument returns (no launch), every
ValueError of LanguageTokens, the op, detect_language and transcribe's two keywords, and, with every core routed through its torch
composition, detect_language against decode() and transcribe(languages=...) against transcribe with the prompts filled by hand."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _params, _tiny_model
from test_whisper_fallback_cpu import LP_TOL
from test_whisper_transcribe_cpu import CLIPS, RULES, V, assert_transcripts_equal, transcribe_model

VS, RS, NS = (64, 131, 1027), (1, 3), (1, 2, 63, 64, 65, 99, 1024)
LANGS = tuple(range(20, 28))                   # the tiny model's language tokens: text ids that RULES leaves alone
SEED = 10                                      # transcribe_model(SEED) hears two languages in the three clips of language_setup, each
#                                                with a float64 top-2 margin above 0.3 (chosen on the CPU path; the tests assert both)
SOT, LANG_AT = 7, 1                            # the prompt is [SOT, a placeholder, 9]
PREV = 98                                      # the sot_prev token of the conditioned case (test_whisper_condition_cpu's)
MARGIN = 1e-3
WIDE_SEED, WIDE_CLIPS, WIDE_WINDOW = 6, (150, 64, 30), 64      # language_setup(wide=True), the GPU file's: the same two conditions hold


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ the float64 restatement
def ref_language_probs(x, ids):
    """x: (R, V) tensor, ids: the language tokens -> (probs (R, n) float64, tokens: R ints).  The softmax over the language
    entries alone (-inf entries add nothing and get 0) and, of the entries at the row's maximum, the smallest token id"""
    rows = x.detach().float().cpu().numpy().astype(np.float64)[:, list(ids)]
    m = rows.max(1, keepdims=True)
    e = np.exp(rows - m)
    tokens = [min(t for t, v in zip(ids, row) if v == row.max()) for row in rows]
    return e / e.sum(1, keepdims=True), tokens


def language_ids(V_, n, seed=0):
    """n distinct ids of [0, V_), V_ - 1 first and 0 second (a descending pair at columns 0 and 1), the rest shuffled"""
    perm = torch.randperm(V_, generator=torch.Generator().manual_seed(100 * V_ + n + seed)).tolist()
    return ([V_ - 1, 0] + [t for t in perm if t not in (0, V_ - 1)])[:n]


def language_cases(V_, R, dtype, n, device="cpu"):
    """-> (name, logits (R, V_), ids), built like stat_cases: plain rows; rows with -inf at every second language entry; an
    exact tie at the maximum between ids[0] = V_ - 1 and ids[1] = 0, so that a tie-break by column order picks the wrong one"""
    g = torch.Generator().manual_seed(1000 * V_ + 10 * R + n)
    base = (torch.randn(R, V_, generator=g) * 3).to(dtype)
    ids = language_ids(V_, n)
    yield "plain", base.clone().to(device), ids
    if n >= 2:
        f = base.clone()
        f[:, ids[1::2]] = float("-inf")
        yield "filtered", f.to(device), ids
        t = base.clone()
        top = (t[:, ids].float().max(1).values + 1).to(dtype)
        t[:, ids[0]] = top
        t[:, ids[1]] = top
        yield "tie", t.to(device), ids
        t = t.clone()                          # the tie below the maximum changes nothing
        t[:, ids[-1]] = (top.float() + 1).to(dtype)
        yield "tie below the maximum", t.to(device), ids


def check_language_probs(res, x, ids, what):
    """one result of an op against the restatement -> the float64 probabilities"""
    R, n = x.shape[0], len(ids)
    p64, tokens = ref_language_probs(x, ids)
    assert res.probs.dtype == torch.float32 and tuple(res.probs.shape) == (R, n), what
    assert res.tokens.dtype == torch.int32 and tuple(res.tokens.shape) == (R,), what
    assert res.tokens.tolist() == tokens, (what, res.tokens.tolist(), tokens)
    p = res.probs.detach().cpu().numpy().astype(np.float64)
    gone = np.isneginf(x.detach().float().cpu().numpy()[:, list(ids)])
    assert (p[gone] == 0).all() and (p64[gone] == 0).all(), what
    err = np.abs(p - p64) - (LP_TOL * p64 + 1e-30)
    assert (err <= 0).all(), (what, float(err.max()))
    return p64


@pytest.mark.parametrize("V_", VS)
@pytest.mark.parametrize("R", RS)
def test_torch_restatement_against_float64(V_, R):
    from mop_amd import ops
    seen = set()
    for n in NS:
        if n > V_:
            continue
        for dtype in (torch.float32, torch.bfloat16):
            for name, x, ids in language_cases(V_, R, dtype, n):
                what = (V_, R, n, dtype, name)
                L = ops.LanguageTokens(V_, ids)
                check_language_probs(ops.language_probs_torch(x, L), x, ids, what)
                got = ops.language_probs(x, L)                             # CPU tensors: the refused route
                check_language_probs(got, x, ids, what)
                bp, bt = torch.full((R, n + 3), -7.0)[:, :n], torch.empty(R, dtype=torch.int32)
                out = ops.language_probs_torch(x, L, bp, bt)
                assert out.probs is bp and out.tokens is bt and torch.equal(bp, got.probs) and torch.equal(bt, got.tokens), what
                if name == "tie":
                    assert got.tokens.tolist() == [0] * R, what            # ids[1], not the first column
                if name == "tie below the maximum":
                    assert got.tokens.tolist() == [ids[-1]] * R, what
                seen.add(name)
    assert seen == {"plain", "filtered", "tie", "tie below the maximum"}
    assert not ops.language_probs_supported(torch.randn(R, V_), ops.LanguageTokens(V_, [1, 0]))         # a CPU tensor


# ------------------------------------------------------------------ signatures, exports, the struct
def test_signatures_and_exports():
    from mop_amd import nn, ops
    from mop_amd.nn import LanguageDetection, LanguageTokens, WhisperMoP
    from mop_amd.nn.whisper_mop import RuledDecoding
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    sig = dict(logits=(e, P), languages=(e, P), out_probs=(None, P), out_tokens=(None, P))
    for fn in (ops.language_probs, ops.language_probs_torch, ops.language_probs_supported):
        assert _params(fn) == sig, fn.__name__
    assert LanguageTokens is ops.LanguageTokens and nn.LanguageDetection is LanguageDetection
    assert ops.LanguageProbs._fields == ("probs", "tokens") and LanguageDetection._fields == ("tokens", "probs")
    assert _params(ops.LanguageTokens.__init__) == dict(vocab_size=(e, P), token_ids=(e, P), device=(None, P))
    assert _params(ops.LanguageTokens.for_whisper) == dict(vocab_size=(e, P), sot_token_id=(e, P), n_languages=(e, P), device=(None, P))
    assert _params(WhisperMoP.detect_language) == dict(mel=(e, P), sot_ids=(e, P), languages=(e, P))
    last = [("condition_on_previous_text", (False, K)), ("initial_prompt", (None, K)), ("sot_prev_token_id", (None, K)),
            ("max_prompt_tokens", (None, K)), ("prompt_reset_temperature", (0.5, K))]
    for fn in (RuledDecoding.transcribe, WhisperMoP._transcribe):
        got = list(_params(fn).items())
        names = [k for k, _ in got]
        at = names.index("median_word_frames")
        assert got[at + 1:at + 3] == [("languages", (None, K)), ("language_index", (1, K))], fn.__name__
        assert at + 2 < names.index("condition_on_previous_text"), fn.__name__
        assert got[-5:] == last, fn.__name__
    assert _params(WhisperMoP.transcribe) == dict(
        mel=(e, P), prompt_ids=(e, P), logit_rules=(e, P), max_new_tokens=(e, P), window=(None, K), frames_per_timestamp=(1, K),
        num_beams=(1, K), length_penalty=(1.0, K), graph=(False, K))
    assert RuledDecoding.transcribe.__doc__ == WhisperMoP._transcribe.__doc__ and "language_index" in WhisperMoP._transcribe.__doc__


def test_language_tokens():
    from mop_amd import ops
    L = ops.LanguageTokens(V, [30, 5, 12])
    assert (L.vocab_size, L.token_ids, L.n) == (V, (30, 5, 12), 3)
    t = L.table("cpu")
    assert t.dtype == torch.int32 and t.tolist() == [30, 5, 12] and L.table("cpu") is t             # kept, in the given order
    assert ops.LanguageTokens(V, torch.tensor([4, 9])).token_ids == (4, 9) and ops.LanguageTokens(V, iter([3])).token_ids == (3,)
    W = ops.LanguageTokens.for_whisper(51865, 50258, 99)                   # Whisper's multilingual vocabulary
    assert W.n == 99 and W.token_ids[0] == 50259 and W.token_ids[-1] == 50357
    assert ops.LanguageTokens(1025, range(1024)).n == 1024
    for args in ((V, []), (V, range(1025)), (1, [0]), (V, [V]), (V, [-1]), (V, [3, 3]), (V, [1.5]), (V, [True]), (V, 3), (V, None),
                 (V, ["a"]), (2.5, [0]), (True, [0])):
        with pytest.raises(ValueError):
            ops.LanguageTokens(*args)
    for args in ((V, V - 3, 3), (V, -2, 2), (V, 5, 0), (V, 5.0, 2), (V, 5, True), (V, 0, 1025)):
        with pytest.raises(ValueError):
            ops.LanguageTokens.for_whisper(*args)
    assert ops.LanguageTokens.for_whisper(V, V - 4, 3).token_ids == (V - 3, V - 2, V - 1)


def test_op_value_errors():
    from mop_amd import ops
    L = ops.LanguageTokens(V, LANGS)
    x, n = torch.randn(3, V), len(LANGS)
    ops.language_probs(x, L, torch.empty(3, n), torch.empty(3, dtype=torch.int32))
    for fn in (ops.language_probs, ops.language_probs_torch, ops.language_probs_supported):
        for args in ((x, list(LANGS)), (x, None), (x, ops.LanguageTokens(V + 1, LANGS)), (x[0], L), (x.view(1, 3, V), L), (x.long(), L),
                     (x[:0], L), (None, L), (x, L, torch.empty(3, n + 1)), (x, L, torch.empty(2, n)), (x, L, torch.empty(3, n).double()),
                     (x, L, torch.empty(3, n, device="meta")), (x, L, [0.0]), (x, L, None, torch.empty(3, dtype=torch.int64)),
                     (x, L, None, torch.empty(4, dtype=torch.int32)), (x, L, None, torch.empty(3, 1, dtype=torch.int32)),
                     (x, L, None, torch.empty(3, dtype=torch.int32, device="meta"))):
            with pytest.raises(ValueError):
                fn(*args)


def test_support_query_and_bad_arguments_need_no_gpu(lib):
    from mop_amd import _lib
    assert lib.mopk_version() == 118
    a = _lib.LanguageProbsArgs()
    a.R, a.V, a.dtype, a.n, a.logits_ld, a.probs_ld = 3, 131, _lib.MOPK_BF16, 99, 131, 99
    assert lib.mopk_language_probs_supported(C.byref(a)) == 1
    assert lib.mopk_language_probs(C.byref(a), None) == -2                 # null pointers: MOPK_ERR_BAD_ARG in the launcher, not the query
    for field, bad in (("R", 0), ("V", 1), ("dtype", 7), ("n", 0), ("n", 1025), ("n", -1), ("logits_ld", 130), ("probs_ld", 98),
                       ("logits", 1), ("ids", 2), ("probs", 6), ("tokens", 1)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.mopk_language_probs_supported(C.byref(a)) == 0, (field, bad)
        assert lib.mopk_language_probs(C.byref(a), None) < 0, (field, bad)
        setattr(a, field, keep if keep is not None else 0)
    a.logits = 2                                                           # bf16 rows are element-aligned only ...
    a.dtype = _lib.MOPK_BF16
    assert lib.mopk_language_probs_supported(C.byref(a)) == 1
    a.dtype = _lib.MOPK_F32                                                # ... and so are fp32 rows: 4 bytes
    assert lib.mopk_language_probs_supported(C.byref(a)) == 0
    a.logits = 4
    assert lib.mopk_language_probs_supported(C.byref(a)) == 1
    a.n, a.probs_ld, a.V, a.logits_ld = 1024, 1024, 51865, 51866
    assert lib.mopk_language_probs_supported(C.byref(a)) == 1
    assert lib.mopk_language_probs_supported(None) == 0 and lib.mopk_language_probs(None, None) < 0


# ------------------------------------------------------------------ the model
def wide_model(seed):
    """transcribe_model at the width of the GPU files' models (heads of 64, 12 mel bins, windows of 64 frames)"""
    m = _tiny_model(vocab_size=V, n_mels=12, n_audio_ctx=WIDE_WINDOW, n_embd=128)
    torch.manual_seed(seed)
    with torch.no_grad():
        m.dec_ln_f.weight.mul_(20.0)
        for p in m.decoder.parameters():
            if p.dim() == 2:
                p.add_(torch.randn_like(p) * 0.05)
    return m


def language_setup(device="cpu", wide=False):
    """-> (model, three clips: several windows, exactly one, shorter than one, the prompt with its placeholder, logit rules,
    language tokens, the window).  wide: the model and clips of the GPU file (the same weights and inputs on either device)"""
    from mop_amd import ops
    m = (wide_model(WIDE_SEED) if wide else transcribe_model(SEED)).to(device)
    torch.manual_seed(11)
    clips = [torch.randn(n, 12 if wide else 10).to(device) for n in (WIDE_CLIPS if wide else CLIPS)]
    prompt = torch.tensor([SOT, 0, 9], device=device)
    return (m, clips, prompt, ops.LogitRules(V, **RULES, device=device), ops.LanguageTokens(V, LANGS, device=device),
            WIDE_WINDOW if wide else 40)


def language_margins(logits, ids=LANGS):
    """the float64 top-2 probability margin of each row of last-position logits over the language tokens"""
    p64, _ = ref_language_probs(logits, ids)
    top = np.sort(p64, 1)
    return (top[:, -1] - top[:, -2]).tolist()


def test_detect_language_equals_the_op_on_decode(torch_cores):             # noqa: F811
    from mop_amd import ops
    from mop_amd.nn import LanguageDetection
    m, clips, prompt, _, L, _ = language_setup()
    first = [c[:40] for c in clips]
    for mel, B in ((first, 3), (torch.stack([c[:17] for c in clips]), 3), (first[2:], 1)):
        for sot, ids in ((SOT, torch.full((B, 1), SOT)), (prompt[:1], prompt[:1].expand(B, 1)),
                         (torch.tensor([[SOT, 3]] * B, dtype=torch.int32), torch.tensor([[SOT, 3]] * B))):
            got = m.detect_language(mel, sot, L)
            logits = m.decode(m.encode(mel)[0], ids)[:, -1]
            want = ops.language_probs_torch(logits, L)
            assert isinstance(got, LanguageDetection) and got.tokens.dtype == torch.int32 and got.probs.dtype == torch.float32
            assert torch.equal(got.tokens, want.tokens) and torch.equal(got.probs, want.probs), (B, sot)
            assert got.probs.shape == (B, len(LANGS)) and not got.probs.requires_grad
            check_language_probs(ops.LanguageProbs(got.probs, got.tokens), logits, LANGS, (B, sot))
    got = m.detect_language(first, SOT, L)
    assert len(set(got.tokens.tolist())) >= 2, got.tokens.tolist()         # the seed's condition: a row mix-up cannot pass
    margins = language_margins(m.decode(m.encode(first)[0], torch.full((3, 1), SOT))[:, -1])
    assert min(margins) > MARGIN, margins                                  # ... and the GPU file's: no row is a near tie
    alone = [m.detect_language([c], SOT, L) for c in first]               # a clip in a ragged batch is the clip alone
    assert [int(a.tokens) for a in alone] == got.tokens.tolist()
    assert torch.allclose(torch.cat([a.probs for a in alone]), got.probs, rtol=1e-4, atol=1e-7)


def test_detect_language_value_errors(torch_cores):                        # noqa: F811
    from mop_amd import ops
    m, clips, prompt, _, L, _ = language_setup()
    first = [c[:40] for c in clips]
    mel = torch.stack([c[:17] for c in clips])
    for args in ((first, SOT, list(LANGS)), (first, SOT, None), (first, SOT, ops.LanguageTokens(V + 1, LANGS)),
                 (first, V, L), (first, -1, L), (first, True, L), (first, 7.0, L), (first, None, L), (first, [SOT], L),
                 (first, torch.tensor([V]), L), (first, torch.tensor([-1]), L), (first, torch.tensor([7.0]), L),
                 (first, torch.tensor([], dtype=torch.long), L), (first, torch.tensor(7), L), (first, torch.zeros(2, 1, dtype=torch.long), L),
                 (first, torch.zeros(3, 1, 1, dtype=torch.long), L), (first, torch.zeros(65, dtype=torch.long), L),
                 (first, torch.tensor([SOT], device="meta"), L), (mel, torch.zeros(4, 1, dtype=torch.long), L),
                 ([], SOT, L), (clips, SOT, L), (mel[0], SOT, L), (torch.randn(2, 17, 11), SOT, L), (torch.randn(2, 41, 10), SOT, L),
                 (None, SOT, L)):
        with pytest.raises(ValueError):
            m.detect_language(*args)
    m.detect_language(first, torch.zeros(64, dtype=torch.long), L)        # T_s = n_text_ctx still fits


def as_lists(transcripts):
    return [tuple(x.tolist() for x in t) for t in transcripts]


def check_transcribe_languages(m, clips, prompt, rules, L, window=40, n_new=12, at=LANG_AT, **kw):
    """transcribe(languages=L, language_index=at, **kw) against transcribe given the (B, T_p) prompts filled by hand from
    detect_language of the first windows: everything returned equal bit for bit, the detection that call's -> (what came back,
    the detection)"""
    B = len(clips)
    d = m.with_logit_rules(rules)
    det = m.detect_language([c[:window] for c in clips], prompt[..., :at], L)
    filled = (prompt if prompt.dim() == 2 else prompt.unsqueeze(0).expand(B, -1)).clone()
    filled[:, at] = det.tokens.to(filled.dtype)
    want = d.transcribe(clips, filled, n_new, window=window, **kw)
    got = d.transcribe(clips, prompt, n_new, window=window, languages=L, language_index=at, **kw)
    want = want if isinstance(want, tuple) else (want,)
    assert isinstance(got, tuple) and len(got) == len(want) + 1, kw
    gd = got[-1]
    assert type(gd).__name__ == "LanguageDetection" and torch.equal(gd.tokens, det.tokens) and torch.equal(gd.probs, det.probs), kw
    assert gd.tokens.dtype == torch.int32 and gd.tokens.device == clips[0].device
    assert_transcripts_equal(got[0], as_lists(want[0]), prompt.dtype, kw)
    assert sum(t.tokens.numel() for t in got[0]) > 0
    for g, w in zip(got[1:-1], want[1:]):                                  # the logs (host lists, NaN where unset), the words
        assert len(g) == len(w) == B
        for x, y in zip(g, w):
            assert type(x) is type(y)
            for p, q in zip(x, y):
                assert torch.equal(p, q) if isinstance(p, torch.Tensor) else repr(p) == repr(q), kw
    return got, det


COND = dict(condition_on_previous_text=True, sot_prev_token_id=PREV, max_prompt_tokens=6)
TRANSCRIBE_CASES = ("greedy", "beams", "fallback with the log", "conditioned", "words", "log, words and conditioning", "per-clip prompts")


def check_transcribe_language_case(case, m, clips, prompt, rules, L, wrules, window=40):
    """one case of transcribe with `languages` (the issue's, in its order: plain with 1 and 3 beams, a fallback policy with the
    log, conditioning, word timestamps; then all of it at once and per-clip prompts): the four return shapes on the way"""
    args = (m, clips, prompt, rules, L, window)
    words = dict(word_timestamps=True, word_rules=wrules, median_word_frames=2)
    if case in ("greedy", "beams"):
        got, det = check_transcribe_languages(*args, num_beams=1 if case == "greedy" else 3)
        assert len(got) == 2 and len(set(det.tokens.tolist())) >= 2, det.tokens.tolist()      # a row mix-up cannot pass
    elif case == "fallback with the log":
        _, base = m.with_logit_rules(rules).transcribe(clips, prompt, 12, window=window, return_log=True, languages=L)[:2]
        avgs = sorted(a for g in base for a in g.avg_logprob)
        got, _ = check_transcribe_languages(*args, temperatures=(0.0, 0.5), logprob_threshold=avgs[len(avgs) // 2], seed=3,
                                            return_log=True)
        temps = [t for g in got[1] for t in g.temperature]
        assert len(got) == 3 and any(t > 0 for t in temps) and any(t == 0 for t in temps), temps
    elif case == "conditioned":
        assert len(check_transcribe_languages(*args, **COND)[0]) == 2
    elif case == "words":
        got, _ = check_transcribe_languages(*args, **words)
        assert len(got) == 3 and type(got[1][0]).__name__ == "TranscriptWords" and sum(len(w.starts) for w in got[1]) >= 3
    elif case == "log, words and conditioning":
        got, _ = check_transcribe_languages(*args, return_log=True, **words, **COND)
        assert len(got) == 4 and type(got[1][0]).__name__ == "TranscribeLog" and type(got[2][0]).__name__ == "TranscriptWords"
    else:                                                                  # int32, the language token second to last
        prompts = torch.tensor([[SOT, 8, 0, 9], [SOT, 9, 0, 8], [SOT, 8, 0, 7]], dtype=torch.int32, device=prompt.device)
        assert case == "per-clip prompts" and len(check_transcribe_languages(m, clips, prompts, rules, L, window, at=2)[0]) == 2


@pytest.mark.parametrize("case", TRANSCRIBE_CASES)
def test_transcribe_with_languages_equals_the_filled_prompts(torch_cores, case):  # noqa: F811
    from test_whisper_words_cpu import word_rules_by_residue
    m, clips, prompt, rules, L, window = language_setup()
    check_transcribe_language_case(case, m, clips, prompt, rules, L, word_rules_by_residue(V), window)
    if case == "greedy":                                                   # the placeholder was replaced: the language is heard
        d = m.with_logit_rules(rules)
        assert as_lists(d.transcribe(clips, prompt, 12)) != as_lists(d.transcribe(clips, prompt, 12, languages=L)[0])


def test_transcribe_audio_passes_the_keywords_on(torch_cores, monkeypatch):  # noqa: F811
    from mop_amd import ops
    from mop_amd.nn import LogMelFrontend
    from test_whisper_frontend_cpu import SR, noise
    monkeypatch.setattr(ops, "log_mel", ops.log_mel_torch)
    m, _, prompt, rules, L, _ = language_setup()
    fe = LogMelFrontend(10, SR, 64, 16)
    audio = [torch.from_numpy(noise(16 * T + 5, seed=T)).float() for T in (100, 40, 17)]
    want, wd = m.with_logit_rules(rules).transcribe(fe(audio), prompt, 12, languages=L)
    got, gd = m.transcribe_audio(audio, fe, prompt, rules, 12, languages=L, language_index=1)
    assert_transcripts_equal(got, as_lists(want), torch.int64, "audio")
    assert torch.equal(gd.tokens, wd.tokens) and torch.equal(gd.probs, wd.probs)


def test_defaults_run_todays_path(torch_cores, monkeypatch):               # noqa: F811
    from mop_amd import ops
    m, clips, prompt, rules, L, _ = language_setup()

    def refuse(*a, **k):
        raise AssertionError("ops.language_probs ran without languages")
    monkeypatch.setattr(ops, "language_probs", refuse)
    monkeypatch.setattr(type(m), "detect_language", refuse)
    ops.LAST_PATH.pop("language_probs", None)
    d = m.with_logit_rules(rules)
    plain = m.transcribe(clips, prompt, rules, 12)
    omitted = d.transcribe(clips, prompt, 12)
    spelled = d.transcribe(clips, prompt, 12, languages=None, language_index=-5)       # not looked at without languages
    assert isinstance(omitted, list) and isinstance(spelled, list) and "language_probs" not in ops.LAST_PATH
    assert_transcripts_equal(omitted, as_lists(plain), torch.int64, "omitted")
    assert_transcripts_equal(spelled, as_lists(plain), torch.int64, "None")
    out, log = d.transcribe(clips, prompt, 12, return_log=True, languages=None)
    assert_transcripts_equal(out, as_lists(plain), torch.int64, "log")
    assert len(log) == 3


def test_transcribe_language_value_errors(torch_cores):                    # noqa: F811
    from mop_amd import ops
    m, clips, prompt, rules, L, _ = language_setup()
    d = m.with_logit_rules(rules)
    d.transcribe([clips[2]], prompt, 2, languages=L, language_index=2)     # the last column is still one
    for kw in (dict(languages=list(LANGS)), dict(languages=ops.LanguageTokens(V + 1, LANGS)), dict(languages=rules),
               dict(languages=L, language_index=0), dict(languages=L, language_index=3), dict(languages=L, language_index=-1),
               dict(languages=L, language_index=1.0), dict(languages=L, language_index=True), dict(languages=L, language_index=None)):
        with pytest.raises(ValueError):
            d.transcribe(clips, prompt, 4, **kw)
    with pytest.raises(ValueError):                                        # a prompt of one token has no column for the language
        d.transcribe(clips, prompt[:1], 4, languages=L)
    with pytest.raises(ValueError):                                        # a host prompt whose sot part leaves the vocabulary
        d.transcribe(clips, torch.tensor([V, 0, 9]), 4, languages=L)
