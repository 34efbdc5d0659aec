"""CPU checks of the decoding statistics and of transcribe's temperature fallback and no-speech skip (no GPU):
ops.token_logprob_torch and ops.greedy_pick_torch against a float64 restatement written here (numpy log-softmax, a Python loop over
the rows: filtered rows, the picked entry being eos, rows already done, an exact tie at the maximum), the
library's support queries (no launch), generate / beam_search / sample with return_stats against recomputations from
the step logits and from a teacher-forced pass, no_speech_prob against decode(), and with_logit_rules(rules).transcribe under the
policy against a naive loop over the same public decoders, with every core routed through its torch composition."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition)
from test_whisper_transcribe_cpu import EOS, RULES, TB, V, assert_transcripts_equal, transcribe_model

LP_TOL = 1e-5                                  # the `lp` tolerance of tests/test_gpu_whisper_sample.py: the same quantity, the same steps
VS, RS = (64, 131, 1027), (1, 3, 16)
NO_SPEECH = 96                                 # a text token the rules never block outright


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------ the float64 restatement
def ref_log_softmax(row):
    """float64 log-softmax of one row (a numpy vector; -inf entries add nothing)"""
    x = np.asarray(row, dtype=np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def ref_token_logprob(x, tokens):
    """x: (R, V) tensor; tokens: R ints -> list of R float64 log-probabilities"""
    rows = x.detach().float().cpu().numpy()
    return [float(ref_log_softmax(rows[r])[int(t)]) for r, t in enumerate(tokens)]


def ref_greedy_pick(x, done, sums, counts, eos):
    """one step, row by row -> (tokens, done, sums (float64), counts) as lists; eos None: no eos"""
    rows = x.detach().float().cpu().numpy()
    toks, done, sums, counts = [], list(done), list(sums), list(counts)
    for r in range(rows.shape[0]):
        if eos is not None and done[r]:
            toks.append(eos)
            continue
        best = int(np.argmax(rows[r]))                                     # numpy documents the first maximal index too
        toks.append(best)
        sums[r] += float(ref_log_softmax(rows[r])[best])
        counts[r] += 1
        if eos is not None and best == eos:
            done[r] = 1
    return toks, done, sums, counts


def stat_cases(V_, R, dtype, device="cpu"):
    """-> (name, logits (R, V), eos, done list): plain rows; rows filtered to -inf except a few entries; the picked entry is eos;
    rows already done; an exact tie at the maximum, built by copying the maximum to a later index"""
    g = torch.Generator().manual_seed(1000 * V_ + R)
    base = (torch.randn(R, V_, generator=g) * 3).to(dtype)
    eos = V_ // 3
    yield "plain", base.clone().to(device), eos, [0] * R
    f = torch.full_like(base, float("-inf"))
    keep = torch.randint(0, V_, (R, 4), generator=g)
    f.scatter_(1, keep, base.gather(1, keep))
    yield "filtered", f.to(device), eos, [0] * R
    e = base.clone()
    e[:, eos] = e.float().max(1).values.to(dtype) + 1
    yield "picks eos", e.to(device), eos, [0] * R
    yield "done rows", base.clone().to(device), eos, [(r + 1) % 2 for r in range(R)]
    t = base.clone()
    first = t.float().argmax(1)
    later = (first + 1 + torch.randint(0, V_ - 1, (R,), generator=g) % (V_ - 1 - first).clamp_min(1)).clamp_max(V_ - 1)
    t.scatter_(1, later.unsqueeze(1), t.gather(1, first.unsqueeze(1)))
    yield "tie", t.to(device), eos, [0] * R
    yield "no eos", base.clone().to(device), None, [0] * R


def fresh_state(ops, R, cap, eos, done, device="cpu"):
    st = ops.GreedyState(R, cap, eos, with_hist=True, device=device)
    st.done.copy_(torch.tensor(done, dtype=torch.int32))
    st.sum_logprobs.copy_(torch.linspace(-3.0, -1.0, R))
    st.n_tokens.copy_(torch.arange(R, dtype=torch.int32) + 2)
    st.hist.fill_(-7)
    return st


def check_pick(ops, pick, x, eos, done, what, device="cpu"):
    """run `pick` on a fresh state and compare it with the restatement -> the state"""
    R, cap, p = x.shape[0], 9, 5
    st = fresh_state(ops, R, cap, eos, done, device)
    sums0, counts0 = st.sum_logprobs.tolist(), st.n_tokens.tolist()
    pick(x, st, torch.tensor([p], dtype=torch.int32, device=device))
    toks, done1, sums, counts = ref_greedy_pick(x, done, sums0, counts0, eos)
    assert st.next_ids.dtype == torch.int32 and st.next_ids.shape == (R, 1), what
    assert st.next_ids.view(-1).tolist() == toks, what
    assert st.done.tolist() == done1 and st.n_tokens.tolist() == counts, what
    err = max(abs(a - b) for a, b in zip(st.sum_logprobs.tolist(), sums))
    assert err <= LP_TOL, (what, err)
    assert st.hist[:, p].tolist() == toks, what
    rest = torch.cat([st.hist[:, :p], st.hist[:, p + 1:]], 1)
    assert bool((rest == -7).all()), what                                  # only column pos is written
    return st


@pytest.mark.parametrize("V_", VS)
@pytest.mark.parametrize("R", RS)
def test_torch_restatements_against_float64(V_, R):
    from mop_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        for name, x, eos, done in stat_cases(V_, R, dtype):
            what = (V_, R, dtype, name)
            check_pick(ops, ops.greedy_pick_torch, x, eos, done, what)
            check_pick(ops, ops.greedy_pick, x, eos, done, what)           # CPU tensors: the refused route
            g = torch.Generator().manual_seed(7)
            finite = torch.where(torch.isfinite(x.float()), 0.0, -1e30) + torch.rand(x.shape, generator=g)
            toks = finite.argmax(1).to(torch.int32)                        # a random finite entry per row ...
            if name == "filtered":
                toks[0] = int((~torch.isfinite(x[0].float())).nonzero()[0])            # ... and one whose own entry is -inf
            want = ref_token_logprob(x, toks.tolist())
            for got in (ops.token_logprob_torch(x, toks), ops.token_logprob(x, toks),
                        ops.token_logprob_torch(x, toks, out=torch.empty(R))):
                assert got.dtype == torch.float32 and got.shape == (R,), what
                for a, b in zip(got.tolist(), want):
                    assert (a == b) if math.isinf(b) else abs(a - b) <= LP_TOL, (what, a, b)
            if name == "filtered":
                assert ops.token_logprob_torch(x, toks)[0] == float("-inf")
            one = int(toks[-1])
            assert torch.equal(ops.token_logprob_torch(x, one), ops.token_logprob_torch(x, torch.full((R,), one)))


def test_op_value_errors():
    from mop_amd import ops
    x, pos = torch.randn(3, 64), torch.tensor([2], dtype=torch.int32)
    st = ops.GreedyState(3, 4, 5, with_hist=True)
    ops.greedy_pick_torch(x, st, pos)
    bad_hist = ops.GreedyState(3, 4, 5, with_hist=True)
    bad_hist.hist = bad_hist.hist.long()
    for bad in (lambda: ops.token_logprob_torch(x, 64), lambda: ops.token_logprob_torch(x, -1), lambda: ops.token_logprob_torch(x, 1.0),
                lambda: ops.token_logprob_torch(x, True), lambda: ops.token_logprob_torch(x, torch.tensor([1, 2])),
                lambda: ops.token_logprob_torch(x, torch.tensor([1, 2, 64])), lambda: ops.token_logprob_torch(x, torch.tensor([1., 2., 3.])),
                lambda: ops.token_logprob_torch(x[0], 1), lambda: ops.token_logprob_torch(x[:, :1], 0),
                lambda: ops.token_logprob_torch(x.long(), 1), lambda: ops.token_logprob_torch(x, 1, out=torch.empty(2)),
                lambda: ops.token_logprob_torch(x, 1, out=torch.empty(3, dtype=torch.float64)),
                lambda: ops.token_logprob(x, 64), lambda: ops.token_logprob_supported(x, 64),
                lambda: ops.GreedyState(0, 4), lambda: ops.GreedyState(3, 0), lambda: ops.GreedyState(3, 4, -1),
                lambda: ops.GreedyState(3, 4, 1.0), lambda: ops.greedy_pick_torch(x, None, pos),
                lambda: ops.greedy_pick_torch(x[:2], st, pos), lambda: ops.greedy_pick_torch(x, st, torch.tensor([1, 2])),
                lambda: ops.greedy_pick_torch(x, st, torch.tensor([1.0])), lambda: ops.greedy_pick_torch(x, st, torch.tensor([4])),
                lambda: ops.greedy_pick_torch(x, st, torch.tensor([-1])), lambda: ops.greedy_pick_torch(x, ops.GreedyState(3, 4, 64), pos),
                lambda: ops.greedy_pick_torch(x, bad_hist, pos), lambda: ops.greedy_pick(x, st, torch.tensor([4])),
                lambda: ops.greedy_pick_supported(x[:2], st, pos)):
        with pytest.raises(ValueError):
            bad()
    assert not ops.token_logprob_supported(x, 1) and not ops.greedy_pick_supported(x, st, pos)      # CPU tensors


# ------------------------------------------------------------------ ABI
def test_support_queries_and_bad_arguments_need_no_gpu(lib):
    from mop_amd import _lib
    t = _lib.TokenLogprobArgs()
    t.R, t.V, t.dtype, t.token, t.logits, t.logits_ld, t.out = 3, 131, _lib.MOPK_BF16, 5, 4098, 134, 4096
    assert lib.mopk_token_logprob_supported(C.byref(t)) == 1               # a row stride >= V at any element alignment
    for field, v in (("R", 0), ("V", 1), ("dtype", 7), ("logits_ld", 130), ("token", 131), ("token", -1), ("logits", 4097),
                     ("out", 4098), ("tokens", 4098)):
        old = getattr(t, field)
        setattr(t, field, v)
        assert lib.mopk_token_logprob_supported(C.byref(t)) == 0, field
        assert lib.mopk_token_logprob(C.byref(t), None) < 0, field
        setattr(t, field, old)
    t.tokens, t.token = 4096, -1                                           # with tokens the scalar is not looked at
    assert lib.mopk_token_logprob_supported(C.byref(t)) == 1
    t.logits = None
    assert lib.mopk_token_logprob(C.byref(t), None) < 0                    # null pointers: refused before any launch
    assert lib.mopk_token_logprob_supported(None) == 0 and lib.mopk_token_logprob(None, None) < 0
    g = _lib.GreedyPickArgs()
    g.R, g.V, g.dtype, g.eos, g.logits, g.logits_ld = 3, 131, _lib.MOPK_F32, -1, 4100, 131
    g.pos, g.next_ids, g.done, g.sum_logprobs, g.n_tokens = 4096, 4096, 4096, 4096, 4096
    assert lib.mopk_greedy_pick_supported(C.byref(g)) == 1
    g.hist, g.hist_cap, g.hist_ld = 4096, 9, 27
    assert lib.mopk_greedy_pick_supported(C.byref(g)) == 1
    for field, v in (("R", 0), ("V", 1), ("dtype", 7), ("logits_ld", 130), ("eos", 131), ("eos", -2), ("reserved", 1),
                     ("logits", 4098), ("hist_ld", 8), ("hist_cap", -1), ("pos", 4098), ("done", 4097), ("hist", 4098)):
        old = getattr(g, field)
        setattr(g, field, v)
        assert lib.mopk_greedy_pick_supported(C.byref(g)) == 0, field
        assert lib.mopk_greedy_pick(C.byref(g), None) < 0, field
        setattr(g, field, old)
    g.done = None
    assert lib.mopk_greedy_pick(C.byref(g), None) < 0
    assert lib.mopk_greedy_pick_supported(None) == 0 and lib.mopk_greedy_pick(None, None) < 0


# ------------------------------------------------------------------ the decoders
def recompute_stats(tokens, logits, T_p, eos):
    """tokens: (B, T_p + n) list; logits (B, n, V): the rows that chose them -> (sums float64, counts): the log-softmax of each
    step's row at the chosen token, stopping after the first eos"""
    sums, counts = [], []
    for b, row in enumerate(tokens):
        s, n = 0.0, 0
        for t, tok in enumerate(row[T_p:]):
            s += float(ref_log_softmax(logits[b, t].float().numpy())[tok])
            n += 1
            if eos is not None and tok == eos:
                break
        sums.append(s)
        counts.append(n)
    return sums, counts


def assert_sums_close(got, want, what):
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (what, a, b)        # the bound of the sampling tests' sum_logprobs


def gen_inputs(kind):
    torch.manual_seed(5)
    if kind == "uniform":
        return torch.randn(3, 40, 10), torch.tensor([[7, 8, 9]] * 3), None
    if kind == "ragged":
        return torch.randn(3, 40, 10), [torch.tensor([7, 8, 9]), torch.tensor([9]), torch.tensor([8, 7])], [3, 1, 2]
    return [torch.randn(n, 10) for n in (40, 23, 9)], torch.tensor([[7, 8, 9]] * 3, dtype=torch.int32), None     # "clips"


@pytest.mark.parametrize("ruled", [False, True], ids=["plain", "rules"])
@pytest.mark.parametrize("kind", ["uniform", "ragged", "clips"])
def test_generate_statistics(torch_cores, kind, ruled):                   # noqa: F811
    from mop_amd import ops
    from mop_amd.nn import DecodeStats
    m = transcribe_model()
    mel, prompt, lens = gen_inputs(kind)
    rules = ops.LogitRules(V, **RULES) if ruled else None
    d = m.with_logit_rules(rules)
    n_new, T_p = 12, 3
    eos = EOS
    if not ruled:                                                          # an eos that the run meets in mid-row
        first = d.generate(mel, prompt, n_new)
        eos = int(first[0][-6])
    plain = d.generate(mel, prompt, n_new, eos)
    plain_l, logits = d.generate(mel, prompt, n_new, eos, return_logits=True)
    got, got_logits, st = d.generate(mel, prompt, n_new, eos, return_logits=True, return_stats=True)
    only, st2 = d.generate(mel, prompt, n_new, eos, return_stats=True)
    assert isinstance(st, DecodeStats) and st.no_speech_prob is None
    rows = lambda t: [r.tolist() for r in t]                               # noqa: E731
    assert rows(got) == rows(plain) == rows(only) == rows(plain_l), (kind, ruled)
    for a, b in zip(got, plain):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(got_logits, logits)
    assert torch.equal(st.sum_logprobs, st2.sum_logprobs) and torch.equal(st.n_tokens, st2.n_tokens)
    assert st.sum_logprobs.dtype == torch.float32 and st.n_tokens.dtype == torch.int32 and st.n_tokens.shape == (3,)
    full = [([0] * (T_p - len(r) + n_new) + r) for r in rows(got)]        # left-pad a ragged row back to T_p columns
    sums, counts = recompute_stats(full, logits, T_p, eos)
    assert st.n_tokens.tolist() == counts, (kind, ruled)
    assert_sums_close(st.sum_logprobs.tolist(), sums, (kind, ruled))
    assert min(counts) < n_new or ruled, counts                            # the plain run's eos really cut a row short


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("sot", [0, 1])
def test_no_speech_prob(torch_cores, kind, sot):                          # noqa: F811
    from mop_amd import ops
    m = transcribe_model()
    mel, prompt, lens = gen_inputs(kind)
    if kind == "ragged":
        prompt[1] = torch.tensor([9, 7])                                   # sot_index 1 lies inside the shortest prompt
    enc = m.encode(mel)[0]
    want = []
    for b in range(3):
        p = prompt[b].unsqueeze(0)
        want.append(float(torch.softmax(m.decode(enc[b:b + 1], p)[0, sot].detach().double(), -1)[NO_SPEECH]))
    for d in (m.with_logit_rules(None), m.with_logit_rules(ops.LogitRules(V, **RULES))):            # read before the rules
        outs = (d.generate(mel, prompt, 4, EOS, return_stats=True, no_speech_token_id=NO_SPEECH, sot_index=sot)[-1],
                d.beam_search(mel, prompt, 4, 2, EOS, return_stats=True, no_speech_token_id=NO_SPEECH, sot_index=sot)[-1],
                d.sample(mel, prompt, 4, num_samples=2, eos_token_id=EOS, return_stats=True, no_speech_token_id=NO_SPEECH,
                         sot_index=sot)[-1])
        for st in outs:
            assert st.no_speech_prob.shape == (3,) and st.no_speech_prob.dtype == torch.float32
            for a, b in zip(st.no_speech_prob.tolist(), want):
                assert abs(a - b) <= 1e-4 * b, (kind, sot, a, b)
    d = m.with_logit_rules(None)
    short = 3 if kind == "uniform" else 2
    for bad in (dict(sot_index=short), dict(sot_index=-1), dict(sot_index=1.0), dict(no_speech_token_id=V),
                dict(no_speech_token_id=-1), dict(no_speech_token_id=2.0), dict(eos_token_id=V), dict(eos_token_id=-1)):
        for call in (lambda kw: d.generate(mel, prompt, 4, return_stats=True, **kw),
                     lambda kw: d.beam_search(mel, prompt, 4, 2, return_stats=True, **kw),
                     lambda kw: d.sample(mel, prompt, 4, return_stats=True, **kw)):
            with pytest.raises(ValueError):
                call(bad)


def teacher_forced_sums(m, mel, tokens, T_p, counts):
    """the sum of log_softmax(decode(...))[token] over each row's first counts[b] generated tokens, in float64"""
    enc = m.encode(mel)[0]
    sums = []
    for b, row in enumerate(tokens):
        seq = torch.tensor(row)
        lg = m.decode(enc[b:b + 1], seq[:-1].unsqueeze(0))[0].detach()
        sums.append(sum(float(ref_log_softmax(lg[T_p - 1 + t].numpy())[row[T_p + t]]) for t in range(counts[b])))
    return sums


def lengths(rows, T_p, eos):
    return [(r[T_p:].index(eos) + 1) if eos in r[T_p:] else len(r) - T_p for r in rows]


@pytest.mark.parametrize("length_penalty", [1.0, 0.6])
def test_beam_search_statistics(torch_cores, length_penalty):             # noqa: F811
    m = transcribe_model()
    mel, prompt, _ = gen_inputs("uniform")
    d = m.with_logit_rules(None)
    eos = int(d.beam_search(mel, prompt, 10, 3)[0][0, -4])                 # an eos the search meets
    tok0, sc0 = d.beam_search(mel, prompt, 10, 3, eos, length_penalty)
    tok, sc, st = d.beam_search(mel, prompt, 10, 3, eos, length_penalty, return_stats=True)
    assert torch.equal(tok, tok0) and torch.equal(sc, sc0)
    counts = lengths(tok.tolist(), 3, eos)
    assert st.n_tokens.tolist() == counts and st.n_tokens.dtype == torch.int32
    assert min(counts) < 10, counts
    assert torch.equal(st.sum_logprobs, sc * st.n_tokens.float() ** length_penalty)
    if length_penalty == 1.0:                                              # the score is Whisper's avg_logprob
        assert torch.allclose(st.sum_logprobs / st.n_tokens, sc, rtol=1e-6, atol=0)
    assert_sums_close(st.sum_logprobs.tolist(), teacher_forced_sums(m, mel, tok.tolist(), 3, counts), length_penalty)
    tok_n, _, st_n = d.beam_search(mel, prompt, 10, 3, None, length_penalty, return_stats=True)     # no eos: every token counts
    assert st_n.n_tokens.tolist() == [10] * 3


def test_sample_statistics(torch_cores):                                  # noqa: F811
    m = transcribe_model()
    mel, prompt, _ = gen_inputs("uniform")
    d = m.with_logit_rules(None)
    kw = dict(temperature=0.7, num_samples=3, seed=4)
    eos = int(d.sample(mel, prompt, 10, **kw)[0][0, 1, -5])
    tok0, slp0 = d.sample(mel, prompt, 10, eos_token_id=eos, **kw)
    tok, slp, st = d.sample(mel, prompt, 10, eos_token_id=eos, return_stats=True, **kw)
    assert torch.equal(tok, tok0) and torch.equal(slp, slp0) and torch.equal(st.sum_logprobs, slp)
    assert st.n_tokens.shape == (3, 3) and st.n_tokens.dtype == torch.int32
    flat = [r for item in tok.tolist() for r in item]
    counts = lengths(flat, 3, eos)
    assert st.n_tokens.view(-1).tolist() == counts and min(counts) < 10, counts
    mel3 = mel.repeat_interleave(3, 0)
    assert_sums_close(slp.view(-1).tolist(), teacher_forced_sums(m, mel3, flat, 3, counts), "sample")
    st_n = d.sample(mel, prompt, 10, return_stats=True, **kw)[-1]
    assert st_n.n_tokens.tolist() == [[10] * 3] * 3


# ------------------------------------------------------------------ transcribe under the policy
CLIPS = (130, 100, 90)                         # four, three and three windows of 40 frames
TEMPS = (0.0, 0.4, 0.8)


def zlib_ratio(tokens):
    """a compression ratio from zlib over the token bytes (a tokenizer's text in Whisper)"""
    assert tokens.dtype == torch.int64 and tokens.dim() == 1 and tokens.device.type == "cpu"
    assert EOS not in tokens.tolist()
    raw = tokens.numpy().tobytes()
    return len(raw) / len(zlib.compress(raw)) if raw else 0.0


def naive_policy_transcribe(m, clips, prompt, rules, n_new, window, *, temperatures=(0.0,), logprob_threshold=None,
                            no_speech_threshold=None, no_speech_token_id=None, sot_index=0, compression_ratio_threshold=None,
                            compression_ratio=None, num_samples=1, seed=0, num_beams=1, length_penalty=1.0, graph=False):
    """the policy written out over the public decoders with return_stats=True and ops.timestamp_segments_torch, one row at a
    time on the host -> (per item (starts, ends, tokens, offsets) lists, per item a list of (seek, temperature, avg_logprob,
    no_speech_prob, compression ratio, skipped))"""
    from mop_amd import ops
    B, T_p, eos, nan = len(clips), prompt.shape[-1], rules.eos_token_id, float("nan")
    dev = clips[0].device
    dec = m.with_logit_rules(rules)
    kw = dict(return_stats=True, no_speech_token_id=no_speech_token_id, sot_index=sot_index)
    seek, calls = [0] * B, 0
    out, log = [([], [], [], [0]) for _ in range(B)], [[] for _ in range(B)]
    while any(seek[b] < clips[b].shape[0] for b in range(B)):
        act = [b for b in range(B) if seek[b] < clips[b].shape[0]]
        wins = {b: clips[b][seek[b]:seek[b] + window] for b in act}
        final, todo = {}, list(act)
        for ti, t in enumerate(temperatures):
            pr = prompt.unsqueeze(0).expand(len(todo), -1)
            sub = [wins[b] for b in todo]
            if t == 0 and num_beams > 1:
                rows, _, st = dec.beam_search(sub, pr, n_new, num_beams, eos, length_penalty, graph, **kw)
                rows, avg = rows.tolist(), (st.sum_logprobs / st.n_tokens).tolist()
            elif t == 0:
                rows, st = dec.generate(sub, pr, n_new, eos, graph, **kw)
                rows, avg = rows.tolist(), (st.sum_logprobs / st.n_tokens).tolist()
            else:
                toks, _, st = dec.sample(sub, pr, n_new, temperature=t, num_samples=num_samples, eos_token_id=eos, seed=seed + calls,
                                         graph=graph, **kw)
                calls += 1
                every = (st.sum_logprobs / st.n_tokens).tolist()
                best = [e.index(max(e)) for e in every]                    # ties to the smaller index
                rows, avg = [toks[k, s].tolist() for k, s in enumerate(best)], [e[s] for e, s in zip(every, best)]
            nsp = st.no_speech_prob.tolist() if st.no_speech_prob is not None else [nan] * len(todo)
            again = []
            for k, b in enumerate(todo):
                gen = rows[k][T_p:]
                gen = gen[:gen.index(eos)] if eos in gen else gen
                cr = compression_ratio(torch.tensor(gen, dtype=torch.int64)) if compression_ratio is not None else nan
                final[b] = (rows[k], t, avg[k], nsp[k], cr)
                need = ((compression_ratio_threshold is not None and cr > compression_ratio_threshold)
                        or (logprob_threshold is not None and avg[k] < logprob_threshold))
                if (no_speech_threshold is not None and logprob_threshold is not None and nsp[k] > no_speech_threshold
                        and avg[k] < logprob_threshold):
                    need = False
                if need:
                    again.append(b)
            todo = again
            if not todo or ti + 1 == len(temperatures):
                break
        for b in act:
            row, t, avg_b, nsp_b, cr = final[b]
            wlen = wins[b].shape[0]
            skip = no_speech_threshold is not None and nsp_b > no_speech_threshold
            if skip and logprob_threshold is not None and avg_b > logprob_threshold:
                skip = False
            log[b].append((seek[b], t, avg_b, nsp_b, cr, skip))
            if skip:
                seek[b] += wlen
                continue
            seg = ops.timestamp_segments_torch(torch.tensor([row], dtype=torch.int32, device=dev), T_p,
                                               torch.tensor([wlen], dtype=torch.int32, device=dev), rules.timestamp_begin, eos, 1)
            st_, en, tk, off = out[b]
            for j in range(int(seg.n_segments[0])):
                st_.append(int(seg.starts[0, j]) + seek[b])
                en.append(int(seg.ends[0, j]) + seek[b])
                tk.extend(row[int(seg.tok_begin[0, j]):int(seg.tok_end[0, j])])
                off.append(len(tk))
            seek[b] += int(seg.advance[0])
    return out, log


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def assert_logs_equal(got, want, what=None):
    from mop_amd.nn import TranscribeLog
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, TranscribeLog) and TranscribeLog._fields == ("seek", "temperature", "avg_logprob", "no_speech_prob",
                                                                          "compression_ratio", "skipped")
        rows = list(zip(g.seek, g.temperature, g.avg_logprob, g.no_speech_prob, g.compression_ratio, g.skipped))
        assert len(rows) == len(w), (what, b, rows, w)
        for x, y in zip(rows, w):
            assert all(same(p, q) for p, q in zip(x, y)), (what, b, x, y)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def policy_setup(device="cpu"):
    from mop_amd import ops
    m = transcribe_model().to(device)
    torch.manual_seed(11)
    clips = [torch.randn(n, 10).to(device) for n in CLIPS]
    return m, clips, torch.tensor([7, 8, 9], device=device), ops.LogitRules(V, **RULES)


def run_policy_case(m, clips, prompt, rules, dtype=torch.int64, window=40, **kw):
    """transcribe under the policy against the naive loop -> (transcripts, logs)"""
    want, wlog = naive_policy_transcribe(m, clips, prompt, rules, 12, window, **kw)
    got, glog = m.with_logit_rules(rules).transcribe(clips, prompt, 12, window=window, return_log=True, **kw)
    assert_transcripts_equal(got, want, dtype, kw)
    assert_logs_equal(glog, wlog, kw)
    return got, glog


def fallback_threshold(m, clips, prompt, rules, window=40):
    """the median of the first windows' avg_logprob at temperature 0, read from a return_log run"""
    _, base = m.with_logit_rules(rules).transcribe(clips, prompt, 12, window=window, return_log=True, no_speech_token_id=NO_SPEECH)
    assert all(len(g.seek) >= 3 for g in base), [g.seek for g in base]    # every clip spans at least three windows
    return median([g.avg_logprob[0] for g in base]), base


def check_fallback_case(m, clips, prompt, rules, window=40):
    thr, _ = fallback_threshold(m, clips, prompt, rules, window)
    _, log = run_policy_case(m, clips, prompt, rules, window=window, temperatures=TEMPS, logprob_threshold=thr, seed=3)
    temps = [t for g in log for t in g.temperature]
    assert any(t > 0 for t in temps) and any(t == 0 for t in temps), temps    # the condition: both ways were taken
    return log


def check_skip_case(m, clips, prompt, rules, window=40):
    _, base = fallback_threshold(m, clips, prompt, rules, window)
    thr = median([p for g in base for p in g.no_speech_prob])
    got, log = run_policy_case(m, clips, prompt, rules, window=window, no_speech_threshold=thr, no_speech_token_id=NO_SPEECH)
    n_skipped = 0
    for b, g in enumerate(log):
        for i, skipped in enumerate(g.skipped):
            if not skipped:
                continue
            n_skipped += 1
            lo, hi = g.seek[i], min(g.seek[i] + window, clips[b].shape[0])
            assert (g.seek[i + 1] if i + 1 < len(g.seek) else hi) == hi, (b, g.seek)     # seek moved by the window's length
            assert not any(lo <= s < hi for s in got[b].starts.tolist()), (b, lo, hi, got[b].starts.tolist())
    assert n_skipped >= 1 and not all(s for g in log for s in g.skipped), [g.skipped for g in log]
    return log


def test_transcribe_fallback_equals_the_naive_loop(torch_cores):          # noqa: F811
    check_fallback_case(*policy_setup())


def test_transcribe_skip_equals_the_naive_loop(torch_cores):              # noqa: F811
    check_skip_case(*policy_setup())


def test_transcribe_compression_ratio_and_silence(torch_cores):           # noqa: F811
    m, clips, prompt, rules = policy_setup()
    _, base = m.with_logit_rules(rules).transcribe(clips, prompt, 12, return_log=True, compression_ratio=zlib_ratio,
                                                   no_speech_token_id=NO_SPEECH)
    ratios = [r for g in base for r in g.compression_ratio]
    assert not any(math.isnan(r) for r in ratios)
    _, log = run_policy_case(m, clips, prompt, rules, temperatures=TEMPS, compression_ratio=zlib_ratio,
                             compression_ratio_threshold=median(ratios) - 1e-9, seed=1, num_samples=2)
    temps = [t for g in log for t in g.temperature]
    assert any(t > 0 for t in temps) and any(t == 0 for t in temps), temps
    # all three thresholds at once (rule 3: a silent window does not fall back), beam search at temperature 0
    lp = median([a for g in base for a in g.avg_logprob])
    ns = median([p for g in base for p in g.no_speech_prob])
    run_policy_case(m, clips, prompt, rules, temperatures=(0.0, 0.5), logprob_threshold=lp, no_speech_threshold=ns,
                    no_speech_token_id=NO_SPEECH, sot_index=1, num_beams=2, length_penalty=0.8, seed=9)
    # a first temperature above 0, several samples
    run_policy_case(m, clips[1:], prompt, rules, temperatures=(0.3,), num_samples=3, seed=2)


def test_transcribe_defaults_run_todays_path(torch_cores, monkeypatch):   # noqa: F811
    from mop_amd import ops
    m, clips, prompt, rules = policy_setup()
    calls = []
    monkeypatch.setattr(ops, "greedy_pick", lambda *a, **k: calls.append("greedy_pick") or ops.greedy_pick_torch(*a, **k))
    monkeypatch.setattr(ops, "token_logprob", lambda *a, **k: calls.append("token_logprob") or ops.token_logprob_torch(*a, **k))
    plain = m.transcribe(clips, prompt, rules, 12)
    ruled = m.with_logit_rules(rules).transcribe(clips, prompt, 12)
    assert not calls                                                       # no statistics are asked for
    logged, log = m.with_logit_rules(rules).transcribe(clips, prompt, 12, temperatures=(0.0,), return_log=True)
    assert "greedy_pick" in calls and "token_logprob" not in calls
    for a, b, c in zip(plain, ruled, logged):
        for x, y, z in zip(a, b, c):
            assert x.dtype == y.dtype == z.dtype and torch.equal(x, y) and torch.equal(x, z)
    assert all(math.isnan(p) for g in log for p in g.no_speech_prob + g.compression_ratio)
    assert not any(s for g in log for s in g.skipped) and all(t == 0.0 for g in log for t in g.temperature)


def test_transcribe_policy_value_errors(torch_cores):                     # noqa: F811
    m, clips, prompt, rules = policy_setup()
    d = m.with_logit_rules(rules)
    d.transcribe([clips[2][:17]], prompt, 2, temperatures=0.0)             # one number is a sequence of one
    for kw in (dict(temperatures=()), dict(temperatures=[]), dict(temperatures=(0.0, 0.0)), dict(temperatures=(0.4, 0.2)),
               dict(temperatures=(-0.1,)), dict(temperatures=(0.0, float("nan"))), dict(temperatures=("0",)), dict(temperatures=None),
               dict(temperatures=(0.0, float("inf"))),
               dict(no_speech_threshold=0.5), dict(compression_ratio_threshold=2.4), dict(compression_ratio=2.4),
               dict(num_samples=0), dict(num_samples=9), dict(num_samples=2.0), dict(num_samples=2),
               dict(num_samples=2, temperatures=(0.0,)), dict(logprob_threshold="-1"), dict(logprob_threshold=float("nan")),
               dict(no_speech_threshold=float("nan"), no_speech_token_id=NO_SPEECH), dict(no_speech_token_id=V),
               dict(no_speech_token_id=NO_SPEECH, sot_index=3), dict(sot_index=-1), dict(seed=1.5)):
        with pytest.raises(ValueError):
            d.transcribe(clips, prompt, 4, **kw)
    with pytest.raises(ValueError):
        m.with_logit_rules(None).transcribe(clips, prompt, 4)
    with pytest.raises(ValueError):
        m.transcribe_audio(clips, None, prompt, rules, 4, temperatures=TEMPS)
