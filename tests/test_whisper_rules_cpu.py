"""CPU checks of Whisper's logit rules (no GPU): ops.logit_rules_torch against a restatement written here (a plain per-row loop in
rule order, rule 3e in float64, no call into ops) over three vocabulary shapes, 1 / 3 / 16 rows, fp32 / bf16 and hand-built
histories that reach every branch; both outcomes of the dominance rule on random rows and on hand-built ones; every ValueError;
and generate / beam_search / sample under rules with every core on its torch composition, whose
outputs must obey the timestamp grammar.  The decoders' own signatures are pinned by the older tests, so the rules come in through
WhisperMoP.with_logit_rules(rules)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_whisper_beam_cpu import _tiny_model
from test_whisper_ragged_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition)

NEG = float("-inf")
T0 = 3                                                       # prompt columns in front of the generated tokens
NEAR_TIE = 1e-4                                              # float64 |L - M| below which rule 3e may go either way in fp32
SHAPES = {"v131": (131, 101, 97), "v64": (64, 63, 40), "v51865": (51865, 50364, 50257)}      # V, tb, eos


def ref_rules(x, hist, pos, t0, V, suppress_tokens=(), suppress_at_begin=(), timestamp_begin=None, eos_token_id=None,
              no_timestamps_token_id=None, max_initial_timestamp_index=None):
    """the rules as the issue states them, row by row in rule order -> (blocked (R, V) bool array, float64 margins |L - M| of
    rule 3e (inf where a side is empty or the rule is off))"""
    x64 = x.detach().double().cpu().numpy()
    R = x64.shape[0]
    blocked, margins = np.zeros((R, V), dtype=bool), np.full(R, math.inf)
    tb, eos, k = timestamp_begin, eos_token_id, max_initial_timestamp_index
    for r in range(R):
        b = blocked[r]
        g = [int(t) for t in hist[r, t0:pos]]
        n = len(g)
        for s in suppress_tokens:                            # 1
            b[s] = True
        if n == 0:                                           # 2
            for s in suppress_at_begin:
                b[s] = True
        if tb is None:
            continue
        if no_timestamps_token_id is not None:               # 3a
            b[no_timestamps_token_id] = True
        last = n >= 1 and g[n - 1] >= tb                     # 3b
        pen = n < 2 or g[n - 2] >= tb
        if last and pen:
            b[tb:] = True
        if last and not pen:
            b[:eos] = True
        stamps = [t for t in g if t >= tb]                   # 3c
        if stamps:
            t = stamps[-1]
            b[tb:(t if last and not pen else t + 1)] = True
        if n == 0:                                           # 3d
            b[:tb] = True
            if k is not None:
                b[tb + k + 1:] = True
        xr = np.where(b, -np.inf, x64[r])                    # 3e
        m = xr[tb:].max()
        L = m + math.log(np.exp(xr[tb:] - m).sum()) if m > -np.inf else -math.inf
        M = xr[:tb].max()
        if math.isfinite(L) and math.isfinite(M):
            margins[r] = abs(L - M)
        if L > M:
            b[:tb] = True
    return blocked, margins


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_rows_match(out, x, blocked, margins, what):
    """out is x with exactly `blocked` set to -inf, on every row outside the near-tie exclusion -> the number of rows left out"""
    keep = torch.from_numpy(margins >= NEAR_TIE)
    want = torch.from_numpy(blocked)
    out, x = out.cpu(), x.cpu()
    assert out.dtype == x.dtype and out.shape == x.shape, what
    assert torch.equal(torch.isneginf(out)[keep], want[keep]), what
    same = (bits(out) == bits(x)) | want
    assert bool(same[keep].all()), what
    return int((~keep).sum())


def histories(V, tb, eos):
    """name -> generated tokens, reaching every branch of rule 3 (x: a text token, the rows' own are drawn at random)"""
    s = lambda d: min(tb + d, V - 1)                         # noqa: E731  a timestamp, inside the vocabulary
    return {
        "n0": [], "text": ["x"], "stamp": [s(2)], "text-stamp": ["x", s(3)], "stamp-stamp": [s(1), s(1)], "stamp-text": [s(1), "x"],
        "pairs-then-lone": [s(0), "x", "x", s(2), s(2), "x", s(4), s(4), "x", s(5)],
        "pairs-then-pair": [s(0), "x", s(2), s(2), "x", "x", s(6), s(6)],
        "pairs-then-text": [s(0), "x", s(2), s(2), "x", s(3), s(3), "x", "x"],
        "last-is-V-1-lone": ["x", V - 1], "last-is-V-1-pair": [V - 1, V - 1], "last-is-V-1-then-text": [s(0), "x", V - 1, V - 1, "x"],
    }


def rule_sets(V, tb, eos):
    """name -> LogitRules keywords"""
    sup = sorted({1, 7, eos - 1, tb - 1, V - 2} - {eos})
    full = dict(suppress_tokens=sup, suppress_at_begin=[0, eos], timestamp_begin=tb, eos_token_id=eos, no_timestamps_token_id=tb - 2)
    return {"full": full, "k0": dict(full, max_initial_timestamp_index=0), "k5": dict(full, max_initial_timestamp_index=5),
            "bare": dict(timestamp_begin=tb, eos_token_id=eos), "no-timestamps": dict(suppress_tokens=sup, suppress_at_begin=[0, eos])}


def build_case(V, tb, eos, R, dtype, g, seed, device="cpu", cap=16):
    """(x (R, V) standard normal with a per-row offset uniform in [-6, 2] on the timestamps, hist (R, cap) int32, pos (1,) int32)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=gen)
    x[:, tb:] += torch.rand(R, 1, generator=gen) * 8 - 6
    hist = torch.randint(0, V, (R, cap), generator=gen).to(torch.int32)           # prompt and tail: anything, never read
    for r in range(R):
        for i, t in enumerate(g):
            hist[r, T0 + i] = int(torch.randint(0, tb, (1,), generator=gen)) if t == "x" else t
    pos = torch.tensor([T0 + len(g)], dtype=torch.int32)
    return x.to(dtype).to(device), hist.to(device), pos.to(device)


def sweep(fn, shape, R, dtype, device="cpu"):
    """fn(x, hist, pos, T0, rules) against ref_rules over every history x rule set of a vocabulary shape -> (rows, rows left out)"""
    from mop_amd import ops
    V, tb, eos = SHAPES[shape]
    rows = left_out = 0
    for ri, (rname, kw) in enumerate(rule_sets(V, tb, eos).items()):
        rules = ops.LogitRules(V, **kw)
        for hi, (hname, g) in enumerate(histories(V, tb, eos).items()):
            if rname in ("k0", "k5") and g:
                continue                                     # max_initial_timestamp_index acts at n = 0 only
            x, hist, pos = build_case(V, tb, eos, R, dtype, g, 1000 * ri + hi, device)
            out = fn(x, hist, pos, T0, rules)
            blocked, margins = ref_rules(x, hist.cpu(), int(pos), T0, V, **kw)
            left_out += assert_rows_match(out, x, blocked, margins, (shape, rname, hname))
            rows += R
    return rows, left_out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,R", [("v131", 1), ("v131", 3), ("v131", 16), ("v64", 1), ("v64", 3), ("v64", 16), ("v51865", 3)])
def test_torch_path_matches_the_restatement(shape, R, dtype):
    from mop_amd import ops
    rows, left_out = sweep(ops.logit_rules_torch, shape, R, dtype)
    print(f"{shape} R={R} {dtype}: {left_out} of {rows} rows left out as near ties")
    assert left_out <= 0.02 * rows


def test_the_sweep_reaches_every_branch():
    """the restatement's own view of the sweep: each block of rule 3 both fires and stays silent somewhere"""
    V, tb, eos = SHAPES["v131"]
    kw = rule_sets(V, tb, eos)["bare"]
    seen = {}
    for name, g in histories(V, tb, eos).items():
        x, hist, pos = build_case(V, tb, eos, 1, torch.float32, g, 5)
        x[0, tb:] -= 40                                      # dominance off: rules 3b-3d alone
        b = ref_rules(x, hist, int(pos), T0, V, **kw)[0][0]
        seen[name] = (bool(b[:eos].all()), bool(b[eos:tb].all()), int(b[tb:].sum()))
    assert seen["n0"] == (True, True, 0) and seen["text"] == (False, False, 0)
    assert seen["stamp"] == (False, False, V - tb) and seen["stamp-stamp"] == (False, False, V - tb)
    assert seen["text-stamp"] == (True, False, 3) and seen["stamp-text"] == (False, False, 2)
    assert seen["pairs-then-lone"] == (True, False, 5) and seen["pairs-then-text"] == (False, False, 4)
    assert seen["last-is-V-1-lone"] == (True, False, V - tb - 1) and seen["last-is-V-1-then-text"] == (False, False, V - tb)


def test_out_buffer_aliasing_and_strides_on_the_torch_path():
    from mop_amd import ops
    V, tb, eos = SHAPES["v131"]
    kw = rule_sets(V, tb, eos)["full"]
    rules = ops.LogitRules(V, **kw)
    x, hist, pos = build_case(V, tb, eos, 4, torch.float32, ["x", tb + 3], 3)
    want = ops.logit_rules_torch(x, hist, pos, T0, rules)
    wide = torch.zeros(4, V + 5)
    wide[:, :V] = x
    big = hist.repeat_interleave(3, 0)
    got = ops.logit_rules_torch(wide[:, :V], big[::3], pos, T0, rules, out=wide[:, :V])
    assert got.data_ptr() == wide.data_ptr() and torch.equal(bits(wide[:, :V]), bits(want))
    assert ops.logit_rules(x, hist, pos, T0, rules).equal(want) and ops.LAST_PATH["logit_rules"] == 1     # CPU: the torch path


def test_dominance_takes_both_outcomes():
    from mop_amd import ops
    V, tb, eos = SHAPES["v131"]
    R = 2000
    kw = dict(timestamp_begin=tb, eos_token_id=eos)
    x, hist, pos = build_case(V, tb, eos, R, torch.float32, ["x"], 11)            # one text token: both sides are open
    blocked, margins = ref_rules(x, hist, int(pos), T0, V, **kw)
    forced = blocked[:, :tb].all(1)
    assert forced.mean() >= 0.10 and (~forced).mean() >= 0.10, forced.mean()
    assert not blocked[~forced].any() and not blocked[:, tb:].any()
    left_out = assert_rows_match(ops.logit_rules_torch(x, hist, pos, T0, ops.LogitRules(V, **kw)), x, blocked, margins, "dominance")
    print(f"dominance: {left_out} of {R} rows left out as near ties; timestamps forced in {int(forced.sum())}")
    assert left_out <= 0.02 * R


def test_dominance_on_hand_built_rows():
    from mop_amd import ops
    V, tb, eos = SHAPES["v131"]
    kw = dict(timestamp_begin=tb, eos_token_id=eos)
    x = torch.full((4, V), -30.0)
    x[:, 3] = 0.0                                            # M = 0 (the other text tokens add nothing to a max)
    x[0, tb + 1] = 1.0                                       # L = 1 + 29 e^-31: margin +1 -> timestamps forced
    x[1, tb + 1] = -1.0                                      # margin -1 -> text stays
    x[2, tb + 1] = 1.0                                       # a complete pair blocks every timestamp: L = -inf -> text stays
    x[3, tb + 1] = -1.0                                      # every text token suppressed: M = -inf, L > M
    hist = torch.zeros(4, 8, dtype=torch.int32)
    hist[:, T0:T0 + 2] = torch.tensor([[5, 6], [5, 6], [tb, tb], [5, 6]])
    pos = torch.tensor([T0 + 2], dtype=torch.int32)
    for rows, extra in (([0, 1, 2], {}), ([3], dict(suppress_tokens=range(tb)))):
        rules = ops.LogitRules(V, **kw, **extra)
        sel = torch.tensor(rows)
        out = ops.logit_rules_torch(x[sel], hist[sel], pos, T0, rules)
        blocked, margins = ref_rules(x[sel], hist[sel], int(pos), T0, V, **kw, **extra)
        assert assert_rows_match(out, x[sel], blocked, margins, rows) == 0
        for i, r in enumerate(rows):
            text_blocked, stamps_blocked = bool(torch.isneginf(out[i, :tb]).all()), bool(torch.isneginf(out[i, tb:]).all())
            assert (text_blocked, stamps_blocked) == {0: (True, False), 1: (False, False), 2: (False, True), 3: (True, False)}[r], r
    assert margins[0] == math.inf                            # row 3: an empty side is no near tie


def test_argument_errors():
    from mop_amd import ops
    from mop_amd.nn import LogitRules
    assert LogitRules is ops.LogitRules
    V = 100
    ok = dict(timestamp_begin=80, eos_token_id=70)
    for kw in (dict(suppress_tokens=[100]), dict(suppress_tokens=[-1]), dict(suppress_at_begin=[100]), dict(suppress_at_begin=[1.5]),
               dict(timestamp_begin=100, eos_token_id=70), dict(timestamp_begin=80), dict(timestamp_begin=80, eos_token_id=80),
               dict(timestamp_begin=80, eos_token_id=90), dict(ok, eos_token_id=-1), dict(ok, no_timestamps_token_id=100),
               dict(ok, max_initial_timestamp_index=-1), dict(eos_token_id=100)):
        with pytest.raises(ValueError):
            LogitRules(V, **kw)
    with pytest.raises(ValueError):
        LogitRules(1)
    r = LogitRules(V, **ok, suppress_tokens=(3,), suppress_at_begin=(4,), no_timestamps_token_id=78, max_initial_timestamp_index=10 ** 12)
    t = r.table("cpu")
    assert t.dtype == torch.uint8 and t.shape == (V,) and t.nonzero().flatten().tolist() == [3, 4, 78] and int(t[4]) == 2
    x, hist, pos = torch.zeros(2, V), torch.zeros(2, 8, dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    for f in (ops.logit_rules, ops.logit_rules_torch, ops.logit_rules_supported):
        for args in ((x[:, :50], hist, pos, 3, r), (x, hist[:1], pos, 3, r), (x, hist.float(), pos, 3, r), (x, hist, pos, 9, r),
                     (x, hist, pos, -1, r), (x, hist, torch.zeros(2, dtype=torch.int32), 3, r), (x, hist, pos, 3, None),
                     (x, hist, pos, 3, r, torch.zeros(2, V, dtype=torch.bfloat16))):
            with pytest.raises(ValueError):
                f(*args)
    assert ops.logit_rules_supported(x, hist, pos, 3, r) is False                 # CPU tensors: the torch path
    m = _tiny_model()
    mel, ids = torch.randn(2, 40, 10), torch.randint(0, 100, (2, 4))
    with pytest.raises(ValueError):
        m.with_logit_rules(LogitRules(99))                   # another vocabulary
    with pytest.raises(ValueError):
        m.with_logit_rules("rules")
    d = m.with_logit_rules(r)
    for call in (lambda: d.generate(mel, ids, 5, eos_token_id=71), lambda: d.beam_search(mel, ids, 5, 2, eos_token_id=71),
                 lambda: d.sample(mel, ids, 5, eos_token_id=71)):
        with pytest.raises(ValueError):                      # before any device work: a CPU encode would raise RuntimeError
            call()


def test_support_query_and_bad_arguments_need_no_gpu():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    lib = _lib.lib()
    a = _lib.LogitRulesArgs()
    a.R, a.V, a.dtype, a.T, a.T0, a.tb, a.eos, a.max_initial = 2, 100, _lib.MOPK_F32, 16, 3, 80, 70, -1
    a.logits_ld = a.out_ld = 100
    a.hist_ld = 16
    assert lib.mopk_logit_rules_supported(C.byref(a)) == 1
    assert lib.mopk_logit_rules(C.byref(a), None) != 0       # null pointers: refused before any launch
    for field, bad in (("V", 1), ("R", 0), ("dtype", 7), ("T0", 17), ("T0", -1), ("tb", 100), ("eos", 80), ("eos", -1), ("logits_ld", 99),
                       ("out_ld", 99), ("hist_ld", 15), ("max_initial", -2), ("tb", -2)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.mopk_logit_rules_supported(C.byref(a)) == 0, (field, bad)
        assert lib.mopk_logit_rules(C.byref(a), None) != 0, (field, bad)
        setattr(a, field, keep)
    a.tb, a.eos = -1, 0                                      # rule 3 off: eos is not looked at
    assert lib.mopk_logit_rules_supported(C.byref(a)) == 1


# ---- the grammar of a decoded row (shared with the GPU tests) ----
def check_grammar(tokens, kw, what=""):
    """tokens: one row's generated tokens.  Up to its first eos: no suppressed id; the first token is a timestamp in [tb, tb + k] and
    no suppress_at_begin id; timestamps never decrease; after the first timestamp or a complete pair comes no timestamp; after a lone
    timestamp that follows text comes an equal-or-later timestamp or eos"""
    tb, eos, k = kw["timestamp_begin"], kw["eos_token_id"], kw.get("max_initial_timestamp_index")
    g = [int(t) for t in tokens]
    if eos in g:
        g = g[:g.index(eos) + 1]
    never = set(kw.get("suppress_tokens", ())) | {kw.get("no_timestamps_token_id")}
    assert not never & set(g), (what, g)
    assert g[0] not in kw.get("suppress_at_begin", ()), (what, g)
    assert tb <= g[0] <= (tb + k if k is not None else math.inf), (what, g)
    stamps = [t for t in g if t >= tb]
    assert stamps == sorted(stamps), (what, g)
    for i in range(len(g) - 1):
        if g[i] < tb:
            continue
        if i == 0 or g[i - 1] >= tb:                         # the first timestamp, or the second of a pair: text (or eos) follows
            assert g[i + 1] < tb, (what, i, g)
        else:                                                # a lone timestamp after text
            assert g[i + 1] == eos or g[i + 1] >= g[i], (what, i, g)


MODEL_RULES = dict(suppress_tokens=[1, 2, 50, 79], suppress_at_begin=[5, 70], timestamp_begin=80, eos_token_id=70,
                   no_timestamps_token_id=78, max_initial_timestamp_index=3)


def _peaked_tiny_model():
    m = _tiny_model()
    with torch.no_grad():
        m.dec_ln_f.weight.mul_(20.0)                         # at the default init the timestamps always outweigh the best text token
    return m


def test_decoders_obey_the_grammar_with_torch_cores(torch_cores):
    from mop_amd import ops
    m = _peaked_tiny_model()
    torch.manual_seed(3)
    mel, prompt = torch.randn(3, 40, 10), torch.randint(0, 70, (3, 3))
    d = m.with_logit_rules(ops.LogitRules(100, **MODEL_RULES))
    n_new, kinds = 24, set()
    out, steps = d.generate(mel, prompt, n_new, return_logits=True)
    assert out.shape == (3, 3 + n_new) and steps.shape == (3, n_new, 100)
    assert torch.equal(steps.argmax(-1), out[:, 3:])         # the returned logits are the filtered ones: they chose the tokens
    assert bool(torch.isneginf(steps[:, 0, :80]).all()) and bool(torch.isneginf(steps[:, :, 50]).all())
    runs = {"generate": out[:, 3:], "generate-eos": d.generate(mel, prompt, n_new, eos_token_id=70)[:, 3:],
            "beam": d.beam_search(mel, prompt, n_new, 3, eos_token_id=70)[0][:, 3:],
            "beam-no-eos": d.beam_search(mel, prompt, n_new, 3)[0][:, 3:],
            "sample": d.sample(mel, prompt, n_new, temperature=0.9, top_k=30, num_samples=2, eos_token_id=70, seed=5)[0][:, :, 3:]}
    for name, toks in runs.items():
        for i, row in enumerate(toks.reshape(-1, n_new)):
            check_grammar(row.tolist(), MODEL_RULES, (name, i))
            kinds |= {"text" if t < 80 else "stamp" for t in row.tolist()}
    assert kinds == {"text", "stamp"}                        # the runs emit both kinds: the grammar had something to decide
    ragged = d.generate(mel, [prompt[0], prompt[1, :2], prompt[2, :1]], n_new)
    for i, row in enumerate(ragged):
        check_grammar(row[3 - i:].tolist(), MODEL_RULES, ("ragged", i))
    plain = m.generate(mel, prompt, 8)
    assert torch.equal(m.with_logit_rules(None).generate(mel, prompt, 8), plain)
    assert not torch.equal(plain, out[:, :11])


@torch.no_grad()
def test_sample_sums_the_filtered_log_probabilities(torch_cores):
    from mop_amd import ops
    m = _peaked_tiny_model()
    torch.manual_seed(4)
    mel, prompt = torch.randn(2, 40, 10), torch.randint(0, 70, (2, 3))
    rules = ops.LogitRules(100, **MODEL_RULES)
    tok, lp = m.with_logit_rules(rules).sample(mel, prompt, 6, temperature=0.8, num_samples=2, seed=9)
    enc, _ = m.encode(mel)
    for b in range(2):
        for s in range(2):
            total = 0.0
            for t in range(6):
                ids = tok[b, s, :3 + t].unsqueeze(0)
                raw = m.decode(enc[b:b + 1], ids)[:, -1]
                blocked, _ = ref_rules(raw, ids.to(torch.int32), 3 + t, 3, 100, **MODEL_RULES)
                x = raw.double().masked_fill(torch.from_numpy(blocked), NEG)
                total += float(torch.log_softmax(x, -1)[0, tok[b, s, 3 + t]])
            assert math.isfinite(total) and abs(total - float(lp[b, s])) <= 1e-3, (b, s, total, float(lp[b, s]))
