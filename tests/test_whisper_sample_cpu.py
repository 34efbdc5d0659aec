"""CPU checks of WhisperMoP sampling (no GPU): signatures and defaults of sample and ops.sample_tokens*,
the support query and bad-argument returns of mopk_sample_*, the ValueErrors raised before any device work, ops.sample_tokens_torch
against a plain-Python restatement of the documented rule on hand-built rows (exact ties at the top-k and nucleus boundaries, -inf
logits, top_k >= V, temperature 0), and sample with every core routed through its torch composition against a naive oracle that
re-runs decode(enc, full ids) for every row at every step."""
import ctypes as C
import inspect
import math
import struct

import pytest
import torch

from test_whisper_beam_cpu import _params, _tiny_model, torch_cores  # noqa: F401  (torch_cores is a fixture)

NEG = float("-inf")
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import WhisperMoP
    e, P = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert _params(WhisperMoP.sample) == dict(mel=(e, P), prompt_ids=(e, P), max_new_tokens=(e, P), temperature=(1.0, P),
                                              top_k=(0, P), top_p=(1.0, P), num_samples=(1, P), eos_token_id=(None, P), seed=(0, P),
                                              graph=(False, P))
    for f in (ops.sample_tokens, ops.sample_tokens_torch, ops.sample_tokens_supported):
        assert _params(f) == dict(logits=(e, P), pos=(e, P), temperature=(1.0, P), top_k=(0, P), top_p=(1.0, P), seed=(0, P),
                                  out=(None, P)), f.__name__


def _args(R=8, n=1, V=51865, bf16=True, top_k=50, top_p=0.95, inv_temp=1.0 / 0.7, greedy=0):
    from mop_amd import _lib
    a = _lib.SampleArgs()
    a.R, a.n, a.V, a.top_k, a.top_p, a.inv_temp, a.greedy = R, n, V, top_k, top_p, inv_temp, greedy
    a.logits_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    a.logits_sb = V
    return a


def test_support_query_and_bad_arguments(lib):
    ok = lambda a: lib.mopk_sample_supported(C.byref(a))
    assert lib.mopk_sample_supported(None) == 0
    for bf16 in (True, False):
        assert ok(_args(bf16=bf16)) == 1 and ok(_args(V=2, bf16=bf16)) == 1 and ok(_args(V=1 << 24, bf16=bf16)) == 1
    assert ok(_args(V=1)) == 0 and ok(_args(V=(1 << 24) + 1)) == 0 and ok(_args(R=0)) == 0 and ok(_args(n=0)) == 0
    a = _args()
    a.logits_dtype = 2
    assert ok(a) == 0
    assert ok(_args(top_k=-1)) == 0 and ok(_args(top_p=0.0)) == 0 and ok(_args(top_p=1.5)) == 0 and ok(_args(top_p=float("nan"))) == 0
    assert ok(_args(inv_temp=0.0)) == 0 and ok(_args(inv_temp=float("inf"))) == 0 and ok(_args(inv_temp=-1.0)) == 0
    assert ok(_args(inv_temp=0.0, top_p=7.0, greedy=1)) == 1 and ok(_args(greedy=2)) == 0
    a = _args()
    a.logits_sk = -1
    assert ok(a) == 0
    a = _args(bf16=False)
    a.logits = 2                                          # not fp32-aligned
    assert ok(a) == 0
    a = _args()
    a.logits = 2                                          # bf16-aligned
    assert ok(a) == 1
    assert lib.mopk_sample_workspace_bytes(C.byref(_args())) == 0
    fn = lib.mopk_sample_step
    assert fn(None, None) == -2
    assert fn(C.byref(_args(V=1)), None) == -1
    assert fn(C.byref(_args(V=(1 << 24) + 1)), None) == -3
    assert fn(C.byref(_args()), None) == -2               # valid shape, null tensors


def test_value_errors_before_device_work():
    from mop_amd import ops
    x, pos = torch.randn(3, 10), torch.tensor([4], dtype=torch.int32)
    bad = [dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=1e-300),
           dict(top_k=-1), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")), dict(top_p=-0.5)]
    for f in (ops.sample_tokens, ops.sample_tokens_torch, ops.sample_tokens_supported):
        for kw in bad:
            with pytest.raises(ValueError):
                f(x, pos, **kw)
        for p in (torch.tensor([[4]], dtype=torch.int32), torch.tensor([4, 5], dtype=torch.int32), torch.tensor(4)):
            with pytest.raises(ValueError, match="pos"):
                f(x, p)
        for lg in (torch.randn(10), torch.randn(2, 3, 10), torch.randn(3, 1)):
            with pytest.raises(ValueError, match="logits"):
                f(lg, pos)
        with pytest.raises(ValueError, match="out"):
            f(x, pos, out=(torch.zeros(4, dtype=torch.int32), torch.zeros(4)))       # 4 rows are not a multiple of 3
        with pytest.raises(ValueError, match="out"):
            f(x, pos, out=(torch.zeros(3, dtype=torch.int64), torch.zeros(3)))
    m = _tiny_model()
    mel, ids = torch.randn(2, 40, 10), torch.zeros(2, 4, dtype=torch.long)
    for kw, msg in ((dict(num_samples=0), "num_samples"), (dict(num_samples=9), "num_samples"), (dict(temperature=-1), "temperature"),
                    (dict(top_k=-3), "top_k"), (dict(top_p=0), "top_p"), (dict(top_p=2), "top_p")):
        with pytest.raises(ValueError, match=msg):
            m.sample(mel, ids, 5, **kw)
    with pytest.raises(ValueError, match="prompt"):
        m.sample(mel, ids[:, :0], 5)
    with pytest.raises(ValueError, match="prompt"):
        m.sample(mel, ids, 0)
    with pytest.raises(ValueError, match="n_text_ctx"):
        m.sample(mel, ids, 61)                           # 4 + 61 > 64


# ---- plain-Python restatement of the rule (steps 1-5 of ops.sample_tokens) ----
def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def py_gumbel(seed, r, pos, v):
    s = seed & 0xFFFFFFFFFFFFFFFF
    rh = _mix(_mix((s & M32) ^ ((r * 0x9E3779B1) & M32)) ^ (s >> 32) ^ ((pos * 0x85EBCA77) & M32))
    h = _mix(rh ^ ((v * 0xC2B2AE3D) & M32))
    u = ((h >> 9) + 0.5) * 2.0 ** -23
    return -math.log(-math.log(u))


def py_sample(x, r, pos, temperature, top_k, top_p, seed):
    """one row (list of fp32 values) -> (token, logprob, kept set, margin between the best and second perturbed scores)"""
    V = len(x)
    mx = max(x)
    lse = mx + math.log(sum(math.exp(v - mx) for v in x if v != NEG))
    if temperature == 0:
        tok = x.index(mx)
        return tok, x[tok] - lse, {tok}, math.inf
    inv = f32(1.0 / temperature)
    z = [f32(v * inv) for v in x]
    kept = set(range(V))
    if 0 < top_k < V:
        zk = sorted(z, reverse=True)[top_k - 1]
        kept = {v for v in range(V) if z[v] >= zk}
    if top_p < 1:
        m = max(z)
        tot = sum(math.exp(z[v] - m) for v in kept)
        tau = max(z[u] for u in kept if sum(math.exp(z[v] - m) for v in kept if z[v] >= z[u]) / tot >= f32(top_p))
        kept = {v for v in kept if z[v] >= tau}
    sc = sorted(((z[v] + py_gumbel(seed, r, pos, v), -v) for v in kept), reverse=True)
    tok = -sc[0][1]
    margin = sc[0][0] - sc[1][0] if len(sc) > 1 else math.inf
    return tok, x[tok] - lse, kept, margin


ROWS = {                                                 # hand-built rows: exact ties at the boundaries, -inf entries
    "topk_tie": [3.0, 1.0, 1.0, 0.5, 1.0, NEG, 2.0, 1.0, -1.0, 0.25, NEG, 0.0],
    "nucleus_tie": [2.0, 1.0, 1.0, 0.0, -1.0, -2.0, 1.0, NEG, -3.0, 0.0],
    "flat": [0.5] * 9,
    "neg_inf": [NEG, -4.0, NEG, -5.0, -4.0, NEG, -6.0],
    "spread": [0.1 * ((7 * v) % 13) - 0.6 for v in range(13)],
}


@pytest.mark.parametrize("name", sorted(ROWS))
@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 1.0), (0.5, 3, 1.0), (2.0, 0, 0.6), (1.0, 4, 0.7), (0.25, 2, 0.9),
                                                     (1.0, 100, 1.0), (1.0, 1, 1.0), (0.0, 0, 1.0), (4.0, 5, 0.3)])
def test_torch_path_matches_the_python_restatement(name, temperature, top_k, top_p):
    from mop_amd import ops
    x = [f32(v) for v in ROWS[name]]
    R, seed = 64, 12345
    lg = torch.tensor([x], dtype=torch.float32)
    seen = set()
    for pos in range(6):
        out = (torch.zeros(R, dtype=torch.int32), torch.zeros(R))
        tok, lp = ops.sample_tokens(lg, torch.tensor([pos], dtype=torch.int32), temperature, top_k, top_p, seed, out=out)
        assert tok.data_ptr() == out[0].data_ptr() and lp.data_ptr() == out[1].data_ptr()
        for r in range(R):
            want, wlp, kept, margin = py_sample(x, r, pos, temperature, top_k, top_p, seed)
            assert margin > 1e-5
            assert int(tok[r]) == want, (r, pos)
            assert abs(float(lp[r]) - wlp) < 1e-5
            seen.add(int(tok[r]))
    assert seen <= kept
    if temperature > 0:                                  # every kept token of probability >= 3 % is drawn somewhere (384 draws)
        z = [f32(v * f32(1.0 / temperature)) for v in x]
        mz = max(z)
        tot = sum(math.exp(z[v] - mz) for v in kept)
        assert {v for v in kept if math.exp(z[v] - mz) / tot >= 0.03} <= seen


def test_tie_rules_are_inclusive():
    x = [f32(v) for v in ROWS["topk_tie"]]
    assert py_sample(x, 0, 0, 1.0, 3, 1.0, 0)[2] == {0, 6, 1, 2, 4, 7}           # the k-th largest (1.0) is tied four times
    x = [f32(v) for v in ROWS["nucleus_tie"]]
    p2 = math.exp(2) / (math.exp(2) + 3 * math.exp(1))
    assert py_sample(x, 0, 0, 1.0, 4, (p2 + 1) / 2, 0)[2] == {0, 1, 2, 6}         # the nucleus ends inside a tie group
    assert py_sample(x, 0, 0, 1.0, 4, p2 * 0.99, 0)[2] == {0}


def test_top_k_at_or_above_v_is_off_and_temperature_zero_is_argmax():
    from mop_amd import ops
    torch.manual_seed(5)
    x = torch.randn(16, 30)
    x[3, 7] = x[3, 21] = 9.0                              # a tied maximum: the smaller index
    pos = torch.tensor([11], dtype=torch.int32)
    off = ops.sample_tokens(x, pos, 0.8, 0, 1.0, 3)
    for k in (30, 31, 10 ** 9):
        got = ops.sample_tokens(x, pos, 0.8, k, 1.0, 3)
        assert torch.equal(got[0], off[0]) and torch.equal(got[1], off[1])
    tok, lp = ops.sample_tokens(x, pos, 0.0, 5, 0.5, 99)
    assert torch.equal(tok.long(), x.argmax(-1)) and int(tok[3]) == 7
    assert torch.allclose(lp, torch.log_softmax(x, -1).gather(1, tok.long().unsqueeze(1)).squeeze(1))
    assert ops.sample_tokens(x, pos, 0.8, seed=4)[0].tolist() != off[0].tolist()  # the seed changes the draws


def test_shared_rows_equal_expanded_rows():
    from mop_amd import ops
    torch.manual_seed(6)
    x = torch.randn(3, 40)
    pos = torch.tensor([2], dtype=torch.int32)
    out = (torch.zeros(12, dtype=torch.int32), torch.zeros(12))
    a = ops.sample_tokens(x, pos, 1.3, 7, 0.8, 17, out=out)
    b = ops.sample_tokens(x.repeat_interleave(4, 0), pos, 1.3, 7, 0.8, 17)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@torch.no_grad()
def naive_sample(m, mel, prompt, n_new, n, temperature, top_k, top_p, seed, eos=None):
    """the documented sampling, re-running decode(enc, full ids) for every row at every step and drawing each row with py_sample ->
    (tokens (B, n, T_p + n_new), sum_logprobs (B, n), the smallest draw margin)"""
    enc, _ = m.encode(mel)
    B, Tp = prompt.shape
    seqs = [prompt[b].tolist() for b in range(B) for _ in range(n)]
    sums, done, margin = [0.0] * (B * n), [False] * (B * n), math.inf
    for t in range(n_new):
        for r in range(B * n):
            ids = torch.tensor([seqs[r]], dtype=prompt.dtype)
            x = m.decode(enc[r // n:r // n + 1], ids)[0, -1].float().tolist()
            tok, lp, _, mg = py_sample(x, r, Tp + t, temperature, top_k, top_p, seed)
            if done[r]:
                tok = eos
            else:
                margin = min(margin, mg)
                sums[r] += lp
                done[r] = eos is not None and tok == eos
            seqs[r].append(tok)
    return torch.tensor(seqs, dtype=prompt.dtype).view(B, n, -1), torch.tensor(sums).view(B, n), margin


@pytest.mark.parametrize("n", [1, 3])
def test_sample_matches_the_naive_oracle_with_torch_cores(torch_cores, n):
    m = _tiny_model()
    torch.manual_seed(13)
    mel = torch.randn(2, 40, 10)
    prompt = torch.randint(0, 100, (2, 3))
    cfg = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7)
    tok, lp = m.sample(mel, prompt, 10, num_samples=n, **cfg)
    ref, rlp, margin = naive_sample(m, mel, prompt, 10, n, **cfg)
    assert margin > 1e-4
    assert torch.equal(tok, ref) and torch.allclose(lp, rlp, atol=1e-4, rtol=1e-5)
    assert tok.shape == (2, n, 13) and tok.dtype == prompt.dtype and lp.dtype == torch.float32
    eos = int(tok[0, 0, 3 + 3])                            # sample 0 of item 0 emits it as its 4th token
    tok, lp = m.sample(mel, prompt, 10, num_samples=n, eos_token_id=eos, **cfg)
    ref, rlp, margin = naive_sample(m, mel, prompt, 10, n, eos=eos, **cfg)
    assert margin > 1e-4
    assert torch.equal(tok, ref) and torch.allclose(lp, rlp, atol=1e-4, rtol=1e-5)
    assert (tok[0, 0, 6:] == eos).all()
    for nb in range(n):                                     # the samples of an item differ
        assert n == 1 or not torch.equal(tok[:, 0], tok[:, nb]) or nb == 0


def test_temperature_zero_is_greedy_with_torch_cores(torch_cores):
    m = _tiny_model()
    mel, prompt = torch.randn(2, 40, 10), torch.randint(0, 100, (2, 3))
    greedy = m.generate(mel, prompt, 12)
    tok, _ = m.sample(mel, prompt, 12, temperature=0.0, num_samples=2)
    assert torch.equal(tok[:, 0], greedy) and torch.equal(tok[:, 1], greedy)
    tok, _ = m.sample(mel, prompt, 12, temperature=1.5, top_k=1)
    assert torch.equal(tok[:, 0], greedy)
