"""CPU checks of ragged WhisperMoP decoding (prompts of different lengths, no GPU): signatures of the new ops,
the support queries and bad-argument returns of mopk_decode_attn_ragged_* / mopk_sample_ragged_*
(no launch), the ValueErrors raised before any device work, ops.decode_attention_ragged_torch against a float64 loop, and generate /
beam_search / sample on ragged prompt lists with every core routed through its torch composition: row b against the same call on
prompt b alone (generate) or on a batch whose every row holds prompt b (beam_search, sample)."""
import ctypes as C
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from test_whisper_beam_cpu import _params, _tiny_model

NEG = float("-inf")
BAD_SHAPE, BAD_ARG, UNSUPPORTED = -1, -2, -3             # MopkStatus


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


@pytest.fixture
def torch_cores(monkeypatch):
    """route every core through its torch composition (the ragged prefill's key-padding mask included) so the module logic runs on
    the CPU"""
    from mop_amd import ops

    def sdpa(q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p=0.0, seed=None):
        qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
        s = qt @ kt.transpose(-1, -2) * q.shape[-1] ** -0.5
        if bias is not None:
            s = s + bias
        if attn_mask is not None:
            s = s.masked_fill(attn_mask == 0, NEG)
        if causal:
            N = q.shape[1]
            s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), NEG)
        y = torch.softmax(s, -1).nan_to_num(0.0) @ vt                       # a row with no open key is 0, as the cores
        return y.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)

    monkeypatch.setattr(ops, "sdpa_core", sdpa)
    monkeypatch.setattr(ops, "decode_attention", lambda q, k, v, kv_len=None, nk=None, causal=False:
                        ops.decode_attention_torch(q, k, v, kv_len, nk, causal))
    monkeypatch.setattr(ops, "decode_attention_rows", ops.decode_attention_rows_torch)
    monkeypatch.setattr(ops, "decode_attention_ragged", ops.decode_attention_ragged_torch)
    monkeypatch.setattr(ops, "beam_step", ops.beam_step_torch)
    monkeypatch.setattr(ops, "sample_tokens", ops.sample_tokens_torch)
    monkeypatch.setattr(ops, "sample_tokens_ragged", ops.sample_tokens_ragged_torch)


def test_signatures():
    from mop_amd import ops
    e, P = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD
    da = dict(q=(e, P), k_cache=(e, P), v_cache=(e, P), kv_start=(e, P), rows=(None, P), kv_len=(None, P), nk=(None, P),
              causal=(False, P))
    for f in (ops.decode_attention_ragged, ops.decode_attention_ragged_torch, ops.decode_attention_ragged_supported):
        assert _params(f) == da, f.__name__
    sp = dict(logits=(e, P), pos=(e, P), pos_off=(e, P), temperature=(1.0, P), top_k=(0, P), top_p=(1.0, P), seed=(0, P),
              out=(None, P))
    for f in (ops.sample_tokens_ragged, ops.sample_tokens_ragged_torch, ops.sample_tokens_ragged_supported):
        assert _params(f) == sp, f.__name__


def _da(B=2, H=4, Tq=1, dk=64, cap=448, bf16=True):
    from mop_amd import _lib
    a = _lib.DecodeAttnRaggedArgs()
    b = a.base
    b.B, b.H, b.Tq, b.dk, b.cap, b.Nk, b.causal = B, H, Tq, dk, cap, cap, 1
    b.io_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    for v in (b.q, b.k, b.v, b.y):
        v.sb, v.sn, v.sh = cap * H * dk, H * dk, dk
    a.kv_start = 256                                      # an aligned stand-in: the queries never dereference it
    return a


def test_decode_attn_ragged_support_query_and_bad_arguments(lib):
    a = _da()
    assert lib.mopk_decode_attn_ragged_supported(C.byref(a)) == 1
    assert lib.mopk_decode_attn_ragged_workspace_bytes(C.byref(a)) == lib.mopk_decode_attn_workspace_bytes(C.byref(a.base)) > 0
    a.rows, a.rows_ld = 512, 448
    assert lib.mopk_decode_attn_ragged_supported(C.byref(a)) == 1
    cases = [("kv_start", None, BAD_ARG), ("kv_start", 258, UNSUPPORTED),
             ("rows_ld", 447, BAD_SHAPE), ("rows", 514, UNSUPPORTED)]
    for field, val, rc in cases:
        a = _da()
        a.rows, a.rows_ld = 512, 448
        setattr(a, field, val)
        assert lib.mopk_decode_attn_ragged_supported(C.byref(a)) == 0, field
        assert lib.mopk_decode_attn_ragged_workspace_bytes(C.byref(a)) == 0, field
        assert lib.mopk_decode_attn_ragged_fwd(C.byref(a), None) == rc, field
    for field, val in [("Tq", 17), ("dk", 96)]:                # the base call's checks, before any launch
        a = _da()
        setattr(a.base, field, val)
        assert lib.mopk_decode_attn_ragged_fwd(C.byref(a), None) == UNSUPPORTED, field
    a = _da()
    a.base.B = 0
    assert lib.mopk_decode_attn_ragged_fwd(C.byref(a), None) == BAD_SHAPE
    assert lib.mopk_decode_attn_ragged_fwd(None, None) == BAD_ARG
    a = _da()                                              # null q / k / v / y / workspace: refused, nothing launched
    assert lib.mopk_decode_attn_ragged_fwd(C.byref(a), None) == BAD_ARG


def test_sample_ragged_support_query_and_bad_arguments(lib):
    from mop_amd import _lib
    from test_whisper_sample_cpu import _args
    a = _lib.SampleRaggedArgs()
    a.base, a.pos_off = _args(), 256
    assert lib.mopk_sample_ragged_supported(C.byref(a)) == 1
    assert lib.mopk_sample_ragged_workspace_bytes(C.byref(a)) == 0
    assert lib.mopk_sample_ragged_step(C.byref(a), None) == BAD_ARG       # null logits / pos / out: no launch
    for val, rc in [(None, BAD_ARG), (258, UNSUPPORTED)]:
        a.pos_off = val
        assert lib.mopk_sample_ragged_supported(C.byref(a)) == 0
        assert lib.mopk_sample_ragged_step(C.byref(a), None) == rc
    a.base, a.pos_off = _args(V=1), 256
    assert lib.mopk_sample_ragged_step(C.byref(a), None) == BAD_SHAPE
    a.base = _args(top_p=1.5)
    assert lib.mopk_sample_ragged_step(C.byref(a), None) == BAD_ARG
    assert lib.mopk_sample_ragged_step(None, None) == BAD_ARG


def test_value_errors_before_device_work(torch_cores):
    m = _tiny_model()
    mel = torch.randn(2, 40, 10)
    good = [torch.tensor([1, 2, 3]), torch.tensor([4])]
    bad = [([], "non-empty list"), ([torch.tensor([1])], "2 mel"), ([torch.tensor([1, 2]), torch.tensor([], dtype=torch.long)], "1-D"),
           ([torch.tensor([[1, 2]]), torch.tensor([3])], "1-D"), ([torch.tensor([1.0]), torch.tensor([2.0])], "integer dtype"),
           ([torch.tensor([1]), torch.tensor([2], dtype=torch.int32)], "integer dtype"), ((torch.tensor([1]), [2]), "1-D")]
    for prompts, msg in bad:
        with pytest.raises(ValueError, match=msg):
            m.generate(mel, prompts, 4)
        with pytest.raises(ValueError, match=msg):
            m.beam_search(mel, prompts, 4, 2)
        with pytest.raises(ValueError, match=msg):
            m.sample(mel, prompts, 4)
    long = [torch.zeros(61, dtype=torch.long), torch.tensor([1])]        # n_text_ctx = 64
    for call in (lambda p: m.generate(mel, p, 4), lambda p: m.beam_search(mel, p, 4, 2), lambda p: m.sample(mel, p, 4)):
        with pytest.raises(ValueError, match="n_text_ctx"):
            call(long)
        call([long[0][:60], long[1]])                                    # 60 + 4 = 64 fits
    with pytest.raises(ValueError, match="num_beams"):
        m.beam_search(mel, good, 4, 9)
    with pytest.raises(ValueError, match="temperature"):
        m.sample(mel, good, 4, temperature=-1.0)


def test_op_value_errors():
    from mop_amd import ops
    q, k = torch.zeros(2, 1, 2, 16), torch.zeros(2, 8, 2, 16)
    with pytest.raises(ValueError, match="kv_start"):
        ops.decode_attention_ragged(q, k, k, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="kv_start"):
        ops.decode_attention_ragged(q, k, k, torch.zeros(2))
    with pytest.raises(ValueError, match="rows"):
        ops.decode_attention_ragged(q, k, k, torch.zeros(2, dtype=torch.int32), rows=torch.zeros(2, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="pos_off"):
        ops.sample_tokens_ragged_torch(torch.zeros(3, 10), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))


def naive_ragged_attention(q, k, v, kv_start, rows, L, causal):
    """float64 loop: query i of row b over the keys kv_start[b] <= j < L (causal: < L - Tq + i + 1), key j from cache row rows[b, j]"""
    B, Tq, H, dk = q.shape
    y = torch.zeros(B, Tq, H, dk, dtype=torch.float64)
    for b in range(B):
        for i in range(Tq):
            lim = L - Tq + i + 1 if causal else L
            js = list(range(max(int(kv_start[b]), 0), lim))
            if not js:
                continue
            src = [int(rows[b, j]) if rows is not None else b for j in js]
            kk = torch.stack([k[s, j] for s, j in zip(src, js)]).double()          # (n, H, dk)
            vv = torch.stack([v[s, j] for s, j in zip(src, js)]).double()
            s = torch.einsum("hd,nhd->hn", q[b, i].double(), kk) / math.sqrt(dk)
            y[b, i] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), vv)
    return y.reshape(B, Tq, H * dk)


@pytest.mark.parametrize("Tq", [1, 5, 16])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("with_rows", [False, True])
def test_torch_composition_against_a_float64_loop(Tq, causal, with_rows):
    from mop_amd import ops
    torch.manual_seed(Tq + 2 * causal)
    B, H, dk, cap, L = 4, 2, 16, 300, 260
    q = torch.randn(B, Tq, H, dk)
    k, v = torch.randn(B, cap, H, dk), torch.randn(B, cap, H, dk)
    kv_start = torch.tensor([0, 37, 128, L], dtype=torch.int32)             # none, inside a chunk, on a chunk edge, everything
    rows = torch.randint(0, B, (B, cap + 3), dtype=torch.int32) if with_rows else None
    kv_len = torch.tensor([L], dtype=torch.int32)
    got = ops.decode_attention_ragged_torch(q, k, v, kv_start, rows, kv_len=kv_len, causal=causal)
    ref = naive_ragged_attention(q, k, v, kv_start, rows, L, causal)
    assert (got.double() - ref).abs().max() < 1e-5
    assert torch.equal(got[3], torch.zeros_like(got[3]))                     # kv_start = L: no key, exactly 0
    with torch.no_grad():
        g64 = ops.decode_attention_ragged_torch(q.double(), k.double(), v.double(), kv_start, rows, nk=L, causal=causal)
    assert (g64 - ref).abs().max() < 1e-12
    zero = torch.zeros(B, dtype=torch.int32)                                 # kv_start = 0 is the plain / row-table composition
    plain = (ops.decode_attention_rows_torch(q, k, v, rows, kv_len, causal) if with_rows
             else ops.decode_attention_torch(q, k, v, kv_len, None, causal))
    assert (ops.decode_attention_ragged_torch(q, k, v, zero, rows, kv_len=kv_len, causal=causal) - plain).abs().max() < 1e-6


def test_sample_ragged_torch_offsets_the_position():
    from mop_amd import ops
    torch.manual_seed(3)
    x = torch.randn(6, 50)
    pos = torch.tensor([20], dtype=torch.int32)
    off = torch.tensor([0, 3, 7, 0, 19, 2], dtype=torch.int32)
    kw = dict(temperature=0.9, top_k=20, top_p=0.9, seed=5)
    tok, lp = ops.sample_tokens_ragged_torch(x, pos, off, **kw)
    for r in range(6):
        t1, l1 = ops.sample_tokens_torch(x, pos - off[r], **kw)
        assert int(tok[r]) == int(t1[r]) and float(lp[r]) == float(l1[r]), r
    t0, l0 = ops.sample_tokens_ragged_torch(x, pos, torch.zeros(6, dtype=torch.int32), **kw)
    ts, ls = ops.sample_tokens_torch(x, pos, **kw)
    assert torch.equal(t0, ts) and torch.equal(l0, ls)


LENS = [1, 5, 20, 3]                                   # the short path (<= 16 tokens) and the masked > 16 prefill


def _ragged_inputs(seed=11):
    torch.manual_seed(seed)
    mel = torch.randn(len(LENS), 40, 10)
    prompts = [torch.randint(0, 100, (n,)) for n in LENS]
    return mel, prompts


@pytest.mark.parametrize("pos", [True, False])
def test_ragged_generate_equals_each_prompt_alone(torch_cores, pos):
    m = _tiny_model(use_abs_pos_emb=pos)
    mel, prompts = _ragged_inputs()
    out, steps = m.generate(mel, prompts, 12, return_logits=True)
    assert isinstance(out, list) and len(out) == 4 and steps.shape == (4, 12, 100)
    for b, p in enumerate(prompts):
        ref, rs = m.generate(mel[b:b + 1], p.unsqueeze(0), 12, return_logits=True)
        assert torch.equal(out[b], ref[0]), b
        assert out[b].dtype == p.dtype and out[b].shape == (LENS[b] + 12,)
        assert (steps[b] - rs[0]).abs().max() < 1e-4, b
    eos = int(out[2][20 + 3])
    got = m.generate(mel, prompts, 12, eos_token_id=eos)
    for b in range(4):
        hit = (out[b][LENS[b]:] == eos).nonzero()
        f = LENS[b] + int(hit[0]) if len(hit) else LENS[b] + 12
        assert torch.equal(got[b][:f + 1], out[b][:f + 1]) and (got[b][f:] == eos).all(), b


def test_ragged_beam_search_equals_the_uniform_batch_of_each_prompt(torch_cores):
    m = _tiny_model()
    mel, prompts = _ragged_inputs()
    tok, sc = m.beam_search(mel, prompts, 10, 3, eos_token_id=5)
    assert isinstance(tok, list) and sc.shape == (4,)
    for b, p in enumerate(prompts):
        rt, rsc = m.beam_search(mel, p.unsqueeze(0).repeat(4, 1), 10, 3, eos_token_id=5)
        assert torch.equal(tok[b], rt[b]), b
        assert abs(float(sc[b]) - float(rsc[b])) < 1e-4, b


@pytest.mark.parametrize("n", [1, 3])
def test_ragged_sample_equals_the_uniform_batch_of_each_prompt(torch_cores, n):
    m = _tiny_model()
    mel, prompts = _ragged_inputs()
    cfg = dict(temperature=0.8, top_k=20, top_p=0.9, num_samples=n, seed=7, eos_token_id=9)
    tok, lp = m.sample(mel, prompts, 10, **cfg)
    assert isinstance(tok, list) and lp.shape == (4, n)
    for b, p in enumerate(prompts):
        rt, rlp = m.sample(mel, p.unsqueeze(0).repeat(4, 1), 10, **cfg)
        assert tok[b].shape == (n, LENS[b] + 10)
        assert torch.equal(tok[b], rt[b]), b
        assert (lp[b] - rlp[b]).abs().max() < 1e-4, b


def test_equal_length_list_equals_the_tensor_call(torch_cores):
    m = _tiny_model()
    torch.manual_seed(2)
    mel, prompt = torch.randn(3, 40, 10), torch.randint(0, 100, (3, 4))
    lst = list(prompt)
    out, steps = m.generate(mel, lst, 8, return_logits=True)
    ref, rsteps = m.generate(mel, prompt, 8, return_logits=True)
    assert isinstance(out, list) and torch.equal(torch.stack(out), ref) and torch.equal(steps, rsteps)
    tok, sc = m.beam_search(mel, lst, 8, 2)
    rt, rsc = m.beam_search(mel, prompt, 8, 2)
    assert torch.equal(torch.stack(tok), rt) and torch.equal(sc, rsc)
    tok, lp = m.sample(mel, lst, 8, num_samples=2, seed=3)
    rt, rlp = m.sample(mel, prompt, 8, num_samples=2, seed=3)
    assert torch.equal(torch.stack(tok), rt) and torch.equal(lp, rlp)


def test_decode_step_on_a_ragged_cache_matches_each_row_alone(torch_cores):
    """driving init_decode_cache / decode_step directly with cache.kv_start"""
    m = _tiny_model()
    torch.manual_seed(4)
    enc = torch.randn(2, 40, 32)
    a, b = torch.randint(0, 100, (7,)), torch.randint(0, 100, (3,))
    cache = m.init_decode_cache(enc, 12)
    cache.kv_start = torch.tensor([0, 4], dtype=torch.int32)
    ids = torch.stack([a, F.pad(b, (4, 0))])
    lg = m.decode_step(cache, ids)
    nxt = torch.randint(0, 100, (2, 1))
    lg2 = m.decode_step(cache, nxt)
    for r, p in enumerate((a, b)):
        full = m.decode(enc[r:r + 1], torch.cat([p, nxt[r]]).unsqueeze(0))
        assert (lg[r, 7 - len(p):] - full[0, :-1]).abs().max() < 1e-5, r
        assert (lg2[r, 0] - full[0, -1]).abs().max() < 1e-5, r
