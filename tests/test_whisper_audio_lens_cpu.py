"""CPU checks of per-row audio lengths in WhisperMoP (clips of different lengths in one batch, no GPU):
the support / size queries and bad-argument returns of mopk_sdpa_lens_* and
mopk_decode_attn_lens_* (no launch), signatures of the new ops, the ValueErrors raised before any device work,
ops.decode_attention_lens_torch and a torch restatement of the length semantics against float64 loops, and the module logic with
every core routed through its torch composition: forward / generate / beam_search / sample on a list of clips, row b against the
same call on clip b alone (or on a uniform batch of clip b), with ragged prompts too, and a float64 gradient check."""
import ctypes as C
import inspect
import math

import pytest
import torch

from test_whisper_beam_cpu import _params, _tiny_model

NEG = float("-inf")
BAD_SHAPE, BAD_ARG, UNSUPPORTED = -1, -2, -3             # MopkStatus
LENS = [40, 25, 1, 13]


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def sdpa_lens_torch(q, k, v, attn_mask=None, bias=None, causal=False, q_lens=None, kv_lens=None):
    """torch restatement of sdpa_core's length semantics: query i < q_lens[b] attends to keys j < kv_lens[b]; padding query rows
    are 0; what padding rows hold is never used (they are zeroed before any product)"""
    B, N, H, dk = q.shape
    Nk = k.shape[1]
    if q_lens is not None:
        qin = torch.arange(N).view(1, N) < q_lens.view(B, 1).long()
        q = q.masked_fill(~qin.view(B, N, 1, 1), 0.0)
    if kv_lens is not None:
        kin = torch.arange(Nk).view(1, Nk) < kv_lens.view(B, 1).long()
        k, v = k.masked_fill(~kin.view(B, Nk, 1, 1), 0.0), v.masked_fill(~kin.view(B, Nk, 1, 1), 0.0)
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    s = qt @ kt.transpose(-1, -2) * dk ** -0.5
    if bias is not None:
        s = s + bias
    if attn_mask is not None:
        s = s.masked_fill(attn_mask == 0, NEG)
    if causal:
        s = s.masked_fill(torch.ones(N, N, dtype=torch.bool).triu(1), NEG)
    if kv_lens is not None:
        s = s.masked_fill(~kin.view(B, 1, 1, Nk), NEG)
    if q_lens is not None:
        s = s.masked_fill(~qin.view(B, 1, N, 1), NEG)
    y = torch.softmax(s, -1).nan_to_num(0.0) @ vt                           # a row with no open key is 0, as the cores
    return y.transpose(1, 2).reshape(B, N, -1)


@pytest.fixture
def torch_cores(monkeypatch):
    """route every core through its torch composition, q_lens / kv_lens included, so the module logic runs on the CPU"""
    from mop_amd import ops

    def sdpa(q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p=0.0, seed=None, q_lens=None, kv_lens=None):
        return sdpa_lens_torch(q, k, v, attn_mask, bias, causal, q_lens, kv_lens)

    monkeypatch.setattr(ops, "sdpa_core", sdpa)
    monkeypatch.setattr(ops, "decode_attention", lambda q, k, v, kv_len=None, nk=None, causal=False:
                        ops.decode_attention_torch(q, k, v, kv_len, nk, causal))
    monkeypatch.setattr(ops, "decode_attention_rows", ops.decode_attention_rows_torch)
    monkeypatch.setattr(ops, "decode_attention_ragged", ops.decode_attention_ragged_torch)
    monkeypatch.setattr(ops, "decode_attention_lens", ops.decode_attention_lens_torch)
    monkeypatch.setattr(ops, "beam_step", ops.beam_step_torch)
    monkeypatch.setattr(ops, "sample_tokens", ops.sample_tokens_torch)
    monkeypatch.setattr(ops, "sample_tokens_ragged", ops.sample_tokens_ragged_torch)


# ------------------------------------------------------------------ ABI
def _sl(B=2, H=4, N=130, Nk=300, dk=64, bf16=True, prec_bf16=True, causal=0):
    from mop_amd import _lib
    a = _lib.SdpaLensArgs()
    b = a.base
    b.B, b.H, b.N, b.dk, b.Nk, b.causal = B, H, N, dk, Nk, causal
    b.io_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    b.precision, b.path = (_lib.PREC_BF16 if prec_bf16 else _lib.PREC_FP32), _lib.PATH_AUTO
    for v, n in ((b.q, N), (b.y, N), (b.k, Nk or N), (b.v, Nk or N)):
        v.ptr, v.sb, v.sn, v.sh = 4096, n * H * dk, H * dk, dk       # aligned stand-ins: the queries never dereference them
    a.q_lens, a.kv_lens = 256, 512
    return a


def test_sdpa_lens_queries_and_bad_arguments(lib):
    a = _sl()
    assert lib.mopk_sdpa_lens_supported(C.byref(a)) == 1 == lib.mopk_sdpa_fused_supported(C.byref(a.base))
    assert lib.mopk_sdpa_lens_saved_bytes(C.byref(a)) == lib.mopk_sdpa_saved_bytes(C.byref(a.base)) > 0
    assert lib.mopk_sdpa_lens_workspace_bytes(C.byref(a)) == lib.mopk_sdpa_workspace_bytes(C.byref(a.base)) > 0
    a.q_lens = a.kv_lens = None                                # both NULL: the full lengths
    assert lib.mopk_sdpa_lens_supported(C.byref(a)) == 1
    for kw in (dict(prec_bf16=False), dict(dk=48), dict(bf16=False, prec_bf16=False)):     # generic path: same sizes as the base
        a = _sl(**kw)
        assert lib.mopk_sdpa_lens_supported(C.byref(a)) == 0 == lib.mopk_sdpa_fused_supported(C.byref(a.base))
        assert lib.mopk_sdpa_lens_saved_bytes(C.byref(a)) == lib.mopk_sdpa_saved_bytes(C.byref(a.base)) > 0
        assert lib.mopk_sdpa_lens_workspace_bytes(C.byref(a)) == lib.mopk_sdpa_workspace_bytes(C.byref(a.base)) > 0
    for field, val, rc in [("q_lens", 258, UNSUPPORTED), ("kv_lens", 513, UNSUPPORTED)]:
        a = _sl()
        setattr(a, field, val)
        assert lib.mopk_sdpa_lens_supported(C.byref(a)) == 0, field
        assert lib.mopk_sdpa_lens_saved_bytes(C.byref(a)) == 0 == lib.mopk_sdpa_lens_workspace_bytes(C.byref(a)), field
        assert lib.mopk_sdpa_lens_fwd(C.byref(a), None) == rc == lib.mopk_sdpa_lens_bwd(C.byref(a), None), field
    for field, val, rc in [("mask", 4096, BAD_ARG), ("bias", 4096, BAD_ARG), ("B", 0, BAD_SHAPE), ("Nk", -1, BAD_SHAPE),
                           ("io_dtype", 7, BAD_ARG)]:
        a = _sl()
        setattr(a.base, field, val)
        assert lib.mopk_sdpa_lens_supported(C.byref(a)) == 0, field
        assert lib.mopk_sdpa_lens_fwd(C.byref(a), None) == rc == lib.mopk_sdpa_lens_bwd(C.byref(a), None), field
    a = _sl(causal=1)                                          # causal is square only
    assert lib.mopk_sdpa_lens_fwd(C.byref(a), None) == UNSUPPORTED
    assert lib.mopk_sdpa_lens_fwd(None, None) == BAD_ARG == lib.mopk_sdpa_lens_bwd(None, None)
    a = _sl()                                                  # null saved / workspace (and dy, dq, ..): refused, nothing launched
    assert lib.mopk_sdpa_lens_fwd(C.byref(a), None) == BAD_ARG == lib.mopk_sdpa_lens_bwd(C.byref(a), None)
    a.base.saved = a.base.workspace = 4096
    a.base.dropout_p = 1.0
    assert lib.mopk_sdpa_lens_fwd(C.byref(a), None) == BAD_ARG


def _dl(B=2, H=4, Tq=1, dk=64, cap=1500, bf16=True):
    from mop_amd import _lib
    a = _lib.DecodeAttnLensArgs()
    b = a.base
    b.B, b.H, b.Tq, b.dk, b.cap, b.Nk, b.causal = B, H, Tq, dk, cap, cap, 0
    b.io_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    for v in (b.q, b.k, b.v, b.y):
        v.sb, v.sn, v.sh = cap * H * dk, H * dk, dk
    a.kv_lens = 256                                        # an aligned stand-in: the queries never dereference it
    return a


def test_decode_attn_lens_queries_and_bad_arguments(lib):
    a = _dl()
    assert lib.mopk_decode_attn_lens_supported(C.byref(a)) == 1
    assert lib.mopk_decode_attn_lens_workspace_bytes(C.byref(a)) == lib.mopk_decode_attn_workspace_bytes(C.byref(a.base)) > 0
    for field, val, rc in [("kv_lens", None, BAD_ARG), ("kv_lens", 258, UNSUPPORTED)]:
        a = _dl()
        setattr(a, field, val)
        assert lib.mopk_decode_attn_lens_supported(C.byref(a)) == 0, field
        assert lib.mopk_decode_attn_lens_workspace_bytes(C.byref(a)) == 0, field
        assert lib.mopk_decode_attn_lens_fwd(C.byref(a), None) == rc, field
    for field, val, rc in [("Tq", 17, UNSUPPORTED), ("dk", 96, UNSUPPORTED), ("causal", 1, BAD_ARG), ("kv_len", 512, BAD_ARG),
                           ("B", 0, BAD_SHAPE), ("Nk", 0, BAD_SHAPE)]:
        a = _dl()
        setattr(a.base, field, val)
        assert lib.mopk_decode_attn_lens_supported(C.byref(a)) == 0, field
        assert lib.mopk_decode_attn_lens_fwd(C.byref(a), None) == rc, field
    assert lib.mopk_decode_attn_lens_fwd(None, None) == BAD_ARG
    a = _dl()                                              # null q / k / v / y / workspace: refused, nothing launched
    assert lib.mopk_decode_attn_lens_fwd(C.byref(a), None) == BAD_ARG


# ------------------------------------------------------------------ signatures and argument errors
def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import EncodedAudio, WhisperMoP
    from mop_amd.nn.whisper_mop import WhisperDecodeCache
    e, P = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert list(inspect.signature(ops.sdpa_core).parameters) == ["q", "k", "v", "attn_mask", "bias", "causal", "dropout_p", "seed",
                                                                 "q_lens", "kv_lens"]
    sig = inspect.signature(ops.sdpa_core).parameters
    assert sig["q_lens"].default is None and sig["kv_lens"].default is None
    dl = dict(q=(e, P), k_cache=(e, P), v_cache=(e, P), kv_lens=(e, P), nk=(None, P))
    for f in (ops.decode_attention_lens, ops.decode_attention_lens_torch, ops.decode_attention_lens_supported):
        assert _params(f) == dl, f.__name__
    assert EncodedAudio._fields == ("out", "lens")
    assert list(inspect.signature(WhisperMoP.encode).parameters) == ["self", "mel"]
    c = WhisperDecodeCache([], [], [torch.zeros(1)], [], torch.zeros(1, dtype=torch.int32), 4)
    assert c.audio_lens is None and c.kv_start is None


def test_model_value_errors_before_device_work(torch_cores):
    m = _tiny_model()
    ids = torch.zeros(2, 4, dtype=torch.long)
    good = [torch.randn(40, 10), torch.randn(7, 10)]
    bad = [([], "non-empty list"), ([torch.randn(2, 5, 10), torch.randn(5, 10)], "2-D"), ([torch.randn(5, 10), [1.0]], "2-D"),
           ([torch.randn(5, 10), torch.randn(5, 9)], "mel bins"), ([torch.randn(5, 10), torch.randn(0, 10)], "frames"),
           ([torch.randn(5, 10), torch.randn(41, 10)], "n_audio_ctx"), ([torch.randn(5, 10), torch.randn(5, 10).double()], "dtype"),
           ([torch.zeros(5, 10, dtype=torch.long)] * 2, "dtype"), ([torch.randn(5, 10), torch.randn(5, 10, device="meta")], "is on")]
    for mel, msg in bad:
        for call in (lambda x: m.encode(x), lambda x: m.get_gate_maps(x), lambda x: m(x, ids), lambda x: m.generate(x, ids, 4),
                     lambda x: m.beam_search(x, ids, 4, 2), lambda x: m.sample(x, ids, 4)):
            with pytest.raises(ValueError, match=msg):
                call(mel)
    three = torch.zeros(3, 4, dtype=torch.long)                           # B of the prompts does not match the clips
    for call in (lambda: m(good, three), lambda: m.generate(good, three, 4), lambda: m.beam_search(good, three, 4, 2),
                 lambda: m.sample(good, three, 4), lambda: m.generate(good, [three[0]], 4)):
        with pytest.raises(ValueError, match="2 mel inputs"):
            call()
    with pytest.raises(ValueError, match="n_text_ctx"):
        m.generate(good, ids, 61)


def test_op_value_errors():
    from mop_amd import ops
    q, k = torch.zeros(2, 1, 2, 16), torch.zeros(2, 8, 2, 16)
    i32 = torch.zeros(2, dtype=torch.int32)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 1, dtype=torch.int32),
                [1, 2]):
        with pytest.raises(ValueError, match="kv_lens"):
            ops.sdpa_core(q, k, k, kv_lens=bad)
        with pytest.raises(ValueError, match="q_lens"):
            ops.sdpa_core(q, k, k, q_lens=bad, kv_lens=i32)
    with pytest.raises(ValueError, match="is on"):
        ops.sdpa_core(q, k, k, kv_lens=torch.zeros(2, dtype=torch.int32, device="meta"))
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2), torch.zeros(2, 1, dtype=torch.int32), [1, 2]):
        with pytest.raises(ValueError, match="kv_lens"):
            ops.decode_attention_lens(q, k, k, bad)
    with pytest.raises(ValueError, match="nk"):
        ops.decode_attention_lens(q, k, k, i32, nk=9)
    with pytest.raises(ValueError, match="k_cache"):
        ops.decode_attention_lens(q, k[:1], k[:1], i32)


# ------------------------------------------------------------------ torch compositions against float64 loops
def naive_lens_attention(q, k, v, q_lens, kv_lens, causal=False):
    """float64 loop: query i < q_lens[b] over the keys j < kv_lens[b] (and j <= i with causal); every other row of y is 0.  Lengths
    are clamped into [0, N] / [0, Nk]; None = full."""
    B, N, H, dk = q.shape
    Nk = k.shape[1]
    y = torch.zeros(B, N, H, dk, dtype=torch.float64)
    for b in range(B):
        nq = N if q_lens is None else min(max(int(q_lens[b]), 0), N)
        nk = Nk if kv_lens is None else min(max(int(kv_lens[b]), 0), Nk)
        for i in range(nq):
            lim = min(nk, i + 1) if causal else nk
            if lim == 0:
                continue
            s = torch.einsum("hd,nhd->hn", q[b, i].double(), k[b, :lim].double()) / math.sqrt(dk)
            y[b, i] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), v[b, :lim].double())
    return y.reshape(B, N, H * dk)


@pytest.mark.parametrize("Tq", [1, 5, 16])
def test_decode_attention_lens_torch_against_a_float64_loop(Tq):
    from mop_amd import ops
    torch.manual_seed(Tq)
    B, H, dk, cap, nk = 5, 2, 16, 300, 260
    q = torch.randn(B, Tq, H, dk)
    k, v = torch.randn(B, cap, H, dk), torch.randn(B, cap, H, dk)
    lens = torch.tensor([0, 37, 128, nk, 400], dtype=torch.int32)
    got = ops.decode_attention_lens_torch(q, k, v, lens, nk=nk)
    ref = naive_lens_attention(q, k[:, :nk], v[:, :nk], None, lens)
    assert (got.double() - ref).abs().max() < 1e-5
    assert torch.equal(got[0], torch.zeros_like(got[0]))                      # no key: exactly 0
    g64 = ops.decode_attention_lens_torch(q.double(), k.double(), v.double(), lens, nk=nk)
    assert (g64 - ref).abs().max() < 1e-12
    kn, vn = k.clone(), v.clone()
    for b in range(B):                                                        # nothing beyond a length is used
        kn[b, min(int(lens[b]), nk):] = float("nan")
        vn[b, min(int(lens[b]), nk):] = float("inf")
    assert torch.equal(ops.decode_attention_lens_torch(q, kn, vn, lens, nk=nk), got)
    full = torch.full((B,), nk, dtype=torch.int32)
    assert (ops.decode_attention_lens_torch(q, k, v, full, nk=nk) - ops.decode_attention_torch(q, k, v, None, nk, False)).abs().max() < 1e-6


@pytest.mark.parametrize("causal", [False, True])
def test_length_semantics_in_torch_against_a_float64_loop(causal):
    from mop_amd import ops
    torch.manual_seed(3 + causal)
    B, N, H, dk = 5, 70, 2, 16
    Nk = N if causal else 90
    q, k, v = torch.randn(B, N, H, dk), torch.randn(B, Nk, H, dk), torch.randn(B, Nk, H, dk)
    ql = torch.tensor([0, 1, 33, 64, N + 9], dtype=torch.int32)
    kl = ql if causal else torch.tensor([Nk, 0, 64, 17, -3], dtype=torch.int32)
    got = sdpa_lens_torch(q.double(), k.double(), v.double(), causal=causal, q_lens=ql, kv_lens=kl)
    ref = naive_lens_attention(q, k, v, ql, kl, causal)
    assert (got - ref).abs().max() < 1e-12
    # the host-side fold of sdpa_core (lengths + attn_mask / bias -> one mask) states the same thing
    m = ops.sdpa_lens_mask(ql, kl, B, N, Nk, q.device)
    assert m.shape == (B, 1, N, Nk) and m.dtype == torch.bool
    folded = sdpa_lens_torch(q.double(), k.double(), v.double(), attn_mask=m, causal=causal)
    assert (folded - ref).abs().max() < 1e-12
    assert ops.sdpa_lens_mask(None, kl, B, N, Nk, q.device).shape == (B, 1, 1, Nk)


# ------------------------------------------------------------------ module logic on the torch cores
def _clips(seed=11, n_mels=10):
    torch.manual_seed(seed)
    return [torch.randn(n, n_mels) for n in LENS]


@pytest.mark.parametrize("pos", [True, False])
def test_forward_equals_each_clip_alone(torch_cores, pos):
    from mop_amd.nn import EncodedAudio
    m = _tiny_model(use_abs_pos_emb=pos).double()
    clips = [c.double() for c in _clips()]
    ids = torch.randint(0, 100, (4, 9))
    logits, loss, gates = m(clips, ids)
    assert loss is None and logits.shape == (4, 9, 100) and gates.shape == (4, 1, 40)
    enc, g2 = m.encode(clips)
    assert isinstance(enc, EncodedAudio) and enc.out.shape == (4, 40, 32) and enc.lens.dtype == torch.int32
    assert enc.lens.tolist() == LENS and torch.equal(g2, gates) and torch.equal(m.get_gate_maps(clips), gates)
    assert torch.equal(m.decode(enc, ids), logits)
    for b, c in enumerate(clips):
        rl, _, rg = m(c.unsqueeze(0), ids[b:b + 1])
        assert (logits[b] - rl[0]).abs().max() < 1e-12, b
        assert (gates[b, :, :LENS[b]] - rg[0]).abs().max() < 1e-12, b
        e1, _ = m.encode(c.unsqueeze(0))
        assert (enc.out[b, :LENS[b]] - e1[0]).abs().max() < 1e-12, b
    # nothing in the padding is read by the decoder: garbage there changes nothing
    out = enc.out.clone()
    for b in range(4):
        out[b, LENS[b]:] = float("nan")
    assert torch.equal(m.decode(EncodedAudio(out, enc.lens), ids), logits)


def test_equal_length_list_equals_the_tensor_call(torch_cores):
    from mop_amd.nn import EncodedAudio
    m = _tiny_model()
    torch.manual_seed(2)
    mel, prompt = torch.randn(3, 33, 10), torch.randint(0, 100, (3, 4))
    lst = list(mel)
    enc, g = m.encode(lst)
    re, rg = m.encode(mel)
    assert isinstance(enc, EncodedAudio) and enc.lens is None and torch.equal(enc.out, re) and torch.equal(g, rg)
    assert torch.equal(m(lst, prompt)[0], m(mel, prompt)[0])
    assert torch.equal(m.generate(lst, prompt, 8), m.generate(mel, prompt, 8))
    tok, sc = m.beam_search(tuple(lst), prompt, 8, 2)
    rt, rsc = m.beam_search(mel, prompt, 8, 2)
    assert torch.equal(tok, rt) and torch.equal(sc, rsc)
    tok, lp = m.sample(lst, prompt, 8, num_samples=2, seed=3)
    rt, rlp = m.sample(mel, prompt, 8, num_samples=2, seed=3)
    assert torch.equal(tok, rt) and torch.equal(lp, rlp)


@pytest.mark.parametrize("T_p", [4, 20])                 # the short path (<= 16 tokens) and the > 16 prefill with kv_lens
def test_generate_equals_each_clip_alone(torch_cores, T_p):
    m = _tiny_model()
    clips = _clips()
    prompt = torch.randint(0, 100, (4, T_p))
    out, steps = m.generate(clips, prompt, 12, return_logits=True)
    assert out.shape == (4, T_p + 12) and steps.shape == (4, 12, 100)
    for b, c in enumerate(clips):
        ref, rs = m.generate(c.unsqueeze(0), prompt[b:b + 1], 12, return_logits=True)
        assert torch.equal(out[b], ref[0]), b
        assert (steps[b] - rs[0]).abs().max() < 1e-4, b
    eos = int(out[1, T_p + 3])
    got = m.generate(clips, prompt, 12, eos_token_id=eos)
    for b in range(4):
        hit = (out[b, T_p:] == eos).nonzero()
        f = T_p + int(hit[0]) if len(hit) else T_p + 12
        assert torch.equal(got[b, :f + 1], out[b, :f + 1]) and (got[b, f:] == eos).all(), b


def test_generate_with_ragged_prompts_too(torch_cores):
    m = _tiny_model()
    clips = _clips()
    torch.manual_seed(5)
    prompts = [torch.randint(0, 100, (n,)) for n in (1, 5, 20, 3)]
    out, steps = m.generate(clips, prompts, 10, return_logits=True)
    assert isinstance(out, list)
    for b, (c, p) in enumerate(zip(clips, prompts)):
        ref, rs = m.generate(c.unsqueeze(0), p.unsqueeze(0), 10, return_logits=True)
        assert torch.equal(out[b], ref[0]), b
        assert (steps[b] - rs[0]).abs().max() < 1e-4, b


def test_decode_step_on_a_cache_with_audio_lens(torch_cores):
    from mop_amd.nn import EncodedAudio
    m = _tiny_model()
    enc, _ = m.encode(_clips())
    cache = m.init_decode_cache(enc, 12)
    assert cache.audio_lens is enc.lens
    ids = torch.randint(0, 100, (4, 7))
    lg = m.decode_step(cache, ids[:, :6])
    lg2 = m.decode_step(cache, ids[:, 6:])
    full = m.decode(enc, ids)
    assert (lg - full[:, :6]).abs().max() < 1e-5 and (lg2[:, 0] - full[:, 6]).abs().max() < 1e-5
    plain = m.init_decode_cache(enc.out, 12)                                # a plain tensor: the uniform cache, as before
    assert plain.audio_lens is None


def test_beam_search_equals_the_uniform_batch_of_each_clip(torch_cores):
    m = _tiny_model()
    clips = _clips()
    torch.manual_seed(6)
    prompt = torch.randint(0, 100, (4, 3))
    tok, sc = m.beam_search(clips, prompt, 10, 3, eos_token_id=5)
    assert tok.shape == (4, 13) and sc.shape == (4,)
    for b, c in enumerate(clips):
        rt, rsc = m.beam_search(c.unsqueeze(0).repeat(4, 1, 1), prompt, 10, 3, eos_token_id=5)
        assert torch.equal(tok[b], rt[b]), b
        assert abs(float(sc[b]) - float(rsc[b])) < 1e-4, b
    prompts = [torch.randint(0, 100, (n,)) for n in (2, 18, 1, 6)]          # with ragged prompts at the same time
    tok, sc = m.beam_search(clips, prompts, 8, 2)
    for b, (c, p) in enumerate(zip(clips, prompts)):
        rt, rsc = m.beam_search(c.unsqueeze(0), p.unsqueeze(0), 8, 2)
        assert torch.equal(tok[b], rt[0]) and abs(float(sc[b]) - float(rsc[0])) < 1e-4, b


@pytest.mark.parametrize("n", [1, 3])
def test_sample_equals_the_uniform_batch_of_each_clip(torch_cores, n):
    m = _tiny_model()
    clips = _clips()
    torch.manual_seed(7)
    prompt = torch.randint(0, 100, (4, 3))
    cfg = dict(temperature=0.8, top_k=20, top_p=0.9, num_samples=n, seed=7, eos_token_id=9)
    tok, lp = m.sample(clips, prompt, 10, **cfg)
    assert tok.shape == (4, n, 13) and lp.shape == (4, n)
    for b, c in enumerate(clips):
        rt, rlp = m.sample(c.unsqueeze(0).repeat(4, 1, 1), prompt, 10, **cfg)
        assert torch.equal(tok[b], rt[b]), b
        assert (lp[b] - rlp[b]).abs().max() < 1e-4, b


def test_parameter_gradients_are_the_weighted_sum_over_rows_alone(torch_cores):
    """float64: the batch loss is the mean over the non-ignored targets of all rows, so its parameter gradients are the sum of each
    row's own gradients weighted by its share of those targets"""
    m = _tiny_model().double()
    clips = [c.double() for c in _clips()]
    torch.manual_seed(9)
    ids = torch.randint(0, 100, (4, 9))
    tg = torch.randint(0, 100, (4, 9))
    tg[0, 6:] = -100
    tg[2, 2:] = -100
    tg[3, :] = -100                                                          # a row with no target at all
    _, loss, _ = m(clips, ids, tg)
    grads = torch.autograd.grad(loss, list(m.parameters()), allow_unused=True)
    n_all = int((tg != -100).sum())
    want = [torch.zeros_like(p) for p in m.parameters()]
    total = 0.0
    for b, c in enumerate(clips):
        n_b = int((tg[b] != -100).sum())
        if n_b == 0:
            continue
        _, lb, _ = m(c.unsqueeze(0), ids[b:b + 1], tg[b:b + 1])
        total = total + float(lb.detach()) * n_b / n_all
        for w, g in zip(want, torch.autograd.grad(lb, list(m.parameters()), allow_unused=True)):
            if g is not None:
                w += g * n_b / n_all
    assert abs(float(loss.detach()) - total) < 1e-12
    for (name, _), g, w in zip(m.named_parameters(), grads, want):
        g = torch.zeros_like(w) if g is None else g
        assert (g - w).abs().max() <= 1e-10 * max(1.0, float(w.abs().max())), name
