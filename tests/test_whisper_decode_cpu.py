"""CPU checks of KV-cached WhisperMoP decoding (no GPU): signatures and defaults of init_decode_cache / decode_step / generate,
the support query and bad-argument returns of mopk_decode_attn_*, the ValueErrors raised before any
device work, the torch composition of ops.decode_attention against float64 loops, the decode_step bookkeeping (positions, append,
bottom-right causal alignment, the long-prompt prefill) with the attention cores routed through torch, and the whgen_* fixtures."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden_names, load_golden

WHGEN = golden_names("whgen_")


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _params(f):
    return {k: (v.default, v.kind) for k, v in inspect.signature(f).parameters.items() if k != "self"}


def test_signatures():
    from mop_amd.nn import WhisperMoP
    from mop_amd.nn.whisper_mop import WhisperDecodeCache  # noqa: F401
    from mop_amd import ops
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert _params(WhisperMoP.init_decode_cache) == dict(enc_out=(e, P), max_len=(e, P))
    assert _params(WhisperMoP.decode_step) == dict(cache=(e, P), ids=(e, P))
    assert _params(WhisperMoP.generate) == dict(mel=(e, P), prompt_ids=(e, P), max_new_tokens=(e, P), eos_token_id=(None, P),
                                                graph=(False, P), return_logits=(False, K))
    assert _params(ops.decode_attention) == dict(q=(e, P), k_cache=(e, P), v_cache=(e, P), kv_len=(None, P), nk=(None, P),
                                                 causal=(False, P))


def _args(B=2, H=8, Tq=1, dk=64, cap=448, Nk=448, bf16=True, causal=0):
    from mop_amd import _lib
    a = _lib.DecodeAttnArgs()
    a.B, a.H, a.Tq, a.dk, a.cap, a.Nk, a.causal = B, H, Tq, dk, cap, Nk, causal
    a.io_dtype = _lib.MOPK_BF16 if bf16 else _lib.MOPK_F32
    for t in (a.k, a.v):                       # a contiguous (B, cap, H, dk) cache
        t.sb, t.sh, t.sn = cap * H * dk, dk, H * dk
    return a


def test_support_query_needs_no_gpu(lib):
    ok = lambda a: lib.mopk_decode_attn_supported(C.byref(a))
    for dk in (32, 64, 128):
        for bf16 in (True, False):
            for tq in (1, 2, 4, 5, 16):
                assert ok(_args(Tq=tq, dk=dk, bf16=bf16, causal=1)) == 1, (tq, dk, bf16)
    assert ok(_args(Tq=0)) == 0 and ok(_args(Tq=17)) == 0
    assert ok(_args(dk=48)) == 0 and ok(_args(dk=256)) == 0 and ok(_args(dk=16)) == 0
    assert ok(_args(cap=100, Nk=101)) == 0
    assert ok(_args(Nk=0)) == 0                          # no kv_len and no Nk
    a = _args()
    a.k.sn = 64 * 8 + 4                                  # a row stride that is not whole 16-byte vectors
    assert ok(a) == 0
    a = _args(bf16=False)
    a.k.sn = 64 * 8 + 4                                  # fp32: 4 elements are a whole vector
    assert ok(a) == 1
    a = _args()
    a.io_dtype = 2
    assert ok(a) == 0
    ws = lambda a: lib.mopk_decode_attn_workspace_bytes(C.byref(a))
    # 1500 keys in 128-key chunks: 12 partials of (m, l, acc[dk]) per (b, h) row and query
    assert ws(_args(B=8, H=8, cap=1500, Nk=1500)) == 8 * 8 * 12 * 1 * (64 + 2) * 4
    assert ws(_args(B=8, H=8, Tq=4, dk=128, cap=1500, Nk=1500, bf16=False)) == 8 * 8 * 24 * 4 * (128 + 2) * 4   # 64-key chunks
    assert ws(_args(Tq=0)) == 0


def test_bad_arguments_return_before_any_launch(lib):
    fn = lib.mopk_decode_attn_fwd
    assert fn(None, None) == -2
    for kw in (dict(B=0), dict(H=0), dict(Tq=0), dict(cap=0), dict(cap=10, Nk=11)):
        assert fn(C.byref(_args(**kw)), None) == -1, kw
    assert fn(C.byref(_args(Tq=17)), None) == -3
    assert fn(C.byref(_args(dk=96)), None) == -3
    assert fn(C.byref(_args(causal=2)), None) == -2
    assert fn(C.byref(_args()), None) == -2              # valid shape, null tensors


def _tiny_model(**kw):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    cfg = dict(n_mels=10, n_audio_ctx=40, vocab_size=100, n_text_ctx=64, n_embd=32, n_head=2, n_layer_enc=1, n_layer_dec=2,
               n_views=3, n_kernels=2, kernel_size=3)
    cfg.update(kw)
    torch.manual_seed(0)
    return WhisperMoP(WhisperConfig(**cfg)).eval()


def test_length_errors_before_device_work():
    m = _tiny_model()
    enc = torch.randn(2, 40, 32)
    with pytest.raises(ValueError, match="n_text_ctx"):
        m.init_decode_cache(enc, 65)
    with pytest.raises(ValueError, match="n_text_ctx"):
        m.init_decode_cache(enc, 0)
    mel, ids = torch.randn(2, 40, 10), torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="n_text_ctx"):
        m.generate(mel, ids, 61)                          # 4 + 61 > 64; a CPU encode would raise RuntimeError instead
    with pytest.raises(ValueError):
        m.generate(mel, ids, 0)


def test_op_shape_errors():
    from mop_amd import ops
    q, k = torch.randn(2, 1, 4, 32), torch.randn(2, 10, 4, 32)
    with pytest.raises(ValueError):
        ops.decode_attention(q, k, torch.randn(2, 11, 4, 32))
    with pytest.raises(ValueError):
        ops.decode_attention(torch.randn(3, 1, 4, 32), k, k)
    with pytest.raises(ValueError):
        ops.decode_attention(q, k, k, nk=11)
    with pytest.raises(ValueError):
        ops.decode_attention(q[0], k, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_attention(q, k, k, nk=5)


def _ref64(q, k, v, L, causal):
    """float64 loops: query i sees keys j < L (and j < L - Tq + i + 1 with causal); no key -> 0"""
    B, Tq, H, dk = q.shape
    y = torch.zeros(B, Tq, H, dk, dtype=torch.float64)
    for i in range(Tq):
        n = min(L - Tq + i + 1, L) if causal else L
        if n <= 0:
            continue
        s = torch.einsum("bhd,bjhd->bhj", q[:, i].double(), k[:, :n].double()) / dk ** 0.5
        y[:, i] = torch.einsum("bhj,bjhd->bhd", s.softmax(-1), v[:, :n].double())
    return y.reshape(B, Tq, H * dk)


@pytest.mark.parametrize("causal", [False, True])
def test_torch_composition_vs_float64(causal):
    from mop_amd import ops
    torch.manual_seed(1)
    cap = 70
    k, v = torch.randn(2, cap, 3, 16), torch.randn(2, cap, 3, 16)
    for Tq in (1, 3, 8):
        q = torch.randn(2, Tq, 3, 16)
        for L in (1, 2, 9, 64, 70):
            ref = _ref64(q, k, v, L, causal)
            got = ops.decode_attention_torch(q, k, v, kv_len=torch.tensor([L], dtype=torch.int32), causal=causal)
            assert (got.double() - ref).abs().max() < 1e-5, (Tq, L)
            got = ops.decode_attention_torch(q, k, v, nk=L, causal=causal)
            assert (got.double() - ref).abs().max() < 1e-5, (Tq, L)
    vn = v.clone()
    vn[:, 40:] = float("nan")                             # rows past the length are never used
    got = ops.decode_attention_torch(q, k, vn, kv_len=torch.tensor([40], dtype=torch.int32), causal=causal)
    assert torch.isfinite(got).all()


@pytest.fixture
def torch_cores(monkeypatch):
    """route the attention cores through torch so the module logic runs on the CPU"""
    from mop_amd import ops

    def sdpa(q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p=0.0, seed=None):
        y = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=bias, is_causal=causal)
        return y.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)

    monkeypatch.setattr(ops, "sdpa_core", sdpa)
    monkeypatch.setattr(ops, "decode_attention", lambda q, k, v, kv_len=None, nk=None, causal=False:
                        ops.decode_attention_torch(q, k, v, kv_len, nk, causal))


@pytest.mark.parametrize("prompt", [1, 4, 20])
@pytest.mark.parametrize("pos", [True, False])
def test_decode_step_bookkeeping_with_torch_cores(torch_cores, prompt, pos):
    m = _tiny_model(use_abs_pos_emb=pos)
    enc = torch.randn(2, 40, 32)
    ids = torch.randint(0, 100, (2, 30))
    cache = m.init_decode_cache(enc, 30)
    assert cache.self_k[0].shape == (2, 30, 2, 16) and cache.cross_k[1].shape == (2, 40, 2, 16) and cache.length.dtype == torch.int32
    lg = m.decode_step(cache, ids[:, :prompt])
    assert lg.shape == (2, prompt, 100)
    assert (lg - m.decode(enc, ids[:, :prompt])).abs().max() < 1e-5
    t = prompt
    while t < 30:                                         # single tokens, then a 3-token chunk (bottom-right causal)
        n = 3 if t == prompt + 2 else 1
        lg = m.decode_step(cache, ids[:, t:t + n])
        assert (lg - m.decode(enc, ids[:, :t + n])[:, t:]).abs().max() < 1e-5, t
        t += n
    assert int(cache.length) == 30 and cache.pos == 30
    with pytest.raises(ValueError, match="max_len"):
        m.decode_step(cache, ids[:, :1])


def test_generate_matches_the_naive_loop_with_torch_cores(torch_cores):
    m = _tiny_model()
    mel = torch.randn(2, 40, 10)
    prompt = torch.randint(0, 100, (2, 3))
    out, steps = m.generate(mel, prompt, 12, return_logits=True)
    enc, _ = m.encode(mel)
    cur = prompt
    for _ in range(12):
        cur = torch.cat([cur, m.decode(enc, cur)[:, -1].argmax(-1, keepdim=True)], dim=1)
    assert torch.equal(out, cur) and steps.shape == (2, 12, 100)
    eos = int(out[0, 5])
    got = m.generate(mel, prompt, 12, eos_token_id=eos)
    for r in range(2):
        hit = (got[r, 3:] == eos).nonzero()
        if len(hit):
            assert (got[r, 3 + int(hit[0]):] == eos).all()
    assert torch.equal(got[0, :6], out[0, :6])


def test_whgen_fixtures():
    from mop_amd.nn import WhisperConfig, WhisperMoP
    assert {"whgen_p1", "whgen_p4_nopos", "whgen_p4_t140"} <= set(WHGEN)
    lengths = []
    for name in WHGEN:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 0.6e6
        d, params, _, meta = load_golden(name)
        B, Tp, n_new, V = d["prompt"].shape[0], int(meta["T_p"]), int(meta["n_new"]), int(meta["vocab"])
        assert d["prompt"].shape == (B, Tp) and d["tokens"].shape == (B, Tp + n_new)
        assert np.array_equal(d["tokens"][:, :Tp], d["prompt"])
        assert d["step_logits"].shape == (B, n_new, V) and d["mel"].shape == (B, int(meta["T_a"]), int(meta["n_mels"]))
        assert np.array_equal(d["step_logits"].argmax(-1), d["tokens"][:, Tp:])
        top = np.sort(d["step_logits"], axis=-1)[..., -2:]
        assert float(meta["min_margin"]) >= 1e-3 and (top[..., 1] - top[..., 0]).min() >= 1e-3
        cfg = WhisperConfig(n_mels=int(meta["n_mels"]), n_audio_ctx=int(meta["T_a"]), vocab_size=V, n_text_ctx=int(meta["n_text_ctx"]),
                            n_embd=int(meta["dim"]), n_head=int(meta["heads"]), n_layer_enc=int(meta["n_layer_enc"]),
                            n_layer_dec=int(meta["n_layer_dec"]), use_abs_pos_emb=bool(meta["use_abs_pos_emb"]),
                            n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]), kernel_size=int(meta["kernel_size"]))
        sd = WhisperMoP(cfg).state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}
        lengths.append(Tp + n_new)
    assert max(lengths) > 130                             # crosses the 64- and 128-key chunk edges
