"""-m gpu: KV-cached WhisperMoP decoding on the split-KV HIP kernels (mopk_decode_attn_*).  ops.decode_attention against float64
over query counts, chunk-edge lengths, head sizes, dtypes, causal and strided caches; the torch path for an unsupported head size;
the device-driven length; decode_step against decode (teacher-forced); generate against the reference's greedy tokens (whgen_*) and
against the naive re-decode loop at a Whisper-base-like size; EOS pinning; bitwise reproducibility; no host sync; graph replay."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu
WHGEN = golden_names("whgen_")


def _ref64(q, k, v, L, causal):
    B, Tq, H, dk = q.shape
    y = torch.zeros(B, Tq, H, dk, dtype=torch.float64, device=q.device)
    for i in range(Tq):
        n = min(L - Tq + i + 1, L) if causal else L
        if n <= 0:
            continue
        s = torch.einsum("bhd,bjhd->bhj", q[:, i].double(), k[:, :n].double()) / dk ** 0.5
        y[:, i] = torch.einsum("bhj,bjhd->bhd", s.softmax(-1), v[:, :n].double())
    return y.reshape(B, Tq, H * dk)


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _cache(B, cap, H, dk, dtype, seed):
    """k, v as strided views of one packed (B, cap + 5, 2, H + 1, dk) buffer: cap > the lengths used, head and row strides != dk"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.randn(B, cap + 5, 2, H + 1, dk, device="cuda", generator=g).to(dtype)
    return buf[:, :cap, 0, :H], buf[:, :cap, 1, :H]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_op_sweep_vs_float64(dtype, dk, causal):
    from mop_amd import _lib, ops
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    tol = 1e-5 if dtype == "fp32" else 1e-2
    B, H, cap = 2, 3, 1507
    k, v = _cache(B, cap, H, dk, dt, dk)
    g = torch.Generator(device="cuda").manual_seed(7)
    for Tq in (1, 2, 4, 16):
        q = torch.randn(B, Tq, H + 2, dk, device="cuda", generator=g).to(dt)[:, :, 1:H + 1]      # strided q as well
        for L in (1, 63, 64, 65, 448, 1500):
            kv_len = torch.tensor([L], dtype=torch.int32, device="cuda")
            y = ops.decode_attention(q, k, v, kv_len=kv_len, causal=causal)
            assert ops.LAST_PATH["decode_attn"] == _lib.PATH_FUSED
            ref = _ref64(q, k, v, L, causal)
            assert y.shape == (B, Tq, H * dk) and y.dtype == dt
            assert _rel(y, ref) <= tol, (Tq, L, _rel(y, ref))
            y2 = ops.decode_attention(q, k[:, :L], v[:, :L], nk=L, causal=causal)
            assert _rel(y2, ref) <= tol, (Tq, L)


def test_unsupported_head_size_takes_the_torch_path():
    from mop_amd import _lib, ops
    k, v = _cache(2, 100, 2, 48, torch.float32, 3)
    q = torch.randn(2, 1, 2, 48, device="cuda")
    kv_len = torch.tensor([77], dtype=torch.int32, device="cuda")
    y = ops.decode_attention(q, k, v, kv_len=kv_len, causal=True)
    assert ops.LAST_PATH["decode_attn"] == _lib.PATH_GENERIC
    assert _rel(y, _ref64(q, k, v, 77, True)) <= 1e-5
    q17 = torch.randn(2, 17, 2, 48, device="cuda")
    ops.decode_attention(q17, k, v, nk=50)
    assert ops.LAST_PATH["decode_attn"] == _lib.PATH_GENERIC


def test_length_is_read_from_the_device():
    from mop_amd import ops
    k, v = _cache(2, 600, 4, 64, torch.bfloat16, 5)
    q = torch.randn(2, 1, 4, 64, device="cuda", dtype=torch.bfloat16)
    kv_len = torch.tensor([100], dtype=torch.int32, device="cuda")
    a = ops.decode_attention(q, k, v, kv_len=kv_len, causal=True)
    kv_len.fill_(513)
    b = ops.decode_attention(q, k, v, kv_len=kv_len, causal=True)
    assert _rel(a, _ref64(q, k, v, 100, True)) <= 1e-2 and _rel(b, _ref64(q, k, v, 513, True)) <= 1e-2
    assert not torch.equal(a, b)


def _model(d=128, H=2, Ta=200, vocab=300, ctx=64, L=2, pos=True):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=Ta, vocab_size=vocab, n_text_ctx=ctx, n_embd=d, n_head=H, n_layer_enc=1,
                        n_layer_dec=L, use_abs_pos_emb=pos)
    return WhisperMoP(cfg).cuda().eval()


@pytest.mark.parametrize("prompt", [1, 4, 20])
@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])
def test_decode_step_matches_decode(prompt, mode):
    from mop_amd import _lib, ops
    m = _model()
    tol = 1e-4 if mode == "fp32" else 2e-2
    mel = torch.randn(2, 200, 12, device="cuda")
    ids = torch.randint(0, 300, (2, 48), device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
        enc, _ = m.encode(mel)
        cache = m.init_decode_cache(enc, 48)
        assert cache.dtype == (torch.float32 if mode == "fp32" else torch.bfloat16)
        lg = m.decode_step(cache, ids[:, :prompt])
        ref = m.decode(enc, ids[:, :prompt])
        assert _rel(lg.float(), ref.float()) <= tol
        for t in range(prompt, 48):
            lg = m.decode_step(cache, ids[:, t:t + 1])[:, -1]
            assert ops.LAST_PATH["decode_attn"] == _lib.PATH_FUSED
            ref = m.decode(enc, ids[:, :t + 1])[:, -1]
            assert _rel(lg.float(), ref.float()) <= tol, (t, _rel(lg.float(), ref.float()))


def _whgen_model(meta, params):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    cfg = WhisperConfig(n_mels=int(meta["n_mels"]), n_audio_ctx=int(meta["T_a"]), vocab_size=int(meta["vocab"]),
                        n_text_ctx=int(meta["n_text_ctx"]), n_embd=int(meta["dim"]), n_head=int(meta["heads"]),
                        n_layer_enc=int(meta["n_layer_enc"]), n_layer_dec=int(meta["n_layer_dec"]),
                        use_abs_pos_emb=bool(meta["use_abs_pos_emb"]), n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]),
                        kernel_size=int(meta["kernel_size"]))
    m = WhisperMoP(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.cuda().eval()


@pytest.mark.parametrize("name", WHGEN)
def test_generate_reproduces_the_reference_tokens(name):
    from mop_amd import _lib, ops
    d, params, _, meta = load_golden(name)
    m = _whgen_model(meta, params)
    mel = torch.from_numpy(d["mel"]).cuda()
    prompt = torch.from_numpy(d["prompt"]).cuda()
    out, steps = m.generate(mel, prompt, int(meta["n_new"]), return_logits=True)
    assert ops.LAST_PATH["decode_attn"] == _lib.PATH_FUSED
    assert torch.equal(out.cpu(), torch.from_numpy(d["tokens"]))
    ref = torch.from_numpy(d["step_logits"]).double()
    assert _rel(steps.cpu(), ref) <= 1e-4


def _base_model():
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=80, n_audio_ctx=1500, vocab_size=51865, n_text_ctx=448, n_embd=512, n_head=8, n_layer_enc=6,
                        n_layer_dec=6)
    m = WhisperMoP(cfg)
    with torch.no_grad():                  # at the default init every logit gap is ~1e-2: widen them so most steps clear 1e-3
        m.dec_ln_f.weight.mul_(20.0)
    return m.cuda().eval()


def test_tokens_match_the_naive_loop_at_the_bench_size():
    m = _base_model()
    B, n_new = 2, 220
    mel = torch.randn(B, 1500, 80, device="cuda")
    prompt = torch.randint(0, 51865, (B, 4), device="cuda")
    with torch.no_grad():
        out = m.generate(mel, prompt, n_new)
        enc, _ = m.encode(mel)
        cur, first_close = prompt, n_new
        for t in range(n_new):
            lg = m.decode(enc, cur)[:, -1]
            top = lg.topk(2, dim=-1).values
            if float((top[:, 0] - top[:, 1]).min()) < 1e-3:
                first_close = t
                break
            cur = torch.cat([cur, lg.argmax(-1, keepdim=True)], dim=1)
    assert first_close > 0
    assert torch.equal(out[:, :4 + first_close], cur[:, :4 + first_close])
    # EOS: row 0's third new token is the EOS; every row matches the plain run up to its first EOS and stays EOS after it
    eos = int(out[0, 6])
    got = m.generate(mel, prompt, 40, eos_token_id=eos)
    for r in range(B):
        hit = (out[r, 4:44] == eos).nonzero()
        f = 4 + int(hit[0]) if len(hit) else 44
        assert torch.equal(got[r, :min(f + 1, 44)], out[r, :min(f + 1, 44)]), r
        assert (got[r, f:] == eos).all(), r


def test_generate_is_bitwise_reproducible():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(2, 300, 12, device="cuda")
    prompt = torch.randint(0, 1000, (2, 4), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a, la = m.generate(mel, prompt, 80, return_logits=True)
        b, lb = m.generate(mel, prompt, 80, return_logits=True)
    assert torch.equal(a, b) and torch.equal(la[:, -1], lb[:, -1])


def test_no_host_sync():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(2, 300, 12, device="cuda")
    prompt = torch.randint(0, 1000, (2, 4), device="cuda")
    ids = torch.randint(0, 1000, (2, 40), device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        enc, _ = m.encode(mel)
        cache = m.init_decode_cache(enc, 40)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.decode_step(cache, ids[:, :4])
            for t in range(4, 36):
                m.decode_step(cache, ids[:, t:t + 1])
            out = m.generate(mel, prompt, 30, eos_token_id=3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.shape == (2, 34) and cache.pos == 36


def test_graph_replay_reproduces_eager():
    """generate(graph=True) against eager generate, in its own process (tools/graph_probe_whisper_decode.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_decode.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-400:]
