"""-m gpu: ragged WhisperMoP decoding (prompts of different lengths left-padded in one cache).  ops.decode_attention_ragged
(mopk_decode_attn_ragged_*) against a float64 loop for fp32 / bf16, dk in {32, 64, 128}, causal and not, Tq in {1, 5, 16}, strided
cache views, with and without a row table, at starts of 0, inside a chunk, on a chunk edge, at L and outside [0, L]; kv_start = 0
bitwise equal to decode_attention / decode_attention_rows.  ops.sample_tokens_ragged (mopk_sample_ragged_*) against sample_tokens
at the shifted position and against its torch path.  generate / beam_search / sample on a ragged list against each prompt alone or
the uniform batch of each prompt (fp32), eos pinning per row, reproducibility, no host sync and graph replay."""
import os
import subprocess
import sys

import pytest
import torch

from sample_rows import _perturbed
from test_gpu_whisper_beam import _model
from test_whisper_ragged_cpu import naive_ragged_attention

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_attention_matches_float64(dtype, dk, causal):
    from mop_amd import _lib, ops
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(dk + causal)
    B, H, cap, L = 6, 2, 300, 261
    chunk = min(32768 // (dk * (4 if dtype == "fp32" else 2)), 128)
    kbuf = torch.randn(B, cap + 5, H + 1, dk, device="cuda", generator=g).to(dt)
    vbuf = torch.randn(B, cap + 5, H + 1, dk, device="cuda", generator=g).to(dt)
    k, v = kbuf[:, 2:cap + 2, 1:], vbuf[:, 3:cap + 3, :H]                     # strided (B, cap, H, dk) views
    kv_start = torch.tensor([0, 37, chunk, 2 * chunk + 1, L, -5], dtype=torch.int32, device="cuda")
    kv_len = torch.tensor([L], dtype=torch.int32, device="cuda")
    rows = torch.randint(0, B, (B, cap + 7), device="cuda", generator=g, dtype=torch.int32)
    ident = torch.arange(B, device="cuda", dtype=torch.int32).unsqueeze(1).repeat(1, cap)
    for Tq in (1, 5, 16):
        q = torch.randn(B, Tq, H, dk, device="cuda", generator=g).to(dt)
        for rt in (None, rows):
            y = ops.decode_attention_ragged(q, k, v, kv_start, rows=rt, kv_len=kv_len, causal=causal)
            assert ops.LAST_PATH["decode_attn_ragged"] == _lib.PATH_FUSED
            ref = naive_ragged_attention(q.cpu().float(), k.cpu().float(), v.cpu().float(), kv_start.cpu(),
                                         None if rt is None else rt.cpu(), L, causal)
            tol = 2e-5 if dtype == "fp32" else 2e-2
            assert (y.cpu().double() - ref).abs().max() <= tol, (Tq, rt is None)
            assert torch.equal(y[4], torch.zeros_like(y[4]))                   # kv_start = L: no key, exactly 0
            zero = torch.zeros(B, dtype=torch.int32, device="cuda")
            y0 = ops.decode_attention_ragged(q, k, v, zero, rows=rt, kv_len=kv_len, causal=causal)
            plain = (ops.decode_attention(q, k, v, kv_len=kv_len, causal=causal) if rt is None
                     else ops.decode_attention_rows(q, k, v, rt, kv_len=kv_len, causal=causal))
            assert torch.equal(y0, plain), (Tq, rt is None)
        yi = ops.decode_attention_ragged(q, k, v, kv_start, rows=ident, kv_len=kv_len, causal=causal)
        assert torch.equal(yi, ops.decode_attention_ragged(q, k, v, kv_start, kv_len=kv_len, causal=causal))


def test_attention_falls_back_where_the_kernels_refuse():
    from mop_amd import _lib, ops
    q, k = torch.randn(2, 20, 2, 48, device="cuda"), torch.randn(2, 30, 2, 48, device="cuda")
    ks = torch.tensor([0, 7], dtype=torch.int32, device="cuda")
    y = ops.decode_attention_ragged(q, k, k, ks, nk=25, causal=True)
    assert ops.LAST_PATH["decode_attn_ragged"] == _lib.PATH_GENERIC
    ref = naive_ragged_attention(q.cpu(), k.cpu(), k.cpu(), ks.cpu(), None, 25, True)
    assert (y.cpu().double() - ref).abs().max() < 1e-5


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampling_offsets_the_position(dtype):
    from mop_amd import _lib, ops
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(5)
    R, V = 48, 51865
    x = (torch.randn(R, V, device="cuda", generator=g) * 2.5).to(dt)
    pos = torch.tensor([90], dtype=torch.int32, device="cuda")
    off = torch.randint(0, 60, (R,), device="cuda", generator=g, dtype=torch.int32)
    for T, k, p in [(0.7, 50, 0.95), (1.0, 0, 1.0), (0.0, 0, 1.0)]:
        tok, lp = ops.sample_tokens_ragged(x, pos, off, T, k, p, seed=77)
        assert ops.LAST_PATH["sample_ragged"] == _lib.PATH_FUSED
        t0, l0 = ops.sample_tokens_ragged(x, pos, torch.zeros_like(off), T, k, p, seed=77)
        ts, ls = ops.sample_tokens(x, pos, T, k, p, seed=77)
        assert torch.equal(t0, ts) and torch.equal(l0, ls)                    # pos_off = 0: bitwise sample_tokens
        tt, _ = ops.sample_tokens_ragged_torch(x, pos, off, T, k, p, seed=77)
        for r in range(R):
            tr, lr = ops.sample_tokens(x, pos - off[r], T, k, p, seed=77)      # row r alone at its own position
            assert int(tok[r]) == int(tr[r]) and float(lp[r]) == float(lr[r]), r
            if T > 0 and int(tok[r]) != int(tt[r]):                           # only a near-tie of the torch path's scores
                sc = _perturbed(x, int(pos) - int(off[r]), T, 77)[r]
                assert abs(float(sc[tok[r]]) - float(sc[tt[r]])) < 1e-4, r
            elif T == 0:
                assert int(tok[r]) == int(tt[r])


LENS = [1, 4, 17, 40]


def _inputs(seed=3):
    torch.manual_seed(seed)
    mel = torch.randn(len(LENS), 200, 12, device="cuda")
    prompts = [torch.randint(0, 300, (n,), device="cuda") for n in LENS]
    return mel, prompts


def _close_step(steps, tol=1e-3):
    """index of the first step whose top-1 / top-2 logit gap is below tol (len(steps) if none)"""
    top = steps.float().topk(2, dim=-1).values
    close = ((top[..., 0] - top[..., 1]) < tol).nonzero()
    return int(close[0, 0]) if len(close) else steps.shape[0]


def test_generate_equals_each_prompt_alone():
    from mop_amd import _lib, ops
    m = _model(widen=10.0)
    mel, prompts = _inputs()
    out, steps = m.generate(mel, prompts, 24, return_logits=True)
    assert ops.LAST_PATH["decode_attn_ragged"] == _lib.PATH_FUSED
    for b, p in enumerate(prompts):
        ref, rs = m.generate(mel[b:b + 1], p.unsqueeze(0), 24, return_logits=True)
        f = _close_step(rs[0])                          # tokens 0 .. f - 1 come from identical prefixes, logits 0 .. f too
        assert f > 0 and torch.equal(out[b][:LENS[b] + f], ref[0][:LENS[b] + f]), b
        assert (steps[b, :f + 1] - rs[0, :f + 1]).abs().max() <= 1e-4, b
    eos = int(out[1][4 + 2])
    got = m.generate(mel, prompts, 24, eos_token_id=eos)
    for b in range(4):
        hit = (out[b][LENS[b]:] == eos).nonzero()
        e = LENS[b] + int(hit[0]) if len(hit) else LENS[b] + 24
        assert torch.equal(got[b][:e + 1], out[b][:e + 1]) and (got[b][e:] == eos).all(), b
    assert all(torch.equal(a, c) for a, c in zip(out, m.generate(mel, prompts, 24)))       # two runs: bitwise


def test_beam_search_equals_the_uniform_batch_of_each_prompt():
    m = _model(widen=10.0)
    mel, prompts = _inputs()
    tok, sc = m.beam_search(mel, prompts, 20, 3, eos_token_id=5)
    tok2, sc2 = m.beam_search(mel, prompts, 20, 3, eos_token_id=5)
    assert all(torch.equal(a, c) for a, c in zip(tok, tok2)) and torch.equal(sc, sc2)
    for b, p in enumerate(prompts):
        rt, rsc = m.beam_search(mel, p.unsqueeze(0).repeat(4, 1), 20, 3, eos_token_id=5)
        if torch.equal(tok[b], rt[b]):
            assert abs(float(sc[b]) - float(rsc[b])) <= 1e-4, b
        else:                                          # a different path only where the uniform batch's ranking nearly ties
            rg = m.generate(mel[b:b + 1], p.unsqueeze(0), 20, return_logits=True)[1][0]
            assert _close_step(rg, 1e-3) < 20 and abs(float(sc[b]) - float(rsc[b])) <= 1e-3, b


def test_sample_equals_the_uniform_batch_of_each_prompt():
    from mop_amd import _lib, ops
    m = _model(widen=10.0)
    mel, prompts = _inputs()
    cfg = dict(temperature=0.7, top_k=50, top_p=0.95, num_samples=3, eos_token_id=9, seed=11)
    tok, lp = m.sample(mel, prompts, 20, **cfg)
    assert ops.LAST_PATH["sample_ragged"] == _lib.PATH_FUSED
    tok2, lp2 = m.sample(mel, prompts, 20, **cfg)
    assert all(torch.equal(a, c) for a, c in zip(tok, tok2)) and torch.equal(lp, lp2)
    same = 0
    for b, p in enumerate(prompts):
        rt, rlp = m.sample(mel, p.unsqueeze(0).repeat(4, 1), 20, **cfg)
        assert tok[b].shape == (3, LENS[b] + 20)
        for s in range(3):
            if torch.equal(tok[b][s], rt[b, s]):
                same += 1
                assert abs(float(lp[b, s]) - float(rlp[b, s])) <= 1e-3, (b, s)
    assert same >= 11                                   # a draw may flip only at a near-tie of its perturbed scores


def test_no_host_sync():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(4, 300, 12, device="cuda")
    prompts = [torch.randint(0, 1000, (n,), device="cuda") for n in LENS]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        m.generate(mel, prompts, 4)                                         # warm-up outside the check
        m.sample(mel, prompts, 4, num_samples=2)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = m.generate(mel, prompts, 30, eos_token_id=3)
            tok, _ = m.beam_search(mel, prompts, 30, 3)
            smp, _ = m.sample(mel, prompts, 30, num_samples=2, eos_token_id=3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert [len(o) for o in out] == [n + 30 for n in LENS] and [len(t) for t in tok] == [n + 30 for n in LENS]
    assert [tuple(s.shape) for s in smp] == [(2, n + 30) for n in LENS]


def test_graph_replay_reproduces_eager():
    """generate / beam_search / sample (graph=True) on a ragged list against eager, in its own process
    (tools/graph_probe_whisper_ragged.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_ragged.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-600:]
