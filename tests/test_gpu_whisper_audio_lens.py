"""-m gpu: per-row audio lengths (clips of different lengths in one WhisperMoP batch).  ops.sdpa_core(q_lens, kv_lens)
(mopk_sdpa_lens_*) against a float64 loop, forward and all three gradients, fp32 and bf16, dk in {32, 64}, causal and not, square and
rectangular, strided views, lengths of 0, 1, inside a tile, on a tile edge, full and outside [0, N]; exact zeros on padding rows; NaN
/ Inf beyond the lengths change nothing; full lengths bitwise the call without lengths; the attn_mask route and its dropout mask.
ops.decode_attention_lens (mopk_decode_attn_lens_*) likewise.  forward / backward / generate / beam_search / sample on a list of clips
against each clip alone (fp32), with ragged prompts too, reproducibility, eos pinning, no host sync and graph replay.

Bounds: kernels against float64 2e-5 (fp32) / 2e-2 (bf16) of max(1, |reference|max) -- fp32 arithmetic against bf16's 2^-8 steps on
operands the reference shares --, model logits 1e-4 in fp32, parameter gradients 1e-3 relative (README)."""
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_whisper_beam import _model
from test_gpu_whisper_ragged import _close_step
from test_whisper_audio_lens_cpu import naive_lens_attention

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-5, "bf16": 2e-2}


def _err(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / max(1.0, float(ref.abs().max())))


def _lens_case(dtype, dk, causal, square, seed=0):
    """strided (B, N, H, dk) views and a set of lengths that hits 0, 1, inside a 64-key tile, a tile edge, the full length and
    values outside [0, N]"""
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(seed + dk + 2 * causal)
    B, H = 7, 2
    N, Nk = (200, 200) if square else (130, 300)

    def view(n):
        buf = torch.randn(B, n + 3, H + 1, dk, device="cuda", generator=g).to(dt)
        return buf[:, 2:n + 2, 1:]
    q, k, v, dy = view(N), view(Nk), view(Nk), torch.randn(B, N, H * dk, device="cuda", generator=g).to(dt)
    kl = torch.tensor([0, 1, 37, 64, 128, Nk, Nk + 50], dtype=torch.int32, device="cuda")
    kl[0] = -4 if not square else 0
    ql = kl if square else None
    return q, k, v, dy, ql, kl


def _run(q, k, v, dy, **kw):
    from mop_amd import ops
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))       # contiguous leaves
    y = ops.sdpa_core(q, k, v, **kw)
    y.backward(dy)
    return y.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("causal,square", [(False, True), (True, True), (False, False)])       # causal is square only
def test_sdpa_lens_matches_float64(dtype, dk, causal, square):
    from mop_amd import _lib, ops
    q, k, v, dy, ql, kl = _lens_case(dtype, dk, causal, square)
    B, N, H, _ = q.shape
    Nk = k.shape[1]
    qs, ks, vs = (t.detach().requires_grad_(True) for t in (q, k, v))             # the strided views themselves
    y = ops.sdpa_core(qs, ks, vs, causal=causal, q_lens=ql, kv_lens=kl)
    assert ops.LAST_PATH["sdpa_fwd"] == (_lib.PATH_FUSED if dtype == "bf16" else _lib.PATH_GENERIC)
    dq, dk_, dv = torch.autograd.grad(y, (qs, ks, vs), dy)
    assert ops.LAST_PATH["sdpa_bwd"] == ops.LAST_PATH["sdpa_fwd"]
    q64, k64, v64 = (t.detach().cpu().double().requires_grad_(True) for t in (q, k, v))
    ref = naive_lens_attention(q64, k64, v64, None if ql is None else ql.cpu(), kl.cpu(), causal)
    rq, rk, rv = torch.autograd.grad(ref, (q64, k64, v64), dy.cpu().double())
    for name, got, want in (("y", y, ref.detach()), ("dq", dq, rq.reshape(B, N, H, -1)), ("dk", dk_, rk), ("dv", dv, rv)):
        e = _err(got.reshape(want.shape), want)
        print(f"sdpa_lens {dtype} dk={dk} causal={causal} square={square} {name}: {e:.3e} (bound {TOL[dtype]:.0e})")
        assert e <= TOL[dtype], (name, e)
    nq = (ql if ql is not None else torch.full_like(kl, N)).clamp(0, N).tolist()
    nk = kl.clamp(0, Nk).tolist()
    for b in range(B):                                                            # padding rows are exactly 0, and written
        assert not y[b, nq[b]:].any() and not dq[b, nq[b]:].any(), b
        assert not dk_[b, nk[b]:].any() and not dv[b, nk[b]:].any(), b


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("square", [True, False])
def test_nothing_beyond_a_length_is_used(dtype, square):
    q, k, v, dy, ql, kl = _lens_case(dtype, 64, False, square, seed=5)
    B, N = q.shape[:2]
    Nk = k.shape[1]
    base = _run(q, k, v, dy, q_lens=ql, kv_lens=kl)
    q2, k2, v2, dy2 = (t.detach().clone() for t in (q, k, v, dy))
    for b in range(B):
        nk = min(max(int(kl[b]), 0), Nk)
        k2[b, nk:] = float("nan")
        v2[b, nk:] = float("inf")
        if ql is not None:
            nq = min(max(int(ql[b]), 0), N)
            q2[b, nq:] = float("-inf")
            dy2[b, nq:] = float("nan")
    poisoned = _run(q2, k2, v2, dy2, q_lens=ql, kv_lens=kl)
    for name, a, c in zip(("y", "dq", "dk", "dv"), base, poisoned):
        assert torch.equal(a, c), name                                            # bitwise, so also finite everywhere


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("causal", [False, True])
def test_full_lengths_are_bitwise_the_call_without_lengths(dtype, dk, causal):
    q, k, v, dy, _, _ = _lens_case(dtype, dk, causal, causal, seed=9)
    B, N = q.shape[:2]
    Nk = k.shape[1]
    plain = _run(q, k, v, dy, causal=causal)
    fq = torch.full((B,), N, dtype=torch.int32, device="cuda")
    fk = torch.full((B,), Nk, dtype=torch.int32, device="cuda")
    for kw in (dict(q_lens=fq, kv_lens=fk), dict(kv_lens=fk), dict(q_lens=fq), dict(q_lens=fq + 7, kv_lens=fk + 1)):
        got = _run(q, k, v, dy, causal=causal, **kw)
        for name, a, c in zip(("y", "dq", "dk", "dv"), plain, got):
            assert torch.equal(a, c), (name, sorted(kw))
    drop = _run(q, k, v, dy, causal=causal, dropout_p=0.25, seed=77)
    got = _run(q, k, v, dy, causal=causal, dropout_p=0.25, seed=77, q_lens=fq, kv_lens=fk)
    assert all(torch.equal(a, c) for a, c in zip(drop, got))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("pdrop", [0.0, 0.2])
def test_kv_lens_equals_the_attn_mask_route(dtype, pdrop):
    """the baseline a user has without lengths: a (B, 1, 1, Nk) key-padding mask; with dropout the same seed draws the same mask"""
    q, k, v, dy, _, kl = _lens_case(dtype, 64, False, False, seed=13)
    B, Nk = q.shape[0], k.shape[1]
    mask = (torch.arange(Nk, device="cuda").view(1, Nk) < kl.view(B, 1)).view(B, 1, 1, Nk)
    kw = dict(dropout_p=pdrop, seed=31) if pdrop else {}
    a = _run(q, k, v, dy, kv_lens=kl, **kw)
    c = _run(q, k, v, dy, attn_mask=mask, **kw)
    for name, x, z in zip(("y", "dq", "dk", "dv"), a, c):
        e = _err(x, z.cpu().double())
        print(f"kv_lens vs attn_mask {dtype} p={pdrop} {name}: {e:.3e} (bound {TOL[dtype]:.0e})")
        assert e <= TOL[dtype], (name, e)


def test_lengths_fold_into_a_mask_when_a_bias_is_given():
    from mop_amd import ops
    q, k, v, dy, _, kl = _lens_case("fp32", 32, False, False, seed=17)
    B, N, H, _ = q.shape
    Nk = k.shape[1]
    bias = torch.randn(1, H, N, Nk, device="cuda")
    y = ops.sdpa_core(q, k, v, bias=bias, kv_lens=kl)
    mask = (torch.arange(Nk, device="cuda").view(1, Nk) < kl.view(B, 1)).view(B, 1, 1, Nk)
    assert torch.equal(y, ops.sdpa_core(q, k, v, bias=bias, attn_mask=mask))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64, 128])
def test_decode_attention_lens_matches_float64(dtype, dk):
    from mop_amd import _lib, ops
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(dk)
    B, H, cap, nk = 6, 2, 300, 261
    chunk = min(32768 // (dk * (4 if dtype == "fp32" else 2)), 128)
    kbuf = torch.randn(B, cap + 5, H + 1, dk, device="cuda", generator=g).to(dt)
    vbuf = torch.randn(B, cap + 5, H + 1, dk, device="cuda", generator=g).to(dt)
    k, v = kbuf[:, 2:cap + 2, 1:], vbuf[:, 3:cap + 3, :H]                     # strided (B, cap, H, dk) views
    lens = torch.tensor([0, 37, chunk, 2 * chunk + 1, nk, nk + 90], dtype=torch.int32, device="cuda")
    full = torch.full((B,), nk, dtype=torch.int32, device="cuda")
    kn, vn = k.clone(), v.clone()
    for b in range(B):
        kn[b, min(int(lens[b]), nk):] = float("nan")
        vn[b, min(int(lens[b]), nk):] = float("inf")
    for Tq in (1, 5, 16):
        q = torch.randn(B, Tq, H, dk, device="cuda", generator=g).to(dt)
        y = ops.decode_attention_lens(q, k, v, lens, nk=nk)
        assert ops.LAST_PATH["decode_attn_lens"] == _lib.PATH_FUSED
        ref = naive_lens_attention(q.cpu().float(), k.cpu().float()[:, :nk], v.cpu().float()[:, :nk], None, lens.cpu())
        e = float((y.cpu().double() - ref).abs().max())
        print(f"decode_attention_lens {dtype} dk={dk} Tq={Tq}: {e:.3e} (bound {TOL[dtype]:.0e})")
        assert e <= TOL[dtype], Tq
        assert torch.equal(y[0], torch.zeros_like(y[0]))                       # no key: exactly 0
        assert torch.equal(ops.decode_attention_lens(q, k, v, full, nk=nk), ops.decode_attention(q, k, v, nk=nk)), Tq
        assert torch.equal(ops.decode_attention_lens(q, kn, vn, lens, nk=nk), y), Tq       # rows beyond a length are never read


def test_decode_attention_lens_falls_back_where_the_kernels_refuse():
    from mop_amd import _lib, ops
    q, k = torch.randn(3, 20, 2, 48, device="cuda"), torch.randn(3, 30, 2, 48, device="cuda")
    lens = torch.tensor([0, 7, 30], dtype=torch.int32, device="cuda")
    y = ops.decode_attention_lens(q, k, k, lens, nk=25)
    assert ops.LAST_PATH["decode_attn_lens"] == _lib.PATH_GENERIC
    ref = naive_lens_attention(q.cpu(), k.cpu()[:, :25], k.cpu()[:, :25], None, lens.cpu())
    assert (y.cpu().double() - ref).abs().max() < 1e-5


# ------------------------------------------------------------------ model level (fp32)
CLIPS = [200, 137, 64, 1]
SEED = 3


def _clips(seed=SEED):
    """drawn on the CPU, so that the same clips can be replayed without a GPU"""
    torch.manual_seed(seed)
    return [torch.randn(n, 12).cuda() for n in CLIPS]


def _prompt(*shape, seed=SEED):
    torch.manual_seed(seed + 100)
    return torch.randint(0, 300, shape).cuda()


def test_forward_and_gradients_equal_each_clip_alone():
    from mop_amd.nn import EncodedAudio
    m = _model(widen=10.0)
    clips = _clips()
    ids = torch.randint(0, 300, (4, 20), device="cuda")
    tg = torch.randint(0, 300, (4, 20), device="cuda")
    tg[1, 15:] = -100
    tg[3, 3:] = -100
    logits, loss, gates = m(clips, ids, tg)
    assert isinstance(m.encode(clips)[0], EncodedAudio) and gates.shape == (4, 1, 200)
    grads = torch.autograd.grad(loss, list(m.parameters()), allow_unused=True)
    n_all = int((tg != -100).sum())
    want = [torch.zeros_like(p) for p in m.parameters()]
    for b, c in enumerate(clips):
        rl, lb, rg = m(c.unsqueeze(0), ids[b:b + 1], tg[b:b + 1])
        e = float((logits[b] - rl[0]).abs().max())
        print(f"forward clip {b} ({CLIPS[b]} frames): logits {e:.3e} (bound 1e-4)")
        assert e <= 1e-4, b
        assert float((gates[b, :, :CLIPS[b]] - rg[0]).abs().max()) <= 1e-4, b
        w = int((tg[b] != -100).sum()) / n_all
        for acc, g in zip(want, torch.autograd.grad(lb, list(m.parameters()), allow_unused=True)):
            if g is not None:
                acc += g * w
    for (name, _), g, w in zip(m.named_parameters(), grads, want):
        g = torch.zeros_like(w) if g is None else g
        e = float((g - w).abs().max() / w.abs().max().clamp_min(1e-12))
        assert e <= 1e-3 or float((g - w).abs().max()) <= 1e-7, (name, e)       # relative 1e-3; a gradient that is 0 (below fp32's
        #                                                                         rounding of the loss, 1e-7) compares absolutely


def test_generate_equals_each_clip_alone():
    from mop_amd import _lib, ops
    m = _model(widen=10.0)
    clips = _clips()
    prompt = _prompt(4, 4)
    n_new = 24
    out, steps = m.generate(clips, prompt, n_new, return_logits=True)
    assert ops.LAST_PATH["decode_attn_lens"] == _lib.PATH_FUSED
    for b, c in enumerate(clips):
        ref, rs = m.generate(c.unsqueeze(0), prompt[b:b + 1], n_new, return_logits=True)
        f = _close_step(rs[0])                          # tokens 0 .. f - 1 come from identical prefixes, logits 0 .. f too
        assert 2 * f >= n_new, (b, f)                   # at least half of the steps are compared in every row
        assert torch.equal(out[b, :4 + f], ref[0, :4 + f]), b
        assert (steps[b, :f + 1] - rs[0, :f + 1]).abs().max() <= 1e-4, b
    eos = int(out[1, 4 + 2])
    got = m.generate(clips, prompt, n_new, eos_token_id=eos)
    for b in range(4):
        hit = (out[b, 4:] == eos).nonzero()
        e = 4 + int(hit[0]) if len(hit) else 4 + n_new
        assert torch.equal(got[b, :e + 1], out[b, :e + 1]) and (got[b, e:] == eos).all(), b
    assert torch.equal(out, m.generate(clips, prompt, n_new))                   # two runs: bitwise


def test_generate_with_ragged_prompts_too():
    m = _model(widen=10.0)
    clips = _clips()
    prompts = [_prompt(n, seed=SEED + n) for n in (1, 4, 17, 40)]
    n_new = 20
    out, steps = m.generate(clips, prompts, n_new, return_logits=True)
    for b, (c, p) in enumerate(zip(clips, prompts)):
        ref, rs = m.generate(c.unsqueeze(0), p.unsqueeze(0), n_new, return_logits=True)
        f = _close_step(rs[0])
        assert 2 * f >= n_new, (b, f)
        assert torch.equal(out[b][:len(p) + f], ref[0][:len(p) + f]), b
        assert (steps[b, :f + 1] - rs[0, :f + 1]).abs().max() <= 1e-4, b


def test_beam_search_equals_the_uniform_batch_of_each_clip():
    m = _model(widen=10.0)
    clips = _clips()
    prompt = _prompt(4, 4)
    tok, sc = m.beam_search(clips, prompt, 20, 3, eos_token_id=5)
    tok2, sc2 = m.beam_search(clips, prompt, 20, 3, eos_token_id=5)
    assert torch.equal(tok, tok2) and torch.equal(sc, sc2)
    same = 0
    for b, c in enumerate(clips):
        rt, rsc = m.beam_search(c.unsqueeze(0).repeat(4, 1, 1), prompt, 20, 3, eos_token_id=5)
        if torch.equal(tok[b], rt[b]):
            same += 1
            assert abs(float(sc[b]) - float(rsc[b])) <= 1e-4, b
        else:                                          # a different path only where the uniform batch's ranking nearly ties
            rg = m.generate(c.unsqueeze(0), prompt[b:b + 1], 20, return_logits=True)[1][0]
            assert _close_step(rg, 1e-3) < 20 and abs(float(sc[b]) - float(rsc[b])) <= 1e-3, b
    assert same >= 2                                   # the escape clause may serve at most half of the rows


def test_sample_equals_the_uniform_batch_of_each_clip():
    m = _model(widen=10.0)
    clips = _clips()
    prompt = _prompt(4, 4)
    cfg = dict(temperature=0.7, top_k=50, top_p=0.95, num_samples=3, eos_token_id=9, seed=11)
    tok, lp = m.sample(clips, prompt, 20, **cfg)
    tok2, lp2 = m.sample(clips, prompt, 20, **cfg)
    assert torch.equal(tok, tok2) and torch.equal(lp, lp2)
    same = 0
    for b, c in enumerate(clips):
        rt, rlp = m.sample(c.unsqueeze(0).repeat(4, 1, 1), prompt, 20, **cfg)
        for s in range(3):
            if torch.equal(tok[b, s], rt[b, s]):
                same += 1
                assert abs(float(lp[b, s]) - float(rlp[b, s])) <= 1e-3, (b, s)
    assert same >= 11                                   # a draw may flip only at a near-tie of its perturbed scores


def test_no_host_sync():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    torch.manual_seed(1)
    clips = [torch.randn(n, 12, device="cuda") for n in (300, 137, 64, 1)]
    prompts = [torch.randint(0, 1000, (n,), device="cuda") for n in (1, 4, 17, 40)]
    ids = torch.randint(0, 1000, (4, 12), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m.train()
        m(clips, ids, ids)[1].backward()                                    # warm-up outside the check
        m.eval()
        with torch.no_grad():
            m.generate(clips, prompts, 4)
            m.sample(clips, prompts, 4, num_samples=2)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.train()
            m(clips, ids, ids)[1].backward()
            m.eval()
            with torch.no_grad():
                out = m.generate(clips, prompts, 30, eos_token_id=3)
                tok, _ = m.beam_search(clips, prompts, 30, 3)
                smp, _ = m.sample(clips, prompts, 30, num_samples=2, eos_token_id=3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert [len(o) for o in out] == [n + 30 for n in (1, 4, 17, 40)] and len(tok) == 4 and len(smp) == 4
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_training_step_with_dropout_and_bf16_autocast_is_finite():
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=200, vocab_size=300, n_text_ctx=64, n_embd=128, n_head=2, n_layer_enc=2, n_layer_dec=2,
                        dropout=0.1)
    m = WhisperMoP(cfg).cuda().train()
    clips = _clips()
    ids = torch.randint(0, 300, (4, 20), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss, _ = m(clips, ids, ids)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_graph_replay_reproduces_eager():
    """generate / beam_search / sample (graph=True) on a list of clips against eager, in its own process
    (tools/graph_probe_whisper_audio_lens.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_audio_lens.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-600:]
