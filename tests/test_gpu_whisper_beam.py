"""-m gpu: WhisperMoP beam search on the row-indirect decode attention (mopk_decode_attn_rows_*) and the beam step kernels
(mopk_beam_*).  decode_attention_rows against a float64 gather over head sizes, dtypes, chunk-edge lengths and tables (random,
repeated, identity: bitwise decode_attention); beam_step against beam_step_torch at V = 51865; beam_search(num_beams=1) against
generate (also on the whgen_* fixtures); fp32 beam_search against the naive re-decode oracle with asserted rank margins; exact search
on tiny vocabularies against brute force; bitwise reproducibility; no host sync; graph replay."""
import itertools
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import golden_names, load_golden
from test_whisper_beam_cpu import naive_beam_search

pytestmark = pytest.mark.gpu
WHGEN = golden_names("whgen_")


def _gather_ref64(q, k, v, rows, L):
    B, cap = k.shape[:2]
    r = rows[:, :cap].long()
    j = torch.arange(cap, device=k.device).unsqueeze(0)
    kg, vg = k[r, j].double()[:, :L], v[r, j].double()[:, :L]
    s = torch.einsum("bihd,bjhd->bhij", q.double(), kg) / q.shape[-1] ** 0.5
    return torch.einsum("bhij,bjhd->bihd", s.softmax(-1), vg).reshape(B, q.shape[1], -1)


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64, 128])
def test_rows_attention_vs_float64_gather(dtype, dk):
    from mop_amd import _lib, ops
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    tol = 1e-5 if dtype == "fp32" else 1e-2
    g = torch.Generator(device="cuda").manual_seed(dk)
    B, H, cap = 10, 3, 300
    buf = torch.randn(B, cap, 2, H, dk, device="cuda", generator=g).to(dt)
    k, v = buf[:, :, 0], buf[:, :, 1]
    q = torch.randn(B, 1, H, dk, device="cuda", generator=g).to(dt)
    ident = torch.arange(B, dtype=torch.int32, device="cuda").unsqueeze(1).repeat(1, cap + 4)
    tables = {"random": torch.randint(0, B, (B, cap + 4), dtype=torch.int32, device="cuda", generator=g),
              "repeat": (torch.arange(B, device="cuda") // 5 * 5).to(torch.int32).unsqueeze(1).repeat(1, cap + 4),
              "identity": ident}
    for L in (1, 63, 64, 65, 127, 128, 129, 300):
        kv_len = torch.tensor([L], dtype=torch.int32, device="cuda")
        for name, rows in tables.items():
            y = ops.decode_attention_rows(q, k, v, rows, kv_len=kv_len, causal=True)
            assert ops.LAST_PATH["decode_attn_rows"] == _lib.PATH_FUSED
            assert _rel(y, _gather_ref64(q, k, v, rows, L)) <= tol, (name, L)
        y = ops.decode_attention_rows(q, k, v, ident, kv_len=kv_len, causal=True)
        assert torch.equal(y, ops.decode_attention(q, k, v, kv_len=kv_len, causal=True)), L


def _state_tensors(st):
    return (st.scores, st.next_ids, st.parents, st.hist, st.rows, st.fin_tokens, st.fin_scores, st.fin_count, st.done)


@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_beam_step_matches_the_torch_composition(K, B):
    from mop_amd import _lib, ops
    V, Tp, T, eos = 51865, 3, 12, 50257
    g = torch.Generator(device="cuda").manual_seed(100 * K + B)
    prompt = torch.randint(0, V, (B, Tp), device="cuda", generator=g)
    sts = [ops.BeamState(prompt, K, T, eos_token_id=eos, length_penalty=0.9) for _ in range(2)]
    pos = torch.tensor([Tp], dtype=torch.int32, device="cuda")
    for t in range(T - Tp):
        rows = B if t == 0 else B * K
        lg = (torch.randn(rows, V, device="cuda", generator=g) * 3).to(torch.bfloat16 if t % 2 else torch.float32)
        lg[:, eos] += 14.0 if t >= 2 else -20.0          # eos competes from the third step on: hypotheses finish, items get done
        if t == 4 and B > 1:
            lg[1, :] = float("-inf")                     # a beam row with no finite logit
        ops.beam_step(lg, sts[0], pos)
        assert ops.LAST_PATH["beam_step"] == _lib.PATH_FUSED
        ops.beam_step_torch(lg, sts[1], pos)
        a, b = _state_tensors(sts[0]), _state_tensors(sts[1])
        for name, x, y in zip(("scores", "next_ids", "parents", "hist", "rows", "fin_tokens", "fin_scores", "fin_count", "done"),
                              a, b):
            if x.dtype == torch.float32:
                fin = torch.isfinite(y)
                assert torch.equal(torch.isfinite(x), fin) and torch.equal(x[~fin], y[~fin]), (name, t)
                assert torch.allclose(x[fin], y[fin], rtol=1e-5, atol=0), (name, t)
            else:
                assert torch.equal(x, y), (name, t)
        pos += 1
    assert int(sts[0].fin_count.sum()) > 0


def _model(d=128, H=2, Ta=200, vocab=300, ctx=64, L=2, seed=0, widen=1.0):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(seed)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=Ta, vocab_size=vocab, n_text_ctx=ctx, n_embd=d, n_head=H, n_layer_enc=1,
                        n_layer_dec=L)
    m = WhisperMoP(cfg)
    with torch.no_grad():
        m.dec_ln_f.weight.mul_(widen)
    return m.cuda().eval()


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])
def test_one_beam_equals_generate(mode):
    m = _model(widen=10.0)
    mel = torch.randn(3, 200, 12, device="cuda")
    prompt = torch.randint(0, 300, (3, 4), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
        greedy = m.generate(mel, prompt, 40)
        tok, _ = m.beam_search(mel, prompt, 40, 1)
        assert torch.equal(tok, greedy)
        eos = int(greedy[0, 10])
        assert torch.equal(m.beam_search(mel, prompt, 40, 1, eos_token_id=eos)[0], m.generate(mel, prompt, 40, eos_token_id=eos))


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
def test_one_beam_reproduces_the_whgen_tokens(name):
    d, params, _, meta = load_golden(name)
    m = _whgen_model(meta, params)
    mel = torch.from_numpy(d["mel"]).cuda()
    prompt = torch.from_numpy(d["prompt"]).cuda()
    n_new = int(meta["n_new"])
    tok, _ = m.beam_search(mel, prompt, n_new, 1)
    assert torch.equal(tok.cpu(), torch.from_numpy(d["tokens"]))
    eos = int(d["tokens"][0, int(meta["T_p"]) + 5])
    assert torch.equal(m.beam_search(mel, prompt, n_new, 1, eos_token_id=eos)[0], m.generate(mel, prompt, n_new, eos_token_id=eos))


@pytest.mark.parametrize("K", [2, 5, 8])
def test_fp32_beam_search_matches_the_naive_oracle(K):
    m = _model(widen=10.0)
    torch.manual_seed(21)
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, 300, (2, 3), device="cuda")
    tok0, _ = m.beam_search(mel, prompt, 16, K)
    eos = int(tok0[1, 3 + 6])
    tok, sc = m.beam_search(mel, prompt, 16, K, eos_token_id=eos)
    ref, rs, margin = naive_beam_search(m, mel, prompt, 16, K, eos=eos)
    assert margin > 1e-4, margin                          # no near-tie at a K-th / 2K-th rank boundary
    assert torch.equal(tok.cpu(), ref.cpu()) and torch.allclose(sc.cpu(), rs, rtol=1e-5)


@pytest.mark.parametrize("V,steps", [(2, 4), (8, 2)])
def test_exact_search_on_a_tiny_vocabulary(V, steps):
    m = _model(vocab=V, seed=3, widen=3.0)
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, V, (2, 2), device="cuda")
    tok, sc = m.beam_search(mel, prompt, steps, 8)
    enc, _ = m.encode(mel)
    for b in range(2):
        best, best_s, scored = None, -math.inf, []
        for seq in itertools.product(range(V), repeat=steps):
            ids = torch.cat([prompt[b], torch.tensor(seq, device="cuda")]).unsqueeze(0)
            with torch.no_grad():
                lp = torch.log_softmax(m.decode(enc[b:b + 1], ids[:, :-1]).double(), -1)[0, 1:]
            s = float(lp.gather(1, ids[0, 2:].unsqueeze(1)).sum())
            scored.append(s)
            if s > best_s:
                best, best_s = seq, s
        top = sorted(scored)[-2:]
        assert top[1] - top[0] > 1e-4                     # a unique best sequence
        assert tuple(tok[b, 2:].tolist()) == best, b
        assert abs(float(sc[b]) * steps - best_s) < 1e-4 * max(1.0, abs(best_s))


def test_bitwise_reproducible():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(2, 300, 12, device="cuda")
    prompt = torch.randint(0, 1000, (2, 4), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a, sa = m.beam_search(mel, prompt, 60, 5, eos_token_id=3)
        b, sb = m.beam_search(mel, prompt, 60, 5, eos_token_id=3)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_no_host_sync():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(2, 300, 12, device="cuda")
    prompt = torch.randint(0, 1000, (2, 4), device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        m.beam_search(mel, prompt, 4, 5, eos_token_id=3)         # warm-up outside the check
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out, sc = m.beam_search(mel, prompt, 30, 5, eos_token_id=3)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.shape == (2, 34) and sc.shape == (2,)


def test_graph_replay_reproduces_eager():
    """beam_search(graph=True) against eager beam_search, in its own process (tools/graph_probe_whisper_beam.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_beam.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-400:]
