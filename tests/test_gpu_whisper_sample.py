"""-m gpu: temperature / top-k / top-p sampling (mopk_sample_*, ops.sample_tokens, WhisperMoP.sample).  The kernel against
sample_tokens_torch at V = 51865 and odd V, fp32 and bf16, rows off a 16-byte boundary (tokens equal except where the torch path's two
best perturbed scores nearly tie; every token inside the float64 kept set; log-probabilities against log_softmax); draw frequencies
against the filtered softmax by a chi-square test; sample against generate at temperature 0 and top_k = 1; reproducibility and seed /
sample-index dependence; eos pinning and sum_logprobs against a teacher-forced decode; no host sync; graph replay."""
import os
import subprocess
import sys

import pytest
import torch

from sample_rows import _perturbed, _z
from test_gpu_whisper_beam import _model

pytestmark = pytest.mark.gpu
NEG = float("-inf")
CHI2_1E6 = [23.93, 27.63, 30.66, 33.38, 35.89, 38.26, 40.52, 42.7, 44.81, 46.86, 48.87]     # chi2.isf(1e-6, df), df = 1 .. 11


def _kept64(x, temperature, top_k, top_p):
    """the kept set in float64 with top_p + 1e-6 (the largest set a rounding of the masses can give)"""
    z = _z(x, temperature).double()
    keep = torch.ones_like(z, dtype=torch.bool)
    if 0 < top_k < z.shape[1]:
        keep = z >= z.topk(top_k, dim=-1).values[:, -1:]
    if top_p < 1:
        p = torch.where(keep, torch.exp(z - z.max(-1, keepdim=True).values), 0.0)
        p = p / p.sum(-1, keepdim=True)
        zs, o = torch.sort(torch.where(keep, z, NEG), dim=-1, descending=True, stable=True)
        first = (p.gather(-1, o).cumsum(-1) >= min(1.0, top_p + 1e-6) - 1e-12).to(torch.int8).argmax(-1, keepdim=True)
        keep = keep & (z >= zs.gather(-1, first))
    return keep


@pytest.mark.parametrize("V", [51865, 1001, 37, 2])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kernel_matches_the_torch_path(V, dtype):
    from mop_amd import _lib, ops
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(V)
    R = 64
    buf = (torch.randn(R, V + 3, device="cuda", generator=g) * 2.5).to(dt)
    x = buf[:, 1:V + 1]                                   # rows off a 16-byte boundary, row stride V + 3
    if V > 8:
        x[5, : V // 3] = NEG                              # -inf entries
        x[6, 1] = x[6, 4] = x[6].max()                    # a tied maximum
    for pos, (T, k, p) in enumerate([(1.0, 0, 1.0), (0.7, 50, 0.95), (1.3, 0, 0.9), (0.5, 5, 1.0), (2.0, 1000, 0.5), (0.0, 0, 1.0),
                                     (1.0, 1, 1.0), (0.9, 3, 0.3)]):
        pos_t = torch.tensor([17 + pos], dtype=torch.int32, device="cuda")
        tok, lp = ops.sample_tokens(x, pos_t, T, k, p, seed=1234 + pos)
        assert ops.LAST_PATH["sample"] == _lib.PATH_FUSED
        tt, tl = ops.sample_tokens_torch(x, pos_t, T, k, p, seed=1234 + pos)
        ref_lp = torch.log_softmax(x.float(), -1).gather(1, tok.long().unsqueeze(1)).squeeze(1)
        assert (lp - ref_lp).abs().max() <= 1e-5, (T, k, p)
        if T == 0:
            assert torch.equal(tok.long(), x.float().argmax(-1)) and torch.equal(tok, tt)
            continue
        keep = _kept64(x, T, k, p)
        assert keep.gather(1, tok.long().unsqueeze(1)).all(), (T, k, p)
        sc = torch.where(keep, _perturbed(x, 17 + pos, T, 1234 + pos), NEG)
        top2 = sc.topk(min(2, V), dim=-1).values
        near = (top2[:, 0] - top2[:, -1]).abs() <= 1e-5 * top2[:, 0].abs().clamp_min(1.0)
        differ = tok != tt
        assert not (differ & ~near).any(), (T, k, p, differ.nonzero().flatten().tolist())
        assert int(differ.sum()) <= 2


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.5, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.8), (1.5, 6, 0.7), (0.8, 12, 0.999)])
def test_draw_frequencies_follow_the_filtered_softmax(T, k, p):
    from mop_amd import ops
    x = torch.tensor([[1.2, 0.3, -0.5, 2.0, 1.2, 0.0, -1.0, 0.7, 1.9, -2.0, 0.5, 1.0]], device="cuda")
    R, P = 4096, 32
    counts = torch.zeros(12, dtype=torch.float64, device="cuda")
    out = (torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, device="cuda"))
    for pos in range(P):
        tok, _ = ops.sample_tokens(x, torch.tensor([pos], dtype=torch.int32, device="cuda"), T, k, p, seed=99, out=out)
        counts += torch.bincount(tok.long(), minlength=12).double()
    keep = _kept64(x, T, k, p)[0]
    assert counts[~keep].sum() == 0                       # filtered tokens never appear
    z = _z(x, T).double()[0]
    prob = torch.where(keep, torch.exp(z - z.max()), 0.0)
    prob = prob / prob.sum()
    n = R * P
    exp = prob[keep] * n
    chi2 = float(((counts[keep] - exp) ** 2 / exp).sum())
    df = int(keep.sum()) - 1
    if df >= 1:
        assert chi2 < CHI2_1E6[df - 1], (chi2, df)


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])
def test_temperature_zero_and_top_k_one_equal_generate(mode):
    m = _model(widen=10.0)
    mel = torch.randn(3, 200, 12, device="cuda")
    prompt = torch.randint(0, 300, (3, 4), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
        greedy = m.generate(mel, prompt, 40)
        tok, _ = m.sample(mel, prompt, 40, temperature=0.0, num_samples=2)
        assert torch.equal(tok[:, 0], greedy) and torch.equal(tok[:, 1], greedy)
        eos = int(greedy[0, 10])
        tok, _ = m.sample(mel, prompt, 40, temperature=0.0, eos_token_id=eos)
        assert torch.equal(tok[:, 0], m.generate(mel, prompt, 40, eos_token_id=eos))
        if mode == "fp32":                                # under bf16, ties at the maximum are likely and top-k keeps them all
            tok, _ = m.sample(mel, prompt, 40, temperature=1.7, top_k=1, num_samples=3, seed=5)
            assert all(torch.equal(tok[:, s], greedy) for s in range(3))


def test_reproducible_and_seeded():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(2, 300, 12, device="cuda")
    prompt = torch.randint(0, 1000, (2, 4), device="cuda")
    cfg = dict(temperature=1.0, top_k=100, top_p=0.95, num_samples=4)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a, sa = m.sample(mel, prompt, 50, seed=3, **cfg)
        b, sb = m.sample(mel, prompt, 50, seed=3, **cfg)
        c, _ = m.sample(mel, prompt, 50, seed=4, **cfg)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert not torch.equal(a, c)
    assert not torch.equal(a[:, 0], a[:, 1]) and not torch.equal(a[:, 1], a[:, 2])      # samples of an item differ
    assert torch.equal(a[:, :, :4], prompt.unsqueeze(1).expand(2, 4, 4))


def test_eos_pinning_and_sum_logprobs_match_a_teacher_forced_decode():
    m = _model(widen=2.0)
    torch.manual_seed(8)
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, 300, (2, 3), device="cuda")
    tok0, _ = m.sample(mel, prompt, 30, temperature=0.9, top_k=40, num_samples=3, seed=11)
    eos = int(tok0[0, 1, 3 + 4])
    tok, slp = m.sample(mel, prompt, 30, temperature=0.9, top_k=40, num_samples=3, seed=11, eos_token_id=eos)
    enc, _ = m.encode(mel)
    hit = 0
    for b in range(2):
        for s in range(3):
            seq = tok[b, s]
            gen = seq[3:]
            at = (gen == eos).nonzero()
            end = int(at[0]) + 1 if len(at) else 30
            assert (gen[end:] == eos).all()
            hit += end < 30
            with torch.no_grad():
                lp = torch.log_softmax(m.decode(enc[b:b + 1], seq[:-1].unsqueeze(0)).float(), -1)[0, 2:]
            want = float(lp[:end].gather(1, gen[:end].unsqueeze(1)).sum())
            assert abs(float(slp[b, s]) - want) <= 1e-4 * max(1.0, abs(want)), (b, s)
    assert hit >= 1
    assert torch.equal(tok[0, 1, :3 + 5], tok0[0, 1, :3 + 5])      # the rows agree with the eos-free run up to the eos


def test_no_host_sync():
    m = _model(d=256, H=4, Ta=300, vocab=1000, ctx=96)
    mel = torch.randn(2, 300, 12, device="cuda")
    prompt = torch.randint(0, 1000, (2, 4), device="cuda")
    cfg = dict(temperature=0.7, top_k=50, top_p=0.95, num_samples=3, eos_token_id=3)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        m.sample(mel, prompt, 4, **cfg)                          # warm-up outside the check
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out, sc = m.sample(mel, prompt, 30, **cfg)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.shape == (2, 3, 34) and sc.shape == (2, 3)


def test_graph_replay_reproduces_eager():
    """sample(graph=True) against eager sample, in its own process (tools/graph_probe_whisper_sample.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_sample.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-400:]
