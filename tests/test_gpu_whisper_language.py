"""GPU checks of language detection: the mopk_language_probs kernel against the torch path on the same device tensors and against
the float64 restatement of tests/test_whisper_language_cpu.py (fp32 and bf16; filtered rows and exact ties; padded row strides, a
column of a cube, an element-aligned base, a padded probs view, given buffers, one row with degenerate strides; bitwise
repeatability; guard bands), detect_language against the op on decode()'s logits and against the CPU path, transcribe with
`languages` against the prompts filled by hand, eagerly here and with graph=True in a process of its own, and no host sync."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from guarded_alloc import embedded, guarded_allocations
from test_whisper_audio_lens_cpu import sdpa_lens_torch
from test_whisper_fallback_cpu import LP_TOL
from test_whisper_language_cpu import (LANGS, MARGIN, SOT, TRANSCRIBE_CASES, check_language_probs, check_transcribe_language_case,
                                       language_cases, language_margins, language_setup)
from test_whisper_transcribe_cpu import V

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 99, 1024)              # one wave short of, at and past a wave; Whisper's 99; every thread's four entries


def _both(ops, x, L, ids, what, **out):
    """the kernel against the restatement, and against the torch path on the same device tensors -> the kernel's result"""
    from mop_amd import _lib
    ops.LAST_PATH.pop("language_probs", None)
    got = ops.language_probs(x, L, **out)
    assert ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED, what
    twin = ops.language_probs_torch(x, L)
    p64 = check_language_probs(got, x, ids, what)
    check_language_probs(twin, x, ids, what)
    assert torch.equal(got.tokens, twin.tokens), what
    assert torch.equal(got.probs == 0, twin.probs == 0), what
    err = (got.probs - twin.probs).abs().double().cpu().numpy() - 2 * LP_TOL * p64      # each within LP_TOL of float64
    assert (err <= 1e-30).all(), (what, float(err.max()))
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("V_", [64, 131, 51865])
def test_kernel_matches_the_torch_path_and_the_restatement(V_, R, dtype):
    from mop_amd import ops
    for n in NS:
        if n > V_:
            continue
        for name, x, ids in language_cases(V_, R, dtype, n, "cuda"):
            what = (V_, R, n, dtype, name)
            assert ids[0] == V_ - 1 and (n == 1 or ids[1] == 0)
            L = ops.LanguageTokens(V_, ids, device="cuda")
            got = _both(ops, x, L, ids, what)
            again = ops.language_probs(x, L)                               # a second run: equal bits
            assert torch.equal(got.probs, again.probs) and torch.equal(got.tokens, again.tokens), what
            if name == "tie":
                assert got.tokens.tolist() == [0] * R, what                # the smaller id, listed second


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V_", [131, 51865])
def test_strides_and_alignment(V_, dtype):
    from mop_amd import _lib, ops
    R, n = 5, 99
    cases = {name: (x, ids) for name, x, ids in language_cases(V_, R, dtype, n, "cuda")}
    ids = cases["plain"][1]
    L = ops.LanguageTokens(V_, ids, device="cuda")
    for name in ("plain", "filtered", "tie"):
        x = cases[name][0]
        plain = _both(ops, x, L, ids, name)
        # an odd padded row stride: rows start at every alignment
        wide = torch.full((R, V_ + 3), 7.0, device="cuda", dtype=dtype)
        wide[:, :V_] = x
        view = wide[:, :V_]
        assert view.stride(0) == V_ + 3
        got = _both(ops, view, L, ids, (name, "padded"))
        assert torch.equal(got.probs, plain.probs) and torch.equal(got.tokens, plain.tokens), name    # the same entries, the same order
        assert bool((wide[:, V_:] == 7.0).all()) and torch.equal(wide[:, :V_], x), name
    x = cases["plain"][0]
    plain = _both(ops, x, L, ids, "plain")
    # a column of a (R, 4, V) cube (what detect_language reads), an odd column with an odd V (bf16: 2 mod 4 bytes)
    cube = torch.randn(R, 4, V_, device="cuda").to(dtype)
    cube[:, 2] = x
    cube[:, 1] = x
    for col in (2, 1):
        assert col != 1 or dtype != torch.bfloat16 or cube[:, 1].data_ptr() % 4 == 2
        got = _both(ops, cube[:, col], L, ids, ("column", col))
        assert torch.equal(got.probs, plain.probs) and torch.equal(got.tokens, plain.tokens)
    # a buffer entered at element 1
    flat = torch.zeros(R * V_ + 1, device="cuda", dtype=dtype)
    off = flat[1:].view(R, V_)
    off.copy_(x)
    assert dtype != torch.bfloat16 or off.data_ptr() % 4 == 2
    got = _both(ops, off, L, ids, "odd base")
    assert torch.equal(got.probs, plain.probs) and torch.equal(got.tokens, plain.tokens)
    # given buffers; probs a view with probs_ld > n, whose padding stays untouched
    big = torch.full((R, n + 5), -7.0, device="cuda")
    bp, bt = big[:, :n], torch.full((R,), -7, dtype=torch.int32, device="cuda")
    assert ops.language_probs_supported(off, L, bp, bt)
    got = _both(ops, off, L, ids, "out buffers", out_probs=bp, out_tokens=bt)
    assert got.probs is bp and got.tokens is bt and torch.equal(bp, plain.probs) and torch.equal(bt, plain.tokens)
    assert bool((big[:, n:] == -7.0).all())
    only = _both(ops, x, L, ids, "out_tokens only", out_tokens=bt.zero_())
    assert only.tokens is bt and torch.equal(bt, plain.tokens) and torch.equal(only.probs, plain.probs)
    # one row with degenerate row strides (never used), for the logits and for probs
    row = x[2].clone()
    for stride0 in (0, 1, 3):
        one = row.as_strided((1, V_), (stride0, 1))
        p1 = torch.full((n + 4,), -7.0, device="cuda")
        got = _both(ops, one, L, ids, ("one row", stride0), out_probs=p1.as_strided((1, n), (stride0, 1)))
        assert torch.equal(got.probs[0], plain.probs[2]) and int(got.tokens) == int(plain.tokens[2]) and bool((p1[n:] == -7.0).all())
    # what the kernel does not take goes to the torch path
    assert not ops.language_probs_supported(x.t().contiguous().t(), L) and not ops.language_probs_supported(x.double(), L)
    assert not ops.language_probs_supported(x, L, torch.empty(n, R, device="cuda").t())
    ops.language_probs(x.double(), L)
    assert ops.LAST_PATH["language_probs"] == _lib.PATH_GENERIC


@pytest.mark.parametrize("n", [99, 1024])
def test_guard_bands_stay_intact(n):
    from mop_amd import _lib, ops
    R, V_, dtype = 3, 51865, torch.bfloat16
    x, ids = next((x, ids) for name, x, ids in language_cases(V_, R, dtype, n, "cuda") if name == "filtered")
    L = ops.LanguageTokens(V_, ids, device="cuda")
    plain = ops.language_probs(x, L)
    G = ops.LanguageTokens(V_, ids)
    G._tables[x.device] = embedded(L.table("cuda"))                        # the id table between guard bytes too
    with guarded_allocations() as ledger:
        bp = torch.empty(R, n, dtype=torch.float32, device="cuda")
        bt = torch.empty(R, dtype=torch.int32, device="cuda")
        xe = embedded(x)
        got = ops.language_probs(xe, G, bp, bt)
        assert ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED
        alloc = ops.language_probs(xe, G)                                  # the op's own result buffers
        assert ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED
    torch.cuda.synchronize()
    assert ledger.count() == 4 and ledger.intact(), ledger.describe_damage()
    for res in (got, alloc):
        assert torch.equal(res.probs, plain.probs) and torch.equal(res.tokens, plain.tokens)
    assert torch.equal(xe, x) and G.table("cuda").tolist() == list(ids)


# ------------------------------------------------------------------ the model
def _cpu_detection(forms):
    """the CPU path on the same weights and inputs, the attention core on its torch composition (undone before any GPU work) ->
    per form (tokens, probs, the float64 top-2 margins of its rows)"""
    from mop_amd import ops
    cm, clips, _, _, cL, W = language_setup(wide=True)
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "sdpa_core", lambda q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p=0.0, seed=None,
                   q_lens=None, kv_lens=None: sdpa_lens_torch(q, k, v, attn_mask, bias, causal, q_lens, kv_lens))
        for form in forms:
            audio = [c[:W] for c in clips] if form == "ragged" else torch.stack([c[:17] for c in clips])
            det = cm.detect_language(audio, SOT, cL)
            with torch.no_grad():
                logits = cm.decode(cm.encode(audio)[0], torch.full((3, 1), SOT))[:, -1]
            out[form] = (det.tokens.tolist(), det.probs.numpy(), language_margins(logits))
    return out


def test_detect_language_equals_the_op_and_the_cpu_path():
    from mop_amd import _lib, ops
    cpu = _cpu_detection(("tensor", "ragged"))
    m, clips, prompt, _, L, W = language_setup("cuda", wide=True)
    first, mel = [c[:W] for c in clips], torch.stack([c[:17] for c in clips])
    for audio, form in ((mel, "tensor"), (first, "ragged")):
        ops.LAST_PATH.pop("language_probs", None)
        got = m.detect_language(audio, prompt[:1], L)
        assert ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED, form
        with torch.no_grad():
            logits = m.decode(m.encode(audio)[0], torch.full((3, 1), SOT, device="cuda"))[:, -1]
        want = ops.language_probs(logits, L)
        assert torch.equal(got.tokens, want.tokens) and torch.equal(got.probs, want.probs), form
        check_language_probs(ops.LanguageProbs(got.probs, got.tokens), logits, LANGS, form)
        # the CPU path: every row's float64 top-2 margin is above MARGIN there (the seed's condition), so the tokens must agree
        tokens, probs, margins = cpu[form]
        assert min(margins) > MARGIN, (form, margins)
        assert got.tokens.tolist() == tokens, (form, margins)
        print(form, "margins", margins, "max |p_gpu - p_cpu|", float(np.abs(got.probs.cpu().numpy() - probs).max()))
    assert len(set(cpu["ragged"][0])) >= 2
    with torch.autocast("cuda", dtype=torch.bfloat16):                     # bf16 logits: a column 2 mod 4 bytes into (B, T_s, V)
        ops.LAST_PATH.pop("language_probs", None)
        got = m.detect_language(first, torch.tensor([SOT, 3], device="cuda"), L)
        assert ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED
        with torch.no_grad():
            logits = m.decode(m.encode(first)[0], torch.tensor([[SOT, 3]] * 3, device="cuda"))[:, -1]
        assert logits.dtype == torch.bfloat16 and logits.data_ptr() % 4 == 2
        want = ops.language_probs(logits, L)
    assert torch.equal(got.tokens, want.tokens) and torch.equal(got.probs, want.probs)


@pytest.mark.parametrize("case", TRANSCRIBE_CASES)
def test_transcribe_with_languages_equals_the_filled_prompts(case):
    from mop_amd import _lib, ops
    from test_whisper_words_cpu import word_rules_by_residue
    m, clips, prompt, rules, L, W = language_setup("cuda", wide=True)
    ops.LAST_PATH.pop("language_probs", None)
    check_transcribe_language_case(case, m, clips, prompt, rules, L, word_rules_by_residue(V, "cuda"), W)
    assert ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED


def test_graph_replay_reproduces_eager():
    """transcribe(languages=..., graph=True), greedy and with 3 beams, against eager and against the prompts filled by hand, in
    a process of its own (tools/graph_probe_whisper_language.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_language.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-800:]


def test_no_host_sync():
    from mop_amd import ops
    V_ = 51865
    x = (torch.randn(8, V_, device="cuda") * 3).to(torch.bfloat16)
    L = ops.LanguageTokens.for_whisper(V_, 50258, 99, device="cuda")
    bp, bt = torch.empty(8, 99, device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda")
    m, clips, prompt, _, ML, _ = language_setup("cuda", wide=True)
    first = torch.stack([c[:17] for c in clips])
    sot = prompt[:1]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ops.language_probs(x, L)
        b = ops.language_probs(x.float(), L, bp, bt)
        c = ops.language_probs_torch(x, L)
        det = m.detect_language(first, sot, ML)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.tokens, c.tokens) and b.probs is bp
    assert bool(((a.probs.sum(1) - 1).abs() < 1e-4).all()) and det.tokens.shape == (3,)
