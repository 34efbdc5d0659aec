"""-m gpu: Whisper's logit rules on the HIP kernel (mopk_logit_rules).  ops.logit_rules against ops.logit_rules_torch on the same
device tensors and against the restatement of tests/test_whisper_rules_cpu.py over its sweep; padded row strides, hist[::K], out
aliasing logits, the device-read position; bitwise reproducibility; generate under rules against a naive re-decode loop (uniform and
ragged prompts); graph replay of all three decoders; the timestamp grammar of their outputs, clips of different lengths included;
the unchanged default; no host sync."""
import os
import subprocess
import sys

import pytest
import torch

from test_whisper_rules_cpu import (NEAR_TIE, SHAPES, T0, assert_rows_match, bits, build_case, check_grammar, histories,
                                    ref_rules, rule_sets)

pytestmark = pytest.mark.gpu


def _both_paths(x, hist, pos, t0, rules, kw, what, out=None):
    """the kernel's result, checked against the torch path on the same tensors (raw bits) and against the restatement, on every
    row outside the near-tie exclusion -> (result, rows left out)"""
    from mop_amd import _lib, ops
    V = x.shape[1]
    src = x.clone()
    ref = ops.logit_rules_torch(src, hist, pos, t0, rules)
    got = ops.logit_rules(x, hist, pos, t0, rules, out=out)
    assert ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED, what
    blocked, margins = ref_rules(src, hist.cpu(), int(pos), t0, V, **kw)
    keep = torch.from_numpy(margins >= NEAR_TIE).cuda()
    assert torch.equal(bits(got)[keep], bits(ref)[keep]), what
    return got, assert_rows_match(got, src, blocked, margins, what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,R", [("v131", 1), ("v131", 3), ("v131", 16), ("v64", 1), ("v64", 3), ("v64", 16), ("v51865", 3)])
def test_kernel_matches_the_torch_path_and_the_restatement(shape, R, dtype):
    from mop_amd import ops
    V, tb, eos = SHAPES[shape]
    rows = left_out = 0
    for ri, (rname, kw) in enumerate(rule_sets(V, tb, eos).items()):
        rules = ops.LogitRules(V, **kw)
        for hi, (hname, g) in enumerate(histories(V, tb, eos).items()):
            if rname in ("k0", "k5") and g:
                continue
            x, hist, pos = build_case(V, tb, eos, R, dtype, g, 1000 * ri + hi, "cuda")
            left_out += _both_paths(x, hist, pos, T0, rules, kw, (shape, rname, hname))[1]
            rows += R
    print(f"{shape} R={R} {dtype}: {left_out} of {rows} rows left out as near ties")
    assert left_out <= 0.02 * rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_strides_aliasing_and_the_device_position(dtype):
    from mop_amd import ops
    V, tb, eos = SHAPES["v51865"]
    kw = rule_sets(V, tb, eos)["full"]
    rules = ops.LogitRules(V, **kw)
    R, K = 5, 3
    g = ["x", tb + 7, tb + 7, "x", tb + 9]
    x, hist, pos = build_case(V, tb, eos, R, dtype, g, 21, "cuda")
    plain, left_out = _both_paths(x, hist, pos, T0, rules, kw, "plain")
    assert left_out == 0
    # a padded row stride (odd: rows start at every alignment) and hist[::K]
    wide = torch.full((R, V + 3), 7.0, device="cuda", dtype=dtype)
    wide[:, :V] = x
    big = torch.full((R * K, hist.shape[1] + 2), -1, device="cuda", dtype=torch.int32)
    big[::K, :hist.shape[1]] = hist
    view, hview = wide[:, :V], big[::K, :hist.shape[1]]
    assert view.stride(0) == V + 3 and hview.stride(0) == K * (hist.shape[1] + 2)
    got, _ = _both_paths(view, hview, pos, T0, rules, kw, "strided")
    assert torch.equal(bits(got), bits(plain))
    # out aliasing logits, in the padded buffer: the padding stays
    same, _ = _both_paths(view, hview, pos, T0, rules, kw, "aliased", out=view)
    assert same.data_ptr() == wide.data_ptr() and torch.equal(bits(wide[:, :V]), bits(plain)) and bool((wide[:, V:] == 7).all())
    # the position is read from the device: the same arguments, another pos
    out = torch.empty_like(x)
    results = {}
    for p in (T0 + len(g), T0 + 2, T0):
        pos.fill_(p)
        _both_paths(x, hist, pos, T0, rules, kw, ("pos", p), out=out)
        results[p] = out.clone()
    assert torch.equal(bits(results[T0 + len(g)]), bits(plain))
    lone = results[T0 + 2]                                   # text, then a lone timestamp tb + 7
    assert bool(torch.isneginf(lone[:, :eos]).all()) and bool(torch.isneginf(lone[:, tb:tb + 7]).all())
    assert not bool(torch.isneginf(lone[:, tb + 7:V - 2]).any())
    assert bool(torch.isneginf(results[T0][:, :tb]).all())
    assert not torch.equal(results[T0], results[T0 + 2]) and not torch.equal(results[T0 + 2], plain)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_single_row_with_degenerate_row_strides(dtype):
    """R = 1: the row strides of logits, out and hist are never used, so any value passes (0 and 1 here, which the kernels would
    refuse for more rows), with the result allocated by the op and with out = logits"""
    from mop_amd import _lib, ops
    V, tb, eos, T = 1027, 900, 890, 8                        # one full pass of the kernel's 1024 threads plus a tail
    kw = rule_sets(V, tb, eos)["full"]
    rules = ops.LogitRules(V, **kw)
    x, hist, pos = build_case(V, tb, eos, 1, dtype, ["x", tb + 3, tb + 3, "x"], 41, "cuda", cap=T)
    assert ref_rules(x, hist.cpu(), int(pos), T0, V, **kw)[1][0] >= NEAR_TIE        # the case itself is no near tie of rule 3e
    for stride in (0, 1):
        view, hview = x.clone().as_strided((1, V), (stride, 1)), hist.as_strided((1, T), (stride, 1))
        ref = ops.logit_rules_torch(view, hview, pos, T0, rules)
        assert bool(torch.isneginf(ref[0, tb:tb + 3]).all()) and not bool(torch.isneginf(ref[0, tb + 4:V - 2]).any())
        got = ops.logit_rules(view, hview, pos, T0, rules)
        print(f"single row, {dtype}, row stride {stride}, out=None: path {ops.LAST_PATH['logit_rules']}")
        assert ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED
        assert got.data_ptr() != view.data_ptr() and got.stride() == (V, 1) and torch.equal(got, ref)
        same = ops.logit_rules(view, hview, pos, T0, rules, out=view)
        print(f"single row, {dtype}, row stride {stride}, out=logits: path {ops.LAST_PATH['logit_rules']}")
        assert ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED
        assert same.data_ptr() == view.data_ptr() and torch.equal(view, ref)


def test_kernel_is_bitwise_reproducible():
    from mop_amd import _lib, ops
    V, tb, eos = SHAPES["v51865"]
    rules = ops.LogitRules(V, **rule_sets(V, tb, eos)["full"])
    for dtype in (torch.float32, torch.bfloat16):
        x, hist, pos = build_case(V, tb, eos, 16, dtype, ["x", tb + 2, tb + 2, "x"], 33, "cuda")
        a = ops.logit_rules(x, hist, pos, T0, rules)
        b = ops.logit_rules(x, hist, pos, T0, rules)
        assert ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED
        assert torch.equal(bits(a), bits(b))
        forced = torch.isneginf(a[:, :tb]).all(1)
        assert 0 < int(forced.sum()) < 16                    # the rows take both outcomes of the dominance rule


TB, EOS = 250, 240
GEN_RULES = dict(suppress_tokens=[1, 2, 100, 249], suppress_at_begin=[5, EOS], timestamp_begin=TB, eos_token_id=EOS,
                 no_timestamps_token_id=248, max_initial_timestamp_index=8)


def _model(d=128, H=2, Ta=200, vocab=300, ctx=64, L=2):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=Ta, vocab_size=vocab, n_text_ctx=ctx, n_embd=d, n_head=H, n_layer_enc=1, n_layer_dec=L)
    m = WhisperMoP(cfg)
    with torch.no_grad():                  # at the default init every logit gap is ~1e-2: widen them so most steps clear 1e-3
        m.dec_ln_f.weight.mul_(20.0)
    return m.cuda().eval()


@torch.no_grad()
def _naive(m, enc_row, prompt_row, n_new, kw):
    """one row alone: full decode, the restatement on the raw last logits, argmax -> (tokens, the first step whose filtered top-2
    gap or dominance margin is below 1e-3 (n_new if none))"""
    cur, P = prompt_row.unsqueeze(0), prompt_row.shape[0]
    for t in range(n_new):
        raw = m.decode(enc_row, cur)[:, -1]
        blocked, margins = ref_rules(raw, cur.cpu(), P + t, P, raw.shape[1], **kw)
        x = raw.double().masked_fill(torch.from_numpy(blocked).cuda(), float("-inf"))
        top = x.topk(2, dim=-1).values[0]
        if float(top[0] - top[1]) < 1e-3 or margins[0] < 1e-3:
            return cur[0], t
        cur = torch.cat([cur, x.argmax(-1, keepdim=True)], dim=1)
    return cur[0], n_new


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_generate_matches_the_naive_loop(ragged):
    from mop_amd import _lib, ops
    m = _model()
    B, n_new = 2, 40
    torch.manual_seed(5)
    mel = torch.randn(B, 200, 12, device="cuda")
    prompts = [torch.randint(0, EOS, (n,), device="cuda") for n in ((4, 2) if ragged else (4, 4))]
    d = m.with_logit_rules(ops.LogitRules(300, **GEN_RULES))
    out, steps = d.generate(mel, prompts if ragged else torch.stack(prompts), n_new, return_logits=True)
    assert ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED
    assert torch.equal(steps.argmax(-1), torch.stack([o[-n_new:] for o in out]))    # the returned logits are the filtered ones
    with torch.no_grad():
        enc, _ = m.encode(mel)
    kinds = set()
    for b in range(B):
        ref, first_close = _naive(m, enc[b:b + 1], prompts[b], n_new, GEN_RULES)
        P = prompts[b].shape[0]
        print(f"row {b}: compared {first_close} of {n_new} steps")
        assert first_close > 0
        assert torch.equal(out[b][:P + first_close], ref[:P + first_close]), b
        check_grammar(out[b][P:].tolist(), GEN_RULES, b)
        kinds |= {"text" if t < TB else "stamp" for t in out[b][P:].tolist()}
    assert kinds == {"text", "stamp"}


def test_graph_replay_reproduces_eager():
    """generate / beam_search (K = 4) / sample (n = 3, temperature 0.7, top_k 20) under rules with graph=True against eager, in a
    process of their own (tools/graph_probe_whisper_rules.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_rules.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-800:]


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])
def test_decoders_obey_the_grammar(mode):
    from mop_amd import _lib, ops
    m = _model()
    torch.manual_seed(6)
    n_new = 40
    d = m.with_logit_rules(ops.LogitRules(300, **GEN_RULES))
    mel = torch.randn(3, 200, 12, device="cuda")
    clips = [mel[0], mel[1, :131], mel[2, :57]]                # clips of different lengths
    prompt = torch.randint(0, EOS, (3, 4), device="cuda")
    kinds = set()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
        for name, audio in (("tensor", mel), ("clips", clips)):
            runs = {"generate": d.generate(audio, prompt, n_new, eos_token_id=EOS)[:, 4:],
                    "beam": d.beam_search(audio, prompt, n_new, 4, eos_token_id=EOS)[0][:, 4:],
                    "sample": d.sample(audio, prompt, n_new, temperature=0.9, top_k=40, num_samples=3, eos_token_id=EOS, seed=2)[0][:, :, 4:]}
            assert ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED
            for run, toks in runs.items():
                for i, row in enumerate(toks.reshape(-1, n_new).tolist()):
                    check_grammar(row, GEN_RULES, (name, run, i))
                    kinds |= {"text" if t < TB else "stamp" for t in row}
    assert kinds == {"text", "stamp"}


def test_default_is_unchanged():
    from mop_amd import ops
    m = _model()
    torch.manual_seed(7)
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, EOS, (2, 4), device="cuda")
    plain = m.with_logit_rules(None)
    ops.LAST_PATH.pop("logit_rules", None)
    assert torch.equal(plain.generate(mel, prompt, 20, eos_token_id=EOS), m.generate(mel, prompt, 20, eos_token_id=EOS))
    a, b = plain.beam_search(mel, prompt, 20, 3, eos_token_id=EOS), m.beam_search(mel, prompt, 20, 3, eos_token_id=EOS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = plain.sample(mel, prompt, 20, 0.8, 10, seed=4), m.sample(mel, prompt, 20, 0.8, 10, seed=4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert "logit_rules" not in ops.LAST_PATH                  # no rules: no launch


def test_no_host_sync():
    from mop_amd import ops
    m = _model()
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, EOS, (2, 4), device="cuda")
    d = m.with_logit_rules(ops.LogitRules(300, **GEN_RULES, device="cuda"))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = d.generate(mel, prompt, 30, eos_token_id=EOS)
            toks, scores = d.beam_search(mel, prompt, 30, 3, eos_token_id=EOS)
            samp, lp = d.sample(mel, prompt, 30, temperature=0.8, top_k=20, num_samples=2, eos_token_id=EOS, seed=1)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.shape == (2, 34) and toks.shape == (2, 34) and samp.shape == (2, 2, 34)
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(lp).all())
