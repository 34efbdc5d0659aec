"""-m gpu: the repetition rules on the HIP kernel (mopk_repeat_rules).  ops.repeat_rules against ops.repeat_rules_torch on the same
device tensors and against the restatement of tests/test_whisper_repeat_cpu.py over its sweep, bit for bit on every row, with a
separate result and in place; long histories (n = 440, n past the kernel's 1024 threads, and the first history that goes to the
torch path); rows shorter than a 16-byte vector at every offset; padded row strides, hist[::K], the device-read position, a
single row with degenerate strides; bitwise reproducibility; guard bands; generate under the rules against a naive re-decode loop
(uniform and ragged prompts); graph replay of all three decoders; no repeated bigram in their outputs, clips of different lengths
included; the unchanged default; no host sync."""
import os
import subprocess
import sys

import pytest
import torch

from guarded_alloc import embedded, guarded_allocations
from test_whisper_repeat_cpu import (T0, assert_bits_equal, build_case, expected, ref_repeat, repeated_bigrams, rules_of, sweep)
from test_whisper_rules_cpu import bits, check_grammar, ref_rules

pytestmark = pytest.mark.gpu


def _both_paths(x, hist, pos, t0, rules, out=None):
    """the kernel's result with a result buffer of its own (or `out`), checked against the torch path on the same tensors and
    against the kernel's in-place result on a copy, all by their raw bits"""
    from mop_amd import _lib, ops
    src = x.clone()
    ref = ops.repeat_rules_torch(src, hist, pos, t0, rules)
    got = ops.repeat_rules(x, hist, pos, t0, rules, out=out)
    assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED
    assert_bits_equal(got, ref, "kernel against the torch path")
    if out is None:
        assert got.data_ptr() != x.data_ptr() and torch.equal(bits(x), bits(src))            # the input is left alone
        same = ops.repeat_rules(src, hist, pos, t0, rules, out=src)
        assert same.data_ptr() == src.data_ptr()
        assert_bits_equal(src, ref, "in place against the torch path")
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,R", [(64, 1), (64, 3), (64, 16), (131, 1), (131, 3), (131, 16), (1027, 3)])
def test_kernel_matches_the_torch_path_and_the_restatement(V, R, dtype):
    seen = sweep(_both_paths, V, R, dtype, "cuda")
    print(f"V={V} R={R} {dtype}: rows banned only / penalised only / both / neither: {seen}")
    assert all(seen)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", range(2, 10))
def test_rows_shorter_than_a_vector_at_every_offset(V, dtype):
    """the copy route on rows with no whole 16-byte vector (csrc/row_helpers.h's RowSpan with nvec == 0, and head clamped to V
    where the row ends before its first boundary): contiguous, and entered 1 ... EPV - 1 elements behind a 16-byte boundary; with
    the result allocated by the op (rows aligned differently once the input is off a boundary) and with an out buffer entered at
    the input's offset (rows aligned alike).  build_case needs V >= 31, so the rows are built here"""
    from mop_amd import ops
    R, es = 3, torch.empty(0, dtype=dtype).element_size()
    rules = ops.RepeatRules(V, 1.3, 2)
    g = torch.Generator().manual_seed(V)
    x = (torch.randn(R, V, generator=g) * 3).to(dtype)
    hist = torch.randint(0, V, (R, T0 + 14), generator=g).to(torch.int32)
    pos = torch.tensor([T0 + 12], dtype=torch.int32)
    want, kinds = expected(x, hist, pos, rules)
    assert all(pen for pen, _ in kinds)
    hist, pos = hist.cuda(), pos.cuda()
    src = torch.zeros(R * V + 16 // es, device="cuda", dtype=dtype)
    for k in range(16 // es):
        dst = torch.zeros_like(src)
        view, out = (buf[k:k + R * V].view(R, V) for buf in (src, dst))
        view.copy_(x)
        assert view.data_ptr() % 16 == k * es and (view.data_ptr() ^ out.data_ptr()) % 16 == 0
        assert_bits_equal(_both_paths(view, hist, pos, T0, rules), want, (V, dtype, k))
        got = _both_paths(view, hist, pos, T0, rules, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert_bits_equal(out, want, (V, dtype, k, "out"))
        assert bool((dst[:k] == 0).all()) and bool((dst[k + R * V:] == 0).all())                  # nothing written beside the rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V,R,n,s", [(51865, 3, 440, 3), (1027, 2, 440, 2), (1027, 2, 2500, 3), (1027, 2, 4096, 5)])
def test_long_histories(V, R, n, s, dtype):
    """n = 440 (a full Whisper window), n past the 1024 threads (a thread then owns several positions) and the longest history
    the kernel takes"""
    rules = rules_of(V, 1.3, s)
    x, hist, pos = build_case(V, R, dtype, n, s, 77, cap=T0 + n + (0 if n == 4096 else 9))
    want, kinds = expected(x, hist, pos, rules)
    assert all(pen for pen, _ in kinds) and any(ban for _, ban in kinds)
    got = _both_paths(x.cuda(), hist.cuda(), pos.cuda(), T0, rules)
    assert_bits_equal(got, want, (V, R, n, s))


def test_a_history_past_the_kernels_limit_takes_the_torch_path():
    from mop_amd import _lib, ops
    V = 131
    rules = rules_of(V, 1.3, 2)
    x, hist, pos = build_case(V, 2, torch.float32, 30, 2, 5, "cuda", cap=T0 + 4097)
    assert not ops.repeat_rules_supported(x, hist, pos, T0, rules) and ops.repeat_rules_supported(x, hist[:, 1:], pos, T0, rules)
    got = ops.repeat_rules(x, hist, pos, T0, rules)
    assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_GENERIC
    assert_bits_equal(got, expected(x.cpu(), hist.cpu(), pos.cpu(), rules)[0], "torch path on the device")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_strides_aliasing_and_the_device_position(dtype):
    V, R, K, n = 1027, 5, 3, 30
    rules = rules_of(V, 1.3, 3)
    x, hist, pos = build_case(V, R, dtype, n, 3, 21, "cuda")
    plain = _both_paths(x, hist, pos, T0, rules)
    assert_bits_equal(plain, expected(x.cpu(), hist.cpu(), pos.cpu(), rules)[0], "plain")
    # a padded row stride (odd: rows start at every alignment) and hist[::K]
    wide = torch.full((R, V + 3), 7.0, device="cuda", dtype=dtype)
    wide[:, :V] = x
    big = torch.full((R * K, hist.shape[1] + 2), -1, device="cuda", dtype=torch.int32)
    big[::K, :hist.shape[1]] = hist
    view, hview = wide[:, :V], big[::K, :hist.shape[1]]
    assert view.stride(0) == V + 3 and hview.stride(0) == K * (hist.shape[1] + 2)
    assert torch.equal(bits(_both_paths(view, hview, pos, T0, rules)), bits(plain))
    # a result buffer with another padded stride: rows aligned differently from their inputs; the padding stays
    res = torch.full((R, V + 6), 9.0, device="cuda", dtype=dtype)
    got = _both_paths(view, hview, pos, T0, rules, out=res[:, :V])
    assert got.data_ptr() == res.data_ptr() and torch.equal(bits(res[:, :V]), bits(plain)) and bool((res[:, V:] == 9).all())
    # out aliasing logits, in the padded buffer: the padding stays
    same = _both_paths(view, hview, pos, T0, rules, out=view)
    assert same.data_ptr() == wide.data_ptr() and torch.equal(bits(wide[:, :V]), bits(plain)) and bool((wide[:, V:] == 7).all())
    # the position is read from the device: the same arguments, three values of pos
    out = torch.empty_like(x)
    results = {}
    for p in (T0 + n, T0 + 12, T0):
        pos.fill_(p)
        _both_paths(x, hist, pos, T0, rules, out=out)
        results[p] = out.clone()
        assert_bits_equal(results[p], expected(x.cpu(), hist.cpu(), pos.cpu(), rules)[0], ("pos", p))
    assert torch.equal(bits(results[T0 + n]), bits(plain)) and torch.equal(bits(results[T0]), bits(x))
    assert not torch.equal(bits(results[T0 + 12]), bits(plain)) and not torch.equal(bits(results[T0 + 12]), bits(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_single_row_with_degenerate_row_strides(dtype):
    """R = 1: the row strides of logits, out and hist are never used, so any value passes (0 and 1 here), with the result
    allocated by the op and with out = logits"""
    from mop_amd import _lib, ops
    V, n = 1027, 30
    rules = rules_of(V, 0.8, 3)
    x, hist, pos = build_case(V, 1, dtype, n, 3, 41, "cuda")
    want = expected(x.cpu(), hist.cpu(), pos.cpu(), rules)[0]
    assert bool((bits(want) != bits(x.cpu())).any())
    for stride in (0, 1):
        view, hview = x.clone().as_strided((1, V), (stride, 1)), hist.as_strided((1, hist.shape[1]), (stride, 1))
        got = ops.repeat_rules(view, hview, pos, T0, rules)
        assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED
        assert got.data_ptr() != view.data_ptr() and got.stride() == (V, 1)
        assert_bits_equal(got, want, ("single row", stride))
        same = ops.repeat_rules(view, hview, pos, T0, rules, out=view)
        assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED and same.data_ptr() == view.data_ptr()
        assert_bits_equal(view, want, ("single row in place", stride))


def test_kernel_is_bitwise_reproducible():
    from mop_amd import _lib, ops
    V = 51865
    rules = rules_of(V, 1.3, 3)
    for dtype in (torch.float32, torch.bfloat16):
        x, hist, pos = build_case(V, 16, dtype, 30, 3, 33, "cuda")
        a = ops.repeat_rules(x, hist, pos, T0, rules)
        b = ops.repeat_rules(x, hist, pos, T0, rules)
        assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED
        assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(x))
        c, d = x.clone(), x.clone()
        ops.repeat_rules(c, hist, pos, T0, rules, out=c)
        ops.repeat_rules(d, hist, pos, T0, rules, out=d)
        assert torch.equal(bits(c), bits(d)) and torch.equal(bits(c), bits(a))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_bands_stay_intact(dtype):
    """the inputs embedded in poison and the result between guard bands: the result is that of the plain run, in place too"""
    from mop_amd import _lib, ops
    V, R = 1027, 3
    rules = rules_of(V, 1.3, 3)
    x, hist, pos = build_case(V, R, dtype, 30, 3, 51, "cuda")
    plain = ops.repeat_rules(x, hist, pos, T0, rules)
    with guarded_allocations() as ledger:
        out = torch.empty(R, V, dtype=dtype, device="cuda")
        xe, he = embedded(x), embedded(hist)
        got = ops.repeat_rules(xe, he, pos, T0, rules, out=out)
        assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED
        work = torch.empty(R, V, dtype=dtype, device="cuda")
        work.copy_(x)
        ops.repeat_rules(work, he, pos, T0, rules, out=work)
    torch.cuda.synchronize()
    assert ledger.count() == 2 and ledger.intact(), ledger.describe_damage()
    assert torch.equal(bits(got), bits(plain)) and torch.equal(bits(work), bits(plain)) and torch.equal(bits(xe), bits(x))


# ------------------------------------------------------------------ the decoders
from test_gpu_whisper_rules import EOS, GEN_RULES, TB, _model  # noqa: E402  (the model with the widened final LayerNorm)

EXEMPT = {EOS} | set(range(TB, 300))


@torch.no_grad()
def _naive(m, enc_row, prompt_row, n_new, kw, rr):
    """one row alone: full decode, the two restatements on the raw last logits (repeat rules first), argmax -> (tokens, the first
    step whose filtered top-2 gap or dominance margin is below 1e-3 (n_new if none))"""
    cur, P = prompt_row.unsqueeze(0), prompt_row.shape[0]
    for t in range(n_new):
        raw = m.decode(enc_row, cur)[:, -1]
        row = ref_repeat(raw[0].float().tolist(), cur[0, P:].tolist(), raw.shape[1], rr.repetition_penalty, rr.inv_penalty,
                         rr.no_repeat_ngram_size, EXEMPT)[0]
        row = torch.tensor([row], dtype=torch.float32)
        blocked, margins = ref_rules(row, cur.cpu(), P + t, P, raw.shape[1], **kw)
        x = row.double().masked_fill(torch.from_numpy(blocked), float("-inf")).cuda()
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
    lr = ops.LogitRules(300, **GEN_RULES)
    rr = ops.RepeatRules.for_whisper(lr, repetition_penalty=1.2, no_repeat_ngram_size=3)
    assert set(rr.table("cpu").nonzero().flatten().tolist()) == EXEMPT
    d = m.with_logit_rules(lr, rr)
    out, steps = d.generate(mel, prompts if ragged else torch.stack(prompts), n_new, return_logits=True)
    assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED and ops.LAST_PATH["logit_rules"] == _lib.PATH_FUSED
    assert torch.equal(steps.argmax(-1), torch.stack([o[-n_new:] for o in out]))    # the returned logits passed both filters
    plain = m.with_logit_rules(lr).generate(mel, prompts if ragged else torch.stack(prompts), n_new)
    assert any(not torch.equal(a, b) for a, b in zip(out, plain))                   # the repeat rules changed the decoding
    with torch.no_grad():
        enc, _ = m.encode(mel)
    for b in range(B):
        ref, first_close = _naive(m, enc[b:b + 1], prompts[b], n_new, GEN_RULES, rr)
        P = prompts[b].shape[0]
        print(f"row {b}: compared {first_close} of {n_new} steps")
        assert first_close > 0
        assert torch.equal(out[b][:P + first_close], ref[:P + first_close]), b
        check_grammar(out[b][P:].tolist(), GEN_RULES, b)


def test_graph_replay_reproduces_eager():
    """generate / beam_search (K = 4) / sample (n = 3, temperature 0.7, top_k 20) under both rule sets with graph=True against
    eager, in a process of their own (tools/graph_probe_whisper_repeat.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_repeat.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-800:]


@pytest.mark.parametrize("mode", ["fp32", "bf16-autocast"])
def test_decoders_emit_no_repeated_bigram(mode):
    from mop_amd import _lib, ops
    m = _model()
    torch.manual_seed(6)
    n_new = 40
    lr = ops.LogitRules(300, **GEN_RULES)
    d = m.with_logit_rules(lr, ops.RepeatRules.for_whisper(lr, no_repeat_ngram_size=2))
    mel = torch.randn(3, 200, 12, device="cuda")
    clips = [mel[0], mel[1, :131], mel[2, :57]]                # clips of different lengths
    prompt = torch.randint(0, EOS, (3, 4), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode != "fp32"):
        loops = [repeated_bigrams(row[4:].tolist(), EXEMPT) for row in m.with_logit_rules(lr).generate(mel, prompt, n_new)]
        print("repeated bigrams without repeat rules:", loops)
        assert any(loops)                                      # without the rules the decoder does repeat itself
        for name, audio in (("tensor", mel), ("clips", clips)):
            runs = {"generate": d.generate(audio, prompt, n_new, eos_token_id=EOS)[:, 4:],
                    "generate-stats": d.generate(audio, prompt, n_new, eos_token_id=EOS, return_stats=True)[0][:, 4:],
                    "beam": d.beam_search(audio, prompt, n_new, 4, eos_token_id=EOS)[0][:, 4:],
                    "sample": d.sample(audio, prompt, n_new, temperature=0.9, top_k=40, num_samples=3, eos_token_id=EOS, seed=2)[0][:, :, 4:]}
            assert ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED
            assert torch.equal(runs["generate"], runs["generate-stats"])
            for run, toks in runs.items():
                for i, row in enumerate(toks.reshape(-1, n_new).tolist()):
                    check_grammar(row, GEN_RULES, (name, run, i))
                    assert not repeated_bigrams(row, EXEMPT), (name, run, i, row)


def test_default_is_unchanged():
    from mop_amd import ops
    m = _model()
    torch.manual_seed(7)
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, EOS, (2, 4), device="cuda")
    lr = ops.LogitRules(300, **GEN_RULES)
    ops.LAST_PATH.pop("repeat_rules", None)
    for rules in (None, lr):
        today = m.with_logit_rules(rules)
        for rr in (None, ops.RepeatRules(300), ops.RepeatRules.for_whisper(lr)):
            d = m.with_logit_rules(rules, rr)
            a, b = d.generate(mel, prompt, 20, eos_token_id=EOS, return_logits=True), today.generate(mel, prompt, 20, eos_token_id=EOS,
                                                                                                 return_logits=True)
            assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))
            a, b = d.beam_search(mel, prompt, 20, 3, eos_token_id=EOS), today.beam_search(mel, prompt, 20, 3, eos_token_id=EOS)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            a, b = d.sample(mel, prompt, 20, 0.8, 10, seed=4), today.sample(mel, prompt, 20, 0.8, 10, seed=4)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert "repeat_rules" not in ops.LAST_PATH                 # no rules, or neutral ones: no launch


def test_no_host_sync():
    from mop_amd import ops
    m = _model()
    mel = torch.randn(2, 200, 12, device="cuda")
    prompt = torch.randint(0, EOS, (2, 4), device="cuda")
    lr = ops.LogitRules(300, **GEN_RULES, device="cuda")
    rr = ops.RepeatRules.for_whisper(lr, 1.2, 3)
    rr.table("cuda")
    for d in (m.with_logit_rules(lr, rr), m.with_logit_rules(None, rr)):
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
