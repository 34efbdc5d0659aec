"""GPU checks of the decoding statistics and of transcribe's temperature fallback and no-speech skip: the mopk_token_logprob and
mopk_greedy_pick kernels against the torch path on the same device tensors and against the float64 restatement of
tests/test_whisper_fallback_cpu.py (fp32 and bf16; filtered rows, done rows, eos picks, exact ties; padded row strides, hist[::K],
one row with degenerate strides; rows shorter than a 16-byte vector at every offset; untouched padding; bitwise repeatability),
generate with statistics against generate without, eagerly here and with graph=True in a process of its own, transcribe's fallback
and skip cases against the naive loop on the device, and no host sync."""
import math
import os
import subprocess
import sys

import pytest
import torch

from test_whisper_fallback_cpu import (LP_TOL, NO_SPEECH, check_fallback_case, check_pick, check_skip_case, fresh_state,
                                       ref_token_logprob, stat_cases)
from test_whisper_transcribe_cpu import EOS, RULES, V

pytestmark = pytest.mark.gpu

VS = (64, 131, 1027, 51865)                    # 64: fewer vectors than threads; 131, 1027: a scalar tail; 51865: Whisper's, several passes


def _pick_both(ops, x, eos, done, what):
    """the kernel against the restatement, and against the torch path on the same device tensors -> the kernel's state"""
    from mop_amd import _lib
    ops.LAST_PATH.pop("greedy_pick", None)
    st = check_pick(ops, ops.greedy_pick, x, eos, done, what, device="cuda")
    assert ops.LAST_PATH["greedy_pick"] == _lib.PATH_FUSED, what
    ref = fresh_state(ops, x.shape[0], 9, eos, done, "cuda")
    ops.greedy_pick_torch(x, ref, torch.tensor([5], dtype=torch.int32, device="cuda"))
    for name in ("next_ids", "done", "n_tokens", "hist"):
        assert torch.equal(getattr(st, name), getattr(ref, name)), (what, name)
    assert (st.sum_logprobs - ref.sum_logprobs).abs().max() <= 2 * LP_TOL, what         # each within LP_TOL of float64
    return st


def _logprob_both(ops, x, toks, what):
    from mop_amd import _lib
    ops.LAST_PATH.pop("token_logprob", None)
    got = ops.token_logprob(x, toks)
    assert ops.LAST_PATH["token_logprob"] == _lib.PATH_FUSED, what
    ref = ops.token_logprob_torch(x, toks)
    want = ref_token_logprob(x, toks.tolist() if isinstance(toks, torch.Tensor) else [toks] * x.shape[0])
    assert got.dtype == torch.float32 and got.shape == (x.shape[0],), what
    for a, r, b in zip(got.tolist(), ref.tolist(), want):
        assert (a == b == r) if math.isinf(b) else (abs(a - b) <= LP_TOL and abs(r - b) <= LP_TOL), (what, a, r, b)
    return got


def _tokens_for(x, name):
    g = torch.Generator().manual_seed(7)
    finite = torch.where(torch.isfinite(x.float().cpu()), 0.0, -1e30) + torch.rand(x.shape, generator=g)
    toks = finite.argmax(1).to(torch.int32)
    if name == "filtered":
        toks[0] = int((~torch.isfinite(x[0].float())).nonzero()[0])        # one whose own entry is -inf
    return toks.cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R", [1, 3, 16])
@pytest.mark.parametrize("V_", VS)
def test_kernels_match_the_torch_path_and_the_restatement(V_, R, dtype):
    from mop_amd import ops
    for name, x, eos, done in stat_cases(V_, R, dtype, "cuda"):
        what = (V_, R, dtype, name)
        st = _pick_both(ops, x, eos, done, what)
        again = _pick_both(ops, x, eos, done, what)                        # a second run: equal bits
        assert torch.equal(st.sum_logprobs, again.sum_logprobs) and torch.equal(st.next_ids, again.next_ids), what
        toks = _tokens_for(x, name)
        got = _logprob_both(ops, x, toks, what)
        assert torch.equal(got, ops.token_logprob(x, toks)), what
        if name == "filtered":
            assert float(got[0]) == float("-inf")
        one = int(toks[-1])
        assert torch.equal(_logprob_both(ops, x, one, what), ops.token_logprob(x, torch.full((R,), one, dtype=torch.int32, device="cuda")))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V_", range(2, 10))
def test_rows_shorter_than_a_vector_at_every_offset(V_, dtype):
    """rows with no whole 16-byte vector (csrc/row_helpers.h's RowSpan with nvec == 0, and head clamped to V where the row ends
    before its first boundary): contiguous, and entered 1 ... EPV - 1 elements behind a 16-byte boundary"""
    from mop_amd import ops
    R, es = 3, torch.empty(0, dtype=dtype).element_size()
    flat = torch.zeros(R * V_ + 16 // es, device="cuda", dtype=dtype)
    for name, x, eos, done in stat_cases(V_, R, dtype, "cuda"):
        kind = name if name != "filtered" or bool(torch.isinf(x[0]).any()) else "all kept"    # four entries can be a whole short row
        toks = _tokens_for(x, kind)
        for k in range(16 // es):
            view = x if k == 0 else flat[k:k + R * V_].view(R, V_).copy_(x)
            assert view.data_ptr() % 16 == k * es
            what = (V_, dtype, name, k)
            _pick_both(ops, view, eos, done, what)
            got = _logprob_both(ops, view, toks, what)
            if kind == "filtered":
                assert float(got[0]) == float("-inf"), what
            _logprob_both(ops, view, int(toks[-1]), what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V_", [131, 1027, 51865])
def test_strides_and_padding(V_, dtype):
    from mop_amd import _lib, ops
    R, K, cap, p = 5, 3, 9, 5
    cases = {n: (x, eos, done) for n, x, eos, done in stat_cases(V_, R, dtype, "cuda")}
    for name in ("plain", "done rows", "tie"):
        x, eos, done = cases[name]
        plain = _pick_both(ops, x, eos, done, name)
        # an odd padded row stride: rows start at every alignment; the state's hist a [::K] view of a wider buffer
        wide = torch.full((R, V_ + 3), 7.0, device="cuda", dtype=dtype)
        wide[:, :V_] = x
        view = wide[:, :V_]
        assert view.stride(0) == V_ + 3
        st = fresh_state(ops, R, cap, eos, done, "cuda")
        big = torch.full((R * K, cap + 2), -9, device="cuda", dtype=torch.int32)
        st.hist = big[::K, :cap]
        st.hist.fill_(-7)
        ops.greedy_pick(view, st, torch.tensor([p], dtype=torch.int32, device="cuda"))
        assert ops.LAST_PATH["greedy_pick"] == _lib.PATH_FUSED
        for f in ("next_ids", "done", "n_tokens"):
            assert torch.equal(getattr(st, f), getattr(plain, f)), (name, f)
        assert torch.equal(st.hist, plain.hist), name
        assert (st.sum_logprobs - plain.sum_logprobs).abs().max() <= 2 * LP_TOL, name       # another alignment: another sum order
        assert bool((wide[:, V_:] == 7.0).all()) and torch.equal(wide[:, :V_], x), name      # the padding and the row: untouched
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[::K, :cap] = False
        assert bool((big[mask] == -9).all()), name
        toks = _tokens_for(x, name)
        assert (_logprob_both(ops, view, toks, name) - ops.token_logprob(x, toks)).abs().max() <= 2 * LP_TOL
    # a column of a (B, T, V) tensor (what no_speech_prob reads)
    x = cases["plain"][0]
    cube = torch.randn(R, 4, V_, device="cuda").to(dtype)
    cube[:, 2] = x
    assert torch.equal(_logprob_both(ops, cube[:, 2], 3, "column"), ops.token_logprob(x, 3))
    # a base address that is element-aligned only: an odd column of a cube with odd V, and a buffer entered at element 1 (in
    # bf16 both are 2 mod 4 bytes); with and without an out buffer
    if V_ % 2:
        cube[:, 1] = x
        assert dtype != torch.bfloat16 or cube[:, 1].data_ptr() % 4 == 2
        assert torch.equal(_logprob_both(ops, cube[:, 1], 3, "odd column"), ops.token_logprob(x, 3))
    flat = torch.zeros(R * V_ + 1, device="cuda", dtype=dtype)
    off = flat[1:].view(R, V_)
    off.copy_(x)
    assert dtype != torch.bfloat16 or off.data_ptr() % 4 == 2
    assert torch.equal(_logprob_both(ops, off, 3, "odd base"), ops.token_logprob(x, 3))
    buf = torch.empty(R, device="cuda")
    assert ops.token_logprob_supported(off, 3, out=buf) and ops.token_logprob(off, 3, out=buf) is buf
    assert ops.LAST_PATH["token_logprob"] == _lib.PATH_FUSED and torch.equal(buf, ops.token_logprob(x, 3))
    toks = _tokens_for(x, "plain")
    assert torch.equal(_logprob_both(ops, off, toks, "odd base, tokens"), ops.token_logprob(x, toks))
    plain = _pick_both(ops, x, cases["plain"][1], cases["plain"][2], "plain again")
    st = _pick_both(ops, off, cases["plain"][1], cases["plain"][2], "odd base pick")
    assert torch.equal(st.next_ids, plain.next_ids)
    # one row with degenerate row strides (never used)
    row = x[2].clone()
    for stride0 in (0, 1, 3):
        one = row.as_strided((1, V_), (stride0, 1))
        st = fresh_state(ops, 1, cap, cases["plain"][1], [0], "cuda")
        st.hist = torch.full((cap,), -7, device="cuda", dtype=torch.int32).as_strided((1, cap), (stride0, 1))
        ops.greedy_pick(one, st, torch.tensor([p], dtype=torch.int32, device="cuda"))
        assert ops.LAST_PATH["greedy_pick"] == _lib.PATH_FUSED
        assert int(st.next_ids) == int(row.float().argmax()) == int(st.hist[0, p]), stride0
        _logprob_both(ops, one, 5, ("one row", stride0))
    # a device position outside the history writes no column; a device token outside the row is clamped into it
    st = fresh_state(ops, R, cap, None, [0] * R, "cuda")
    ops.greedy_pick(x, st, torch.tensor([cap], dtype=torch.int32, device="cuda"))
    assert bool((st.hist == -7).all()) and st.n_tokens.tolist() == [r + 3 for r in range(R)]
    far = torch.tensor([-4, V_, 2 ** 31 - 1, 0, V_ - 1], dtype=torch.int32, device="cuda")
    assert torch.equal(ops.token_logprob(x, far), ops.token_logprob(x, far.clamp(0, V_ - 1)))
    # what the kernels do not take goes to the torch path
    assert not ops.token_logprob_supported(x.t().contiguous().t(), 1) and not ops.greedy_pick_supported(x.double(), st, far[:1])
    assert not ops.token_logprob_supported(x, far.long())


def _model(vocab=V):
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=64, vocab_size=vocab, n_text_ctx=64, n_embd=128, n_head=2, n_layer_enc=1, n_layer_dec=2)
    m = WhisperMoP(cfg)
    with torch.no_grad():                      # at the default init every logit gap is ~1e-2: widen them
        m.dec_ln_f.weight.mul_(20.0)
    return m.cuda().eval()


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16"])
def test_generate_with_statistics_equals_generate(autocast):
    from mop_amd import _lib, ops
    m = _model()
    torch.manual_seed(2)
    mel = torch.randn(3, 64, 12, device="cuda")
    prompt = torch.tensor([[7, 8, 9]] * 3, device="cuda")
    ragged = [prompt[0], prompt[1, :1], prompt[2, :2]]
    rules = ops.LogitRules(V, **RULES)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        for d, eos in ((m.with_logit_rules(None), None), (m.with_logit_rules(rules), EOS)):
            if eos is None:
                eos = int(d.generate(mel, prompt, 20)[0, -9])              # an eos the plain run meets
            for p in (prompt, ragged):
                plain, logits = d.generate(mel, p, 20, eos, return_logits=True)
                ops.LAST_PATH.clear()
                got, got_logits, st = d.generate(mel, p, 20, eos, return_logits=True, return_stats=True,
                                                 no_speech_token_id=NO_SPEECH)
                assert ops.LAST_PATH["greedy_pick"] == _lib.PATH_FUSED and ops.LAST_PATH["token_logprob"] == _lib.PATH_FUSED
                if p is prompt:                # sot_index 1 at the odd V: under autocast a bf16 column 2 mod 4 bytes into the logits
                    ops.LAST_PATH.clear()
                    st1 = d.generate(mel, p, 20, eos, return_stats=True, no_speech_token_id=NO_SPEECH, sot_index=1)[-1]
                    assert ops.LAST_PATH["token_logprob"] == _lib.PATH_FUSED, autocast
                    cache = m.init_decode_cache(m.encode(mel)[0], 23)      # the prompt pass generate runs: the same logits
                    want = torch.softmax(m.decode_step(cache, p)[:, 1].double(), -1)[:, NO_SPEECH]
                    assert torch.allclose(st1.no_speech_prob.double(), want, rtol=1e-4, atol=0), autocast   # LP_TOL in the log
                assert all(torch.equal(a, b) for a, b in zip(got, plain)) and torch.equal(got_logits, logits)
                rows = [r.tolist() for r in got]
                T_p = [len(r) - 20 for r in rows]
                lp = torch.log_softmax(logits.double(), -1).cpu()
                for b, r in enumerate(rows):
                    gen = r[T_p[b]:]
                    n = gen.index(eos) + 1 if eos in gen else 20
                    want = sum(float(lp[b, t, gen[t]]) for t in range(n))
                    assert int(st.n_tokens[b]) == n
                    assert abs(float(st.sum_logprobs[b]) - want) <= 1e-4 * max(1.0, abs(want)), (b, want)
                assert st.no_speech_prob.shape == (3,) and bool(((st.no_speech_prob > 0) & (st.no_speech_prob < 1)).all())


def test_graph_replay_reproduces_eager():
    """generate(return_stats=True, graph=True) -- the decoder step, logit_rules and greedy_pick captured and replayed -- against
    eager and against generate() without statistics, in a process of its own (tools/graph_probe_whisper_stats.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_stats.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-800:]


def _policy_setup():
    from mop_amd import ops
    m = _model()
    torch.manual_seed(4)
    clips = [torch.randn(n, 12, device="cuda") for n in (200, 150, 140)]  # four, three and three windows of 64 frames
    return m, clips, torch.tensor([7, 8, 9], device="cuda"), ops.LogitRules(V, **RULES, device="cuda")


def test_transcribe_fallback_equals_the_naive_loop():
    log = check_fallback_case(*_policy_setup(), window=64)
    print("temperatures kept:", [g.temperature for g in log])


def test_transcribe_skip_equals_the_naive_loop():
    log = check_skip_case(*_policy_setup(), window=64)
    print("skipped:", [g.skipped for g in log])


def test_no_host_sync():
    from mop_amd import ops
    x = (torch.randn(16, 51865, device="cuda") * 3).to(torch.bfloat16)
    st = ops.GreedyState(16, 8, 11, with_hist=True, device="cuda")
    pos = torch.tensor([3], dtype=torch.int32, device="cuda")
    toks = torch.arange(16, dtype=torch.int32, device="cuda")
    m = _model()
    mel = torch.randn(2, 64, 12, device="cuda")
    prompt = torch.tensor([[7, 8, 9]] * 2, device="cuda")
    d = m.with_logit_rules(ops.LogitRules(V, **RULES, device="cuda"))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.greedy_pick(x, st, pos)
        lp = ops.token_logprob(x, toks)
        lp1 = ops.token_logprob(x, 7)
        out, stats = d.generate(mel, prompt, 12, EOS, return_stats=True, no_speech_token_id=NO_SPEECH)
        _, _, bstats = d.beam_search(mel, prompt, 12, 3, EOS, return_stats=True, no_speech_token_id=NO_SPEECH)
        _, _, sstats = d.sample(mel, prompt, 12, num_samples=2, eos_token_id=EOS, return_stats=True, no_speech_token_id=NO_SPEECH)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lp1).all()) and st.n_tokens.tolist() == [1] * 16
    assert out.shape == (2, 15) and stats.n_tokens.shape == bstats.n_tokens.shape == (2,) and sstats.n_tokens.shape == (2, 2)
