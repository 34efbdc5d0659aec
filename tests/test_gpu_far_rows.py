"""-m gpu: every export family on operands whose rows lie more than 2^32 bytes apart (tests/far_rows.py).

The other GPU tests hand the kernels tensors of a few kilobytes, so no element offset in them reaches 2^31.  The C ABI carries
every stride as int64_t and the kernels form `index * stride` by hand; here each case gives a kernel views with a leading (batch
or row) stride of FAR_STRIDE = 2^31 + 2^16 elements out of one 8 GiB + 64 MiB buffer of the sentinel byte: bf16 with 3 rows (row 1
past 2^31 elements and 2^32 bytes, row 2 past 2^32 elements), fp32 / int32 with 2 rows (row 1 past 2^31 elements and 8 GiB).

Every case runs the op twice, on far views and on compact clones of the same values, and asserts

  1. the far result against the op's float64 reference under the bound of the op's own test file (imported, named at each case;
     nothing here has a tolerance of its own);
  2. the far result torch.equal to the compact one, every output and gradient, parameter gradients included (same grid, same
     order; each row keeps the 16-byte phase of its compact twin) -- or, where the case says why not, oracle 1 alone;
  3. ops.LAST_PATH: the intended path;
  4. the struct the kernel was launched with: ops._launch / ops._core_launch are wrapped, and the stride fields named by the
     case must equal FAR_STRIDE in the far run (and must not in the compact run), so a wrapper that copied the input is caught;
     where an ops wrapper copies by design the export is driven through the C ABI;
  5. FarBuffer.check_guards(): the 1 MiB on either side of every row still holds the sentinel.

The last test scans the whole buffer: the sentinel everywhere outside the rows handed out.

The attention subjects are those of test_gpu_attn_layouts.py, built at B = 3 (bf16) / 2 (fp32 io), H = 2, N = 130, with their
references and bounds.

Families: the sdpa, quartet (use_quartet on and off, plain and lens=), dualpath and crossview cores, edgewise_lowrank_core and
edgewise_general_core (fused and generic; the struct edited on its way into the library, since the wrappers make qkv
contiguous), the four decode ops, token_logprob, greedy_pick, logit_rules, repeat_rules, sample and sample_ragged,
language_probs, beam_step, cross_entropy (through ops and through the C ABI), token_gate_1d (plain and lens=), the gated
residual, mel_gate, the LayerNorm kernels (C ABI), log_mel, resample, alignment_cost, dtw_align, timestamp_segments, the
prompt-history update, window_prompts, alignment_rows and word_spans.  Every family is bit-equal to its compact twin.

Out of scope: the MoE kernels (contiguous operands only; their M * max(D, F) < 2^31 refusal is pinned in test_moe_cpu.py) and the
generic path's (B*H, N, N) maps past 2^31 elements, which would need tens of GB (test_far_rows_cpu.py covers their sizes).
"""
import ctypes as C
import math
import time

import pytest
import torch

import ce_rows as CR
import far_rows as FR
import test_gpu_attn_layouts as LAY

pytestmark = pytest.mark.gpu
FAR = FR.FAR_STRIDE
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
FUSED, GENERIC = 2, 1


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def far_buffer():
    t0 = time.time()
    fb = FR.FarBuffer.on_device()
    torch.cuda.synchronize()
    print(f"\nFIG far buffer: {fb.nbytes / 2 ** 30:.3f} GiB filled in {time.time() - t0:.2f} s")
    yield fb
    del fb.buf
    torch.cuda.empty_cache()


@pytest.fixture
def fb(far_buffer):
    assert not far_buffer.live
    yield far_buffer
    torch.cuda.synchronize()
    far_buffer.release()


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


class _Seen(list):
    hook = None


@pytest.fixture
def launches(monkeypatch):
    """[(symbol or "core:<core>", a copy of the args struct as it was launched)] of every ops._launch / ops._core_launch"""
    from mop_amd import ops
    seen = _Seen()
    real_launch, real_core = ops._launch, ops._core_launch

    def launch(sym, a, key=None):
        if seen.hook is not None:
            seen.hook(sym, a)                          # may edit the struct the library is about to get (the C ABI driven by hand)
        seen.append((sym, type(a).from_buffer_copy(a)))
        return real_launch(sym, a, key)

    def core_launch(core, a, dev, saved=None):
        out = real_core(core, a, dev, saved)
        seen.append(("core:" + core, type(a).from_buffer_copy(a)))
        return out
    monkeypatch.setattr(ops, "_launch", launch)
    monkeypatch.setattr(ops, "_core_launch", core_launch)
    return seen


_MISSING = object()


def _field(a, path):
    """the field `path` ("q.sb", "logits_ld") of the struct, or of the struct it wraps as .base; _MISSING if it has none"""
    for root in (a, getattr(a, "base", None)):
        obj = root
        for p in path.split("."):
            obj = getattr(obj, p, _MISSING) if obj is not None else _MISSING
            if obj is _MISSING:
                break
        if obj is not _MISSING:
            return obj
    return _MISSING


def strides_seen(seen, fields):
    """{field: the values it had over the launches whose struct has it}; "symbol:field" looks at the launches of that symbol only"""
    out = {f: [] for f in fields}
    for sym, a in seen:
        for f in fields:
            only, _, name = f.rpartition(":")
            v = _field(a, name) if only in ("", sym) else _MISSING
            if v is not _MISSING:
                out[f].append(int(v))
    return out


def assert_far_strides(seen, fields, what, stride=FAR):
    got = strides_seen(seen, fields)
    for f in fields:
        assert got[f], f"{what}: no launch carried a struct with the field {f} ({[s for s, _ in seen]})"
        assert all(v == stride for v in got[f]), f"{what}: {f} = {got[f]} in the launched structs, the far stride is {stride}"


def assert_compact_strides(seen, fields, what):
    got = strides_seen(seen, fields)
    for f in fields:
        assert got[f] and all(abs(v) < 2 ** 31 for v in got[f]), f"{what}: the compact run's {f} = {got[f]}"


def same(got, want, what):
    """bit for bit, dtype and shape included (None: the run has no such result)"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for n in sorted(want):
        g, w = got[n], want[n]
        if g is None or w is None:
            assert g is None and w is None, (what, n)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {n} is {g.dtype} {tuple(g.shape)}, the compact run's {w.dtype} {tuple(w.shape)}"
        assert torch.equal(g, w), (f"{what}: {n} of the far run differs from the compact run in {int((g != w).sum())} value(s), "
                                   f"max |diff| {float((g.double() - w.double()).abs().max()):.3e}")


def compact_like(t):
    """a clone of t laid out as a far view is, with a small leading stride: every row on a 256-byte boundary (contiguous where
    a row's bytes are a multiple of 256, as the attention operands' are), so each row has the 16-byte phase of its far twin"""
    isz = t.element_size()
    row = math.prod(t.shape[1:])
    ld = (row * isz + FR.ALIGN - 1) // FR.ALIGN * FR.ALIGN // isz
    if t.dim() < 2 or ld == row:
        return t.detach().clone(memory_format=torch.contiguous_format)
    buf = torch.empty(t.shape[0], ld, dtype=t.dtype, device=t.device)
    buf.view(torch.uint8).fill_(FR.SENTINEL)
    out = buf[:, :row].view(t.shape)
    out.copy_(t.detach())
    return out


def far_vs_compact(fb, launches, run, fields, what, check=None, paths=None, bitwise=True):
    """run(put) -> {name: tensor}: the op on operands made by put(tensor) -- a far view holding the tensor's values, then a compact
    clone.  Oracles 3, 4, 5 on the far run, 1 through check(result), 2 through same() unless bitwise is False."""
    from mop_amd import ops
    for k in paths or {}:
        ops.LAST_PATH.pop(k, None)
    del launches[:]
    far = run(fb.far_like)
    torch.cuda.synchronize()
    took = {k: ops.LAST_PATH.get(k) for k in paths or {}}
    assert took == (paths or {}), f"{what}: the far run took {took}, intended {paths}"
    assert_far_strides(launches, fields, what)
    fb.check_guards()
    del launches[:]
    compact = run(compact_like)
    torch.cuda.synchronize()
    assert {k: ops.LAST_PATH.get(k) for k in paths or {}} == took, what
    assert_compact_strides(launches, fields, what)
    if check is not None:
        check(far)
    if bitwise:
        same(far, compact, what)
    return far, compact


def _rows(dtype):
    return FR.far_rows(dtype)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ attention cores
# The subjects of test_gpu_attn_layouts.py (values, call, float64 check under the core's own bounds, expected path), built by that
# file's builders at this file's extents: its module-level B, H, N are set for the duration of a test, since the builders and the
# checks they return read them when they run.  q, k, v (and the second pair) are far along B; the outputs and gradients an ops
# wrapper allocates itself are compact by design.
ATTN = {
    # name: (builder, its arguments after the name, far fields)
    "sdpa-fused-causal-bf16-dk64": ("_sdpa", (130, 64, BF16, "bf16", "causal"), ("q.sb", "k.sb", "v.sb")),
    "sdpa-fused-rect-bf16-dk32": ("_sdpa", (LAY.NK, 32, BF16, "bf16", "plain"), ("q.sb", "k.sb", "v.sb")),
    "sdpa-fused-lens-fp32io-dk64": ("_sdpa", (LAY.NK, 64, F32, "bf16", "lens"), ("q.sb", "k.sb", "v.sb")),
    "sdpa-generic-causal-fp32-dk32": ("_sdpa", (130, 32, F32, "fp32", "causal"), ("q.sb", "k.sb", "v.sb")),
    "sdpa-generic-rect-fp32-dk64": ("_sdpa", (LAY.NK, 64, F32, "fp32", "plain"), ("q.sb", "k.sb", "v.sb")),
    "sdpa-generic-lens-fp32-dk32": ("_sdpa", (LAY.NK, 32, F32, "fp32", "lens"), ("q.sb", "k.sb", "v.sb")),
    "quartet-fused-bf16-dk64": ("_quartet", (64, BF16, False, False), ("q.sb", "k.sb", "v.sb", "q2.sb", "k2.sb")),
    "quartet-fused-fp32io-dk32": ("_quartet", (32, F32, False, False), ("q.sb", "k.sb", "v.sb", "q2.sb", "k2.sb")),
    "quartet-generic-weights-bf16-dk32": ("_quartet", (32, BF16, True, False), ("q.sb", "k.sb", "v.sb", "q2.sb", "k2.sb")),
    "dualpath-fused-bf16-dk64": ("_dualpath", (64, BF16, 0.0, False), ("q1.sb", "k1.sb", "v1.sb", "q2.sb", "k2.sb", "v2.sb")),
    "dualpath-fused-causal-fp32io-dk32": ("_dualpath", (32, F32, 0.0, True), ("q1.sb", "k1.sb", "v1.sb", "q2.sb", "k2.sb", "v2.sb")),
    "dualpath-generic-chain-bf16-dk64": ("_dualpath", (64, BF16, 0.5, False), ("q1.sb", "k1.sb", "v1.sb", "q2.sb", "k2.sb", "v2.sb")),
    "crossview-prior-bf16-dk40": ("_crossview", (), ("q1.sb", "k1.sb", "v1.sb", "q2.sb", "k2.sb")),
    "decode-bf16-dk64-tq1": ("_decode", ("decode_attention", 3, 1, 64, BF16, False), ("q.sb", "k.sb", "v.sb")),
    "decode-causal-fp32-dk128-tq3": ("_decode", ("decode_attention", 2, 3, 128, F32, True), ("q.sb", "k.sb", "v.sb")),
    "decode-ragged-causal-fp32-dk128-tq3": ("_decode", ("decode_attention_ragged", 2, 3, 128, F32, True), ("q.sb", "k.sb", "v.sb")),
    "decode-ragged-bf16-dk64-tq1": ("_decode", ("decode_attention_ragged", 2, 1, 64, BF16, False), ("q.sb", "k.sb", "v.sb")),
    "decode-lens-bf16-dk64-tq1": ("_decode", ("decode_attention_lens", 2, 1, 64, BF16, False), ("q.sb", "k.sb", "v.sb")),
    "decode-lens-fp32-dk128-tq3": ("_decode", ("decode_attention_lens", 2, 3, 128, F32, False), ("q.sb", "k.sb", "v.sb")),
}


def _attn_dtype(args):
    return next(a for a in args if isinstance(a, torch.dtype)) if args else BF16


@pytest.mark.parametrize("name", list(ATTN))
def test_attention_cores_and_decode(name, fb, launches, monkeypatch):
    builder, args, fields = ATTN[name]
    dt = _attn_dtype(args)
    monkeypatch.setattr(LAY, "B", 2 if "lens" in name else _rows(dt))       # the builders' length vectors have two entries
    monkeypatch.setattr(LAY, "H", 2)
    monkeypatch.setattr(LAY, "N", 130)
    s = getattr(LAY, builder)(name, *args)
    assert all(v.shape[0] == (LAY.B if not name.startswith("decode") else args[1]) for v in s.vals.values())
    want = FUSED if ("-fused-" in name or name.startswith("decode-")) else GENERIC

    def run(put):
        views = {n: put(s.vals[n]).requires_grad_(s.grad) for n in s.names}
        assert s.expect(views) == want, name                     # from the alignment rule, before anything runs
        res, paths = LAY.run(s, views)
        assert paths == {k: want for k in s.keys}, f"{name}: took {paths}"
        LAY.finite(res, name)
        return res
    far_vs_compact(fb, launches, run, fields, name, check=s.check)


def test_lens_forms_on_three_bf16_rows(fb, launches):
    """the builders of test_gpu_attn_layouts.py give their length vectors two entries, which holds the lens subjects above to B = 2;
    here sdpa_core with q_lens / kv_lens, decode_attention_ragged and decode_attention_lens run on three bf16 rows, so row 2 lies
    past 2^32 elements.  References and bounds: attn_ref.sdpa_ref64 under test_gpu_attn_layouts._close, and _decode_ref64 under
    DECODE_TOL."""
    import mop_amd
    from mop_amd import ops
    B, N, NK, H, dk = 3, 130, LAY.NK, 2, 64
    g = LAY._gen("far-sdpa-lens-bf16-three-rows")
    vals = {n: LAY._rand((B, m, H, dk), g, BF16) for n, m in (("q", N), ("k", NK), ("v", NK))}
    dy = LAY._rand((B, N, H * dk), g, BF16)
    q_lens = torch.tensor([N, 67, 1], dtype=I32, device="cuda")
    kv_lens = torch.tensor([NK - 5, 33, 64], dtype=I32, device="cuda")
    mask = ops.sdpa_lens_mask(q_lens, kv_lens, B, N, NK, "cuda")

    def run(put):
        mop_amd.set_precision("bf16")
        t = {n: put(v).requires_grad_() for n, v in vals.items()}
        y = ops.sdpa_core(t["q"], t["k"], t["v"], q_lens=q_lens, kv_lens=kv_lens)
        y.backward(dy)
        return {"y": y.detach(), "dq": t["q"].grad, "dk": t["k"].grad, "dv": t["v"].grad}

    def check(res):
        r = [vals[n].detach().double().requires_grad_(True) for n in "qkv"]
        yr = LAY.sdpa_ref64(*r, mask=mask)
        (yr * dy.double()).sum().backward()
        LAY._close(LAY._np(res["y"]), LAY._np(yr), {n: LAY._np(res[n]) for n in ("dq", "dk", "dv")},
                   {n: LAY._np(x.grad) for n, x in zip(("dq", "dk", "dv"), r)}, False, "sdpa lens, three bf16 rows")
    far_vs_compact(fb, launches, run, ("q.sb", "k.sb", "v.sb"), "sdpa lens, three bf16 rows", check=check,
                   paths={"sdpa_fwd": FUSED, "sdpa_bwd": FUSED})
    torch.cuda.synchronize()
    fb.release()

    gq = _gen(97)
    q, k, v = (torch.randn(B, m, H, dk, generator=gq).to(BF16).cuda() for m in (1, LAY.CAP, LAY.CAP))
    kv_len = torch.tensor([LAY.KV_LEN], dtype=I32, device="cuda")
    forms = (("decode_attention_ragged", dict(kv_start=torch.tensor([0, 70, 5], dtype=I32, device="cuda")), dict(kv_len=kv_len), LAY.KV_LEN),
             ("decode_attention_lens", dict(kv_lens=torch.tensor([LAY.KV_LEN, 65, 7], dtype=I32, device="cuda")), {}, LAY.CAP))
    for op, rkw, kw, L_ in forms:
        def run_d(put):
            return {"y": getattr(ops, op)(put(q), put(k), put(v), **rkw, **kw)}

        def check_d(res):
            ref = LAY._decode_ref64(q, k, v, L_, False, **rkw)
            e = float((res["y"].double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            print(f"\nFIG {op}, three bf16 rows: y {e:.3e}")
            assert e <= LAY.DECODE_TOL[BF16], e
        far_vs_compact(fb, launches, run_d, ("q.sb", "k.sb", "v.sb"), op + ", three bf16 rows", check=check_d,
                       paths={ops._DA_OPS[op][2]: FUSED})
        torch.cuda.synchronize()
        fb.release()


def test_decode_rows_against_the_cache_rows_in_reverse(fb, launches):
    """decode_attention_rows with the row table sending query row b to cache row B - 1 - b: (r - b) * sb is negative and beyond
    2^31 in magnitude.  Reference and bound: test_gpu_attn_layouts._decode_ref64 / DECODE_TOL (test_gpu_whisper_decode's)."""
    from mop_amd import ops
    for dt, Bd, Tq, dk, causal in ((BF16, 3, 3, 64, True), (F32, 2, 1, 128, False)):
        g = _gen(dk + Tq)
        q, k, v = (torch.randn(Bd, m, 2, dk, generator=g).to(dt).cuda() for m in (Tq, LAY.CAP, LAY.CAP))
        rows = (Bd - 1 - torch.arange(Bd, dtype=I32))[:, None].repeat(1, LAY.CAP).cuda()
        kv_len = torch.tensor([LAY.KV_LEN], dtype=I32, device="cuda")
        what = f"decode-rows-reversed-{dt}"

        def run(put):
            qq, kk, vv = put(q), put(k), put(v)
            y = ops.decode_attention_rows(qq, kk, vv, rows, kv_len=kv_len, causal=causal)
            return {"y": y}

        def check(res):
            ref = LAY._decode_ref64(q, k, v, LAY.KV_LEN, causal, rows=rows)
            e = float((res["y"].double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            print(f"\nFIG {what}: y {e:.3e}")
            assert e <= LAY.DECODE_TOL[dt], e
        far_vs_compact(fb, launches, run, ("q.sb", "k.sb", "v.sb"), what, check=check, paths={"decode_attn_rows": FUSED})
        torch.cuda.synchronize()
        fb.release()


# ------------------------------------------------------------------------------------------------ row ops over logits
def _upstream(red, R):
    return torch.ones(R, device="cuda") if red == "none" else torch.tensor(1.0, device="cuda")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,start", [(1000, 0), (1003, 0), (1003, 3)], ids=["V1000", "V1003", "V1003+3"])
def test_cross_entropy_forward_and_backward(V, start, dtype, fb, launches):
    """ops.cross_entropy on far logits rows, the gradient as a new tensor and written over the far rows (dlogits_ld far as well).
    start = 3: the rows begin 3 elements behind a 16-byte boundary (RowSpan's head).  Reference and bounds: ce_rows.py."""
    from mop_amd import ops
    R = _rows(dtype)
    x_cpu, t = CR.normal(R, V, seed=V + start)
    xs = CR.stored(x_cpu, dtype)
    ref = CR.Ref(xs, t)
    wide = torch.cat([torch.full((R, start), float("nan"), dtype=dtype), xs], 1).cuda()
    tc = t.cuda()
    for red, inplace in (("none", False), ("sum", True), ("mean", False)):
        what = f"cross_entropy V={V} start={start} {dtype} {red} inplace={inplace}"

        def run(put):
            x = put(wide)[:, start:].requires_grad_()
            loss = ops.cross_entropy(x, tc, -100, red, inplace)
            val = loss.detach().clone()
            (g,) = torch.autograd.grad(loss, x, _upstream(red, R))
            if inplace:
                assert g.data_ptr() == x.data_ptr() and g.stride(0) == x.stride(0)
            return {"loss": val, "g": g.detach().clone(memory_format=torch.contiguous_format)}

        def check(res):
            f_loss = CR.worst(res["loss"], *ref.reduced(red))
            f_grad = CR.worst(res["g"], *ref.grad(red, 1.0))
            print(f"\nFIG {what}: loss {f_loss:.3f} grad {f_grad:.3f} of the bound")
            assert f_loss <= 1.0 and f_grad <= 1.0, (what, f_loss, f_grad)
        fields = ("logits_ld",) + (("mopk_cross_entropy_bwd:dlogits_ld",) if inplace else ())
        far_vs_compact(fb, launches, run, fields, what, check=check, paths={"cross_entropy_fwd": FUSED, "cross_entropy_bwd": FUSED})
        torch.cuda.synchronize()
        fb.release()

    # through the C ABI: a gradient buffer of its own, far as the logits are (ops.cross_entropy allocates a compact one, and
    # reaches a far dlogits_ld only where the gradient is written over the logits, as above)
    what = f"cross_entropy C ABI V={V} start={start} {dtype}"

    def run_abi(put):
        x, d = put(wide)[:, start:], put(torch.zeros_like(wide))[:, start:]
        a = ops._ce_args(x, tc, -100)
        lse, row_loss = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
        a.lse, a.row_loss = lse.data_ptr(), row_loss.data_ptr()
        ops._row_launch(a, "mopk_cross_entropy_fwd", "cross_entropy_fwd")
        up = torch.ones(R, device="cuda")
        a.grad, a.grad_stride, a.dlogits, a.dlogits_ld = up.data_ptr(), 1, d.data_ptr(), d.stride(0)
        assert d.data_ptr() != x.data_ptr() and d.stride(0) == x.stride(0)
        ops._row_launch(a, "mopk_cross_entropy_bwd", "cross_entropy_bwd")
        torch.cuda.synchronize()
        return {"loss": row_loss, "g": d.detach().clone(memory_format=torch.contiguous_format)}

    def check_abi(res):
        f_loss, f_grad = CR.worst(res["loss"], *ref.reduced("none")), CR.worst(res["g"], *ref.grad("none", 1.0))
        print(f"\nFIG {what}: loss {f_loss:.3f} grad {f_grad:.3f} of the bound")
        assert f_loss <= 1.0 and f_grad <= 1.0, (what, f_loss, f_grad)
    far_vs_compact(fb, launches, run_abi, ("logits_ld", "mopk_cross_entropy_bwd:dlogits_ld"), what, check=check_abi,
                   paths={"cross_entropy_fwd": FUSED, "cross_entropy_bwd": FUSED})


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [1000, 1003])
def test_token_logprob_and_greedy_pick(V, dtype, fb, launches):
    """reference and bound: test_gpu_whisper_fallback._logprob_both / _pick_both (float64 restatement, LP_TOL)"""
    import test_gpu_whisper_fallback as FB
    from mop_amd import ops
    R = _rows(dtype)
    for name, x, eos, done in FB.stat_cases(V, R, dtype, "cuda"):
        if name not in ("plain", "filtered", "tie"):
            continue
        what = f"V={V} {dtype} {name}"
        toks = FB._tokens_for(x, name)

        def run_lp(put):
            return {"lp": FB._logprob_both(ops, put(x), toks, what), "lp_one": FB._logprob_both(ops, put(x), int(toks[-1]), what)}
        far_vs_compact(fb, launches, run_lp, ("logits_ld",), "token_logprob " + what, paths={"token_logprob": FUSED})

        def run_pick(put):
            st = FB._pick_both(ops, put(x), eos, done, what)
            return {n: getattr(st, n).clone() for n in ("next_ids", "done", "n_tokens", "hist", "sum_logprobs")}
        far_vs_compact(fb, launches, run_pick, ("logits_ld",), "greedy_pick " + what, paths={"greedy_pick": FUSED})
        torch.cuda.synchronize()
        fb.release()


RULE_SHAPES = {1000: (1000, 900, 890), 1003: (1003, 900, 890)}          # V -> (V, first timestamp, eos), as SHAPES of the rules tests


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [1000, 1003])
def test_logit_rules_and_repeat_rules(V, dtype, fb, launches):
    """logits far, the result in a buffer of the op's own and written over the far logits (out_ld far); fp32: the int32 history
    far as well (hist_ld; an int32 view has two far rows, a bf16 call three).  References: test_gpu_whisper_rules._both_paths
    (the float64 restatement of the rules outside its near-tie exclusion) and test_gpu_whisper_repeat._both_paths with
    test_whisper_repeat_cpu.expected (bit for bit)."""
    import test_gpu_whisper_repeat as RP
    import test_gpu_whisper_rules as RU
    import test_whisper_repeat_cpu as RPC
    from mop_amd import ops
    R = _rows(dtype)
    hist_far = R == _rows(I32)
    _, tb, eos = RULE_SHAPES[V]
    kw = RU.rule_sets(V, tb, eos)["full"]
    rules = ops.LogitRules(V, **kw)
    for hname in ("pairs-then-lone", "n0", "last-is-V-1-pair"):
        x, hist, pos = RU.build_case(V, tb, eos, R, dtype, RU.histories(V, tb, eos)[hname], 31 + V, "cuda")
        for alias in (False, True):
            what = f"logit_rules V={V} {dtype} {hname} out=logits:{alias}"

            def run(put):
                xx, hh = put(x), (put(hist) if hist_far else hist)
                got, left_out = RU._both_paths(xx, hh, pos, RU.T0, rules, kw, what, out=xx if alias else None)
                assert (got.data_ptr() == xx.data_ptr()) == alias, what
                return {"out": got.detach().clone(memory_format=torch.contiguous_format)}
            fields = ("logits_ld",) + (("out_ld",) if alias else ()) + (("hist_ld",) if hist_far else ())
            far_vs_compact(fb, launches, run, fields, what, paths={"logit_rules": FUSED})
            torch.cuda.synchronize()
            fb.release()
    for ci, (s, p, n) in enumerate(((3, 1.3, 30), (0, 1.5, 30), (2, 1.3, 8))):
        rr = RPC.rules_of(V, p, s, device="cuda")
        x, hist, pos = (t.cuda() for t in RPC.build_case(V, R, dtype, n, s, 100 * ci + R))
        want, _ = RPC.expected(x.cpu(), hist.cpu(), pos.cpu(), RPC.rules_of(V, p, s))
        for alias in (False, True):
            what = f"repeat_rules V={V} {dtype} ngram={s} penalty={p} out=logits:{alias}"

            def run(put):
                xx, hh = put(x), (put(hist) if hist_far else hist)
                if alias:
                    got = RP._both_paths(xx, hh, pos, RPC.T0, rr, out=xx)
                else:                                  # _both_paths would add an in-place launch on a compact copy of its own
                    got = ops.repeat_rules(xx, hh, pos, RPC.T0, rr)
                    RPC.assert_bits_equal(got, ops.repeat_rules_torch(xx.clone(), hh, pos, RPC.T0, rr), what + " (torch path)")
                RPC.assert_bits_equal(got, want, what)
                return {"out": got.detach().clone(memory_format=torch.contiguous_format)}
            fields = ("logits_ld",) + (("out_ld",) if alias else ()) + (("hist_ld",) if hist_far else ())
            far_vs_compact(fb, launches, run, fields, what, paths={"repeat_rules": FUSED})
            torch.cuda.synchronize()
            fb.release()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [1000, 1003])
def test_sample_and_sample_ragged(V, dtype, fb, launches):
    """as test_gpu_whisper_sample.test_kernel_matches_the_torch_path: the log-probability within LP_TOL of the fp32 log-softmax, the
    token inside the float64 kept set (_kept64); the ragged form row by row against sample_tokens at the row's own position
    (test_gpu_whisper_ragged.test_sampling_offsets_the_position)."""
    import test_gpu_whisper_sample as SM
    from mop_amd import ops
    from test_whisper_fallback_cpu import LP_TOL       # "the `lp` tolerance of tests/test_gpu_whisper_sample.py"
    R = _rows(dtype)
    g = _gen(V)
    x = (torch.randn(R, V, generator=g) * 2.5).to(dtype).cuda()
    x[0, : V // 3] = SM.NEG
    x[1, 1] = x[1, 4] = x[1].max()
    off = torch.tensor([0, 7, 3][:R], dtype=I32, device="cuda")
    for i, (T, k, p) in enumerate([(1.0, 0, 1.0), (0.7, 50, 0.95), (0.0, 0, 1.0), (0.9, 3, 0.3)]):
        pos = torch.tensor([17 + i], dtype=I32, device="cuda")
        what = f"sample V={V} {dtype} T={T} k={k} p={p}"

        def run(put):
            xx = put(x)
            tok, lp = ops.sample_tokens(xx, pos, T, k, p, seed=1234 + i)
            rt, rl = ops.sample_tokens_ragged(xx, pos, off, T, k, p, seed=1234 + i)
            return {"tok": tok, "lp": lp, "ragged_tok": rt, "ragged_lp": rl}

        def check(res):
            ref_lp = torch.log_softmax(x.float(), -1).gather(1, res["tok"].long().unsqueeze(1)).squeeze(1)
            assert (res["lp"] - ref_lp).abs().max() <= LP_TOL, what
            if T == 0:
                assert torch.equal(res["tok"].long(), x.float().argmax(-1)), what
            else:
                assert SM._kept64(x, T, k, p).gather(1, res["tok"].long().unsqueeze(1)).all(), what
            for r in range(R):
                tr, lr = ops.sample_tokens(x, pos - off[r], T, k, p, seed=1234 + i)
                assert int(res["ragged_tok"][r]) == int(tr[r]) and float(res["ragged_lp"][r]) == float(lr[r]), (what, r)
        far_vs_compact(fb, launches, run, ("logits_sb",), what, check=check, paths={"sample": FUSED, "sample_ragged": FUSED})
        torch.cuda.synchronize()
        fb.release()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V", [1000, 1003])
def test_language_probs(V, dtype, fb, launches):
    """reference and bound: test_gpu_whisper_language._both (check_language_probs: float64 restatement, LP_TOL); fp32: the (R, n)
    result far as well (probs_ld)"""
    import test_gpu_whisper_language as LG
    from mop_amd import ops
    R, n = _rows(dtype), 99
    for name, x, ids in LG.language_cases(V, R, dtype, n, "cuda"):
        L_ = ops.LanguageTokens(V, ids, device="cuda")
        what = f"language_probs V={V} {dtype} {name}"

        def run(put):
            out = {}
            if dtype == F32:
                out = dict(out_probs=put(torch.zeros(R, n, device="cuda")))
            got = LG._both(ops, put(x), L_, ids, what, **out)
            return {"probs": got.probs.detach().clone(memory_format=torch.contiguous_format), "tokens": got.tokens.clone()}
        fields = ("logits_ld",) + (("probs_ld",) if dtype == F32 else ())
        far_vs_compact(fb, launches, run, fields, what, paths={"language_probs": FUSED})
        torch.cuda.synchronize()
        fb.release()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_beam_step(dtype, fb, launches):
    """(B, V) logits shared by each item's K = 4 beams, far along B (logits_sb).  Reference and bound: tests/beam_rows.py for rows
    that start on a 16-byte boundary (offset 0, a row stride of whole vectors), which is how the far rows and their twins lie."""
    import beam_rows as BR
    import test_gpu_beam_rows as BT
    B, K, V = _rows(dtype), 4, 1003
    g = BR._gen(77 + B)
    x = torch.cat([BR._dense(g, K, V, dtype, eos=9)[0][:1] for _ in range(B)])
    sc = -3.0 * torch.randperm(B * K, generator=g).float() - torch.rand(B * K, generator=g)
    c = BR.Case(f"far-shared-rows-{BR.tag(dtype)}", "edges", B, K, x, sc, eos=9, offset=0, sk=1024, ld_pad=2)
    assert BR.decided(c) is None and all(c.row_mod16(r) == 0 for r in range(B))
    ref = BR.reference(c)

    def run(put):
        st, wide = c.state("cuda")
        BT._steps(c, put(x.cuda()), st)
        got = BR.state_dict(st)
        frac = BR.compare(c, ref, got, wide)
        print(f"\nFIG {c.name}: {frac:.3f} of the bound")
        return {k: v.cuda() for k, v in got.items()}
    far_vs_compact(fb, launches, run, ("logits_sb",), c.name, paths={"beam_step": FUSED})


# ------------------------------------------------------------------------------------------------ gates and norms
@pytest.mark.parametrize("with_lens", [False, True], ids=["plain", "lens"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_token_gate_1d(dtype, with_lens, fb, launches):
    """x and a far along B, plain and lens=.  Reference: gpt_lens_ref.token_gate_rows_alone (full lengths: the plain op); bounds:
    test_gpu_gpt_lens.test_token_gate_rows_are_as_alone (those of test_gpu_gpt.test_token_gate_op_against_float64)."""
    import test_gpu_gpt_lens as GL
    from gpt_lens_ref import token_gate_rows_alone
    from mop_amd import ops
    B, T, D = _rows(dtype), 40, 64
    tol = GL.TG_TOL["bf16" if dtype == BF16 else "fp32"]
    lens_v = (33, 40, 17)[:B] if with_lens else (T,) * B
    x, a, u, dout = GL._tg_inputs(B, T, D, dtype, True, seed=D + B)
    ro, rdr, rdu = token_gate_rows_alone(x, a, u, lens_v, dout)
    lens = GL._lens(lens_v) if with_lens else None
    what = f"token_gate_1d {dtype} lens={with_lens}"

    def run(put):
        xr, ar, ur = put(x.cuda()).requires_grad_(), put(a.cuda()).requires_grad_(), u.cuda().clone().requires_grad_()
        out = ops.token_gate_1d(xr, ar, ur, lens)
        out.backward(dout.cuda())
        return {"out": out.detach(), "dx": xr.grad, "da": ar.grad, "du": ur.grad}

    def check(res):
        errs = {k: GL._nerr(res[k], r) for k, r in (("out", ro), ("dx", rdr), ("da", rdr), ("du", rdu))}
        print(f"\nFIG {what}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        assert all(e <= tol for e in errs.values()), errs
    far_vs_compact(fb, launches, run, ("x_sb", "a_sb"), what, check=check, paths={"token_gate_fwd": FUSED, "token_gate_bwd": FUSED})


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_gated_residual(dt, fb, launches):
    """x and a far along B (fp32: the (B, T) gate as well, gate_sb).  The float64 formulas and bounds of
    test_gpu_whisper_gate.test_gated_residual_against_float64."""
    import test_gpu_whisper_gate as GT
    from mop_amd import ops
    B = _rows(GT.GR_DTYPES[dt][0])
    x, a, gate, dout, odt = GT._gr_case(B, 37, 384, dt)
    gate_far = dt == "fp32"
    what = f"gated_residual {dt}"

    def run(put):
        xs, as_, gs = (t.requires_grad_() for t in (put(x), put(a), put(gate) if gate_far else gate.detach().clone()))
        out = ops.gated_residual(xs, as_, gs)
        out.backward(dout)
        return {"out": out.detach(), "dx": xs.grad, "da": as_.grad, "dgate": gs.grad}

    def check(res):
        r64 = x.double() + a.double()
        ref_out, ref_dr, ref_dg = r64 * gate.double().unsqueeze(-1), dout.double() * gate.double().unsqueeze(-1), (dout.double() * r64).sum(-1)
        tol = GT.GR_TOL
        for name, ref, bound in (("out", ref_out, tol[odt]), ("dx", ref_dr, tol[x.dtype]), ("da", ref_dr, tol[a.dtype]),
                                 ("dgate", ref_dg, GT.GR_DGATE_TOL)):
            e = GT._rel(res[name], ref)
            print(f"\nFIG {what} {name}: {e:.3e} (bound {bound:.1e})")
            assert e <= bound, name
    fields = ("x_sb", "a_sb") + (("gate_sb",) if gate_far else ())
    far_vs_compact(fb, launches, run, fields, what, check=check, paths={"gated_residual_fwd": FUSED, "gated_residual_bwd": FUSED})


@pytest.mark.parametrize("how", ["bf16", "fp32"])
def test_mel_gate_forward_and_backward(how, fb, launches):
    """mel far along B (mel_sb).  The forward against ops.mel_gate_torch in float64 and the backward against float64
    autograd of it (MG_BWD_TOL), as test_gpu_whisper_gate's two float64 tests (the forward's bound is its MG_FWD_TOL)."""
    import test_gpu_whisper_gate as GT
    from mop_amd import ops
    B, T, Fm, L_, k = _rows(BF16 if how == "bf16" else F32), 130, 80, 3, 5
    W, mel = GT._taps(L_, k, Fm, seed=1), GT._mel(B, T, Fm, how, seed=2)
    dg = torch.randn(B, L_, T, generator=_gen(3)).cuda()
    what = f"mel_gate {how}"

    def run(put):
        Wl = W.detach().clone().requires_grad_()
        got = ops.mel_gate(put(mel), Wl)
        got.backward(dg)
        return {"gates": got.detach(), "dW": Wl.grad}

    def check(res):
        W64 = W.double().requires_grad_()
        ref = ops.mel_gate_torch(mel.double(), W64)
        (ref_dW,) = torch.autograd.grad(ref, W64, dg.double())
        e, eg = GT._rel(res["gates"], ref.detach()), GT._rel(res["dW"], ref_dW)
        print(f"\nFIG {what}: gates {e:.3e} (bound {GT.MG_FWD_TOL:.0e}) dW {eg:.3e} (bound {GT.MG_BWD_TOL:.0e})")
        assert e <= GT.MG_FWD_TOL and eg <= GT.MG_BWD_TOL
    far_vs_compact(fb, launches, run, ("mel_sb",), what, check=check, paths={"mel_gate_fwd": FUSED, "mel_gate_bwd": FUSED})


@pytest.mark.parametrize("xdt,ydt", [(BF16, BF16), (F32, F32), (F32, BF16)], ids=["bf16", "f32", "f32-bf16"])
def test_layernorm_kernels_through_the_c_abi(xdt, ydt, fb, launches):
    """mopk_layernorm_fwd / _bwd with x_ld and y_ld far, rows = 3 where the dtype has three far rows: ops.layernorm_residual makes x
    contiguous, so the stride reaches the kernels through the C ABI (as test_gpu_bounds.test_layernorm_kernels_with_a_row_stride
    builds its arguments).  y and dx are written into far rows.  Reference and bounds: test_gpu_layernorm._ref, as that test."""
    from mop_amd import _lib as L, ops
    from test_gpu_layernorm import _ref, ln_tols
    rows, dim = min(_rows(xdt), _rows(ydt)), 72
    gen = _gen(rows * 131 + dim)
    x = (torch.randn(rows, dim, generator=gen) * 1.7 + 0.3).to(xdt)
    g, b = (1.0 + 0.2 * torch.randn(dim, generator=gen)), (0.1 * torch.randn(dim, generator=gen))
    dy, dres = torch.randn(rows, dim, generator=gen).to(ydt), torch.randn(rows, dim, generator=gen).to(xdt)
    yr, dxr, dgr, dbr = _ref(x.float(), g, b, 1e-5, dy.float(), dres.float())
    what = f"layernorm C ABI {xdt} -> {ydt}"

    def run(put):
        xw, drw, dyw = put(x.cuda()), put(dres.cuda()), put(dy.cuda())
        yw, dxw = put(torch.zeros(rows, dim, dtype=ydt, device="cuda")), put(torch.zeros(rows, dim, dtype=xdt, device="cuda"))
        gg, bb = g.cuda(), b.cuda()
        f32 = dict(dtype=F32, device="cuda")
        mean, rstd, dg, db = torch.empty(rows, **f32), torch.empty(rows, **f32), torch.empty(dim, **f32), torch.empty(dim, **f32)
        a = L.LayerNormArgs(rows=rows, dim=dim, x_dtype=ops._io_dtype(xw), y_dtype=ops._io_dtype(yw), p_dtype=ops._io_dtype(gg), eps=1e-5,
                            x_ld=xw.stride(0), y_ld=yw.stride(0), x=xw.data_ptr(), gamma=gg.data_ptr(), beta=bb.data_ptr(), y=yw.data_ptr(),
                            mean=mean.data_ptr(), rstd=rstd.data_ptr())
        assert dxw.stride(0) == drw.stride(0) == xw.stride(0) and dyw.stride(0) == yw.stride(0)
        ops._launch("mopk_layernorm_fwd", a)
        a.dy, a.dres, a.dx, a.dgamma, a.dbeta = dyw.data_ptr(), drw.data_ptr(), dxw.data_ptr(), dg.data_ptr(), db.data_ptr()
        ws = torch.empty(max(1, L.lib().mopk_layernorm_workspace_bytes(C.byref(a))), dtype=torch.uint8, device="cuda")
        a.workspace = ws.data_ptr()
        ops._launch("mopk_layernorm_bwd", a)
        torch.cuda.synchronize()
        return dict(y=yw.clone(), dx=dxw.clone(), dgamma=dg, dbeta=db, mean=mean, rstd=rstd)

    def check(res):
        ytol, gt = ln_tols(xdt, ydt)
        assert (res["y"].float().cpu().double() - yr).abs().max().item() <= ytol * max(1.0, yr.abs().max().item())
        for name, ref in (("dx", dxr), ("dgamma", dgr), ("dbeta", dbr)):
            err = (res[name].float().cpu().double() - ref).abs().max().item() / max(1e-6, ref.abs().max().item())
            print(f"\nFIG {what} {name}: {err:.2e} (bound {gt:.0e})")
            assert err <= gt, f"{name} {err:.2e}"
    far_vs_compact(fb, launches, run, ("x_ld", "y_ld"), what, check=check)


# ------------------------------------------------------------------------------------------------ alignment
def test_alignment_cost_and_dtw_align(fb, launches):
    """fp32 maps, two items far apart: alignment_cost reads (B, S, N, M) probabilities (probs_sb), dtw_align (B, N, M) costs
    (cost_sb).  References: test_gpu_whisper_align._cost_both (float64, the torch restatement's own error as the yardstick) and
    _dtw_both with test_whisper_align_cpu.ref_dtw_batch (integers, exact)."""
    import numpy as np
    import test_gpu_whisper_align as AL
    S, N, M = 3, 40, 150
    probs, nt, nf = AL.cost_case(S, N, M, [40, 17], [150, 65], 9, "cuda")

    def run_cost(put):
        got, _, _ = AL._cost_both(put(probs), nt, nf, 7, "far rows")
        return {"cost": AL._inside(got, nt, nf)}
    far_vs_compact(fb, launches, run_cost, ("probs_sb",), "alignment_cost", paths={"alignment_cost": FUSED})
    torch.cuda.synchronize()
    fb.release()

    cost, nr, nc = AL.dtw_case(70, 93, 7, B=2, n_rows=[70, 66], n_cols=[93, 64], row0=2)
    rs, re = AL.ref_dtw_batch(cost, nr, nc, 2)

    def run_dtw(put):
        s, e = AL._dtw_both(put(cost.cuda()), nr.cuda(), nc.cuda(), 2, "far rows")
        assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(e.cpu().numpy(), re)
        return {"starts": s, "ends": e}
    far_vs_compact(fb, launches, run_dtw, ("cost_sb",), "dtw_align", paths={"dtw_align": FUSED})


# ------------------------------------------------------------------------------------------------ integer token ops
def test_timestamp_segments_and_the_prompt_history_update(fb, launches):
    """int32 token rows, two of them far apart (tokens_ld).  timestamp_segments against test_whisper_transcribe_cpu.ref_segments,
    the prompt-history update through test_whisper_condition_cpu.check_update (its restatement, its guards); integers, exact.
    MopkPromptHistoryArgs has no stride for hist itself (a contiguous (B, n) state): the token rows are what can lie far."""
    import test_whisper_condition_cpu as CO
    import test_whisper_transcribe_cpu as TR
    from mop_amd import ops
    rows, window = TR.random_rows(2, 70, 3, seed=8)
    tok, win = TR.tensors(rows, window, "cuda")
    want = TR.ref_segments(rows, 3, window, TR.TB, TR.EOS, 2)

    def run_ts(put):
        got = ops.timestamp_segments(put(tok), 3, win, TR.TB, TR.EOS, 2)
        TR.assert_segments_equal(got, want, "far rows")
        return dict(zip(("starts", "ends", "tok_begin", "tok_end", "n_segments", "advance"), got))
    far_vs_compact(fb, launches, run_ts, ("tokens_ld",), "timestamp_segments", paths={"timestamp_segments": FUSED})
    torch.cuda.synchronize()
    fb.release()

    t0 = 3
    case = (2, 6, [5, 2], CO.token_rows(2, t0 + 8, 5), t0, [4, 3], [1, 0], [0, 0], "far token rows")

    def run_ph(put):
        def fn(hist, hist_len, tokens, *rest):
            return ops.prompt_history_update(hist, hist_len, put(tokens), *rest)
        hist, hl = CO.check_update(fn, *case, device="cuda")
        return {"hist": hist.clone(), "hist_len": hl.clone()}
    far_vs_compact(fb, launches, run_ph, ("tokens_ld",), "prompt_history_update", paths={"prompt_history_update": FUSED})


# ------------------------------------------------------------------------------------------------ Edgewise cores
EDGEWISE = {
    # name: (dense head, mode of test_gpu_edgewise_peaks.run_core, I/O dtype, ops.set_path before the run)
    "lowrank-fused-bf16": (False, 1, BF16, "auto"),
    "lowrank-generic-fp32": (False, 5, F32, "auto"),
    "general-dense-fused-fp32io": (True, 1, F32, "auto"),
    "general-dense-generic-bf16": (True, 4, BF16, "generic"),
}


@pytest.mark.parametrize("name", list(EDGEWISE))
def test_edgewise_cores_through_the_c_abi(name, fb, launches):
    """edgewise_lowrank_core and edgewise_general_core, fused and generic, forward and backward, with the packed (B, N, 1, 3, H, dk)
    qkv far along B.  The wrappers make qkv contiguous and derive the strides from its shape (ops._ew_views), so a far qkv reaches
    the kernels through the C ABI only: the wrapper runs on a compact qkv and the struct it built is edited on its way into the
    library, q / k / v0 / vL pointing into a far twin that holds the same values with sb = FAR_STRIDE.  The gradient buffer is the
    wrapper's own (compact).  Runner, reference and bounds: test_gpu_edgewise_peaks.run_core / judge on a case of
    edgewise_peaks.peaked_case (N = 65, dk = 32, V = 3, r = 2, level 2) at this file's B."""
    import numpy as np
    import edgewise_peaks as EPK
    import test_gpu_edgewise_peaks as EP
    from mop_amd import ops
    dense, mode, dt, pin = EDGEWISE[name]
    B = _rows(dt)
    case = EPK.peaked_case(65, 32, 3, 2, 2, 4242 + dense, B=B, dense=dense)
    twin = fb.far_like(case.qkv().cuda().to(dt))
    views = ("q", "k", "v0", "vL")
    row_bytes = twin[0].numel() * twin.element_size()

    def retarget(sym, a):
        if not sym.startswith("mopk_edgewise") or _field(a, "v0.sb") is _MISSING:
            return
        base = a.q.ptr
        for n in views:
            v = getattr(a, n)
            assert 0 <= v.ptr - base < row_bytes and v.sb * twin.element_size() == row_bytes, (name, n)
            v.ptr, v.sb = twin.data_ptr() + (v.ptr - base), FAR
    fields = tuple(n + ".sb" for n in views)
    ops.set_path(pin)
    launches.hook = retarget
    try:
        far = EP.run_core(case, mode, dt)
    finally:
        launches.hook = None
    stem = "mopk_edgewise" if dense else "mopk_edgewise_lowrank"
    assert {stem + "_fwd", stem + "_bwd"} <= {s_ for s_, _ in launches}, [s_ for s_, _ in launches]
    assert_far_strides(launches, fields, name)
    fb.check_guards()
    del launches[:]
    ops.set_path(pin)
    compact = EP.run_core(case, mode, dt)
    assert_compact_strides(launches, fields, name)
    EP.judge(case, far, mode, dt, "far rows")
    assert set(far) == set(compact)
    for k in far:
        assert np.array_equal(far[k], compact[k]), f"{name}: {k} of the far run differs from the compact run"


# ------------------------------------------------------------------------------------------------ quartet without the term, with lens=
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("uq,with_lens", [(False, False), (True, True), (False, True)], ids=["off", "on-lens", "off-lens"])
def test_quartet_core_without_the_quartet_term_and_with_lens(uq, with_lens, prec, fb, launches):
    """reference: gpt_lens_ref.quartet_rows_alone (full lengths: the plain op); bounds: test_gpu_gpt_lens._qt_check; inputs drawn
    as test_gpu_gpt_lens._qt_case draws them (the first draw whose smallest score-row std is at least SD_MIN)"""
    import test_gpu_gpt_lens as GL
    from gpt_lens_ref import quartet_rows_alone
    from mop_amd import ops
    dt = BF16 if prec == "bf16" else F32
    B, T, H, dk = _rows(dt), 130, 2, (64 if prec == "bf16" else 32)
    lens_v = (130, 67, 2)[:B] if with_lens else (T,) * B
    for draw in range(64):
        g = _gen(100000 * draw + 1000 * dk + 10 * uq + B)
        ts = tuple(torch.randn(B, T, H, dk, generator=g).to(dt) for _ in range(5))
        dy = torch.randn(B, T, H * dk, generator=g).to(dt)
        if GL._min_row_sd(ts, lens_v, uq) >= GL.SD_MIN:
            break
    else:
        raise AssertionError("no well-conditioned draw in 64")
    ref = quartet_rows_alone(*ts[:3], ts[3] if uq else None, ts[4] if uq else None, GL.MIX, GL.QS, lens_v, GL.EPS, uq, dy)
    lens = GL._lens(lens_v) if with_lens else None
    what = f"quartet_core use_quartet={uq} lens={with_lens} {prec}"

    def run(put):
        xs = [put(t.cuda()).requires_grad_() for t in (ts if uq else ts[:3])]
        mix, qs = (torch.tensor([v], device="cuda", requires_grad=True) for v in (GL.MIX, GL.QS))
        y = ops.quartet_core(xs[0], xs[1], xs[2], xs[3] if uq else None, xs[4] if uq else None, mix if uq else None,
                             qs if uq else None, None, GL.EPS, uq, False, lens=lens)
        y.backward(dy.cuda())
        res = {"y": y.detach()}
        res.update({"d" + k: t.grad for k, t in zip(("q", "k", "v", "q2", "k2"), xs)})
        if uq:
            res.update(dmixture=mix.grad, dquartet_scale=qs.grad)
        return res
    fields = ("q.sb", "k.sb", "v.sb") + (("q2.sb", "k2.sb") if uq else ())
    far_vs_compact(fb, launches, run, fields, what, check=lambda res: GL._qt_check(res, ref, prec, lens_v, uq),
                   paths={"quartet_fwd": FUSED if prec == "bf16" else GENERIC})


# ------------------------------------------------------------------------------------------------ audio
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_log_mel_and_resample(dtype, fb, launches, monkeypatch):
    """audio rows far apart: log_mel (audio_ld) and resample (audio_sb).  Each goes through its own test file's check() -- float64
    restatement, the torch path, their bounds -- with the op wrapped so that the audio check() built reaches it as a far view (or
    as its compact twin)."""
    import test_gpu_whisper_frontend as FE
    import test_gpu_whisper_resample as RS
    from mop_amd import ops
    B = _rows(dtype)
    real_mel, real_rs = ops.log_mel, ops.resample
    clips = [FE.noise(160 * 35 + 9, seed=40 + b) for b in range(B)]

    def run_mel(put):
        monkeypatch.setattr(ops, "log_mel", lambda audio, *a, **k: real_mel(put(audio), *a, **k))
        try:
            return {"mel": FE.check(clips, FE.DEF, "broadband", f"far rows {dtype}", in_dtype=dtype)}
        finally:
            monkeypatch.setattr(ops, "log_mel", real_mel)
    far_vs_compact(fb, launches, run_mel, ("audio_ld",), f"log_mel {dtype}", paths={"log_mel": FUSED})
    torch.cuda.synchronize()
    fb.release()

    rclips = [RS.noise(3 * 1200 + 7, seed=40 + b) for b in range(B)]

    def run_rs(put):
        monkeypatch.setattr(ops, "resample", lambda audio, *a, **k: real_rs(put(audio), *a, **k))
        try:
            return {"out": RS.check(rclips, 48000, RS.NEW, f"far rows {dtype}", in_dtype=dtype)}
        finally:
            monkeypatch.setattr(ops, "resample", real_rs)
    far_vs_compact(fb, launches, run_rs, ("audio_sb",), f"resample {dtype}", paths={"resample": FUSED})


# ------------------------------------------------------------------------------------------------ prompts and word timestamps
def test_window_prompts_alignment_rows_and_word_spans(fb, launches):
    """int32 rows, two of them far apart, each op through its own test file's check_* helper (restatement, integers exact; word
    probabilities under that helper's bound): window_prompts with per-clip sot rows (sot_ld; its hist is a contiguous state
    without a stride of its own), alignment_rows with far token rows and per-row sot (tokens_ld, sot_ld), word_spans with far
    tokens, times and probs (tokens_ld, times_ld, probs_ld)."""
    import test_whisper_condition_cpu as CO
    import test_whisper_words_cpu as WD
    from mop_amd import ops

    def run_wp(put):
        def fn(hist, hl, item, sot, *rest):
            return ops.window_prompts(hist, hl, item, put(sot), *rest)
        got = CO.check_prompts(fn, 2, 6, [6, 2], [1, 0], [[7, 8, 9], [10, 11, 12]], CO.PREV, 12, I32, "far sot rows", device="cuda",
                               sot_dtype=I32)
        return {"ids": got.ids, "kv_start": got.kv_start}
    far_vs_compact(fb, launches, run_wp, ("sot_ld",), "window_prompts", paths={"window_prompts": FUSED})
    torch.cuda.synchronize()
    fb.release()

    t0, S = 3, 65
    rows, take = WD.decoded_rows(2, t0 + S, t0, S + t0)

    def run_ar(put):
        def fn(tokens, t0_, n_take, sot, *rest):
            return ops.alignment_rows(put(tokens), t0_, n_take, put(sot), *rest)
        got = WD.check_rows(fn, rows, t0, take, [[7, 8, 9], [10, 11, 12]], WD.NOTS, WD.EOS, I32, "far rows", device="cuda", sot_dtype=I32)
        return {"ids": got.ids, "n_tokens": got.n_tokens, "col": got.col}
    far_vs_compact(fb, launches, run_ar, ("tokens_ld", "sot_ld"), "alignment_rows", paths={"alignment_rows": FUSED})
    torch.cuda.synchronize()
    fb.release()

    rules = WD.table_rules(device="cuda")
    tokens, times, probs, n_text = WD.random_rows(65, 2, 65001)

    def run_ws(put):
        def fn(tk, tm, pr, *rest):
            return ops.word_spans(put(tk), put(tm), put(pr), *rest)
        got = WD.check_spans(fn, tokens, times, probs, n_text, rules, 70, "far rows", device="cuda")
        return dict(zip(("starts", "ends", "probs", "tok_begin", "tok_end", "n_words"), got))
    far_vs_compact(fb, launches, run_ws, ("tokens_ld", "times_ld", "probs_ld"), "word_spans", paths={"word_spans": FUSED})


# ------------------------------------------------------------------------------------------------ one tensor past 2^32 elements
BIG_R, BIG_V, BIG_CHUNK = 85_400, 50_304, 4096


def test_cross_entropy_on_logits_of_more_than_2_to_the_32_elements(fb, launches):
    """ops.cross_entropy on bf16 (85,400, 50,304) logits, 4,295,961,600 elements in the far buffer: reduction "sum", the backward
    written over the logits.  Every row's lse and loss against torch's float64 logsumexp on the device under ce_rows.py's per-row
    bounds; the kept rows (first, last, either side of element offsets 2^31 and 2^32, 64 random ones) bit-equal in lse, loss and
    dlogits to the same rows run alone (the same 16-byte phase: test_gpu_cross_entropy pins that property); the total equal to the
    float64 sum of the kernel's own row losses to one fp32 rounding."""
    from mop_amd import ops
    R, V = BIG_R, BIG_V
    assert R * V > 2 ** 32 and (V * 2) % 16 == 0
    x = fb.far((1, R, V), BF16)[0]
    assert x.is_contiguous() and x.data_ptr() % 256 == 0
    g = torch.Generator(device="cuda").manual_seed(2031)
    for r0 in range(0, R, BIG_CHUNK):
        n = min(BIG_CHUNK, R - r0)
        x[r0:r0 + n] = (2.0 * torch.randn(n, V, device="cuda", generator=g)).to(BF16)
    t = torch.randint(0, V, (R,), device="cuda", generator=g)
    at31, at32 = 2 ** 31 // V, 2 ** 32 // V
    assert (at31, at32) == (42_690, 85_380)
    keep = sorted({0, R - 1, at31 - 1, at31, at31 + 1, at32 - 1, at32, at32 + 1,
                   *torch.randint(0, R, (64,), generator=_gen(64)).tolist()})
    t[keep[3]] = -100                                                       # one ignored row among the kept ones
    keep_t = torch.tensor(keep, device="cuda")
    kept_x = x[keep_t].clone()

    # float64 reference over all rows, before the backward overwrites them
    lse64 = torch.empty(R, dtype=torch.float64, device="cuda")
    xt64 = torch.empty(R, dtype=torch.float64, device="cuda")
    valid = t != -100
    tt = torch.where(valid, t, torch.zeros_like(t))
    for r0 in range(0, R, BIG_CHUNK):
        c = x[r0:r0 + BIG_CHUNK].double()
        lse64[r0:r0 + BIG_CHUNK] = torch.logsumexp(c, 1)
        xt64[r0:r0 + BIG_CHUNK] = c.gather(1, tt[r0:r0 + BIG_CHUNK, None])[:, 0]
        del c
    loss64 = torch.where(valid, lse64 - xt64, torch.zeros_like(lse64))
    lse_bound = CR.U * (4 * CR.depth(V, BF16) + 2 * math.log(V) + lse64.abs())
    loss_bound = torch.where(valid, lse_bound + CR.U * loss64.abs(), torch.zeros_like(lse_bound))

    xr = x.requires_grad_()
    del launches[:]
    rows = ops.cross_entropy(xr, t, -100, "none")
    lse = rows.grad_fn.saved_tensors[2]
    total = ops.cross_entropy(xr, t, -100, "sum", True)
    total_val = total.detach().clone()
    row_loss, lse = rows.detach().clone(), lse.clone()
    (gx,) = torch.autograd.grad(total, xr)
    torch.cuda.synchronize()
    assert ops.LAST_PATH["cross_entropy_fwd"] == ops.LAST_PATH["cross_entropy_bwd"] == FUSED
    assert gx.data_ptr() == x.data_ptr()
    got = strides_seen(launches, ("R", "logits_ld", "mopk_cross_entropy_bwd:dlogits_ld"))
    assert got == {"R": [R, R, R], "logits_ld": [V, V, V], "mopk_cross_entropy_bwd:dlogits_ld": [V]}, got
    fb.check_guards()

    f_lse = float(((lse.double() - lse64).abs() / lse_bound).max())
    f_loss = float(torch.where(valid, (row_loss.double() - loss64).abs() / loss_bound.clamp_min(1e-300), torch.zeros_like(loss64)).max())
    print(f"\nFIG big cross_entropy: lse {f_lse:.3f} loss {f_loss:.3f} of the per-row bound over {R} rows")
    assert f_lse <= 1.0 and f_loss <= 1.0, (f_lse, f_loss)
    assert bool((row_loss[~valid] == 0).all())
    s64 = float(row_loss.double().sum())
    assert abs(float(total_val) - s64) <= CR.U * abs(s64) * (1 + 2.0 ** -20), (float(total_val), s64)

    # the kept rows alone
    alone = kept_x.clone().requires_grad_()
    a_rows = ops.cross_entropy(alone, t[keep_t], -100, "none")
    a_lse = a_rows.grad_fn.saved_tensors[2]
    (a_g,) = torch.autograd.grad(a_rows, alone, torch.ones(len(keep), device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(a_rows.detach(), row_loss[keep_t]) and torch.equal(a_lse, lse[keep_t])
    assert torch.equal(a_g, x.detach()[keep_t]), "a kept row's dlogits differ from the row run alone"
    assert not bool(a_g[3].any()) and bool(torch.isfinite(a_g).all())


def test_scan_untouched_last(far_buffer):
    """one pass over the whole buffer after every case above: the sentinel everywhere (all rows have been given back)"""
    assert not far_buffer.live and far_buffer.handed_out
    t0 = time.time()
    far_buffer.scan_untouched()
    print(f"\nFIG far buffer: {len(far_buffer.handed_out)} rows were handed out; scanned {far_buffer.nbytes} bytes in {time.time() - t0:.2f} s")
