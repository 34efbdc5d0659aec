"""GPU checks of the cross-entropy kernels (mopk_cross_entropy_*), of ops.linear_cross_entropy and of the models' loss(), against
the float64 reference and the derived bounds of ce_rows.py.  Every case runs on the fused path, forward and backward; the largest
fraction of a bound each family used is printed (pytest -s) by the last test."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import ce_rows as CR
from guarded_alloc import embedded, guarded_allocations

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
USED = {}                                                               # family -> largest fraction of a bound used


def _note(family, *fracs):
    USED[family] = max(USED.get(family, 0.0), *fracs)


def _upstream(red, R, up):
    """the upstream gradient on the device: a scalar, or for "none" a strided (R,) vector"""
    if red != "none":
        return torch.tensor(1.0 if up is None else up, device="cuda")
    v = torch.ones(R) if up is None else torch.as_tensor(up, dtype=torch.float32)
    buf = torch.full((3 * R,), float("nan"), device="cuda")
    buf[::3] = v.cuda()
    return buf[::3]


def _run(x, t, ii=-100, red="mean", up=None, inplace=False):
    """ops.cross_entropy and its gradient on the view x -> (loss, gradient); both must have run on the kernels"""
    from mop_amd import _lib, ops
    ops.LAST_PATH.pop("cross_entropy_fwd", None), ops.LAST_PATH.pop("cross_entropy_bwd", None)
    x = x.detach().requires_grad_()
    loss = ops.cross_entropy(x, t, ii, red, inplace)
    assert loss.dtype == torch.float32 and loss.shape == ((x.shape[0],) if red == "none" else ())
    loss_val = loss.detach().clone()
    (g,) = torch.autograd.grad(loss, x, _upstream(red, x.shape[0], up))
    torch.cuda.synchronize()
    assert ops.LAST_PATH["cross_entropy_fwd"] == ops.LAST_PATH["cross_entropy_bwd"] == _lib.PATH_FUSED
    assert g.dtype == x.dtype and g.shape == x.shape
    return loss_val, g


def _judge(family, x_cpu, t, dtype, ld=None, start=0, ii=-100, red="none", up=None, inplace=False):
    """one case, laid out on the device with NaN around the rows, against float64 under the bounds"""
    xv = CR.layout(x_cpu, dtype, ld, start, device="cuda")
    tc = t.cuda()
    ref = CR.Ref(CR.stored(x_cpu, dtype), t, ii)
    loss, g = _run(xv, tc, ii, red, up, inplace)
    want, bound = ref.reduced(red)
    if red == "mean" and ref.n == 0:
        assert bool(torch.isnan(loss))
        f_loss = 0.0
    else:
        assert bool(torch.isfinite(loss).all())
        f_loss = CR.worst(loss, want, bound)
    gw, gb = ref.grad(red, 1.0 if up is None else up)
    assert bool(torch.isfinite(g).all())
    f_grad = CR.worst(g, gw, gb)
    print(f"{family}: loss {f_loss:.3f} grad {f_grad:.3f} of the bound (V={x_cpu.shape[1]}, {dtype}, {red})")
    assert f_loss <= 1.0 and f_grad <= 1.0, (family, f_loss, f_grad)
    assert bool((g[~ref.valid.cuda()] == 0).all())                  # ignored rows: exact zeros
    family = family.split("/")[0] + ("/bf16" if dtype == torch.bfloat16 else "/f32")
    _note(family + "/loss", f_loss), _note(family + "/grad", f_grad)
    return xv, loss, g


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lengths(dtype):
    for V in CR.lengths(dtype):
        for R in (1, 3):
            x, t = CR.normal(R, V, seed=V + R)
            _judge("lengths", x, t, dtype, red=("none", "mean", "sum")[(V + R) % 3])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_many_rows_and_the_whisper_vocabulary(dtype):
    x, t = CR.normal(1031, 33, seed=5)
    _judge("rows", x, t, dtype, red="mean")
    x, t = CR.normal(2, 51865, seed=6)                                  # ld = V odd: each row at another 16-byte phase
    _judge("vocab", x, t, dtype, red="none")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layouts(dtype):
    x, t = CR.normal(3, 1001, seed=8)
    _judge("layouts", x, t, dtype, ld=1001)                             # odd stride
    for inplace in (False, True):                                       # ld > V, NaN in the padding columns and around the rows
        xv, loss, g = _judge("layouts", x, t, dtype, ld=1013, start=3, inplace=inplace)
        whole = torch.as_strided(xv, (3, 1013), (1013, 1))
        assert bool(torch.isnan(whole[:, 1001:]).all()), "the backward wrote into the padding"
        if inplace:
            assert g.data_ptr() == xv.data_ptr()
    wide = CR.layout(torch.cat([torch.full((3, 1), float("nan")), x], 1), dtype, device="cuda")
    sl = wide[:, 1:]                                                    # a column slice
    ref = CR.Ref(CR.stored(x, dtype), t)
    loss, g = _run(sl, t.cuda(), red="none")
    assert CR.worst(loss, *ref.reduced("none")) <= 1.0 and CR.worst(g, *ref.grad("none", 1.0)) <= 1.0
    assert bool(torch.isnan(wide[:, 0]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_positions(dtype):
    V, ld, start = CR.position_shape(dtype)
    for name, r, j, x, t, t_on in CR.position_cases(dtype):
        for tt in (t, t_on):
            _judge("positions", x, tt, dtype, ld=ld, start=start)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_values(dtype):
    for name, (x, t) in CR.value_cases(dtype).items():
        xv, loss, g = _judge("values/" + name, x, t, dtype)
        if name == "target_60_above":
            assert float(loss.abs().max()) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_targets(dtype):
    x, _ = CR.normal(7, 300, seed=9)
    t = torch.tensor([3, -100, 300, -1, 2 ** 40, 0, 299])
    for ii in (-100, 0):                                                # 0: a real class is ignored
        for red in ("mean", "sum", "none"):
            with guarded_allocations() as ledger:
                xv, loss, g = _judge("targets", x, t, dtype, ld=301, ii=ii, red=red)
            assert ledger.intact(), ledger.describe_damage()
        ref_all = CR.Ref(CR.stored(x, dtype), t, ii)                    # the reference itself: an ignored row is an absent row
        ref_absent = CR.Ref(CR.stored(x, dtype)[ref_all.valid], t[ref_all.valid], ii)
        assert abs(float(ref_all.reduced("mean")[0]) - float(ref_absent.reduced("mean")[0])) <= 1e-12
    t_none = torch.tensor([-100, 300, -1, 2 ** 40, -100, -7, 301])
    for red, check in (("mean", torch.isnan), ("sum", lambda v: v == 0)):
        xv, loss, g = _judge("targets", x, t_none, dtype, red=red, up=-3.5)
        assert bool(check(loss)) and bool((g == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reductions_and_upstream_gradients(dtype):
    x, t = CR.normal(5, 777, seed=10)
    t[1] = -100
    for red in ("mean", "sum"):
        for up in (None, -3.5):
            _judge("reductions", x, t, dtype, red=red, up=up)
    _judge("reductions", x, t, dtype, red="none", up=[1.5, 2.0, 0.0, -0.75, 3.0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bit_for_bit(dtype):
    x, t = CR.normal(5, 2 * CR.THREADS * CR.epv(dtype) + 5, seed=12)
    xv, tc = CR.layout(x, dtype, device="cuda"), t.cuda()
    for red in ("none", "mean"):
        a, b = _run(xv, tc, red=red), _run(xv, tc, red=red)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    rows, grads = _run(xv, tc, red="none")
    # a row alone against the same row in the batch, at the same place relative to 16 bytes (the head / vector / tail split, and
    # with it the order of the sums, follows the row's address)
    one = CR.layout(x[3:4], dtype, start=(3 * x.shape[1]) % CR.epv(dtype), device="cuda")
    r1, g1 = _run(one, tc[3:4], red="none")
    assert torch.equal(r1[0], rows[3]) and torch.equal(g1[0], grads[3])
    for red, up in (("mean", -3.5), ("none", None)):
        _, g_out = _run(xv, tc, red=red, up=up)
        _, g_in = _run(xv.clone(), tc, red=red, up=up, inplace=True)
        assert torch.equal(g_out, g_in)


def test_autograd_contract():
    from mop_amd import _lib, ops
    x, t = CR.normal(4, 500, seed=13)
    xc, tc = x.cuda(), t.cuda()
    ops.LAST_PATH.pop("cross_entropy_bwd", None)
    ops.cross_entropy(xc, tc)                                           # logits without grad: no backward is launched
    assert ops.LAST_PATH["cross_entropy_fwd"] == _lib.PATH_FUSED and "cross_entropy_bwd" not in ops.LAST_PATH
    leaf = xc.clone().requires_grad_()
    loss = ops.cross_entropy(leaf, tc)
    g1 = torch.autograd.grad(loss, leaf, retain_graph=True)[0]
    g2 = torch.autograd.grad(loss, leaf, retain_graph=True)[0]
    assert torch.equal(g1, g2)
    (g,) = torch.autograd.grad(loss, leaf, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    spent = ops.cross_entropy(xc.clone().requires_grad_(), tc, inplace_backward=True)
    spent.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="inplace_backward"):
        spent.backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ops.cross_entropy(leaf, tc).dtype == torch.float32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l2 = ops.cross_entropy(leaf, tc)
        gs = torch.autograd.grad(l2, leaf)[0]
    side.synchronize()
    assert torch.equal(l2, loss) and torch.equal(gs, g1)
    xh = xc.half().requires_grad_()                                     # fp16: the twin
    ops.cross_entropy(xh, tc).backward()
    assert ops.LAST_PATH["cross_entropy_fwd"] == _lib.PATH_GENERIC and xh.grad is not None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guarded_run(dtype):
    from mop_amd import _lib, ops
    x, t = CR.normal(3, 1029, seed=14)
    xs, tc = CR.stored(x, dtype).cuda(), t.cuda()
    plain = _run(xs, tc, red="mean")
    with guarded_allocations() as ledger:
        got = _run(embedded(xs), embedded(tc), red="mean")
        torch.cuda.synchronize()
        assert ledger.intact(), ledger.describe_damage()
    assert ledger.count() >= 3
    assert bool(torch.isfinite(got[0])) and bool(torch.isfinite(got[1]).all())
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    assert ops.LAST_PATH["cross_entropy_bwd"] == _lib.PATH_FUSED


# ---- linear_cross_entropy: against float64, held to twice the unchunked torch head's own error plus the kernel's bound ----
def _head_case(V, bias, seed=20, M=37, D=24):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    w = torch.randn(V, D, generator=g) * 0.3
    b = torch.randn(V, generator=g) * 0.1 if bias else None
    t = torch.randint(0, V, (M,), generator=g)
    t[5] = -100
    return x, w, b, t


def _head_grads(fn, x, w, b, t, autocast):
    leaves = [v.detach().clone().requires_grad_() for v in (x, w, b) if v is not None]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss = fn(leaves[0], leaves[1], t, leaves[2] if b is not None else None)
    grads = torch.autograd.grad(loss, leaves)
    torch.cuda.synchronize()
    return [loss.detach()] + [g.detach() for g in grads]


def _head_rule(x, w, b, t, autocast, got, whole):
    """every result's max error against float64 <= 2 x the unchunked head's + the kernel's bound carried through the GEMMs"""
    ldt = torch.bfloat16 if autocast else torch.float32
    x64, w64 = [CR.stored(v.cpu(), ldt).double().requires_grad_() for v in (x, w)]
    b64 = None if b is None else CR.stored(b.cpu(), ldt).double().requires_grad_()
    logits64 = F.linear(x64, w64, b64)
    loss64 = F.cross_entropy(logits64, t.cpu())
    leaves = [x64, w64] + ([] if b is None else [b64])
    want = [loss64.detach()] + list(torch.autograd.grad(loss64, leaves))
    ref = CR.Ref(CR.stored(logits64.detach().float(), ldt), t.cpu())
    gb = ref.grad("mean", 1.0)[1]
    bounds = [ref.reduced("mean")[1], gb @ w64.detach().abs(), gb.t() @ x64.detach().abs()] + ([] if b is None else [gb.sum(0)])
    ratios = []
    for name, g, wh, wa, bd in zip(("loss", "dx", "dW", "db"), got, whole, want, bounds):
        err, err_whole = float((g.double().cpu() - wa).abs().max()), float((wh.double().cpu() - wa).abs().max())
        lim = 2 * err_whole + float(torch.as_tensor(bd).max())
        ratios.append(err / lim if lim > 0 else 0.0)
        assert err <= lim, (name, err, err_whole, float(torch.as_tensor(bd).max()))
    return max(ratios)


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16-autocast"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("V", [1000, 8 * CR.THREADS + 3])
def test_linear_cross_entropy(V, bias, autocast):
    from mop_amd import _lib, ops
    x, w, b, t = [None if v is None else v.cuda() for v in _head_case(V, bias)]
    whole = _head_grads(lambda x_, w_, t_, b_: F.cross_entropy(F.linear(x_, w_, b_).float(), t_), x, w, b, t, autocast)
    for chunk in (1, 8, 37, 64):
        got = _head_grads(lambda x_, w_, t_, b_: ops.linear_cross_entropy(x_, w_, t_, b_, chunk_rows=chunk), x, w, b, t, autocast)
        assert ops.LAST_PATH["linear_cross_entropy"] == ops.LAST_PATH["cross_entropy_bwd"] == _lib.PATH_FUSED
        assert got[0].dtype == torch.float32 and [g.dtype for g in got[1:]] == [torch.float32] * (len(got) - 1)
        frac = _head_rule(x, w, b, t, autocast, got, whole)
        print(f"linear V={V} bias={bias} autocast={autocast} chunk={chunk}: {frac:.3f} of the limit")
        _note("linear", frac)


def test_linear_cross_entropy_contract():
    from mop_amd import ops
    x, w, b, t = [v.cuda() for v in _head_case(1000, True)]
    leaves = [v.clone().requires_grad_() for v in (x, w, b)]
    loss = ops.linear_cross_entropy(leaves[0].view(1, 37, 24), leaves[1], t.view(1, 37), leaves[2], chunk_rows=8)
    g1 = torch.autograd.grad(loss, leaves, retain_graph=True)
    g2 = torch.autograd.grad(loss, leaves, retain_graph=True)
    g3 = torch.autograd.grad(loss * -3.5, leaves)
    for a, a2, a3 in zip(g1, g2, g3):
        assert torch.equal(a, a2) and torch.equal(a3, a * -3.5)
    total = ops.linear_cross_entropy(x, w, t, b, reduction="sum", chunk_rows=8)     # no grad: forward only
    n = int(CR.counted(t, 1000, -100).sum())
    assert abs(float(total) / n - float(loss.detach())) <= 4 * CR.U * abs(float(loss.detach()))
    a = ops.linear_cross_entropy(x, w, t, b, chunk_rows=37)
    assert torch.equal(a, ops.cross_entropy(F.linear(x, w, b), t))      # one chunk: the op on the whole logits


def test_loss_peak_memory_is_below_forwards_by_an_fp32_logits_tensor():
    from mop_amd import ops
    M, D, V = 4096, 64, 8192
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, D, generator=g).cuda().requires_grad_()
    w = (torch.randn(V, D, generator=g) * 0.1).cuda().requires_grad_()
    t = torch.randint(0, V, (M,), generator=g).cuda()

    def peak(fn):
        x.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            fn().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    p_torch = peak(lambda: F.cross_entropy(F.linear(x, w).float(), t))
    p_loss = peak(lambda: ops.linear_cross_entropy(x, w, t, chunk_rows=M // 8))
    print(f"peak bytes: torch head + loss {p_torch}, linear_cross_entropy {p_loss}")
    assert p_torch - p_loss >= M * V * 4


# ---- the models ----
def _models():
    from mop_amd.nn import GPT_MoP, WhisperConfig, WhisperMoP
    from mop_amd.nn.quartet_attn_patch import TinyTransformerLM, TransformerConfig
    cfg = TransformerConfig(n_layer=2, n_head=2, n_embd=64, block_size=32, dropout=0.0, bias=True)
    g = torch.Generator().manual_seed(2)
    idx, tg = torch.randint(0, 211, (2, 16), generator=g).cuda(), torch.randint(0, 211, (2, 16), generator=g).cuda()
    tg[1, 4] = -100
    torch.manual_seed(0)
    mop = GPT_MoP(211, cfg, n_views=2, n_kernels=1).cuda()
    yield "gpt_mop", mop, (lambda: mop(idx, targets=tg)[1]), (lambda c: mop.loss(idx, tg, chunk_rows=c))
    lm = TinyTransformerLM(211, cfg).cuda()
    yield "quartet", lm, (lambda: lm(idx, targets=tg)[1]), (lambda c: lm.loss(idx, tg, chunk_rows=c))
    wh = WhisperMoP(WhisperConfig(n_mels=12, n_audio_ctx=64, vocab_size=211, n_text_ctx=16, n_embd=64, n_head=2, n_layer_enc=1,
                                  n_layer_dec=2, dropout=0.0)).cuda()
    mel = torch.randn(2, 40, 12, generator=g).cuda()
    yield "whisper", wh, (lambda: wh(mel, idx, tg)[1]), (lambda c: wh.loss(mel, idx, tg, chunk_rows=c)[0])


def test_models_loss_is_forwards_loss():
    """fp32 models, dropout off: the stack before the head runs the same deterministic kernels either way, so the two losses differ
    by the head alone: fp32 roundings in another order.  The loss is held to twice the row-loss bound of ce_rows.py at the models'
    V (both sides carry one), every parameter gradient to 1e-4 of its tensor's largest entry: the head's gradients agree to a few
    fp32 roundings of sums over V = 211 and M = 32 terms (~1e-6 relative), and the stack carries them on linearly.  A tensor whose
    gradient is zero by construction (a key bias under the softmax) holds rounding noise alone: as in gpu_util.check_grads, the
    scale of a tensor is at least 1e-3 of the model's largest gradient."""
    from mop_amd import _lib, ops
    for name, m, fwd, loss in _models():
        params = [p for p in m.parameters() if p.requires_grad]
        want = fwd()
        gw = torch.autograd.grad(want, params, allow_unused=True)
        gscale = max(float(b.abs().max()) for b in gw if b is not None)
        for chunk in (None, 5):
            got = loss(chunk)
            assert ops.LAST_PATH["linear_cross_entropy"] == ops.LAST_PATH["cross_entropy_fwd"] == _lib.PATH_FUSED, name
            gl = torch.autograd.grad(got, params, allow_unused=True)
            bound = 2 * CR.U * (4 * CR.depth(211, torch.float32) + 2 * math.log(211) + 2 * abs(float(want.detach())))
            assert abs(float(got.detach()) - float(want.detach())) <= bound, (name, float(got), float(want))
            for a, b in zip(gl, gw):
                assert (a is None) == (b is None)
                if a is not None:
                    assert float((a - b).abs().max()) <= 1e-4 * max(float(b.abs().max()), 1e-3 * gscale), name


def test_graph_replay_reproduces_eager():
    """ops.cross_entropy + backward and ops.linear_cross_entropy + backward captured on one stream and replayed on new logits and
    targets, in a process of their own (tools/graph_probe_cross_entropy.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_cross_entropy.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "CE_REPLAY_IDENTICAL True" in r.stdout, r.stdout[-800:]
    assert "LINEAR_REPLAY_WITHIN_RULE True" in r.stdout, r.stdout[-800:]


def test_report_the_fractions_used():
    for k in sorted(USED):
        print(f"largest fraction of the bound used, {k}: {USED[k]:.3f}")
