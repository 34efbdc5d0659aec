"""-m gpu: FusedAdamW on the HIP kernels (mopk_adamw_step) against the float64 statement and bounds of tests/optim_ref.py, its
bitwise properties, the norm, the skip and no-gradient rules, graph capture, guard bands, and five training steps of a small GPT."""
import pytest
import torch

import optim_cases as K
import optim_ref as R
from guarded_alloc import embedded, guarded_allocations
from mop_amd import _lib, ops
from mop_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
C = _lib.ADAMW_CHUNK
DEV = "cuda"
H = K.HYPER
# the largest loss difference between two torch runs of _gpt_steps that differ only in foreach against single-tensor mode, measured
# on an MI355X; FusedAdamW gets 4x that: it applies the clip in fp32 where torch rounds it into the gradient
E2E_TORCH_SPREAD = 4.768e-07       # one fp32 spacing of a loss in [4, 8)


def _fused(params, **kw):
    return FusedAdamW(params, lr=H["lr"], betas=(H["beta1"], H["beta2"]), eps=H["eps"], weight_decay=H["weight_decay"], **kw)


def _steps(params, gdt, n, grads_of=None, **kw):
    """n plain steps -> (optimiser, the parameters' values and states afterwards)"""
    opt = _fused(params, **kw)
    for s in range(n):
        for p, g in zip(params, (grads_of or K.grads_for)(params, gdt, s)):
            p.grad = g
        opt.step()
    ema = kw.get("ema_decay") is not None
    return opt, [K.state_of(opt, p, ema) for p in params]


def _same(a, b):
    return all(x["step"] == y["step"] and all(torch.equal(x[k], y[k]) for k in x if k != "step") for x, y in zip(a, b))


@pytest.mark.parametrize("max_grad_norm,ema_decay", [(None, None), (1.0, 0.99), (1e9, None)], ids=["plain", "clip_ema", "clip_inactive"])
def test_mixed_list_against_float64(max_grad_norm, ema_decay):
    params, gdt = K.mixed_list(DEV)
    assert params[-2].data_ptr() % 16 == 4 and params[-1].data_ptr() % 16 == 2          # the two views start off a boundary
    opt = _fused(params, max_grad_norm=max_grad_norm, ema_decay=ema_decay)
    shares = {}
    for s in range(3):
        sh = K.checked_step(opt, params, K.grads_for(params, gdt, s), hypers=[H] * len(params), max_grad_norm=max_grad_norm,
                            ema_decay=ema_decay, norm=(lambda: opt.grad_norm) if max_grad_norm is not None else None, what=f"step {s}")
        assert ops.LAST_PATH["adamw"] == _lib.PATH_FUSED
        shares = {k: max(shares.get(k, 0.0), v) for k, v in sh.items()}
    print("largest share of each bound:", shares)
    if max_grad_norm == 1e9:            # a norm below max_grad_norm gives exactly the no-clip result
        ref, gd = K.mixed_list(DEV)
        _, want = _steps(ref, gd, 3)
        assert _same([K.state_of(opt, p, False) for p in params], want)


def _flat_list(n_tensors, each, seed):
    """n_tensors tensors of `each` elements, views of one flat buffer that starts one element off a 16-byte boundary"""
    gen = torch.Generator().manual_seed(seed)
    flat = K.view_at(torch.randn(n_tensors * each, generator=gen).to(DEV), 1)
    grad = torch.randn(n_tensors * each, generator=gen).to(DEV)
    params = [torch.nn.Parameter(flat[i * each:(i + 1) * each]) for i in range(n_tensors)]
    return flat, grad, params, [grad[i * each:(i + 1) * each] for i in range(n_tensors)]


def test_many_tiny_tensors():
    """2 * (tensor capacity) + 1 eight-element tensors: three launches' worth, each starting off a 16-byte boundary"""
    n_tensors, each = 2 * _lib.ADAMW_MAX_TENSORS + 1, 8
    flat, grad, params, grads = _flat_list(n_tensors, each, 5)
    before = dict(p=flat.clone(), g=grad.clone(), m=torch.zeros_like(flat), v=torch.zeros_like(flat), ema=flat.clone())
    opt = _fused(params, max_grad_norm=1.0, ema_decay=0.9)
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()
    assert ops.LAST_PATH["adamw"] == _lib.PATH_FUSED
    ref, nb = R.ref_norm([grad]), R.norm_bound([grad], C)
    assert abs(float(opt.grad_norm) - ref) <= nb
    coef, eps_c = R.coef_and_eps(ref, 1.0, nb / ref)
    cat = lambda k: torch.cat([opt.state[p][k] for p in params])                 # noqa: E731
    R.check_step(before, dict(p=flat, m=cat("exp_avg"), v=cat("exp_avg_sq"), ema=cat("ema")), 0, coef=coef, eps_c=eps_c, hyper=H,
                 ema_decay=0.9, what=f"{n_tensors} x {each}")
    assert torch.equal(grad, before["g"]) and all(int(opt.state[p]["step"]) == 1 for p in params)
    # the documented launch count: S = 3 slices -> S + 1 for the norm, 2 S for the update
    groups = [dict(params=params, grads=grads, exp_avgs=[opt.state[p]["exp_avg"] for p in params],
                   exp_avg_sqs=[opt.state[p]["exp_avg_sq"] for p in params], steps=[opt.state[p]["step"] for p in params],
                   emas=[opt.state[p]["ema"] for p in params], lr=H["lr"], beta1=H["beta1"], beta2=H["beta2"], eps=H["eps"],
                   weight_decay=H["weight_decay"])]
    assert ops.adamw_launches(groups, max_grad_norm=1.0, ema_decay=0.9, stats=opt._stats) == 3 * 3 + 1


def test_one_chunk_more_than_a_launch_holds():
    """a list of (chunk capacity) + 1 chunks: the big tensor's last chunk travels in a second launch.  The float64 check reads
    the elements around every boundary and a strided sample (the whole tensor in float64 would take seconds on the host); the
    whole tensor is compared bit for bit with the same values updated as two tensors cut at the launch boundary."""
    n = (_lib.ADAMW_MAX_CHUNKS - 1) * C + 1        # with the 5-element tensor's chunk: capacity + 1 chunks
    gen = torch.Generator().manual_seed(6)
    small = torch.randn(5, generator=gen).to(DEV)
    vals, grad = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    big = [torch.nn.Parameter(small.clone()), torch.nn.Parameter(vals.clone())]
    opt = _fused(big, max_grad_norm=1e9)
    big[0].grad, big[1].grad = torch.ones(5, device=DEV), grad
    opt.step()
    assert ops.LAST_PATH["adamw"] == _lib.PATH_FUSED and int(opt.state[big[1]]["step"]) == 1
    ref, nb = R.ref_norm([big[0].grad, grad]), R.norm_bound([big[0].grad, grad], C)
    assert abs(float(opt.grad_norm) - ref) <= nb
    cut = (_lib.ADAMW_MAX_CHUNKS - 1) * C          # the first launch holds the 5-element tensor's chunk and this many elements
    idx = torch.cat([torch.arange(0, 2 * C), torch.arange(cut - 2 * C, n), torch.arange(0, n, 4099)]).to(DEV)
    st = opt.state[big[1]]
    z = torch.zeros(idx.numel(), device=DEV)
    R.check_step(dict(p=vals[idx], g=grad[idx], m=z, v=z), dict(p=big[1][idx], m=st["exp_avg"][idx], v=st["exp_avg_sq"][idx]), 0,
                 hyper=H, what="chunk capacity + 1")
    parts = [torch.nn.Parameter(vals[:cut].clone()), torch.nn.Parameter(vals[cut:].clone())]
    opt2 = _fused(parts)
    parts[0].grad, parts[1].grad = grad[:cut].clone(), grad[cut:].clone()
    opt2.step()
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(st[k], torch.cat([opt2.state[p][k] for p in parts]))
    assert torch.equal(big[1].detach(), torch.cat([p.detach() for p in parts])) and torch.equal(grad, torch.cat([p.grad for p in parts]))


def test_bitwise_properties():
    params, gdt = K.mixed_list(DEV)
    _, a = _steps(params, gdt, 2, max_grad_norm=1.0, ema_decay=0.9)
    params2, _ = K.mixed_list(DEV)
    _, b = _steps(params2, gdt, 2, max_grad_norm=1.0, ema_decay=0.9)
    assert _same(a, b), "two runs differ"
    # without clipping, a tensor updated inside the long list equals the same tensor updated alone
    params3, _ = K.mixed_list(DEV)
    _, whole = _steps(params3, gdt, 2, ema_decay=0.9)
    fresh, _ = K.mixed_list(DEV)
    for i in range(len(fresh)):
        one = lambda ps, gd, s, i=i: [K.grads_for(params3, gdt, s)[i]]             # noqa: E731
        _, alone = _steps([fresh[i]], [gdt[i]], 2, grads_of=one, ema_decay=0.9)
        assert _same(alone, [whole[i]]), f"tensor {i} (n = {fresh[i].numel()}) alone differs from itself in the list"
    # the unaligned views equal aligned copies, with clipping too (the gradients are the same tensors)
    views, _ = K.mixed_list(DEV)
    copies, _ = K.mixed_list(DEV)
    copies[-2], copies[-1] = (torch.nn.Parameter(p.detach().clone()) for p in copies[-2:])
    assert copies[-2].data_ptr() % 16 == 0 and copies[-1].data_ptr() % 16 == 0 and views[-1].data_ptr() % 16 != 0
    _, x = _steps(views, gdt, 2, max_grad_norm=1.0, ema_decay=0.9)
    _, y = _steps(copies, gdt, 2, max_grad_norm=1.0, ema_decay=0.9)
    assert _same(x, y), "a view that starts off a 16-byte boundary differs from its aligned copy"


def _norm_of(grads, **kw):
    params = [torch.nn.Parameter(torch.ones_like(g, dtype=F32)) for g in grads]
    for p, g in zip(params, grads):
        if g.dtype != p.dtype:
            p.grad_dtype = g.dtype
    opt = _fused(params, **kw)
    for p, g in zip(params, grads):
        p.grad = g
    keep = [p.detach().clone() for p in params]
    opt.step()
    return opt, params, keep


def test_norm_special_values():
    gen = torch.Generator().manual_seed(9)
    base = [torch.randn(n, generator=gen).to(DEV) for n in (C + 3, 50, 2 * C)]
    for bad in (float("inf"), float("nan")):
        grads = [g.clone() for g in base]
        grads[2][C + 17] = bad
        opt, params, keep = _norm_of(grads, max_grad_norm=1.0, skip_nonfinite=True)
        n = float(opt.grad_norm)
        assert (n == float("inf")) if bad == float("inf") else (n != n)
        assert int(opt.skipped_steps) == 1 and all(torch.equal(p, k) for p, k in zip(params, keep))
        assert all(int(opt.state[p]["step"]) == 0 for p in params)
    # magnitudes 1e-30 and 1e18 in one set: 64 squares of 1e18 sum to 6.4e37, inside fp32; the squares of 1e-30 vanish in both
    grads = [torch.full((C + 3,), 1e-30, device=DEV), torch.full((64,), 1e18, device=DEV), torch.full((2 * C,), -1e-30, device=DEV).to(BF16)]
    opt, _, _ = _norm_of(grads, max_grad_norm=1.0)
    ref, nb = R.ref_norm(grads), R.norm_bound(grads, C)
    assert abs(float(opt.grad_norm) - ref) <= nb and ref > 7e18
    grads = [torch.full((3 * C + 1,), 1e-30, device=DEV)]
    opt, _, _ = _norm_of(grads, max_grad_norm=1.0)
    assert abs(float(opt.grad_norm) - R.ref_norm(grads)) <= R.norm_bound(grads, C)


def test_skip_and_no_gradient_rules():
    params, gdt = K.mixed_list(DEV)
    opt = _fused(params, max_grad_norm=1.0, ema_decay=0.9, skip_nonfinite=True)
    for s in range(5):
        grads = K.grads_for(params, gdt, s)
        if s in (1, 2):
            grads[9] = None
        if s == 2:
            grads[12][5] = float("inf")
            before = [K.state_of(opt, p, True) for p in params]
            for p, g in zip(params, grads):
                p.grad = g
            opt.step()
            assert _same([K.state_of(opt, p, True) for p in params], before) and int(opt.skipped_steps) == 1
        else:
            K.checked_step(opt, params, grads, hypers=[H] * len(params), max_grad_norm=1.0, ema_decay=0.9, norm=lambda: opt.grad_norm,
                           what=f"step {s}")
    assert int(opt.skipped_steps) == 1
    assert [int(opt.state[p]["step"]) for p in params] == [3 if i == 9 else 4 for i in range(len(params))]


def test_last_path_and_param_groups():
    a = [torch.nn.Parameter(torch.randn(100, device=DEV)), torch.nn.Parameter(torch.randn(C + 1, device=DEV).to(BF16))]
    b = [torch.nn.Parameter(torch.randn(77, device=DEV))]
    hb = dict(lr=1e-4, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.0)
    opt = FusedAdamW([dict(params=a), dict(params=b, lr=hb["lr"], betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)], lr=H["lr"],
                     betas=(H["beta1"], H["beta2"]), eps=H["eps"], weight_decay=H["weight_decay"], max_grad_norm=0.5)
    for s in range(2):
        K.checked_step(opt, a + b, K.grads_for(a + b, [F32, BF16, F32], s), hypers=[H, H, hb], max_grad_norm=0.5, norm=lambda: opt.grad_norm)
        assert ops.LAST_PATH["adamw"] == _lib.PATH_FUSED
    half = [torch.nn.Parameter(torch.randn(64, device=DEV).half()), torch.nn.Parameter(torch.randn(64, device=DEV))]
    opt = _fused(half)
    for p in half:
        p.grad = torch.randn_like(p)
    opt.step()
    assert ops.LAST_PATH["adamw"] == _lib.PATH_GENERIC and int(opt.state[half[0]]["step"]) == 1


def test_captured_step_equals_eager_steps():
    def setup():
        params, gdt = K.mixed_list(DEV)
        lr = torch.tensor([H["lr"]], device=DEV)
        opt = FusedAdamW(params, lr=lr, betas=(H["beta1"], H["beta2"]), eps=H["eps"], weight_decay=H["weight_decay"], max_grad_norm=1.0,
                         ema_decay=0.9)
        for p, g in zip(params, K.grads_for(params, gdt, 0)):
            p.grad = g
        opt.step()                          # warm-up: state, workspace and stats exist before the capture
        return params, gdt, lr, opt

    params, gdt, lr, opt = setup()
    for s in (1, 2, 3):
        for p, g in zip(params, K.grads_for(params, gdt, s)):
            p.grad.copy_(g)
        lr.fill_(H["lr"] / s)
        opt.step()
    eager = [K.state_of(opt, p, True) for p in params]

    params, gdt, lr, opt = setup()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    before = [K.state_of(opt, p, True) for p in params]
    try:
        with torch.cuda.graph(graph):
            opt.step()
    except RuntimeError as e:
        if "not permitted when stream is capturing" in str(e) or "StreamCaptureUnsupported" in str(e):
            pytest.skip(f"the runtime refused the capture: {e}")
        raise
    assert ops.LAST_PATH["adamw"] == _lib.PATH_FUSED
    assert _same([K.state_of(opt, p, True) for p in params], before), "capturing ran the step"
    for s in (1, 2, 3):
        for p, g in zip(params, K.grads_for(params, gdt, s)):
            p.grad.copy_(g)
        lr.fill_(H["lr"] / s)
        graph.replay()
    torch.cuda.synchronize()
    replayed = [K.state_of(opt, p, True) for p in params]
    assert all(x["step"] == 4 for x in replayed) and _same(replayed, eager)


def test_guard_bands_stay_intact():
    def run(embed):
        params, gdt = K.mixed_list(DEV)
        if embed:
            params = [torch.nn.Parameter(embedded(p.detach()) if p.numel() else p.detach()) for p in params[:-2]]
            gdt = gdt[:-2]
            for p, d in zip(params, gdt):
                if d != p.dtype:
                    p.grad_dtype = d
        else:
            params = params[:-2]
            gdt = gdt[:-2]
        opt = _fused(params, max_grad_norm=1.0, ema_decay=0.9, skip_nonfinite=True)
        for s in range(2):
            for p, g in zip(params, K.grads_for(params, gdt, s)):
                p.grad = embedded(g) if embed and g.numel() else g
            opt.step()
        torch.cuda.synchronize()
        return [K.state_of(opt, p, True) for p in params], float(opt.grad_norm)

    plain, n0 = run(False)
    with guarded_allocations() as ledger:
        guarded, n1 = run(True)
        torch.cuda.synchronize()
    assert ledger.intact(), ledger.describe_damage()
    assert ledger.count() > 0 and n0 == n1 and _same(plain, guarded)
    assert all(bool(torch.isfinite(x[k].float()).all()) for x in guarded for k in ("p", "m", "v", "ema"))


def _gpt_steps(make_opt, after_step=None, steps=5):
    from mop_amd.nn import GPT_MoP
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    cfg = TransformerConfig(n_layer=2, n_head=2, n_embd=64, block_size=32, dropout=0.0, bias=True)
    torch.manual_seed(0)
    m = GPT_MoP(128, cfg, n_views=2, n_kernels=1).to(DEV)
    gen = torch.Generator().manual_seed(4)
    idx, tg = torch.randint(0, 128, (4, 32), generator=gen).to(DEV), torch.randint(0, 128, (4, 32), generator=gen).to(DEV)
    opt = make_opt(m)
    ema = [p.detach().clone() for p in m.parameters()]
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = m.loss(idx, tg)
        loss.backward()
        if after_step is None:
            opt.step()
        else:
            after_step(m, opt, ema)
        losses.append(float(loss))
    return losses, [p.detach().clone() for p in m.parameters()], ema


def _torch_step(m, opt, ema):
    """the reference drivers' step: clip_grad_norm_, AdamW, the EMA loop"""
    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    with torch.no_grad():
        for e, p in zip(ema, m.parameters()):
            e.mul_(0.99).add_(p.detach(), alpha=0.01)


def gpt_curves():
    """(torch single-tensor, torch foreach, fused) loss curves, final weights and EMAs of the five-step run"""
    kw = dict(lr=3e-3, weight_decay=0.05)
    single = _gpt_steps(lambda m: torch.optim.AdamW(m.parameters(), foreach=False, **kw), _torch_step)
    foreach = _gpt_steps(lambda m: torch.optim.AdamW(m.parameters(), foreach=True, **kw), _torch_step)
    fused_opt = []

    def make(m):
        fused_opt.append(FusedAdamW(m.parameters(), max_grad_norm=1.0, ema_decay=0.99, **kw))
        return fused_opt[0]
    l, w, _ = _gpt_steps(make)
    return single, foreach, (l, w, fused_opt[0].ema_parameters())


def test_gpt_training_steps_follow_torch():
    single, foreach, fused = gpt_curves()
    assert ops.LAST_PATH["adamw"] == _lib.PATH_FUSED
    spread = max(abs(a - b) for a, b in zip(single[0], foreach[0]))
    diff = max(abs(a - b) for a, b in zip(single[0], fused[0]))
    print(f"loss curve: torch single-tensor {single[0]}, spread against foreach {spread:.3e}, fused against single-tensor {diff:.3e}")
    assert E2E_TORCH_SPREAD is not None, "the torch spread has not been measured on an MI355X yet"
    assert diff <= 4 * E2E_TORCH_SPREAD, (diff, E2E_TORCH_SPREAD)
    assert single[0][-1] < single[0][0] and fused[0][-1] < fused[0][0]
