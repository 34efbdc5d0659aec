"""FusedAdamW without a GPU: the class on CPU parameters (ops.adamw_step_torch) against the float64 statement of tests/optim_ref.py,
torch's own AdamW against the same bounds on the lists the GPU test uses, checkpoints, the EMA swap, refused arguments, the
schedule factory, and the library's size queries and constants."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

import optim_cases as K
import optim_ref as R
from conftest import ROOT
from mop_amd import _lib, ops, training
from mop_amd.optim import FusedAdamW

F32, BF16 = torch.float32, torch.bfloat16


def _two_groups(seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = [torch.nn.Parameter(torch.randn(33, 5, generator=gen)), torch.nn.Parameter(torch.randn(17, generator=gen).to(BF16))]
    b = [torch.nn.Parameter(torch.randn(64, generator=gen)), torch.nn.Parameter(torch.randn(3, 3, generator=gen))]
    ga = dict(params=a, lr=2e-3, weight_decay=0.1)
    gb = dict(params=b, lr=5e-4, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)
    ha = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
    hb = dict(lr=5e-4, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.0)
    return a + b, [ga, gb], [ha, ha, hb, hb]


@pytest.mark.parametrize("max_grad_norm", [None, 0.5, 1e6], ids=["noclip", "clip_active", "clip_inactive"])
@pytest.mark.parametrize("ema_decay", [None, 0.98], ids=["noema", "ema"])
def test_cpu_trajectory_against_float64(max_grad_norm, ema_decay):
    """5 steps: weight decay, two groups with their own hyper-parameters, a parameter without a gradient on steps 2 and 3"""
    params, groups, hypers = _two_groups()
    opt = FusedAdamW(groups, max_grad_norm=max_grad_norm, ema_decay=ema_decay)
    gdt = [p.dtype for p in params]
    for s in range(5):
        grads = K.grads_for(params, gdt, s)
        if s in (1, 2):
            grads[2] = None
        K.checked_step(opt, params, grads, hypers=hypers, max_grad_norm=max_grad_norm, ema_decay=ema_decay,
                       norm=(lambda: opt.grad_norm) if max_grad_norm is not None else None, what=f"step {s}")
    assert ops.LAST_PATH["adamw"] == _lib.PATH_GENERIC
    assert [int(opt.state[p]["step"]) for p in params] == [5, 5, 3, 5]
    assert all(opt.state[p]["exp_avg"].dtype == F32 and opt.state[p]["exp_avg_sq"].dtype == F32 for p in params)
    if max_grad_norm == 1e6:            # a norm below max_grad_norm: exactly the no-clip trajectory
        ref_params, ref_groups, _ = _two_groups()
        ref = FusedAdamW(ref_groups, ema_decay=ema_decay)
        for s in range(5):
            grads = K.grads_for(ref_params, gdt, s)
            for i, (p, g) in enumerate(zip(ref_params, grads)):
                p.grad = None if (s in (1, 2) and i == 2) else g
            ref.step()
        assert all(torch.equal(a, b) for a, b in zip(params, ref_params))


def test_cpu_skip_nonfinite_leaves_everything_untouched():
    params, groups, hypers = _two_groups()
    opt = FusedAdamW(groups, max_grad_norm=1.0, ema_decay=0.9, skip_nonfinite=True)
    gdt = [p.dtype for p in params]
    for s in range(5):
        grads = K.grads_for(params, gdt, s)
        if s == 2:
            grads[1][3] = float("inf")
            before = [K.state_of(opt, p, True) for p in params]
            for p, g in zip(params, grads):
                p.grad = g
            opt.step()
            for p, b in zip(params, before):
                a = K.state_of(opt, p, True)
                assert a["step"] == b["step"] and all(torch.equal(a[k], b[k]) for k in ("p", "m", "v", "ema"))
            assert int(opt.skipped_steps) == 1 and not torch.isfinite(opt.grad_norm)
        else:
            K.checked_step(opt, params, grads, hypers=hypers, max_grad_norm=1.0, ema_decay=0.9, norm=lambda: opt.grad_norm, what=f"step {s}")
    assert int(opt.skipped_steps) == 1 and [int(opt.state[p]["step"]) for p in params] == [4] * 4


@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["plain", "clip"])
def test_torch_adamw_meets_the_same_bounds_on_the_gpu_tests_lists(max_grad_norm):
    """the bounds can be met: torch.optim.AdamW in fp32, alone and behind clip_grad_norm_, on every list of test_gpu_optim.py"""
    params, gdt = K.mixed_list("cpu")
    shares = K.torch_reference_alone(params, gdt, 3, max_grad_norm)
    print("torch fp32 AdamW, largest share of each bound:", shares)
    tiny = [torch.nn.Parameter(torch.randn(8)) for _ in range(2 * _lib.ADAMW_MAX_TENSORS + 1)]
    K.torch_reference_alone(tiny, [F32] * len(tiny), 1, max_grad_norm)


def test_state_dict_round_trip_with_torch_adamw():
    def make(cls, **kw):
        gen = torch.Generator().manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(40, generator=gen)), torch.nn.Parameter(torch.randn(6, 7, generator=gen))]
        return ps, cls(ps, lr=1e-2, weight_decay=0.1, **kw)

    def run(ps, opt, steps, first=0):
        for s in range(first, first + steps):
            for p, g in zip(ps, K.grads_for(ps, [F32, F32], s)):
                p.grad = g
            opt.step()

    pf, fused = make(FusedAdamW)
    pt, plain = make(torch.optim.AdamW)
    run(pf, fused, 2)
    run(pt, plain, 2)
    # fused -> torch: torch continues from our state as it continues from its own, within fp32 rounding of one step
    p2, plain2 = make(torch.optim.AdamW)
    plain2.load_state_dict(copy.deepcopy(fused.state_dict()))        # torch's loader keeps the tensors it is given
    with torch.no_grad():
        for a, b in zip(p2, pf):
            a.copy_(b)
    run(p2, plain2, 1, first=2)
    run(pf, fused, 1, first=2)
    for a, b in zip(p2, pf):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
    assert int(plain2.state[p2[0]]["step"]) == 3
    # torch -> fused, arriving in bf16 and float64: the moments become fp32
    sd = copy.deepcopy(plain.state_dict())
    sd["state"][0]["exp_avg"] = sd["state"][0]["exp_avg"].to(BF16)
    sd["state"][1]["exp_avg_sq"] = sd["state"][1]["exp_avg_sq"].double()
    p3, fused3 = make(FusedAdamW)
    fused3.load_state_dict(sd)
    assert all(fused3.state[p][k].dtype == F32 for p in p3 for k in ("exp_avg", "exp_avg_sq", "step"))
    assert torch.equal(fused3.state[p3[1]]["exp_avg_sq"], plain.state[pt[1]]["exp_avg_sq"])
    with torch.no_grad():
        for a, b in zip(p3, pt):
            a.copy_(b)
    sd1 = plain.state_dict()
    p4, fused4 = make(FusedAdamW)
    fused4.load_state_dict(sd1)
    with torch.no_grad():
        for a, b in zip(p4, pt):
            a.copy_(b)
    run(p4, fused4, 1, first=2)
    run(pt, plain, 1, first=2)
    for a, b in zip(p4, pt):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
    assert int(fused4.state[p4[0]]["step"]) == 3


def test_fp32_moments_of_a_bf16_parameter_survive_our_own_checkpoint(tmp_path):
    m = torch.nn.Linear(8, 4).to(BF16)
    opt = FusedAdamW(m.parameters(), lr=1e-2, ema_decay=0.9)
    m(torch.randn(3, 8).to(BF16)).float().sum().backward()
    opt.step()
    training.save_checkpoint(m, opt, 1, 0.5, str(tmp_path / "c.pt"))
    m2 = torch.nn.Linear(8, 4).to(BF16)
    opt2 = FusedAdamW(m2.parameters(), lr=1e-2, ema_decay=0.9)
    training.load_checkpoint(m2, opt2, str(tmp_path / "c.pt"))
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
        for k in ("step", "exp_avg", "exp_avg_sq", "ema"):
            assert opt2.state[b][k].dtype == opt.state[a][k].dtype and torch.equal(opt2.state[b][k], opt.state[a][k])


def test_swap_ema_restores_bit_exact_parameters():
    params, groups, _ = _two_groups()
    opt = FusedAdamW(groups, ema_decay=0.5)
    for s in range(2):
        for p, g in zip(params, K.grads_for(params, [p.dtype for p in params], s)):
            p.grad = g
        opt.step()
    w = [p.detach().clone() for p in params]
    e = [x.clone() for x in opt.ema_parameters()]
    assert not torch.equal(w[0], e[0])
    with opt.swap_ema():
        assert all(torch.equal(p, x) for p, x in zip(params, e))
        assert all(torch.equal(x, y) for x, y in zip(opt.ema_parameters(), w))
    assert all(torch.equal(p, x) for p, x in zip(params, w))
    assert all(torch.equal(x, y) for x, y in zip(opt.ema_parameters(), e))
    with pytest.raises(RuntimeError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(2))]).ema_parameters()


def test_refused_arguments_raise_value_error():
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError):
        FusedAdamW(p, amsgrad=True)
    with pytest.raises(ValueError):
        FusedAdamW(p, maximize=True)
    with pytest.raises(ValueError):
        FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.complex64))])
    with pytest.raises(ValueError):
        FusedAdamW(p, max_grad_norm=0.0)
    emb = torch.nn.Embedding(10, 3, sparse=True)
    opt = FusedAdamW(emb.parameters())
    emb(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(ValueError):
        opt.step()


def test_make_optimizer_and_schedule_default_and_fused():
    def lrs(**kw):
        m = torch.nn.Linear(4, 4)
        opt, sched = training.make_optimizer_and_schedule(m, 1e-3, 0.05, 20, warmup_frac=0.2, **kw)
        out = []
        for _ in range(20):
            m(torch.ones(2, 4)).sum().backward()
            opt.step()
            sched.step()
            out.append(opt.param_groups[0]["lr"])
        return opt, out

    plain, a = lrs()
    fused, b = lrs(fused=True, max_grad_norm=1.0, ema_decay=0.99)
    assert type(plain) is torch.optim.AdamW and isinstance(fused, FusedAdamW)
    assert a == b
    with pytest.raises(ValueError):
        training.make_optimizer_and_schedule(torch.nn.Linear(2, 2), 1e-3, 0.0, 5, max_grad_norm=1.0)


def _fake_tensors(sizes):
    t = (_lib.OptimTensor * len(sizes))()
    for i, n in enumerate(sizes):                      # addresses that are never read: the queries look at counts and alignment only
        t[i].p, t[i].g, t[i].m, t[i].v, t[i].step, t[i].n = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, n
    return t


@pytest.mark.parametrize("sizes", [[2 ** 31 - 1], [2 ** 31 + 5], [2 ** 32 + 1], [2 ** 31, 2 ** 31, 7], [2 ** 30] * 5 + [0, 1]])
def test_size_queries_across_2_31_and_2_32_elements(sizes):
    from mop_amd import build
    build.build_lib()
    lib, t = _lib.lib(), _fake_tensors(sizes)
    a = _lib.AdamWArgs()
    a.n_tensors, a.phases = len(sizes), _lib.ADAMW_NORM | _lib.ADAMW_UPDATE
    chunks = sum(-(-n // _lib.ADAMW_CHUNK) for n in sizes)
    assert lib.mopk_adamw_supported(C.byref(a), t) == 1
    assert lib.mopk_adamw_workspace_bytes(C.byref(a), t) == -(-chunks * 4 // 256) * 256
    # the documented launch count: slices filled greedily by tensor parts and chunks
    S = nt = nc = 0
    for n in sizes:
        rem = -(-n // _lib.ADAMW_CHUNK)
        while True:
            if nt == _lib.ADAMW_MAX_TENSORS or nc == _lib.ADAMW_MAX_CHUNKS:
                S, nt, nc = S + 1, 0, 0
            take = min(rem, _lib.ADAMW_MAX_CHUNKS - nc)
            nt, nc, rem = nt + 1, nc + take, rem - take
            if rem == 0:
                break
    S += nt > 0
    assert lib.mopk_adamw_launches(C.byref(a), t) == 3 * S + 1
    z = (_lib.OptimTensor * 1)()                       # an empty tensor: torch hands out a null data_ptr(); only the step is needed
    z[0].step, a.n_tensors = 0x50000, 1
    assert lib.mopk_adamw_supported(C.byref(a), z) == 1 and lib.mopk_adamw_launches(C.byref(a), z) == 2
    z[0].step = 0
    assert lib.mopk_adamw_supported(C.byref(a), z) == 0
    a.n_tensors = len(sizes)
    t[0].n = -1
    assert lib.mopk_adamw_supported(C.byref(a), t) == 0
    t[0].n, t[0].p_dtype = sizes[0], 2
    assert lib.mopk_adamw_supported(C.byref(a), t) == 0
    t[0].p_dtype, t[0].m = 0, 0x30002
    assert lib.mopk_adamw_supported(C.byref(a), t) == 0
    assert lib.mopk_adamw_step(None, None, None) < 0


def test_header_constants_have_their_twins():
    src = open(os.path.join(ROOT, "include", "mopk.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define\s+(MOPK_ADAMW_\w+)\s+(\d+)", src)}
    assert got == {"MOPK_ADAMW_CHUNK": _lib.ADAMW_CHUNK, "MOPK_ADAMW_MAX_TENSORS": _lib.ADAMW_MAX_TENSORS,
                   "MOPK_ADAMW_MAX_CHUNKS": _lib.ADAMW_MAX_CHUNKS, "MOPK_ADAMW_NORM": _lib.ADAMW_NORM, "MOPK_ADAMW_UPDATE": _lib.ADAMW_UPDATE}
