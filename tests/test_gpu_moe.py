"""-m gpu: the top-1 routed MoE MLP (mopk_moe_*) on the MI355X.  Parity with the reference's fixtures (MoEMLP, a skewed route with
an idle expert, BlockMoE, ViT_MoP(use_moe=True)): routes equal, outputs <= 1e-3 (fp32) / 1e-2 (bf16), gradients within the
check_grads tolerances, no gradient for the gate and exact zeros for an expert without tokens.  An op sweep against float64 torch
over tile-edge token counts, widths, expert counts (to the 64 cap), skewed and balanced routes, fp32 / bf16 / autocast, with and
without the residual; the torch path for shapes the kernels refuse; bitwise reproducibility; no host sync; HIP-graph replay."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_names, load_golden
from gpu_util import check_grads, max_abs, rel_err

pytestmark = pytest.mark.gpu
TOL = {"fp32": (1e-3, 1e-3), "bf16": (1e-2, 3e-2)}
MOE = golden_names("moe_")
BF16_MARGIN = 0.03      # fixtures whose every token clears this margin in the reference's fp32 and bf16 runs


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _build(d, meta):
    """the fixture's module: parameters from the numpy stream of tests/vit_fixture.py, then the stored (perturbed) gate tensors"""
    from vit_fixture import fill_params
    from mop_amd.nn import ViT_MoP
    from mop_amd.nn.components import BlockMoE, MoEMLP
    kind = str(meta["kind"])
    if kind == "moe_mlp":
        m = MoEMLP(int(meta["dim"]), float(meta["mlp_ratio"]), int(meta["num_experts"]))
    elif kind == "block_moe":
        m = BlockMoE(int(meta["dim"]), int(meta["heads"]), float(meta["mlp_ratio"]), num_experts=int(meta["num_experts"]))
    else:
        m = ViT_MoP(dim=int(meta["dim"]), depth=int(meta["depth"]), heads=int(meta["heads"]), n_classes=int(meta["n_classes"]),
                    n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]), drop_path=0.0, use_moe=True,
                    moe_experts=int(meta["moe_experts"]))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = {k: torch.from_numpy(np.asarray(v)).reshape(shapes[k]) for k, v in fill_params(shapes, int(meta["param_seed"])).items()}
    sd.update({k[6:]: torch.from_numpy(d[k]) for k in d if k.startswith("param:")})
    m.load_state_dict(sd, strict=True)
    assert sum(p.numel() for p in m.parameters()) == int(meta["n_params"])
    return m.cuda().eval()


def _watch_routes(m):
    """route of every MoEMLP's input, from the kernels' own route entry point (ops.moe_route), keyed by module name"""
    from mop_amd import ops
    from mop_amd.nn.components import MoEMLP
    got, hs = {}, []
    for n, mod in m.named_modules():
        if isinstance(mod, MoEMLP):
            hs.append(mod.register_forward_pre_hook(
                lambda mod_, inp, n=n: got.__setitem__(n, ops.moe_route(inp[0], mod_.gate.weight, mod_.gate.bias).cpu().numpy())))
    return got, hs


def _fixture_run(name, prec):
    import mop_amd
    from mop_amd import _lib, ops
    d, _, gref, meta = load_golden(name)
    m = _build(d, meta)
    vit = str(meta["kind"]) == "vit_mop_moe"
    dtype = torch.float32
    if prec == "bf16":
        if vit:
            mop_amd.set_precision("bf16")
        else:
            dtype = torch.bfloat16
            m = m.to(dtype)
    routes, hooks = _watch_routes(m)
    x = torch.from_numpy(d["x"]).cuda().to(dtype).requires_grad_(True)
    y = m(x)
    y.backward(torch.from_numpy(d["w"]).cuda().to(dtype))
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert ops.LAST_PATH["moe_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["moe_bwd"] == _lib.PATH_FUSED
    return d, gref, meta, m, x, y, routes


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", MOE)
def test_moe_modules_vs_reference_golden(name, prec):
    """MoEMLP / BlockMoE against the reference: identical routes, output, dx and every gradient; the gate gets none"""
    d, gref, meta, m, x, y, routes = _fixture_run(name, prec)
    assert float(meta["min_margin"]) >= BF16_MARGIN
    for k in (k for k in d if k.startswith("route:")):
        assert np.array_equal(routes[k[6:]], d[k]), f"route of {k[6:]!r}: {int((routes[k[6:]] != d[k]).sum())} tokens differ"
    tol, gtol = TOL[prec]
    yv = y.detach().float().cpu().numpy()
    assert max_abs(yv, d["y"]) <= tol * max(1.0, float(np.abs(d["y"]).max())), f"y {max_abs(yv, d['y']):.3e}"
    none = {k[9:] for k in d if k.startswith("gradnone:")}
    params = dict(m.named_parameters())
    assert none == {k for k, p in params.items() if p.grad is None}, "gate.weight / gate.bias must get no gradient"
    grads = {k: p.grad.detach().float().cpu().numpy() for k, p in params.items() if p.grad is not None}
    gr = {k: v for k, v in gref.items() if k not in none}
    gr["dx"] = d["dx"]
    grads["dx"] = x.grad.detach().float().cpu().numpy()
    check_grads(grads, gr, gtol, d=d if prec == "bf16" else None)
    # an expert without tokens: gradients of exact zeros (not None)
    for k, r in (kv for kv in d.items() if kv[0].startswith("route:")):
        pre = k[6:] + "." if k[6:] else ""
        for e in set(range(int(meta["num_experts"]))) - set(r.tolist()):
            for fc in ("fc1", "fc2"):
                g = params[f"{pre}{fc}.{e}.weight"].grad
                assert g is not None and not bool(g.any()), f"{pre}{fc}.{e} got tokens-free gradient {g.abs().max()}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", golden_names("moevit_"))
def test_vit_mop_use_moe_vs_reference_golden(name, prec):
    """ViT_MoP(use_moe=True) end to end: routes of every block, logits, dx and the sampled gradients (tests/vit_fixture.py); the
    fp32-only margin case (configs[0] dims) is held in bf16 to >= 99 % route agreement and finite values"""
    from vit_fixture import grad_sample
    d, _, meta, m, x, y, routes = _fixture_run(name, prec)
    margin_ok = float(meta["min_margin"]) >= BF16_MARGIN
    yv = y.detach().float().cpu().numpy()
    if prec == "bf16" and not margin_ok:
        agree = np.mean(np.concatenate([routes[k[6:]] == d[k] for k in d if k.startswith("route:")]))
        assert agree >= 0.99, f"route agreement {agree:.4f}"
        assert np.isfinite(yv).all() and np.isfinite(x.grad.float().cpu().numpy()).all()
        return
    for k in (k for k in d if k.startswith("route:")):
        assert np.array_equal(routes[k[6:]], d[k]), f"route of {k[6:]}: {int((routes[k[6:]] != d[k]).sum())} tokens differ"
    tol, gtol = TOL[prec]
    assert max_abs(yv, d["y"]) <= tol, f"logits {max_abs(yv, d['y']):.3e}"
    assert rel_err(x.grad.float().cpu().numpy(), d["dx"]) <= gtol, f"dx {rel_err(x.grad.float().cpu().numpy(), d['dx']):.3e}"
    none = {k[9:] for k in d if k.startswith("gradnone:")}
    gscale = max(float(d[k]) for k in d if k.startswith("gnorm:"))
    for k, p in m.named_parameters():
        if k in none:
            assert p.grad is None, k
            continue
        smp, nrm = grad_sample(p.grad.detach().float().cpu().numpy())
        ref_s, ref_n = d["gsample:" + k], float(d["gnorm:" + k])
        assert abs(float(nrm) - ref_n) <= gtol * max(ref_n, 1e-3 * gscale), f"|grad {k}| {float(nrm):.4e} vs {ref_n:.4e}"
        assert max_abs(smp, ref_s) <= gtol * max(float(np.abs(ref_s).max()), 1e-3 * gscale / max(1.0, np.sqrt(p.numel()))), \
            f"grad sample {k}"


# ---- op sweep against float64 torch, on the kernels' own route ----
def _ref64(x, gw, gb, w1s, w2s, route, dy, residual=None):
    """float64 routed top-1 MLP and its gradients (dx, dW1_e, dW2_e), every token through expert route[t]"""
    x = x.detach().double().reshape(-1, x.shape[-1]).requires_grad_(True)
    w1 = [w.detach().double().requires_grad_(True) for w in w1s]
    w2 = [w.detach().double().requires_grad_(True) for w in w2s]
    r = route.long()
    y = torch.zeros_like(x)
    for e in range(len(w1)):
        sel = (r == e).nonzero().squeeze(1)
        y = y.index_add(0, sel, F.linear(F.gelu(F.linear(x[sel], w1[e]), approximate="tanh"), w2[e]))
    if residual is not None:
        y = y + residual.detach().double().reshape(y.shape)
    y.backward(dy.detach().double().reshape(y.shape))
    return y.detach(), x.grad, [w.grad for w in w1], [w.grad for w in w2]


def _case(M, D, F_, E, skew, seed, dtype=torch.float32, wdtype=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    wdtype = wdtype or dtype
    x = torch.randn(M, D, device="cuda", generator=g).to(dtype)
    gw = (torch.randn(E, D, device="cuda", generator=g) / D ** 0.5).to(wdtype)
    gb = (0.1 * torch.randn(E, device="cuda", generator=g)).to(wdtype)
    if skew:                                    # every token to expert E - 1
        gb = gb + torch.arange(E, device="cuda", dtype=wdtype) * 1e3
    w1s = [(torch.randn(F_, D, device="cuda", generator=g) / D ** 0.5).to(wdtype).requires_grad_(True) for _ in range(E)]
    w2s = [(torch.randn(D, F_, device="cuda", generator=g) / F_ ** 0.5).to(wdtype).requires_grad_(True) for _ in range(E)]
    dy = torch.randn(M, D, device="cuda", generator=g)
    res = torch.randn(M, D, device="cuda", generator=g)
    return x, gw, gb, w1s, w2s, dy, res


def _sweep_check(M, D, F_, E, skew, mode, with_res, seed=0):
    from mop_amd import _lib, ops
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    x, gw, gb, w1s, w2s, dy, res = _case(M, D, F_, E, skew, seed, dtype=dt)
    x.requires_grad_(True)
    odt = torch.bfloat16 if mode in ("bf16", "autocast") else torch.float32
    r = res.to(odt).requires_grad_(True) if with_res else None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "autocast"):
        y = ops.moe_mlp(x, gw, gb, w1s, w2s, residual=r)
    assert y.dtype == odt
    y.backward(dy.to(odt))
    assert ops.LAST_PATH["moe_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["moe_bwd"] == _lib.PATH_FUSED
    route = ops.moe_route(x, gw, gb)
    if skew:
        assert bool((route == E - 1).all())
    rdt = torch.float32 if mode == "fp32" else torch.bfloat16             # the operands the kernels see, rounded as they do
    q = lambda t: t.detach().to(rdt)
    y64, dx64, dw1, dw2 = _ref64(q(x), gw, gb, [q(w) for w in w1s], [q(w) for w in w2s], route, dy.to(odt),
                                 None if r is None else r.detach())
    tol = 2e-5 if mode == "fp32" else 2e-2
    yv = y.detach().double().reshape(y64.shape)
    assert float((yv - y64).abs().max()) <= tol * max(1.0, float(y64.abs().max())), f"y {float((yv - y64).abs().max()):.3e}"
    got = {"dx": x.grad.double().reshape(dx64.shape)}
    ref = {"dx": dx64}
    for e in range(E):
        got[f"w1.{e}"], ref[f"w1.{e}"] = w1s[e].grad.double(), dw1[e]
        got[f"w2.{e}"], ref[f"w2.{e}"] = w2s[e].grad.double(), dw2[e]
    check_grads({k: v.cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in ref.items()},
                1e-4 if mode == "fp32" else 3e-2)
    if with_res:
        assert torch.equal(r.grad, dy.to(odt))
    used = set(route.tolist())
    for e in set(range(E)) - used:
        assert not bool(w1s[e].grad.any()) and not bool(w2s[e].grad.any())


SWEEP = [
    # M at the 64 / 128-row tile edges, D, F, E, skewed route, arithmetic, residual
    (1, 72, 288, 4, False, "fp32", False),
    (63, 8, 32, 2, False, "fp32", True),
    (64, 72, 288, 4, True, "fp32", False),
    (65, 384, 1536, 4, False, "fp32", True),
    (127, 72, 288, 8, False, "fp32", False),
    (128, 8, 64, 64, False, "fp32", True),
    (129, 384, 1536, 2, True, "fp32", False),
    (3001, 72, 288, 8, False, "fp32", True),
    (1, 8, 32, 2, False, "bf16", False),
    (63, 72, 288, 4, True, "bf16", True),
    (64, 384, 1536, 4, False, "bf16", False),
    (65, 8, 32, 8, False, "bf16", True),
    (127, 72, 288, 64, False, "bf16", False),
    (129, 384, 1536, 4, False, "bf16", True),
    (4099, 384, 1536, 4, True, "bf16", False),
    (3001, 72, 288, 8, False, "bf16", True),
    (1, 72, 288, 2, False, "autocast", True),
    (128, 384, 1536, 4, False, "autocast", False),
    (2049, 72, 288, 64, False, "autocast", True),
    (257, 8, 32, 4, True, "autocast", False),
]


@pytest.mark.parametrize("M,D,F_,E,skew,mode,with_res", SWEEP)
def test_moe_op_sweep_vs_float64(M, D, F_, E, skew, mode, with_res):
    _sweep_check(M, D, F_, E, skew, mode, with_res)


@pytest.mark.parametrize("what", ["d_not_multiple_of_8", "fp16", "too_many_experts"])
def test_unsupported_calls_take_the_torch_path(what):
    from mop_amd import _lib, ops
    D, F_, E, dt = 64, 256, 4, torch.float32
    if what == "d_not_multiple_of_8":
        D, F_ = 12, 48
    elif what == "fp16":
        dt = torch.float16
    else:
        E = 65
    x, gw, gb, w1s, w2s, dy, _ = _case(100, D, F_, E, False, 3, dtype=dt)
    x.requires_grad_(True)
    y = ops.moe_mlp(x, gw, gb, w1s, w2s)
    y.backward(dy.to(dt))
    assert ops.LAST_PATH["moe_fwd"] == _lib.PATH_GENERIC
    route = F.linear(x.detach(), gw, gb).argmax(-1)                      # the torch path's own route (same op, same dtype)
    y64, dx64, dw1, dw2 = _ref64(x, gw, gb, w1s, w2s, route, dy.to(dt))
    tol = 1e-2 if dt == torch.float16 else 1e-4
    assert float((y.double() - y64).abs().max()) <= tol * max(1.0, float(y64.abs().max()))
    assert rel_err(x.grad.double().cpu().numpy(), dx64.cpu().numpy()) <= (3e-2 if dt == torch.float16 else 1e-4)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_bitwise_reproducible(mode):
    from mop_amd import ops
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    outs = []
    for _ in range(2):
        x, gw, gb, w1s, w2s, dy, res = _case(3000, 384, 1536, 4, False, 7, dtype=dt)
        x.requires_grad_(True)
        y = ops.moe_mlp(x, gw, gb, w1s, w2s, residual=res.to(dt))
        y.backward(dy.to(dt))
        outs.append([y.detach(), x.grad] + [w.grad for w in w1s + w2s])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_no_host_sync():
    from mop_amd import ops
    x, gw, gb, w1s, w2s, dy, res = _case(2000, 72, 288, 4, False, 11, dtype=torch.bfloat16)
    x.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = ops.moe_mlp(x, gw, gb, w1s, w2s, residual=res.to(torch.bfloat16))
        y.backward(dy.to(torch.bfloat16))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(x.grad).all()


def test_graph_replay_reproduces_eager():
    """one single-stream torch.cuda.graph capture of MoEMLP forward + backward, in its own process (tools/graph_probe_moe.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_moe.py")], cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-400:]
