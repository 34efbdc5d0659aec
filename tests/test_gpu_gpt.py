"""-m gpu: the GPT line on the MI355X.  MoPBlock / GPT_MoP / Quartet TinyTransformerLM parity with the reference's fixtures
(fp32 arithmetic <= 1e-3, bf16 MFMA <= 1e-2), the fused token gate (mopk_token_gate_*) against a float64 statement of the
unfolded gate over batch, tile-boundary sequence lengths, widths, dtypes and strides, its bitwise reproducibility, and a
HIP-graph capture of a 2-block GPT_MoP."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
from gpu_util import check_grads, max_abs, module_from_golden, rel_err, run_fwd_bwd

pytestmark = pytest.mark.gpu
TOL = {"fp32": (1e-3, 1e-3), "bf16": (1e-2, 3e-2)}
TILE = 16          # tokens per workgroup tile of mop_amd/csrc/token_gate.hip (TG_TILE)


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    yield
    mop_amd.set_precision("auto")


def _cfg(meta, **kw):
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    return TransformerConfig(n_head=int(meta["heads"]), n_embd=int(meta["dim"]), block_size=int(meta["block_size"]), dropout=0.0,
                             bias=bool(meta["bias"]), **kw)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", golden_names("gpt_blk_"))
def test_mop_block_matches_the_reference(name, prec):
    import mop_amd
    from mop_amd import _lib, ops
    from mop_amd.nn import MoPBlock
    d, params, gref, meta = load_golden(name)
    mop_amd.set_precision(prec)
    m = module_from_golden(MoPBlock, params, config=_cfg(meta), n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]))
    fk = {}
    if "attention_mask" in d:
        fk["attention_mask"] = torch.from_numpy(d["attention_mask"]).cuda()
    ops.LAST_PATH.pop("token_gate_fwd", None)
    y, dx, grads = run_fwd_bwd(m, d["x"], d["w"], **fk)
    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["token_gate_bwd"] == _lib.PATH_FUSED
    tol, gtol = TOL[prec]
    assert max_abs(y, d["y"]) <= tol, f"y {max_abs(y, d['y']):.3e}"
    assert rel_err(dx, d["dx"]) <= gtol, f"dx {rel_err(dx, d['dx']):.3e}"
    check_grads(grads, gref, gtol, scalar_tol=5e-2 if prec == "bf16" else None, floor=1e-2 if prec == "bf16" else 1e-3,
                d=d if prec == "bf16" else None)


def _lm(meta):
    from mop_amd.nn import GPT_MoP
    from mop_amd.nn.quartet_attn_patch import TinyTransformerLM
    cfg = _cfg(meta, n_layer=int(meta["n_layer"]), use_abs_pos_emb=bool(meta["use_abs_pos_emb"]),
               use_quartet=meta["model"] != "baseline")
    if meta["model"] == "mop":
        return GPT_MoP(int(meta["vocab"]), cfg, n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]))
    return TinyTransformerLM(int(meta["vocab"]), cfg)


def _lm_from_golden(name):
    d, params, gref, meta = load_golden(name)
    m = _lm(meta)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    return d, gref, meta, m.cuda().eval()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", golden_names("gpt_lm_"))
def test_language_model_matches_the_reference(name, prec):
    import mop_amd
    from mop_amd import _lib, ops
    d, gref, meta, m = _lm_from_golden(name)
    mop_amd.set_precision(prec)
    idx, tgt = torch.from_numpy(d["idx"]).cuda(), torch.from_numpy(d["targets"]).cuda()
    ops.LAST_PATH.pop("token_gate_fwd", None)
    logits, loss = m(idx, targets=tgt)
    loss.backward()
    torch.cuda.synchronize()
    if meta["model"] == "mop":
        assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_FUSED
    else:
        assert "token_gate_fwd" not in ops.LAST_PATH
    tol, gtol = TOL[prec]
    assert max_abs(logits.detach().cpu().numpy(), d["logits"]) <= tol
    assert abs(float(loss.detach()) - float(d["loss"])) <= tol
    grads = {k: p.grad.float().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    check_grads(grads, gref, gtol, scalar_tol=5e-2 if prec == "bf16" else None, floor=1e-2 if prec == "bf16" else 1e-3,
                d=d if prec == "bf16" else None)


def test_gate_maps_match_the_reference():
    for name in golden_names("gpt_lm_mop"):
        d, gref, meta, m = _lm_from_golden(name)
        with torch.no_grad():
            g, V, K = m.get_gate_maps(torch.from_numpy(d["idx"]).cuda())
        assert g.shape == d["gate_maps"].shape and V.shape == d["view_maps"].shape and K.shape == d["kernel_maps"].shape
        for ours, ref in ((g, d["gate_maps"]), (V, d["view_maps"]), (K, d["kernel_maps"])):
            assert max_abs(ours.cpu().numpy(), ref) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


def test_reference_forward_pass_shapes():
    """reference tests/test_gpt_mop.py::test_forward_pass on the GPU"""
    from mop_amd.nn import create_gpt_baseline, create_gpt_mop, create_gpt_quartet
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    config = TransformerConfig(n_layer=2, n_head=2, n_embd=64, block_size=32, dropout=0.1, bias=False)
    x = torch.randint(0, 100, (2, 16), device="cuda")
    y = torch.randint(0, 100, (2, 16), device="cuda")
    for make in (create_gpt_baseline, create_gpt_quartet, lambda v, c: create_gpt_mop(v, c, n_views=2, n_kernels=1)):
        m = make(100, config).cuda().eval()
        with torch.no_grad():
            logits, loss = m(x, targets=y)
        assert logits.shape[:2] == (2, 16) and torch.isfinite(loss)


# ---- the op against float64 -------------------------------------------------------------------------------------------------
def _inputs(B, T, D, xdt, adt, strided, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:       # x: every other 2D-wide row's first half; a: a (T,B,D) buffer seen as (B,T,D)
        x = torch.randn(B, T, 2 * D, device="cuda", generator=g).to(xdt)[..., :D]
        a = None if adt is None else torch.randn(T, B, D, device="cuda", generator=g).to(adt).transpose(0, 1)
    else:
        x = torch.randn(B, T, D, device="cuda", generator=g).to(xdt)
        a = None if adt is None else torch.randn(B, T, D, device="cuda", generator=g).to(adt)
    u = 0.05 * torch.randn(3, D, device="cuda", generator=g)
    dout = torch.randn(B, T, D, device="cuda", generator=g)
    return x, a, u, dout


def _ref64(x, a, u, dout):
    """the reference's unfolded composition (views -> conv1d -> cat -> conv1d -> alpha) with the taps as its only parameters:
    views = u (3 views), a conv1d whose kernel picks view j at offset j - 1, fuse = sum of the three kernel channels"""
    import torch.nn.functional as F
    x64 = x.detach().double().requires_grad_(True)
    a64 = None if a is None else a.detach().double().requires_grad_(True)
    u64 = u.detach().double().requires_grad_(True)
    r = x64 if a64 is None else x64 + a64
    V = F.linear(r, u64).transpose(1, 2)                                  # (B,3,T)
    Wk = torch.zeros(3, 3, 3, dtype=torch.float64, device=x.device)
    for j in range(3):
        Wk[j, j, j] = 1.0
    K = F.conv1d(V, Wk, padding=1)
    gate = 1 + F.conv1d(torch.cat([V, K], 1), torch.tensor([[[0.0]] * 3 + [[1.0]] * 3], dtype=torch.float64, device=x.device))
    out = r * gate.transpose(1, 2)
    ins = [x64] + ([a64] if a64 is not None else []) + [u64]
    grads = torch.autograd.grad((out * dout.double()).sum(), ins)
    return out.detach(), grads[0], grads[-1]


def _nerr(a, b):
    return float((a.detach().double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


_DT = {"fp32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "mixed": (torch.float32, torch.bfloat16)}
_TS = sorted({1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 1023, 1024, 1025})


@pytest.mark.parametrize("D", [64, 96, 640, 768, 1024])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "mixed"])
def test_token_gate_op_against_float64(dt, D):
    from mop_amd import _lib, ops
    xdt, adt = _DT[dt]
    tol = 1e-2 if dt == "bf16" else 1e-4
    n = 0
    for B in (1, 3):
        for T in _TS:
            for with_a in (True, False):
                for strided in ((False, True) if T in (1, TILE + 1, 1025) else (False,)):
                    x, a, u, dout = _inputs(B, T, D, xdt, adt if with_a else None, strided, seed=B * 10007 + T * 31 + D)
                    xr = x.detach().requires_grad_(True)
                    ar = None if a is None else a.detach().requires_grad_(True)
                    ur = u.clone().requires_grad_(True)
                    out = ops.token_gate_1d(xr, ar, ur)
                    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_FUSED
                    odt = torch.bfloat16 if (xdt == torch.bfloat16 and (a is None or adt == torch.bfloat16)) else torch.float32
                    assert out.dtype == odt
                    out.backward(dout.to(odt))
                    ro, rdx, rdu = _ref64(x, a, u, dout.to(odt))
                    what = f"B={B} T={T} D={D} {dt} a={with_a} strided={strided}"
                    assert _nerr(out, ro) <= tol, what + f" out {_nerr(out, ro):.2e}"
                    assert _nerr(xr.grad, rdx) <= tol, what + f" dx {_nerr(xr.grad, rdx):.2e}"
                    if ar is not None:
                        tol_a = 1e-2 if adt == torch.bfloat16 else 1e-4           # da: dr rounded to a's dtype
                        assert ar.grad.dtype == adt and _nerr(ar.grad, rdx) <= tol_a, what + f" da {_nerr(ar.grad, rdx):.2e}"
                    assert _nerr(ur.grad, rdu) <= (1e-2 if dt == "bf16" else 1e-4), what + f" du {_nerr(ur.grad, rdu):.2e}"
                    n += 1
    assert n > 40


def test_unsupported_width_takes_the_torch_route():
    from mop_amd import _lib, ops
    x, a, u, dout = _inputs(2, 37, 100, torch.float32, torch.float32, False, seed=5)
    assert not ops.token_gate_supported(x, a)
    xr, ar, ur = x.requires_grad_(True), a.requires_grad_(True), u.requires_grad_(True)
    out = ops.token_gate_1d(xr, ar, ur)
    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_GENERIC
    out.backward(dout)
    ro, rdx, rdu = _ref64(x, a, u, dout)
    assert _nerr(out, ro) <= 1e-5 and _nerr(xr.grad, rdx) <= 1e-5 and _nerr(ur.grad, rdu) <= 1e-5


def test_mop_block_of_unsupported_width_is_still_the_reference():
    """D = 100: the block keeps the reference's composition (views -> conv -> fuse) in torch"""
    from mop_amd import _lib, ops
    from mop_amd.nn import MoPBlock
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    torch.manual_seed(3)
    blk = MoPBlock(TransformerConfig(n_head=2, n_embd=100, block_size=32, dropout=0.0), n_views=3, n_kernels=2).cuda()
    x = torch.randn(2, 20, 100, device="cuda")
    a = torch.randn(2, 20, 100, device="cuda")
    y = blk._gated_residual(x, a)
    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_GENERIC
    g, _, _ = blk.get_gate_maps(x + a)
    assert torch.allclose(y, (x + a) * g.transpose(1, 2))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_token_gate_backward_is_bitwise_reproducible(dt):
    from mop_amd import ops
    xdt, adt = _DT[dt]
    x, a, u, dout = _inputs(8, 1024, 768, xdt, adt, False, seed=11)
    res = []
    for _ in range(2):
        xr, ar, ur = x.detach().requires_grad_(True), a.detach().requires_grad_(True), u.clone().requires_grad_(True)
        ops.token_gate_1d(xr, ar, ur).backward(dout.to(xdt))
        torch.cuda.synchronize()
        res.append((xr.grad.clone(), ur.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_graphed_gpt_mop_reproduces_eager():
    """forward + backward of a 2-block GPT_MoP captured into HIP graphs and replayed, in its own process (tools/graph_probe_gpt.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_gpt.py")], cwd=root, capture_output=True,
                       text=True, timeout=300)
    if r.returncode == 0 and "CAPTURE_UNSUPPORTED" in r.stdout:
        pytest.skip("graph capture refused here: " + r.stdout[-300:])
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "FUSED_GATE True" in r.stdout, r.stdout[-500:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-500:]
