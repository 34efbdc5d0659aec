"""GPT line, host side (no GPU): constructor signatures, state_dict layouts of the reference's fixtures, the reference's own
tests/test_gpt_mop.py tests 1-2, and the fold of the 1-D MoP token gate into three taps (float64, values and gradients)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_names, load_golden


def _sig(f):
    return [(k, p.default) for k, p in inspect.signature(f).parameters.items() if k != "self"]


def test_constructor_signatures_are_the_reference_ones():
    from mop_amd.nn import gpt_mop as G
    from mop_amd.nn import quartet_attn_patch as Q
    E = inspect.Parameter.empty
    assert _sig(G.ViewsLinear1D.__init__) == [("dim", E), ("n_views", 5)]
    assert _sig(G.Kernels1D.__init__) == [("in_ch", E), ("n_kernels", 3), ("kernel_size", 3)]
    assert _sig(G.FuseExcInh1D.__init__) == [("in_ch", E)]
    assert _sig(G.MoPBlock.__init__) == [("config", E), ("n_views", 5), ("n_kernels", 3)]
    assert _sig(G.GPT_MoP.__init__) == [("vocab_size", E), ("config", E), ("n_views", 5), ("n_kernels", 3)]
    assert _sig(G.create_gpt_mop) == [("vocab_size", E), ("config", E), ("n_views", 5), ("n_kernels", 3)]
    assert _sig(G.create_gpt_baseline) == [("vocab_size", E), ("config", E)]
    assert _sig(G.create_gpt_quartet) == [("vocab_size", E), ("config", E)]
    assert _sig(Q.MLP.__init__) == [("config", E)] and _sig(Q.Block.__init__) == [("config", E)]
    assert _sig(Q.TinyTransformerLM.__init__) == [("vocab_size", E), ("config", E)]
    for cls in (G.GPT_MoP, Q.TinyTransformerLM):
        assert _sig(cls.forward) == [("idx", E), ("attention_mask", None), ("targets", None)]


def test_exports_keep_the_vit_mlp_and_block():
    import mop_amd.nn as nn_
    from mop_amd.nn import components, quartet_attn_patch
    assert nn_.MLP is components.MLP and nn_.Block is components.Block
    assert quartet_attn_patch.Block is not components.Block
    for n in ("GPT_MoP", "MoPBlock", "ViewsLinear1D", "Kernels1D", "FuseExcInh1D", "create_gpt_mop", "create_gpt_baseline",
              "create_gpt_quartet"):
        assert hasattr(nn_, n), n


def _lm_from_meta(meta):
    from mop_amd.nn import GPT_MoP
    from mop_amd.nn.quartet_attn_patch import TinyTransformerLM, TransformerConfig
    cfg = TransformerConfig(n_layer=int(meta["n_layer"]), n_head=int(meta["heads"]), n_embd=int(meta["dim"]),
                            block_size=int(meta["block_size"]), dropout=0.0, bias=bool(meta["bias"]),
                            use_abs_pos_emb=bool(meta["use_abs_pos_emb"]), use_quartet=meta["model"] != "baseline")
    if meta["model"] == "mop":
        return GPT_MoP(int(meta["vocab"]), cfg, n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]))
    return TinyTransformerLM(int(meta["vocab"]), cfg)


def _block_from_meta(meta):
    from mop_amd.nn import MoPBlock
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    cfg = TransformerConfig(n_head=int(meta["heads"]), n_embd=int(meta["dim"]), block_size=int(meta["block_size"]), dropout=0.0,
                            bias=bool(meta["bias"]))
    return MoPBlock(cfg, n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]))


@pytest.mark.parametrize("name", golden_names("gpt_"))
def test_fixture_state_dict_loads_strict(name):
    d, params, gref, meta = load_golden(name)
    m = _lm_from_meta(meta) if meta["kind"] == "gpt_lm" else _block_from_meta(meta)
    sd = m.state_dict()
    assert set(sd) == set(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert set(gref) == {k for k, _ in m.named_parameters()}
    if meta["kind"] == "gpt_lm":
        assert sum(p.numel() for p in m.parameters()) == int(meta["n_params"])
        assert m.lm_head.weight is m.wte.weight                    # tied, as in the reference
        assert "lm_head.weight" in sd and "wte.weight" in sd
        assert (m.wpe is None) == (not bool(meta["use_abs_pos_emb"]))


def test_reference_individual_models():
    """reference tests/test_gpt_mop.py::test_individual_models"""
    from mop_amd.nn import create_gpt_baseline, create_gpt_mop, create_gpt_quartet
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    config = TransformerConfig(n_layer=2, n_head=2, n_embd=64, block_size=32, dropout=0.1, bias=False)
    baseline = create_gpt_baseline(200, config)
    quartet = create_gpt_quartet(200, config)
    mop = create_gpt_mop(200, config, n_views=2, n_kernels=1)
    for m in (baseline, quartet, mop):
        assert sum(p.numel() for p in m.parameters() if p.requires_grad) > 0
    assert baseline.config.use_quartet is False and quartet.config.use_quartet is True
    assert baseline.blocks[0].attn.mixture is None and quartet.blocks[0].attn.mixture is not None
    assert tuple(mop.blocks[1].fuse.conv.weight.shape) == (2, 3, 1) and tuple(mop.blocks[1].kernels.conv.weight.shape) == (1, 2, 3)


def test_factories_copy_only_the_reference_fields():
    """the reference's create_gpt_baseline / _quartet copy six fields; use_abs_pos_emb and the Quartet extras take defaults"""
    from mop_amd.nn import create_gpt_quartet
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    cfg = TransformerConfig(n_layer=1, n_head=2, n_embd=32, block_size=8, use_abs_pos_emb=False, quartet_gate_init=1.0)
    m = create_gpt_quartet(50, cfg)
    assert m.wpe is not None and float(m.blocks[0].attn.mixture.detach()) == -5.0


def test_reference_forward_pass_on_cpu_takes_the_library_route():
    """reference tests/test_gpt_mop.py::test_forward_pass: on CPU tensors the attention core, like every other module here, refuses
    (no CPU fallback); tests/test_gpu_gpt.py runs the same three models on the GPU and checks the logits' shape."""
    from mop_amd.nn import create_gpt_baseline, create_gpt_mop, create_gpt_quartet
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    config = TransformerConfig(n_layer=2, n_head=2, n_embd=64, block_size=32, dropout=0.1, bias=False)
    x = torch.randint(0, 100, (2, 16))
    y = torch.randint(0, 100, (2, 16))
    for make in (create_gpt_baseline, create_gpt_quartet, lambda v, c: create_gpt_mop(v, c, n_views=2, n_kernels=1)):
        m = make(100, config).eval()
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x, targets=y)


def _unfolded(r, Wv, Wk, Wf, alpha):
    """the reference's gate composition (gpt_mop.py:109-123) written with functional ops"""
    V = F.linear(r, Wv).transpose(1, 2)
    K = F.conv1d(V, Wk, padding=1)
    g = F.conv1d(torch.cat([V, K], dim=1), Wf)
    gate = 1 + alpha[0] * g[:, :1] - alpha[1] * g[:, 1:]
    return r * gate.transpose(1, 2)


@pytest.mark.parametrize("V,K,B,T,D", [(5, 3, 2, 7, 16), (2, 1, 3, 1, 8), (4, 6, 1, 2, 12), (3, 2, 2, 33, 24)])
def test_fold_equals_the_unfolded_gate_float64(V, K, B, T, D):
    from mop_amd import ops
    g = torch.Generator().manual_seed(V * 100 + T)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)
    Wv, Wk, Wf, alpha, x, a = mk(V, D), mk(K, V, 3), mk(2, V + K, 1), mk(2), mk(B, T, D), mk(B, T, D)
    w = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    ref = _unfolded(x + a, Wv, Wk, Wf, alpha)
    gr = torch.autograd.grad((ref * w).sum(), (x, a, Wv, Wk, Wf, alpha))
    u = ops.token_gate_taps(Wv.double(), Wk, Wf, alpha).double()
    out = ops.token_gate_1d_torch(x, a, u)
    go = torch.autograd.grad((out * w).sum(), (x, a, Wv, Wk, Wf, alpha))
    assert torch.allclose(out, ref, rtol=1e-10, atol=1e-10)
    for name, p, q in zip(("x", "a", "Wv", "Wk", "Wf", "alpha"), go, gr):
        assert torch.allclose(p, q, rtol=1e-9, atol=1e-9), name


def test_fold_as_the_kernels_state_it():
    """gate_t = 1 + u0.r_{t-1} + u1.r_t + u2.r_{t+1} and its adjoint dr, du (the formulas of mop_amd/csrc/token_gate.hip), written
    out token by token in float64, against autograd of the folded torch form"""
    from mop_amd import ops
    g = torch.Generator().manual_seed(7)
    B, T, D = 2, 5, 8
    r = torch.randn(B, T, D, generator=g, dtype=torch.float64).requires_grad_(True)
    u = torch.randn(3, D, generator=g, dtype=torch.float64).requires_grad_(True)
    dout = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    out = ops.token_gate_1d_torch(r, None, u)
    dr_ref, du_ref = torch.autograd.grad((out * dout).sum(), (r, u))
    rr, uu = r.detach(), u.detach()
    at = lambda b, t: rr[b, t] if 0 <= t < T else torch.zeros(D, dtype=torch.float64)
    gate = torch.tensor([[1 + uu[0] @ at(b, t - 1) + uu[1] @ at(b, t) + uu[2] @ at(b, t + 1) for t in range(T)] for b in range(B)])
    assert torch.allclose(out.detach(), rr * gate[..., None])
    delta = (dout * rr).sum(-1)
    dl = lambda b, t: delta[b, t] if 0 <= t < T else 0.0
    dr = torch.stack([torch.stack([dout[b, t] * gate[b, t] + uu[0] * dl(b, t + 1) + uu[1] * dl(b, t) + uu[2] * dl(b, t - 1)
                                   for t in range(T)]) for b in range(B)])
    du = torch.stack([sum(dl(b, t + 1 - s) * rr[b, t] for b in range(B) for t in range(T)) for s in range(3)])
    assert torch.allclose(dr, dr_ref) and torch.allclose(du, du_ref)


def test_token_gate_on_cpu_takes_the_torch_route():
    from mop_amd import _lib, ops
    from mop_amd.nn import MoPBlock
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    torch.manual_seed(0)
    blk = MoPBlock(TransformerConfig(n_head=2, n_embd=16, block_size=8), n_views=3, n_kernels=2).double()
    with torch.no_grad():
        blk.fuse.alpha.copy_(torch.tensor([0.6, 1.4]))
    x = torch.randn(2, 6, 16, dtype=torch.float64)
    a = torch.randn(2, 6, 16, dtype=torch.float64)
    ref = _unfolded(x + a, blk.views.proj.weight, blk.kernels.conv.weight, blk.fuse.conv.weight, blk.fuse.alpha)
    assert torch.allclose(blk._gated_residual(x, a), ref)
    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_GENERIC
    assert torch.allclose(blk.apply_mop(x + a), ref)
    assert torch.allclose(ops.token_gate_1d(x, a, blk.taps().double()), ref)
    assert not ops.token_gate_supported(x.float(), a.float())
    gate, Vm, Km = blk.get_gate_maps(x)
    assert gate.shape == (2, 1, 6) and Vm.shape == (2, 3, 6) and Km.shape == (2, 2, 6)


def test_token_gate_support_query_needs_no_gpu():
    from mop_amd import _lib
    lib = _lib.lib()
    a = _lib.TokenGateArgs()
    a.B, a.T, a.D = 8, 1024, 768
    a.x_dtype = a.o_dtype = _lib.MOPK_BF16
    a.x_sb, a.x_st = 1024 * 768, 768
    assert lib.mopk_token_gate_supported(C.byref(a)) == 1
    assert lib.mopk_token_gate_workspace_bytes(C.byref(a)) == 512 * 3 * 768 * 4
    a.a, a.a_dtype, a.a_sb, a.a_st = 256, _lib.MOPK_F32, 1024 * 768, 768   # a fp32 branch: the output must be fp32
    assert lib.mopk_token_gate_supported(C.byref(a)) == 0
    a.o_dtype = _lib.MOPK_F32
    assert lib.mopk_token_gate_supported(C.byref(a)) == 1
    a.a = 264                                                                # not 16-byte aligned
    assert lib.mopk_token_gate_supported(C.byref(a)) == 0
    a.a = 256
    for D, ok in ((100, 0), (1024, 1), (1032, 0), (8, 1)):
        a.D, a.x_st, a.a_st = D, max(D, 8), max(D, 8)
        assert lib.mopk_token_gate_supported(C.byref(a)) == ok, D
    a.D, a.x_st = 64, 68                                                     # row stride not a multiple of 8
    assert lib.mopk_token_gate_supported(C.byref(a)) == 0
    a.T = 0
    assert lib.mopk_token_gate_supported(C.byref(a)) == 0 and lib.mopk_token_gate_workspace_bytes(C.byref(a)) == 0
    assert lib.mopk_token_gate_fwd(None, None) < 0 and lib.mopk_token_gate_bwd(None, None) < 0
    b = _lib.TokenGateArgs()
    b.B, b.T, b.D, b.x_st = 1, 4, 64, 64
    assert lib.mopk_token_gate_fwd(C.byref(b), None) == -2                  # null pointers are refused before any launch


def test_mop_block_fixture_on_cpu_float64_through_the_torch_gate():
    """the gate of every MoPBlock fixture: the block's torch gate on the fixture's parameters reproduces the reference composition"""
    from mop_amd import ops
    for name in golden_names("gpt_blk_"):
        d, params, gref, meta = load_golden(name)
        blk = _block_from_meta(meta)
        blk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        blk = blk.double()
        r = torch.from_numpy(d["x"]).double()
        ref = _unfolded(r, blk.views.proj.weight, blk.kernels.conv.weight, blk.fuse.conv.weight, blk.fuse.alpha)
        assert torch.allclose(ops.token_gate_1d_torch(r, None, blk.taps().double()), ref, rtol=1e-10, atol=1e-10), name
