"""CPU checks of the top-1 MoE MLP line (no GPU): the reference's constructor signatures and defaults, state_dict layouts against
the `moe_*` / `moevit_*` fixtures, ViT_MoP(use_moe=True) construction, the support query and bad-argument
returns of mopk_moe_*, and the no-CPU-fallback error."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden

MOE_FIXTURES = golden_names("moe_") + golden_names("moevit_")


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _defaults(f):
    return {k: v.default for k, v in inspect.signature(f).parameters.items() if k != "self"}


def test_signatures_match_the_reference():
    """reference mop/models/components.py:84-121, :144-168, :208-252 and vit_mop.py:33-47"""
    from mop_amd.nn.components import BlockMoE, MoEMLP, ViTEncoderMoE
    from mop_amd.nn import ViT_MoP
    e = inspect.Parameter.empty
    assert _defaults(MoEMLP.__init__) == dict(dim=e, mlp_ratio=4.0, num_experts=4)
    assert _defaults(BlockMoE.__init__) == dict(dim=e, heads=e, mlp_ratio=4.0, drop=0.0, attn_drop=0.0, drop_path=0.0, num_experts=4)
    assert _defaults(ViTEncoderMoE.__init__) == dict(dim=256, depth=6, heads=4, mlp_ratio=4.0, drop=0.0, drop_path=0.1, patch=4,
                                                     num_tokens=64, num_experts=4)
    d = _defaults(ViT_MoP.__init__)
    assert d["use_moe"] is False and d["moe_experts"] == 4
    assert list(inspect.signature(MoEMLP.forward).parameters)[:2] == ["self", "x"]
    with pytest.raises(AssertionError):
        MoEMLP(16, 4.0, 1)


def test_vit_mop_use_moe_constructs():
    from mop_amd.nn import ViT_MoP
    from mop_amd.nn.components import BlockMoE, MoEMLP, ViTEncoderMoE
    m = ViT_MoP(dim=64, depth=2, heads=4, n_views=3, n_kernels=2, use_moe=True, moe_experts=3)
    assert isinstance(m.enc, ViTEncoderMoE)
    assert all(isinstance(b, BlockMoE) and isinstance(b.mlp, MoEMLP) for b in m.enc.blocks)
    assert all(b.mlp.num_experts == 3 and len(b.mlp.fc1) == 3 and len(b.mlp.fc2) == 3 for b in m.enc.blocks)
    sd = m.state_dict()
    assert sd["enc.blocks.1.mlp.fc1.2.weight"].shape == (256, 64) and sd["enc.blocks.1.mlp.fc2.0.weight"].shape == (64, 256)
    assert sd["enc.blocks.0.mlp.gate.weight"].shape == (3, 64) and sd["enc.blocks.0.mlp.gate.bias"].shape == (3,)
    assert m.enc.blocks[0].mlp.fc1[0].bias is None and m.enc.blocks[0].mlp.fc2[0].bias is None


def _module_for(meta):
    from mop_amd.nn import ViT_MoP
    from mop_amd.nn.components import BlockMoE, MoEMLP
    kind = str(meta["kind"])
    if kind == "moe_mlp":
        return MoEMLP(int(meta["dim"]), float(meta["mlp_ratio"]), int(meta["num_experts"]))
    if kind == "block_moe":
        return BlockMoE(int(meta["dim"]), int(meta["heads"]), float(meta["mlp_ratio"]), num_experts=int(meta["num_experts"]))
    return ViT_MoP(dim=int(meta["dim"]), depth=int(meta["depth"]), heads=int(meta["heads"]), n_classes=int(meta["n_classes"]),
                   n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]), drop_path=0.0, use_moe=True,
                   moe_experts=int(meta["moe_experts"]))


def test_fixtures_present():
    assert {"moe_d64_e4", "moe_d72_e3", "moe_skew_d64_e4", "moe_block_d64_e4", "moevit_tiny_e3", "moevit_cfg0_e4"} <= set(MOE_FIXTURES)


@pytest.mark.parametrize("name", MOE_FIXTURES)
def test_state_dict_layout_matches_the_fixture(name):
    """keys, shapes and order of the reference's state_dict (shape: entries are written in state_dict order, param: entries of the
    stored gate tensors interleaved) and the parameter count"""
    d, params, _, meta = load_golden(name)
    m = _module_for(meta)
    sd = m.state_dict()
    ref = {}
    for k in d:                                  # npz keeps insertion order
        if k.startswith("shape:"):
            ref[k[6:]] = tuple(int(s) for s in d[k])
        elif k.startswith("param:"):
            ref[k[6:]] = tuple(d[k].shape)
    assert set(ref) == set(sd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    if "moevit" in name:                         # vit fixtures write every shape: in state_dict order
        assert [k[6:] for k in d if k.startswith("shape:")] == list(sd)
    assert sum(p.numel() for p in m.parameters()) == int(meta["n_params"])
    routes = [k for k in d if k.startswith("route:")]
    assert routes and all(k[6:] == "" or k[6:].endswith("mlp") for k in routes)
    gnone = sorted(k[9:] for k in d if k.startswith("gradnone:"))
    assert gnone and all(".gate." in "." + k for k in gnone)
    assert float(meta["min_margin"]) >= (0.03 if "bf16err:dx" in d else 1e-3)


def test_cpu_tensor_raises_no_cpu_fallback():
    from mop_amd.nn.components import MoEMLP
    m = MoEMLP(16, 2.0, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(1, 4, 16))
    from mop_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moe_route(torch.randn(4, 16), m.gate.weight, m.gate.bias)


def _args(M=64, D=64, F=256, E=4, prec=1):
    from mop_amd import _lib
    a = _lib.MoeArgs()
    a.M, a.D, a.F, a.E, a.precision = M, D, F, E, prec
    a.x_dtype = a.w_dtype = a.gate_dtype = a.o_dtype = _lib.MOPK_F32
    return a


def test_support_query_needs_no_gpu(lib):
    from mop_amd import _lib
    ok = lambda a: lib.mopk_moe_supported(C.byref(a))
    assert ok(_args()) == 1 and ok(_args(prec=0)) == 1 and ok(_args(M=1, D=8, F=8, E=2)) == 1
    assert ok(_args(E=_lib.MOE_MAX_EXPERTS)) == 1
    assert ok(_args(E=_lib.MOE_MAX_EXPERTS + 1)) == 0
    assert ok(_args(D=68)) == 0 and ok(_args(F=260)) == 0
    a = _args(prec=0)
    a.x_dtype = _lib.MOPK_BF16                   # exact fp32 arithmetic takes fp32 tensors only
    assert ok(a) == 0
    a.precision = 1
    assert ok(a) == 1
    a.o_dtype = 2                                # not a MopkDtype (fp16 has none)
    assert ok(a) == 0
    assert lib.mopk_moe_workspace_bytes(C.byref(_args()), 0) == 0
    assert lib.mopk_moe_workspace_bytes(C.byref(_args()), 1) > 64 * 256 * 2
    assert lib.mopk_moe_workspace_bytes(C.byref(_args(M=0)), 1) == 0


def test_support_query_at_the_int32_element_bound(lib):
    """M F and M D stay below 2^31 (the kernels index rows with int64 but the scan and the tile walk count in int32): the largest
    accepted products with D, F multiples of 8 and the first refused ones"""
    ok = lambda a: lib.mopk_moe_supported(C.byref(a))
    assert (2 ** 20 - 1) * 2048 == 2 ** 31 - 2048
    assert ok(_args(M=2 ** 20 - 1, D=8, F=2048, E=2)) == 1
    assert ok(_args(M=2 ** 20, D=8, F=2048, E=2)) == 0
    assert ok(_args(M=2 ** 20 - 1, D=2048, F=8, E=2)) == 1
    assert ok(_args(M=2 ** 20, D=2048, F=8, E=2)) == 0
    assert ok(_args(M=2 ** 20 - 1, D=2048, F=2048, E=2, prec=0)) == 1
    assert ok(_args(M=2 ** 20, D=8, F=8, E=2)) == 1


def test_bad_arguments_return_before_any_launch(lib):
    from mop_amd import _lib
    for fn in (lib.mopk_moe_route, lib.mopk_moe_fwd, lib.mopk_moe_bwd):
        assert fn(None, None) == -2
        for kw in (dict(M=0), dict(D=0), dict(F=-8), dict(E=1)):
            assert fn(C.byref(_args(**kw)), None) == -1, (fn, kw)
        assert fn(C.byref(_args(prec=7)), None) == -2
        assert fn(C.byref(_args(E=65)), None) == -3
        assert fn(C.byref(_args()), None) == -2          # valid shape, null tensors


def test_module_default_init_matches_the_reference_order():
    """same construction order as the reference (fc1 list, fc2 list, gate): one seed gives the reference's initial values; here
    checked as nn.Linear draws in that order"""
    from mop_amd.nn.components import MoEMLP
    torch.manual_seed(5)
    m = MoEMLP(16, 2.0, 3)
    torch.manual_seed(5)
    ref = [torch.nn.Linear(16, 32, bias=False) for _ in range(3)] + [torch.nn.Linear(32, 16, bias=False) for _ in range(3)]
    gate = torch.nn.Linear(16, 3, bias=True)
    got = [l.weight for l in m.fc1] + [l.weight for l in m.fc2]
    assert all(torch.equal(a, b.weight) for a, b in zip(got, ref))
    assert torch.equal(m.gate.weight, gate.weight) and torch.equal(m.gate.bias, gate.bias)
    assert list(m.state_dict()) == [f"fc1.{e}.weight" for e in range(3)] + [f"fc2.{e}.weight" for e in range(3)] + \
        ["gate.weight", "gate.bias"]
