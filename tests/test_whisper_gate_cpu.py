"""WhisperMoP's mel gate, host side (no GPU): the fold of MoP2D into taps (L, k, F) against the convolutions in float64 (values and
parameter gradients), per-clip lengths, the torch routes of calls the kernels do not take, and the new exports of libmopk."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

SHAPES = [(1, 1, 1, 2, 1, 3), (2, 7, 10, 5, 3, 5), (3, 2, 3, 5, 3, 7), (2, 9, 16, 4, 2, 1), (2, 33, 80, 5, 3, 5)]   # B,T,F,V,K,k


def _params(L, V, K, k, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    return r(L, V, 1, 1), r(L, K, V, k, k) / k, r(L, 2, V + K, 1, 1), r(L, 2)


def _conv_gates(mel, Wv, Wk, Wf, alpha):
    """the reference's composition, layer by layer: conv2d -> conv2d(padding=k//2) -> cat -> conv2d -> mean -> 1 + a0 g+ - a1 g-"""
    out = []
    for wv, wk, wf, al in zip(Wv, Wk, Wf, alpha):
        views = F.conv2d(mel.unsqueeze(1), wv.unsqueeze(-1))
        maps = F.conv2d(views, wk, padding=wk.shape[-1] // 2)
        g = F.conv2d(torch.cat([views, maps], dim=1), wf).mean(dim=3)                  # (B,2,T)
        out.append(1 + al[0] * g[:, 0] - al[1] * g[:, 1])
    return torch.stack(out, dim=1)                                                     # (B,L,T)


@pytest.mark.parametrize("B,T,Fm,V,K,k", SHAPES)
def test_fold_equals_the_convolutions_in_float64(B, T, Fm, V, K, k):
    from mop_amd import ops
    torch.manual_seed(0)
    prm = _params(2, V, K, k, seed=1)
    mel = torch.randn(B, T, Fm, dtype=torch.float64)
    ref = _conv_gates(mel, *prm)
    W = ops.mel_gate_taps(*prm, Fm)
    assert W.shape == (2, k, Fm) and W.dtype == torch.float64
    got = ops.mel_gate_torch(mel, W)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_fold_is_fp32_for_fp32_parameters_and_ignores_autocast():
    from mop_amd import ops
    prm = _params(3, 5, 3, 5, seed=2, dtype=torch.float32)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        W = ops.mel_gate_taps(*prm, 80)
    assert W.dtype == torch.float32 and W.shape == (3, 5, 80)
    assert torch.equal(W, ops.mel_gate_taps(*prm, 80))
    ref = ops.mel_gate_taps(*(p.double() for p in prm), 80)
    assert float((W.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_fold_gradcheck():
    from mop_amd import ops
    prm = [p.requires_grad_() for p in _params(2, 3, 2, 3, seed=3)]
    assert torch.autograd.gradcheck(lambda *p: ops.mel_gate_taps(*p, 4), prm)


@pytest.mark.parametrize("B,T,Fm,V,K,k", SHAPES)
def test_parameter_gradients_through_the_fold_equal_the_convolutions(B, T, Fm, V, K, k):
    from mop_amd import ops
    torch.manual_seed(0)
    mel = torch.randn(B, T, Fm, dtype=torch.float64)
    dg = torch.randn(B, 2, T, dtype=torch.float64)
    grads = []
    for route in ("fold", "conv"):
        prm = [p.requires_grad_() for p in _params(2, V, K, k, seed=4)]
        g = ops.mel_gate_torch(mel, ops.mel_gate_taps(*prm, Fm)) if route == "fold" else _conv_gates(mel, *prm)
        grads.append(torch.autograd.grad(g, prm, dg))
    for name, a, b in zip(("Wv", "Wk", "Wf", "alpha"), *grads):
        assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), name


def test_module_taps_and_gate_equal_forward():
    from mop_amd.nn import MoP2D
    torch.manual_seed(0)
    m = MoP2D(5, 3, 5).double()
    with torch.no_grad():
        m.fuse.alpha.copy_(torch.tensor([0.7, 1.3]))
    mel2d = torch.randn(2, 1, 11, 16, dtype=torch.float64)
    with torch.no_grad():
        gate_t, _, _ = m(mel2d)
        got = m.gate(mel2d)
    assert m.taps(16).shape == (1, 5, 16) and m.taps(16).requires_grad
    assert got.shape == gate_t.shape == (2, 11, 1) and got.dtype == gate_t.dtype
    assert float((got - gate_t).abs().max()) <= 1e-12 * float(gate_t.abs().max())


def test_lens_columns_and_poisoned_rows():
    from mop_amd import ops
    torch.manual_seed(0)
    B, T, Fm, k = 4, 13, 6, 5
    W = ops.mel_gate_taps(*_params(3, 4, 2, k, seed=5), Fm)
    mel = torch.randn(B, T, Fm, dtype=torch.float64)
    lens = torch.tensor([13, 1, 7, 4], dtype=torch.int32)
    poisoned = mel.clone()
    for b, n in enumerate(lens.tolist()):
        poisoned[b, n:] = float("nan")
    got = ops.mel_gate(mel, W, lens)
    assert torch.equal(ops.mel_gate(poisoned, W, lens), got)           # the rows behind lens[b] change nothing
    for b, n in enumerate(lens.tolist()):
        alone = ops.mel_gate(mel[b:b + 1, :n], W)
        assert torch.equal(got[b, :, n:], torch.ones(3, T - n, dtype=torch.float64)), b
        assert float((got[b, :, :n] - alone[0]).abs().max()) <= 1e-14 * float(alone.abs().max()), b    # float64 round-off of two sums
    assert torch.isfinite(got).all()


def test_calls_the_kernels_do_not_take_run_the_torch_route():
    from mop_amd import _lib, ops
    torch.manual_seed(0)
    for dtype, k in ((torch.float32, 5), (torch.float64, 5), (torch.float32, 4)):       # CPU fp32, float64, an even k
        mel = torch.randn(2, 9, 8, dtype=dtype)
        W = torch.randn(2, k, 8, dtype=dtype)
        assert not ops.mel_gate_supported(mel, W)
        ops.LAST_PATH.pop("mel_gate_fwd", None)
        g = ops.mel_gate(mel, W)
        assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_GENERIC
        assert g.shape == (2, 2, 9) and g.dtype == dtype and torch.equal(g, ops.mel_gate_torch(mel, W))
        x, a, gate = torch.randn(2, 9, 16, dtype=dtype), torch.randn(2, 9, 16, dtype=dtype), torch.randn(2, 9, dtype=dtype)
        assert not ops.gated_residual_supported(x, a, gate)
        ops.LAST_PATH.pop("gated_residual_fwd", None)
        out = ops.gated_residual(x, a, gate)
        assert ops.LAST_PATH["gated_residual_fwd"] == _lib.PATH_GENERIC
        assert out.dtype == dtype and torch.equal(out, (x + a) * gate.unsqueeze(-1))
    # an even k in the twin: frames t - k//2 .. t - k//2 + k - 1, zeros outside
    mel, W = torch.randn(1, 5, 2, dtype=torch.float64), torch.randn(1, 2, 2, dtype=torch.float64)
    want = 1 + torch.stack([sum((mel[0, t + i - 1] * W[0, i]).sum() for i in range(2) if 0 <= t + i - 1 < 5) for t in range(5)])
    assert torch.allclose(ops.mel_gate_torch(mel, W)[0, 0], want, rtol=1e-13, atol=1e-13)


def test_twin_gradients_of_mel_and_gate():
    from mop_amd import ops
    torch.manual_seed(0)
    mel = torch.randn(2, 5, 3, dtype=torch.float64, requires_grad=True)
    W = torch.randn(2, 3, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda m, w: ops.mel_gate(m, w, torch.tensor([5, 2], dtype=torch.int32)), (mel, W))
    x, a = (torch.randn(2, 3, 8, dtype=torch.float64, requires_grad=True) for _ in range(2))
    gate = torch.randn(2, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(ops.gated_residual, (x, a, gate))


def test_the_two_functions_keep_the_autograd_contract():
    """tests/test_autograd_contract_cpu.py holds the Functions of mop_amd/ops.py to it; these two live in mop_amd/mel_gate_fn.py:
    backward marked once_differentiable, incoming gradients through _grad_in, no `.contiguous()` of their own"""
    import inspect
    from mop_amd import mel_gate_fn, ops
    assert ops._mel_gate_fn is mel_gate_fn
    for fn in (mel_gate_fn._MelGateFn, mel_gate_fn._GatedResidualFn):
        src = inspect.getsource(fn.backward)
        assert fn.backward is not torch.autograd.Function.backward and "once_differentiable" in src.split("def backward")[0], fn.__name__
        assert "_grad_in(" in src and ".contiguous()" not in src and "dout.to(" not in src and "dgates.to(" not in src, fn.__name__


def test_argument_checks_raise_value_errors():
    from mop_amd import ops
    mel, W = torch.zeros(2, 5, 8), torch.zeros(3, 5, 8)
    for bad_mel, bad_W, bad_lens in ((mel[0], W, None), (mel, W[0], None), (mel, torch.zeros(3, 5, 7), None),
                                     (mel, W, torch.zeros(2, dtype=torch.int64)), (mel, W, torch.zeros(3, dtype=torch.int32)),
                                     (mel.long(), W, None), (mel, W.to("meta"), None)):
        for f in (ops.mel_gate, ops.mel_gate_torch):
            with pytest.raises(ValueError, match="mel_gate"):
                f(bad_mel, bad_W, bad_lens)
    x, gate = torch.zeros(2, 5, 8), torch.zeros(2, 5)
    for bx, ba, bg in ((x, x[:, :4], gate), (x, x, gate.unsqueeze(-1)), (x[0], x[0], gate), (x, x, gate.long()), (x, x.to("meta"), gate)):
        for f in (ops.gated_residual, ops.gated_residual_torch):
            with pytest.raises(ValueError, match="gated_residual"):
                f(bx, ba, bg)
    prm = _params(2, 3, 2, 3, seed=6)
    with pytest.raises(ValueError, match="mel_gate_taps"):
        ops.mel_gate_taps(prm[0], prm[1], prm[2][:, :, :4], prm[3], 8)
    with pytest.raises(ValueError, match="mel_gate_taps"):
        ops.mel_gate_taps(prm[0][0], prm[1][0], prm[2][0], prm[3][0], 8)


def test_model_hands_every_layer_its_gate_and_get_gate_maps_skips_the_encoder():
    from mop_amd import ops
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=10, n_audio_ctx=40, vocab_size=50, n_text_ctx=16, n_embd=32, n_head=2, n_layer_enc=3, n_layer_dec=1)
    m = WhisperMoP(cfg).eval()
    mel = torch.randn(2, 12, 10)
    with torch.no_grad():
        for blk in m.encoder:
            blk.mop.fuse.alpha.copy_(torch.rand(2) + 0.5)
        want = torch.cat([blk.mop(mel.unsqueeze(1))[0] for blk in m.encoder], dim=2).transpose(1, 2)   # (B,L,T) from the convolutions
        ops.LAST_PATH.pop("sdpa_fwd", None)
        gates = m.get_gate_maps(mel)                                   # the attention cores have no CPU route: it must not reach them
    assert "sdpa_fwd" not in ops.LAST_PATH
    assert gates.shape == want.shape and gates.dtype == want.dtype
    assert float((gates - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def test_new_symbols_resolve(lib):
    from mop_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mopk.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mopk_(?:mel_gate|gated_residual)[a-z0-9_]*)\s*\(", src)))
    assert names == sorted(f"mopk_{op}_{what}" for op in ("mel_gate", "gated_residual")
                           for what in ("supported", "workspace_bytes", "fwd", "bwd"))
    for n in names:
        assert hasattr(lib, n) and n in _lib.SYMBOLS, n
    assert lib.mopk_version() == 118


def test_support_queries_need_no_gpu(lib):
    from mop_amd import _lib
    a = _lib.MelGateArgs()
    a.B, a.T, a.F, a.L, a.k, a.mel_st, a.mel_sb = 8, 1500, 80, 6, 5, 80, 1500 * 80
    assert lib.mopk_mel_gate_supported(C.byref(a)) == 1
    assert lib.mopk_mel_gate_workspace_bytes(C.byref(a)) == 256 * 6 * 5 * 80 * 4      # min(8 * ceil(1500 / 32), 256) partial rows
    a.B, a.T = 1, 33
    assert lib.mopk_mel_gate_workspace_bytes(C.byref(a)) == 2 * 6 * 5 * 80 * 4
    for field, bad in (("k", 4), ("k", 9), ("F", 129), ("L", 0), ("T", 0), ("mel_dtype", 2), ("mel_st", 79)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.mopk_mel_gate_supported(C.byref(a)) == 0 and lib.mopk_mel_gate_workspace_bytes(C.byref(a)) == 0, field
        setattr(a, field, keep)
    a.L, a.k, a.F, a.mel_st = 13, 7, 128, 128                                         # more layers than one launch holds
    assert lib.mopk_mel_gate_supported(C.byref(a)) == 1
    assert lib.mopk_mel_gate_fwd(C.byref(a), None) == -2 and lib.mopk_mel_gate_bwd(C.byref(a), None) == -2    # null pointers
    assert lib.mopk_mel_gate_fwd(None, None) < 0 and lib.mopk_mel_gate_bwd(None, None) < 0
    g = _lib.GatedResidualArgs()
    g.B, g.T, g.gate_sb = 2, 5, 5
    for D in (8, 384, 512, 768, 1024, 1280, 4, 12):
        g.D, g.x_st, g.a_st, g.x_sb, g.a_sb = D, D, D, 5 * D, 5 * D
        assert lib.mopk_gated_residual_supported(C.byref(g)) == (D % 8 == 0), D
    g.D, g.x_st, g.a_st, g.x_sb, g.a_sb = 512, 512, 512, 2560, 2560
    assert lib.mopk_gated_residual_workspace_bytes(C.byref(g)) == 0
    g.x_dtype, g.a_dtype, g.o_dtype = _lib.MOPK_BF16, _lib.MOPK_F32, _lib.MOPK_BF16   # the output is the promotion of x and a
    assert lib.mopk_gated_residual_supported(C.byref(g)) == 0
    g.o_dtype = _lib.MOPK_F32
    assert lib.mopk_gated_residual_supported(C.byref(g)) == 1
    g.x_st = 516
    assert lib.mopk_gated_residual_supported(C.byref(g)) == 0
    g.x_st = 520
    assert lib.mopk_gated_residual_supported(C.byref(g)) == 1
    assert lib.mopk_gated_residual_fwd(C.byref(g), None) == -2 and lib.mopk_gated_residual_bwd(C.byref(g), None) == -2
    assert lib.mopk_gated_residual_fwd(None, None) < 0 and lib.mopk_gated_residual_bwd(None, None) < 0
