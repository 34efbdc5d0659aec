"""-m gpu: rectangular plain SDPA (N queries, Nk keys: cross-attention) and the Whisper-MoP decoder on the MI355X.  The core against
float64 torch over lengths at the 64-token tile edges, head sizes, io dtypes, precisions, both paths and strided views, with
mask / bias / dropout; causal rectangular refusals; DecoderBlock / WhisperMoP parity with the reference's fixtures (fp32 arithmetic
<= 1e-3, bf16 MFMA <= 1e-2 on values, scaled by the reference's own bf16 noise on gradients); one Whisper-size cross-attention;
bitwise-reproducible backward of the tiny model."""
import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
from gpu_util import check_grads, max_abs, rel_err

pytestmark = pytest.mark.gpu
TOL = {"fp32": (1e-3, 1e-3), "bf16": (1e-2, 3e-2)}


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _ref64(q, k, v, mask=None, bias=None, keep=None, p=0.0):
    """float64 softmax(q k^T / sqrt(dk) [+ bias] [mask]) [dropout] v; q (B,N,H,dk), k, v (B,Nk,H,dk) -> (B,N,H*dk)"""
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5
    if bias is not None:
        s = s + bias.double()
    if mask is not None:
        s = s.masked_fill(mask == 0, float("-inf"))
    a = torch.softmax(s, -1)
    if keep is not None:
        a = a * keep.to(a.device).double() / (1.0 - p)
    y = a @ v
    return y.transpose(1, 2).reshape(q.shape[0], q.shape[2], -1)


def _qkv(B, N, Nk, H, dk, dtype, strided, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:         # q: first half of a 2dk-wide row; k, v: two views of one (B, Nk, 2, H, dk) buffer
        q = torch.randn(B, N, H, 2 * dk, device="cuda", generator=g).to(dtype)[..., :dk]
        kv = torch.randn(B, Nk, 2, H, dk, device="cuda", generator=g).to(dtype)
        k, v = kv[:, :, 0], kv[:, :, 1]
    else:
        q = torch.randn(B, N, H, dk, device="cuda", generator=g).to(dtype)
        k = torch.randn(B, Nk, H, dk, device="cuda", generator=g).to(dtype)
        v = torch.randn(B, Nk, H, dk, device="cuda", generator=g).to(dtype)
    return [t.detach().requires_grad_(True) for t in (q, k, v)]


def _grad_errs(pairs, floor):
    """max-abs error of each gradient over max(|ref|max, floor x the call's largest reference gradient), as gpu_util.check_grads
    normalises: with one key (Nk = 1) the softmax is constant and dq, dk are analytically zero"""
    refs = [b.grad.cpu().numpy() for _, _, b in pairs]
    gscale = max(float(np.abs(r).max()) for r in refs)
    return {name: max_abs(a.grad.float().cpu().numpy(), r) / max(float(np.abs(r).max()), floor * gscale, 1e-30)
            for (name, a, _), r in zip(pairs, refs)}


def _check_core(N, Nk, dk, io, mode, strided=False, with_mask=False, with_bias=False, H=2, B=1, seed=0):
    import mop_amd
    from mop_amd import _lib, ops
    prec, path = {"fp32-generic": ("fp32", "generic"), "bf16-generic": ("bf16", "generic"), "bf16-fused": ("bf16", "fused")}[mode]
    mop_amd.set_precision(prec)
    ops.set_path(path)
    dtype = torch.float32 if io == "fp32" else torch.bfloat16
    q, k, v = _qkv(B, N, Nk, H, dk, dtype, strided, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    mask = bias = None
    if with_mask:
        mask = (torch.rand(N, Nk, device="cuda", generator=g) > 0.3)
        mask[:, 0] = True                                   # every query keeps a key
    if with_bias:
        bias = torch.randn(B, 1, N, Nk, device="cuda", generator=g)
    ops.LAST_PATH.pop("sdpa_fwd", None)
    y = ops.sdpa_core(q, k, v, attn_mask=mask, bias=bias)
    w = torch.randn(y.shape, device="cuda", generator=g)
    (y.float() * w).sum().backward()
    want = _lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC
    assert ops.LAST_PATH["sdpa_fwd"] == want and ops.LAST_PATH["sdpa_bwd"] == want
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    yr = _ref64(q64, k64, v64, mask, bias)
    (yr * w.double()).sum().backward()
    tol, gtol = (1e-3, 1e-3) if (prec == "fp32" and io == "fp32") else (2e-2, 3e-2)
    assert y.shape == (B, N, H * dk)
    assert rel_err(y.detach().float().cpu().numpy(), yr.detach().cpu().numpy()) <= tol
    pairs = (("dq", q, q64), ("dk", k, k64), ("dv", v, v64))
    assert all(a.grad.shape == b.shape for _, a, b in pairs)
    # Nk = 1: dq, dk are analytically zero, and on bf16 arithmetic with fp32 io they are p (dP - delta) with dP from the bf16-rounded
    # dy and delta from the fp32 one -- one bf16 rounding of dy . v, ~1e-3 of the call's gradient scale; judged at that scale
    floor = 1e-3 if tol == 1e-3 else 1e-1 if Nk == 1 else 1e-2
    for name, err in _grad_errs(pairs, floor).items():
        assert err <= gtol, f"{name} {err:.3e}"


PAIRS = [(1, 1500), (63, 64), (64, 65), (65, 63), (1, 63), (64, 1), (200, 1500), (448, 1500), (1500, 448), (448, 200), (65, 200)]
MODES = ["fp32-generic", "bf16-generic", "bf16-fused"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("dk", [32, 64])
@pytest.mark.parametrize("N,Nk", PAIRS)
def test_rectangular_core_matches_float64(N, Nk, dk, io, mode):
    _check_core(N, Nk, dk, io, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,Nk", [(37, 150), (130, 65)])
def test_rectangular_core_strided_masked_biased(N, Nk, mode):
    _check_core(N, Nk, 32, "bf16", mode, strided=True, with_mask=True, with_bias=True, B=2)
    _check_core(N, Nk, 64, "fp32", mode, strided=True, with_mask=True, B=2, seed=3)
    _check_core(N, Nk, 64, "fp32", mode, with_bias=True, B=2, seed=5)


@pytest.mark.parametrize("path", ["fused", "generic"])
def test_rectangular_dropout_mask_is_the_counter(path):
    import mop_amd
    from mop_amd import _lib, ops
    B, N, Nk, H, dk, p, seed = 2, 70, 150, 2, 32, 0.3, 0x5EED_1234
    mop_amd.set_precision("bf16")
    ops.set_path(path)
    q, k, v = _qkv(B, N, Nk, H, dk, torch.float32, False, 11)
    y = ops.sdpa_core(q, k, v, dropout_p=p, seed=seed)
    assert ops.LAST_PATH["sdpa_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    keep = ops.dropout_keep_mask(seed, p, B, H, N, Nk)
    assert keep.shape == (B, H, N, Nk) and 0.6 < float(keep.float().mean()) < 0.8
    w = torch.randn(y.shape, device="cuda")
    (y * w).sum().backward()
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    yr = _ref64(q64, k64, v64, keep=keep, p=p)
    (yr * w.double()).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), yr.detach().cpu().numpy()) <= 2e-2
    for name, err in _grad_errs((("dq", q, q64), ("dk", k, k64), ("dv", v, v64)), 1e-2).items():
        assert err <= 3e-2, f"{name} {err:.3e}"
    # a different mask is visibly different: the test above would catch a square (N x N) or transposed draw
    yw = _ref64(q64, k64, v64, keep=ops.dropout_keep_mask(seed + 1, p, B, H, N, Nk), p=p)
    assert rel_err(y.detach().cpu().numpy(), yw.detach().cpu().numpy()) > 0.1


def test_fused_and_generic_dropout_agree():
    import mop_amd
    from mop_amd import ops
    mop_amd.set_precision("bf16")
    q, k, v = _qkv(1, 100, 333, 2, 64, torch.bfloat16, False, 21)
    outs = []
    for path in ("fused", "generic"):
        ops.set_path(path)
        outs.append(ops.sdpa_core(q, k, v, dropout_p=0.2, seed=77).float().detach())
    assert rel_err(outs[0].cpu().numpy(), outs[1].cpu().numpy()) <= 2e-2


def test_causal_rectangular_is_rejected():
    import ctypes as C
    from mop_amd import _lib, ops
    q, k, v = _qkv(1, 64, 100, 2, 32, torch.bfloat16, False, 0)
    with pytest.raises(ValueError, match="causal"):
        ops.sdpa_core(q, k, v, causal=True)
    a = _lib.SdpaArgs()
    a.B, a.H, a.N, a.dk, a.Nk, a.causal = 1, 2, 64, 32, 100, 1
    a.io_dtype, a.precision, a.path = _lib.MOPK_BF16, _lib.PREC_BF16, _lib.PATH_FUSED
    a.q, a.k, a.v = ops._v4(q), ops._v4(k), ops._v4(v)
    y = torch.empty_like(q)
    a.y = ops._v4(y)
    a.saved = a.workspace = y.data_ptr()
    assert _lib.lib().mopk_sdpa_fwd(C.byref(a), None) == -3
    # the square causal call still runs
    ys = ops.sdpa_core(q, q, q, causal=True)
    assert torch.isfinite(ys.float()).all()


# ---- the reference's fixtures -------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from mop_amd.nn import WhisperConfig
    return WhisperConfig(**kw)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", golden_names("whdec_"))
def test_decoder_block_matches_the_reference(name, prec):
    import mop_amd
    from mop_amd import _lib, ops
    from mop_amd.nn import DecoderBlock
    d, params, gref, meta = load_golden(name)
    mop_amd.set_precision(prec)
    m = DecoderBlock(_cfg(n_embd=int(meta["dim"]), n_head=int(meta["heads"]), bias=bool(meta["bias"]), n_audio_ctx=int(meta["T_a"]),
                          n_text_ctx=int(meta["T_t"])))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    m = m.cuda().eval()
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    enc = torch.from_numpy(d["enc"]).cuda().requires_grad_(True)
    y = m(x, enc)
    y.backward(torch.from_numpy(d["w"]).cuda())
    torch.cuda.synchronize()
    fused = prec == "bf16" and int(meta["dim"]) // int(meta["heads"]) in (32, 64)
    assert ops.LAST_PATH["sdpa_fwd"] == (_lib.PATH_FUSED if fused else _lib.PATH_GENERIC)
    tol, gtol = TOL[prec]
    assert max_abs(y.detach().cpu().numpy(), d["y"]) <= tol * max(1.0, float(np.abs(d["y"]).max()))
    noise = (lambda k: 4.0 * float(d["bf16err:" + k])) if prec == "bf16" else (lambda k: 0.0)
    for k, ours in (("dx", x.grad), ("denc", enc.grad)):
        err = rel_err(ours.cpu().numpy(), d[k])
        assert err <= max(gtol, noise(k)), f"{k} {err:.3e}"
    grads = {k: p.grad.float().cpu().numpy() for k, p in m.named_parameters()}
    check_grads(grads, gref, gtol, floor=1e-2 if prec == "bf16" else 1e-3, d=d if prec == "bf16" else None)


def _lm_from_golden(name):
    from mop_amd.nn import create_whisper_baseline, create_whisper_mop
    d, params, gref, meta = load_golden(name)
    cfg = _cfg(n_mels=int(meta["n_mels"]), n_audio_ctx=int(meta["T_a"]), vocab_size=int(meta["vocab"]), n_text_ctx=int(meta["T_t"]),
               n_embd=int(meta["dim"]), n_head=int(meta["heads"]), n_layer_enc=int(meta["n_layer_enc"]),
               n_layer_dec=int(meta["n_layer_dec"]), bias=bool(meta["bias"]), use_abs_pos_emb=bool(meta["use_abs_pos_emb"]),
               n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]), kernel_size=int(meta["kernel_size"]))
    m = (create_whisper_mop if meta["model"] == "mop" else create_whisper_baseline)(cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    return d, gref, meta, m.cuda().eval()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", golden_names("whlm_"))
def test_whisper_model_matches_the_reference(name, prec):
    import mop_amd
    from mop_amd import _lib, ops
    d, gref, meta, m = _lm_from_golden(name)
    mop_amd.set_precision(prec)
    mel, idx, tgt = (torch.from_numpy(d[k]).cuda() for k in ("mel", "idx", "targets"))
    logits, loss, gates = m(mel, idx, tgt)
    loss.backward()
    torch.cuda.synchronize()
    assert ops.LAST_PATH["sdpa_fwd"] == (_lib.PATH_FUSED if prec == "bf16" else _lib.PATH_GENERIC)
    tol, gtol = TOL[prec]
    assert max_abs(logits.detach().cpu().numpy(), d["logits"]) <= tol
    assert abs(float(loss.detach()) - float(d["loss"])) <= max(tol, 4.0 * float(d["bf16err:loss"]) if prec == "bf16" else 0.0)
    assert max_abs(gates.detach().cpu().numpy(), d["gates"]) <= 1e-4 * max(1.0, float(np.abs(d["gates"]).max()))
    with torch.no_grad():
        assert torch.equal(m.get_gate_maps(mel), gates.detach())
    grads = {k: p.grad.float().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    check_grads(grads, gref, gtol, scalar_tol=5e-2 if prec == "bf16" else None, floor=1e-2 if prec == "bf16" else 1e-3,
                d=d if prec == "bf16" else None)


def test_reference_forward_shapes():
    """reference usage: WhisperMoP(cfg)(mel, ids, targets) -> (logits, loss, gates), with dropout in training mode"""
    from mop_amd.nn import create_whisper_baseline, create_whisper_mop
    cfg = _cfg(n_mels=16, n_audio_ctx=96, vocab_size=120, n_text_ctx=40, n_embd=64, n_head=2, n_layer_enc=2, n_layer_dec=2,
               dropout=0.1)
    mel = torch.randn(2, 96, 16, device="cuda")
    ids = torch.randint(0, 120, (2, 40), device="cuda")
    for make in (create_whisper_mop, create_whisper_baseline):
        m = make(cfg).cuda().train()
        logits, loss, gates = m(mel, ids, ids)
        loss.backward()
        assert logits.shape == (2, 40, 120) and gates.shape == (2, 2, 96) and torch.isfinite(loss)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


# ---- Whisper size, reproducibility ---------------------------------------------------------------------------------------------
def test_whisper_size_cross_attention():
    """T_t = 448 queries against T_a = 1500 keys, d = 384, H = 6 (head size 64), bf16 on the fused kernels; float64 on 2 heads"""
    import mop_amd
    from mop_amd import _lib, ops
    from mop_amd.nn import MultiheadCrossAttention
    mop_amd.set_precision("auto")
    torch.manual_seed(0)
    ca = MultiheadCrossAttention(384, 384, 6, 0.0, False).cuda().to(torch.bfloat16).eval()
    xq = torch.randn(2, 448, 384, device="cuda", dtype=torch.bfloat16)
    xkv = torch.randn(2, 1500, 384, device="cuda", dtype=torch.bfloat16)
    H, Dh = 6, 64
    q = ca.q_proj(xq).view(2, 448, H, Dh).detach().requires_grad_(True)
    k = ca.k_proj(xkv).view(2, 1500, H, Dh).detach().requires_grad_(True)
    v = ca.v_proj(xkv).view(2, 1500, H, Dh).detach().requires_grad_(True)
    y = ops.sdpa_core(q, k, v)
    assert ops.LAST_PATH["sdpa_fwd"] == _lib.PATH_FUSED
    w = torch.randn(y.shape, device="cuda")
    (y.float() * w).sum().backward()
    hs = slice(2, 4)
    q64, k64, v64 = (t.detach()[:, :, hs].double().requires_grad_(True) for t in (q, k, v))
    yr = _ref64(q64, k64, v64)
    (yr * w.view(2, 448, H, Dh)[:, :, hs].reshape(2, 448, -1).double()).sum().backward()
    ys = y.detach().view(2, 448, H, Dh)[:, :, hs].reshape(2, 448, -1)
    assert rel_err(ys.float().cpu().numpy(), yr.detach().cpu().numpy()) <= 2e-2
    for a, b in ((q, q64), (k, k64), (v, v64)):
        assert rel_err(a.grad[:, :, hs].float().cpu().numpy(), b.grad.cpu().numpy()) <= 3e-2
    out = ca(xq, xkv)
    assert out.shape == (2, 448, 384) and torch.isfinite(out.float()).all()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_backward_is_bitwise_reproducible(prec):
    import mop_amd
    mop_amd.set_precision(prec)
    name = golden_names("whlm_")[0]
    d, gref, meta, m = _lm_from_golden(name)
    mel, idx, tgt = (torch.from_numpy(d[k]).cuda() for k in ("mel", "idx", "targets"))
    runs, det = [], torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                    # the MoP2D convolutions: deterministic MIOpen solvers
    try:
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            logits, loss, _ = m(mel, idx, tgt)
            loss.backward()
            torch.cuda.synchronize()
            runs.append([logits.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
    finally:
        torch.backends.cudnn.deterministic = det
    assert all(torch.equal(a, b) for a, b in zip(*runs))
