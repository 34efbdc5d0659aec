"""Whisper-MoP decoder line without a GPU: the reference's constructor / forward signatures (stated here, the reference tree is not
available to the tests), state_dict layouts against the whdec_ / whlm_ fixtures, the tied lm_head, the baseline factory, the
rectangular SDPA's C ABI field and its refusals (causal with Nk != N), and the (N, Nk) dropout mask."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden

# reference mop/models/whisper_mop.py
SIGNATURES = {
    "MultiheadCrossAttention.__init__": ["self", "dim_q", "dim_kv", "n_head", "dropout", "bias"],
    "MultiheadCrossAttention.forward": ["self", "x_q", "x_kv", "attn_mask"],
    "DecoderBlock.__init__": ["self", "cfg"],
    "DecoderBlock.forward": ["self", "x", "enc"],
    "WhisperMoP.__init__": ["self", "cfg"],
    "WhisperMoP.forward": ["self", "mel", "dec_input_ids", "targets"],
    "WhisperMoP.encode": ["self", "mel"],
    "WhisperMoP.decode": ["self", "enc_out", "dec_input_ids"],
    "WhisperMoP.get_gate_maps": ["self", "mel"],
    "create_whisper_mop": ["cfg"],
    "create_whisper_baseline": ["cfg"],
}
DEFAULTS = {"MultiheadCrossAttention.forward": {"attn_mask": None}, "WhisperMoP.forward": {"targets": None}}


def _tiny_cfg(**kw):
    from mop_amd.nn import WhisperConfig
    base = dict(n_mels=10, n_audio_ctx=40, vocab_size=100, n_text_ctx=16, n_embd=32, n_head=1, n_layer_enc=2, n_layer_dec=2,
                n_views=3, n_kernels=2, kernel_size=3)
    base.update(kw)
    return WhisperConfig(**base)


@pytest.mark.parametrize("qual", sorted(SIGNATURES))
def test_signatures_match_the_reference(qual):
    import mop_amd.nn as nn_
    obj = nn_
    for part in qual.split("."):
        obj = getattr(obj, part)
    sig = inspect.signature(obj)
    assert list(sig.parameters) == SIGNATURES[qual]
    for name, default in DEFAULTS.get(qual, {}).items():
        assert sig.parameters[name].default is default


def test_exports():
    from mop_amd.nn import (DecoderBlock, MultiheadCrossAttention, WhisperMoP, create_whisper_baseline,  # noqa: F401
                            create_whisper_mop)
    from mop_amd.nn.linear import TokenLinear
    ca = MultiheadCrossAttention(32, 48, 2, 0.0, True)
    assert all(isinstance(getattr(ca, n), TokenLinear) for n in ("q_proj", "k_proj", "v_proj", "o_proj"))
    assert ca.k_proj.weight.shape == (32, 48) and ca.v_proj.weight.shape == (32, 48) and ca.q_proj.weight.shape == (32, 32)


@pytest.mark.parametrize("name", golden_names("whdec_"))
def test_decoder_block_state_dict_matches_fixture(name):
    from mop_amd.nn import DecoderBlock
    d, params, gref, meta = load_golden(name)
    m = DecoderBlock(_tiny_cfg(n_embd=int(meta["dim"]), n_head=int(meta["heads"]), bias=bool(meta["bias"])))
    sd = m.state_dict()
    assert sorted(sd) == sorted(params)
    assert all(tuple(sd[k].shape) == params[k].shape for k in sd)
    assert sorted(k for k, _ in m.named_parameters()) == sorted(gref)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)


def _lm_from_meta(meta):
    from mop_amd.nn import create_whisper_baseline, create_whisper_mop
    cfg = _tiny_cfg(n_mels=int(meta["n_mels"]), n_audio_ctx=int(meta["T_a"]), vocab_size=int(meta["vocab"]),
                    n_text_ctx=int(meta["T_t"]), n_embd=int(meta["dim"]), n_head=int(meta["heads"]),
                    n_layer_enc=int(meta["n_layer_enc"]), n_layer_dec=int(meta["n_layer_dec"]), bias=bool(meta["bias"]),
                    use_abs_pos_emb=bool(meta["use_abs_pos_emb"]), n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]),
                    kernel_size=int(meta["kernel_size"]))
    return (create_whisper_mop if meta["model"] == "mop" else create_whisper_baseline)(cfg)


@pytest.mark.parametrize("name", golden_names("whlm_"))
def test_whisper_state_dict_matches_fixture(name):
    d, params, gref, meta = load_golden(name)
    m = _lm_from_meta(meta)
    sd = m.state_dict()
    assert sorted(sd) == sorted(params)
    assert all(tuple(sd[k].shape) == params[k].shape for k in sd)
    assert (m.audio_pos is None) == (not meta["use_abs_pos_emb"]) and (m.text_pos is None) == (not meta["use_abs_pos_emb"])
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    assert m.lm_head.weight is m.wte.weight


def test_tied_head_and_init():
    from mop_amd.nn import WhisperMoP
    torch.manual_seed(0)
    m = WhisperMoP(_tiny_cfg(bias=True))
    assert m.lm_head.weight is m.wte.weight
    assert abs(float(m.wte.weight.detach().std()) - 0.02) < 0.004
    blk = m.decoder[0]
    assert float(blk.cross_attn.q_proj.bias.abs().max()) == 0.0 and float(blk.ln2.weight.min()) == 1.0
    assert float(m.audio_proj.bias.abs().max()) == 0.0


def test_baseline_alphas_are_zero():
    from mop_amd.nn import create_whisper_baseline, create_whisper_mop
    base, mop = create_whisper_baseline(_tiny_cfg()), create_whisper_mop(_tiny_cfg())
    assert all(float(b.mop.fuse.alpha.abs().max()) == 0.0 for b in base.encoder)
    assert all(float(b.mop.fuse.alpha.min()) == 1.0 for b in mop.encoder)


def test_sdpa_args_has_key_length_last():
    from mop_amd import _lib
    names = [f[0] for f in _lib.SdpaArgs._fields_]
    assert names[-1] == "Nk" and dict(_lib.SdpaArgs._fields_)["Nk"] is C.c_int32


def test_ops_rejects_causal_rectangular_and_empty_keys():
    from mop_amd import ops
    q = torch.zeros(1, 8, 2, 32)
    k = torch.zeros(1, 12, 2, 32)
    with pytest.raises(ValueError, match="causal"):
        ops.sdpa_core(q, k, k.clone(), causal=True)
    with pytest.raises(ValueError):
        ops.sdpa_core(q, k, torch.zeros(1, 11, 2, 32))
    with pytest.raises(ValueError):
        ops.sdpa_core(q, torch.zeros(1, 0, 2, 32), torch.zeros(1, 0, 2, 32))


def test_c_abi_rejects_causal_rectangular():
    """the shape check comes before any device access: no GPU is needed to see the refusal"""
    from mop_amd import _lib
    lib = _lib.lib()
    a = _lib.SdpaArgs()
    a.B, a.H, a.N, a.dk, a.Nk = 1, 2, 64, 32, 100
    a.io_dtype, a.precision, a.path, a.causal = _lib.MOPK_BF16, _lib.PREC_BF16, _lib.PATH_AUTO, 1
    assert lib.mopk_sdpa_fwd(C.byref(a), None) == -3          # MOPK_ERR_UNSUPPORTED
    assert lib.mopk_sdpa_bwd(C.byref(a), None) == -3
    assert lib.mopk_sdpa_fused_supported(C.byref(a)) == 0
    assert lib.mopk_sdpa_saved_bytes(C.byref(a)) == 0 and lib.mopk_sdpa_workspace_bytes(C.byref(a)) == 0
    a.Nk = -1
    a.causal = 0
    assert lib.mopk_sdpa_fwd(C.byref(a), None) == -1          # MOPK_ERR_BAD_SHAPE


def test_saved_bytes_follow_the_key_length():
    from mop_amd import _lib
    lib = _lib.lib()
    a = _lib.SdpaArgs()
    a.B, a.H, a.N, a.dk = 1, 2, 48, 16                          # dk 16: the generic path, whose maps are N x Nk
    a.io_dtype, a.precision, a.path = _lib.MOPK_F32, _lib.PREC_FP32, _lib.PATH_AUTO
    square = lib.mopk_sdpa_saved_bytes(C.byref(a))
    a.Nk = 48
    assert lib.mopk_sdpa_saved_bytes(C.byref(a)) == square      # Nk = N is the square call
    a.Nk = 480
    assert lib.mopk_sdpa_saved_bytes(C.byref(a)) > 5 * square


def test_dropout_keep_mask_is_rectangular_and_matches_the_library():
    from mop_amd import _lib, ops
    lib = _lib.lib()
    seed, p, B, H, N, Nk = 0x1234_5678_9ABC, 0.3, 2, 3, 5, 70
    keep = ops.dropout_keep_mask(seed, p, B, H, N, Nk)
    assert keep.shape == (B, H, N, Nk)
    assert torch.equal(ops.dropout_keep_mask(seed, p, B, H, N)[..., :N], keep[..., :N])
    for bh in range(B * H):
        for i in range(N):
            for j in (0, 1, 33, 64, Nk - 1):
                assert bool(keep[bh // H, bh % H, i, j]) == bool(lib.mopk_dropout_keep(seed, p, bh, i, j))
