"""-m gpu: WhisperMoP's mel gate on the HIP kernels.  ops.mel_gate (mopk_mel_gate_*) against its torch twin in float64 on the same
taps -- T < k, F below a vector width, the 32-frame tile edge and its halo, F = 128, more layers than one launch holds, fp32 / bf16
/ strided and unaligned mel --, per-clip lengths over NaN, dW and the four parameter gradients against float64 autograd of the
convolutions, reproducibility; ops.gated_residual (mopk_gated_residual_*) against float64; every entry point between guard bands;
the model: the reference's fixture, get_gate_maps without the encoder, reproducible training, clips of different lengths, graph replay.

Bounds: mel_gate forward 1e-5 of |reference|max (the project's bound for its fp32-accumulating row kernels); dW and parameter
gradients 1e-4 relative (the fp32 fold's 2.9e-6 plus an fp32 reduction over B T); gated_residual 1e-6 in fp32 (two roundings),
2^-8 in bf16 (one bf16 rounding of the float64 result), dgate 1e-5 (an fp32 sum over D); model gates 1e-4 (test_gpu_whisper.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded_alloc import embedded, guarded_allocations
from test_whisper_gate_cpu import _conv_gates, _params

pytestmark = pytest.mark.gpu

FWD_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 1, 5), (3, 37, 10, 2, 3), (2, 65, 16, 3, 7), (2, 130, 80, 6, 5), (1, 257, 128, 1, 5),
              (2, 40, 16, 11, 3)]                       # B,T,F,L,k; the last: more layers than one launch holds (8)


MG_FWD_TOL, MG_BWD_TOL = 1e-5, 1e-4                   # mel gate against float64: the gates, the tap gradients
GR_TOL = {torch.float32: 1e-6, torch.bfloat16: 2.0 ** -8}      # gated residual against float64, by the dtype of the tensor
GR_DGATE_TOL = 1e-5


def _rel(got, ref):
    return float((got.detach().double().cpu() - ref.cpu()).abs().max() / ref.abs().max().clamp_min(1e-300))


def _taps(L, k, Fm, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(L, k, Fm, generator=g) / (k * Fm) ** 0.5).cuda()


def _mel(B, T, Fm, how, seed):
    """fp32 / bf16: contiguous; strided: a slice of a wider tensor whose rows stay on 16-byte boundaries where F allows it;
    offset: a slice that starts one element into its buffer"""
    g = torch.Generator().manual_seed(seed)
    if how == "strided":
        return torch.randn(B, T + 3, Fm + 16, generator=g).cuda()[:, 1:T + 1, 8:8 + Fm]
    if how == "offset":
        return torch.randn(B * T * Fm + 1, generator=g).cuda()[1:].view(B, T, Fm)
    m = torch.randn(B, T, Fm, generator=g).cuda()
    return m.to(torch.bfloat16) if how == "bf16" else m


@pytest.mark.parametrize("how", ["fp32", "bf16", "strided", "offset"])
@pytest.mark.parametrize("B,T,Fm,L,k", FWD_SHAPES)
def test_mel_gate_forward_against_float64(B, T, Fm, L, k, how):
    from mop_amd import _lib, ops
    W, mel = _taps(L, k, Fm, seed=1), _mel(B, T, Fm, how, seed=2)
    assert ops.mel_gate_supported(mel, W)
    ops.LAST_PATH.pop("mel_gate_fwd", None)
    got = ops.mel_gate(mel, W)
    assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_FUSED
    assert got.shape == (B, L, T) and got.dtype == torch.float32 and got.is_contiguous()
    ref = ops.mel_gate_torch(mel.double(), W.double())
    e = _rel(got, ref)
    print(f"mel_gate fwd {how} B={B} T={T} F={Fm} L={L} k={k}: {e:.3e} (bound 1e-5)")
    assert e <= MG_FWD_TOL


@pytest.mark.parametrize("T,Fm,L,k,lens", [(130, 80, 6, 5, (130, 1, 37, 64)), (70, 10, 2, 7, (70, 1, 33, 32)), (40, 16, 9, 3, (1, 40, 31, 2))])
def test_mel_gate_lens_over_poisoned_rows(T, Fm, L, k, lens):
    from mop_amd import _lib, ops
    W, mel = _taps(L, k, Fm, seed=3), _mel(len(lens), T, Fm, "fp32", seed=4)
    poisoned = embedded(mel)
    for b, n in enumerate(lens):
        poisoned[b, n:] = float("nan")
    dev_lens = torch.tensor(lens, dtype=torch.int32).cuda()
    got = ops.mel_gate(poisoned, W, dev_lens)
    assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_FUSED
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        alone = ops.mel_gate(mel[b:b + 1, :n].contiguous(), W)
        assert torch.equal(got[b, :, :n], alone[0]), b
        assert torch.equal(got[b, :, n:], torch.ones(L, T - n, device="cuda")), b


BWD_CASES = [(2, 130, 80, 5, 3, 5, 6, None), (3, 37, 10, 4, 2, 3, 2, None), (2, 70, 16, 5, 3, 7, 9, None),
             (3, 65, 16, 5, 3, 5, 3, (65, 1, 40))]      # B,T,F,V,K,k,L,lens


def _mel_gate_grads(mel, prm, dg, lens):
    from mop_amd import ops
    leaves = [p.detach().clone().requires_grad_() for p in prm]
    W = ops.mel_gate_taps(*leaves, mel.shape[2])
    W.retain_grad()
    (ops.mel_gate(mel, W, lens) * dg).sum().backward()
    torch.cuda.synchronize()
    return [W.grad] + [p.grad for p in leaves]


@pytest.mark.parametrize("how", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,Fm,V,K,k,L,lens", BWD_CASES)
def test_mel_gate_backward_against_float64_autograd_of_the_convolutions(B, T, Fm, V, K, k, L, lens, how):
    from mop_amd import _lib, ops
    torch.manual_seed(5)
    prm = [p.cuda() for p in _params(L, V, K, k, seed=6, dtype=torch.float32)]
    mel = _mel(B, T, Fm, how, seed=7)
    dg = torch.randn(B, L, T, device="cuda")
    dev_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    ops.LAST_PATH.pop("mel_gate_bwd", None)
    got = _mel_gate_grads(mel, prm, dg, dev_lens)
    assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["mel_gate_bwd"] == _lib.PATH_FUSED
    # float64: the clips cut to their lengths are what lens means (zero rows behind, no gradient from the columns behind)
    mel64, dg64 = mel.double(), dg.double()
    if lens is not None:
        live = (torch.arange(T, device="cuda").unsqueeze(0) < dev_lens.unsqueeze(1))
        mel64, dg64 = mel64 * live.unsqueeze(-1), dg64 * live.unsqueeze(1)
    p64 = [p.double().requires_grad_() for p in prm]
    ref = list(torch.autograd.grad(_conv_gates(mel64, *p64), p64, dg64))
    W64 = ops.mel_gate_taps(*[p.double() for p in prm], Fm).requires_grad_()
    ref.insert(0, torch.autograd.grad(ops.mel_gate_torch(mel64, W64), W64, dg64)[0])
    for name, g, r in zip(("dW", "Wv", "Wk", "Wf", "alpha"), got, ref):
        e = _rel(g.reshape(r.shape), r)
        print(f"mel_gate bwd {how} B={B} T={T} F={Fm} L={L} k={k} lens={lens} {name}: {e:.3e} (bound 1e-4)")
        assert e <= MG_BWD_TOL, name
    again = _mel_gate_grads(mel, prm, dg, dev_lens)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_a_mel_that_requires_grad_runs_the_torch_twin():
    from mop_amd import _lib, ops
    W, mel = _taps(2, 5, 16, seed=8).requires_grad_(), _mel(2, 20, 16, "fp32", seed=9).requires_grad_()
    assert not ops.mel_gate_supported(mel, W) and ops.mel_gate_supported(mel.detach(), W)
    ops.mel_gate(mel, W).square().sum().backward()
    assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_GENERIC
    assert mel.grad is not None and torch.isfinite(mel.grad).all() and float(mel.grad.abs().max()) > 0 and W.grad is not None


# ---- ops.gated_residual ----------------------------------------------------------------------------------------------------------
GR_SHAPES = [(1, 1, 8), (2, 5, 64), (3, 37, 384), (2, 19, 1280)]
GR_DTYPES = {"fp32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "mixed": (torch.float32, torch.bfloat16)}


def _gr_case(B, T, D, dt, seed=10, strided=False):
    g = torch.Generator().manual_seed(seed)
    xdt, adt = GR_DTYPES[dt]
    odt = torch.float32 if torch.float32 in (xdt, adt) else torch.bfloat16
    if strided:                                           # rows of a wider tensor, the gate one layer of a (B,L,T) tensor
        x = torch.randn(B, T, D + 8, generator=g).cuda().to(xdt)[:, :, :D]
        a = torch.randn(B, T + 1, D, generator=g).cuda().to(adt)[:, 1:]
        gate = (1 + 0.5 * torch.randn(B, 3, T, generator=g)).cuda()[:, 1]
    else:
        x, a = torch.randn(B, T, D, generator=g).cuda().to(xdt), torch.randn(B, T, D, generator=g).cuda().to(adt)
        gate = (1 + 0.5 * torch.randn(B, T, generator=g)).cuda()
    dout = torch.randn(B, T, D, generator=g).cuda().to(odt)
    return x, a, gate, dout, odt


def _gr_run(x, a, gate, dout):
    from mop_amd import ops
    x, a, gate = (t.detach().requires_grad_() for t in (x, a, gate))
    out = ops.gated_residual(x, a, gate)
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach(), x.grad, a.grad, gate.grad


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dt", list(GR_DTYPES))
@pytest.mark.parametrize("B,T,D", GR_SHAPES)
def test_gated_residual_against_float64(B, T, D, dt, strided):
    from mop_amd import _lib, ops
    x, a, gate, dout, odt = _gr_case(B, T, D, dt, strided=strided)
    assert ops.gated_residual_supported(x, a, gate)
    for key in ("gated_residual_fwd", "gated_residual_bwd"):
        ops.LAST_PATH.pop(key, None)
    out, dx, da, dgate = _gr_run(x, a, gate, dout)
    assert ops.LAST_PATH["gated_residual_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["gated_residual_bwd"] == _lib.PATH_FUSED
    assert out.dtype == odt and dx.dtype == x.dtype and da.dtype == a.dtype and dgate.dtype == torch.float32 and dgate.shape == (B, T)
    r64 = x.double() + a.double()
    ref_out, ref_dr, ref_dg = r64 * gate.double().unsqueeze(-1), dout.double() * gate.double().unsqueeze(-1), (dout.double() * r64).sum(-1)
    tol = GR_TOL
    for name, got, ref, bound in (("out", out, ref_out, tol[odt]), ("dx", dx, ref_dr, tol[x.dtype]), ("da", da, ref_dr, tol[a.dtype]),
                                  ("dgate", dgate, ref_dg, GR_DGATE_TOL)):
        e = _rel(got, ref)
        print(f"gated_residual {dt} B={B} T={T} D={D} strided={strided} {name}: {e:.3e} (bound {bound:.1e})")
        assert e <= bound, name
    again = _gr_run(x, a, gate, dout)
    assert all(torch.equal(p, q) for p, q in zip((out, dx, da, dgate), again))


def test_gated_residual_takes_a_bf16_gate_and_refuses_what_the_kernels_cannot_read():
    from mop_amd import _lib, ops
    x, a, gate, dout, _ = _gr_case(2, 5, 64, "mixed")
    out = ops.gated_residual(x, a, gate.to(torch.bfloat16))
    assert ops.LAST_PATH["gated_residual_fwd"] == _lib.PATH_FUSED
    assert torch.equal(out, ops.gated_residual(x, a, gate.to(torch.bfloat16).float()))
    for bx, ba in ((x[:, :, :60], a[:, :, :60].float()), (x.double(), a.double()), (x.half(), a.half())):
        assert not ops.gated_residual_supported(bx, ba, gate)
        out = ops.gated_residual(bx, ba, gate)
        assert ops.LAST_PATH["gated_residual_fwd"] == _lib.PATH_GENERIC
        assert torch.equal(out, ops.gated_residual_torch(bx, ba, gate))


def test_odd_gradients_are_taken_in_and_a_second_differentiation_raises():
    """a stride-0 gradient (what .sum() hands a backward) and a sliced one go through ops._grad_in; the kernels' gradients carry no
    graph, so differentiating them again raises (ops._once_differentiable)"""
    from mop_amd import ops
    x, a, gate, dout, _ = _gr_case(2, 5, 64, "fp32", seed=15)
    W, mel = _taps(2, 5, 16, seed=16), _mel(2, 20, 16, "fp32", seed=17)
    wide = torch.randn(2, 5, 128, generator=torch.Generator().manual_seed(18)).cuda()
    x, a, gate, W = (t.requires_grad_() for t in (x, a, gate, W))
    for dy in (torch.ones((), device="cuda").expand(2, 5, 64), wide[:, :, 3:67]):
        got = torch.autograd.grad(ops.gated_residual(x, a, gate), (x, gate), dy)
        ref = torch.autograd.grad(ops.gated_residual_torch(x, a, gate), (x, gate), dy)
        assert all(_rel(g, r.double()) <= 1e-5 for g, r in zip(got, ref))
    dg = torch.ones((), device="cuda").expand(2, 2, 20)
    (got,), (ref,) = torch.autograd.grad(ops.mel_gate(mel, W), W, dg), torch.autograd.grad(ops.mel_gate_torch(mel, W), W, dg)
    assert _rel(got, ref.double()) <= 1e-5
    for out, leaf in ((ops.gated_residual(x, a, gate), gate), (ops.mel_gate(mel, W), W)):
        (g,) = torch.autograd.grad(out.sum(), leaf, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g.square().sum().backward()


# ---- every entry point between guard bands ----------------------------------------------------------------------------------------
def _guarded_twice(call, inputs, paths):
    """call(dict of tensors) -> tuple of results, once on plain tensors and once with every input embedded in NaN and every buffer
    the ops allocate handed out between guard bands: guards intact, finite, bit-identical results, on the kernels"""
    from mop_amd import _lib, ops
    plain = call({k: t.detach().clone() for k, t in inputs.items()})
    torch.cuda.synchronize()
    for k in paths:
        ops.LAST_PATH.pop(k, None)
    with guarded_allocations() as ledger:
        guarded = call({k: embedded(t) for k, t in inputs.items()})
        torch.cuda.synchronize()
    assert ledger.intact(), ledger.describe_damage()
    assert ledger.count() > 0
    assert all(ops.LAST_PATH[k] == _lib.PATH_FUSED for k in paths)
    for p, g in zip(plain, guarded):
        assert torch.isfinite(g).all() and torch.equal(p, g)


@pytest.mark.parametrize("how", ["fp32", "bf16"])
def test_mel_gate_entry_points_stay_inside_their_buffers(how):
    from mop_amd import ops
    B, T, Fm, L, k = 3, 70, 80, 9, 5
    lens = torch.tensor([70, 33, 1], dtype=torch.int32)

    def call(t):
        W = t["W"].requires_grad_()
        gates = ops.mel_gate(t["mel"], W, t["lens"])
        gates.backward(t["dg"])
        return gates.detach(), W.grad
    _guarded_twice(call, dict(mel=_mel(B, T, Fm, how, seed=11), W=_taps(L, k, Fm, seed=12), lens=lens.cuda(),
                              dg=torch.randn(B, L, T, generator=torch.Generator().manual_seed(13)).cuda()),
                   ("mel_gate_fwd", "mel_gate_bwd"))


@pytest.mark.parametrize("dt", list(GR_DTYPES))
def test_gated_residual_entry_points_stay_inside_their_buffers(dt):
    x, a, gate, dout, _ = _gr_case(3, 37, 384, dt, seed=14)
    _guarded_twice(lambda t: _gr_run(t["x"], t["a"], t["gate"], t["dout"]), dict(x=x, a=a, gate=gate, dout=dout),
                   ("gated_residual_fwd", "gated_residual_bwd"))


# ---- the model --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whlm_mop():
    from mop_amd.nn import WhisperConfig, create_whisper_mop
    d, params, _, meta = load_golden("whlm_mop")
    cfg = WhisperConfig(n_mels=int(meta["n_mels"]), n_audio_ctx=int(meta["T_a"]), vocab_size=int(meta["vocab"]), n_text_ctx=int(meta["T_t"]),
                        n_embd=int(meta["dim"]), n_head=int(meta["heads"]), n_layer_enc=int(meta["n_layer_enc"]),
                        n_layer_dec=int(meta["n_layer_dec"]), bias=bool(meta["bias"]), use_abs_pos_emb=bool(meta["use_abs_pos_emb"]),
                        n_views=int(meta["n_views"]), n_kernels=int(meta["n_kernels"]), kernel_size=int(meta["kernel_size"]))
    m = create_whisper_mop(cfg)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}, strict=True)
    return d, m.cuda().eval()


def test_model_gates_match_the_reference_and_get_gate_maps_skips_the_encoder(whlm_mop):
    from mop_amd import _lib, ops
    d, m = whlm_mop
    mel, idx = torch.from_numpy(d["mel"]).cuda(), torch.from_numpy(d["idx"]).cuda()
    with torch.no_grad():
        ops.LAST_PATH.pop("mel_gate_fwd", None)
        _, _, gates = m(mel, idx)
        assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["gated_residual_fwd"] == _lib.PATH_FUSED
        ref = torch.from_numpy(d["gates"])
        e = float((gates.cpu().double() - ref.double()).abs().max())
        print(f"model gates against the reference: {e:.3e} (bound {1e-4 * max(1.0, float(ref.abs().max())):.3e})")
        assert gates.shape == ref.shape and gates.dtype == torch.float32
        assert e <= 1e-4 * max(1.0, float(ref.abs().max()))
        ops.LAST_PATH.pop("sdpa_fwd", None)
        maps = m.get_gate_maps(mel)
        torch.cuda.synchronize()
        assert "sdpa_fwd" not in ops.LAST_PATH                      # no attention kernel: the encoder was not run
        assert torch.equal(maps, gates)


def test_model_training_step_is_bitwise_reproducible_without_deterministic_convolutions(whlm_mop):
    d, m = whlm_mop
    assert not torch.backends.cudnn.deterministic
    mel, idx, tgt = (torch.from_numpy(d[k]).cuda() for k in ("mel", "idx", "targets"))
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        logits, loss, _ = m(mel, idx, tgt)
        loss.backward()
        torch.cuda.synchronize()
        runs.append([logits.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))
    for blk in m.encoder:                                            # the gate's parameters are part of what was compared
        assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in blk.mop.parameters())
    m.zero_grad(set_to_none=True)


def test_model_clips_of_different_lengths_equal_each_clip_alone():
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=200, vocab_size=300, n_text_ctx=64, n_embd=128, n_head=2, n_layer_enc=3, n_layer_dec=1)
    m = WhisperMoP(cfg).cuda().eval()
    with torch.no_grad():
        for blk in m.encoder:
            blk.mop.fuse.alpha.copy_(torch.rand(2) + 0.5)
        clips = [torch.randn(n, 12).cuda() for n in (200, 37, 1, 130)]
        enc, gates = m.encode(clips)
        assert gates.shape == (4, 3, 200) and enc.lens.tolist() == [200, 37, 1, 130]
        for b, c in enumerate(clips):
            n = c.shape[0]
            ro, rg = m.encode(c.unsqueeze(0))
            assert float((gates[b, :, :n] - rg[0]).abs().max()) <= 1e-4, b
            assert torch.equal(gates[b, :, n:], torch.ones(3, 200 - n, device="cuda")), b
            e = float((enc.out[b, :n] - ro[0]).abs().max() / max(1.0, float(ro.abs().max())))
            print(f"clip {b} ({n} frames): encoder rows {e:.3e} (bound 1e-4)")
            assert e <= 1e-4, b


def test_graph_replay_of_encode_reproduces_eager():
    """encode captured with torch.cuda.graph (the warm-up outside the capture) and replayed on new mel values, in its own process
    (tools/graph_probe_whisper_gate.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_gate.py")], cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-600:]
