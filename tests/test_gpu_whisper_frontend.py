"""GPU checks of the log-mel audio frontend: the mopk_log_mel kernels against the float64 restatement of
test_whisper_frontend_cpu.py and against ops.log_mel_torch on the same device tensors (a sweep of small shapes around the tile of
32 frames, a ragged batch over garbage, the clamp across workgroups, edge values, strides and dtypes), bit-exact repeats and
rows, the zero tail over recycled memory, no host sync, graph capture (in a process of its own), the torch fallback outside the
envelope, and LogMelFrontend feeding WhisperMoP.  Every comparison prints its figure before it asserts.

The sweep's T = 1 exists only at (400, 160, 80): at hop <= n_fft/4 a clip of one frame is shorter than the n_fft/2 + 1 samples a
reflection needs, so (16, 4, 3) and (64, 16, 10) start at the smallest legal clip (T = 2)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_whisper_frontend_cpu import (BF16_REL, SHAPES, SR, TOL_BROADBAND, TOL_PEAKED, filters_for, min_len, noise, pad_batch,
                                       ref_batch, sweep_lengths, tone)

pytestmark = pytest.mark.gpu
TOL = dict(broadband=TOL_BROADBAND, peaked=TOL_PEAKED)
GARBAGE = 1e4
DEF = (400, 160, 80)


def _rounded(clips, dtype):
    return [torch.from_numpy(np.asarray(c, dtype=np.float64)).to(dtype).double().numpy() for c in clips]


def check(clips, shape, cls, what, in_dtype=torch.float32, out_dtype=torch.float32, extra=0, fused=True):
    """the op's result on the clips (padded over garbage), after it matched the restatement, the torch path on the same device
    tensors matched it too, and the two matched each other"""
    from mop_amd import _lib, ops
    n_fft, hop, n_mels = shape
    filt = filters_for(n_fft, n_mels)
    audio, lens = pad_batch(clips, GARBAGE, in_dtype, extra)
    audio, lens = audio.cuda(), (lens.cuda() if len({len(c) for c in clips}) > 1 else None)
    want = torch.from_numpy(ref_batch(_rounded(clips, in_dtype), n_fft, hop, filt.double().numpy()))
    got = ops.log_mel(audio, filt.cuda(), n_fft, hop, lens, out_dtype)
    assert ops.LAST_PATH["log_mel"] == (_lib.PATH_FUSED if fused else _lib.PATH_GENERIC), what
    assert got.shape == want.shape and got.dtype == out_dtype, what
    composed = ops.log_mel_torch(audio, filt.cuda(), n_fft, hop, lens, out_dtype)
    bound = TOL[cls] + (BF16_REL * want.abs() if out_dtype == torch.bfloat16 else 0.0)
    e_k, e_t = (got.double().cpu() - want).abs(), (composed.double().cpu() - want).abs()
    e_kt = (got.double() - composed.double()).abs().cpu()
    print(f"{what} [{cls}]: kernel-f64 {float(e_k.max()):.3g} torch-f64 {float(e_t.max()):.3g} kernel-torch {float(e_kt.max()):.3g}")
    assert bool((e_k <= bound).all()), (what, float(e_k.max()))
    assert bool((e_t <= bound).all()), (what, float(e_t.max()))
    assert bool((e_kt <= 2 * bound).all()), (what, float(e_kt.max()))
    return got


# ------------------------------------------------------------------ the inputs (tools and the tests below share them)
def clamp_clip(tile):
    """3 tiles of frames at the defaults: 1e-4 noise, a full-scale tone over the samples of the last tile"""
    L = 3 * tile * 160 + 80
    x = noise(L, seed=21, scale=1e-4)
    x[2 * tile * 160 + 200:] += tone(L)[2 * tile * 160 + 200:]
    return x


def edge_clips():
    L = 160 * 40 + 77
    return dict(dc=np.full(L, 0.5), tone_noise=tone(L) + noise(L, seed=22, scale=1e-3))


def ragged_clips():
    return [noise(L, seed=30 + L) for L in (min_len(400, 160), 160 * 31 + 7, 160 * 32 + 1, 160 * 33 + 50, 160 * 67 + 80)]


# ------------------------------------------------------------------ the kernel against both references
@pytest.mark.parametrize("shape", SHAPES)
def test_small_sweep(shape):
    from mop_amd import ops
    n_fft, hop, _ = shape
    lengths = sweep_lengths(n_fft, hop, ops.LOG_MEL_TILE_FRAMES)
    assert sorted(L // hop for L in lengths)[-3:] == [32, 33, 67] and all(L % hop for L in lengths if hop > 1 and L > min_len(n_fft, hop))
    for L in lengths:
        check([noise(L, seed=L)], shape, "broadband", f"{shape} L = {L} (T = {L // hop})")
    check([noise(L, seed=L + 1) for L in lengths], shape, "broadband", f"{shape} all lengths in one batch")


def test_ragged_batch_over_garbage_rows_alone_and_the_zero_tail():
    from mop_amd import _lib, ops
    clips = ragged_clips()
    got = check(clips, DEF, "broadband", "ragged batch")
    filt = filters_for(400, 80).cuda()
    for b, c in enumerate(clips):                                          # each row bit for bit the clip alone
        alone = ops.log_mel(torch.from_numpy(c).float().cuda()[None], filt)
        assert ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED
        assert torch.equal(got[b, :len(c) // 160], alone[0]), b
        assert float(got[b, len(c) // 160:].abs().max() if len(c) // 160 < got.shape[1] else 0.0) == 0.0, b
    # the zero tail is written by the launch: the library called on buffers of this test's own, filled with garbage beforehand
    audio, lens = pad_batch(clips, GARBAGE)
    audio, lens = audio.cuda(), lens.cuda()
    for dtype, code in ((torch.float32, _lib.MOPK_F32), (torch.bfloat16, _lib.MOPK_BF16)):
        out = torch.full(got.shape, 1e30, dtype=dtype, device="cuda")
        a = ops._lm_args(audio, filt, 400, 160, lens, dtype, ops._lm_tables(400, audio.device, torch.float32), ops._lm_bands(filt))
        assert a.out_dtype == code
        a.out = out.data_ptr()
        ws = torch.full((_lib.lib().mopk_log_mel_workspace_bytes(a) // 4,), 1e30, dtype=torch.float32, device="cuda")
        a.workspace = ws.data_ptr()
        ops._launch("mopk_log_mel", a)
        torch.cuda.synchronize()
        assert torch.equal(out, got.to(dtype)), dtype                      # bf16: the same fp32 value, rounded once
        for b, c in enumerate(clips[:-1]):
            assert float(out[b, len(c) // 160:].float().abs().max()) == 0.0, (dtype, b)
    # without the band table (a C caller that has none) the sums run over every bin: the same numbers up to the order of zeros
    a = ops._lm_args(audio, filt, 400, 160, lens, torch.float32, ops._lm_tables(400, audio.device, torch.float32), None)
    out = torch.full(got.shape, 1e30, dtype=torch.float32, device="cuda")
    a.out, a.workspace = out.data_ptr(), ws.data_ptr()
    ops._launch("mopk_log_mel", a)
    torch.cuda.synchronize()
    assert torch.equal(out, got)


@pytest.mark.parametrize("reverse", [False, True])
def test_clamp_across_workgroups(reverse):
    from mop_amd import ops
    F = ops.LOG_MEL_TILE_FRAMES
    x = clamp_clip(F)
    x = x[::-1].copy() if reverse else x
    got = check([x], DEF, "peaked", f"quiet + loud tile, reversed = {reverse}")[0]
    quiet = got[F + 3:] if reverse else got[:2 * F - 3]                    # tiles whose own maximum is far under the clip's
    assert quiet.unique().numel() == 1                                     # all on the floor the loud tile sets
    assert abs(float(quiet[0, 0]) - (float(got.max()) - 2.0)) <= 1e-6


def test_edge_values():
    from mop_amd import _lib, ops
    filt = filters_for(400, 80).cuda()
    out = ops.log_mel(torch.zeros(2, 160 * 40 + 77, device="cuda"), filt)
    assert ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED and bool((out == -1.5).all())           # silence, exactly
    for name, x in edge_clips().items():
        check([x], DEF, "peaked", name)


def test_strides_and_dtypes():
    from mop_amd import _lib, ops
    clips = [noise(160 * 35 + 9, seed=40 + b) for b in range(6)]
    filt = filters_for(400, 80).cuda()
    full = check(clips, DEF, "broadband", "six rows")
    audio = pad_batch(clips, GARBAGE)[0].cuda()
    half = ops.log_mel(audio[::2], filt)                                   # audio[::2]: a row stride of 2 L
    assert ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED and torch.equal(half, full[::2])
    padded = check(clips, DEF, "broadband", "padded row stride", extra=9)
    assert torch.equal(padded, full)
    check(clips[:2], DEF, "broadband", "bf16 input", in_dtype=torch.bfloat16)
    check(clips[:2], DEF, "broadband", "fp16 input", in_dtype=torch.float16)
    check(clips[:2] + [clips[2][:700]], DEF, "broadband", "bf16 output", out_dtype=torch.bfloat16)
    assert not ops.log_mel_supported(audio.t().contiguous().t(), filt)     # an inner stride: the torch path
    check([noise(1024 * 3 + 5, seed=50)], (1024, 256, 20), "broadband", "n_fft = 1024: outside the envelope", fused=False)


def test_repeatable_and_no_host_sync():
    from mop_amd import _lib, ops
    clips = ragged_clips()
    audio, lens = pad_batch(clips, GARBAGE)
    audio, lens, filt = audio.cuda(), lens.cuda(), filters_for(400, 80).cuda()
    first, first_t = ops.log_mel(audio, filt, lens=lens), ops.log_mel(audio, filt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again, again_t = ops.log_mel(audio, filt, lens=lens), ops.log_mel(audio, filt)
        assert ops.log_mel_supported(audio, filt, lens=lens)
        ops.log_mel_torch(audio, filt, lens=lens)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED
    assert torch.equal(first, again) and torch.equal(first_t, again_t)


def test_graph_replay_reproduces_eager():
    """one captured ops.log_mel call (two launches in a line) replayed on new audio in its static buffer, in a process of its own
    (tools/graph_probe_whisper_frontend.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_frontend.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "REPLAY_IDENTICAL True" in r.stdout, r.stdout[-800:]


def test_frontend_feeds_the_model():
    from test_gpu_whisper_transcribe import RULES, V, _model
    from mop_amd import _lib, ops
    from mop_amd.nn import EncodedAudio, LogMelFrontend
    m = _model()
    fe = LogMelFrontend(12, SR, 64, 16).cuda()
    clips = [torch.from_numpy(noise(16 * T + 5, seed=T)).float().cuda() for T in (150, 64, 37)]
    mel = fe(clips)
    assert ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED and [tuple(x.shape) for x in mel] == [(150, 12), (64, 12), (37, 12)]
    want = ref_batch([c.double().cpu().numpy() for c in clips], 64, 16, fe.filters.double().cpu().numpy())
    for b, x in enumerate(mel):
        assert float((x.double().cpu() - torch.from_numpy(want[b, :x.shape[0]])).abs().max()) <= TOL_BROADBAND
    prompt = torch.tensor([7, 8, 9], device="cuda")
    rules = ops.LogitRules(V, **RULES, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        enc, _ = m.encode([x[:64] for x in mel])
        assert isinstance(enc, EncodedAudio) and enc.out.shape[:2] == (3, 64) and bool(torch.isfinite(enc.out).all())
        got = m.transcribe_audio(clips, fe, prompt, rules, 12, window=64)
        same = m.transcribe(fe(clips), prompt, rules, 12, window=64)
    assert len(got) == 3 and sum(t.tokens.numel() for t in got) > 0
    for g, w in zip(got, same):
        assert all(torch.equal(x, y) for x, y in zip(g, w))
