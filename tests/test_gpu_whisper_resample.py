"""GPU checks of the audio resampler: the mopk_resample kernel against the float64 restatement of test_whisper_resample_cpu.py
(under the tolerance derived there) and against ops.resample_torch on the same device tensors: the sweep of small lengths around
the tile of 1024 outputs, a ragged batch over garbage (clips bit for bit as alone, the zero tail and out_lens over recycled memory),
dtypes, strides and channel layouts, guard bands and NaN poison around every buffer, bit-exact repeats without a host sync, graph
capture (in a process of its own), the torch path outside the envelope, and ResampledLogMelFrontend feeding WhisperMoP.  Every
comparison prints its figure before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from guarded_alloc import embedded, guarded_allocations
from test_whisper_resample_cpu import (BF16_REL, NEW, SWEEP_PAIRS, len_for, noise, out_len, pad_batch, ragged_clips, ref_batch, ref_mono,
                                       ref_resample, sweep_lengths, tol)

pytestmark = pytest.mark.gpu
GARBAGE = 1e4


def _rounded(clips, dtype):
    """the clips as the kernel reads them from `dtype` storage, float64"""
    if dtype == torch.int16:
        return [np.round(np.asarray(c) * 32767).astype(np.int16).astype(np.float64) / 32768 for c in clips]
    return [torch.from_numpy(np.asarray(c, dtype=np.float64)).to(dtype).double().numpy() for c in clips]


def _stored(clips, dtype):
    return [np.round(np.asarray(c) * 32767) for c in clips] if dtype == torch.int16 else clips


def check(clips, orig, new, what, in_dtype=torch.float32, out_dtype=torch.float32, extra=0, fused=True):
    """the op's result on the mono clips (padded over garbage), after it matched the restatement, the torch path on the same device
    tensors matched it too, and the two matched each other"""
    from mop_amd import _lib, ops
    audio, lens = pad_batch(_stored(clips, in_dtype), GARBAGE, in_dtype, extra)
    audio, lens = audio.cuda(), (lens.cuda() if len({len(c) for c in clips}) > 1 else None)
    want = torch.from_numpy(ref_batch(_rounded(clips, in_dtype), orig, new))
    got, got_lens = ops.resample(audio, orig, new, lens, out_dtype=out_dtype)
    assert ops.LAST_PATH["resample"] == (_lib.PATH_FUSED if fused else _lib.PATH_GENERIC), what
    assert got.shape == want.shape and got.dtype == out_dtype, what
    composed, composed_lens = ops.resample_torch(audio, orig, new, lens, out_dtype=out_dtype)
    if lens is None:
        assert got_lens is None and composed_lens is None
    else:
        assert got_lens.dtype == torch.int32 and got_lens.tolist() == composed_lens.tolist() == [out_len(orig, new, len(c)) for c in clips], what
    bound = tol(orig, new) + (BF16_REL * want.abs() if out_dtype == torch.bfloat16 else 0.0)
    e_k, e_t = (got.double().cpu() - want).abs(), (composed.double().cpu() - want).abs()
    e_kt = (got.double() - composed.double()).abs().cpu()
    print(f"{what}: kernel-f64 {float(e_k.max()):.3g} torch-f64 {float(e_t.max()):.3g} kernel-torch {float(e_kt.max()):.3g} "
          f"(tol {tol(orig, new):.3g})")
    assert bool((e_k <= bound).all()), (what, float(e_k.max()))
    assert bool((e_t <= bound).all()), (what, float(e_t.max()))
    assert bool((e_kt <= 2 * bound).all()), (what, float(e_kt.max()))
    return got


# ------------------------------------------------------------------ the kernel against both references
@pytest.mark.parametrize("orig,new", SWEEP_PAIRS)
def test_small_sweep(orig, new):
    from mop_amd import ops
    lengths = sweep_lengths(orig, new, ops.RESAMPLE_TILE)
    for L in lengths:
        check([noise(L, seed=L)], orig, new, f"{orig}->{new} L = {L} ({out_len(orig, new, L)} out)")
    check([noise(L, seed=L + 1) for L in lengths], orig, new, f"{orig}->{new} all lengths in one batch")


def test_ragged_batch_over_garbage_rows_alone_and_the_zero_tail():
    from mop_amd import _lib, ops
    clips = ragged_clips(44100, NEW, ops.RESAMPLE_TILE)
    got = check(clips, 44100, NEW, "ragged batch")
    for b, c in enumerate(clips):                                          # each row bit for bit the clip alone
        lo = out_len(44100, NEW, len(c))
        if len(c):
            alone, _ = ops.resample(torch.from_numpy(c).float().cuda()[None], 44100, NEW)
            assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and torch.equal(got[b, :lo], alone[0]), b
        assert float(got[b, lo:].abs().max() if lo < got.shape[1] else 0.0) == 0.0, b
    two = ops.resample(pad_batch(clips[2:0:-1], GARBAGE)[0].cuda(), 44100, NEW,            # another batch around the same clips
                       torch.tensor([len(clips[2]), len(clips[1])], dtype=torch.int32).cuda())[0]
    assert torch.equal(two[0, :out_len(44100, NEW, len(clips[2]))], got[2, :out_len(44100, NEW, len(clips[2]))])
    assert torch.equal(two[1, :1], got[1, :1])
    # the zero tail and out_lens are written by the launch: the library called on buffers of this test's own, filled beforehand
    audio, lens = pad_batch(clips, GARBAGE)
    audio, lens = audio.cuda(), lens.cuda()
    for dtype, code in ((torch.float32, _lib.MOPK_F32), (torch.bfloat16, _lib.MOPK_BF16)):
        out = torch.full(got.shape, 1e30, dtype=dtype, device="cuda")
        out_lens = torch.full((len(clips),), -7, dtype=torch.int32, device="cuda")
        a = ops._rs_accept(audio, 44100, NEW, lens, 6, 0.99, dtype)
        assert a is not None and a.out_dtype == code
        a.out, a.out_lens = out.data_ptr(), out_lens.data_ptr()
        ops._launch("mopk_resample", a)
        torch.cuda.synchronize()
        assert torch.equal(out, got.to(dtype)), dtype                      # bf16: the same fp32 value, rounded once
        assert out_lens.tolist() == [out_len(44100, NEW, len(c)) for c in clips]
        for b, c in enumerate(clips[1:], 1):
            assert float(out[b, out_len(44100, NEW, len(c)):].float().abs().max()) == 0.0, (dtype, b)


def test_many_tiles_per_clip():
    """clips of nine tiles and a bit, of five tiles and a bit and of exactly four, in one batch (the shorter clips' last tiles
    are padding workgroups) and alone"""
    from mop_amd import ops
    T = ops.RESAMPLE_TILE
    for orig in (48000, 44100):
        clips = [noise(len_for(orig, NEW, m), seed=m) for m in (9 * T + 5, 5 * T + 7, 4 * T)]
        assert [out_len(orig, NEW, len(c)) for c in clips] == [9 * T + 5, 5 * T + 7, 4 * T]
        got = check(clips, orig, NEW, f"{orig}: 9, 5 and 4 tiles")
        for b, c in enumerate(clips):
            alone, _ = ops.resample(torch.from_numpy(c).float().cuda()[None], orig, NEW)
            assert torch.equal(alone[0], got[b, :alone.shape[1]]) and not got[b, alone.shape[1]:].any(), (orig, b)


def test_table_too_large_for_lds_is_read_through_l2():
    """1000 -> 1001: 1001 phases of 13 taps and a span of 3014 samples are 68 KB together, past the 64 KiB of a launch, so the
    kernel leaves the table where it is; same numbers, same properties"""
    from mop_amd import ops
    o, n = 1000, 1001
    w, S = ops._rs_dims(o, n, 6, 0.99)
    span = ((ops.RESAMPLE_TILE + n - 2) // n) * o + 2 * w + o
    assert span <= ops.RESAMPLE_MAX_SPAN and 4 * (span + n * (S | 1) + n) > 65536
    clips = [noise(L, seed=90 + L) for L in (2 * ops.RESAMPLE_TILE + 3, 1, ops.RESAMPLE_TILE, 0, 1500)]
    got = check(clips, o, n, "1000 -> 1001, the table in L2")
    alone, _ = ops.resample(torch.from_numpy(clips[4]).float().cuda()[None], o, n)
    assert torch.equal(alone[0], got[4, :alone.shape[1]]) and not got[4, alone.shape[1]:].any()


def test_dtypes_strides_and_channel_layouts():
    from mop_amd import _lib, ops
    L = 3 * 1200 + 7
    clips = [noise(L, seed=40 + b) for b in range(6)]
    full = check(clips, 48000, NEW, "six rows")
    audio = pad_batch(clips, GARBAGE)[0].cuda()
    half, _ = ops.resample(audio[::2], 48000, NEW)                         # audio[::2]: a row stride of 2 L
    assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and torch.equal(half, full[::2])
    assert torch.equal(check(clips, 48000, NEW, "padded row stride", extra=9), full)
    every_other, _ = ops.resample(audio.repeat_interleave(2, dim=1)[:, ::2], 48000, NEW)           # a sample stride of 2
    assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and torch.equal(every_other, full)
    ragged = clips[:2] + [clips[2][:700]]
    check(ragged, 48000, NEW, "bf16 input", in_dtype=torch.bfloat16)
    check(ragged, 48000, NEW, "fp16 input", in_dtype=torch.float16)
    check(ragged, 44100, NEW, "int16 input", in_dtype=torch.int16)
    check(ragged, 44100, NEW, "bf16 output", out_dtype=torch.bfloat16)
    check(ragged, 44100, NEW, "int16 input, bf16 output", in_dtype=torch.int16, out_dtype=torch.bfloat16)
    same, _ = ops.resample(audio, 48000, 48000)                            # the identity goes through the kernel as well
    assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and torch.equal(same, audio)
    for Cn in (2, 3):                                                      # channel-first, and the transposed view of channel-last
        for dtype in (torch.float32, torch.int16):
            a = [noise(L - 100 * b, seed=60 + Cn + b, channels=Cn) for b in range(2)]
            stored = [np.round(x * 32767) if dtype == torch.int16 else x for x in a]
            first = torch.full((2, Cn, L), GARBAGE, dtype=torch.float64)
            for b, x in enumerate(stored):
                first[b, :, :x.shape[1]] = torch.from_numpy(x)
            first = first.to(dtype).cuda()
            last = first.transpose(1, 2).contiguous().transpose(1, 2)
            assert last.stride() == (Cn * L, 1, Cn) and first.stride() == (Cn * L, L, 1)
            lens = torch.tensor([L, L - 100], dtype=torch.int32).cuda()
            got, got_lens = ops.resample(first, 48000, NEW, lens)
            assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and got_lens.tolist() == [out_len(48000, NEW, L), out_len(48000, NEW, L - 100)]
            got_last, _ = ops.resample(last, 48000, NEW, lens)
            assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and torch.equal(got, got_last)
            scale = 1 / 32768 if dtype == torch.int16 else 1.0
            want = ref_batch([ref_mono(first[b, :, :x.shape[1]].double().cpu().numpy() * scale) for b, x in enumerate(a)], 48000, NEW)
            e = float((got.double().cpu() - torch.from_numpy(want)).abs().max())
            print(f"C = {Cn} {dtype}: kernel-f64 {e:.3g} (tol {tol(48000, NEW, Cn):.3g})")
            assert e <= tol(48000, NEW, Cn)
            assert float((got - ops.resample_torch(first, 48000, NEW, lens)[0]).abs().max()) <= 2 * tol(48000, NEW, Cn)
            alone, _ = ops.resample(first[1:, :, :L - 100], 48000, NEW)
            assert torch.equal(alone[0], got[1, :alone.shape[1]])


def test_guard_bands_and_poison_around_every_buffer():
    """as test_gpu_bounds.py does for the other ops: the inputs embedded in NaN / 0xFF, the outputs handed out between guard bands
    and poisoned; the guards stay intact and the results equal the plain run's bit for bit"""
    from mop_amd import _lib, ops
    clips = ragged_clips(44100, NEW, ops.RESAMPLE_TILE)
    mono = pad_batch(clips, float("nan"))
    stereo = torch.from_numpy(np.round(noise(4000, seed=5, channels=6).reshape(3, 2, 4000) * 32767)).to(torch.int16)
    cases = [("mono fp32, 44100", mono[0].cuda(), mono[1].cuda(), 44100, torch.float32),
             ("stereo int16, 48000, bf16 out", stereo.cuda(), torch.tensor([4000, 0, 1234], dtype=torch.int32).cuda(), 48000, torch.bfloat16),
             ("mono fp32 without lens, 96000", torch.from_numpy(noise(6200, seed=6)).float()[None].cuda(), None, 96000, torch.float32)]
    for what, audio, lens, orig, out_dtype in cases:
        plain, plain_lens = ops.resample(audio, orig, NEW, lens, out_dtype=out_dtype)
        torch.cuda.synchronize()
        with guarded_allocations() as ledger:
            g, g_lens = ops.resample(embedded(audio), orig, NEW, None if lens is None else embedded(lens), out_dtype=out_dtype)
            torch.cuda.synchronize()
        assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED, what
        assert ledger.intact(), f"{what}: {ledger.describe_damage()}"
        assert ledger.count(plain.numel() * plain.element_size()) >= 1 and ledger.count() >= (1 if lens is None else 2), what
        assert bool(torch.isfinite(g.float()).all()) and torch.equal(g, plain), what
        assert (g_lens is None and plain_lens is None) if lens is None else torch.equal(g_lens, plain_lens), what


def test_repeatable_and_no_host_sync():
    from mop_amd import _lib, ops
    clips = ragged_clips(44100, NEW, ops.RESAMPLE_TILE)
    audio, lens = pad_batch(clips, GARBAGE)
    audio, lens = audio.cuda(), lens.cuda()
    first, first_lens = ops.resample(audio, 44100, NEW, lens)
    first_t = ops.resample_torch(audio, 44100, NEW, lens)[0]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again, again_lens = ops.resample(audio, 44100, NEW, lens)
        assert ops.resample_supported(audio, 44100, NEW, lens)
        again_t = ops.resample_torch(audio, 44100, NEW, lens)[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED
    assert torch.equal(first, again) and torch.equal(first_lens, again_lens) and torch.equal(first_t, again_t)


def test_graph_replay_reproduces_eager():
    """one captured ops.resample call replayed on new audio and lengths in its static buffers, in a process of its own
    (tools/graph_probe_whisper_resample.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_resample.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "REPLAY_IDENTICAL True" in r.stdout, r.stdout[-800:]


def test_outside_the_envelope_takes_the_torch_path():
    from mop_amd import _lib, ops
    clips = [noise(L, seed=70 + L) for L in (2000, 1, 777)]
    check(clips, 13, 1, "13 -> 1: a span past the envelope", fused=False)
    x = torch.from_numpy(clips[0])[None].cuda()                            # float64 audio computes in float64, in torch
    assert not ops.resample_supported(x, 48000, NEW) and ops.resample_supported(x.float(), 48000, NEW)
    got, _ = ops.resample(x, 48000, NEW, out_dtype=torch.float64)
    assert ops.LAST_PATH["resample"] == _lib.PATH_GENERIC
    assert float((got[0].cpu() - torch.from_numpy(ref_resample(clips[0], 48000, NEW))).abs().max()) <= 1e-12
    many = torch.zeros(1, ops.RESAMPLE_MAX_CHANNELS + 1, 300, device="cuda")
    assert not ops.resample_supported(many, 48000, NEW) and ops.resample_supported(many[:, 1:], 48000, NEW)


# ------------------------------------------------------------------ the frontend
def test_resampled_frontend_feeds_the_model():
    from test_gpu_whisper_transcribe import RULES, V, _model
    from mop_amd import _lib, ops
    from mop_amd.nn import Resample, ResampledLogMelFrontend
    m = _model()
    fe = ResampledLogMelFrontend(48000, 12, NEW, 64, 16).cuda()
    batch = torch.from_numpy(np.stack([noise(48 * 70 + 5, seed=b) for b in range(2)])).float().cuda()
    mel = fe(batch)
    assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED
    assert mel.shape == (2, 70, 12) and torch.equal(mel, ops.log_mel(ops.resample(batch, 48000, NEW)[0], fe.filters, 64, 16))
    clips = [torch.from_numpy(noise(48 * 150 + 5, seed=1)).float().cuda(),                  # mono, stereo and three channels
             torch.from_numpy(np.round(noise(48 * 64 + 5, seed=2, channels=2) * 32767) / 32767).float().cuda(),
             torch.from_numpy(noise(48 * 37 + 5, seed=3, channels=3)).float().cuda()]
    mel = fe(clips)
    assert ops.LAST_PATH["resample"] == _lib.PATH_FUSED and ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED
    assert [tuple(x.shape) for x in mel] == [(150, 12), (64, 12), (37, 12)]
    waves = Resample(48000, NEW)(clips)
    for b, (x, c) in enumerate(zip(mel, clips)):                           # clip by clip as alone, through both stages
        assert torch.equal(x, fe(c[None])[0]), b
        assert torch.equal(waves[b], ops.resample(c[None], 48000, NEW)[0][0]), b
        want = ref_resample(ref_mono(c.double().cpu().numpy()), 48000, NEW)
        assert float((waves[b].double().cpu() - torch.from_numpy(want)).abs().max()) <= tol(48000, NEW, 3), b
    prompt = torch.tensor([7, 8, 9], device="cuda")
    rules = ops.LogitRules(V, **RULES, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = m.transcribe_audio(clips, fe, prompt, rules, 12, window=64)
        same = m.transcribe(fe(clips), prompt, rules, 12, window=64)
    assert len(got) == 3 and sum(t.tokens.numel() for t in got) > 0
    for g, w in zip(got, same):
        assert all(torch.equal(x, y) for x, y in zip(g, w))
