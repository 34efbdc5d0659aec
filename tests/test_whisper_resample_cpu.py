"""CPU checks of the audio resampler (no GPU): a float64 numpy restatement of the windowed-sinc polyphase definition with the
full, uncompacted tap table (the yardstick of this file and of test_gpu_whisper_resample.py, which imports it, the input builders
and the tolerance), ops.resample_torch in float64 and float32 against it, the ragged batch, the compact-support claim the kernel's
table rests on, properties of the restatement alone (tones), the identity rate, int16 scaling, the channel mean in both layouts,
signatures and exports, every ValueError, the support query at the envelope's edges and the bad-argument returns of mopk_resample
(no launch), and Resample / ResampledLogMelFrontend up to WhisperMoP.transcribe_audio on the torch compositions."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _params
from test_whisper_frontend_cpu import TOL_BROADBAND, assert_same_transcripts
from test_whisper_transcribe_cpu import RULES, V, transcribe_model

NEW = 16000
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)       # every rate the envelope must take, -> 16000
SWEEP_PAIRS = ((2, 3), (3, 2), (8000, NEW), (11025, NEW), (44100, NEW), (48000, NEW), (96000, NEW))
BF16_REL = 2.0 ** -8                                         # one rounding to bf16 (2^-9 relative), a factor 2 of margin


# ------------------------------------------------------------------ the restatement
def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def ref_table(orig, new, lpw=6, rolloff=0.99):
    """(o, n, w, K (n, 2 w + o) float64): the full tap table of the definition"""
    o, n = reduced(orig, new)
    base = min(o, n) * rolloff
    w = math.ceil(lpw * o / base)
    p, j = np.arange(n, dtype=np.float64)[:, None], np.arange(2 * w + o, dtype=np.float64)[None]
    t = np.clip((-p / n + (j - w) / o) * base, -lpw, lpw)
    sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / np.where(t == 0, 1.0, np.pi * t))
    return o, n, w, (base / o) * np.cos(t * np.pi / (2 * lpw)) ** 2 * sinc


def taps_per_phase(orig, new, lpw=6, rolloff=0.99):
    o, n = reduced(orig, new)
    return math.floor(2 * lpw * o / (min(o, n) * rolloff)) + 1


def out_len(orig, new, length):
    o, n = reduced(orig, new)
    return -(-n * length // o)


def ref_resample(x, orig, new, lpw=6, rolloff=0.99):
    """one mono clip, float64, in the order of the definition -> (ceil(n len / o),)"""
    x = np.asarray(x, dtype=np.float64)
    if orig == new:
        return x.copy()
    o, n, w, K = ref_table(orig, new, lpw, rolloff)
    lo = out_len(orig, new, len(x))
    frames = -(-lo // n)
    xp = np.concatenate([np.zeros(w), x, np.zeros(max(0, (frames - 1) * o + w + o - len(x)) + 1)])
    fr = np.stack([xp[f * o:f * o + 2 * w + o] for f in range(frames)]) if frames else np.zeros((0, 2 * w + o))
    return (fr @ K.T).reshape(-1)[:lo]                        # y[f n + p] = sum_j K[p, j] x[f o + j - w]


def ref_mono(audio):
    """(L,) or (C, L) float64 samples -> the channel mean"""
    a = np.asarray(audio, dtype=np.float64)
    return a if a.ndim == 1 else a.mean(0)


def ref_batch(clips, orig, new, lpw=6, rolloff=0.99):
    """mono clips of different lengths -> (B, ceil(n max len / o)) float64 with zeros behind each clip's output"""
    full = np.zeros((len(clips), out_len(orig, new, max(len(c) for c in clips))))
    for b, c in enumerate(clips):
        y = ref_resample(c, orig, new, lpw, rolloff)
        full[b, :len(y)] = y
    return full


def tol(orig, new, channels=1, xmax=1.0, lpw=6, rolloff=0.99):
    """the derived fp32 bound against the restatement: an fmaf chain over S taps of a table rounded to fp32, and the channel mean
    of C terms: (S + C + 2) 2^-24 A max|x|, A = max_p sum_j |K[p, j]|"""
    if orig == new:
        return (channels + 2) * 2.0 ** -24 * xmax
    A = float(np.abs(ref_table(orig, new, lpw, rolloff)[3]).sum(1).max())
    return (taps_per_phase(orig, new, lpw, rolloff) + channels + 2) * 2.0 ** -24 * A * xmax


# ------------------------------------------------------------------ inputs
def noise(L, seed, channels=None):
    """uniform samples in [-1, 1): (L,) or (channels, L)"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, L if channels is None else (channels, L))


def len_for(orig, new, m):
    """the shortest clip with at least m output samples (exactly m wherever a length gives m: always when downsampling)"""
    o, n = reduced(orig, new)
    return (m - 1) * o // n + 1


def sweep_lengths(orig, new, tile, lpw=6, rolloff=0.99):
    """clip lengths 1, w - 1 and w + o, and those giving 1, tile - 1, tile, tile + 1 and 2 tile + 3 outputs"""
    o, _, w, _ = ref_table(orig, new, lpw, rolloff)
    return sorted({1, w - 1, w + o} | {len_for(orig, new, m) for m in (1, tile - 1, tile, tile + 1, 2 * tile + 3)})


def pad_batch(clips, fill, dtype=torch.float32, extra=0):
    """(audio (B, L_max [+ extra columns of row stride]) with `fill` behind every clip, lens int32 (B,))"""
    Lm = max(len(c) for c in clips)
    a = torch.full((len(clips), Lm + extra), fill, dtype=torch.float64)
    for b, c in enumerate(clips):
        a[b, :len(c)] = torch.from_numpy(np.asarray(c, dtype=np.float64))
    return a.to(dtype)[:, :Lm], torch.tensor([len(c) for c in clips], dtype=torch.int32)


def ragged_clips(orig, new, tile):
    return [noise(L, seed=100 + L) for L in (len_for(orig, new, 2 * tile + 3), 1, len_for(orig, new, tile + 1) + 1, 0, len_for(orig, new, tile))]


def tone(L, rate, hz=440.0):
    return np.sin(2 * np.pi * hz * np.arange(L) / rate)


# ------------------------------------------------------------------ the torch composition against the restatement
@pytest.mark.parametrize("orig,new", SWEEP_PAIRS)
def test_torch_composition_equals_the_restatement(orig, new):
    from mop_amd import _lib, ops
    lengths = sweep_lengths(orig, new, ops.RESAMPLE_TILE)
    outs = sorted(out_len(orig, new, L) for L in lengths)
    if new < orig:
        assert {1, ops.RESAMPLE_TILE - 1, ops.RESAMPLE_TILE, ops.RESAMPLE_TILE + 1, 2 * ops.RESAMPLE_TILE + 3} <= set(outs)
    bound = tol(orig, new)
    for L in lengths:
        x = noise(L, seed=L)
        want = ref_resample(x, orig, new)
        got, got_lens = ops.resample_torch(torch.from_numpy(x)[None], orig, new, out_dtype=torch.float64)
        assert got_lens is None and got.shape == (1, out_len(orig, new, L)) and got.dtype == torch.float64
        e64 = float(np.abs(got[0].numpy() - want).max())
        got32, _ = ops.resample(torch.from_numpy(x).float()[None], orig, new)                     # the public op on a CPU tensor
        assert ops.LAST_PATH["resample"] == _lib.PATH_GENERIC and got32.dtype == torch.float32
        e32 = float(np.abs(got32[0].double().numpy() - ref_resample(x.astype(np.float32), orig, new)).max())
        print(f"{orig}->{new} L = {L}: float64 {e64:.3g} float32 {e32:.3g} (tol {bound:.3g})")
        assert e64 <= 1e-12, L
        assert e32 <= bound, L
    assert 1.5e-6 <= bound <= 7.5e-6


def test_ragged_batch_over_nan_rows_alone_zero_tails_and_lengths():
    from mop_amd import ops
    for orig, new in ((44100, NEW), (2, 3)):
        clips = ragged_clips(orig, new, ops.RESAMPLE_TILE)
        audio, lens = pad_batch(clips, float("nan"), torch.float64)
        got, got_lens = ops.resample_torch(audio, orig, new, lens, out_dtype=torch.float64)
        assert got_lens.dtype == torch.int32 and got_lens.tolist() == [out_len(orig, new, len(c)) for c in clips] and got_lens[3] == 0
        assert np.abs(got.numpy() - ref_batch(clips, orig, new)).max() <= 1e-12
        got32, lens32 = ops.resample(audio.float(), orig, new, lens)
        assert torch.equal(lens32, got_lens)
        for b, c in enumerate(clips):
            lo = out_len(orig, new, len(c))
            assert float(got32[b, lo:].abs().max() if lo < got32.shape[1] else 0.0) == 0.0, b
            if len(c):
                alone, _ = ops.resample(torch.from_numpy(c).float()[None], orig, new)
                assert torch.equal(got32[b, :lo], alone[0]), b
        over, over_lens = ops.resample_torch(audio.float(), orig, new, lens + 10 ** 6)          # lens are clamped into [0, L]
        assert over_lens.tolist() == [got.shape[1]] * len(clips) and bool(torch.isnan(over[1]).any())


@pytest.mark.parametrize("orig,new", [(r, NEW) for r in RATES] + [(2, 3), (3, 2)])
def test_compact_support_of_the_tap_table(orig, new):
    """a phase's taps with |t| < lpw are one contiguous run of at most S taps, every other tap is below 2e-49 in float64 and a
    zero in float32, and the table ops builds is exactly those runs"""
    from mop_amd import ops
    o, n, w, K = ref_table(orig, new)
    S, base = taps_per_phase(orig, new), min(o, n) * 0.99
    p, j = np.arange(n, dtype=np.float64)[:, None], np.arange(2 * w + o, dtype=np.float64)[None]
    inside = np.abs((-p / n + (j - w) / o) * base) < 6
    K32 = K.astype(np.float32)
    ow, oS, table, first = ops._rs_filter(o, n, 6, 0.99)
    assert (ow, oS) == (w, S) == ops._rs_dims(o, n, 6, 0.99) and table.shape == (n, S) and 13 <= S <= 73
    for ph in range(n):
        idx = np.nonzero(inside[ph])[0]
        assert len(idx) and (np.diff(idx) == 1).all() and len(idx) <= S, ph
        assert np.abs(K[ph][~inside[ph]]).max(initial=0.0) < 2e-49 and not K32[ph][~inside[ph]].any(), ph
        f = int(first[ph])
        assert 0 <= f <= idx[0] and idx[-1] < f + S <= 2 * w + o, ph                               # the run lies inside the row's slice
        assert np.abs(table[ph].numpy() - K[ph, f:f + S]).max() <= 1e-15, ph
    _, _, dev_table, dev_first = ops._rs_tables(o, n, 6, 0.99, "cpu", torch.float32)
    assert dev_table.shape == (n, S | 1) and dev_table.dtype == torch.float32 and dev_first.dtype == torch.int32
    full = np.zeros_like(K32)
    for ph in range(n):
        full[ph, int(dev_first[ph]):int(dev_first[ph]) + S] = dev_table[ph, :S].numpy()
    assert np.array_equal(full, K32) and not dev_table[:, S:].any()                                # the fp32 table, nothing lost
    assert ops._rs_tables(o, n, 6, 0.99, "cpu", torch.float32)[2] is dev_table                     # kept


def test_taps_per_phase_of_the_nine_rates():
    S = {r: taps_per_phase(r, NEW) for r in RATES}
    assert S[44100] == 34 and min(S.values()) == 13 and max(S.values()) == 73
    o, n, w, K = ref_table(44100, NEW)
    assert (o, n, 2 * w + o) == (441, 160, 475)


# ------------------------------------------------------------------ properties of the restatement alone
def test_tones_through_the_restatement():
    for rate, bound in ((48000, 1e-3), (44100, 1e-3), (8000, 1e-3)):
        y = ref_resample(tone(rate // 2, rate), rate, NEW)
        want = tone(len(y), NEW)
        e = float(np.abs(y - want)[200:-200].max())
        print(f"440 Hz at {rate} -> {NEW}: {e:.3g}")
        assert e <= bound, rate
    y = ref_resample(tone(24000, 48000, 12000.0), 48000, NEW)                 # above the new Nyquist: filtered out
    print(f"12 kHz at 48000 -> {NEW}: {float(np.abs(y)[200:-200].max()):.3g}")
    assert float(np.abs(y)[200:-200].max()) <= 1e-2
    # the checks have teeth: a wrong ratio or reversed phases are O(1) off
    wrong = ref_resample(tone(24000, 48000), 48000, 16500)
    assert float(np.abs(wrong[:7800] - tone(7800, NEW))[200:].max()) > 0.5
    o, n, w, K = ref_table(8000, NEW)
    x = np.concatenate([np.zeros(w), tone(4000, 8000), np.zeros(w + o + 1)])
    rev = (np.stack([x[f * o:f * o + 2 * w + o] for f in range(4000)]) @ K[::-1].T).reshape(-1)
    assert float(np.abs(rev - tone(8000, NEW))[200:-200].max()) > 0.05


# ------------------------------------------------------------------ identity, int16, channels
def test_identity_rate_int16_scaling_and_the_channel_mean():
    from mop_amd import ops
    x = torch.from_numpy(noise(777, seed=1)).float()[None]
    for rate in (16000, 1):
        y, yl = ops.resample(x, rate, rate)
        assert yl is None and torch.equal(y, x)
    lens = torch.tensor([500], dtype=torch.int32)
    y, yl = ops.resample(x, 7, 7, lens)
    assert yl.tolist() == [500] and torch.equal(y[:, :500], x[:, :500]) and not y[:, 500:].any()
    i16 = torch.from_numpy(np.random.default_rng(2).integers(-32768, 32768, (2, 3, 900))).to(torch.int16)
    y, _ = ops.resample(i16, 5, 5)
    third = float(np.float32(1) / np.float32(3))                              # the mean: the ascending sum times the fp32 reciprocal of C
    assert torch.equal(y, ((i16[:, 0].float() / 32768 + i16[:, 1].float() / 32768) + i16[:, 2].float() / 32768) * third)
    for Cn in (1, 2, 3):                                                       # channel-first and the transposed channel-last view
        a = noise(1500, seed=10 + Cn, channels=Cn)
        want = ref_resample(ref_mono(a.astype(np.float32)), 48000, NEW)
        first = torch.from_numpy(a).float()[None]
        last = torch.from_numpy(np.ascontiguousarray(a.T)).float()[None].transpose(1, 2)
        assert last.stride(2) == Cn and last.shape == first.shape
        got, _ = ops.resample(first, 48000, NEW)
        assert torch.equal(got, ops.resample(last, 48000, NEW)[0])
        assert float(np.abs(got[0].double().numpy() - want).max()) <= tol(48000, NEW, Cn)
    mono, _ = ops.resample(torch.from_numpy(noise(1500, seed=11, channels=1)).float(), 48000, NEW)   # (1, L): a batch of one
    assert torch.equal(mono, ops.resample(torch.from_numpy(noise(1500, seed=11, channels=1)).float()[None], 48000, NEW)[0])
    y16, _ = ops.resample(i16[:, 0], 48000, NEW)
    want = ref_resample(i16[0, 0].double().numpy() / 32768, 48000, NEW)
    assert float(np.abs(y16[0].double().numpy() - want).max()) <= tol(48000, NEW)
    yb, _ = ops.resample(x, 48000, NEW, out_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, ops.resample(x, 48000, NEW)[0].to(torch.bfloat16))


# ------------------------------------------------------------------ signatures, exports, ValueErrors
def test_signatures_and_exports():
    import mop_amd.nn as mnn
    from mop_amd import _lib, ops
    from mop_amd.nn import LogMelFrontend, Resample, ResampledLogMelFrontend, WhisperMoP
    e, P, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    sig = dict(audio=(e, P), orig_rate=(e, P), new_rate=(e, P), lens=(None, P), lowpass_filter_width=(6, K), rolloff=(0.99, K),
               out_dtype=(torch.float32, K))
    for fn in (ops.resample, ops.resample_torch, ops.resample_supported):
        assert _params(fn) == sig, fn.__name__
    assert _params(Resample.__init__) == dict(orig_rate=(e, P), new_rate=(e, P), lowpass_filter_width=(6, P), rolloff=(0.99, P))
    assert _params(ResampledLogMelFrontend.__init__) == dict(input_sample_rate=(e, P), n_mels=(80, P), sample_rate=(16000, P),
                                                            n_fft=(400, P), hop_length=(160, P), lowpass_filter_width=(6, P),
                                                            rolloff=(0.99, P))
    assert _params(LogMelFrontend.__init__) == dict(n_mels=(80, P), sample_rate=(16000, P), n_fft=(400, P), hop_length=(160, P))
    assert issubclass(ResampledLogMelFrontend, LogMelFrontend) and hasattr(WhisperMoP, "transcribe_audio")
    assert mnn.Resample is Resample and mnn.ResampledLogMelFrontend is ResampledLogMelFrontend
    src = open(os.path.join(ROOT, "mop_amd", "csrc", "resample.hip")).read()
    assert ops.RESAMPLE_TILE == int(re.search(r"constexpr int RS_TILE = (\d+);", src).group(1)) == 1024
    assert ops.RESAMPLE_MAX_SPAN == int(re.search(r"constexpr int RS_MAX_SPAN = (\d+);", src).group(1))
    assert ops.RESAMPLE_MAX_CHANNELS == int(re.search(r"constexpr int RS_MAX_C = (\d+);", src).group(1))
    assert ops._RS_I16 == int(re.search(r"constexpr int RS_I16 = (\d+);", src).group(1)) and ops._RS_I16 not in (
        _lib.MOPK_F32, _lib.MOPK_BF16, _lib.LOG_MEL_F16)
    assert "mopk_resample" in _lib.SYMBOLS and "mopk_resample_supported" in _lib.SYMBOLS
    assert "resampling" not in LogMelFrontend.__doc__.split("Out of scope")[1]


def test_op_value_errors():
    from mop_amd import ops
    audio = torch.zeros(2, 1000)
    lens = torch.tensor([1000, 500], dtype=torch.int32)
    ok = dict(audio=audio, orig_rate=48000, new_rate=16000, lens=lens, lowpass_filter_width=6, rolloff=0.99, out_dtype=torch.float32)
    bad = [("audio", audio.long()), ("audio", audio.to(torch.int32)), ("audio", audio.to(torch.uint8)), ("audio", audio[0]),
           ("audio", audio[:, :0]), ("audio", audio.view(2, 1, 10, 100)), ("audio", [[0.0] * 1000]), ("audio", None),
           ("orig_rate", 0), ("orig_rate", -48000), ("orig_rate", 48000.0), ("orig_rate", True), ("orig_rate", None),
           ("new_rate", 0), ("new_rate", 16000.0), ("new_rate", False), ("new_rate", "16000"),
           ("lens", lens.long()), ("lens", lens[:1]), ("lens", [1000, 500]), ("lens", lens.view(2, 1)), ("lens", lens.to("meta")),
           ("lens", lens.float()),
           ("lowpass_filter_width", 0), ("lowpass_filter_width", 6.0), ("lowpass_filter_width", True), ("lowpass_filter_width", -1),
           ("rolloff", 0.0), ("rolloff", 1.01), ("rolloff", -0.5), ("rolloff", "0.99"), ("rolloff", None), ("rolloff", True),
           ("out_dtype", torch.float16), ("out_dtype", torch.float64), ("out_dtype", None), ("out_dtype", "float32")]
    for fn in (ops.resample, ops.resample_torch, ops.resample_supported):
        fn(**ok)
        fn(**dict(ok, rolloff=1.0, audio=audio.to(torch.int16).view(2, 2, 500), lens=None))
        fn(**dict(ok, audio=audio.double(), out_dtype=torch.float64))
        for k, v in bad:
            with pytest.raises(ValueError):
                fn(**dict(ok, **{k: v}))


# ------------------------------------------------------------------ ABI
BAD_SHAPE, BAD_ARG = -1, -2                                                # MopkStatus
POINTERS = ("audio", "lens", "table", "first", "out", "out_lens")


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _args(orig=44100, new=NEW, B=3, Cn=1, L=5000, **over):
    from mop_amd import _lib, ops
    o, n = reduced(orig, new)
    w, S = ops._rs_dims(o, n, 6, 0.99)
    a = _lib.ResampleArgs()
    a.B, a.C, a.L, a.o, a.n, a.w, a.S, a.table_ld = B, Cn, L, o, n, w, S, S | 1
    a.audio_dtype, a.out_dtype, a.audio_sb, a.audio_sc, a.audio_sl = _lib.MOPK_F32, _lib.MOPK_F32, Cn * L, L, 1
    for f in POINTERS:
        setattr(a, f, 4096)                                                # aligned stand-ins: the queries never dereference them
    for k, v in over.items():
        setattr(a, k, v)
    if "Lout" not in over and a.o > 0:
        a.Lout = -(-a.n * a.L // a.o)                                      # (a value past int32 wraps: the library refuses it)
    return a


def test_support_query_and_bad_arguments_need_no_gpu(lib):
    from mop_amd import _lib, ops
    q = lambda *p, **k: lib.mopk_resample_supported(C.byref(_args(*p, **k)))         # noqa: E731
    assert all(q(r, NEW) == 1 for r in RATES) and q(2, 3) == 1 and q(3, 2) == 1 and q(1, 1) == 1
    assert (q(B=0), q(B=65535), q(B=65536)) == (0, 1, 0)
    assert (q(Cn=0), q(Cn=ops.RESAMPLE_MAX_CHANNELS), q(Cn=ops.RESAMPLE_MAX_CHANNELS + 1)) == (0, 1, 0)
    assert (q(L=0), q(L=1), q(48000, NEW, L=2 ** 31 - 1), q(NEW, 48000, L=2 ** 31 - 1)) == (0, 1, 1, 0)       # ceil(n L / o) < 2^31
    assert q(Lout=5000) == 0                                               # Lout must be ceil(n L / o)
    span = lambda o, n: ((ops.RESAMPLE_TILE + n - 2) // n) * o + 2 * ops._rs_dims(o, n, 6, 0.99)[0] + o     # noqa: E731
    assert span(11, 1) <= ops.RESAMPLE_MAX_SPAN < span(12, 1) and (q(11, 1), q(12, 1)) == (1, 0)              # the span bound
    assert (q(S=0), q(S=36), q(table_ld=33), q(w=-1), q(o=0), q(n=0)) == (0, 0, 0, 0, 0, 0)                   # S <= table_ld = 35
    assert (q(2, 3, S=16, table_ld=17), q(2, 3, S=17, table_ld=17)) == (1, 0)                                 # S <= 2 w + o = 16
    assert (q(n=ops.RESAMPLE_MAX_TABLE // 35), q(n=ops.RESAMPLE_MAX_TABLE // 35 + 1)) == (1, 0)               # the table bound
    for k in (dict(B=0), dict(Cn=65), dict(L=0), dict(Lout=1), dict(S=0), dict(o=0), dict(orig=12, new=1)):
        assert lib.mopk_resample(C.byref(_args(**k)), None) == BAD_SHAPE, k                                   # before any launch
    for field, v in (("audio_dtype", 4), ("audio_dtype", -1), ("out_dtype", 2), ("out_dtype", 3), ("audio", 2), ("out", 2), ("lens", 2),
                     ("table", 2), ("first", 2), ("out_lens", 2)):
        a = _args(**{field: v})
        assert lib.mopk_resample_supported(C.byref(a)) == 0, field
        assert lib.mopk_resample(C.byref(a), None) < 0, field
    for dt in (_lib.MOPK_BF16, _lib.LOG_MEL_F16, ops._RS_I16):                                                # 2-byte samples: 2-byte alignment
        assert q(audio_dtype=dt, audio=4098) == 1
    assert q(out_dtype=_lib.MOPK_BF16, out=4098) == 1 and q(lens=None, out_lens=None) == 1                    # both optional
    for field in ("audio", "table", "first", "out"):
        assert lib.mopk_resample(C.byref(_args(**{field: None})), None) == BAD_ARG, field                     # null pointers: no launch
    assert lib.mopk_resample_supported(None) == 0 and lib.mopk_resample(None, None) == BAD_ARG
    assert not ops.resample_supported(torch.zeros(2, 100), 48000, NEW)                                        # CPU tensors: the torch path


# ------------------------------------------------------------------ the modules
def test_resample_module_forms_and_errors():
    from mop_amd.nn import Resample
    for bad in (dict(orig_rate=0), dict(new_rate=0), dict(orig_rate=48000.0), dict(new_rate=True), dict(lowpass_filter_width=0),
                dict(rolloff=0.0), dict(rolloff=1.5)):
        with pytest.raises(ValueError):
            Resample(**dict(dict(orig_rate=48000, new_rate=NEW), **bad))
    rs = Resample(48000, NEW)
    assert not list(rs.parameters()) and not list(rs.buffers()) and rs.out_samples(1000) == 334
    clips = [torch.from_numpy(noise(700, 1)).float(), torch.from_numpy(noise(1501, 2, channels=2)).float(),
             torch.from_numpy(noise(33, 3, channels=3)).float()]
    for bad in ([], None, torch.zeros(100), [clips[0], torch.zeros(2, 2, 100)], [clips[0], clips[1].double()], [clips[0], clips[1].long()],
                [clips[0], clips[1].to("meta")], [clips[0], None], [clips[0], clips[0][:0]]):
        with pytest.raises(ValueError):
            rs(bad)
    out = rs(clips)
    assert [tuple(o.shape) for o in out] == [(234,), (501,), (11,)]
    base = out[0]._base if out[0]._base is not None else out[0]
    assert all(o._base is base or o is base for o in out)                  # views of one padded buffer
    for o, c in zip(out, clips):                                           # each clip as it would come out alone
        alone = rs(c[None])[0]
        assert torch.equal(o, alone)
        assert float(np.abs(o.double().numpy() - ref_resample(ref_mono(c.double().numpy()), 48000, NEW)).max()) <= tol(48000, NEW, 3)
    same = rs([clips[1], clips[1].flip(1)])                                # one form: the clips stay as they are, (B, C, L)
    assert torch.equal(torch.stack(same), rs(torch.stack([clips[1], clips[1].flip(1)])))
    i16 = [(c * 32767).to(torch.int16) for c in clips[:2]]
    assert all(torch.equal(a, rs(c[None])[0]) for a, c in zip(rs(i16), i16))


def test_resampled_frontend_forms_errors_and_composition():
    from mop_amd import ops
    from mop_amd.nn import ResampledLogMelFrontend
    from mop_amd.nn.whisper_mop import _pad_waveforms
    for bad in (dict(input_sample_rate=0), dict(input_sample_rate=44100.0), dict(n_mels=0), dict(n_fft=401), dict(hop_length=0),
                dict(lowpass_filter_width=0), dict(rolloff=0.0)):
        with pytest.raises(ValueError):
            ResampledLogMelFrontend(**dict(dict(input_sample_rate=48000), **bad))
    fe = ResampledLogMelFrontend(48000, 10, NEW, 64, 16)
    assert fe.frame_seconds == 16 / NEW and fe.filters.shape == (10, 33) and "filters" not in fe.state_dict()
    assert fe.min_samples == 97 and out_len(48000, NEW, 97) == 33 and out_len(48000, NEW, 96) == 32          # in input samples
    assert ResampledLogMelFrontend(8000, 10, NEW, 64, 16).min_samples == 17 and ResampledLogMelFrontend(NEW).min_samples == 201
    clips = [torch.from_numpy(noise(97, 1)).float(), torch.from_numpy(noise(48 * 40 + 5, 2, channels=2)).float(),
             torch.from_numpy(noise(48 * 9, 3)).float()]
    for bad in ([], None, torch.zeros(100), torch.zeros(2, 96), torch.zeros(1, 2, 3, 100), [clips[0], clips[0][:96]],
                [clips[0], clips[2].double()], [clips[0], None]):
        with pytest.raises(ValueError):
            fe(bad)
    out = fe(clips)
    assert [tuple(o.shape) for o in out] == [(2, 10), (40, 10), (9, 10)]
    base = out[0]._base if out[0]._base is not None else out[0]
    assert all(o._base is base or o is base for o in out)
    padded, lens, n = _pad_waveforms(clips, 1, "test")                     # mixed channel counts: averaged clip by clip
    assert padded.shape == (3, 1925) and lens.tolist() == n == [97, 1925, 432]
    wave, wave_lens = ops.resample_torch(padded, 48000, NEW, lens)
    mel = ops.log_mel_torch(wave, fe.filters, 64, 16, wave_lens)
    for b, (o, c) in enumerate(zip(out, clips)):                           # the composition; clip by clip as alone
        assert torch.equal(o, mel[b, :o.shape[0]]) and not mel[b, o.shape[0]:].any()
        alone_wave, _ = ops.resample_torch(c[None], 48000, NEW)
        assert torch.equal(alone_wave[0], wave[b, :alone_wave.shape[1]])
        alone = ops.log_mel_torch(alone_wave, fe.filters, 64, 16)[0]      # two fp32 matmul orders, each within the log-mel bound
        assert float((o - alone).abs().max()) <= 2 * TOL_BROADBAND
    batch = torch.stack([clips[2], clips[2].flip(0)])
    assert torch.equal(fe(batch), ops.log_mel_torch(ops.resample_torch(batch, 48000, NEW)[0], fe.filters, 64, 16))
    stereo = torch.stack([clips[1], clips[1].flip(1)])
    assert torch.equal(fe(stereo), ops.log_mel_torch(ops.resample_torch(stereo, 48000, NEW)[0], fe.filters, 64, 16))


def test_transcribe_audio_takes_the_resampled_frontend(torch_cores, monkeypatch):     # noqa: F811
    from mop_amd import ops
    from mop_amd.nn import ResampledLogMelFrontend
    monkeypatch.setattr(ops, "log_mel", ops.log_mel_torch)
    monkeypatch.setattr(ops, "resample", ops.resample_torch)
    m = transcribe_model()
    fe = ResampledLogMelFrontend(48000, 10, NEW, 64, 16)
    clips = [torch.from_numpy(noise(48 * T + 7, seed=T)).float() for T in (100, 40, 17)]
    prompt = torch.tensor([7, 8, 9])
    rules = ops.LogitRules(V, **RULES)
    mel = fe(clips)
    assert [x.shape[0] for x in mel] == [100, 40, 17]
    got = m.transcribe_audio(clips, fe, prompt, rules, 12)
    assert_same_transcripts(got, m.transcribe(mel, prompt, rules, 12))
    assert got[0].tokens.numel() > 0
    with pytest.raises(ValueError):
        m.transcribe_audio(clips, ResampledLogMelFrontend(48000, 12, NEW, 64, 16), prompt, rules, 12)
