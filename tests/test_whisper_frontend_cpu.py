"""CPU checks of the log-mel audio frontend (no GPU): a float64 numpy restatement of Whisper's log_mel_spectrogram (the yardstick
of this file and of test_gpu_whisper_frontend.py, which imports it, the input builders and the tolerance constants),
ops.log_mel_torch in float64 against it (and torch.stft where it runs), ops.mel_filterbank, every ValueError of ops.log_mel and
LogMelFrontend, the support query at the envelope's edges and the bad-argument returns of mopk_log_mel
(no launch), and WhisperMoP.transcribe_audio with every core routed through its torch composition."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

from test_whisper_audio_lens_cpu import torch_cores  # noqa: F401  (a fixture: every core on its torch composition, lengths included)
from test_whisper_beam_cpu import _params
from test_whisper_transcribe_cpu import EOS, RULES, V, transcribe_model

SHAPES = ((16, 4, 3), (64, 16, 10), (400, 160, 80))          # (n_fft, hop, n_mels) of the small sweep
SR = 16000

# fp32 bounds against the float64 restatement, per class of input.  Each is 4 x the largest |ops.log_mel_torch in fp32 -
# restatement| over this suite's own inputs of the class (every input of test_gpu_whisper_frontend.py; the kernel's own figures
# play no part): an MFMA chain and a BLAS tree order the n_fft terms differently, and fp32 sums of this length differ by a small
# factor between orders; a wrong twiddle, window or reflection shows at 1e-2 or worse.
# Measured on an MI355X (gfx950, torch 2.10.0+rocm7.0) by tools/measure_whisper_frontend_tol.py; its run is
# profiles/whisper_frontend_tol.json:
#   broadband (seeded noise):                           9.58e-7 (six rows of 5609 samples at (400, 160, 80)) -> 3.83e-6
#   peaked (tones, DC, quiet + loud: bins near the floor, where the DFT's absolute rounding is a large relative error before the
#   log):                                               2.238e-4 (full-scale 440 Hz tone + 1e-3 noise) -> 8.95e-4
# (the kernel in the same run: 5.52e-7 and 1.48e-4)
TOL_BROADBAND = 3.83e-6
TOL_PEAKED = 8.95e-4
BF16_REL = 2.0 ** -8                                         # one rounding to bf16 (2^-9 relative), a factor 2 of margin


# ------------------------------------------------------------------ the restatement
def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000, 15 + np.log(np.maximum(f, 1e-9) / 1000) / (np.log(6.4) / 27), f / (200 / 3))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15, 1000 * np.exp((np.log(6.4) / 27) * (m - 15)), m * 200 / 3)


def mel_points(sr, n_mels):
    return mel_to_hz(np.linspace(hz_to_mel(0), hz_to_mel(sr / 2), n_mels + 2))


def ref_filterbank(sr, n_fft, n_mels):
    """the Slaney-scale, area-normalised triangles in float64 -> (n_mels, n_fft/2 + 1)"""
    freqs, pts = np.linspace(0, sr / 2, n_fft // 2 + 1), mel_points(sr, n_mels)
    d, r = np.diff(pts), pts[:, None] - freqs[None]
    w = np.maximum(0, np.minimum(-r[:-2] / d[:-1, None], r[2:] / d[1:, None]))
    return w * (2 / (pts[2:] - pts[:-2]))[:, None]


def ref_log_mel(x, n_fft, hop, filt):
    """one clip, float64, in the order of the definition -> (len(x) // hop, n_mels)"""
    x, filt, p = np.asarray(x, dtype=np.float64), np.asarray(filt, dtype=np.float64), n_fft // 2
    T = len(x) // hop
    xp = np.pad(x, (p, p), mode="reflect")
    n = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
    fr = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)]) * win
    ang = 2 * np.pi * np.outer(n, np.arange(p + 1)) / n_fft
    re, im = fr @ np.cos(ang), fr @ np.sin(ang)
    g = np.log10(np.maximum((re * re + im * im) @ filt.T, 1e-10))
    return (np.maximum(g, g.max() - 8) + 4) / 4


def ref_batch(clips, n_fft, hop, filt):
    """clips of different lengths -> (B, max T, n_mels) float64 with zeros behind each clip's frames"""
    outs = [ref_log_mel(c, n_fft, hop, filt) for c in clips]
    full = np.zeros((len(clips), max(len(c) for c in clips) // hop, filt.shape[0]))
    for b, o in enumerate(outs):
        full[b, :o.shape[0]] = o
    return full


# ------------------------------------------------------------------ inputs
def filters_for(n_fft, n_mels):
    from mop_amd import ops
    return ops.mel_filterbank(SR, n_fft, n_mels)


def min_len(n_fft, hop):
    return max(hop, n_fft // 2 + 1)


def noise(L, seed, scale=0.1):
    return np.random.default_rng(seed).standard_normal(L) * scale


def tone(L, hz=440.0, amp=1.0):
    return amp * np.sin(2 * np.pi * hz * np.arange(L) / SR)


def sweep_lengths(n_fft, hop, tile):
    """clip lengths, no multiple of hop (hop > 1), with T = 1, tile - 1, tile, tile + 1, 2 tile + 3 frames; a T whose clips
    would all be shorter than the minimum legal length n_fft/2 + 1 (T = 1 at hop <= n_fft/4) becomes the smallest legal T"""
    out = []
    for T in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        L = T * hop + hop // 2
        if L < min_len(n_fft, hop):
            L = min_len(n_fft, hop) + (1 if min_len(n_fft, hop) % hop == 0 and hop > 1 else 0)
        if L not in out:
            out.append(L)
    return out


def pad_batch(clips, fill, dtype=torch.float32, extra=0):
    """(audio (B, L_max [+ extra columns of row stride]) with `fill` behind every clip, lens int32 (B,))"""
    Lm = max(len(c) for c in clips)
    a = torch.full((len(clips), Lm + extra), fill, dtype=torch.float64)
    for b, c in enumerate(clips):
        a[b, :len(c)] = torch.from_numpy(np.asarray(c, dtype=np.float64))
    return a.to(dtype)[:, :Lm], torch.tensor([len(c) for c in clips], dtype=torch.int32)


# ------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("n_fft,hop,n_mels", SHAPES)
def test_torch_composition_in_float64_equals_the_restatement(n_fft, hop, n_mels):
    from mop_amd import _lib, ops
    filt = torch.from_numpy(ref_filterbank(SR, n_fft, n_mels))
    for L in sweep_lengths(n_fft, hop, ops.LOG_MEL_TILE_FRAMES):
        x = noise(L, seed=L)
        got = ops.log_mel_torch(torch.from_numpy(x)[None], filt, n_fft, hop, out_dtype=torch.float64)
        assert got.shape == (1, L // hop, n_mels) and got.dtype == torch.float64
        assert np.abs(got[0].numpy() - ref_log_mel(x, n_fft, hop, filt.numpy())).max() <= 1e-10, L
    # a ragged batch over garbage, the float32 path and the public op on CPU tensors
    clips = [noise(L, seed=7 + L) for L in (min_len(n_fft, hop), 5 * hop + 1, 40 * hop + hop // 2)]
    audio, lens = pad_batch(clips, 1e6, torch.float64)
    want = ref_batch(clips, n_fft, hop, filt.numpy())
    got = ops.log_mel_torch(audio, filt, n_fft, hop, lens, torch.float64)
    assert np.abs(got.numpy() - want).max() <= 1e-10
    assert all(float(got[b, len(c) // hop:].abs().max()) == 0.0 for b, c in enumerate(clips[:2]))
    got32 = ops.log_mel(audio.float(), filt.float(), n_fft, hop, lens)
    assert ops.LAST_PATH["log_mel"] == _lib.PATH_GENERIC and got32.dtype == torch.float32
    assert not ops.log_mel_supported(audio.float(), filt.float(), n_fft, hop, lens)          # CPU tensors take the torch path
    assert np.abs(got32.double().numpy() - want).max() <= TOL_BROADBAND                      # the class bound
    assert ops.log_mel(audio.float(), filt.float(), n_fft, hop, lens, torch.bfloat16).dtype == torch.bfloat16


def test_torch_stft_agrees_where_it_runs():
    filt = ref_filterbank(SR, 400, 80)
    x = noise(16000 + 37, seed=3)
    try:
        spec = torch.stft(torch.from_numpy(x), 400, 160, window=torch.hann_window(400, dtype=torch.float64), center=True,
                          pad_mode="reflect", return_complex=True)
    except RuntimeError as e:                                              # a torch built without an FFT library says so
        if "fft" not in str(e).lower():
            raise
        pytest.skip("torch.stft does not run here: " + repr(e)[:200])
    m = torch.from_numpy(filt) @ (spec[:, :-1].abs() ** 2)
    g = m.clamp(min=1e-10).log10()
    g = (torch.maximum(g, g.max() - 8) + 4) / 4
    assert np.abs(g.T.numpy()[:len(x) // 160] - ref_log_mel(x, 400, 160, filt)).max() <= 1e-10


def test_edge_values_of_the_definition():
    from mop_amd import ops
    filt = filters_for(400, 80)
    out = ops.log_mel_torch(torch.zeros(2, 1000), filt)
    assert out.shape == (2, 6, 80) and bool((out == -1.5).all())           # silence: log10(1e-10) = -10 everywhere
    assert bool((torch.from_numpy(ref_log_mel(np.zeros(1000), 400, 160, filt.numpy())) == -1.5).all())


def test_band_table_and_its_cache():
    from mop_amd import ops
    filt = filters_for(400, 80)
    bands = ops._lm_bands(filt)
    assert bands.dtype == torch.int32 and bands.shape == (80, 2)
    for m, (lo, hi) in enumerate(bands.tolist()):                          # the non-zero span of every row
        nz = torch.nonzero(filt[m])[:, 0]
        assert (lo, hi) == (int(nz[0]), int(nz[-1]) + 1), m
    assert ops._lm_bands(filt) is bands                                    # the same unchanged tensor: kept
    filt[3] = 0                                                            # changed in place: derived again, an empty row is (0, 0)
    again = ops._lm_bands(filt)
    assert again is not bands and again[3].tolist() == [0, 0]
    with torch.inference_mode():                                           # no version counter: derived on every call, no error
        inf = filters_for(64, 10)
        a, b = ops._lm_bands(inf), ops._lm_bands(inf)
    assert a is not b and torch.equal(a, b)


# ------------------------------------------------------------------ the filterbank
@pytest.mark.parametrize("sr,n_fft,n_mels", [(16000, 400, 80), (16000, 400, 128), (16000, 64, 10), (22050, 512, 40), (8000, 16, 3)])
def test_mel_filterbank(sr, n_fft, n_mels):
    from mop_amd import ops
    f = ops.mel_filterbank(sr, n_fft, n_mels)
    assert f.shape == (n_mels, n_fft // 2 + 1) and f.dtype == torch.float32 and f.device.type == "cpu"
    assert bool((f >= 0).all())
    want = ref_filterbank(sr, n_fft, n_mels)
    assert np.abs(f.double().numpy() - want).max() <= 2.0 ** -23 * want.max()              # the float64 formula, rounded once
    pts, freqs = mel_points(sr, n_mels), np.linspace(0, sr / 2, n_fft // 2 + 1)
    for m in range(n_mels):
        row = f[m].double().numpy()
        nz = np.nonzero(row)[0]
        inside = np.nonzero((freqs > pts[m]) & (freqs < pts[m + 2]))[0]
        assert nz.tolist() == inside.tolist(), m                           # exactly the bins strictly inside (f_m, f_{m+2})
        if len(nz):                                                        # a single triangle: up to the bin nearest f_{m+1}, then down
            assert (np.diff(nz) == 1).all()
            k = int(row.argmax())
            assert (np.diff(row[nz[0]:k + 1]) > 0).all() and (np.diff(row[k:nz[-1] + 1]) < 0).all(), m
            peak = 2 / (pts[m + 2] - pts[m])                               # the triangle's height at f_{m+1}
            assert row.max() <= peak * (1 + 1e-6)
            lo, up = (freqs[nz] - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - freqs[nz]) / (pts[m + 2] - pts[m + 1])
            assert np.abs(row[nz] - peak * np.minimum(lo, up)).max() <= 1e-6 * peak, m
        for o in range(n_mels):                                            # rows overlap only their neighbours
            if abs(o - m) > 1:
                assert float((f[m] * f[o]).sum()) == 0.0, (m, o)
    if (sr, n_fft, n_mels) == (16000, 400, 80):
        assert bool((f.sum(1) > 0).all())                                  # Whisper's own bank has no empty row
    for bad in ((0, 400, 80), (16000, 401, 80), (16000, 400, 0), (16000.0, 400, 80), (16000, True, 80)):
        with pytest.raises(ValueError):
            ops.mel_filterbank(*bad)


# ------------------------------------------------------------------ signatures and ValueErrors
def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import LogMelFrontend, WhisperMoP
    e, P, VK = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.VAR_KEYWORD
    sig = dict(audio=(e, P), filters=(e, P), n_fft=(400, P), hop_length=(160, P), lens=(None, P), out_dtype=(torch.float32, P))
    for fn in (ops.log_mel, ops.log_mel_torch, ops.log_mel_supported):
        assert _params(fn) == sig, fn.__name__
    assert _params(ops.mel_filterbank) == dict(sample_rate=(e, P), n_fft=(e, P), n_mels=(e, P), device=(None, P))
    assert _params(LogMelFrontend.__init__) == dict(n_mels=(80, P), sample_rate=(16000, P), n_fft=(400, P), hop_length=(160, P))
    assert _params(WhisperMoP.transcribe_audio) == dict(audio=(e, P), frontend=(e, P), prompt_ids=(e, P), logit_rules=(e, P),
                                                        max_new_tokens=(e, P), transcribe_kwargs=(e, VK))
    assert ops.LOG_MEL_TILE_FRAMES == 32


def test_op_value_errors():
    from mop_amd import ops
    audio, filt = torch.zeros(2, 1000), filters_for(400, 80)
    lens = torch.tensor([1000, 500], dtype=torch.int32)
    ok = (audio, filt, 400, 160, lens, torch.float32)
    bad = [(0, audio.long()), (0, audio[0]), (0, audio[:, :0]), (0, audio.view(2, 10, 100)), (0, [[0.0] * 1000]), (0, audio.to("meta")),
           (0, audio[:, :200]), (0, audio[:, :159]),                       # shorter than n_fft/2 + 1, shorter than hop
           (1, filt[:, :200]), (1, filt[0]), (1, filt.half()), (1, filt[:0]), (1, filt.to("meta")), (1, None),
           (2, 401), (2, 0), (2, 400.0), (2, True), (2, 402),              # 402: the filters no longer fit
           (3, 0), (3, 401), (3, 160.0), (3, True),
           (4, lens.long()), (4, lens[:1]), (4, [1000, 500]), (4, lens.view(2, 1)), (4, lens.to("meta")), (4, lens.float()),
           (5, torch.float16), (5, torch.float64), (5, None), (5, "float32")]
    for fn in (ops.log_mel, ops.log_mel_torch, ops.log_mel_supported):
        fn(*ok)
        for i, v in bad:
            args = list(ok)
            args[i] = v
            with pytest.raises(ValueError):
                fn(*args)


def test_frontend_value_errors_and_forms():
    from mop_amd.nn import LogMelFrontend
    for bad in (dict(n_mels=0), dict(sample_rate=0), dict(n_fft=401), dict(n_fft=0), dict(hop_length=0), dict(hop_length=401),
                dict(n_mels=80.0), dict(hop_length=True)):
        with pytest.raises(ValueError):
            LogMelFrontend(**bad)
    fe = LogMelFrontend(10, SR, 64, 16)
    assert fe.frame_seconds == 16 / SR and fe.filters.shape == (10, 33) and "filters" not in fe.state_dict()
    clips = [torch.from_numpy(noise(L, L)).float() for L in (33, 16 * 40 + 3, 16 * 9)]
    for bad in ([], None, torch.zeros(100), torch.zeros(1, 2, 100), [clips[0], torch.zeros(2, 100)], [clips[0], clips[1].double()],
                [clips[0], clips[1].long()], [clips[0], clips[1].to("meta")], [clips[0], clips[1][:32]], [clips[0], None],
                torch.zeros(2, 32)):
        with pytest.raises(ValueError):
            fe(bad)
    out = fe(clips)
    assert [tuple(o.shape) for o in out] == [(2, 10), (40, 10), (9, 10)]
    base = out[0]._base if out[0]._base is not None else out[0]
    assert all(o._base is base or o is base for o in out)                  # views of one padded buffer
    for o, c in zip(out, clips):                                           # each clip as it would come out alone
        assert np.abs(o.double().numpy() - ref_log_mel(c.double().numpy(), 64, 16, fe.filters.double().numpy())).max() <= TOL_BROADBAND
    same = fe([clips[1], clips[1]])                                        # equal lengths: no lens
    assert torch.equal(same[0], same[1]) and torch.equal(torch.stack(same), fe(torch.stack([clips[1], clips[1]])))


# ------------------------------------------------------------------ ABI
FIELDS = ["B", "L", "n_fft", "hop", "n_mels", "audio_dtype", "out_dtype", "reserved", "audio", "audio_ld", "lens", "filters", "bands",
          "twiddle", "window", "out", "workspace"]
BAD_SHAPE, BAD_ARG = -1, -2                                                # MopkStatus


@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


def _args(n_fft=400, hop=160, n_mels=80, B=3, L=4000):
    from mop_amd import _lib
    assert FIELDS == [f for f, _ in _lib.LogMelArgs._fields_]
    a = _lib.LogMelArgs()
    a.B, a.L, a.n_fft, a.hop, a.n_mels, a.audio_ld = B, L, n_fft, hop, n_mels, L
    a.audio_dtype, a.out_dtype = _lib.MOPK_F32, _lib.MOPK_F32
    for f in FIELDS[8:]:
        if f != "audio_ld":
            setattr(a, f, 4096)                                            # aligned stand-ins: the queries never dereference them
    return a


def test_support_query_and_bad_arguments_need_no_gpu(lib):
    from mop_amd import _lib
    q = lambda **k: lib.mopk_log_mel_supported(C.byref(_args(**k)))       # noqa: E731
    assert q() == 1
    assert (q(n_fft=14, hop=4), q(n_fft=16, hop=4), q(n_fft=512), q(n_fft=514)) == (0, 1, 1, 0)
    assert q(n_fft=401) == 0 and q(n_fft=17, hop=4) == 0                   # odd
    assert (q(hop=0), q(hop=400), q(hop=401)) == (0, 1, 0)
    assert (q(n_mels=128), q(n_mels=129), q(n_mels=0)) == (1, 0, 0)
    assert (q(L=201), q(L=200), q(hop=300, L=299), q(hop=300, L=300)) == (1, 0, 0, 1)      # max(hop, n_fft/2 + 1)
    assert (q(B=0), q(B=65535), q(B=65536)) == (0, 1, 0)
    for k in (dict(n_fft=14, hop=4), dict(n_fft=514), dict(n_fft=401), dict(hop=0), dict(hop=401), dict(n_mels=129), dict(L=200), dict(B=0)):
        assert lib.mopk_log_mel(C.byref(_args(**k)), None) == BAD_SHAPE, k                 # bad shapes, before any launch
    for field, v in (("audio_dtype", 3), ("out_dtype", _lib.LOG_MEL_F16), ("audio_ld", 3999), ("audio", 2), ("out", 2), ("lens", 2),
                     ("filters", 2), ("bands", 2), ("twiddle", 4), ("window", 2), ("workspace", 2)):
        a = _args()
        setattr(a, field, v)
        assert lib.mopk_log_mel_supported(C.byref(a)) == 0, field
        assert lib.mopk_log_mel(C.byref(a), None) < 0, field
    a = _args()
    a.audio_dtype, a.audio = _lib.MOPK_BF16, 4098                          # 2-byte samples: 2-byte alignment
    assert lib.mopk_log_mel_supported(C.byref(a)) == 1
    a.lens = a.bands = None                                                # both optional
    assert lib.mopk_log_mel_supported(C.byref(a)) == 1
    for field in ("audio", "filters", "twiddle", "window", "out", "workspace"):
        a = _args()
        setattr(a, field, None)
        assert lib.mopk_log_mel(C.byref(a), None) == BAD_ARG, field       # null pointers: refused before any launch
    assert lib.mopk_log_mel_supported(None) == 0 and lib.mopk_log_mel(None, None) == BAD_ARG
    # the workspace: one word per (clip, tile of 32 frames), and an fp32 copy of the output for a bf16 output
    a = _args(B=3, L=160 * 65)
    assert lib.mopk_log_mel_workspace_bytes(C.byref(a)) == 256
    a.out_dtype = _lib.MOPK_BF16
    assert lib.mopk_log_mel_workspace_bytes(C.byref(a)) == 256 + math.ceil(3 * 65 * 80 * 4 / 256) * 256
    assert lib.mopk_log_mel_workspace_bytes(None) == 0


# ------------------------------------------------------------------ the model
def assert_same_transcripts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w)
        for x, y in zip(g, w):
            assert x.dtype == y.dtype and torch.equal(x, y)


def test_transcribe_audio_equals_transcribe_of_the_frontend_output(torch_cores, monkeypatch):     # noqa: F811
    from mop_amd import ops
    from mop_amd.nn import LogMelFrontend
    monkeypatch.setattr(ops, "log_mel", ops.log_mel_torch)
    m = transcribe_model()
    fe = LogMelFrontend(10, SR, 64, 16)
    clips = [torch.from_numpy(noise(16 * T + 5, seed=T)).float() for T in (100, 40, 17)]
    prompt = torch.tensor([7, 8, 9])
    rules = ops.LogitRules(V, **RULES)
    want = m.transcribe(fe(clips), prompt, rules, 12)
    got = m.transcribe_audio(clips, fe, prompt, rules, 12)
    assert_same_transcripts(got, want)
    assert [int(t.offsets[-1]) for t in got] == [t.tokens.numel() for t in got] and got[0].tokens.numel() > 0
    batch = torch.stack([clips[1], clips[1].flip(0)])                      # the tensor form, keyword arguments passed on
    assert_same_transcripts(m.transcribe_audio(batch, fe, prompt, rules, 9, window=24, num_beams=2),
                            m.transcribe(fe(batch), prompt, rules, 9, window=24, num_beams=2))
    assert rules.eos_token_id == EOS
    for bad in (LogMelFrontend(12, SR, 64, 16), None, fe.filters):
        with pytest.raises(ValueError):
            m.transcribe_audio(clips, bad, prompt, rules, 12)
