#!/usr/bin/env python3
"""Where TOL_BROADBAND and TOL_PEAKED of tests/test_whisper_frontend_cpu.py come from (GPU box):

    python tools/measure_whisper_frontend_tol.py          # writes profiles/whisper_frontend_tol.json

ops.log_mel_torch in fp32 on the GPU against the float64 restatement, over every input of tests/test_gpu_whisper_frontend.py (built
by that file's own builders, in its order; nothing is asserted here), the largest error per class of input.  Each test
bound is 4 x the figure of its class.  The kernel's own error is recorded beside it and plays no part in the bound."""
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_whisper_frontend as G  # noqa: E402
from test_whisper_frontend_cpu import SHAPES, filters_for, noise, pad_batch, ref_batch  # noqa: E402
from mop_amd import _lib, ops  # noqa: E402

WORST = dict(broadband=(0.0, ""), peaked=(0.0, ""))
KERNEL = dict(broadband=(0.0, ""), peaked=(0.0, ""))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "whisper_frontend_tol.json")


def check(clips, shape, cls, what, in_dtype=torch.float32, out_dtype=torch.float32, extra=0, fused=True):
    n_fft, hop, n_mels = shape
    filt = filters_for(n_fft, n_mels)
    audio, lens = pad_batch(clips, G.GARBAGE, in_dtype, extra)
    audio, lens = audio.cuda(), (lens.cuda() if len({len(c) for c in clips}) > 1 else None)
    want = torch.from_numpy(ref_batch(G._rounded(clips, in_dtype), n_fft, hop, filt.double().numpy()))
    composed = ops.log_mel_torch(audio, filt.cuda(), n_fft, hop, lens, torch.float32)
    e_t = float((composed.double().cpu() - want).abs().max())
    if e_t > WORST[cls][0]:
        WORST[cls] = (e_t, what)
    line = f"{what} [{cls}]: torch-f64 {e_t:.4g}"
    got = ops.log_mel(audio, filt.cuda(), n_fft, hop, lens, torch.float32)
    e_k = float((got.double().cpu() - want).abs().max())
    if e_k > KERNEL[cls][0]:
        KERNEL[cls] = (e_k, what)
    print(line + f" kernel-f64 {e_k:.4g} ({'HIP' if ops.LAST_PATH['log_mel'] == _lib.PATH_FUSED else 'torch'} path)", flush=True)
    return got.to(out_dtype)


F = ops.LOG_MEL_TILE_FRAMES
for shape in SHAPES:
    n_fft, hop, _ = shape
    lengths = G.sweep_lengths(n_fft, hop, F)
    for L in lengths:
        check([noise(L, seed=L)], shape, "broadband", f"{shape} L = {L}")
    check([noise(L, seed=L + 1) for L in lengths], shape, "broadband", f"{shape} batch")
check(G.ragged_clips(), G.DEF, "broadband", "ragged batch")
for rev in (False, True):
    x = G.clamp_clip(F)
    check([x[::-1].copy() if rev else x], G.DEF, "peaked", f"quiet + loud, reversed = {rev}")
for name, x in G.edge_clips().items():
    check([x], G.DEF, "peaked", name)
clips = [noise(160 * 35 + 9, seed=40 + b) for b in range(6)]
check(clips, G.DEF, "broadband", "six rows")
check(clips, G.DEF, "broadband", "padded row stride", extra=9)
check(clips[:2], G.DEF, "broadband", "bf16 input", in_dtype=torch.bfloat16)
check(clips[:2], G.DEF, "broadband", "fp16 input", in_dtype=torch.float16)
check(clips[:2] + [clips[2][:700]], G.DEF, "broadband", "bf16 output case (measured in fp32)")
check([noise(1024 * 3 + 5, seed=50)], (1024, 256, 20), "broadband", "n_fft = 1024", fused=False)
check([noise(16 * T + 5, seed=T) for T in (150, 64, 37)], (64, 16, 12), "broadband", "frontend clips (64, 16, 12)")

rec = dict(device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, torch=torch.__version__,
           composition_fp32_vs_f64={c: dict(max_abs_err=v, worst_input=w, bound_4x=4 * v) for c, (v, w) in WORST.items()},
           kernel_vs_f64={c: dict(max_abs_err=v, worst_input=w) for c, (v, w) in KERNEL.items()})
print(json.dumps(rec), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(json.dumps(rec, indent=1) + "\n")
