#!/usr/bin/env python3
"""Log-mel frontend benchmark (GPU box): one JSON line per shape, appended to --out (default profiles/whisper_frontend_bench.jsonl).

    python tools/bench_whisper_frontend.py

At Whisper's defaults (n_fft 400, hop 160, 80 mels, 16 kHz), fp32 noise: B = 8 clips of 480 000 samples (30 s each) and one clip of
9 600 000 samples (ten minutes).  Timed in one process with HIP events after a warm-up, back to back on one stream: ops.log_mel
(the HIP kernels), ops.log_mel_torch in fp32 (the gather-and-matmul composition) and the torch.stft composition a user would
write (stft, |.|^2, filterbank matmul, log10, two clamps, a scale), recorded as absent when torch.stft does not run on the box.
flops counts the DFT as the kernel computes it (frames x n_fft x 2 (n_fft/2 + 1) multiply-adds) plus the dense filterbank product;
share_of_fp32_peak is flops / kernel time / 157.3 TFLOP/s.  max_abs_diff_vs_torch is the kernel against ops.log_mel_torch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N_FFT, HOP, N_MELS, SR, PEAK_TF = 400, 160, 80, 16000, 157.3


def _events(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _stft_composition(audio, filt, window):
    import torch
    spec = torch.stft(audio, N_FFT, HOP, window=window, center=True, pad_mode="reflect", return_complex=True)
    g = (filt @ (spec[..., :-1].abs() ** 2)).clamp(min=1e-10).log10()
    g = torch.maximum(g, g.amax(dim=(1, 2), keepdim=True) - 8.0)
    return ((g + 4.0) / 4.0).transpose(1, 2)


def main():
    import torch
    from mop_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_frontend_bench.jsonl"))
    args = ap.parse_args()
    filt = ops.mel_filterbank(SR, N_FFT, N_MELS, device="cuda")
    window = torch.hann_window(N_FFT, device="cuda")
    for B, L in ((8, 480000), (1, 9600000)):
        torch.manual_seed(B)
        audio = torch.randn(B, L, device="cuda") * 0.1
        T = L // HOP
        out = ops.log_mel(audio, filt)
        fused = ops.LAST_PATH["log_mel"] == _lib.PATH_FUSED
        diff = float((out - ops.log_mel_torch(audio, filt)).abs().max())
        kernel_ms = _events(lambda: ops.log_mel(audio, filt), args.steps, args.warmup)
        torch_ms = _events(lambda: ops.log_mel_torch(audio, filt), max(args.steps // 4, 2), 1)
        try:
            stft_diff = float((out - _stft_composition(audio, filt, window)).abs().max())
            stft_ms = _events(lambda: _stft_composition(audio, filt, window), args.steps, args.warmup)
        except RuntimeError as e:
            stft_ms, stft_diff = None, repr(e)[:200]
        flops = 2.0 * B * T * (N_FFT * 2 * (N_FFT // 2 + 1) + (N_FFT // 2 + 1) * N_MELS)
        rec = dict(workload="log_mel", B=B, samples=L, frames=T, n_fft=N_FFT, hop=HOP, n_mels=N_MELS, fused=fused,
                   kernel_ms=round(kernel_ms, 4), torch_composition_ms=round(torch_ms, 4),
                   stft_composition_ms=None if stft_ms is None else round(stft_ms, 4), stft_composition=stft_diff if stft_ms is None else "ran",
                   max_abs_diff_vs_torch=diff, max_abs_diff_vs_stft=stft_diff if stft_ms is not None else None,
                   gflop=round(flops / 1e9, 3), kernel_tflops=round(flops / kernel_ms / 1e9, 2),
                   share_of_fp32_peak=round(flops / kernel_ms / 1e9 / PEAK_TF, 4), steps=args.steps, warmup=args.warmup)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del audio, out


if __name__ == "__main__":
    main()
