#!/usr/bin/env python3
"""Audio resampler benchmark (GPU box): one JSON line per case, appended to --out (default profiles/whisper_resample_bench.jsonl).

    python tools/bench_whisper_resample.py

Cases: B = 8 clips of 30 s and one clip of ten minutes, each as 48 kHz int16 stereo and as 44.1 kHz fp32 mono, to 16 kHz fp32.
Timed in one process with HIP events after a warm-up, back to back on one stream: ops.resample per call (the HIP kernel: one
launch plus the Python around it), the same call captured in a graph and replayed (the kernel alone), and ops.resample_torch on the
same device tensors (one gather, multiply and add per tap).  byte_bound_ms is (bytes in + bytes out) / 8.0 TB/s, the HBM3E peak
of the MI355X; share_of_byte_bound is byte_bound_ms / graph_ms.  max_abs_diff_vs_torch is the kernel against ops.resample_torch.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

NEW, HBM_TBS = 16000, 8.0


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


def _commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    import torch
    from mop_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_resample_bench.jsonl"))
    ap.add_argument("--commit", default=None, help="the commit the numbers are taken at (default: git rev-parse, None outside a checkout)")
    args = ap.parse_args()
    commit = args.commit or _commit()
    for B, seconds in ((8, 30), (1, 600)):
        for rate, channels, dtype in ((48000, 2, torch.int16), (44100, 1, torch.float32)):
            torch.manual_seed(B + rate)
            L = rate * seconds
            shape = (B, L) if channels == 1 else (B, channels, L)
            audio = (torch.randint(-32768, 32768, shape, device="cuda").to(torch.int16) if dtype == torch.int16
                     else torch.rand(shape, device="cuda") * 2 - 1)
            out, _ = ops.resample(audio, rate, NEW)
            fused = ops.LAST_PATH["resample"] == _lib.PATH_FUSED
            diff = float((out - ops.resample_torch(audio, rate, NEW)[0]).abs().max())
            call_ms = _events(lambda: ops.resample(audio, rate, NEW), args.steps, args.warmup)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static = ops.resample(audio, rate, NEW)[0]
            graph_ms = _events(graph.replay, args.steps, args.warmup)
            same = bool(torch.equal(static, out))
            torch_ms = _events(lambda: ops.resample_torch(audio, rate, NEW), max(args.steps // 10, 2), 1)
            nbytes = audio.numel() * audio.element_size() + out.numel() * out.element_size()
            bound_ms = nbytes / (HBM_TBS * 1e12) * 1e3
            rec = dict(workload="resample", commit=commit, B=B, seconds=seconds, orig_rate=rate, new_rate=NEW, channels=channels,
                       audio_dtype=str(dtype).replace("torch.", ""), samples_in=L, samples_out=out.shape[1], fused=fused,
                       graph_replay_identical=same, call_ms=round(call_ms, 4), graph_ms=round(graph_ms, 4),
                       torch_composition_ms=round(torch_ms, 4), max_abs_diff_vs_torch=diff, mbytes=round(nbytes / 1e6, 2),
                       byte_bound_ms=round(bound_ms, 4), share_of_byte_bound=round(bound_ms / graph_ms, 4),
                       speedup_vs_torch=round(torch_ms / graph_ms, 1), steps=args.steps, warmup=args.warmup)
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            del audio, out, static, graph


if __name__ == "__main__":
    main()
