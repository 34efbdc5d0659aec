#!/usr/bin/env python3
"""Token-level timestamps benchmark (GPU box): one JSON line per case, appended to --out (default
profiles/whisper_align_bench.jsonl).

    python tools/bench_whisper_align.py

Shape: the cross-attention maps of a d = 512, H = 8, 6 + 6 layer WhisperMoP at T_a = 1500 frames and 224 tokens with the default
alignment heads (the upper three decoder layers: S = 24 heads), B in {1, 8}, fp32 softmax rows of random logits, medfilt_width 7,
4 prompt rows.  ops.alignment_cost + ops.dtw_align are timed by three routes:
    kernels:  the HIP kernels (mopk_alignment_cost, mopk_dtw_align)
    torch:    ops.alignment_cost_torch + ops.dtw_align_torch on the GPU (the restatements: a launch per anti-diagonal)
    whisper:  Whisper's way: the torch filter on the GPU, the cost copied to the host, the DTW there in numpy, item by item
Each route is timed with a host clock around calls that end in a device synchronise (the whisper route ends on the host), --iters
calls after --warmup, --repeats times, routes interleaved within a repeat; the record holds the median and the min / max over the
repeats (the run-to-run spread), and the two kernels' own times by HIP events.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

S, N, M, WIDTH, ROW0 = 24, 224, 1500, 7, 4


def dtw_numpy(x):
    """Whisper's dtw_cpu (without numba) on one (R, C) float32 array -> the path's (rows, columns)"""
    import numpy as np
    R, Cn = x.shape
    D = np.full((R + 1, Cn + 1), np.inf, dtype=np.float32)
    tr = -np.ones((R + 1, Cn + 1), dtype=np.int8)
    D[0, 0] = 0
    for j in range(1, Cn + 1):
        for i in range(1, R + 1):
            c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            D[i, j] = x[i - 1, j - 1] + c
            tr[i, j] = t
    i, j, path = R, Cn, []
    tr[0, :], tr[:, 0] = 2, 1
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        i, j = (i - 1, j - 1) if tr[i, j] == 0 else (i - 1, j) if tr[i, j] == 1 else (i, j - 1)
    return path[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-dtw", action="store_true", help="also time the whisper route (minutes: a Python loop per cell)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "whisper_align_bench.jsonl"))
    args = ap.parse_args()
    import torch
    from mop_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_whisper_align: needs the GPU")
    for B in (1, 8):
        g = torch.Generator(device="cuda").manual_seed(B)
        probs = torch.softmax(2.0 * torch.randn(B, S, N, M, device="cuda", generator=g), dim=-1)
        nt = torch.full((B,), N, dtype=torch.int32, device="cuda")
        nf = torch.full((B,), M, dtype=torch.int32, device="cuda")

        def kernels():
            return ops.dtw_align(ops.alignment_cost(probs, nt, nf, WIDTH), nt - 1, nf, ROW0)

        def restated():
            return ops.dtw_align_torch(ops.alignment_cost_torch(probs, nt, nf, WIDTH), nt - 1, nf, ROW0)

        def whisper():
            x = ops.alignment_cost_torch(probs, nt, nf, WIDTH).cpu().numpy()
            return [dtw_numpy(x[b, ROW0:N - 1]) for b in range(B)]

        routes = {"kernels": kernels, "torch": restated}
        if args.host_dtw:
            routes["whisper"] = whisper
        s0, e0 = kernels()
        assert ops.LAST_PATH["alignment_cost"] == _lib.PATH_FUSED and ops.LAST_PATH["dtw_align"] == _lib.PATH_FUSED
        s1, e1 = ops.dtw_align_torch(ops.alignment_cost(probs, nt, nf, WIDTH), nt - 1, nf, ROW0)
        assert torch.equal(s0, s1) and torch.equal(e0, e1)               # faster and different is not faster
        times = {k: [] for k in routes}
        for name, fn in routes.items():
            for _ in range(args.warmup if name != "whisper" else 0):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name, fn in routes.items():
                n = args.iters if name != "whisper" else 1
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / n)
        ops.enable_timing(True)
        for _ in range(args.iters):
            kernels()
        torch.cuda.synchronize()
        own = {k: statistics.median(v) for k, v in ops.timing_results().items() if k in ("alignment_cost", "dtw_align")}
        ops.enable_timing(False)
        rec = {"bench": "whisper_align", "B": B, "S": S, "N": N, "M": M, "width": WIDTH, "row0": ROW0, "iters": args.iters,
               "repeats": args.repeats, "kernel_ms": own,
               "probs_gb": probs.numel() * 4 / 1e9}
        for name, v in times.items():
            rec[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        rec["torch_over_kernels"] = rec["torch_ms"]["median"] / rec["kernels_ms"]["median"]
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
