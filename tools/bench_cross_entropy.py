#!/usr/bin/env python3
"""Cross-entropy benchmark (GPU box): JSON lines, appended to profiles/cross_entropy_bench.jsonl with --record.

    python tools/bench_cross_entropy.py --workload op       # ops.cross_entropy against F.cross_entropy(logits.float()), fwd and fwd+bwd
    python tools/bench_cross_entropy.py --workload head     # ops.linear_cross_entropy against lm_head + F.cross_entropy: time and peak memory
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_cross_entropy.py --workload op-trace --shape 0 --dtype bf16
    python tools/bench_cross_entropy.py --stats DIR/<host>/<pid>_kernel_stats.csv --shape 0 --dtype bf16   # the kernels against their byte bound
    python tools/bench_cross_entropy.py --workload step --model quartet_lm --loss fused    # one training step; pair it with --loss torch

Shapes: 0 = (R 8192, V 50304), the GPT benchmark's logits; 1 = (R 3584, V 51865), Whisper's.  Times come from HIP events around
--steps iterations after --warmup ones.  The byte bound is R V itemsize / 6.3 TB/s (the measured HBM copy rate) for the forward,
which reads the logits once, and twice that for the backward, which reads them and writes the gradient.  `step` runs ONE model with
ONE loss per process: alternate the two losses in fresh processes and compare the spread of the pairs before a difference.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = [(8192, 50304), (3584, 51865)]
D = 768
HBM_BYTES_PER_S = 6.3e12
CHUNKS = (512, 1024, 2048, 4096, None)
RECORD = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(line + "\n")


def _time(fn, steps, warmup):
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


def _dtypes(args):
    import torch
    return [(n, d) for n, d in (("bf16", torch.bfloat16), ("fp32", torch.float32)) if args.dtype in (None, n)]


def _shapes(args):
    return SHAPES if args.shape is None else [SHAPES[args.shape]]


def _logits(R, V, dt):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(R, V, device="cuda", generator=g).to(dt).requires_grad_()
    return x, torch.randint(0, V, (R,), device="cuda", generator=g)


def bench_op(args):
    import torch
    import torch.nn.functional as F
    from mop_amd import _lib, ops
    for R, V in _shapes(args):
        for name, dt in _dtypes(args):
            x, t = _logits(R, V, dt)

            def fwd_bwd(loss_fn):
                x.grad = None
                loss_fn().backward()
            fused, ref = (lambda: ops.cross_entropy(x, t)), (lambda: F.cross_entropy(x.float(), t))
            with torch.no_grad():
                f_fwd, t_fwd = _time(fused, args.steps, args.warmup), _time(ref, args.steps, args.warmup)
            f_all, t_all = _time(lambda: fwd_bwd(fused), args.steps, args.warmup), _time(lambda: fwd_bwd(ref), args.steps, args.warmup)
            assert ops.LAST_PATH["cross_entropy_fwd"] == ops.LAST_PATH["cross_entropy_bwd"] == _lib.PATH_FUSED
            bound = R * V * x.element_size() / HBM_BYTES_PER_S * 1e3
            emit({"workload": "cross_entropy_op", "R": R, "V": V, "dtype": name, "fused_fwd_ms": f_fwd, "torch_fwd_ms": t_fwd,
                  "fused_fwd_bwd_ms": f_all, "torch_fwd_bwd_ms": t_all, "hbm_bound_fwd_ms": bound, "hbm_bound_fwd_bwd_ms": 3 * bound,
                  "steps": args.steps, "warmup": args.warmup,
                  "what": "mean loss of (R, V) logits; torch = F.cross_entropy(logits.float(), targets); event times, whole op"})
            del x
            torch.cuda.empty_cache()


def op_trace(args):
    """the fused op only, forward and backward (under rocprofv3 --kernel-trace)"""
    import torch
    from mop_amd import ops
    (R, V), (_, dt) = _shapes(args)[0], _dtypes(args)[0]
    x, t = _logits(R, V, dt)
    for _ in range(args.warmup + args.steps):
        x.grad = None
        ops.cross_entropy(x, t).backward()
    torch.cuda.synchronize()


def stats(args):
    """rocprofv3 kernel_stats.csv of an op-trace run -> the kernels' mean time against bytes / 6.3 TB/s"""
    (R, V), name = _shapes(args)[0], args.dtype or "bf16"
    nbytes = R * V * (2 if name == "bf16" else 4)
    rows = list(csv.DictReader(open(args.stats)))
    for key, b in (("ce_fwd_kernel", nbytes), ("ce_bwd_kernel", 2 * nbytes), ("ce_reduce_kernel", 12 * R)):
        hit = [r for r in rows if key in r["Name"]]
        if not hit:
            continue
        mean_us, bound_us = float(hit[0]["AverageNs"]) / 1e3, b / HBM_BYTES_PER_S * 1e6
        emit({"workload": "cross_entropy_kernel_trace", "kernel": key, "R": R, "V": V, "dtype": name, "calls": int(hit[0]["Calls"]),
              "mean_us": mean_us, "min_us": float(hit[0]["MinNs"]) / 1e3, "bytes": b, "hbm_bound_us": bound_us,
              "fraction_of_bound": bound_us / mean_us, "bound": "HBM copy rate 6.3 TB/s"})


def bench_head(args):
    import torch
    import torch.nn.functional as F
    from mop_amd import _lib, ops
    for M, V in _shapes(args):
        for name, dt in _dtypes(args):
            g = torch.Generator(device="cuda").manual_seed(0)
            x = torch.randn(M, D, device="cuda", generator=g).to(dt).requires_grad_()
            w = (torch.randn(V, D, device="cuda", generator=g) * 0.02).to(dt).requires_grad_()
            t = torch.randint(0, V, (M,), device="cuda", generator=g)

            def run(loss_fn):
                x.grad = w.grad = None
                loss_fn().backward()

            def measure(loss_fn):
                ms = _time(lambda: run(loss_fn), args.steps, args.warmup)
                x.grad = w.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                run(loss_fn)
                torch.cuda.synchronize()
                return ms, torch.cuda.max_memory_allocated() - base
            ms_t, peak_t = measure(lambda: F.cross_entropy(F.linear(x, w).float(), t))
            for c in CHUNKS:
                ms, peak = measure(lambda: ops.linear_cross_entropy(x, w, t, chunk_rows=c or M))
                assert ops.LAST_PATH["linear_cross_entropy"] == _lib.PATH_FUSED
                emit({"workload": "linear_cross_entropy", "M": M, "D": D, "V": V, "dtype": name, "chunk_rows": c or M, "fused_ms": ms,
                      "torch_ms": ms_t, "fused_peak_bytes": peak, "torch_peak_bytes": peak_t, "peak_fraction": peak / peak_t,
                      "steps": args.steps, "warmup": args.warmup,
                      "what": "head + mean loss, forward and backward to x and weight; torch = F.cross_entropy(F.linear(x, w).float(), t); "
                              "peak = max_memory_allocated above what was allocated before the call (gradients included)"})
            del x, w
            torch.cuda.empty_cache()


def bench_step(args):
    """one training step of one model with one loss (bench_gpt.py's / bench_whisper.py's shapes)"""
    import torch
    import torch.nn.functional as F
    from mop_amd import ops
    torch.manual_seed(0)
    if args.model == "whisper":
        from mop_amd.nn import WhisperConfig, create_whisper_mop     # bench_whisper.py's step: fp32 parameters, bf16 autocast
        Bw, Ta, Tt, Vw = 8, 1500, 448, 51865
        m = create_whisper_mop(WhisperConfig(n_mels=80, n_audio_ctx=Ta, vocab_size=Vw, n_text_ctx=Tt, n_embd=512, n_head=8,
                                             n_layer_enc=6, n_layer_dec=6)).cuda().train()
        mel = torch.randn(Bw, Ta, 80, device="cuda")
        ids, tgt = torch.randint(0, Vw, (Bw, Tt), device="cuda"), torch.randint(0, Vw, (Bw, Tt), device="cuda")

        def torch_loss():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return m(mel, ids, tgt)[1]

        def fused_loss():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return m.loss(mel, ids, tgt)[0]
    else:
        from mop_amd.nn.quartet_attn_patch import TinyTransformerLM, TransformerConfig
        Bg, Tg, Vg = 8, 1024, 50304
        m = TinyTransformerLM(Vg, TransformerConfig(n_layer=12, n_head=12, n_embd=768, block_size=Tg, dropout=0.0)).cuda().to(torch.bfloat16).train()
        idx, tgt = torch.randint(0, Vg, (Bg, Tg), device="cuda"), torch.randint(0, Vg, (Bg, Tg), device="cuda")
        torch_loss = lambda: F.cross_entropy(m(idx)[0].float().view(-1, Vg), tgt.view(-1))        # noqa: E731
        fused_loss = lambda: m.loss(idx, tgt)                                                      # noqa: E731
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    loss_fn = fused_loss if args.loss == "fused" else torch_loss

    def step():
        opt.zero_grad(set_to_none=True)
        loss_fn().backward()
        opt.step()
    ms = _time(step, args.steps, args.warmup)
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    emit({"workload": args.model + "_train_step", "loss": args.loss, "ms_per_step": ms, "peak_bytes": torch.cuda.max_memory_allocated(),
          "steps": args.steps, "warmup": args.warmup, "dtype": "bf16", "pair": args.pair, "chunk_rows": ops.LINEAR_CE_CHUNK_ROWS,
          "what": "forward, loss, backward, AdamW; loss torch = the step of bench_gpt.py / bench_whisper.py, fused = model.loss()"})


def main():
    global RECORD
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["op", "op-trace", "head", "step"], default="op")
    ap.add_argument("--shape", type=int, choices=[0, 1], default=None)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default=None)
    ap.add_argument("--model", choices=["quartet_lm", "whisper"], default="quartet_lm")
    ap.add_argument("--loss", choices=["torch", "fused"], default="fused")
    ap.add_argument("--pair", type=int, default=0, help="which of the alternating pairs this run belongs to (recorded)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --workload op-trace run")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/cross_entropy_bench.jsonl")
    args = ap.parse_args()
    if args.record:
        RECORD = os.path.join(ROOT, "profiles", "cross_entropy_bench.jsonl")
    if args.stats:
        return stats(args)
    {"op": bench_op, "op-trace": op_trace, "head": bench_head, "step": bench_step}[args.workload](args)


if __name__ == "__main__":
    main()
