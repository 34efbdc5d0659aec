#!/usr/bin/env python3
"""Whisper-MoP benchmark (GPU box): one JSON line per measurement, appended to --out (default profiles/whisper_bench.jsonl).

    python tools/bench_whisper.py --workload step    # a WhisperMoP training step (fwd, bwd, AdamW) at a Whisper-base-like size
    python tools/bench_whisper.py --workload core    # the cross-attention core alone, fwd and fwd+bwd, vs torch SDPA
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_whisper.py --workload core-trace
    python tools/bench_whisper.py --stats DIR/<host>/<pid>_kernel_stats.csv   # cross-attention kernels against the bf16 MFMA peak

Step shape: d = 512, H = 8, 6 encoder + 6 decoder layers, T_a = 1500 audio frames, T_t = 448 tokens, vocab 51865, B = 8, fp32
parameters under bf16 autocast.  Three attention back ends run the same model: the default path (fused HIP kernels), libmopk's
generic path (ops.set_path("generic")), and "torch-eager": every attention core replaced by the reference's own composition
(q k^T * scale, masked_fill, softmax, @ v in torch).  Times come from HIP events around --steps iterations after --warmup ones.

Roofline: the cross-attention forward needs 4 B H N Nk dk FLOP (two GEMMs), the backward about 2.5x that (five GEMMs, with the
score recompute); the bf16 dense MFMA peak of the MI355X is 2.5 PFLOP/s (spec).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, TA, TT, D, H, LAYERS, VOCAB, NMELS = 8, 1500, 448, 512, 8, 6, 51865, 80
BF16_PEAK = 2.5e15


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


def _torch_sdpa_core(q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p=0.0, seed=None):
    """the reference's attention arithmetic in eager torch (whisper_mop.py MultiheadSelfAttention / MultiheadCrossAttention)"""
    import torch
    import torch.nn.functional as F
    Bq, N, Hh, dk = q.shape
    q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    att = (q @ k.transpose(-2, -1)) * dk ** -0.5
    if causal:
        att = att.masked_fill(~torch.tril(torch.ones(N, N, device=q.device, dtype=torch.bool)), float("-inf"))
    if bias is not None:
        att = att + bias
    att = F.softmax(att, dim=-1)
    return (att @ v).transpose(1, 2).reshape(Bq, N, Hh * dk)


def bench_step(args):
    import torch
    from mop_amd import ops
    from mop_amd.nn import WhisperConfig, create_whisper_mop
    from mop_amd.nn import whisper_mop as wm
    cfg = WhisperConfig(n_mels=NMELS, n_audio_ctx=TA, vocab_size=VOCAB, n_text_ctx=TT, n_embd=D, n_head=H, n_layer_enc=LAYERS,
                        n_layer_dec=LAYERS)
    torch.manual_seed(0)
    m = create_whisper_mop(cfg).cuda().train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    mel = torch.randn(B, TA, NMELS, device="cuda")
    ids = torch.randint(0, VOCAB, (B, TT), device="cuda")
    tgt = torch.randint(0, VOCAB, (B, TT), device="cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, loss, _ = m(mel, ids, tgt)
        loss.backward()
        opt.step()

    out = []
    orig = wm.ops.sdpa_core
    for backend in ("default", "generic", "torch-eager"):
        ops.set_path("generic" if backend == "generic" else "auto")
        if backend == "torch-eager":
            wm.ops.sdpa_core = _torch_sdpa_core
        try:
            ms = _time(step, args.steps, args.warmup)
            peak = torch.cuda.max_memory_allocated() / 2 ** 30
        finally:
            wm.ops.sdpa_core = orig
            ops.set_path("auto")
        out.append(dict(workload="whisper_step", backend=backend, ms=round(ms, 3), B=B, T_a=TA, T_t=TT, d=D, H=H,
                        layers=f"{LAYERS}+{LAYERS}", vocab=VOCAB, dtype="bf16-autocast", max_mem_gib=round(peak, 1),
                        steps=args.steps, warmup=args.warmup))
        print(json.dumps(out[-1]), flush=True)
    return out


def bench_core(args, trace=False):
    import torch
    import torch.nn.functional as F
    from mop_amd import _lib, ops
    N, Nk, dk = TT, TA, D // H
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, N, H, dk, device="cuda", dtype=torch.bfloat16, generator=g).requires_grad_(True)
    k = torch.randn(B, Nk, H, dk, device="cuda", dtype=torch.bfloat16, generator=g).requires_grad_(True)
    v = torch.randn(B, Nk, H, dk, device="cuda", dtype=torch.bfloat16, generator=g).requires_grad_(True)
    dy = torch.randn(B, N, H * dk, device="cuda", dtype=torch.bfloat16, generator=g)
    flop_f = 4.0 * B * H * N * Nk * dk
    cases = {
        "mopk": lambda: ops.sdpa_core(q, k, v),
        "torch_sdpa": lambda: F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2),
                                                              v.transpose(1, 2)).transpose(1, 2).reshape(B, N, H * dk),
    }
    out = []
    for name, fn in cases.items():
        def fwd():
            with torch.no_grad():
                fn()

        def fwdbwd():
            fn().backward(dy)
        if trace:
            if name == "mopk":
                for _ in range(args.warmup + args.steps):
                    fwdbwd()
                torch.cuda.synchronize()
            continue
        tf, tfb = _time(fwd, args.steps, args.warmup), _time(fwdbwd, args.steps, args.warmup)
        out.append(dict(workload="cross_attention_core", impl=name, B=B, H=H, N=N, Nk=Nk, dk=dk, dtype="bf16", fwd_ms=round(tf, 4),
                        fwd_bwd_ms=round(tfb, 4), fwd_tflops=round(flop_f / tf / 1e9, 1),
                        fwd_bwd_tflops=round(3.5 * flop_f / tfb / 1e9, 1), steps=args.steps, warmup=args.warmup))
        if name == "mopk":
            out[-1]["path"] = "fused" if ops.LAST_PATH.get("sdpa_fwd") == _lib.PATH_FUSED else "generic"
        print(json.dumps(out[-1]), flush=True)
    return out


def stats(path):
    """the fused SDPA kernels of a `core-trace` run against the bf16 MFMA peak (per call averages)"""
    N, Nk, dk = TT, TA, D // H
    flop_f = 4.0 * B * H * N * Nk * dk
    rows = list(csv.DictReader(open(path)))
    out = []
    for r in rows:
        name = r["Name"]
        if "sdpa_flash" not in name:
            continue
        avg_ns = float(r["AverageNs"])
        kind = "fwd" if "fwd_kernel" in name else "dq" if "dq_kernel" in name else "dkv" if "dkv_kernel" in name else "delta"
        flop = {"fwd": flop_f, "dq": 1.5 * flop_f, "dkv": 2.0 * flop_f, "delta": 0.0}[kind]   # dq: S, dP, dQ; dkv: S, dP, dV, dK
        out.append(dict(workload="cross_attention_kernels", kernel=kind, calls=int(r["Calls"]), avg_us=round(avg_ns / 1e3, 1),
                        tflops=round(flop / avg_ns / 1e3, 1) if flop else None,
                        pct_bf16_peak=round(100 * flop / (avg_ns * 1e-9) / BF16_PEAK, 1) if flop else None))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["step", "core", "core-trace"], default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "whisper_bench.jsonl"))
    args = ap.parse_args()
    if args.stats:
        lines = stats(args.stats)
    elif args.workload == "step":
        lines = bench_step(args)
    elif args.workload in ("core", "core-trace"):
        lines = bench_core(args, trace=args.workload == "core-trace")
    else:
        ap.error("--workload or --stats")
    if lines and args.out != "-":
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
