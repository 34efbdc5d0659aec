#!/usr/bin/env python3
"""GPT-line benchmark (GPU box): one JSON line per workload, at BASELINE.json configs[3]'s shape (B = 8, T = 1024, d = 768, 12 heads,
bf16).

    python tools/bench_gpt.py --workload step     # GPT_MoP and the Quartet TinyTransformerLM training step (12 layers, vocab 50304)
    python tools/bench_gpt.py --workload gate     # the MoPBlock gate alone: fused op vs the reference's torch composition, fwd+bwd
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_gpt.py --workload gate-trace
    python tools/bench_gpt.py --stats DIR/<host>/<pid>_kernel_stats.csv   # the two gate kernels against their byte bound

Times come from HIP events around `--steps` iterations after `--warmup` ones.  The byte bound divides the bytes a kernel must move
(each input read once, each output written once) by 6.3 TB/s, the measured HBM copy rate; at this shape one (B,T,D) bf16 tensor is
12.6 MB, which fits in the 256 MiB last-level cache (MALL), so a kernel in a loop can beat the HBM bound.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, T, D, H, LAYERS, VOCAB, V, K = 8, 1024, 768, 12, 12, 50304, 5, 3
HBM_BYTES_PER_S = 6.3e12


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


def bench_step(args):
    import torch
    import torch.nn.functional as F
    from mop_amd import _lib, ops
    from mop_amd.nn import GPT_MoP
    from mop_amd.nn.quartet_attn_patch import TinyTransformerLM, TransformerConfig
    cfg = TransformerConfig(n_layer=LAYERS, n_head=H, n_embd=D, block_size=T, dropout=0.0)
    for name, make in (("gpt_mop", lambda: GPT_MoP(VOCAB, cfg, n_views=V, n_kernels=K)),
                       ("quartet_lm", lambda: TinyTransformerLM(VOCAB, cfg))):
        torch.manual_seed(0)
        m = make().cuda().to(torch.bfloat16).train()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
        idx = torch.randint(0, VOCAB, (B, T), device="cuda")
        tgt = torch.randint(0, VOCAB, (B, T), device="cuda")

        def step():
            opt.zero_grad(set_to_none=True)
            logits, _ = m(idx)
            F.cross_entropy(logits.float().view(-1, VOCAB), tgt.view(-1)).backward()
            opt.step()
        ms = _time(step, args.steps, args.warmup)
        fused = ops.LAST_PATH.get("token_gate_fwd") == _lib.PATH_FUSED if name == "gpt_mop" else None
        print(json.dumps({"workload": name + "_train_step", "ms_per_step": ms, "sequences_per_s": B / ms * 1e3, "steps": args.steps,
                          "warmup": args.warmup, "dtype": "bf16", "fused_gate": fused,
                          "config": {"batch": B, "seq": T, "dim": D, "heads": H, "layers": LAYERS, "vocab": VOCAB,
                                     "n_views": V if name == "gpt_mop" else None, "n_kernels": K if name == "gpt_mop" else None,
                                     "n_params": sum(p.numel() for p in m.parameters()),
                                     "step": "forward, cross-entropy on fp32 logits, backward, AdamW"}}), flush=True)
        del m, opt
        torch.cuda.empty_cache()


def _gate_setup():
    import torch
    from mop_amd.nn import MoPBlock
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    torch.manual_seed(0)
    blk = MoPBlock(TransformerConfig(n_head=H, n_embd=D, block_size=T, dropout=0.0), n_views=V, n_kernels=K).cuda().to(torch.bfloat16)
    x = torch.randn(B, T, D, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
    a = torch.randn(B, T, D, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, T, D, device="cuda", dtype=torch.bfloat16)
    return blk, x, a, dout


def bench_gate(args):
    import torch
    from mop_amd import _lib, ops
    blk, x, a, dout = _gate_setup()

    def fused():
        blk.zero_grad(set_to_none=True)
        y = blk._gated_residual(x, a)
        y.backward(dout)

    def torch_ref():                     # the reference's MoPBlock: x + attn, then apply_mop's views -> conv -> cat -> fuse -> multiply
        blk.zero_grad(set_to_none=True)
        r = x + a
        y = r * blk._gate_torch(r)[0].transpose(1, 2)
        y.backward(dout)
    t_f = _time(fused, args.steps, args.warmup)
    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_FUSED
    t_t = _time(torch_ref, args.steps, args.warmup)
    print(json.dumps({"workload": "mop_gate_fwd_bwd", "fused_ms": t_f, "torch_ms": t_t, "speedup": t_t / t_f, "steps": args.steps,
                      "warmup": args.warmup, "dtype": "bf16",
                      "config": {"batch": B, "seq": T, "dim": D, "n_views": V, "n_kernels": K,
                                 "what": "residual add + gate + multiply of one MoPBlock, forward and backward to x, a and the four "
                                         "gate parameters; fused = taps fold (torch) + mopk_token_gate_{fwd,bwd}"}}), flush=True)


def gate_trace(args):
    """the fused gate only (under rocprofv3 --kernel-trace)"""
    blk, x, a, dout = _gate_setup()
    import torch
    for _ in range(args.warmup + args.steps):
        blk.zero_grad(set_to_none=True)
        blk._gated_residual(x, a).backward(dout)
    torch.cuda.synchronize()


def stats(path):
    """rocprofv3 kernel_stats.csv -> the gate kernels' mean time against bytes / 6.3 TB/s"""
    n_tok, n_el = B * T, B * T * D
    tiles = B * ((T + 15) // 16)
    parts = min(tiles, 512)
    part_bytes = parts * 3 * D * 4
    bytes_ = {"tg_fwd_kernel": 3 * 2 * n_el + 4 * n_tok,                               # x, a read; out written (bf16); gate (fp32)
              "tg_bwd_kernel": 4 * 2 * n_el + 4 * n_tok + part_bytes,                 # dout, x, a read; dr written; gate; partials
              "tg_reduce_kernel": part_bytes + 3 * D * 4}
    rows = list(csv.DictReader(open(path)))
    for key, nbytes in bytes_.items():
        hit = [r for r in rows if key in r["Name"]]
        if not hit:
            continue
        r = hit[0]
        mean_us = float(r["AverageNs"]) / 1e3
        bound_us = nbytes / HBM_BYTES_PER_S * 1e6
        print(json.dumps({"workload": "mop_gate_kernel_trace", "kernel": key, "calls": int(r["Calls"]), "mean_us": mean_us,
                          "min_us": float(r["MinNs"]) / 1e3, "bytes": nbytes, "hbm_bound_us": bound_us, "x_bound": mean_us / bound_us,
                          "bound": "HBM copy rate 6.3 TB/s (each tensor 12.6 MB bf16: L3/MALL-resident in a loop)",
                          "config": {"batch": B, "seq": T, "dim": D, "dtype": "bf16"}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["step", "gate", "gate-trace"], default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a --workload gate-trace run")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)
    {"step": bench_step, "gate": bench_gate, "gate-trace": gate_trace}[args.workload or "gate"](args)


if __name__ == "__main__":
    main()
