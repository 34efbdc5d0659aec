#!/usr/bin/env python3
"""Top-1 MoE MLP benchmark (GPU box): one JSON line per measurement, appended to --out (default profiles/moe_bench.jsonl).

    python tools/bench_moe.py --workload op      # the MoE MLP alone, fwd and fwd+bwd, bf16: HIP kernels vs two torch compositions
    python tools/bench_moe.py --workload step    # ViT_MoP(use_moe=True) bf16 training step at BASELINE configs[0] dims, eager and graphed
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_moe.py --workload op-trace
    python tools/bench_moe.py --stats DIR/<host>/<pid>_kernel_stats.csv   # per-kernel times against the bf16 MFMA peak

Op shape: M = 256 x 64 tokens, D = 384, F = 1536, E = 4, bf16 tensors, balanced routing (random gate) and skewed routing (gate bias
sending ~80 % of the tokens to one expert).  Implementations: "hip" (ops.moe_mlp), "dense" (the reference's composition: every
expert on every token, one-hot combine), "routed" (torch sort by expert + one matmul pair per expert; it needs the per-expert counts
on the host, a sync).  Times: HIP events around --steps iterations after --warmup, median of --repeats.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

M, D, F, E = 256 * 64, 384, 1536, 4
BF16_PEAK = 2.5e15


def _time(fn, steps, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out)


def _routed_torch(x, gw, gb, w1s, w2s):
    """torch routed composition: stable sort by expert, per-expert matmuls on the host-known counts, scatter back"""
    import torch
    import torch.nn.functional as Fn
    xf = x.reshape(-1, x.shape[-1])
    top = Fn.linear(xf, gw, gb).argmax(-1)
    order = torch.argsort(top, stable=True)
    counts = torch.bincount(top, minlength=len(w1s)).tolist()          # host sync
    xs = xf[order]
    ys = []
    for e, part in enumerate(torch.split(xs, counts)):
        ys.append(Fn.linear(Fn.gelu(Fn.linear(part, w1s[e]), approximate="tanh"), w2s[e]))
    y = torch.empty_like(xf)
    y[order] = torch.cat(ys)
    return y.view(x.shape)


def _op_inputs(skew):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(256, 64, D, device="cuda", generator=g, dtype=torch.bfloat16)
    gw = (torch.randn(E, D, device="cuda", generator=g) / D ** 0.5).to(torch.bfloat16)
    gb = torch.zeros(E, device="cuda", dtype=torch.bfloat16)
    if skew:
        lg = torch.nn.functional.linear(x.reshape(-1, D).float(), gw.float())
        gb[0] = float(torch.quantile((lg[:, 1:].max(-1).values - lg[:, 0])[:100000], 0.8))
    w1s = [(torch.randn(F, D, device="cuda", generator=g) / D ** 0.5).to(torch.bfloat16).requires_grad_(True) for _ in range(E)]
    w2s = [(torch.randn(D, F, device="cuda", generator=g) / F ** 0.5).to(torch.bfloat16).requires_grad_(True) for _ in range(E)]
    return x.requires_grad_(True), gw, gb, w1s, w2s


def bench_op(args, emit):
    import torch
    from mop_amd import ops
    for skew in (False, True):
        x, gw, gb, w1s, w2s = _op_inputs(skew)
        dy = torch.randn_like(x)
        counts = torch.bincount(ops.moe_route(x, gw, gb).long(), minlength=E).tolist()
        impls = {"hip": lambda: ops.moe_mlp(x, gw, gb, w1s, w2s), "dense": lambda: ops.moe_mlp_torch(x, gw, gb, w1s, w2s),
                 "routed": lambda: _routed_torch(x, gw, gb, w1s, w2s)}
        for name, f in impls.items():
            def fb(f=f):
                y = f()
                torch.autograd.grad(y, [x] + w1s + w2s, dy)
            with torch.no_grad():
                t_f = _time(f, args.steps, args.warmup, args.repeats)
            t_fb = _time(fb, args.steps, args.warmup, args.repeats)
            routed_flop = 2 * M * D * F * 2
            emit(dict(workload="moe_op", impl=name, routing="skewed" if skew else "balanced", tokens_per_expert=counts, M=M, D=D, F=F,
                      E=E, dtype="bf16", fwd_ms=round(t_f, 4), fwd_bwd_ms=round(t_fb, 4),
                      routed_fwd_tflops=round(routed_flop / t_f / 1e9, 1), routed_fwd_bwd_tflops=round(3 * routed_flop / t_fb / 1e9, 1)))


def bench_op_trace(args):
    """the fused op alone, for rocprofv3 --kernel-trace --stats: balanced routing, 20 fwd+bwd iterations"""
    import torch
    from mop_amd import ops
    x, gw, gb, w1s, w2s = _op_inputs(False)
    dy = torch.randn_like(x)
    for _ in range(25):
        y = ops.moe_mlp(x, gw, gb, w1s, w2s)
        torch.autograd.grad(y, [x] + w1s + w2s, dy)
    torch.cuda.synchronize()


# FLOPs per launch at the op shape (grouped GEMMs: 2 M D F each; route: 2 M D E)
KERNEL_FLOP = {"FC1": 2 * M * D * F, "FC2": 2 * M * D * F, "DU": 2 * M * D * F, "DX": 2 * M * D * F, "WG2": 2 * M * D * F,
               "WG1": 2 * M * D * F, "moe_logits_kernel": 2 * M * D * E}
MODE_NAMES = ["FC1", "FC2", "DU", "DX", "WG2", "WG1"]            # moe_gemm_kernel<MODE, ...> (mop_amd/csrc/moe_mlp.hip MoeMode)


def stats(path, emit):
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "moe_" not in name:
            continue
        mode = re.search(r"moe_gemm_kernel<(\d),", name)
        key = MODE_NAMES[int(mode.group(1))] if mode else \
            next((k for k in ("moe_logits_kernel", "moe_scan_kernel", "moe_wsum_kernel") if k in name), name)
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0)
        flop = KERNEL_FLOP.get(key)
        emit(dict(workload="moe_kernel", kernel=key, calls=int(r.get("Calls", 0)), avg_us=round(avg_ns / 1e3, 2),
                  tflops=round(flop / avg_ns / 1e3, 1) if flop and avg_ns else None,
                  bf16_peak_share=round(flop / avg_ns * 1e9 / BF16_PEAK, 3) if flop and avg_ns else None))


def bench_step(args, emit):
    import torch
    import torch.nn.functional as Fn
    from mop_amd.nn import ViT_MoP
    torch.manual_seed(0)
    for graph in (False, True):
        model = ViT_MoP(dim=384, depth=3, heads=6, n_classes=100, n_views=5, n_kernels=3, drop_path=0.0, use_moe=True,
                        moe_experts=4).cuda().to(torch.bfloat16).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
        xi = torch.randn(args.batch, 3, 32, 32, device="cuda", dtype=torch.bfloat16)
        tgt = torch.randint(0, 100, (args.batch,), device="cuda")

        def step(net):
            opt.zero_grad(set_to_none=True)
            loss = Fn.cross_entropy(net(xi).float(), tgt)
            loss.backward()
            opt.step()
        for _ in range(3):                        # eager warm-up before any capture (tools/graph_probe.py)
            step(model)
        torch.cuda.synchronize()
        net = model
        if graph:
            # the MoE gates get no gradient (as in the reference), and make_graphed_callables differentiates every parameter that
            # requires one: take them out of that set (their .grad is None either way, so AdamW skips them in both runs)
            for n, p in model.named_parameters():
                if ".mlp.gate." in n:
                    p.requires_grad_(False)
            net = torch.cuda.make_graphed_callables(model, (xi,), num_warmup_iters=0)
        t = _time(lambda: step(net), args.steps, args.warmup, args.repeats)
        emit(dict(workload="vit_moe_step", graph=graph, batch=args.batch, dim=384, depth=3, heads=6, experts=4, dtype="bf16",
                  step_ms=round(t, 3), images_per_s=round(args.batch / t * 1e3, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="op", choices=["op", "op-trace", "step"])
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of an op-trace run")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "moe_bench.jsonl"))
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if args.stats:
        return stats(args.stats, emit)
    import torch
    emit(dict(workload="device", name=torch.cuda.get_device_name(0), torch=torch.__version__))
    {"op": bench_op, "step": bench_step}.get(args.workload, lambda a, e: bench_op_trace(a))(args, emit)


if __name__ == "__main__":
    main()
