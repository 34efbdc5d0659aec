#!/usr/bin/env python3
"""Optimiser-step benchmark (GPU box): one JSON line per measurement, appended to --out (default profiles/optimizer_bench.jsonl).

    python tools/bench_optimizer.py                    # the optimiser step alone, three fresh processes
    python tools/bench_optimizer.py --workload step    # bench_gpt.py's GPT_MoP training step, torch.optim.AdamW against FusedAdamW

Parameter sets: the shapes and dtypes of the real models (ViT-MoP 5.4 M in bf16 as tools/bench_vit.py builds it, the 124 M GPT_MoP
of tools/bench_gpt.py in bf16, the WhisperMoP of tools/bench_whisper.py in fp32) with random values and random gradients.
Configurations: (a) torch.optim.AdamW as the tools construct it, (b) torch.optim.AdamW(fused=True) where this torch build has it,
(c) mop_amd.optim.FusedAdamW; each plain and with clipping + EMA (for (a) and (b): clip_grad_norm_ and the reference drivers' EMA
loop, experiments/imagenet_ab_param_budgets.py:699-716).  Times come from HIP events around --steps steps after --warmup ones; the
configurations of a set alternate inside one process, --rounds times, and the median is reported; launches per step are counted
with torch.profiler on one step (FusedAdamW's also by mopk_adamw_launches).  The byte bound divides the bytes a step must move (p, g,
m, v read and p, m, v written once; clipping reads g once more; the EMA is read and written once) by 6.3 TB/s, the measured HBM copy
rate.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12
MAX_NORM, EMA_DECAY = 1.0, 0.999


def _shapes(name):
    """[(shape, dtype)] of the model's parameters, built on the CPU and dropped"""
    import torch
    if name == "vit_mop_5m":
        from mop_amd.nn import ViT_MoP
        m = ViT_MoP(dim=384, depth=3, heads=6, n_classes=100, n_views=5, n_kernels=3, drop_path=0.0).to(torch.bfloat16)
    elif name == "gpt_124m":
        import bench_gpt as bg
        from mop_amd.nn import GPT_MoP
        from mop_amd.nn.quartet_attn_patch import TransformerConfig
        cfg = TransformerConfig(n_layer=bg.LAYERS, n_head=bg.H, n_embd=bg.D, block_size=bg.T, dropout=0.0)
        m = GPT_MoP(bg.VOCAB, cfg, n_views=bg.V, n_kernels=bg.K).to(torch.bfloat16)
    else:
        import bench_whisper as bw
        from mop_amd.nn import WhisperConfig, create_whisper_mop
        m = create_whisper_mop(WhisperConfig(n_mels=bw.NMELS, n_audio_ctx=bw.TA, vocab_size=bw.VOCAB, n_text_ctx=bw.TT, n_embd=bw.D,
                                             n_head=bw.H, n_layer_enc=bw.LAYERS, n_layer_dec=bw.LAYERS))
    return [(tuple(p.shape), p.dtype) for p in m.parameters() if p.requires_grad]


def _bytes(shapes, clip_ema):
    import torch
    total = 0
    for shape, dt in shapes:
        n, s = int(torch.Size(shape).numel()), torch.empty((), dtype=dt).element_size()
        total += n * (2 * s + s + 16 + ((s + 2 * s) if clip_ema else 0))
    return total


def _make(config, shapes, clip_ema):
    """-> (step function, optimiser)"""
    import torch
    from mop_amd.optim import FusedAdamW
    gen = torch.Generator(device="cuda").manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen).to(d) * 0.02) for s, d in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen).to(p.dtype)
    kw = dict(lr=1e-4, weight_decay=5e-2)
    if config == "fused_adamw":
        opt = FusedAdamW(params, max_grad_norm=MAX_NORM if clip_ema else None, ema_decay=EMA_DECAY if clip_ema else None, **kw)
        return opt.step, opt
    opt = torch.optim.AdamW(params, fused=True, **kw) if config == "torch_fused" else torch.optim.AdamW(params, **kw)
    if not clip_ema:
        return opt.step, opt
    ema = [p.detach().clone() for p in params]

    def step():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        with torch.no_grad():
            for e, p in zip(ema, params):
                e.mul_(EMA_DECAY).add_(p.detach(), alpha=1.0 - EMA_DECAY)
    return step, opt


def _launches(step):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:                                    # the count is a report, the timing does not depend on it
        return f"unavailable: {type(e).__name__}"


def _time(step, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def child(args):
    import torch
    from mop_amd import _lib, ops
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    for name in args.sets.split(","):
        shapes = _shapes(name)
        n_params = sum(int(torch.Size(s).numel()) for s, _ in shapes)
        for clip_ema in (False, True):
            configs = ["torch_adamw", "torch_fused", "fused_adamw"]
            made = {}
            for c in configs:
                try:
                    made[c] = _make(c, shapes, clip_ema)
                    for _ in range(args.warmup):
                        made[c][0]()
                except Exception as e:
                    if c != "torch_fused":
                        raise
                    print(json.dumps({"set": name, "config": c, "unavailable": f"{type(e).__name__}: {e}"[:200]}), flush=True)
            torch.cuda.synchronize()
            times = {c: [] for c in made}
            for _ in range(args.rounds):
                for c in made:                                 # alternating order
                    times[c].append(_time(made[c][0], args.steps))
            bound_ms = _bytes(shapes, clip_ema) / HBM_BYTES_PER_S * 1e3
            for c in made:
                ms = statistics.median(times[c])
                rec = {"workload": "optimizer_step", "set": name, "n_params": n_params, "n_tensors": len(shapes), "config": c,
                       "clip_ema": clip_ema, "ms_per_step": ms, "ms_rounds": times[c], "launches_per_step": _launches(made[c][0]),
                       "bytes": _bytes(shapes, clip_ema), "byte_bound_ms": bound_ms, "share_of_byte_bound": bound_ms / ms,
                       "steps": args.steps, "warmup": args.warmup, "pid": os.getpid()}
                if c == "fused_adamw":
                    rec["path"] = "fused" if ops.LAST_PATH.get("adamw") == _lib.PATH_FUSED else "generic"
                print(json.dumps(rec), flush=True)
            del made
            torch.cuda.empty_cache()


def step_workload(args):
    """bench_gpt.py's GPT_MoP training step with torch.optim.AdamW against FusedAdamW, in alternating pairs"""
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_gpt as bg
    from mop_amd.nn import GPT_MoP
    from mop_amd.nn.quartet_attn_patch import TransformerConfig
    from mop_amd.optim import FusedAdamW
    cfg = TransformerConfig(n_layer=bg.LAYERS, n_head=bg.H, n_embd=bg.D, block_size=bg.T, dropout=0.0)
    torch.manual_seed(0)
    m = GPT_MoP(bg.VOCAB, cfg, n_views=bg.V, n_kernels=bg.K).cuda().to(torch.bfloat16).train()
    idx = torch.randint(0, bg.VOCAB, (bg.B, bg.T), device="cuda")
    tgt = torch.randint(0, bg.VOCAB, (bg.B, bg.T), device="cuda")
    opts = {"torch_adamw": torch.optim.AdamW(m.parameters(), lr=1e-4), "fused_adamw": FusedAdamW(m.parameters(), lr=1e-4)}

    def step(opt):
        opt.zero_grad(set_to_none=True)
        logits, _ = m(idx)
        F.cross_entropy(logits.float().view(-1, bg.VOCAB), tgt.view(-1)).backward()
        opt.step()
    for o in opts.values():
        for _ in range(args.warmup):
            step(o)
    torch.cuda.synchronize()
    times = {c: [] for c in opts}
    for _ in range(3):
        for c, o in opts.items():
            times[c].append(_time(lambda: step(o), args.steps))
    for c in opts:
        print(json.dumps({"workload": "gpt_mop_train_step", "optimizer": c, "ms_per_step": statistics.median(times[c]), "ms_pairs": times[c],
                          "steps": args.steps, "warmup": args.warmup}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["optimizer", "step"], default="optimizer")
    ap.add_argument("--sets", default="vit_mop_5m,gpt_124m,whisper")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds inside one process")
    ap.add_argument("--processes", type=int, default=3, help="fresh processes, one after the other")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args) if args.workload == "optimizer" else step_workload(args)
    procs = args.processes if args.workload == "optimizer" else 1
    for i in range(procs):                                     # this process never opens the GPU: every measurement starts fresh
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(dict(json.loads(ln), process=i)) + "\n")
        print("\n".join(lines), flush=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
