#!/usr/bin/env python3
"""WhisperMoP mel-gate benchmark (GPU box): one JSON line per measurement, appended to --out (default
profiles/whisper_gate_bench.jsonl).  Shapes and conventions of tools/bench_whisper.py.

    python tools/bench_whisper_gate.py --workload ops                   # ops.mel_gate and ops.gated_residual against torch
    python tools/bench_whisper_gate.py --workload model --parent DIR    # training step and bare encode against the parent commit

ops: ops.mel_gate (taps fold included) at L = 6, B = 8, T = 1500, F = 80, k = 5, forward and forward + backward to the MoP2D
parameters, against the six MoP2D.forward calls it replaces (fp32, as the encoder's mel map is); ops.gated_residual at D = 512
(fp32 x, bf16 a: what the block sees under bf16 autocast) against (x + a) * g.
model: DIR is a checkout of the parent commit with its library built.  Each measurement is a fresh process (--child) that imports
mop_amd from its own tree; this tree and the parent run in alternating pairs, and the line records every pair, the medians and the
spread of the pairs (max - min of each side)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
B, TA, TT, D, H, LAYERS, VOCAB, NMELS = 8, 1500, 448, 512, 8, 6, 51865, 80
VIEWS, KERNELS, KSIZE = 5, 3, 5


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


def _launch_ms(fn, keys, steps):
    """median milliseconds between HIP events around each libmopk launch of fn (ops.enable_timing): the kernels without the host"""
    import torch
    from mop_amd import ops
    ops.enable_timing(True)
    try:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        res = ops.timing_results()
    finally:
        ops.enable_timing(False)
    return {k: round(statistics.median(res[k]), 4) for k in keys}


def bench_ops(args):
    import torch
    from mop_amd import _lib, ops
    from mop_amd.nn import MoP2D
    from mop_amd.nn.whisper_mop import _stacked_taps
    torch.manual_seed(0)
    mops = [MoP2D(VIEWS, KERNELS, KSIZE).cuda() for _ in range(LAYERS)]
    params = [p for m in mops for p in m.parameters()]
    mel = torch.randn(B, TA, NMELS, device="cuda")
    mel2d = mel.unsqueeze(1).contiguous()
    dg = torch.randn(B, LAYERS, TA, device="cuda")

    def fused():
        return ops.mel_gate(mel, _stacked_taps(mops, NMELS))

    def convs():
        return torch.cat([m(mel2d)[0] for m in mops], dim=2).transpose(1, 2)

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def fwdbwd(fn):
        def run():
            for p in params:
                p.grad = None
            (fn() * dg).sum().backward()
        return run

    out = []
    line = dict(workload="mel_gate", B=B, T=TA, F=NMELS, L=LAYERS, k=KSIZE, n_views=VIEWS, n_kernels=KERNELS, dtype="fp32",
                steps=args.steps, warmup=args.warmup,
                what="all layers' gates from the mel map; fused = taps fold (torch) + mopk_mel_gate_{fwd,bwd}, torch = six MoP2D.forward")
    for name, fn in (("fused", fused), ("torch", convs)):
        line[name + "_fwd_ms"] = round(_time(fwd(fn), args.steps, args.warmup), 4)
        line[name + "_fwd_bwd_ms"] = round(_time(fwdbwd(fn), args.steps, args.warmup), 4)
    assert ops.LAST_PATH["mel_gate_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["mel_gate_bwd"] == _lib.PATH_FUSED
    line["fwd_speedup"] = round(line["torch_fwd_ms"] / line["fused_fwd_ms"], 2)
    line["fwd_bwd_speedup"] = round(line["torch_fwd_bwd_ms"] / line["fused_fwd_bwd_ms"], 2)
    line["launch_ms"] = _launch_ms(fwdbwd(fused), ("mel_gate_fwd", "mel_gate_bwd"), args.steps)
    out.append(line)
    print(json.dumps(line), flush=True)

    x = torch.randn(B, TA, D, device="cuda", requires_grad=True)
    a = torch.randn(B, TA, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    g = (1 + 0.1 * torch.randn(B, TA, device="cuda")).requires_grad_()
    dout = torch.randn(B, TA, D, device="cuda")
    cases = {"fused": lambda: ops.gated_residual(x, a, g), "torch": lambda: (x + a) * g.unsqueeze(-1)}
    line = dict(workload="gated_residual", B=B, T=TA, D=D, dtype="fp32 x, bf16 a", steps=args.steps, warmup=args.warmup)
    def fb(fn):
        def run():
            x.grad = a.grad = g.grad = None
            fn().backward(dout)
        return run
    for name, fn in cases.items():
        line[name + "_fwd_ms"] = round(_time(fwd(fn), args.steps, args.warmup), 4)
        line[name + "_fwd_bwd_ms"] = round(_time(fb(fn), args.steps, args.warmup), 4)
    assert ops.LAST_PATH["gated_residual_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["gated_residual_bwd"] == _lib.PATH_FUSED
    line["launch_ms"] = _launch_ms(fb(cases["fused"]), ("gated_residual_fwd", "gated_residual_bwd"), args.steps)
    nbytes = B * TA * D * (4 + 2 + 4)                                # x, a in, out
    line["launch_fwd_gbps"] = round(nbytes / line["launch_ms"]["gated_residual_fwd"] / 1e6, 1)
    line["fwd_speedup"] = round(line["torch_fwd_ms"] / line["fused_fwd_ms"], 2)
    line["fwd_bwd_speedup"] = round(line["torch_fwd_bwd_ms"] / line["fused_fwd_bwd_ms"], 2)
    out.append(line)
    print(json.dumps(line), flush=True)
    return out


def child(args):
    """one process, one tree: the training step of tools/bench_whisper.py (default back end) and a bare encode"""
    sys.path.insert(0, args.root)
    import torch
    import mop_amd
    from mop_amd.nn import WhisperConfig, create_whisper_mop
    assert os.path.realpath(os.path.dirname(os.path.dirname(mop_amd.__file__))) == os.path.realpath(args.root)
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

    def encode():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            m.encode(mel)

    step_ms = _time(step, args.steps, args.warmup)
    m.eval()
    encode_ms = _time(encode, args.steps, args.warmup)
    print("CHILD " + json.dumps(dict(step_ms=step_ms, encode_ms=encode_ms)), flush=True)


def bench_model(args):
    if not args.parent or not os.path.isdir(os.path.join(args.parent, "mop_amd")):
        raise SystemExit("--workload model needs --parent DIR, a checkout of the parent commit with its library built")
    trees = {"parent": os.path.abspath(args.parent), "this": os.path.abspath(os.path.join(HERE, ".."))}
    runs = {k: [] for k in trees}
    for _ in range(args.pairs):
        for name, root in trees.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--steps", str(args.steps),
                                "--warmup", str(args.warmup)], cwd=root, capture_output=True, text=True, timeout=600)
            rows = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not rows:
                raise SystemExit(f"{name}: the measuring process ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:])
            runs[name].append(json.loads(rows[-1][6:]))
            print(name, runs[name][-1], flush=True)
    out = []
    for key, workload in (("step_ms", "whisper_step_vs_parent"), ("encode_ms", "whisper_encode_vs_parent")):
        p, t = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        line = dict(workload=workload, parent_ms=[round(v, 3) for v in p], this_ms=[round(v, 3) for v in t],
                    parent_median_ms=round(statistics.median(p), 3), this_median_ms=round(statistics.median(t), 3),
                    spread_ms=round(max(max(p) - min(p), max(t) - min(t)), 3), pairs=args.pairs, B=B, T_a=TA, T_t=TT, d=D, H=H,
                    layers=f"{LAYERS}+{LAYERS}", dtype="bf16-autocast", steps=args.steps, warmup=args.warmup)
        line["this_minus_parent_ms"] = round(line["this_median_ms"] - line["parent_median_ms"], 3)
        out.append(line)
        print(json.dumps(line), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["ops", "model"], default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "whisper_gate_bench.jsonl"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    sys.path.insert(0, os.path.join(HERE, ".."))
    if args.workload == "ops":
        lines = bench_ops(args)
    elif args.workload == "model":
        lines = bench_model(args)
    else:
        ap.error("--workload")
    if lines and args.out != "-":
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
