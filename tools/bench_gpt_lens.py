#!/usr/bin/env python3
"""Per-row sequence lengths on the GPT line (GPU box): one JSON line per case, appended to --out (default
profiles/gpt_lens_bench.jsonl).

    python tools/bench_gpt_lens.py --workload core     # ops.quartet_core: lengths vs no lengths vs every row alone
    python tools/bench_gpt_lens.py --workload gate     # ops.token_gate_1d at the same shape
    python tools/bench_gpt_lens.py --workload model    # GPT_MoP / TinyTransformerLM training step through loss(), list vs padded tensor

Core: bf16, B = 8, T = 1024, H = 12, dk = 64 (the README's GPT shape), Quartet term on, forward and forward + backward, for three
length profiles -- full (every row T), spread (uniform over [T/8, T]), one_long (one row T, seven rows T/8) -- by three routes:
    lens:    quartet_core(lens=)            the length-aware kernels
    nolens:  quartet_core()                 the same launch on the padded batch without the feature (computes the padding, and
                                            lets it into every row's statistics: a different function, the cost baseline)
    alone:   B calls, row b at its own T    the only way to these results before
Every case is timed with HIP events over --iters calls after --warmup calls, --repeats times, routes interleaved within a repeat;
the record holds the median and the min / max over repeats (the run-to-run spread) and the ideal work fraction of the profile,
sum len^2 / (B T^2).  The full-length overhead of the feature is lens / nolens at profile "full", to be read against the spread of
nolens itself.
Model: d = 768, 12 heads, 12 layers, vocab 50304, B = 8, T = 1024, bf16 autocast, loss() + backward (no optimiser): a list of
documents against the padded tensor without lengths.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, T, H, DK = 8, 1024, 12, 64


def profiles():
    return {"full": [T] * B,
            "spread": [round(T / 8 + i * (T - T / 8) / (B - 1)) for i in range(B)],
            "one_long": [T] + [T // 8] * (B - 1)}


def _emit(args, rec):
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _timed(fns, iters, warmup, repeats):
    """{name: [ms per call, one per repeat]}: the routes are interleaved inside a repeat so that drift hits them alike"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / iters)
    return out


def _stats(res, nd=4):
    return dict(ms={r: round(statistics.median(x), nd) for r, x in res.items()},
                ms_min={r: round(min(x), nd) for r, x in res.items()}, ms_max={r: round(max(x), nd) for r, x in res.items()})


def bench_core(args):
    import torch
    from mop_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    ts = [torch.randn(B, T, H, DK, device="cuda", generator=g).bfloat16().requires_grad_(True) for _ in range(5)]
    dy = torch.randn(B, T, H * DK, device="cuda", generator=g).bfloat16()
    mix = torch.tensor([0.3], device="cuda", requires_grad=True)
    qs = torch.tensor([0.8], device="cuda", requires_grad=True)

    def core(xs, **kw):
        return ops.quartet_core(xs[0], xs[1], xs[2], xs[3], xs[4], mix, qs, None, 1e-5, True, **kw)

    for pname, lens in profiles().items():
        lt = torch.tensor(lens, dtype=torch.int32, device="cuda")
        rows = [[t[b:b + 1, :n].detach().clone().requires_grad_(True) for t in ts] for b, n in enumerate(lens)]
        drow = [dy[b:b + 1, :n].clone() for b, n in enumerate(lens)]
        for mode in ("fwd", "fwd_bwd"):
            def batch(kw):
                def f():
                    if mode == "fwd":
                        with torch.no_grad():
                            core(ts, **kw)
                    else:
                        core(ts, **kw).backward(dy)
                        for t in ts + [mix, qs]:
                            t.grad = None
                return f

            def alone():
                for xs, d in zip(rows, drow):
                    if mode == "fwd":
                        with torch.no_grad():
                            core(xs)
                    else:
                        core(xs).backward(d)
                        for t in xs + [mix, qs]:
                            t.grad = None
            res = _timed({"lens": batch(dict(lens=lt)), "nolens": batch({}), "alone": alone}, args.iters, args.warmup, args.repeats)
            st = _stats(res)
            med = st["ms"]
            _emit(args, dict(workload="quartet_core_lens", mode=mode, B=B, T=T, H=H, dk=DK, dtype="bf16", profile=pname, lens=lens,
                             ideal_work_fraction=round(sum(n * n for n in lens) / (B * T * T), 4), **st,
                             lens_over_nolens=round(med["lens"] / med["nolens"], 4), lens_over_alone=round(med["lens"] / med["alone"], 4),
                             nolens_spread=round((st["ms_max"]["nolens"] - st["ms_min"]["nolens"]) / med["nolens"], 4),
                             iters=args.iters, warmup=args.warmup, repeats=args.repeats))


def bench_gate(args):
    import torch
    from mop_amd import ops
    D = H * DK
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, T, D, device="cuda", generator=g).bfloat16().requires_grad_(True)
    a = torch.randn(B, T, D, device="cuda", generator=g).bfloat16().requires_grad_(True)
    u = (0.05 * torch.randn(3, D, device="cuda", generator=g)).requires_grad_(True)
    dout = torch.randn(B, T, D, device="cuda", generator=g).bfloat16()
    for pname, lens in profiles().items():
        lt = torch.tensor(lens, dtype=torch.int32, device="cuda")
        for mode in ("fwd", "fwd_bwd"):
            def mk(l):
                def f():
                    if mode == "fwd":
                        with torch.no_grad():
                            ops.token_gate_1d(x, a, u, l)
                    else:
                        ops.token_gate_1d(x, a, u, l).backward(dout)
                        x.grad = a.grad = u.grad = None
                return f
            res = _timed({"lens": mk(lt), "nolens": mk(None)}, args.iters, args.warmup, args.repeats)
            st = _stats(res)
            _emit(args, dict(workload="token_gate_lens", mode=mode, B=B, T=T, D=D, dtype="bf16", profile=pname, lens=lens,
                             ideal_work_fraction=round(sum(lens) / (B * T), 4), **st,
                             lens_over_nolens=round(st["ms"]["lens"] / st["ms"]["nolens"], 4),
                             nolens_spread=round((st["ms_max"]["nolens"] - st["ms_min"]["nolens"]) / st["ms"]["nolens"], 4),
                             iters=args.iters, warmup=args.warmup, repeats=args.repeats))


def bench_model(args):
    import torch
    from mop_amd.nn import GPT_MoP, TinyTransformerLM, TransformerConfig
    V = 50304
    cfg = TransformerConfig(n_layer=12, n_head=H, n_embd=H * DK, dropout=0.0, block_size=T)
    for name, cls in (("GPT_MoP", GPT_MoP), ("TinyTransformerLM", TinyTransformerLM)):
        torch.manual_seed(0)
        m = cls(V, cfg).cuda().train()
        for pname, lens in profiles().items():
            g = torch.Generator(device="cuda").manual_seed(2)
            docs = [torch.randint(1, V, (n,), device="cuda", generator=g) for n in lens]
            tgts = [torch.randint(0, V, (n,), device="cuda", generator=g) for n in lens]
            pad_i = torch.nn.utils.rnn.pad_sequence(docs, batch_first=True)
            pad_t = torch.nn.utils.rnn.pad_sequence(tgts, batch_first=True, padding_value=-100)

            def step(i, t):
                def f():
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        loss = m.loss(i, t)
                    loss.backward()
                    m.zero_grad(set_to_none=True)
                return f
            res = _timed({"list": step(docs, tgts), "padded": step(pad_i, pad_t)}, max(args.iters // 10, 3), 2, args.repeats)
            st = _stats(res, 3)
            _emit(args, dict(workload="gpt_lens_model", model=name, profile=pname, lens=lens, B=B, T=T, d=H * DK, H=H, layers=12,
                             vocab=V, dtype="bf16-autocast", step="loss() + backward, no optimiser",
                             ideal_attention_fraction=round(sum(n * n for n in lens) / (B * T * T), 4),
                             list_over_padded=round(st["ms"]["list"] / st["ms"]["padded"], 4), **st, repeats=args.repeats))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["core", "gate", "model"], default="core")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "gpt_lens_bench.jsonl"))
    args = ap.parse_args()
    {"core": bench_core, "gate": bench_gate, "model": bench_model}[args.workload](args)
