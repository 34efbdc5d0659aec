#!/usr/bin/env python3
"""Per-row audio lengths benchmark (GPU box): one JSON line per case, appended to --out (default
profiles/whisper_audio_lens_bench.jsonl).

    python tools/bench_whisper_audio_lens.py --workload core     # ops.sdpa_core: lengths vs attn_mask vs no lengths
    python tools/bench_whisper_audio_lens.py --workload model    # WhisperMoP training step and generate, list vs padded tensor

Core: bf16, H x dk = 8 x 64 at T = 1500 (the README's Whisper shape, B = 8) and 6 x 64 at T = 3000 (the encoder shape of DESIGN
section 4.3, B = 8); encoder self-attention (N = Nk = T, q_lens = kv_lens) and cross-attention (N = 448 text queries, Nk = T,
kv_lens), forward and forward + backward, for three length profiles -- full (every row T), spread (uniform over [T/8, T]), one_long
(one row T, seven rows T/8) -- by three routes:
    lens:    sdpa_core(q_lens=, kv_lens=)      the length-aware kernels
    mask:    sdpa_core(attn_mask=(B,1,1,T))    a key-padding mask, what a caller could do before (the baseline)
    nolens:  sdpa_core()                       the padded batch with no lengths at all (computes the padding too)
Every case is timed with HIP events over --iters calls after --warmup calls, --repeats times, routes interleaved within a repeat;
the record holds the median and the min / max over repeats (the run-to-run spread), and the ideal work fraction of the profile:
sum len^2 / (B T^2) for self-attention, sum len / (B T) for cross-attention.
Model: d = 512, H = 8, 6 + 6 layers, T = 1500, B = 8, bf16 autocast: one training step (forward + loss + backward, 64 text tokens)
and generate (4 prompt tokens, --new-tokens new ones, ms per token), a list of clips against the zero-padded tensor.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B = 8


def profiles(T):
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


def bench_core(args):
    import torch
    from mop_amd import ops
    for T, H in ((1500, 8), (3000, 6)):
        for kind in ("self", "cross"):
            N = T if kind == "self" else 448
            g = torch.Generator(device="cuda").manual_seed(0)
            q = torch.randn(B, N, H, 64, device="cuda", generator=g).bfloat16().requires_grad_(True)
            k = torch.randn(B, T, H, 64, device="cuda", generator=g).bfloat16().requires_grad_(True)
            v = torch.randn(B, T, H, 64, device="cuda", generator=g).bfloat16().requires_grad_(True)
            dy = torch.randn(B, N, H * 64, device="cuda", generator=g).bfloat16()
            for pname, lens in profiles(T).items():
                lt = torch.tensor(lens, dtype=torch.int32, device="cuda")
                mask = (torch.arange(T, device="cuda").view(1, T) < lt.view(B, 1)).view(B, 1, 1, T)
                kw = {"lens": dict(q_lens=lt if kind == "self" else None, kv_lens=lt), "mask": dict(attn_mask=mask), "nolens": {}}
                ideal = sum(n * n for n in lens) / (B * T * T) if kind == "self" else sum(lens) / (B * T)
                for mode in ("fwd", "fwd_bwd"):
                    def mk(kws):
                        if mode == "fwd":
                            def f():
                                with torch.no_grad():
                                    ops.sdpa_core(q, k, v, **kws)
                        else:
                            def f():
                                ops.sdpa_core(q, k, v, **kws).backward(dy)
                                q.grad = k.grad = v.grad = None
                        return f
                    res = _timed({r: mk(kws) for r, kws in kw.items()}, args.iters, args.warmup, args.repeats)
                    med = {r: statistics.median(x) for r, x in res.items()}
                    _emit(args, dict(workload="sdpa_core_lens", attention=kind, mode=mode, T=T, N=N, B=B, H=H, dk=64, dtype="bf16",
                                     profile=pname, lens=lens, ideal_work_fraction=round(ideal, 4),
                                     ms={r: round(med[r], 4) for r in med},
                                     ms_min={r: round(min(x), 4) for r, x in res.items()},
                                     ms_max={r: round(max(x), 4) for r, x in res.items()},
                                     lens_over_mask=round(med["lens"] / med["mask"], 4),
                                     lens_over_nolens=round(med["lens"] / med["nolens"], 4),
                                     iters=args.iters, warmup=args.warmup, repeats=args.repeats))


def bench_model(args):
    import torch
    from mop_amd.nn import WhisperConfig, WhisperMoP
    T = 1500
    cfg = WhisperConfig(n_mels=80, n_audio_ctx=T, vocab_size=51865, n_text_ctx=448, n_embd=512, n_head=8, n_layer_enc=6, n_layer_dec=6)
    torch.manual_seed(0)
    m = WhisperMoP(cfg).cuda()
    ids = torch.randint(0, cfg.vocab_size, (B, 64), device="cuda")
    prompt = torch.randint(0, cfg.vocab_size, (B, 4), device="cuda")
    for pname, lens in profiles(T).items():
        clips = [torch.randn(n, 80, device="cuda") for n in lens]
        padded = torch.zeros(B, T, 80, device="cuda")
        for b, c in enumerate(clips):
            padded[b, :lens[b]] = c

        def train(mel):
            def f():
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = m(mel, ids, ids)[1]
                loss.backward()
                m.zero_grad(set_to_none=True)
            return f

        def gen(mel):
            def f():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    m.generate(mel, prompt, args.new_tokens, graph=True)
            return f
        m.train()
        res = _timed({"list": train(clips), "padded": train(padded)}, max(args.iters // 10, 3), 2, args.repeats)
        m.eval()
        gres = _timed({"list": gen(clips), "padded": gen(padded)}, 2, 1, args.repeats)
        _emit(args, dict(workload="whisper_audio_lens_model", profile=pname, lens=lens, B=B, T=T, d=512, H=8, layers="6+6",
                         dtype="bf16-autocast", ideal_self_fraction=round(sum(n * n for n in lens) / (B * T * T), 4),
                         ideal_cross_fraction=round(sum(lens) / (B * T), 4),
                         train_step_ms={r: round(statistics.median(x), 3) for r, x in res.items()},
                         train_step_ms_min={r: round(min(x), 3) for r, x in res.items()},
                         train_step_ms_max={r: round(max(x), 3) for r, x in res.items()},
                         generate_ms_per_token={r: round(statistics.median(x) / args.new_tokens, 4) for r, x in gres.items()},
                         generate_note="graph=True, encoder included, padded = the zero-padded tensor without lengths",
                         new_tokens=args.new_tokens, repeats=args.repeats))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["core", "model"], default="core")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new-tokens", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "whisper_audio_lens_bench.jsonl"))
    args = ap.parse_args()
    {"core": bench_core, "model": bench_model}[args.workload](args)
