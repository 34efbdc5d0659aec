#!/usr/bin/env python3
"""KV-cached WhisperMoP decoding benchmark (GPU box): one JSON line per measurement, appended to --out
(default profiles/whisper_decode_bench.jsonl).

    python tools/bench_whisper_decode.py --workload generate   # per-token latency: naive re-decode, cached eager, cached + graph
    python tools/bench_whisper_decode.py --workload core       # the decode attention core vs ops.sdpa_core (N = 1) and torch SDPA
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_whisper_decode.py --workload core-trace
    python tools/bench_whisper_decode.py --stats DIR/<host>/<pid>_kernel_stats.csv   # decode kernels against the byte bound
    python tools/bench_whisper_decode.py --workload beam --out profiles/whisper_beam_bench.jsonl   # beam search, K = 5
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_whisper_decode.py --workload beam-trace
    python tools/bench_whisper_decode.py --workload sample --out profiles/whisper_sample_bench.jsonl   # sampling against greedy
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_whisper_decode.py --workload sample-trace
    python tools/bench_whisper_decode.py --workload ragged --batch 8 --out profiles/whisper_ragged_bench.jsonl   # ragged prompts
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_whisper_decode.py --workload ragged-trace
    python tools/bench_whisper_decode.py --workload rules --out profiles/whisper_rules_bench.jsonl   # Whisper's logit rules
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_whisper_decode.py --workload rules-trace

Model: d = 512, H = 8, 6 + 6 layers, T_a = 1500, vocab 51865 (Whisper-base-like), fp32 parameters under bf16 autocast, prompt 4,
220 new tokens, B in {1, 8}.  Variants: (a) naive: decode(enc, whole prefix) per token; (b) cached eager: generate(); (c) cached +
graph: generate(graph=True).  Each variant is timed end to end (encoder included) with HIP events after a warm-up run; per-token
latency = time / new tokens.  Core: B = 8, H = 8, dk = 64, Tq = 1, Nk in {448, 1500}, bf16.  Byte bound: K and V are read once,
2 B Nk H dk 2 bytes, at 6.3 TB/s (the MI355X's achievable HBM rate); a kernel faster than that bound was served from the 256 MiB
Infinity Cache (the same 2-12 MB cache is read by every timed call).
Beam: K = 5, B in {1, 8}, same model, prompt and length.  Variants: (a) torch_beam: the same search composed of torch ops
(log_softmax + topk over K * V + an index_select of every layer's self-attention cache by parent beam, cross cache repeated K times,
no eos); (b) beam_search eager; (c) beam_search(graph=True).  beam-trace runs (b) at B = 8 for rocprofv3; --stats then also prints
the beam kernels (bs_*) and the row-indirect attention (da_* with ROWS) next to their byte bounds: B K V 2 bytes of bf16 logits per
step, and 2 B K L H dk 2 + 4 B K L bytes of K, V and row table per layer and step at the mean length L = T_p + 110.
Sample: temperature 0.7, top_k 50, top_p 0.95, n in {1, 5} samples per item, B in {1, 8}, same model, prompt and length.  Variants:
(a) generate(graph=True), the greedy baseline; (b) sample eager; (c) sample(graph=True).  sample-trace runs (c) at B = 8, n = 1 and
n = 5 for rocprofv3; --stats then also prints the sampling kernel (sp_row_kernel).
Ragged: generate on B prompts of lengths spread over 1 ... 64 (a list: left-padded in one cache, WhisperDecodeCache.kv_start) against a
uniform (B, 64) prompt, same model and length, eager and graph=True.  ragged-trace runs both with graphs at B = 8 for rocprofv3, so
the ragged split kernel (da_split_kernel<..., START = true>) can be compared with the plain one (START = false) at the same shape.
Rules: generate(graph=True) on the same model, prompt and length, B in {1, 8}: (a) no_rules; (b) rules_hip: with_logit_rules (Whisper's
multilingual ids: timestamps from 50364, eot 50257, 88 suppressed ids) on the HIP kernel; (c) rules_torch: the same with
ops.logit_rules forced onto ops.logit_rules_torch.  rules-trace runs (b) at B = 8 for rocprofv3; --stats then also prints the rules
kernel (lr_row_kernel) next to the time to stream one bf16 row twice at the HBM rate.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

TA, D, H, LAYERS, VOCAB, NMELS, TP, NEW = 1500, 512, 8, 6, 51865, 80, 4, 220
HBM_BPS = 6.3e12


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


def _emit(args, rec):
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def bench_generate(args):
    import torch
    from mop_amd.nn import WhisperConfig, WhisperMoP
    cfg = WhisperConfig(n_mels=NMELS, n_audio_ctx=TA, vocab_size=VOCAB, n_text_ctx=448, n_embd=D, n_head=H, n_layer_enc=LAYERS,
                        n_layer_dec=LAYERS)
    torch.manual_seed(0)
    m = WhisperMoP(cfg).cuda().eval()
    for B in args.batch:
        mel = torch.randn(B, TA, NMELS, device="cuda")
        prompt = torch.randint(0, VOCAB, (B, TP), device="cuda")

        @torch.no_grad()
        def naive():
            enc, _ = m.encode(mel)
            cur = prompt
            for _ in range(NEW):
                cur = torch.cat([cur, m.decode(enc, cur)[:, -1].argmax(-1, keepdim=True)], dim=1)
            return cur

        outs = {}
        for name, fn in (("naive", naive), ("cached", lambda: m.generate(mel, prompt, NEW)),
                         ("cached_graph", lambda: m.generate(mel, prompt, NEW, graph=True))):
            if name == "naive" and args.skip_naive:
                continue
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ms = _time(lambda: outs.__setitem__(name, fn()), args.steps, args.warmup)
            _emit(args, dict(workload="whisper_generate", variant=name, B=B, T_a=TA, T_p=TP, new_tokens=NEW, d=D, H=H, layers="6+6",
                             vocab=VOCAB, dtype="bf16-autocast", total_ms=round(ms, 3), ms_per_token=round(ms / NEW, 4),
                             tokens_per_s=round(B * NEW / ms * 1e3, 1), steps=args.steps, warmup=args.warmup))
        if "naive" in outs:
            agree = (outs["naive"] == outs["cached"]).all(1).float().mean().item()
            _emit(args, dict(workload="whisper_generate_agreement", B=B, rows_equal_naive_vs_cached=agree,
                             graph_equals_eager=bool(torch.equal(outs["cached"], outs["cached_graph"]))))


def _base_model():
    import torch
    from mop_amd.nn import WhisperConfig, WhisperMoP
    cfg = WhisperConfig(n_mels=NMELS, n_audio_ctx=TA, vocab_size=VOCAB, n_text_ctx=448, n_embd=D, n_head=H, n_layer_enc=LAYERS,
                        n_layer_dec=LAYERS)
    torch.manual_seed(0)
    return WhisperMoP(cfg).cuda().eval()


@__import__("torch").no_grad()
def torch_beam(m, mel, prompt, K, n_new):
    """the beam search of WhisperMoP.beam_search (without eos) composed of torch ops: log_softmax + topk, and every layer's
    self-attention cache copied by parent beam (index_select) at every step"""
    import torch
    B, V = prompt.shape[0], m.cfg.vocab_size
    enc, _ = m.encode(mel)
    cache = m.init_decode_cache(enc.repeat_interleave(K, 0), prompt.shape[1] + n_new)
    hist = prompt.repeat_interleave(K, 0)
    logits = m.decode_step(cache, hist)[:, -1]
    scores = torch.zeros(B, K, device=mel.device)
    scores[:, 1:] = float("-inf")
    base = (torch.arange(B, device=mel.device) * K).unsqueeze(1)
    for t in range(n_new):
        cand = (torch.log_softmax(logits.float(), -1).view(B, K, V) + scores.unsqueeze(2)).view(B, K * V)
        scores, idx = cand.topk(K, dim=1)
        sel = (base + idx // V).view(-1)
        tok = (idx % V).view(-1, 1)
        hist = torch.cat([hist.index_select(0, sel), tok], dim=1)
        if t == n_new - 1:
            break
        for l in range(len(cache.self_k)):
            cache.self_k[l] = cache.self_k[l].index_select(0, sel)
            cache.self_v[l] = cache.self_v[l].index_select(0, sel)
        logits = m.decode_step(cache, tok)[:, -1]
    return hist.view(B, K, -1)[:, 0], scores[:, 0] / n_new


def bench_beam(args):
    import torch
    m = _base_model()
    K = 5
    for B in args.batch:
        mel = torch.randn(B, TA, NMELS, device="cuda")
        prompt = torch.randint(0, VOCAB, (B, TP), device="cuda")
        outs = {}
        for name, fn in (("torch_beam", lambda: torch_beam(m, mel, prompt, K, NEW)),
                         ("beam_search", lambda: m.beam_search(mel, prompt, NEW, K)),
                         ("beam_search_graph", lambda: m.beam_search(mel, prompt, NEW, K, graph=True))):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ms = _time(lambda: outs.__setitem__(name, fn()), args.steps, args.warmup)
            _emit(args, dict(workload="whisper_beam", variant=name, K=K, B=B, T_a=TA, T_p=TP, new_tokens=NEW, d=D, H=H, layers="6+6",
                             vocab=VOCAB, dtype="bf16-autocast", total_ms=round(ms, 3), ms_per_token=round(ms / NEW, 4),
                             steps=args.steps, warmup=args.warmup))
        _emit(args, dict(workload="whisper_beam_agreement", K=K, B=B,
                         rows_equal_torch_vs_kernels=(outs["torch_beam"][0] == outs["beam_search"][0]).all(1).float().mean().item(),
                         graph_equals_eager=bool(torch.equal(outs["beam_search"][0], outs["beam_search_graph"][0]))))


def bench_beam_trace(args):
    import torch
    m = _base_model()
    mel = torch.randn(8, TA, NMELS, device="cuda")
    prompt = torch.randint(0, VOCAB, (8, TP), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(2):
            m.beam_search(mel, prompt, NEW, 5)
    torch.cuda.synchronize()


SAMPLE_CFG = dict(temperature=0.7, top_k=50, top_p=0.95)


def bench_sample(args):
    import torch
    m = _base_model()
    for B in args.batch:
        mel = torch.randn(B, TA, NMELS, device="cuda")
        prompt = torch.randint(0, VOCAB, (B, TP), device="cuda")
        for n in (1, 5):
            outs = {}
            for name, fn in (("generate_graph", lambda: m.generate(mel, prompt, NEW, graph=True)),
                             ("sample", lambda: m.sample(mel, prompt, NEW, num_samples=n, **SAMPLE_CFG)),
                             ("sample_graph", lambda: m.sample(mel, prompt, NEW, num_samples=n, graph=True, **SAMPLE_CFG))):
                if name == "generate_graph" and n != 1:
                    continue
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    ms = _time(lambda: outs.__setitem__(name, fn()), args.steps, args.warmup)
                _emit(args, dict(workload="whisper_sample", variant=name, n=n, B=B, T_a=TA, T_p=TP, new_tokens=NEW, d=D, H=H,
                                 layers="6+6", vocab=VOCAB, dtype="bf16-autocast", **SAMPLE_CFG, total_ms=round(ms, 3),
                                 ms_per_token=round(ms / NEW, 4), steps=args.steps, warmup=args.warmup))
            _emit(args, dict(workload="whisper_sample_agreement", n=n, B=B,
                             graph_equals_eager=bool(torch.equal(outs["sample"][0], outs["sample_graph"][0]) and
                                                     torch.equal(outs["sample"][1], outs["sample_graph"][1]))))


def bench_sample_trace(args):
    import torch
    m = _base_model()
    mel = torch.randn(8, TA, NMELS, device="cuda")
    prompt = torch.randint(0, VOCAB, (8, TP), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for n in (1, 5):
            for _ in range(2):
                m.sample(mel, prompt, NEW, num_samples=n, graph=True, **SAMPLE_CFG)
    torch.cuda.synchronize()


def _core_inputs(Nk):
    import torch
    B = 8
    q = torch.randn(B, 1, H, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Nk, H, 64, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Nk, H, 64, device="cuda", dtype=torch.bfloat16)
    return q, k, v


def _core_impls(q, k, v):
    import torch
    import torch.nn.functional as F
    from mop_amd import ops
    kv_len = torch.tensor([k.shape[1]], dtype=torch.int32, device="cuda")
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    return {"decode_attention": lambda: ops.decode_attention(q, k, v, kv_len=kv_len),
            "sdpa_core_n1": lambda: ops.sdpa_core(q, k, v),
            "torch_sdpa": lambda: F.scaled_dot_product_attention(qt, kt, vt)}


def bench_core(args):
    import torch
    for Nk in (448, 1500):
        q, k, v = _core_inputs(Nk)
        bound_us = 2 * q.shape[0] * Nk * H * 64 * 2 / HBM_BPS * 1e6
        with torch.no_grad():
            for name, fn in _core_impls(q, k, v).items():
                ms = _time(fn, args.steps * 20, args.warmup * 5)
                _emit(args, dict(workload="decode_attention_core", impl=name, B=8, H=H, Tq=1, Nk=Nk, dk=64, dtype="bf16",
                                 us=round(ms * 1e3, 2), hbm_byte_bound_us=round(bound_us, 2), steps=args.steps * 20))


RAGGED_P = 64


def _ragged_prompts(B):
    """B prompt lengths spread evenly over 1 ... RAGGED_P (B = 1: RAGGED_P)"""
    import torch
    lens = [RAGGED_P] if B == 1 else [1 + (RAGGED_P - 1) * b // (B - 1) for b in range(B)]
    return [torch.randint(0, VOCAB, (n,), device="cuda") for n in lens], lens


def bench_ragged(args):
    import torch
    m = _base_model()
    for B in args.batch:
        mel = torch.randn(B, TA, NMELS, device="cuda")
        ragged, lens = _ragged_prompts(B)
        uniform = torch.randint(0, VOCAB, (B, RAGGED_P), device="cuda")
        outs = {}
        for name, prompt, graph in (("uniform", uniform, False), ("uniform_graph", uniform, True), ("ragged", ragged, False),
                                    ("ragged_graph", ragged, True)):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ms = _time(lambda: outs.__setitem__(name, m.generate(mel, prompt, NEW, graph=graph)), args.steps, args.warmup)
            _emit(args, dict(workload="whisper_ragged", variant=name, B=B, T_a=TA, prompt_lens=lens if "ragged" in name else
                             [RAGGED_P] * B, new_tokens=NEW, d=D, H=H, layers="6+6", vocab=VOCAB, dtype="bf16-autocast",
                             total_ms=round(ms, 3), ms_per_token=round(ms / NEW, 4), steps=args.steps, warmup=args.warmup))
        _emit(args, dict(workload="whisper_ragged_agreement", B=B,
                         graph_equals_eager=all(torch.equal(a, b) for a, b in zip(outs["ragged"], outs["ragged_graph"]))))


def bench_ragged_trace(args):
    import torch
    m = _base_model()
    mel = torch.randn(8, TA, NMELS, device="cuda")
    ragged, _ = _ragged_prompts(8)
    uniform = torch.randint(0, VOCAB, (8, RAGGED_P), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for prompt in (uniform, ragged):
            for _ in range(2):
                m.generate(mel, prompt, NEW, graph=True)
    torch.cuda.synchronize()


RULES_TB, RULES_EOS = 50364, 50257


def _whisper_rules():
    """a rule set of Whisper's size: timestamps from 50364, eot 50257, the specials 50258 ... 50363 and 88 - 106 other ids never
    emitted, blank (220) and eot blocked at the first position, a first timestamp of at most 1 s (index 50)"""
    from mop_amd.nn import LogitRules
    never = list(range(1, 1000, 12)) + [i for i in range(50258, RULES_TB - 1) if i != 50363]
    return LogitRules(VOCAB, suppress_tokens=never, suppress_at_begin=[220, RULES_EOS], timestamp_begin=RULES_TB,
                      eos_token_id=RULES_EOS, no_timestamps_token_id=50363, max_initial_timestamp_index=50, device="cuda")


def bench_rules(args):
    import torch
    from mop_amd import ops
    m = _base_model()
    d = m.with_logit_rules(_whisper_rules())
    hip = ops.logit_rules
    for B in args.batch:
        mel = torch.randn(B, TA, NMELS, device="cuda")
        prompt = torch.randint(0, RULES_EOS, (B, TP), device="cuda")
        outs = {}
        for name, fn, op in (("no_rules", lambda: m.generate(mel, prompt, NEW, graph=True), hip),
                             ("rules_hip", lambda: d.generate(mel, prompt, NEW, graph=True), hip),
                             ("rules_torch", lambda: d.generate(mel, prompt, NEW, graph=True), ops.logit_rules_torch)):
            ops.logit_rules = op
            try:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    ms = _time(lambda: outs.__setitem__(name, fn()), args.steps, args.warmup)
            finally:
                ops.logit_rules = hip
            _emit(args, dict(workload="whisper_rules", variant=name, B=B, T_a=TA, T_p=TP, new_tokens=NEW, d=D, H=H, layers="6+6",
                             vocab=VOCAB, dtype="bf16-autocast", total_ms=round(ms, 3), ms_per_token=round(ms / NEW, 4),
                             steps=args.steps, warmup=args.warmup))
        stamps = (outs["rules_hip"][:, TP:] >= RULES_TB).float().mean().item()
        _emit(args, dict(workload="whisper_rules_agreement", B=B, timestamp_share=round(stamps, 3),
                         rows_equal_hip_vs_torch=(outs["rules_hip"] == outs["rules_torch"]).all(1).float().mean().item()))


def bench_rules_trace(args):
    import torch
    m = _base_model()
    d = m.with_logit_rules(_whisper_rules())
    mel = torch.randn(8, TA, NMELS, device="cuda")
    prompt = torch.randint(0, RULES_EOS, (8, TP), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(2):
            d.generate(mel, prompt, NEW)
    torch.cuda.synchronize()


def bench_core_trace(args):
    import torch
    with torch.no_grad():
        for Nk in (448, 1500):
            q, k, v = _core_inputs(Nk)
            for fn in _core_impls(q, k, v).values():
                for _ in range(50):
                    fn()
    torch.cuda.synchronize()


def stats(path):
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        if "da_" in r["Name"] or "sdpa" in r["Name"] or "attention" in r["Name"].lower() or "fmha" in r["Name"].lower() \
                or "bs_" in r["Name"] or "sp_row" in r["Name"] or "lr_row" in r["Name"]:
            print(f"{float(r['AverageNs']) / 1e3:9.2f} us  x{r['Calls']:>5}  {r['Name'][:150]}")
    B, K, L = 8, 5, TP + NEW // 2
    print(f"beam bounds at B = {B}, K = {K}: logits {B * K * VOCAB * 2 / HBM_BPS * 1e6:.2f} us; row-indirect attention per layer at "
          f"L = {L}: {(2 * B * K * L * H * 64 * 2 + 4 * B * K * L) / HBM_BPS * 1e6:.2f} us")
    print(f"logit rules: one bf16 row of {VOCAB} streamed twice (read + write) at the HBM rate: {2 * VOCAB * 2 / HBM_BPS * 1e6:.3f} us; "
          f"{B} rows: {B * 2 * VOCAB * 2 / HBM_BPS * 1e6:.3f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["generate", "core", "core-trace", "beam", "beam-trace", "sample", "sample-trace",
                                           "ragged", "ragged-trace", "rules", "rules-trace"], default="generate")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-naive", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "whisper_decode_bench.jsonl"))
    ap.add_argument("--stats")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)
    {"generate": bench_generate, "core": bench_core, "core-trace": bench_core_trace, "beam": bench_beam,
     "beam-trace": bench_beam_trace, "sample": bench_sample, "sample-trace": bench_sample_trace, "ragged": bench_ragged,
     "ragged-trace": bench_ragged_trace, "rules": bench_rules, "rules-trace": bench_rules_trace}[args.workload](args)


if __name__ == "__main__":
    main()
