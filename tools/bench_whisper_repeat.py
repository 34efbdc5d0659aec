#!/usr/bin/env python3
"""WhisperMoP decoding under repeat rules (GPU box): one JSON line per measurement, appended to --out (default
profiles/whisper_repeat_bench.jsonl).

    python tools/bench_whisper_repeat.py                       # the op against its torch twin, then generate with and without it

Op: ops.repeat_rules in place (out = logits, what the decoders call) at R = 8 rows, V = 51865, n = 64 and n = 440 generated tokens
drawn from 40 ids (so n-grams do repeat), penalty 1.1 and trigram blocking with Whisper's exemptions, fp32 and bf16: (a) called
back to back (what an eager step pays: the launch and the Python around it), (b) captured 100 times in one graph and replayed (the
kernel's own time), (c) ops.repeat_rules_torch on the same tensors.
Decoding: with_logit_rules(rules[, repeat_rules]).generate(graph=True) on the model of tools/bench_whisper_decode.py (d = 512,
H = 8, 6 + 6 layers, n_audio_ctx 1500, vocab 51865, fp32 parameters under bf16 autocast, random weights), B = 8, a prompt of 4 and
--new tokens (default 220), under the same Whisper-sized LogitRules in every variant: (a) no repeat rules, (b) neutral repeat
rules, which run the same code as (a), (c) penalty 1.1 plus trigram blocking.  The three alternate --repeat times in one process,
each timed end to end (encoder included) with HIP events after a warm-up run; the last record holds the means and, per pair,
the differences (b) - (a) and (c) - (a): read (b) - (a) as the spread of the measurement, it is no cost.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_whisper_condition import _graph_us  # noqa: E402
from bench_whisper_transcribe import NMELS, RULES_EOS, RULES_TB, TA, TP, VOCAB, _emit, _events, _model_and_rules  # noqa: E402

R, T0 = 8, 4


def bench_op(args, lr):
    import torch
    from mop_amd import _lib, ops
    rules = ops.RepeatRules.for_whisper(lr, repetition_penalty=1.1, no_repeat_ngram_size=3)
    rules.table("cuda")
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.bfloat16, torch.float32):
        for n in (64, 440):
            x = torch.randn(R, VOCAB, generator=g).to(dtype).cuda()
            hist = (torch.randint(0, 40, (R, T0 + n), generator=g) * 997 % RULES_EOS).to(torch.int32).cuda()
            pos = torch.tensor([T0 + n], dtype=torch.int32, device="cuda")
            call = lambda: ops.repeat_rules(x, hist, pos, T0, rules, out=x)                                       # noqa: E731
            twin = lambda: ops.repeat_rules_torch(x, hist, pos, T0, rules, out=x)                                 # noqa: E731
            call()
            _emit(args, dict(workload="repeat_rules", R=R, V=VOCAB, n=n, T0=T0, dtype=str(dtype).split(".")[1], in_place=True,
                             penalty=1.1, ngram=3, fused=ops.LAST_PATH["repeat_rules"] == _lib.PATH_FUSED,
                             op_call_us=round(_events(call, 2000, 50) * 1e3, 2), kernel_in_graph_us=round(_graph_us(call), 2),
                             torch_path_us=round(_events(twin, 200, 10) * 1e3, 2)))


def bench_generate(args, m, lr):
    import torch
    from mop_amd import ops
    variants = (("no_repeat_rules", None), ("neutral_repeat_rules", ops.RepeatRules.for_whisper(lr)),
                ("penalty_1.1_trigram", ops.RepeatRules.for_whisper(lr, repetition_penalty=1.1, no_repeat_ngram_size=3)))
    torch.manual_seed(1)
    mel = torch.randn(R, TA, NMELS, device="cuda")
    prompt = torch.randint(0, RULES_EOS, (R, TP), device="cuda")
    ms, outs = {name: [] for name, _ in variants}, {}
    for rep in range(args.repeat):
        for name, rr in variants:
            d = m.with_logit_rules(lr, rr)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                t = _events(lambda: outs.__setitem__(name, d.generate(mel, prompt, args.new, graph=True)), args.steps, args.warmup)
            ms[name].append(t)
            _emit(args, dict(workload="whisper_generate_repeat", variant=name, pair=rep, B=R, T_a=TA, T_p=TP, new_tokens=args.new,
                             vocab=VOCAB, dtype="bf16-autocast", graph=True, total_ms=round(t, 3), ms_per_token=round(t / args.new, 4),
                             steps=args.steps, warmup=args.warmup))
    base = ms["no_repeat_rules"]
    per_token = lambda name: [round((a - b) / args.new, 4) for a, b in zip(ms[name], base)]                       # noqa: E731

    def trigrams(rows):                          # rows whose generated tokens repeat a trigram that ends in a text token
        hit = 0
        for row in rows[:, TP:].tolist():
            seen = set()
            grams = [g for g in zip(row, row[1:], row[2:]) if g[2] < RULES_TB and g[2] != RULES_EOS]
            hit += any(g in seen or seen.add(g) for g in grams)
        return hit

    _emit(args, dict(workload="whisper_generate_repeat_summary", B=R, new_tokens=args.new, pairs=args.repeat,
                     mean_ms_per_token={k: round(sum(v) / len(v) / args.new, 4) for k, v in ms.items()},
                     neutral_minus_none_ms_per_token=per_token("neutral_repeat_rules"),
                     rules_minus_none_ms_per_token=per_token("penalty_1.1_trigram"),
                     neutral_equals_none=bool(torch.equal(outs["neutral_repeat_rules"], outs["no_repeat_rules"])),
                     rows_with_a_repeated_trigram={k: trigrams(v) for k, v in outs.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=4, help="the three generate variants alternate this many times")
    ap.add_argument("--new", type=int, default=220)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_repeat_bench.jsonl"))
    args = ap.parse_args()
    m, lr = _model_and_rules()
    bench_op(args, lr)
    bench_generate(args, m, lr)


if __name__ == "__main__":
    main()
