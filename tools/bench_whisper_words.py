#!/usr/bin/env python3
"""WhisperMoP word timestamps (GPU box): one JSON line per measurement, appended to --out (default
profiles/whisper_words_bench.jsonl).

    python tools/bench_whisper_words.py                        # the two ops, and a transcribe window with and without word timestamps

Model and shapes: those of tools/bench_whisper_condition.py (d = 512, H = 8, 6 + 6 layers, n_audio_ctx 1500, n_text_ctx 448, vocab
51865, fp32 parameters under bf16 autocast, random weights; Whisper's multilingual ids, a sot sequence of 4 tokens), --new tokens
per window (default 64), B = 8.
Ops: ops.alignment_rows at R = 8 rows of 4 + --new columns, and ops.word_spans at R = 8 rows of N text tokens, N = --new and
N = 1024 (the kernel's limit: the rank-based median's O(K^2) compares at their largest, every fourth token beginning a word and
every token beginning one), each (a) called back to back (what transcribe pays per call: the launch and the Python around it),
(b) captured 100 times in one graph and replayed (the kernel's own time), (c) its torch twin.
Loop: with_logit_rules(rules).transcribe end to end on B = 8 clips of --windows x 1500 frames (default 4.0), without and with
word_timestamps=True (the table marks every third id as a word begin and a few residues as punctuation; median_word_frames 70),
timed with HIP events after a warm-up run; ms per window = total / sets of windows.  The two variants run as interleaved pairs,
--repeat times in one process: the eager loop is host-bound and spreads by several per cent between runs, so the record of the
second variant carries the difference against its own pair and the spread of the unconditioned runs seen so far.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_whisper_condition import _graph_us  # noqa: E402
from bench_whisper_transcribe import NMELS, RULES_EOS, RULES_TB, TA, TP, VOCAB, _emit, _events, _model_and_rules  # noqa: E402

B, NOTS = 8, 50363


def _word_rules():
    from mop_amd import ops
    ids = range(VOCAB)
    return ops.WordRules(VOCAB, [v for v in ids if v % 3 == 0 or v % 11 == 4], [v for v in ids if v % 11 == 4],
                         [v for v in ids if v % 11 == 7], [v for v in ids if v % 7 == 2], device="cuda")


def bench_ops(args):
    import torch
    from mop_amd import _lib, ops
    i32 = dict(dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(0)
    T = TP + args.new
    u = torch.rand(B, T, generator=g)
    tokens = torch.where(u < 0.3, RULES_TB + torch.randint(0, 100, (B, T), generator=g), torch.randint(0, RULES_EOS, (B, T), generator=g))
    tokens = tokens.to(**i32)
    n_take = torch.tensor([args.new, args.new // 2, 0, args.new, 3, args.new - 1, args.new, 9], **i32).clamp_max(args.new)
    sot = torch.randint(0, 1000, (TP,), generator=g).cuda()
    call = lambda: ops.alignment_rows(tokens, TP, n_take, sot, NOTS, RULES_EOS, torch.int32)                        # noqa: E731
    twin = lambda: ops.alignment_rows_torch(tokens, TP, n_take, sot, NOTS, RULES_EOS, torch.int32)                  # noqa: E731
    call()
    _emit(args, dict(workload="alignment_rows", R=B, T=T, T_p=TP, fused=ops.LAST_PATH["alignment_rows"] == _lib.PATH_FUSED,
                     op_call_us=round(_events(call, 2000, 50) * 1e3, 2), kernel_in_graph_us=round(_graph_us(call), 2),
                     torch_path_us=round(_events(twin, 200, 10) * 1e3, 2)))
    rules = _word_rules()
    every = ops.WordRules(VOCAB, torch.ones(VOCAB, dtype=torch.bool), device="cuda")
    for N, wr, name in ((args.new, rules, "residues"), (1024, rules, "residues"), (1024, every, "every token a word")):
        tok = torch.randint(0, RULES_EOS, (B, N), generator=g).to(**i32)
        times = torch.randint(0, 4, (B, N + 1), generator=g).cumsum(1).to(**i32)
        probs = torch.rand(B, N, generator=g).cuda()
        n_text = torch.full((B,), N, **i32)
        call = lambda: ops.word_spans(tok, times, probs, n_text, wr, 70)                                            # noqa: E731
        twin = lambda: ops.word_spans_torch(tok, times, probs, n_text, wr, 70)                                      # noqa: E731
        out = call()
        _emit(args, dict(workload="word_spans", R=B, N=N, table=name, words_per_row=round(float(out.n_words.float().mean()), 1),
                         fused=ops.LAST_PATH["word_spans"] == _lib.PATH_FUSED, op_call_us=round(_events(call, 2000, 50) * 1e3, 2),
                         kernel_in_graph_us=round(_graph_us(call), 2), torch_path_us=round(_events(twin, 200, 10) * 1e3, 2)))


def bench_loop(args):
    import torch
    from mop_amd import ops
    m, rules = _model_and_rules()
    d = m.with_logit_rules(rules)
    wr = _word_rules()
    torch.manual_seed(B)
    clips = [torch.randn(int(args.windows * TA), NMELS, device="cuda") for _ in range(B)]
    sot = torch.randint(0, 1000, (TP,), device="cuda")
    segments = ops.timestamp_segments
    sets = [0]

    def counted(*a, **k):                        # one call per set of windows
        sets[0] += 1
        return segments(*a, **k)

    base, seen = None, []
    for name, kw in (("plain", {}), ("word_timestamps", dict(word_timestamps=True, word_rules=wr, median_word_frames=70))) * args.repeat:
        out = {}

        def run():
            out["t"] = d.transcribe(clips, sot, args.new, **kw)

        ops.timestamp_segments = counted
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                sets[0] = 0
                run()                            # warm-up; it also counts the sets of windows of one run
                n_sets = sets[0]
                ms = _events(run, args.steps, 0)
        finally:
            ops.timestamp_segments = segments
        rec = dict(workload="whisper_transcribe_words", variant=name, B=B, frames=int(args.windows * TA), window=TA, T_s=TP,
                   new_tokens_per_window=args.new, dtype="bf16-autocast", window_sets=n_sets, total_ms=round(ms, 3),
                   ms_per_window=round(ms / n_sets, 3), steps=args.steps, warmup=1)
        if not kw:
            base = ms / n_sets
            seen.append(base)
        else:
            rec["words"] = [int(w.starts.numel()) for w in out["t"][1]]
            rec["ms_per_window_over_plain"] = round(ms / n_sets - base, 3)
            rec["plain_ms_per_window_spread"] = round(max(seen) - min(seen), 3)
        _emit(args, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3, help="the two loop variants run as this many interleaved pairs")
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--windows", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_words_bench.jsonl"))
    args = ap.parse_args()
    bench_ops(args)
    bench_loop(args)


if __name__ == "__main__":
    main()
