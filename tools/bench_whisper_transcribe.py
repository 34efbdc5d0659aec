#!/usr/bin/env python3
"""Long-form WhisperMoP transcription benchmark (GPU box): one JSON line per measurement, appended to --out
(default profiles/whisper_transcribe_bench.jsonl).

    python tools/bench_whisper_transcribe.py                       # the loop, B in {1, 8}, eager and graph=True
    python tools/bench_whisper_transcribe.py --workload segments   # the segment parse alone: HIP launch against the host parse

Model: d = 512, H = 8, 6 + 6 layers, n_audio_ctx 1500, vocab 51865 (Whisper-base-like, the model of tools/bench_whisper_decode.py),
fp32 parameters under bf16 autocast, random weights; Whisper's multilingual ids (timestamps from 50364, eot 50257), a prompt of 4
tokens, --new tokens per window (default 64), clips of --windows x 1500 frames (default 3.2: several windows, the last one short).
Loop: WhisperMoP.transcribe end to end (encoder, decoder steps, segment kernel and the one copy per window), timed with HIP events
after a warm-up run; the number of windows a run takes depends on the decoded timestamps and is reported with it; ms per window =
total / windows.  Segments: on the rows one window's decode produced, (a) ops.timestamp_segments called back to back (what a caller
pays per call: the launch plus the Python around it), (b) the same launch captured 100 times in one graph and replayed (the
kernel's own time, launch overhead excluded as far as a graph excludes it), (c) ops.timestamp_segments_torch, (d) the host parse a
caller would write without the op: tokens.tolist() (a synchronising copy) and the per-row Python loop of
tests/test_whisper_transcribe_cpu.py (ref_row), timed with perf_counter after a device synchronise.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

TA, D, H, LAYERS, VOCAB, NMELS, TP = 1500, 512, 8, 6, 51865, 80, 4
RULES_TB, RULES_EOS = 50364, 50257


def _emit(args, rec):
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _events(fn, steps, warmup):
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


def _model_and_rules():
    import torch
    from mop_amd.nn import LogitRules, WhisperConfig, WhisperMoP
    cfg = WhisperConfig(n_mels=NMELS, n_audio_ctx=TA, vocab_size=VOCAB, n_text_ctx=448, n_embd=D, n_head=H, n_layer_enc=LAYERS,
                        n_layer_dec=LAYERS)
    torch.manual_seed(0)
    m = WhisperMoP(cfg).cuda().eval()
    never = list(range(1, 1000, 12)) + [i for i in range(50258, RULES_TB - 1) if i != 50363]
    rules = LogitRules(VOCAB, suppress_tokens=never, suppress_at_begin=[220, RULES_EOS], timestamp_begin=RULES_TB,
                       eos_token_id=RULES_EOS, no_timestamps_token_id=50363, max_initial_timestamp_index=50, device="cuda")
    return m, rules


def bench_loop(args):
    import torch
    from mop_amd import ops
    m, rules = _model_and_rules()
    frames = int(args.windows * TA)
    windows = [0]
    segments = ops.timestamp_segments

    def counted(*a, **k):                        # one call per window
        windows[0] += 1
        return segments(*a, **k)

    for B in args.batch:
        torch.manual_seed(B)
        clips = [torch.randn(frames - 97 * b, NMELS, device="cuda") for b in range(B)]
        prompt = torch.randint(0, 1000, (TP,), device="cuda")
        for graph in (False, True):
            out = {}

            def run():
                out["t"] = m.transcribe(clips, prompt, rules, args.new, graph=graph)

            ops.timestamp_segments = counted
            try:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    windows[0] = 0
                    run()                        # warm-up; it also counts the windows of one run
                    n_win = windows[0]
                    print(f"B={B} graph={graph}: {n_win} windows per run", flush=True)
                    ms = _events(run, args.steps, 0)
            finally:
                ops.timestamp_segments = segments
            _emit(args, dict(workload="whisper_transcribe", variant="graph" if graph else "eager", B=B, frames=[int(c.shape[0]) for c in clips],
                             window=TA, T_p=TP, new_tokens_per_window=args.new, d=D, H=H, layers="6+6", vocab=VOCAB,
                             dtype="bf16-autocast", windows=n_win, segments=[int(t.starts.numel()) for t in out["t"]],
                             total_ms=round(ms, 3), ms_per_window=round(ms / n_win, 3), steps=args.steps, warmup=1))


def bench_segments(args):
    import torch
    from mop_amd import _lib, ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_whisper_transcribe_cpu import ref_row
    m, rules = _model_and_rules()
    for B in args.batch:
        torch.manual_seed(B)
        mel = torch.randn(B, TA, NMELS, device="cuda")
        prompt = torch.randint(0, 1000, (B, TP), device="cuda")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            rows = m.with_logit_rules(rules).generate(mel, prompt, args.new, RULES_EOS, graph=True).to(torch.int32)
        win = torch.full((B,), TA, dtype=torch.int32, device="cuda")
        call = lambda: ops.timestamp_segments(rows, TP, win, RULES_TB, RULES_EOS)                     # noqa: E731
        got = call()
        fused = ops.LAST_PATH["timestamp_segments"] == _lib.PATH_FUSED
        op_us = _events(call, 2000, 50) * 1e3
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            for _ in range(100):
                call()
        graph_us = _events(g.replay, 50, 5) * 1e3 / 100
        torch_us = _events(lambda: ops.timestamp_segments_torch(rows, TP, win, RULES_TB, RULES_EOS), 200, 10) * 1e3

        def host():
            return [ref_row(r, TP, TA, RULES_TB, RULES_EOS, 1) for r in rows.tolist()]

        want = host()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            host()
        host_us = (time.perf_counter() - t0) / 200 * 1e6
        agree = got.advance.tolist() == [w[1] for w in want] and got.n_segments.tolist() == [len(w[0]) for w in want]
        _emit(args, dict(workload="timestamp_segments", B=B, T=TP + args.new, S=args.new, fused=fused, op_call_us=round(op_us, 2),
                         kernel_in_graph_us=round(graph_us, 2), torch_path_us=round(torch_us, 2), host_parse_us=round(host_us, 2),
                         kernel_equals_host_parse=agree, n_segments=got.n_segments.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["loop", "segments"], default="loop")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--windows", type=float, default=3.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_transcribe_bench.jsonl"))
    args = ap.parse_args()
    {"loop": bench_loop, "segments": bench_segments}[args.workload](args)


if __name__ == "__main__":
    main()
