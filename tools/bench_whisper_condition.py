#!/usr/bin/env python3
"""WhisperMoP transcription conditioned on the previous text (GPU box): one JSON line per measurement, appended to --out
(default profiles/whisper_condition_bench.jsonl).

    python tools/bench_whisper_condition.py                    # the two ops, the prompt pass, and the loop with and without conditioning

Model: that of tools/bench_whisper_decode.py and tools/bench_whisper_transcribe.py (d = 512, H = 8, 6 + 6 layers, n_audio_ctx 1500,
n_text_ctx 448, vocab 51865, fp32 parameters under bf16 autocast, random weights; Whisper's multilingual ids, a sot sequence of 4
tokens), --new tokens per window (default 64), B = 8.
Ops, at B = 8 clips, n = 223 (n_text_ctx // 2 - 1), rows of 4 + --new columns, width 4 + 1 + 223: ops.prompt_history_update and
ops.window_prompts (a) called back to back (what transcribe pays per call: the launch and the Python around it), (b) captured 100
times in one graph and replayed (the kernel's own time), (c) their torch twins.
Prompt pass: the decoder over the prompt matrix alone, on a cache whose audio is already encoded: 4 columns (unconditioned), 228
columns as a uniform batch, 228 columns as a ragged batch with histories spread over [0, 223]; and, of the 228-column pass, the
final LayerNorm and vocabulary projection of every prompt column, which the decoders compute today and of which one or two
columns per row are read (their share of the pass is the record a later restriction of the projection starts from).
Loop: with_logit_rules(rules).transcribe end to end on B = 8 clips of --windows x 1500 frames (default 4.0), without conditioning
and with condition_on_previous_text=True at the default cap, timed with HIP events after a warm-up run; the number of windows and the
widths of the prompt matrices a run takes depend on the decoded timestamps and are reported with it; ms per window = total /
sets of windows.  The two variants alternate --repeat times in one process (the eager loop is host-bound and spreads by several
per cent between runs: read the difference against that spread).  The prompt pass record also holds the single-token step that
follows each prompt (the ragged batch runs ops.decode_attention_ragged in every later step).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_whisper_transcribe import NMELS, RULES_EOS, RULES_TB, TA, TP, _emit, _events, _model_and_rules  # noqa: E402

B, N_HIST, SOT_PREV = 8, 223, 50361


def _graph_us(call, copies=100):
    import torch
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        for _ in range(copies):
            call()
    return _events(g.replay, 50, 5) * 1e3 / copies


def bench_ops(args):
    import torch
    from mop_amd import _lib, ops
    i32 = dict(dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(0)
    hist = torch.randint(0, RULES_TB, (B, N_HIST), generator=g).to(**i32)
    hist_len = torch.tensor([0, 223, 100, 223, 17, 223, 160, 64], **i32)
    tokens = torch.randint(0, RULES_TB, (B, TP + args.new), generator=g).to(**i32)
    n_take = torch.tensor([args.new, args.new // 2, 0, args.new, 3, args.new - 1, args.new, 9], **i32).clamp_max(args.new)
    item = torch.arange(B, **i32)
    mode = torch.tensor([0, 0, 1, 0, 2, 0, 0, 0], **i32)
    sot = torch.randint(0, 1000, (TP,), generator=g).cuda()
    width = TP + 1 + N_HIST
    update = lambda: ops.prompt_history_update(hist, hist_len, tokens, TP, n_take, item, mode)                      # noqa: E731
    prompts = lambda: ops.window_prompts(hist, hist_len, item, sot, SOT_PREV, width)                                # noqa: E731
    twins = dict(prompt_history_update=lambda: ops.prompt_history_update_torch(hist, hist_len, tokens, TP, n_take, item, mode),
                 window_prompts=lambda: ops.window_prompts_torch(hist, hist_len, item, sot, SOT_PREV, width))
    for key, call in (("prompt_history_update", update), ("window_prompts", prompts)):
        call()
        fused = ops.LAST_PATH[key] == _lib.PATH_FUSED
        _emit(args, dict(workload=key, B=B, A=B, n=N_HIST, T=TP + args.new, T_s=TP, width=width, fused=fused,
                         op_call_us=round(_events(call, 2000, 50) * 1e3, 2), kernel_in_graph_us=round(_graph_us(call), 2),
                         torch_path_us=round(_events(twins[key], 200, 10) * 1e3, 2)))


def bench_prompt_pass(args):
    import torch
    from mop_amd import ops
    m, _ = _model_and_rules()
    torch.manual_seed(1)
    mel = torch.randn(B, TA, NMELS, device="cuda")
    width = TP + 1 + N_HIST
    i32 = dict(dtype=torch.int32, device="cuda")
    hist = torch.randint(0, RULES_TB, (B, N_HIST)).to(**i32)
    sot = torch.randint(0, 1000, (TP,), device="cuda")
    item = torch.arange(B, **i32)
    full = ops.window_prompts(hist, torch.full((B,), N_HIST, **i32), item, sot, SOT_PREV, width)
    spread = ops.window_prompts(hist, torch.tensor([223, 0, 100, 223, 17, 190, 160, 64], **i32), item, sot, SOT_PREV, width)
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        cache = m.init_decode_cache(m.encode(mel)[0], width + args.new)

        def prompt_pass(ids, kv_start):
            cache.length.zero_()
            cache.pos = 0
            cache.kv_start = kv_start
            return m.decode_step(cache, ids)

        one = torch.randint(0, 1000, (B, 1), device="cuda")

        def next_step(P):                        # the single-token decoder step that follows a prompt of P columns
            cache.length.fill_(P)
            cache.pos = P
            return m.decode_step(cache, one)

        ms = {}
        for name, ids, ks in (("bare_4_columns", sot.unsqueeze(0).expand(B, -1).contiguous(), None),
                              ("uniform_228_columns", full.ids, None), ("ragged_228_columns", spread.ids, spread.kv_start)):
            ms[name] = _events(lambda: prompt_pass(ids, ks), 50, 5)
            ms["step_after_" + name] = _events(lambda: next_step(ids.shape[1]), 200, 10)
        x = torch.randn(B, width, m.cfg.n_embd, device="cuda")
        ms["projection_of_228_columns"] = _events(lambda: m.lm_head(m.dec_ln_f(x)), 50, 5)
        ms["projection_of_1_column"] = _events(lambda: m.lm_head(m.dec_ln_f(x[:, -1:])), 50, 5)
    _emit(args, dict(workload="whisper_prompt_pass", B=B, T_s=TP, n=N_HIST, width=width, dtype="bf16-autocast",
                     ms={k: round(v, 3) for k, v in ms.items()},
                     projection_share_of_uniform_pass=round(ms["projection_of_228_columns"] / ms["uniform_228_columns"], 3)))
    return ms


def bench_loop(args, pass_ms):
    import torch
    from mop_amd import ops
    m, rules = _model_and_rules()
    d = m.with_logit_rules(rules)
    torch.manual_seed(B)
    clips = [torch.randn(int(args.windows * TA), NMELS, device="cuda") for _ in range(B)]
    sot = torch.randint(0, 1000, (TP,), device="cuda")
    segments, prompts = ops.timestamp_segments, ops.window_prompts
    sets, widths = [0], []

    def counted(*a, **k):                        # one call per set of windows
        sets[0] += 1
        return segments(*a, **k)

    def recorded(*a, **k):
        widths.append(a[5])
        return prompts(*a, **k)

    base = None
    for name, kw in (("unconditioned", {}), ("conditioned", dict(condition_on_previous_text=True, sot_prev_token_id=SOT_PREV))) * args.repeat:
        out = {}

        def run():
            out["t"] = d.transcribe(clips, sot, args.new, **kw)

        ops.timestamp_segments, ops.window_prompts = counted, recorded
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                sets[0] = 0
                del widths[:]
                run()                            # warm-up; it also counts the sets of windows of one run
                n_sets, w = sets[0], list(widths)
                ms = _events(run, args.steps, 0)
        finally:
            ops.timestamp_segments, ops.window_prompts = segments, prompts
        rec = dict(workload="whisper_transcribe_condition", variant=name, B=B, frames=int(args.windows * TA), window=TA, T_s=TP,
                   new_tokens_per_window=args.new, n=N_HIST if kw else 0, dtype="bf16-autocast", window_sets=n_sets, prompt_widths=w,
                   tokens=[int(t.tokens.numel()) for t in out["t"]], total_ms=round(ms, 3), ms_per_window=round(ms / n_sets, 3),
                   steps=args.steps, warmup=1)
        if not kw:
            base = ms / n_sets
        else:
            rec["ms_per_window_over_unconditioned"] = round(ms / n_sets - base, 3)
            rec["prompt_pass_ms_at_full_width_minus_bare"] = round(pass_ms["uniform_228_columns"] - pass_ms["bare_4_columns"], 3)
        _emit(args, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3, help="the two loop variants alternate this many times")
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--windows", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_condition_bench.jsonl"))
    args = ap.parse_args()
    bench_ops(args)
    bench_loop(args, bench_prompt_pass(args))


if __name__ == "__main__":
    main()
