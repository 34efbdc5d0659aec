#!/usr/bin/env python3
"""WhisperMoP language detection (GPU box): one JSON line per measurement, appended to --out (default
profiles/whisper_language_bench.jsonl).

    python tools/bench_whisper_language.py                     # the op against its torch twin, then detect_language end to end

Op: ops.language_probs into static result buffers at R = 8 rows, V = 51865, n = 99 languages (Whisper's multilingual vocabulary:
the ids behind <|startoftranscript|> = 50258), bf16 and fp32: (a) called back to back (what an eager caller pays: the launch and
the Python around it), (b) captured 100 times in one graph and replayed (the kernel's own time), (c) ops.language_probs_torch on
the same tensors, (d) the twin captured and replayed the same way (its kernels without their Python).
Detection: detect_language on the model of tools/bench_whisper_decode.py (d = 512, H = 8, 6 + 6 layers, n_audio_ctx 1500, vocab
51865, fp32 parameters under bf16 autocast, random weights), B = 8 clips of 1500 frames, sot_ids = [<|startoftranscript|>], timed
end to end (encoder, one decoder pass over one token, the launch) with HIP events after a warm-up, --repeat times; beside it the
same pass without the last step (encode + decode alone), so their difference is what the language step adds.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bench_whisper_condition import _graph_us  # noqa: E402
from bench_whisper_transcribe import NMELS, TA, VOCAB, _emit, _events, _model_and_rules  # noqa: E402

R, SOT, N_LANG = 8, 50258, 99


def bench_op(args, languages):
    import torch
    from mop_amd import _lib, ops
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.bfloat16, torch.float32):
        x = (torch.randn(R, VOCAB, generator=g) * 3).to(dtype).cuda()
        probs = torch.empty(R, N_LANG, device="cuda")
        tokens = torch.empty(R, dtype=torch.int32, device="cuda")
        call = lambda: ops.language_probs(x, languages, probs, tokens)                                            # noqa: E731
        twin = lambda: ops.language_probs_torch(x, languages, probs, tokens)                                      # noqa: E731
        call()
        for rep in range(args.repeat):           # kernel and twin alternate: the spread between runs is in the file
            _emit(args, dict(workload="language_probs", run=rep, R=R, V=VOCAB, n=N_LANG, dtype=str(dtype).split(".")[1],
                             fused=ops.LAST_PATH["language_probs"] == _lib.PATH_FUSED,
                             op_call_us=round(_events(call, 20000, 200) * 1e3, 2), kernel_in_graph_us=round(_graph_us(call), 2),
                             torch_path_us=round(_events(twin, 5000, 50) * 1e3, 2), torch_path_in_graph_us=round(_graph_us(twin), 2)))


def bench_detect(args, m, languages):
    import torch
    torch.manual_seed(1)
    mel = torch.randn(R, TA, NMELS, device="cuda")
    ids = torch.full((R, 1), SOT, device="cuda")
    for rep in range(args.repeat):
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            full = _events(lambda: m.detect_language(mel, SOT, languages), args.steps, args.warmup)
            bare = _events(lambda: m.decode(m.encode(mel)[0], ids)[:, -1], args.steps, args.warmup)
        _emit(args, dict(workload="whisper_detect_language", run=rep, B=R, T_a=TA, T_s=1, n=N_LANG, vocab=VOCAB, dtype="bf16-autocast",
                         detect_language_ms=round(full, 3), encode_decode_alone_ms=round(bare, 3), difference_ms=round(full - bare, 3),
                         steps=args.steps, warmup=args.warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3, help="the end-to-end pair is timed this many times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_language_bench.jsonl"))
    args = ap.parse_args()
    from mop_amd import ops
    m, _ = _model_and_rules()
    languages = ops.LanguageTokens.for_whisper(VOCAB, SOT, N_LANG, device="cuda")
    bench_op(args, languages)
    bench_detect(args, m, languages)


if __name__ == "__main__":
    main()
