#!/usr/bin/env python3
"""ms/token of WhisperMoP.generate with and without return_stats, eager and graph=True, at tools/bench_whisper_decode.py's shapes
(d = 512, H = 8, 6 + 6 layers, T_a = 1500, vocab 51865, bf16 autocast, prompt 4 + 220 tokens, B in {1, 8}; end to end, encoder
included).  One JSON line per (B, variant), appended to <out.jsonl>: the median, minimum and maximum of five timed repetitions after
one warm-up, the variants interleaved inside every repetition.

    python tools/bench_whisper_decode_stats.py <package root> <label> <out.jsonl>

<package root> is the directory that holds the mop_amd package to measure (with its built libmopk.so): "." for this tree, or a
checkout of another commit, which has no statistics route and is measured on the default route only.  profiles/
whisper_decode_stats_bench.jsonl was written by alternating processes: parent commit, this tree, parent commit, this tree."""
import json
import statistics
import sys

root, label, out = sys.argv[1:4]
sys.path.insert(0, root)
import torch  # noqa: E402
from mop_amd.nn import WhisperConfig, WhisperMoP  # noqa: E402

TA, D, H, LAYERS, VOCAB, NMELS, TP, NEW = 1500, 512, 8, 6, 51865, 80, 4, 220
cfg = WhisperConfig(n_mels=NMELS, n_audio_ctx=TA, vocab_size=VOCAB, n_text_ctx=448, n_embd=D, n_head=H, n_layer_enc=LAYERS, n_layer_dec=LAYERS)
torch.manual_seed(0)
m = WhisperMoP(cfg).cuda().eval()
d = m.with_logit_rules(None)
import inspect  # noqa: E402
has_stats = "return_stats" in inspect.signature(d.generate).parameters
for B in (1, 8):
    mel = torch.randn(B, TA, NMELS, device="cuda")
    prompt = torch.randint(0, VOCAB, (B, TP), device="cuda")
    variants = {"default_eager": lambda: m.generate(mel, prompt, NEW), "default_graph": lambda: m.generate(mel, prompt, NEW, graph=True)}
    if has_stats:
        variants["stats_eager"] = lambda: d.generate(mel, prompt, NEW, return_stats=True)
        variants["stats_graph"] = lambda: d.generate(mel, prompt, NEW, graph=True, return_stats=True)
    times = {k: [] for k in variants}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for rep in range(6):                      # repetition 0 is the warm-up
            for name, fn in variants.items():
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(a.elapsed_time(b))
    for name, ts in times.items():
        rec = dict(workload="whisper_generate_stats", tree=label, variant=name, B=B, T_a=TA, T_p=TP, new_tokens=NEW, d=D, H=H,
                   layers="6+6", vocab=VOCAB, dtype="bf16-autocast", reps=len(ts), ms_per_token_median=round(statistics.median(ts) / NEW, 4),
                   ms_per_token_min=round(min(ts) / NEW, 4), ms_per_token_max=round(max(ts) / NEW, 4))
        print(json.dumps(rec), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
