"""test helper (GPU box): the three WhisperMoP decoders under repeat rules and Whisper's logit rules (with_logit_rules(rules,
repeat_rules)) with graph=True -- one step with its ops.repeat_rules and ops.logit_rules launches captured with torch.cuda.graph
and replayed per token -- against the eager runs, in fp32 and under bf16 autocast, and once more under the repeat rules alone;
prints whether both rule sets ran on their HIP kernels and whether tokens, step logits, scores and sum_logprobs are bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import LogitRules, RepeatRules, WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=300, vocab_size=1000, n_text_ctx=96, n_embd=256, n_head=4, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
with torch.no_grad():
    m.dec_ln_f.weight.mul_(20.0)                 # peaked logits: text and timestamps both win steps
rules = LogitRules(1000, suppress_tokens=[1, 2, 500, 899], suppress_at_begin=[5, 800], timestamp_begin=900, eos_token_id=800,
                   no_timestamps_token_id=898, max_initial_timestamp_index=10)
repeat = RepeatRules.for_whisper(rules, repetition_penalty=1.2, no_repeat_ngram_size=3)
both, alone = m.with_logit_rules(rules, repeat), m.with_logit_rules(None, repeat)
mel = torch.randn(2, 300, 16, device="cuda")
prompt = torch.randint(0, 800, (2, 4), device="cuda")


def runs_of(d):
    return {
        "generate": lambda g: d.generate(mel, prompt, 40, eos_token_id=800, graph=g, return_logits=True),
        "beam_search": lambda g: d.beam_search(mel, prompt, 40, 4, eos_token_id=800, graph=g),
        "sample": lambda g: d.sample(mel, prompt, 40, temperature=0.7, top_k=20, num_samples=3, eos_token_id=800, seed=3, graph=g),
    }


def fused_paths(with_logit_rules):
    keys = ("repeat_rules", "logit_rules") if with_logit_rules else ("repeat_rules",)
    return all(ops.LAST_PATH.get(k) == _lib.PATH_FUSED for k in keys)


ok = all_fused = True
for autocast, d in ((False, both), (True, both), (False, alone)):
    for name, run in runs_of(d).items():
        ops.LAST_PATH.pop("repeat_rules", None)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            eager = run(False)
            fused = fused_paths(d is both)
            try:
                graphed = run(True)
            except RuntimeError as e:
                print("CAPTURE_UNSUPPORTED", name, repr(e)[:300], flush=True)
                sys.exit(0)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(eager, graphed))
        print(f"autocast={autocast} logit_rules={d is both} {name} fused {fused} identical {same}", flush=True)
        ok = ok and same and fused
        all_fused = all_fused and fused
print("FUSED", all_fused, flush=True)
print("GRAPH_IDENTICAL", ok, flush=True)
