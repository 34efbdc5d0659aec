"""test helper (GPU box): the three WhisperMoP decoders under Whisper's logit rules (with_logit_rules) with graph=True -- one step
with its ops.logit_rules launch captured with torch.cuda.graph and replayed per token -- against the eager runs, in fp32 and under
bf16 autocast; prints whether the rules ran on the HIP kernel and whether tokens, step logits, scores and sum_logprobs are
bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import LogitRules, WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=300, vocab_size=1000, n_text_ctx=96, n_embd=256, n_head=4, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
with torch.no_grad():
    m.dec_ln_f.weight.mul_(20.0)                 # peaked logits: text and timestamps both win steps
rules = LogitRules(1000, suppress_tokens=[1, 2, 500, 899], suppress_at_begin=[5, 800], timestamp_begin=900, eos_token_id=800,
                   no_timestamps_token_id=898, max_initial_timestamp_index=10)
d = m.with_logit_rules(rules)
mel = torch.randn(2, 300, 16, device="cuda")
prompt = torch.randint(0, 800, (2, 4), device="cuda")
runs = {
    "generate": lambda g: d.generate(mel, prompt, 40, eos_token_id=800, graph=g, return_logits=True),
    "beam_search": lambda g: d.beam_search(mel, prompt, 40, 4, eos_token_id=800, graph=g),
    "sample": lambda g: d.sample(mel, prompt, 40, temperature=0.7, top_k=20, num_samples=3, eos_token_id=800, seed=3, graph=g),
}
ok = True
for autocast in (False, True):
    for name, run in runs.items():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            eager = run(False)
            fused = ops.LAST_PATH.get("logit_rules") == _lib.PATH_FUSED
            try:
                graphed = run(True)
            except RuntimeError as e:
                print("CAPTURE_UNSUPPORTED", name, repr(e)[:300], flush=True)
                sys.exit(0)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(eager, graphed))
        print(f"autocast={autocast} {name} FUSED {fused} identical {same}", flush=True)
        ok = ok and same and fused
print("FUSED", ops.LAST_PATH.get("logit_rules") == _lib.PATH_FUSED, flush=True)
print("GRAPH_IDENTICAL", ok, flush=True)
