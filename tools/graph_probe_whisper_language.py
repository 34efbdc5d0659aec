"""test helper (GPU box): WhisperMoP.transcribe with language detection (languages=...) and graph=True -- every window's decoder
step captured with torch.cuda.graph and replayed per token, the detection pass in front of the loop eager -- against the eager run
and against transcribe given the prompts filled by hand from detect_language, greedy and with 3 beams, in fp32 and under bf16
autocast; prints whether the language step ran on the HIP kernel and whether transcripts and detection are bit-identical."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402
from mop_amd.nn import LanguageTokens, LogitRules, WhisperConfig, WhisperMoP  # noqa: E402

torch.manual_seed(0)
cfg = WhisperConfig(n_mels=16, n_audio_ctx=100, vocab_size=1000, n_text_ctx=96, n_embd=256, n_head=4, n_layer_enc=1, n_layer_dec=2)
m = WhisperMoP(cfg).cuda().eval()
with torch.no_grad():
    m.dec_ln_f.weight.mul_(20.0)                 # peaked logits: text and timestamps both win steps
rules = LogitRules(1000, suppress_tokens=[1, 2, 500, 899], suppress_at_begin=[5, 800], timestamp_begin=900, eos_token_id=800,
                   no_timestamps_token_id=898, max_initial_timestamp_index=10)
languages = LanguageTokens(1000, range(700, 720))
clips = [torch.randn(n, 16, device="cuda") for n in (230, 100, 41)]
prompt = torch.tensor([799, 0, 3], device="cuda")
d = m.with_logit_rules(rules)
ok = True
for autocast in (False, True):
    for beams in (1, 3):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            det = m.detect_language([c[:100] for c in clips], prompt[:1], languages)
            filled = prompt.unsqueeze(0).expand(3, -1).clone()
            filled[:, 1] = det.tokens
            byhand = d.transcribe(clips, filled, 20, num_beams=beams)
            ops.LAST_PATH.pop("language_probs", None)
            eager, edet = d.transcribe(clips, prompt, 20, num_beams=beams, languages=languages)
            fused = ops.LAST_PATH.get("language_probs") == _lib.PATH_FUSED
            try:
                graph, gdet = d.transcribe(clips, prompt, 20, num_beams=beams, graph=True, languages=languages)
            except RuntimeError as e:
                print("CAPTURE_UNSUPPORTED", beams, repr(e)[:300], flush=True)
                sys.exit(0)
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) and torch.equal(x, z) for a, b, c in zip(byhand, eager, graph) for x, y, z in zip(a, b, c))
        same = same and all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(det, edet, gdet))
        print(f"autocast={autocast} beams={beams} FUSED {fused} identical {same} languages {gdet.tokens.tolist()} "
              f"tokens {[int(t.tokens.numel()) for t in graph]}", flush=True)
        ok = ok and same and fused and all(t.tokens.numel() > 0 for t in graph)
print("FUSED", ops.LAST_PATH.get("language_probs") == _lib.PATH_FUSED, flush=True)
print("GRAPH_IDENTICAL", ok, flush=True)
