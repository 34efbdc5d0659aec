"""test helper (GPU box): one ops.alignment_rows launch and one ops.word_spans launch, each captured once with torch.cuda.graph and
replayed after its static input buffers changed, against the eager op and the torch restatement on the new contents; prints
whether both ran on the HIP kernels and whether everything is identical (the words' probabilities bit for bit against the eager
kernel, the integers against the torch restatement too)."""
import sys

import torch

sys.path.insert(0, ".")
from mop_amd import _lib, ops  # noqa: E402

TB, EOS, V = 101, 97, 131


def rows(R, T, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(R, T, generator=g)
    tok = torch.randint(0, EOS, (R, T), generator=g)
    tok = torch.where(u < 0.4, TB + torch.randint(0, 7, (R, T), generator=g), tok)
    return torch.where(u < 0.03, EOS, tok).to(torch.int32)


def spans_inputs(R, N, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, V, (R, N), generator=g).to(torch.int32)
    times = torch.randint(0, 4, (R, N + 1), generator=g).cumsum(1).to(torch.int32)
    return tok, times, torch.rand(R, N, generator=g), torch.randint(0, N + 1, (R,), generator=g).to(torch.int32)


def same(x, y):
    return all(torch.equal(p, q) for p, q in zip(x, y))


ids = range(V)
rules = ops.WordRules(V, [v for v in ids if v % 2 == 0 or v % 5 == 0], [v for v in ids if v % 5 == 0], [v for v in ids if v % 5 == 1],
                      [v for v in ids if v % 2 == 1], device="cuda")
tok, take = rows(5, 70, 1).cuda(), torch.tensor([40, 67, 0, 64, 17], dtype=torch.int32).cuda()
sot = torch.tensor([7, 8, 9], device="cuda")
stok, stimes, sprobs, sn = (t.cuda() for t in spans_inputs(5, 130, 1))
ops.alignment_rows(tok, 3, take, sot, 100, EOS)                  # warm-up outside the capture
ops.word_spans(stok, stimes, sprobs, sn, rules, 3)
fused = ops.LAST_PATH.get("alignment_rows") == _lib.PATH_FUSED and ops.LAST_PATH.get("word_spans") == _lib.PATH_FUSED
torch.cuda.synchronize()
g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(g1):
        out_rows = ops.alignment_rows(tok, 3, take, sot, 100, EOS)
    with torch.cuda.graph(g2):
        out_spans = ops.word_spans(stok, stimes, sprobs, sn, rules, 3)
except RuntimeError as e:
    print("CAPTURE_UNSUPPORTED", repr(e)[:300], flush=True)
    sys.exit(0)
ok = True
for seed in (2, 3):
    tok.copy_(rows(5, 70, seed))
    take.copy_(torch.tensor([seed, 67, 9, 40, 70], dtype=torch.int32))
    for dst, src in zip((stok, stimes, sprobs, sn), spans_inputs(5, 130, seed)):
        dst.copy_(src)
    g1.replay()
    g2.replay()
    torch.cuda.synchronize()
    ok = ok and same(out_rows, ops.alignment_rows_torch(tok, 3, take, sot, 100, EOS)) and same(out_rows, ops.alignment_rows(tok, 3, take, sot, 100, EOS))
    want = ops.word_spans_torch(stok, stimes, sprobs, sn, rules, 3)
    ok = ok and same(out_spans, ops.word_spans(stok, stimes, sprobs, sn, rules, 3))
    ok = ok and all(torch.equal(getattr(out_spans, f), getattr(want, f)) for f in ("starts", "ends", "tok_begin", "tok_end", "n_words"))
    # against the twin only a flat bound: 131 = N + 1, the (count + 1) * 2^-24 of a word that holds all N = 130 tokens (the
    # bit-for-bit comparison with the eager kernel above is the check of the replay)
    ok = ok and float((out_spans.probs - want.probs).abs().max()) <= 131 * 2.0 ** -24 and int(out_spans.n_words.sum()) > 0
print("FUSED", fused, flush=True)
print("OP_REPLAY_IDENTICAL", ok, flush=True)
