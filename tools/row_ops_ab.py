#!/usr/bin/env python3
"""dev tool: the row ops (token_logprob, greedy_pick, language_probs, sample_tokens[_ragged], logit_rules, repeat_rules, beam_step)
under whichever library MOPK_LIB names, on seeded inputs, for a bit-for-bit comparison of two builds of libmopk.so.

    MOPK_LIB=old/libmopk.so python tools/row_ops_ab.py --out old.pt [--time profiles/row_helpers_ab.jsonl --label parent]
    python tools/row_ops_ab.py --out new.pt [--time profiles/row_helpers_ab.jsonl --label new]
    python tools/row_ops_ab.py --compare old.pt new.pt         # torch.equal per entry (raw bits); exit status 1 on any difference

Shapes: V = 131 and 51865, R = 8 rows (beam: B = 8, K = 5), fp32 and bf16, each once contiguous and once entered one element behind
a 16-byte boundary.  --time appends one line per op: the median device time of 200 calls (V = 51865, bf16, R = 8, contiguous)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

R, K, T0 = 8, 5, 3


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def inputs(V, dtype, off, rows=R):
    """(rows, V) logits, contiguous or entered `off` elements behind a 16-byte boundary; a few -inf entries and an exact tie"""
    g = torch.Generator().manual_seed(V * 7 + rows)
    x = torch.randn(rows, V, generator=g) * 3
    x[:, 5] = float("-inf")
    x[1, 7] = x[1].max()
    flat = torch.zeros(rows * V + off, device="cuda", dtype=dtype)
    view = flat[off:].view(rows, V)
    view.copy_(x.to(dtype))
    assert view.data_ptr() % 16 == off * view.element_size()
    return view, g


def run_ops(V, dtype, off):
    """-> ({name: tensor}, {name: a call to time})"""
    from mop_amd import _lib, ops
    ops.LAST_PATH.clear()
    x, g = inputs(V, dtype, off)
    dev = dict(device="cuda")
    out, calls = {}, {}
    eos, tb = V // 3, V - 40
    pos = torch.tensor([T0 + 6], dtype=torch.int32, **dev)
    hist = torch.randint(0, V, (R, T0 + 9), generator=g).to(torch.int32).cuda()
    hist[::2, T0 + 5] = tb + 3                                             # rows whose last token is a timestamp
    hist[::4, T0 + 4] = tb + 2                                             # ... and the one before it

    toks = torch.randint(0, V, (R,), generator=g).to(torch.int32).cuda()
    out["token_logprob"] = ops.token_logprob(x, toks)
    calls["token_logprob"] = lambda: ops.token_logprob(x, toks)

    st = ops.GreedyState(R, 12, eos, with_hist=True, **dev)
    st.done[1] = 1
    ops.greedy_pick(x, st, pos)
    for f in ("next_ids", "done", "sum_logprobs", "n_tokens", "hist"):
        out["greedy_pick." + f] = getattr(st, f).clone()
    st2 = ops.GreedyState(R, 12, None, with_hist=True, **dev)
    calls["greedy_pick"] = lambda: ops.greedy_pick(x, st2, pos)

    langs = ops.LanguageTokens(V, torch.randperm(V, generator=g)[:min(99, V // 2)], **dev)
    lp = ops.language_probs(x, langs)
    out["language_probs.probs"], out["language_probs.tokens"] = lp.probs, lp.tokens
    calls["language_probs"] = lambda: ops.language_probs(x, langs)

    pos_off = (torch.arange(R, dtype=torch.int32) % 3).cuda()
    for tag, kw in (("greedy", dict(temperature=0.0)), ("topk_topp", dict(temperature=0.8, top_k=40, top_p=0.9, seed=5))):
        out[f"sample.{tag}.tokens"], out[f"sample.{tag}.logprobs"] = ops.sample_tokens(x, pos, **kw)
        out[f"sample_ragged.{tag}.tokens"], out[f"sample_ragged.{tag}.logprobs"] = ops.sample_tokens_ragged(x, pos, pos_off, **kw)
        calls["sample." + tag] = lambda kw=kw: ops.sample_tokens(x, pos, **kw)
        calls["sample_ragged." + tag] = lambda kw=kw: ops.sample_tokens_ragged(x, pos, pos_off, **kw)

    lr = ops.LogitRules(V, suppress_tokens=(2, 11), suppress_at_begin=(9, eos), timestamp_begin=tb, eos_token_id=eos,
                        no_timestamps_token_id=tb - 1, max_initial_timestamp_index=10, **dev)
    rr = ops.RepeatRules(V, 1.3, 3, exempt_tokens=(eos,), exempt_from=tb, **dev)
    for p in (T0, T0 + 6):                                                 # the first generated position, and a later one
        pp = torch.tensor([p], dtype=torch.int32, **dev)
        out[f"logit_rules.pos{p}"] = ops.logit_rules(x, hist, pp, T0, lr)
        out[f"repeat_rules.pos{p}"] = ops.repeat_rules(x, hist, pp, T0, rr)
    calls["logit_rules"] = lambda: ops.logit_rules(x, hist, pos, T0, lr)
    calls["repeat_rules"] = lambda: ops.repeat_rules(x, hist, pos, T0, rr)

    # three consecutive beam steps: the prompt's logits shared by each item's beams, then one row per beam
    prompt = torch.randint(0, V, (R, T0), generator=g).cuda()
    bs = ops.BeamState(prompt, K, T0 + 6, eos, 1.0)
    bpos = torch.tensor([T0], dtype=torch.int32, **dev)
    xk = inputs(V, dtype, off, R * K)[0]
    for step in range(3):
        ops.beam_step(x if step == 0 else xk, bs, bpos)
        bpos += 1
        for f in ("scores", "next_ids", "parents", "hist", "rows", "fin_tokens", "fin_scores", "fin_count", "done"):
            out[f"beam_step{step}.{f}"] = getattr(bs, f).clone()
    bs2 = ops.BeamState(prompt, K, T0 + 6, None, 1.0)
    tpos = torch.tensor([T0], dtype=torch.int32, **dev)
    calls["beam_step"] = lambda: ops.beam_step(xk, bs2, tpos)

    keys = ("token_logprob", "greedy_pick", "language_probs", "sample", "sample_ragged", "logit_rules", "repeat_rules", "beam_step")
    slow = [k for k in keys if ops.LAST_PATH.get(k) != _lib.PATH_FUSED]
    assert not slow, f"not on the HIP kernel: {slow}"
    torch.cuda.synchronize()
    return {k: bits(v).cpu() for k, v in out.items()}, calls


def median_us(call, n=200, warm=20):
    for _ in range(warm):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)[n // 2]


def compare(fa, fb):
    a, b = torch.load(fa), torch.load(fb)
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not torch.equal(a[k], b[k])]
    for k in bad:
        print("DIFFERS", k)
    print(f"{len(set(a) | set(b)) - len(bad)} of {len(set(a) | set(b))} entries bit-equal")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--time", metavar="JSONL")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    res = {}
    for V in (131, 51865):
        for dtype in (torch.float32, torch.bfloat16):
            for off in (0, 1):
                got, calls = run_ops(V, dtype, off)
                res.update({f"V{V}.{str(dtype)[6:]}.off{off}.{k}": v for k, v in got.items()})
                if args.time and (V, dtype, off) == (51865, torch.bfloat16, 0):
                    with open(args.time, "a") as f:
                        for name, call in calls.items():
                            f.write(json.dumps({"tool": "row_ops_ab", "label": args.label, "op": name, "V": V, "R": R, "dtype": "bf16", "calls": 200,
                                                "median_us": round(median_us(call), 3)}) + "\n")
    if args.out:
        torch.save(res, args.out)
    print(f"{len(res)} entries" + (f" -> {args.out}" if args.out else ""))
