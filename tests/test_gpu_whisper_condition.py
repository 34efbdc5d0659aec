"""GPU checks of transcribe's conditioning on the previous text: the mopk_prompt_history_update and mopk_window_prompts kernels
against the torch path on the same device tensors and against the Python-list restatement of tests/test_whisper_condition_cpu.py
(the hand-built rows and the sweep over caps, rows, sot lengths, first columns, history lengths, token counts, modes, items out of
range, padded row strides, per-item sot sequences, both output dtypes and every width; sentinels around the state and in untouched
clips; what the kernels do not take; bitwise repeatability; no host sync), and transcribe on the device against the naive loop
over the public decoders with list prompts: greedy, three beams, graph=True, and a fallback run that shows a reset."""
import warnings

import pytest
import torch

from test_gpu_whisper_fallback import _model
from test_whisper_condition_cpu import (N_HIST, PREV, SWEEP_N, check_conditioned_case, check_prompts, check_reset_case, check_update,
                                        prompt_cases, state, token_rows, update_hand_cases, update_sweep_cases)
from test_whisper_transcribe_cpu import RULES, V

pytestmark = pytest.mark.gpu


def _fused(ops, key, what):
    from mop_amd import _lib
    assert ops.LAST_PATH.pop(key) == _lib.PATH_FUSED, (key, what)


def _update_both(ops, *case, pad=0):
    """the kernel against the restatement, then the torch path on device tensors against it: equal to each other, then"""
    name = case[-1] if isinstance(case[-1], str) else None
    ops.LAST_PATH.pop("prompt_history_update", None)
    got = check_update(ops.prompt_history_update, *case, device="cuda", pad=pad)
    _fused(ops, "prompt_history_update", name)
    ref = check_update(ops.prompt_history_update_torch, *case, device="cuda", pad=pad)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), name
    return got


def _prompts_both(ops, *case, **kw):
    ops.LAST_PATH.pop("window_prompts", None)
    got = check_prompts(ops.window_prompts, *case, device="cuda", **kw)
    _fused(ops, "window_prompts", case[-1])
    ref = check_prompts(ops.window_prompts_torch, *case, device="cuda", **kw)
    assert torch.equal(got.ids, ref.ids) and torch.equal(got.kv_start, ref.kv_start), case[-1]
    return got


def test_hand_built_rows():
    from mop_amd import ops
    for name, B, n, lens, rows, t0, take, item, mode in update_hand_cases():
        _update_both(ops, B, n, lens, rows, t0, take, item, mode, name)
        _update_both(ops, B, n, lens, rows, t0, take, item, mode, name, pad=3)
    sot = [7, 8, 9]
    for name, lens, item, width in (("bare", [0, 0, 0], [0, 1, 2], 3), ("unequal", [6, 2, 0], [0, 1, 2], 10),
                                    ("equal", [4, 4, 4], [2, 0, 1], 8), ("narrower", [6, 2, 0], [0, 1, 2], 7),
                                    ("sot_prev and one token", [6, 2, 0], [0, 1, 2], 5), ("sot_prev alone", [6, 2, 0], [0, 1, 2], 4),
                                    ("a subset with an item out of range", [6, 2, 3], [2, -1, 0, 3], 10),
                                    ("hist_len outside [0, n]", [9, -1, 3], [0, 1, 2], 10)):
        for dt in (torch.int64, torch.int32):
            _prompts_both(ops, 3, 6, lens, item, sot, PREV, width, dt, name)


@pytest.mark.parametrize("n", SWEEP_N)
def test_kernels_match_the_torch_path_and_the_restatement(n):
    from mop_amd import ops
    for name, B, n_, lens, rows, t0, take, item, mode, pad in update_sweep_cases(n):
        first = _update_both(ops, B, n_, lens, rows, t0, take, item, mode, name, pad=pad)
        again = _update_both(ops, B, n_, lens, rows, t0, take, item, mode, name, pad=pad)      # a second run: equal bits
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), name
    for name, B, n_, lens, item, sot, width in prompt_cases(n):
        kw = dict(sot_dtype=(torch.int64, torch.int32)[n % 2])
        first = _prompts_both(ops, B, n_, lens, item, sot, PREV, width, (torch.int64, torch.int32)[width % 2], name, **kw)
        again = _prompts_both(ops, B, n_, lens, item, sot, PREV, width, (torch.int64, torch.int32)[width % 2], name, **kw)
        assert torch.equal(first.ids, again.ids) and torch.equal(first.kv_start, again.kv_start), name


def test_what_the_kernels_do_not_take():
    from mop_amd import _lib, ops
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")      # noqa: E731
    # n = 1025 and T - t0 = 1025: the torch path, with the same results
    for n, S in ((1025, 8), (6, 1025)):
        rows = token_rows(2, S, n)
        _, _, hist, hl = state(3, n, [n, 2, 0], 0, "cuda")
        args = (torch.tensor(rows, dtype=torch.int32, device="cuda"), 0, i32([n + 1, 3]), i32([0, 2]), i32([0, 0]))
        assert not ops.prompt_history_update_supported(hist, hl, *args)
        check_update(ops.prompt_history_update, 3, n, [n, 2, 0], rows, 0, [n + 1, 3], [0, 2], [0, 0], (n, S), device="cuda")
        assert ops.LAST_PATH["prompt_history_update"] == _lib.PATH_GENERIC
    _, _, hist, hl = state(3, 6, [6, 2, 0], 0, "cuda")
    tok = torch.tensor(token_rows(2, 8, 1), dtype=torch.int32, device="cuda")
    two = i32([0, 1])
    assert ops.prompt_history_update_supported(hist, hl, tok, 3, two, two, two)
    assert not ops.prompt_history_update_supported(hist, hl, tok.long(), 3, two, two, two)
    assert not ops.prompt_history_update_supported(hist, hl, tok.t().contiguous().t(), 3, two, two, two)
    assert not ops.prompt_history_update_supported(hist, hl, tok, 3, two.long(), two, two)
    assert not ops.prompt_history_update_supported(hist, hl, tok, 3, two, i32([0, 9, 1, 9])[::2], two)
    sot = torch.tensor([7, 8, 9], device="cuda")
    assert ops.window_prompts_supported(hist, hl, two, sot, PREV, 2048)
    assert not ops.window_prompts_supported(hist, hl, two, sot, PREV, 2049)
    assert not ops.window_prompts_supported(hist, hl, two.long(), sot, PREV, 10)
    assert not ops.window_prompts_supported(hist, hl, two, sot.to(torch.int16), PREV, 10)
    check_prompts(ops.window_prompts, 3, 6, [6, 2, 0], [0, 1, 2], [7, 8, 9], PREV, 2049, torch.int32, "width 2049", device="cuda")
    assert ops.LAST_PATH["window_prompts"] == _lib.PATH_GENERIC
    check_prompts(ops.window_prompts, 3, 6, [6, 2, 0], [0, 1, 2], [7, 8, 9], PREV, 2048, torch.int32, "width 2048", device="cuda")
    assert ops.LAST_PATH["window_prompts"] == _lib.PATH_FUSED


def test_no_host_sync():
    from mop_amd import ops
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")      # noqa: E731
    _, _, hist, hl = state(9, 223, [223, 100, 0, 5, 223, 1, 7, 222, 50], 0, "cuda")
    tok = torch.tensor(token_rows(8, 4 + 220, 3), dtype=torch.int32, device="cuda")
    take, item, mode = i32([220, 0, 3, 150, 1, 9, 40, 7]), i32([8, 0, 1, 2, 3, 4, 5, 6]), i32([0, 0, 1, 0, 2, 0, 0, 1])
    sot = torch.tensor([7, 8, 9, 10], device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.prompt_history_update(hist, hl, tok, 4, take, item, mode)
        a = ops.LAST_PATH["prompt_history_update"]
        out = ops.window_prompts(hist, hl, item, sot, PREV, 228)
        b = ops.LAST_PATH["window_prompts"]
        ops.prompt_history_update_torch(hist, hl, tok, 4, take, item, mode)
        ref = ops.window_prompts_torch(hist, hl, item, sot, PREV, 228)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    from mop_amd import _lib
    assert a == b == _lib.PATH_FUSED
    assert out.ids.shape == (8, 228) and ref.ids.shape == (8, 228)


# ------------------------------------------------------------------ the model
def _condition_setup():
    from mop_amd import ops
    m = _model()
    torch.manual_seed(4)
    clips = [torch.randn(n, 12, device="cuda") for n in (200, 150, 140)]  # four, three and three windows of 64 frames
    return m, clips, torch.tensor([7, 8, 9], device="cuda"), ops.LogitRules(V, **RULES, device="cuda")


def _hints():
    """an initial prompt per clip, of different lengths, one empty and one beyond the cap: the first decoder call is ragged and
    truncated whatever the model decodes"""
    hint = torch.tensor([11, 12, 13, 14, 15, 16, 17, 18, 19], device="cuda")
    return [hint[:2], hint[:0], hint]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("num_beams", [1, 3])
def test_conditioned_transcribe_equals_the_naive_loop(num_beams, graph):
    """tokens compared exactly: both sides run the same kernels on the same tensors.  The synchronising calls counted are the ones
    torch's sync debug mode reports; conditioning adds none to the one (A, 3) copy per set of windows"""
    from mop_amd import _lib, ops
    m, clips, prompt, rules = _condition_setup()
    caught = []

    def run(call):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = call()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        caught.extend(str(x.message) for x in w if "synchroniz" in str(x.message))
        return out

    ops.LAST_PATH.clear()
    got, log, widths = check_conditioned_case(m, clips, prompt, rules, window=64, expect_effect=False, run=run, num_beams=num_beams,
                                              graph=graph, initial_prompt=_hints())
    print(f"num_beams={num_beams} graph={graph}: prompt lengths per call {widths}, synchronising calls {len(caught)}")
    assert ops.LAST_PATH["window_prompts"] == ops.LAST_PATH["prompt_history_update"] == _lib.PATH_FUSED
    assert widths[0] == [6, 3, 10] and len(widths) >= 3
    assert all(g.tokens.is_cuda for g in got)
    assert len(caught) == len(widths), caught                              # one decoder call and one (A, 3) copy per set of windows


def test_fallback_resets_the_history():
    m, clips, prompt, rules = _condition_setup()
    log = check_reset_case(m, clips, prompt, rules, window=64)
    print("per clip (seek, temperature, prompt length):", [[(w[0], w[1], w[5]) for w in g] for g in log])
