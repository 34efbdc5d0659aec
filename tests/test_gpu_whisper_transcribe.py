"""GPU checks of long-form transcription: the mopk_timestamp_segments kernel against the torch path on the same device tensors and
against the per-row Python restatement (the CPU sweep's rows and shapes, exactly: these are integers), strides, the -1 tail over
recycled memory, the window read from the device, repeatability, no host sync, graph capture (in a process of its own), and
WhisperMoP.transcribe against the naive loop over the same public decoders with one synchronising copy per window."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

from test_whisper_transcribe_cpu import (EOS, RULES, SWEEP_S, TB, V, assert_segments_equal, assert_transcripts_equal,
                                         check_transcript_shape, hand_cases, naive_transcribe, random_rows, ref_segments, sweep_cases,
                                         tensors)

pytestmark = pytest.mark.gpu


def _both(rows, t0, window, f, what, pad=0):
    """the kernel's result, after it matched the torch path on the same device tensors and the restatement"""
    from mop_amd import _lib, ops
    tok, win = tensors(rows, window, "cuda", pad)
    got = ops.timestamp_segments(tok, t0, win, TB, EOS, f)
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_FUSED, what
    assert_segments_equal(got, tuple(x.cpu() for x in ops.timestamp_segments_torch(tok, t0, win, TB, EOS, f)), what + " (torch)")
    assert_segments_equal(got, ref_segments(rows, t0, window, TB, EOS, f), what + " (restatement)")
    return got


@pytest.mark.parametrize("S", SWEEP_S)
def test_kernel_equals_both_references_on_random_rows(S):
    for name, rows, t0, window, f in sweep_cases(S):
        _both(rows, t0, window, f, name)


def test_kernel_equals_both_references_on_hand_built_rows():
    for name, rows, t0, window in hand_cases():
        for f in (1, 2):
            _both(rows, t0, window, f, f"{name}, f = {f}")


def test_full_width_rows():
    """T - t0 = 1024, the widest row the kernel takes (sixteen waves), and 1025, which goes to the torch path"""
    from mop_amd import _lib, ops
    rows, window = random_rows(3, 1024, 3, seed=5)
    _both(rows, 3, window, 1, "S = 1024")
    rows, window = random_rows(2, 1025, 0, seed=6)
    tok, win = tensors(rows, window, "cuda")
    assert not ops.timestamp_segments_supported(tok, 0, win, TB, EOS)
    assert_segments_equal(ops.timestamp_segments(tok, 0, win, TB, EOS), ref_segments(rows, 0, window, TB, EOS), "S = 1025")
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_GENERIC


def test_strides_tail_and_window():
    from mop_amd import _lib, ops
    rows, window = random_rows(6, 70, 3, seed=8)
    _both(rows, 3, window, 2, "padded row stride", pad=9)
    tok, win = tensors(rows, window, "cuda")
    got = ops.timestamp_segments(tok[::2], 3, win[::2].contiguous(), TB, EOS, 2)           # tokens[::K]: a row stride of K * T
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_FUSED
    assert_segments_equal(got, ref_segments(rows[::2], 3, window[::2], TB, EOS, 2), "tokens[::2]")
    one = ops.timestamp_segments(tok[0, 3:].unsqueeze(0), 0, win[:1], TB, EOS)              # a single row: any stride
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_FUSED
    assert_segments_equal(one, ref_segments([rows[0][3:]], 0, window[:1], TB, EOS), "one row")
    # the -1 tail is written by the launch: the library called on buffers of this test's own, filled with garbage beforehand
    seg = torch.full((4, 6, 70), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    row = torch.full((2, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    a = ops._ts_args(tok, 3, win, TB, EOS, 1)
    a.starts, a.ends, a.tok_begin, a.tok_end = (seg[k].data_ptr() for k in range(4))
    a.n_segments, a.advance = row[0].data_ptr(), row[1].data_ptr()
    ops._launch("mopk_timestamp_segments", a)
    torch.cuda.synchronize()
    assert_segments_equal(tuple(seg) + tuple(row), ref_segments(rows, 3, window, TB, EOS, 1), "garbage")
    assert int((seg == -1).sum()) > 0 and int((seg == 0x5A5A5A5A).sum()) == 0
    # the window is read from the device: another tensor, another advance
    rows = [[7, 8, 9, 5, 6, EOS]] * 2
    tok, _ = tensors(rows, [1, 1], "cuda")
    a = ops.timestamp_segments(tok, 3, torch.tensor([40, 13], dtype=torch.int32, device="cuda"), TB, EOS)
    b = ops.timestamp_segments(tok, 3, torch.tensor([21, 0], dtype=torch.int32, device="cuda"), TB, EOS)
    assert a.advance.tolist() == [40, 13] and b.advance.tolist() == [21, 1] and a.ends[:, 0].tolist() == [40, 13]


def test_repeatable_and_no_host_sync():
    from mop_amd import _lib, ops
    rows, window = random_rows(16, 445, 3, seed=9)
    tok, win = tensors(rows, window, "cuda")
    first = ops.timestamp_segments(tok, 3, win, TB, EOS, 2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ops.timestamp_segments(tok, 3, win, TB, EOS, 2)
        assert ops.timestamp_segments_supported(tok, 3, win, TB, EOS, 2)
        generic = ops.timestamp_segments_torch(tok, 3, win, TB, EOS, 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_FUSED
    for x, y, z in zip(first, again, generic):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_graph_replay_reproduces_eager():
    """one captured ops.timestamp_segments launch replayed on changed tokens, and transcribe(graph=True) against eager, in a
    process of their own (tools/graph_probe_whisper_transcribe.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_whisper_transcribe.py")], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + (r.stderr or r.stdout)[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "FUSED True" in r.stdout, r.stdout[-400:]
    assert "OP_REPLAY_IDENTICAL True" in r.stdout, r.stdout[-800:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-800:]


def _model():
    from mop_amd.nn import WhisperConfig, WhisperMoP
    torch.manual_seed(0)
    cfg = WhisperConfig(n_mels=12, n_audio_ctx=64, vocab_size=V, n_text_ctx=64, n_embd=128, n_head=2, n_layer_enc=1, n_layer_dec=2)
    m = WhisperMoP(cfg)
    with torch.no_grad():                      # at the default init every logit gap is ~1e-2: widen them
        m.dec_ln_f.weight.mul_(20.0)
    return m.cuda().eval()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("num_beams", [1, 3])
def test_transcribe_equals_the_naive_loop(num_beams, graph):
    """the synchronising calls counted are the ones torch's sync debug mode reports (copies that wait, .item(), ...); the device
    synchronise with which torch.cuda.graph opens every capture of graph=True is not among them"""
    from mop_amd import _lib, ops
    m = _model()
    torch.manual_seed(4)
    clips = [torch.randn(n, 12, device="cuda") for n in (150, 64, 37)]
    prompt = torch.tensor([7, 8, 9], device="cuda")
    rules = ops.LogitRules(V, **RULES, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want, log, seek = naive_transcribe(m, clips, prompt, rules, 12, 64, 1, num_beams, graph)
        n_windows = max(len(item) for item in log)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                got = m.transcribe(clips, prompt, rules, 12, window=64, num_beams=num_beams, graph=graph)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in caught if "synchroniz" in str(w.message)]
    print(f"num_beams={num_beams} graph={graph}: windows {n_windows}, synchronising calls {len(syncs)}, advances {log}")
    assert ops.LAST_PATH["timestamp_segments"] == _lib.PATH_FUSED
    assert_transcripts_equal(got, want, torch.int64, (num_beams, graph))
    for g in got:
        check_transcript_shape(g, ordered=False)
        assert g.starts.is_cuda and g.tokens.is_cuda
    assert all(s >= n for s, n in zip(seek, (150, 64, 37))) and n_windows >= 3
    assert len(syncs) == n_windows, syncs                                  # the one (A, 3) copy of each window, nothing else
