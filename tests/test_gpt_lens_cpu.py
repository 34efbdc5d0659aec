"""Per-row lengths on the GPT line, the parts that need no GPU: the torch statements of the semantics against the float64
row-alone reference (tests/gpt_lens_ref.py), the refusals, the new library queries, and the list padding of the language models."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpt_lens_ref import quartet_rows_alone, token_gate_rows_alone

B, T, H, DH = 5, 9, 2, 8
LENS = (9, 5, 2, 1, 0)          # T, an interior length, the shortest row with a defined std, a single key, an empty row


def _qt_inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(B, T, H, DH, dtype=torch.float64, generator=g) for _ in range(5)]
    dy = torch.randn(B, T, H * DH, dtype=torch.float64, generator=g)
    return ts, dy


@pytest.mark.parametrize("uq", [True, False])
def test_quartet_core_lens_torch_is_every_row_alone(uq):
    from mop_amd import ops
    ts, dy = _qt_inputs()
    lens = torch.tensor(LENS, dtype=torch.int32)
    ref = quartet_rows_alone(*ts[:3], ts[3] if uq else None, ts[4] if uq else None, 0.3, 0.8, LENS, 1e-5, uq, dy)
    tr = [t.clone().requires_grad_(True) for t in ts]
    mix = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    qs = torch.tensor([0.8], dtype=torch.float64, requires_grad=True)
    y, attn = ops.quartet_core_lens_torch(tr[0], tr[1], tr[2], tr[3] if uq else None, tr[4] if uq else None, mix if uq else None,
                                          qs if uq else None, lens, 1e-5, uq, need_weights=True)
    y.backward(dy)
    assert np.abs(y.detach().numpy() - ref["y"]).max() <= 1e-12
    assert np.abs(attn.detach().double().numpy() - ref["P"]).max() <= 1e-6          # the weights are returned as float32
    names = ["q", "k", "v"] + (["q2", "k2"] if uq else [])
    for n, t in zip(names, tr):
        assert np.abs(t.grad.numpy() - ref["d" + n]).max() <= 1e-12, n
    if uq:
        assert abs(float(mix.grad) - ref["dmixture"]) <= 1e-12 and abs(float(qs.grad) - ref["dquartet_scale"]) <= 1e-12
    for b, n in enumerate(LENS):                                           # padding: exactly zero
        assert not y[b, n:].detach().any() and all(not t.grad[b, n:].any() for t in tr[:len(names)])


def test_quartet_core_lens_torch_reads_nothing_beyond_a_length():
    from mop_amd import ops
    ts, _ = _qt_inputs(1)
    lens = torch.tensor(LENS, dtype=torch.int32)
    y = ops.quartet_core_lens_torch(*ts, torch.tensor([0.3]), torch.tensor([0.8]), lens, 1e-5, True)
    for t in ts:
        for b, n in enumerate(LENS):
            t[b, n:] = float("nan")
    assert torch.equal(y, ops.quartet_core_lens_torch(*ts, torch.tensor([0.3]), torch.tensor([0.8]), lens, 1e-5, True))


@pytest.mark.parametrize("with_a", [True, False])
def test_token_gate_torch_with_lens_is_every_row_alone(with_a):
    from mop_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, 16, dtype=torch.float64, generator=g)
    a = torch.randn(B, T, 16, dtype=torch.float64, generator=g) if with_a else None
    u = 0.1 * torch.randn(3, 16, dtype=torch.float64, generator=g)
    dout = torch.randn(B, T, 16, dtype=torch.float64, generator=g)
    ro, rdr, rdu = token_gate_rows_alone(x, a, u, LENS, dout)
    for poison in (False, True):
        xp = x.clone()
        if poison:                                                         # r beyond a length is never read
            for b, n in enumerate(LENS):
                xp[b, n:] = float("nan")
        xr, ur = xp.requires_grad_(True), u.clone().requires_grad_(True)
        ar = None if a is None else a.clone().requires_grad_(True)
        out = ops.token_gate_1d_torch(xr, ar, ur, torch.tensor(LENS, dtype=torch.int32))
        out.backward(dout)
        assert float((out.detach() - ro).abs().max()) <= 1e-12
        assert float((xr.grad - rdr).abs().max()) <= 1e-12 and float((ur.grad - rdu).abs().max()) <= 1e-12
        if ar is not None:
            assert float((ar.grad - rdr).abs().max()) <= 1e-12
    assert torch.equal(ops.token_gate_1d_torch(x, a, u, torch.full((B,), T, dtype=torch.int32)), ops.token_gate_1d_torch(x, a, u))


def test_lens_refusals():
    from mop_amd import ops
    ts, _ = _qt_inputs(2)
    ts = [t.float() for t in ts]
    sc = (torch.tensor([0.3]), torch.tensor([0.8]))
    ok = torch.tensor(LENS, dtype=torch.int32)
    bad = {"dtype": ok.long(), "shape": torch.zeros(B + 1, dtype=torch.int32), "rank": ok.view(B, 1), "device": ok.to("meta"),
           "type": list(LENS)}
    for what, lens in bad.items():
        with pytest.raises(ValueError, match="lens"):
            ops.quartet_core(*ts, *sc, None, 1e-5, True, lens=lens)
        with pytest.raises(ValueError, match="lens"):
            ops.token_gate_1d(ts[0].reshape(B, T, H * DH), None, torch.zeros(3, H * DH), lens)
    with pytest.raises(ValueError, match="add_mask"):
        ops.quartet_core(*ts, *sc, torch.zeros(T, T), 1e-5, True, lens=ok)
    # a CPU call with good lengths: the token gate takes the torch route, the core says that it needs the GPU
    x = ts[0].reshape(B, T, H * DH)
    assert not ops.token_gate_supported(x, None, ok)
    assert torch.equal(ops.token_gate_1d(x, None, torch.ones(3, H * DH), ok), ops.token_gate_1d_torch(x, None, torch.ones(3, H * DH), ok))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.quartet_core(*ts, *sc, None, 1e-5, True, lens=ok)


def _qt_struct(L, T_, dh, prec, io, path, uq=1):
    a = L.QuartetArgs()
    a.B, a.H, a.T, a.dh, a.io_dtype, a.precision, a.path, a.use_quartet = 3, 2, T_, dh, io, prec, path, uq
    for v in (a.q, a.k, a.v, a.q2, a.k2, a.y, a.dy, a.dq, a.dk_, a.dv, a.dq2, a.dk2):
        v.sb, v.sn, v.sh = T_ * 2 * dh, 2 * dh, dh
    return a


def test_lens_queries_answer_as_the_base():
    from mop_amd import _lib as L
    lib = L.lib()
    n = 0
    for T_ in (1, 64, 200):
        for dh in (16, 32, 64):
            for prec, io in ((L.PREC_FP32, L.MOPK_F32), (L.PREC_BF16, L.MOPK_BF16), (L.PREC_BF16, L.MOPK_F32)):
                for path in (L.PATH_AUTO, L.PATH_GENERIC, L.PATH_FUSED):
                    a = _qt_struct(L, T_, dh, prec, io, path)
                    la = L.QuartetLensArgs(base=a, lens=None)
                    assert lib.mopk_quartet_lens_fused_supported(C.byref(la)) == lib.mopk_quartet_fused_supported(C.byref(a))
                    assert lib.mopk_quartet_lens_saved_bytes(C.byref(la)) == lib.mopk_quartet_saved_bytes(C.byref(a)) > 0
                    assert lib.mopk_quartet_lens_workspace_bytes(C.byref(la)) == lib.mopk_quartet_workspace_bytes(C.byref(a)) > 0
                    n += lib.mopk_quartet_lens_fused_supported(C.byref(la))
    assert n > 0                                                            # some of these calls are the fused kernels'
    a = _qt_struct(L, 64, 64, L.PREC_BF16, L.MOPK_BF16, L.PATH_AUTO)
    a.add_mask = 4096                                                       # lengths do not combine with an additive mask
    la = L.QuartetLensArgs(base=a, lens=None)
    assert lib.mopk_quartet_lens_fused_supported(C.byref(la)) == 0 and lib.mopk_quartet_lens_saved_bytes(C.byref(la)) == 0
    for D, T_ in ((64, 40), (1024, 1000), (1032, 8), (100, 8)):
        g = L.TokenGateArgs()
        g.B, g.T, g.D, g.x_dtype, g.o_dtype, g.x_sb, g.x_st = 7, T_, D, L.MOPK_F32, L.MOPK_F32, T_ * D, D
        lg = L.TokenGateLensArgs(base=g, lens=None)
        assert lib.mopk_token_gate_lens_supported(C.byref(lg)) == lib.mopk_token_gate_supported(C.byref(g)) == int(D in (64, 1024))
        assert lib.mopk_token_gate_lens_workspace_bytes(C.byref(lg)) == lib.mopk_token_gate_workspace_bytes(C.byref(g)) > 0
    lg.base.D, lg.lens = 64, 2                                              # a misaligned lengths pointer is not taken
    assert lib.mopk_token_gate_lens_supported(C.byref(lg)) == 0


@pytest.mark.parametrize("which", ["quartet", "mop"])
def test_models_pad_a_list_of_documents(which):
    from mop_amd.nn import GPT_MoP, TinyTransformerLM, TransformerConfig
    cfg = TransformerConfig(n_layer=1, n_head=2, n_embd=16, dropout=0.0, block_size=16)
    m = (TinyTransformerLM if which == "quartet" else GPT_MoP)(11, cfg)
    docs = [torch.arange(1, n + 1) % 11 for n in (7, 3, 1)]
    tgts = [d + 1 for d in docs]
    idx, tg, lens = m._batch(docs, tgts, ignore_index=-100)
    assert idx.shape == (3, 7) and lens.dtype == torch.int32 and lens.tolist() == [7, 3, 1]
    for b, d in enumerate(docs):
        assert torch.equal(idx[b, :len(d)], d) and not idx[b, len(d):].any()                 # pad id 0
        assert torch.equal(tg[b, :len(d)], tgts[b]) and bool((tg[b, len(d):] == -100).all())  # ignore_index
    assert bool((m._batch(docs, tgts, ignore_index=-7)[1][1, 3:] == -7).all())
    # an equal-length list is the stacked tensor without lengths: the tensor path
    same = [torch.arange(5), torch.arange(5) + 1]
    idx, tg, lens = m._batch(same, [t + 1 for t in same])
    assert lens is None and torch.equal(idx, torch.stack(same)) and torch.equal(tg, torch.stack(same) + 1)
    # a tensor call is passed through untouched
    t = torch.ones(2, 5, dtype=torch.long)
    out = m._batch(t, t)
    assert out[0] is t and out[1] is t and out[2] is None
    for bad in (dict(idx=docs, targets=tgts[:2]), dict(idx=t, targets=tgts), dict(idx=[torch.ones(2, 2, dtype=torch.long)], targets=None)):
        with pytest.raises(ValueError):
            m._batch(bad["idx"], bad["targets"])
    # the reference's parameters are kept: lengths reach the models as lists
    import inspect
    assert list(inspect.signature(m.forward).parameters) == ["idx", "attention_mask", "targets"]
