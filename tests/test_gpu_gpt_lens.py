"""Per-row sequence lengths on the GPT line (mopk_quartet_lens_*, mopk_token_gate_lens_*, the `lens` / list arguments of the
language models) on the MI355X: every row of a right-padded batch comes out as it would alone -- values, loss and gradients --
against the float64 row-alone reference of tests/gpt_lens_ref.py; nothing beyond a length is read; full lengths are bitwise the
call without lengths."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpt_lens_ref import quartet_rows_alone, token_gate_rows_alone
from gpu_util import check_grads, rel_err

pytestmark = pytest.mark.gpu
TOL = {"fp32": (1e-3, 1e-3), "bf16": (1e-2, 3e-2)}        # tests/test_gpu_siblings.py
QT_B, QT_H, QT_T = 6, 2, 200
QT_LENS = (200, 137, 128, 64, 2, 1)    # full | inside the 2nd 128-query block, partial key tile | block edge | key-tile edge | 2 | 1 key
MIX, QS, EPS = 0.3, 0.8, 1e-5


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _lens(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


SD_MIN = 0.1


def _min_row_sd(ts, lens, uq):
    """the smallest unbiased std of a score row (both maps with the quartet term) over the rows of two keys or more, in float64"""
    lo = float("inf")
    for b, n in enumerate(lens):
        if n >= 2:
            for q, k in ((ts[0], ts[1]), (ts[3], ts[4]))[:2 if uq else 1]:
                S = torch.einsum("ihd,jhd->hij", q[b, :n].double(), k[b, :n].double()) / q.shape[-1] ** 0.5
                lo = min(lo, float(S.std(-1).min()))
    return lo


@functools.lru_cache(maxsize=None)
def _qt_case(dk, uq, prec, lens=QT_LENS):
    """inputs in the io dtype (so the reference sees what the kernels see) and the float64 row-alone reference, computed once.

    A float64 comparison says something about a row only where the function is well conditioned.  The z-norm divides by sd + eps
    with eps = 1e-5, and the gradient of a two-key row is (dz0 - dz1) / 2 / (sd + eps) * eps / (sd + eps): exactly zero for eps = 0,
    but of order one when sd approaches eps, and then 1 / (sd + eps) multiplies the 2^-9 relative rounding of the bf16 MFMA
    operands (q / sqrt(dk) is rounded to bf16 once) into the result.  Measured: a draw whose two-key row had sd = 0.0019 gave a dq
    24 % of the tensor's maximum off the float64 value -- on the length-aware kernels and, bit for bit the same, on the plain
    kernels given that row alone at T = 2.  That is the conditioning of the problem, not the lengths, so the inputs are the first draw
    of a seeded sequence whose smallest row std, computed here in float64 from the inputs alone, is at least SD_MIN = 0.1 (about
    half of the draws; rows of 64 keys and more have sd near 1 and never decide it).  test_quartet_fused_rows_are_bitwise_the_rows_alone
    holds the kernels to the rows alone on any draw."""
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    B = len(lens)
    for draw in range(64):
        g = torch.Generator().manual_seed(100000 * draw + 1000 * dk + 10 * uq + (prec == "bf16"))
        ts = tuple(torch.randn(B, QT_T, QT_H, dk, generator=g).to(dt) for _ in range(5))
        dy = torch.randn(B, QT_T, QT_H * dk, generator=g).to(dt)
        if _min_row_sd(ts, lens, uq) >= SD_MIN:
            break
    else:
        raise AssertionError("no well-conditioned draw in 64")
    ref = quartet_rows_alone(*ts[:3], ts[3] if uq else None, ts[4] if uq else None, MIX, QS, lens, EPS, uq, dy)
    return ts, dy, ref


def _qt_run(ts, dy, uq, lens, poison=None, seed=None, p=0.0, need_weights=False, embed=False):
    """quartet_core forward + backward on CUDA copies; poison: a value written into every input beyond the lengths first;
    embed: every input sits in the middle of a buffer of NaN (guarded_alloc.embedded)"""
    from guarded_alloc import embedded
    from mop_amd import ops
    xs = [t.cuda().clone() for t in ts]
    g = dy.cuda().clone()
    if poison is not None:
        for b, n in enumerate(lens.tolist()):
            for t in xs + [g]:
                t[b, n:] = poison
    if embed:
        xs, g, lens = [embedded(t) for t in xs], embedded(g), embedded(lens)
    xs = [t.requires_grad_(True) for t in xs]
    mix = torch.tensor([MIX], device="cuda", requires_grad=True)
    qs = torch.tensor([QS], device="cuda", requires_grad=True)
    out = ops.quartet_core(xs[0], xs[1], xs[2], xs[3] if uq else None, xs[4] if uq else None, mix if uq else None, qs if uq else None,
                           None, EPS, uq, need_weights, dropout_p=p, seed=seed, lens=lens)
    y, attn = out if need_weights else (out, None)
    y.backward(g)
    n = 5 if uq else 3
    res = {"y": y.detach()}
    res.update({"d" + k: t.grad for k, t in zip(("q", "k", "v", "q2", "k2")[:n], xs)})
    if uq:
        res.update(dmixture=mix.grad, dquartet_scale=qs.grad)
    if attn is not None:
        res["P"] = attn
    return res


def _per_row(got, ref, lens):
    den = max(float(np.abs(ref).max()), 1e-30)
    return ", ".join(f"row {b} (n={n}): {float(np.abs(got[b] - ref[b]).max()) / den:.2e}" for b, n in enumerate(lens))


def _qt_check(res, ref, prec, lens, uq):
    tol, gtol = TOL[prec]
    y = res["y"].float().cpu().numpy()
    assert rel_err(y, ref["y"]) <= tol, "y " + _per_row(y, ref["y"], lens)
    names = ["dq", "dk", "dv"] + (["dq2", "dk2"] if uq else [])
    grads = {k: res[k].float().cpu().numpy() for k in names}
    gref = {k: ref[k] for k in names}
    for k in names:
        assert rel_err(grads[k], gref[k]) <= gtol, f"{k} " + _per_row(grads[k], gref[k], lens)
    if uq:
        grads.update({k: res[k].float().cpu().numpy() for k in ("dmixture", "dquartet_scale")})
        gref.update({k: np.asarray([ref[k]]) for k in ("dmixture", "dquartet_scale")})
    check_grads(grads, gref, gtol, scalar_tol=5e-2 if prec == "bf16" else None, floor=1e-2 if prec == "bf16" else 1e-3)
    for b, n in enumerate(lens):                                  # padding outputs and gradients: exactly 0
        for k in ["y"] + names:
            assert not bool(res[k][b, n:].any()), f"{k} row {b} beyond {n}"
    assert all(bool(torch.isfinite(res[k]).all()) for k in res)


# ---- Quartet core -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("uq", [True, False])
@pytest.mark.parametrize("dk", [32, 64])
def test_quartet_core_rows_are_as_alone(dk, uq, prec):
    from mop_amd import _lib, ops
    ts, dy, ref = _qt_case(dk, uq, prec)
    res = _qt_run(ts, dy, uq, _lens(QT_LENS))
    assert ops.LAST_PATH["quartet_fwd"] == (_lib.PATH_FUSED if prec == "bf16" else _lib.PATH_GENERIC)
    _qt_check(res, ref, prec, QT_LENS, uq)


@pytest.mark.parametrize("uq", [True, False])
@pytest.mark.parametrize("dk", [32, 64])
def test_quartet_fused_rows_are_bitwise_the_rows_alone(dk, uq):
    """the fused kernels walk a row of n real tokens exactly as the plain kernels walk the row alone at T = n: same tiles, same
    bounds, same counts, so every tensor of the row is the same bit for bit, on any draw (here one that _qt_case would reject: no
    conditioning is needed to compare a kernel with itself).  The two scalar gradients are sums over the batch, in another order."""
    from mop_amd import _lib, ops
    g = torch.Generator().manual_seed(dk + uq)
    ts = tuple(torch.randn(QT_B, QT_T, QT_H, dk, generator=g).bfloat16() for _ in range(5))
    dy = torch.randn(QT_B, QT_T, QT_H * dk, generator=g).bfloat16()
    res = _qt_run(ts, dy, uq, _lens(QT_LENS))
    assert ops.LAST_PATH["quartet_fwd"] == _lib.PATH_FUSED
    for b, n in enumerate(QT_LENS):
        alone = _qt_run([t[b:b + 1, :n] for t in ts], dy[b:b + 1, :n], uq, None)
        assert ops.LAST_PATH["quartet_fwd"] == _lib.PATH_FUSED
        for k in ("y", "dq", "dk", "dv") + (("dq2", "dk2") if uq else ()):
            assert torch.equal(alone[k][0], res[k][b, :n]), (k, b, n)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_quartet_core_row_of_length_zero(prec):
    from mop_amd import _lib, ops
    lens = (0, 200)
    ts, dy, ref = _qt_case(64, True, prec, lens)
    res = _qt_run(ts, dy, True, _lens(lens))
    assert ops.LAST_PATH["quartet_fwd"] == (_lib.PATH_FUSED if prec == "bf16" else _lib.PATH_GENERIC)
    _qt_check(res, ref, prec, lens, True)
    assert all(not bool(res[k][0].any()) for k in ("y", "dq", "dk", "dv", "dq2", "dk2"))


def test_quartet_need_weights_beyond_a_length_are_zero():
    ts, dy, ref = _qt_case(32, True, "fp32")
    res = _qt_run(ts, dy, True, _lens(QT_LENS), need_weights=True)
    P = res["P"].double().cpu().numpy()
    assert float(np.abs(P - ref["P"]).max()) <= 1e-3
    for b, n in enumerate(QT_LENS):
        assert not P[b, :, n:, :].any() and not P[b, :, :, n:].any()
        assert float(np.abs(P[b, :, :n, :n].sum(-1) - 1).max()) <= 1e-5


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("uq", [True, False])
def test_quartet_core_reads_nothing_beyond_a_length(uq, prec):
    ts, dy, _ = _qt_case(64, uq, prec)
    lens = _lens(QT_LENS)
    a = _qt_run(ts, dy, uq, lens)
    b = _qt_run(ts, dy, uq, lens, poison=float("nan"))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_quartet_full_lengths_are_bitwise_the_call_without_lengths(prec, p):
    ts, dy, _ = _qt_case(64, True, prec)
    for uq in (True, False):
        a = _qt_run(ts, dy, uq, None, seed=77, p=p)
        b = _qt_run(ts, dy, uq, _lens((QT_T,) * QT_B), seed=77, p=p)
        c = _qt_run(ts, dy, uq, _lens((QT_T + 5,) * QT_B), seed=77, p=p)          # values are clamped
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (k, uq)


@pytest.mark.parametrize("uq", [True, False])
def test_quartet_fused_matches_generic_with_lengths(uq):
    """the bounds of test_quartet_fused_matches_generic (tests/test_gpu_siblings.py)"""
    import mop_amd
    from mop_amd import _lib, ops
    mop_amd.set_precision("bf16")
    ts, dy, _ = _qt_case(64, uq, "bf16")
    res = {}
    for path in ("fused", "generic"):
        ops.set_path(path)
        res[path] = _qt_run(ts, dy, uq, _lens(QT_LENS))
        assert ops.LAST_PATH["quartet_fwd"] == (_lib.PATH_FUSED if path == "fused" else _lib.PATH_GENERIC)
    for k, b_ in res["generic"].items():
        a_, b_ = res["fused"][k].float(), b_.float()
        den = max(1.0, float(b_.abs().max())) if k == "y" else max(float(b_.abs().max()), 1e-6)
        assert float((a_ - b_).abs().max()) / den <= (1e-2 if k == "y" else 5e-2), k


# ---- token gate -------------------------------------------------------------------------------------------------------------
TG_TOL = {"bf16": 1e-2, "fp32": 1e-4}    # the bounds of test_token_gate_op_against_float64 (tests/test_gpu_gpt.py)
TG_LENS = (40, 33, 32, 17, 16, 1, 0)   # either side of and on the 16-token tile edges, a lone token, an empty row


def _tg_inputs(B, T, D, dt, with_a, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, D, generator=g).to(dt)
    a = torch.randn(B, T, D, generator=g).to(dt) if with_a else None
    u = 0.05 * torch.randn(3, D, generator=g)
    dout = torch.randn(B, T, D, generator=g).to(dt)
    return x, a, u, dout


def _tg_run(x, a, u, dout, lens, poison=None, embed=False):
    from guarded_alloc import embedded
    from mop_amd import _lib, ops
    xs = [None if t is None else t.cuda().clone() for t in (x, a, dout)]
    if poison is not None:
        for b, n in enumerate(lens.tolist()):
            for t in xs:
                if t is not None:
                    t[b, n:] = poison
    if embed:
        xs, lens = [None if t is None else embedded(t) for t in xs], embedded(lens)
    xr = xs[0].requires_grad_(True)
    ar = None if xs[1] is None else xs[1].requires_grad_(True)
    ur = u.cuda().clone().requires_grad_(True)
    out = ops.token_gate_1d(xr, ar, ur, lens)
    assert ops.LAST_PATH["token_gate_fwd"] == _lib.PATH_FUSED
    out.backward(xs[2])
    return {"out": out.detach(), "dx": xr.grad, "da": None if ar is None else ar.grad, "du": ur.grad}


def _nerr(a, b):
    return float((a.detach().double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("D", [64, 1024])
def test_token_gate_rows_are_as_alone(D, dt, with_a):
    """the bounds of test_token_gate_op_against_float64 (tests/test_gpu_gpt.py)"""
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    tol = TG_TOL[dt]
    x, a, u, dout = _tg_inputs(len(TG_LENS), 40, D, tdt, with_a, seed=D + with_a)
    ro, rdr, rdu = token_gate_rows_alone(x, a, u, TG_LENS, dout)
    lens = _lens(TG_LENS)
    res = _tg_run(x, a, u, dout, lens)
    assert res["out"].dtype == tdt
    assert _nerr(res["out"], ro) <= tol and _nerr(res["dx"], rdr) <= tol and _nerr(res["du"], rdu) <= tol, \
        f"out {_nerr(res['out'], ro):.2e} dx {_nerr(res['dx'], rdr):.2e} du {_nerr(res['du'], rdu):.2e}"
    if with_a:
        assert _nerr(res["da"], rdr) <= tol
    for b, n in enumerate(TG_LENS):
        assert not bool(res["out"][b, n:].any()) and not bool(res["dx"][b, n:].any())
    # nothing beyond a length is read, and the backward is reproducible bit for bit
    for poison in (float("nan"), None):
        again = _tg_run(x, a, u, dout, lens, poison=poison)
        for k, v in res.items():
            assert v is None or torch.equal(v, again[k]), (k, poison)
    # full lengths: bitwise the call without lengths, du included
    full, plain = _tg_run(x, a, u, dout, _lens((40,) * len(TG_LENS))), _tg_run(x, a, u, dout, None)
    for k, v in plain.items():
        assert v is None or torch.equal(v, full[k]), k


def test_token_gate_lengths_beyond_the_partial_rows_of_the_backward():
    """B * ceil(T / 16) = 37 * 15 = 555 tiles > the 512 partial rows: the backward workgroups loop over tiles of different rows"""
    B, T, D = 37, 233, 64
    lens = tuple((7 * b * b + 3) % (T + 1) for b in range(B))
    assert B * ((T + 15) // 16) > 512 and 0 in [n % 16 for n in lens] and max(lens) > 200 and min(lens) < 16
    x, a, u, dout = _tg_inputs(B, T, D, torch.float32, True, seed=9)
    ro, rdr, rdu = token_gate_rows_alone(x, a, u, lens, dout)
    res = _tg_run(x, a, u, dout, _lens(lens))
    assert _nerr(res["out"], ro) <= 1e-4 and _nerr(res["dx"], rdr) <= 1e-4 and _nerr(res["du"], rdu) <= 1e-4
    again = _tg_run(x, a, u, dout, _lens(lens), poison=float("nan"))
    for k, v in res.items():
        assert torch.equal(v, again[k]), k


# ---- models -----------------------------------------------------------------------------------------------------------------
DOCS = (40, 33, 16, 1)


def _model(which):
    from mop_amd.nn import GPT_MoP, TinyTransformerLM, TransformerConfig
    torch.manual_seed(3)
    cfg = TransformerConfig(n_layer=2, n_head=2, n_embd=64, dropout=0.0, block_size=64, use_quartet=not which.endswith("baseline"))
    return (GPT_MoP if which.startswith("mop") else TinyTransformerLM)(97, cfg).cuda().train()


@pytest.mark.parametrize("which", ["mop", "mop_baseline", "quartet", "baseline"])
def test_models_give_every_document_its_own_result(which):
    m = _model(which)
    g = torch.Generator().manual_seed(11)
    docs = [torch.randint(1, 97, (n,), generator=g).cuda() for n in DOCS]
    tgts = [torch.randint(0, 97, (n,), generator=g).cuda() for n in DOCS]
    logits, loss = m(docs, targets=tgts)
    assert logits.shape == (4, 40, 97) and bool(torch.isfinite(logits).all())
    alone = [m(d[None])[0][0].detach() for d in docs]
    err = [float((logits[b, :n].detach() - alone[b]).abs().max()) for b, n in enumerate(DOCS)]
    print(f"{which}: logits of a padded row against the row alone, max-abs (bound 1e-4): {err}")
    assert max(err) <= 1e-4, err
    # without lengths the same padded batch is another function: the comparison notices a `lens` that is dropped
    padded = torch.nn.utils.rnn.pad_sequence(docs, batch_first=True)
    plain = m(padded)[0].detach()
    off = [float((plain[b, :n] - alone[b]).abs().max()) for b, n in enumerate(DOCS)]
    print(f"{which}: the same without lengths: {off}")
    assert max(off[1:]) > 10 * 1e-4, off
    # loss and parameter gradients: the documents alone, each weighted by its share of the targets
    names = [n_ for n_, _ in m.named_parameters()]
    m.zero_grad()
    total = m.loss(docs, tgts)
    total.backward()
    got = {n_: p.grad.detach().double().cpu().numpy() for n_, p in m.named_parameters()}
    assert abs(float(total) - float(loss)) <= 1e-5 * max(1.0, abs(float(loss)))
    want = {n_: 0.0 for n_ in names}
    ntok, lsum = sum(DOCS), 0.0
    for d, t in zip(docs, tgts):
        m.zero_grad()
        li = m.loss(d[None], t[None])
        li.backward()
        lsum += float(li) * len(d) / ntok
        for n_, p in m.named_parameters():
            want[n_] = want[n_] + p.grad.detach().double().cpu().numpy() * (len(d) / ntok)
    assert abs(float(total) - lsum) <= 1e-4 * max(1.0, abs(lsum))
    check_grads(got, want, TOL["fp32"][1], floor=1e-3)


def test_gate_maps_of_a_list_are_those_of_the_documents():
    m = _model("mop").eval()
    g = torch.Generator().manual_seed(12)
    docs = [torch.randint(1, 97, (n,), generator=g).cuda() for n in DOCS]
    with torch.no_grad():
        maps = m.get_gate_maps(docs)
        for b, d in enumerate(docs):
            for got, want in zip(maps, m.get_gate_maps(d[None])):
                assert float((got[b, ..., :len(d)] - want[0]).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


# ---- no host sync, graph capture, guarded allocations --------------------------------------------------------------------
def test_no_host_sync():
    m = _model("mop")
    g = torch.Generator().manual_seed(13)
    docs = [torch.randint(1, 97, (n,), generator=g).cuda() for n in DOCS]
    tgts = [torch.randint(0, 97, (n,), generator=g).cuda() for n in DOCS]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m.loss(docs, tgts).backward()                                       # warm-up outside the check
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.zero_grad()
            m.loss(docs, tgts).backward()
            logits, _ = m(docs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_graph_replay_reproduces_eager(prec):
    """forward + backward of both ops with lengths captured in a HIP graph and replayed on two sets of lengths, against eager, in its
    own process (tools/graph_probe_gpt_lens.py): the fused kernels (bf16) and the generic path (fp32)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_probe_gpt_lens.py"), prec], cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"graph probe ended abnormally (rc {r.returncode}): " + r.stdout[-300:] + r.stderr[-600:]
    assert "CAPTURE_UNSUPPORTED" not in r.stdout, r.stdout[-400:]
    assert "GRAPH_IDENTICAL True" in r.stdout, r.stdout[-600:]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_guarded_quartet_core_with_lengths(prec):
    from guarded_alloc import guarded_allocations
    ts, dy, _ = _qt_case(64, True, prec)
    lens = _lens(QT_LENS)
    want = _qt_run(ts, dy, True, lens)
    with guarded_allocations() as ledger:
        got = _qt_run(ts, dy, True, lens, embed=True)
        torch.cuda.synchronize()
    assert ledger.count() > 0 and ledger.intact(), ledger.describe_damage()
    for k in want:
        assert torch.equal(want[k], got[k]), k


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_guarded_token_gate_with_lengths(dt):
    from guarded_alloc import guarded_allocations
    x, a, u, dout = _tg_inputs(len(TG_LENS), 40, 64, dt, True, seed=21)
    lens = _lens(TG_LENS)
    want = _tg_run(x, a, u, dout, lens)
    with guarded_allocations() as ledger:
        got = _tg_run(x, a, u, dout, lens, embed=True)
        torch.cuda.synchronize()
    assert ledger.count() > 0 and ledger.intact(), ledger.describe_damage()
    for k in want:
        assert torch.equal(want[k], got[k]), k
