"""-m gpu: the MoE router, scan and grouped GEMMs on routes the test chooses (tests/moe_ref.py), never on the kernel's own pick.
  router: moe_logits_kernel's argmax against the float64 argmax under the rounding bound beta of moe_ref.route_ref64, its ties and
          start value bit for bit, and its logits themselves, read out of the argmax by bisection;
  scan:   the whole route buffer [expert | perm | offsets] of mopk_moe_route against a stable sort and a bincount;
  GEMMs:  ops.moe_mlp forward and backward at per-expert counts on the 64 / 128-row tile edges, the 256 / 512-row weight-gradient
          chunk edges and the attained grid bound ceil(M / TM) + E - 1, at widths with a K-tail, against test_gpu_moe._ref64 under
          the prescribed route and the sweep's own tolerances;
  dtypes: the sixteen combinations of x, expert-weight and gate dtype with and without autocast: which the kernels take, and each
          taken one against float64."""
import functools

import pytest
import torch

import moe_ref as R
from gpu_util import check_grads
from test_gpu_moe import _ref64

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _reset():
    import mop_amd
    from mop_amd import ops
    yield
    mop_amd.set_precision("auto")
    ops.set_path("auto")


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


# ---- 2. the router against float64 ----
@functools.lru_cache(maxsize=None)
def _router_ref(case):
    x, gw, gb = R.router_case(*case)
    logits, beta = R.route_ref64(x, gw, gb)
    return x, gw, gb, logits, beta


@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=R.case_id)
def test_router_picks_the_float64_argmax(case):
    """a decided token gets the float64 argmax; an undecided one an expert within beta_top1 + beta_e of the top"""
    from mop_amd import ops
    x, gw, gb, logits, beta = _router_ref(case)
    top1, decided = R.decide(logits, beta)
    share = 1.0 - float(decided.double().mean())
    assert share <= R.UNDECIDED_CAP, f"the case is not fit to judge a router: undecided share {share:.4%}"
    got = ops.moe_route(*_cuda(x, gw, gb)).cpu().long()
    assert got.shape == top1.shape
    wrong = (got != top1) & decided
    assert not bool(wrong.any()), f"{int(wrong.sum())} decided tokens off the float64 argmax, first {wrong.nonzero()[:4].flatten().tolist()}"
    assert bool(((got >= 0) & (got < case[2])).all())
    assert bool(R.admissible(logits, beta, got).all()), "an undecided token went to an expert outside the bound"


def _route(x, gw, gb):
    from mop_amd import ops
    return ops.moe_route(*_cuda(x, gw, gb)).cpu().tolist()


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["gfp32", "gbf16"])
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["xfp32", "xbf16"])
@pytest.mark.parametrize("E,D", [(8, 72), (64, 384), (2, 8)])
def test_equal_gate_rows_go_to_the_lower_index(E, D, xdt, gdt):
    """equal operands give equal fp32 sums, so duplicated rows tie exactly and torch.argmax's rule applies: the lowest index"""
    g = torch.Generator().manual_seed(E)
    M = 67
    x = torch.randn(M, D, generator=g).to(xdt)
    gw = (torch.randn(E, D, generator=g) / D ** 0.5).to(gdt)
    gb = (0.1 * torch.randn(E, generator=g)).to(gdt)
    lift = (3.0 * torch.randn(D, generator=g) / D ** 0.5).to(gdt)      # a row every token prefers once its bias is 100
    for lo, hi in sorted({(0, 1), (E - 2, E - 1)}):
        w, b = gw.clone(), gb.clone()
        w[lo] = w[hi] = lift
        b[lo] = b[hi] = 100.0
        assert _route(x, w, b) == [lo] * M, (lo, hi)
        r = _route(x, w, None)                   # without the bias the pair leads for some tokens only: never the upper one
        assert lo in r and hi not in r, (lo, hi)
    w = lift.repeat(E, 1)
    assert _route(x, w, torch.full((E,), 0.5).to(gdt)) == [0] * M
    assert _route(x, w, None) == [0] * M


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["gfp32", "gbf16"])
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["xfp32", "xbf16"])
def test_start_value_and_last_expert(xdt, gdt):
    g = torch.Generator().manual_seed(9)
    D = 72
    x0 = torch.zeros(5, D).to(xdt)
    gw3 = torch.randn(3, D, generator=g).to(gdt)
    assert _route(x0, gw3, None) == [0] * 5                            # every logit 0: the first
    # every logit negative: the argmax starts from expert 0's logit, not from 0
    assert _route(x0, gw3, torch.tensor([-50.0, -10.0, -30.0]).to(gdt)) == [1] * 5
    assert _route(x0, gw3, torch.tensor([-10.0, -50.0, -30.0]).to(gdt)) == [0] * 5
    xn = -torch.ones(5, D).to(xdt)                                     # negative through the products too, no bias
    wn = torch.ones(3, D).to(gdt) * torch.tensor([4.0, 1.0, 2.0]).reshape(3, 1).to(gdt)
    assert _route(xn, wn, None) == [1] * 5
    # the largest logit at the last of 64 experts, by the bias and by the products
    E = 64
    x = torch.randn(131, D, generator=g).to(xdt)
    gw = (torch.randn(E, D, generator=g) / D ** 0.5).to(gdt)
    gb = torch.zeros(E).to(gdt)
    gb[E - 1] = 64.0
    assert _route(x, gw, gb) == [E - 1] * 131
    xp, pw, pb = R.prescribed_gate(torch.full((131,), E - 1), D, E, gdt)
    assert _route(R.patched(x, xp), pw, pb) == [E - 1] * 131
    assert _route(R.patched(x, xp), pw, None) == [E - 1] * 131


def _kernel_logits(x, w0, b0, gdt):
    """the logits kernel's own fp32 value of x[t] . w0 + b0 per token, read out of its argmax.  Two experts: row 0 is w0 with a zero
    in the last column, row 1 is the unit vector of that column with bias 0, so logit 1 is x[t, D - 1] exactly (one lane holds
    fma(x, 1, 0), the other partial sums and the bias are zeros) and that column adds nothing to logit 0.  The strict comparison
    picks expert 1 iff x[t, D - 1] > logit 0: a bisection over the fp32 values of that column, all tokens at once, ends at the
    largest value that does not win, which is logit 0 itself."""
    from mop_amd import ops
    M, D = x.shape
    gw = torch.zeros(2, D)
    gw[0], gw[1, D - 1] = w0, 1.0
    gw[0, D - 1] = 0.0
    gw = gw.to(gdt).cuda()
    gb = None if b0 is None else torch.tensor([b0, 0.0]).to(gdt).cuda()
    x = x.clone().cuda()

    def val(key):               # ordered key -> fp32: int32 order equals float order once negative patterns are flipped
        k = key.to(torch.int32)
        return torch.where(k >= 0, k, k ^ 0x7FFFFFFF).view(torch.float32)

    def key_of(v):
        k = torch.tensor([v], dtype=torch.float32).view(torch.int32).long()
        return int(torch.where(k >= 0, k, k ^ 0x7FFFFFFF))
    lo = torch.full((M,), key_of(-1e30), dtype=torch.int64, device="cuda")     # never wins
    hi = torch.full((M,), key_of(1e30), dtype=torch.int64, device="cuda")      # always wins
    for i, k in enumerate((lo, hi)):
        x[:, D - 1] = val(k)
        assert bool((ops.moe_route(x, gw, gb) == i).all())
    for _ in range(33):
        mid = lo + (hi - lo) // 2
        x[:, D - 1] = val(mid)
        won = ops.moe_route(x, gw, gb) == 1
        hi = torch.where(won, mid, hi)
        lo = torch.where(won, lo, mid)
    assert bool((hi - lo == 1).all())
    return val(lo).double().cpu(), gw.cpu(), None if gb is None else gb.cpu()


@pytest.mark.parametrize("M,D,gdt,bias,seed", [
    (4099, 384, F32, True, 0), (257, 8, F32, True, 2), (2049, 1024, F32, True, 3), (3001, 72, BF16, True, 1),
    (1025, 136, F32, False, 6), (5, 64, F32, True, 7)],
    ids=lambda v: {F32: "gfp32", BF16: "gbf16"}.get(v, str(v)))
def test_kernel_logits_stay_inside_beta(M, D, gdt, bias, seed):
    """the number the router bound rests on: the kernel's fp32 logit against float64, as a fraction of beta (fp32 x, so that the
    probing column takes every fp32 value).  Measured on an MI355X: 0.24 beta at D = 8, 0.13 at D = 72, 0.06 at D = 136, 0.04 at
    D = 384, 0.02 at D = 1024 (an fp32 torch F.linear of the router cases: up to 0.44 beta)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    w0 = torch.randn(D, generator=g) / D ** 0.5
    b0 = float(0.1 * torch.randn(1, generator=g)) if bias else None
    got, gw, gb = _kernel_logits(x, w0, b0, gdt)
    logits, beta = R.route_ref64(x, gw[:1], None if gb is None else gb[:1])
    ratio = ((got - logits[:, 0]).abs() / beta[:, 0]).max()
    print(f"kernel logit error M={M} D={D}: {float(ratio):.3f} beta")
    assert float(ratio) <= 1.0


# ---- 3. the scan, read directly ----
def _route_buffer(x, gw, gb):
    """mopk_moe_route called the way ops.moe_route builds its arguments, the whole [expert (M) | perm (M) | offsets (E + 1)] kept"""
    from mop_amd import _lib as L, ops
    a = L.MoeArgs()
    a.M, a.D, a.F, a.E, a.precision = x.shape[0], x.shape[1], 8, gw.shape[0], L.PREC_BF16
    a.x_dtype = a.w_dtype = a.o_dtype = ops._io_dtype(x)
    a.gate_dtype = ops._io_dtype(gw)
    buf = ops._moe_route_buf(a.M, a.E, x.device)
    buf.fill_(-7)
    a.x, a.gate_w, a.gate_b, a.route = x.data_ptr(), gw.data_ptr(), ops._ptr(gb), buf.data_ptr()
    ops._launch("mopk_moe_route", a)
    torch.cuda.synchronize()
    return buf.cpu().long()


def _scan_routes(M, E):
    g = torch.Generator().manual_seed(M + E)
    t = torch.arange(M)
    yield "random", torch.randint(0, E, (M,), generator=g)
    for name, e in (("first", 0), ("middle", E // 2), ("last", E - 1)):
        yield name, torch.full((M,), e)
    yield "round_robin", t % E
    yield "descending_blocks", (E - 1 - (t * E) // M).clamp(0, E - 1)


@pytest.mark.parametrize("E", [2, 64])
@pytest.mark.parametrize("M", [1, 2, 255, 256, 257, 511, 512, 513, 4099, 65537])
def test_scan_is_a_stable_counting_sort(M, E):
    """256 threads own ceil(M / 256) tokens each: M on both sides of one and two tokens per thread, and far beyond"""
    D = 8                                                              # E = 2: unit rows; E = 64 > D: the one-coordinate code
    x0 = torch.randn(M, D, generator=torch.Generator().manual_seed(M))
    for name, route in _scan_routes(M, E):
        xp, gw, gb = R.prescribed_gate(route, D, E, F32)
        buf = _route_buffer(*_cuda(R.patched(x0, xp), gw, gb))
        assert buf.numel() == 2 * M + E + 1
        assert torch.equal(buf[:M], route), name
        assert torch.equal(buf[M:2 * M], torch.sort(route, stable=True).indices), f"perm, {name}"
        counts = torch.bincount(route, minlength=E)
        assert torch.equal(buf[2 * M:2 * M + E], counts.cumsum(0) - counts), f"offsets, {name}"
        assert int(buf[2 * M + E]) == M, name


# ---- 4. grouped GEMMs at prescribed counts ----
def _mlp_inputs(route, E, D, F_, xdt, wdt, gdt, seed):
    """x, a gate that realises `route`, expert weights and the upstream gradient's fp32 draw, on the GPU"""
    M = route.numel()
    g = torch.Generator().manual_seed(seed)
    xp, gw, gb = R.prescribed_gate(route, D, E, gdt)
    x = R.patched(torch.randn(M, D, generator=g).to(xdt), xp).cuda().requires_grad_(True)
    w1s = [(torch.randn(F_, D, generator=g) / D ** 0.5).to(wdt).cuda().requires_grad_(True) for _ in range(E)]
    w2s = [(torch.randn(D, F_, generator=g) / F_ ** 0.5).to(wdt).cuda().requires_grad_(True) for _ in range(E)]
    dy, res = torch.randn(M, D, generator=g).cuda(), torch.randn(M, D, generator=g).cuda()
    return x, gw.cuda(), gb.cuda(), w1s, w2s, dy, res


def _mlp_check(route, E, D, F_, xdt, wdt, gdt, autocast, seed, with_res=False):
    """ops.moe_mlp forward + backward (fused) on a gate that realises `route`, against _ref64 under `route` on operands rounded as
    the precision stages them, with the sweep's tolerances; an expert without tokens gets exact zeros"""
    from mop_amd import _lib, ops
    x, gw, gb, w1s, w2s, dy, res = _mlp_inputs(route, E, D, F_, xdt, wdt, gdt, seed)
    bf = autocast or xdt == BF16
    odt = BF16 if bf else F32
    dy = dy.to(odt)
    r = res.to(odt).requires_grad_(True) if with_res else None
    assert torch.equal(ops.moe_route(x, gw, gb).cpu().long(), route), "the gate does not realise the prescribed route"
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        assert ops.moe_supported(x, gw, gb, w1s, w2s)
        y = ops.moe_mlp(x, gw, gb, w1s, w2s, residual=r)
    assert y.dtype == odt
    y.backward(dy)
    assert ops.LAST_PATH["moe_fwd"] == _lib.PATH_FUSED and ops.LAST_PATH["moe_bwd"] == _lib.PATH_FUSED
    assert x.grad.dtype == xdt and all(w.grad.dtype == wdt for w in w1s + w2s)
    q = lambda t: t.detach().to(BF16 if bf else F32)
    y64, dx64, dw1, dw2 = _ref64(q(x), gw, gb, [q(w) for w in w1s], [q(w) for w in w2s], route.cuda(), dy,
                                 None if r is None else r.detach())
    tol = 2e-2 if bf else 2e-5
    err = float((y.detach().double().reshape(y64.shape) - y64).abs().max())
    assert err <= tol * max(1.0, float(y64.abs().max())), f"y {err:.3e}"
    got, ref = {"dx": x.grad.double().reshape(dx64.shape)}, {"dx": dx64}
    for e in range(E):
        got[f"w1.{e}"], ref[f"w1.{e}"] = w1s[e].grad.double(), dw1[e]
        got[f"w2.{e}"], ref[f"w2.{e}"] = w2s[e].grad.double(), dw2[e]
    check_grads({k: v.cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in ref.items()}, 3e-2 if bf else 1e-4)
    if with_res:
        assert torch.equal(r.grad, dy)
    counts = torch.bincount(route, minlength=E).tolist()
    for e in range(E):
        if counts[e] == 0:
            assert not bool(w1s[e].grad.any()) and not bool(w2s[e].grad.any()), f"expert {e} has no tokens"


SHAPES = [(72, 40), (8, 104), (136, 264)]      # (D, F): an 8-wide K-tail both ways; E > D and F % 32 = 8; one vector past 128
MODES = {"fp32": (F32, F32, False), "bf16": (BF16, BF16, False), "autocast": (F32, F32, True)}
COUNTS = [
    (0, 1, 63, 64, 65, 0, 127, 128, 129, 0),   # the 64-row (FC2, DX; all of fp32) and 128-row (FC1, DU) tile edges
    (1, 1, 1, 61),                             # sum_e ceil(c_e / TM) = ceil(M / TM) + E - 1: TM = 64, M = 64
    (1, 1, 1, 125),                            # ... TM = 128, M = 128
    (65, 65, 65, 61),                          # ... TM = 64, M = 256
    (0, 70, 0, 0, 58, 0),                      # empty experts at both ends
    (255, 257), (256, 256), (257, 1, 254), (0, 513),   # weight-gradient chunk edges (chunk = 256 while M <= 4096)
    (511, 513, 3076),                          # M = 4100: chunk = 512
]
ATTAINED = {(1, 1, 1, 61): 64, (1, 1, 1, 125): 128, (65, 65, 65, 61): 64}     # counts -> the TM whose grid bound they attain


def _count_cases():
    out = []
    for i, counts in enumerate(COUNTS):
        for j, mode in enumerate(MODES):
            for k, order in enumerate(("sorted", "shuffled")):
                D, F_ = SHAPES[1] if sum(counts) > 4096 else SHAPES[(i + j + k) % 3]
                out.append(pytest.param(counts, order, mode, D, F_, id=f"{'_'.join(map(str, counts))}-{order}-{mode}-D{D}-F{F_}"))
    return out


COUNT_CASES = _count_cases()
# every shape meets every mode
assert {(p.values[2], p.values[3]) for p in COUNT_CASES} == {(m, s[0]) for m in MODES for s in SHAPES}


@pytest.mark.parametrize("counts,order,mode,D,F_", COUNT_CASES)
def test_grouped_gemms_at_prescribed_counts(counts, order, mode, D, F_):
    xdt, wdt, autocast = MODES[mode]
    route = R.counts_to_route(counts, order, seed=len(counts))
    E = len(counts)
    # tiles of TM rows laid end to end never exceed the grid: attained by the three "bound" vectors
    for TM in (64, 128):
        tiles, bound = sum(-(-c // TM) for c in counts), -(-route.numel() // TM) + E - 1
        assert tiles <= bound and (tiles == bound or ATTAINED.get(counts) != TM)
    _mlp_check(route, E, D, F_, xdt, wdt, wdt, autocast, seed=sum(counts), with_res=order == "shuffled")


# ---- 5. the accepted dtype table ----
@pytest.mark.parametrize("autocast", [False, True], ids=["plain", "autocast"])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["gfp32", "gbf16"])
@pytest.mark.parametrize("wdt", [F32, BF16], ids=["wfp32", "wbf16"])
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["xfp32", "xbf16"])
def test_dtype_table(xdt, wdt, gdt, autocast):
    """without autocast x and the expert weights share a dtype and the gate is free; under bf16 autocast all eight pass: twelve of
    sixteen.  A refused mix takes the torch composition, where torch refuses it as nn.Linear does (mat1 / mat2 dtypes)"""
    from mop_amd import _lib, ops
    route = R.counts_to_route((1, 0, 64), "shuffled", seed=5)
    if autocast or xdt == wdt:
        _mlp_check(route, 3, 72, 40, xdt, wdt, gdt, autocast, seed=11)
        return
    x, gw, gb, w1s, w2s, dy, _ = _mlp_inputs(route, 3, 72, 40, xdt, wdt, gdt, seed=11)
    assert not ops.moe_supported(x, gw, gb, w1s, w2s)
    ops.LAST_PATH["moe_fwd"] = ops.LAST_PATH["moe_bwd"] = None
    with pytest.raises(RuntimeError, match="dtype"):
        ops.moe_mlp(x, gw, gb, w1s, w2s)
    assert ops.LAST_PATH["moe_fwd"] == _lib.PATH_GENERIC and ops.LAST_PATH["moe_bwd"] == _lib.PATH_GENERIC
