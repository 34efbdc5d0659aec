"""What can be said about ops.cross_entropy / ops.linear_cross_entropy and the models' loss() without a device: the signatures, the
torch twin against the float64 reference of ce_rows.py under its derived bounds (so every case is fit to judge a kernel), that the
position cases cannot hide a dropped or doubled element, the library's refusals (the pattern of test_entry_refusals_cpu.py), and
the generic route of the chunked head loss and of loss() on CPU tensors."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn.functional as F

import ce_rows as CR

BAD_SHAPE, BAD_ARG = -1, -2
DTYPES = [torch.float32, torch.bfloat16]
E = inspect.Parameter.empty


def _sig(f):
    return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]


def test_signatures():
    from mop_amd import ops
    from mop_amd.nn import GPT_MoP, WhisperMoP
    from mop_amd.nn.quartet_attn_patch import TinyTransformerLM, _LMBase
    assert _sig(ops.cross_entropy) == [("logits", E), ("targets", E), ("ignore_index", -100), ("reduction", "mean"), ("inplace_backward", False)]
    assert _sig(ops.cross_entropy_supported) == [("logits", E), ("targets", E), ("ignore_index", -100), ("reduction", "mean")]
    assert _sig(ops.cross_entropy_torch) == [("logits", E), ("targets", E), ("ignore_index", -100), ("reduction", "mean")]
    assert _sig(ops.linear_cross_entropy) == [("x", E), ("weight", E), ("targets", E), ("bias", None), ("ignore_index", -100),
                                              ("reduction", "mean"), ("chunk_rows", None)]
    lm = inspect.signature(_LMBase.loss).parameters
    assert list(lm) == ["self", "idx", "targets", "attention_mask", "chunk_rows", "ignore_index"]
    assert lm["chunk_rows"].kind is lm["ignore_index"].kind is inspect.Parameter.KEYWORD_ONLY and lm["ignore_index"].default == -100
    assert GPT_MoP.loss is _LMBase.loss and TinyTransformerLM.loss is _LMBase.loss
    wh = inspect.signature(WhisperMoP.loss).parameters
    assert list(wh) == ["self", "mel", "dec_input_ids", "targets", "chunk_rows", "ignore_index"]
    assert wh["chunk_rows"].kind is inspect.Parameter.KEYWORD_ONLY


def test_functions_live_beside_ops():
    """tests/test_autograd_contract_cpu.py counts the Functions of mop_amd/ops.py; these two live in mop_amd/cross_entropy_fn.py"""
    from mop_amd import cross_entropy_fn, ops
    assert ops._cross_entropy_fn is cross_entropy_fn
    for fn in (cross_entropy_fn._CrossEntropyFn, cross_entropy_fn._LinearCrossEntropyFn):
        assert issubclass(fn, torch.autograd.Function)


def _cases(dtype):
    """every (name, stored logits, targets) the GPU test judges a kernel on, small enough for a CPU"""
    out = []
    for V in CR.lengths(dtype):
        for R in (1, 3):
            x, t = CR.normal(R, V, seed=V + R)
            out.append((f"len-{V}-{R}", CR.stored(x, dtype), t))
    x, t = CR.normal(1031, 33, seed=5)
    out.append(("rows-1031", CR.stored(x, dtype), t))
    x, t = CR.normal(2, 51865, seed=6)
    out.append(("vocab-51865", CR.stored(x, dtype), t))
    for name, (x, t) in CR.value_cases(dtype).items():
        out.append((name, CR.stored(x, dtype), t))
    for name, r, j, x, t, t_on in CR.position_cases(dtype):
        out += [(f"pos-{name}-elsewhere", CR.stored(x, dtype), t), (f"pos-{name}-on", CR.stored(x, dtype), t_on)]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_twin_stays_under_the_bound_on_every_case(dtype):
    from mop_amd import ops
    worst = {}
    for name, x, t in _cases(dtype):
        ref = CR.Ref(x, t)
        got = ops.cross_entropy_torch(x, t, reduction="none")
        assert got.dtype == torch.float32
        want, bound = ref.reduced("none")
        worst[name] = CR.worst(got, want, bound)
        assert worst[name] <= 1.0, (name, worst[name])
    print("largest fraction of the row-loss bound the twin uses:", max(worst.values()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_position_cases_cannot_hide_a_lost_or_doubled_element(dtype):
    """on the reference alone: leaving the marked element out, or counting it twice, moves the loss by more than 10 bounds"""
    cases = CR.position_cases(dtype)
    names = {n.split("-")[0] for n, *_ in cases}
    assert names == {"first", "last", "head_last", "vec0_first", "vec0_last", "vec_last", "sweep0_last", "sweep1_first", "tail_first"}
    for name, r, j, x, t, t_on in cases:
        xs = CR.stored(x, dtype)
        for tt in (t, t_on):
            ref = CR.Ref(xs, tt)
            drop, twice = CR.dropped_and_doubled(xs[r], int(tt[r]), j)
            for moved in (drop, twice):
                assert abs(moved - float(ref.loss[r])) > 10 * float(ref.loss_bound[r]), (name, moved)


def test_flat_rows_would_hide_one():
    """why flat rows guard no position: at V = 51865 one lost element moves lse by about the bound"""
    x = CR.stored(torch.full((1, 51865), 0.25), torch.float32)
    ref = CR.Ref(x, torch.tensor([3]))
    drop, _ = CR.dropped_and_doubled(x[0], 3, 100)
    assert abs(drop - float(ref.loss[0])) < 10 * float(ref.loss_bound[0])


def test_twin_ignores_what_the_kernel_ignores():
    from mop_amd import ops
    x, t = CR.normal(6, 50, seed=1)
    t = torch.tensor([3, -100, 50, -1, 2 ** 40, 7])
    for ii in (-100, 3):
        ref = CR.Ref(x, t, ii)
        for red in ("mean", "sum", "none"):
            want, bound = ref.reduced(red)
            assert CR.worst(ops.cross_entropy_torch(x, t, ii, red), want, bound + 4 * CR.U * want.abs()) <= 1.0
    t_all = torch.full((6,), -100)
    assert torch.isnan(ops.cross_entropy_torch(x, t_all)) and float(ops.cross_entropy_torch(x, t_all, reduction="sum")) == 0.0


def test_value_errors():
    from mop_amd import ops
    x, t = CR.normal(4, 10)
    for f in (ops.cross_entropy, ops.cross_entropy_torch, ops.cross_entropy_supported):
        with pytest.raises(ValueError):
            f(x, t.to(torch.int32))
        with pytest.raises(ValueError):
            f(x, t[:3])
        with pytest.raises(ValueError):
            f(x[:, :1], t)
        with pytest.raises(ValueError):
            f(x, t, reduction="max")
        with pytest.raises(ValueError):
            f(x, t, ignore_index=1.5)
    with pytest.raises(ValueError):
        ops.linear_cross_entropy(x, torch.randn(7, 9), t)
    with pytest.raises(ValueError):
        ops.linear_cross_entropy(x, torch.randn(7, 10), t, chunk_rows=0)
    assert ops.cross_entropy_supported(x, t) is False                 # CPU tensors: the twin's


# ---- the library's refusals, in the pattern of test_entry_refusals_cpu.py ----
@pytest.fixture(scope="module")
def lib():
    from mop_amd import build
    build.build_lib()
    from mop_amd import _lib
    return _lib.lib()


FILL = dict(R=1, V=8, dtype=0, row0=0, n_rows=1, ignore_index=-100, logits_ld=8, dlogits_ld=8, grad_stride=0)
MASKS = {"logits": 3, "targets": 7, "lse": 3, "row_loss": 3, "out": 3, "dlogits": 3, "grad": 3, "scale": 3}
NEEDS = {"mopk_cross_entropy_fwd": ("logits", "targets", "lse", "row_loss"),
         "mopk_cross_entropy_bwd": ("logits", "targets", "lse", "dlogits", "grad")}


def _filled(**kw):
    from mop_amd import _lib
    a = _lib.CrossEntropyArgs()
    ptrs = [n for n, tp in a._fields_ if tp is C.c_void_p]
    assert sorted(ptrs) == sorted(MASKS), "the row must name every pointer field"
    for k, v in {**FILL, **kw}.items():
        setattr(a, k, v)
    addr = {f: 0x100000 + 256 * i for i, f in enumerate(ptrs)}
    for f, p in addr.items():
        setattr(a, f, p)
    return a, addr


def test_query_accepts_the_fill_and_looks_at_each_pointer_at_its_mask(lib):
    a, addr = _filled()
    q = lib.mopk_cross_entropy_supported
    assert q(C.byref(a)) == 1
    for f, mask in MASKS.items():
        for off, want in (((mask + 1) // 2, 0), (mask + 1, 1)):
            setattr(a, f, addr[f] + off)
            assert q(C.byref(a)) == want, f"{f} at +{off} (mask {mask})"
        setattr(a, f, addr[f])
    a, addr = _filled(dtype=1)                                        # bf16: logits and dlogits on 2 bytes
    for f in ("logits", "dlogits"):
        for off, want in ((1, 0), (2, 1)):
            setattr(a, f, addr[f] + off)
            assert q(C.byref(a)) == want
        setattr(a, f, addr[f])
    assert q(None) == 0


@pytest.mark.parametrize("entry", sorted(NEEDS))
def test_entry_refuses_a_missing_pointer_before_any_launch(lib, entry):
    fn = getattr(lib, entry)
    for f in NEEDS[entry]:
        a, _ = _filled()
        setattr(a, f, None)
        assert fn(C.byref(a), None) == BAD_ARG, f
    assert fn(None, None) == BAD_ARG


def test_shapes_dtypes_and_strides_are_refused(lib):
    for kw, code in ((dict(V=1), BAD_SHAPE), (dict(V=0), BAD_SHAPE), (dict(R=0), BAD_SHAPE), (dict(dtype=2), BAD_ARG),
                     (dict(logits_ld=7), BAD_ARG), (dict(dlogits_ld=7), BAD_ARG), (dict(row0=-1), BAD_ARG),
                     (dict(row0=1), BAD_ARG), (dict(grad_stride=-1), BAD_ARG), (dict(reserved=1), BAD_ARG)):
        a, _ = _filled(**kw)
        assert lib.mopk_cross_entropy_supported(C.byref(a)) == 0, kw
        for entry in NEEDS:
            assert getattr(lib, entry)(C.byref(a), None) == code, (entry, kw)


def test_backward_refuses_a_gradient_laid_out_unlike_the_logits(lib):
    """16-byte stores follow the loads' split: dlogits equal to logits modulo 16 bytes, row strides equal modulo a vector"""
    UNSUPPORTED = -3
    a, addr = _filled(R=2, n_rows=2)
    a.dlogits = addr["dlogits"] + 4
    assert lib.mopk_cross_entropy_bwd(C.byref(a), None) == UNSUPPORTED
    a, _ = _filled(R=2, n_rows=2, dlogits_ld=9)
    assert lib.mopk_cross_entropy_bwd(C.byref(a), None) == UNSUPPORTED


# ---- the chunked head loss on its generic route ----
def _head(M=11, D=6, V=23, seed=3, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    w = torch.randn(V, D, generator=g) * 0.5
    b = torch.randn(V, generator=g) * 0.1 if bias else None
    t = torch.randint(0, V, (M,), generator=g)
    t[2] = -100
    return x, w, b, t


@pytest.mark.parametrize("chunk", [1, 3, 11, 16])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_linear_cross_entropy_against_float64(chunk, reduction):
    from mop_amd import _lib, ops
    x, w, b, t = _head()
    ref = CR.Ref(F.linear(x.double(), w.double(), b.double()).float(), t)       # the GEMM's own rounding is judged apart, below
    want64 = F.cross_entropy(F.linear(x.double(), w.double(), b.double()), t, reduction=reduction)
    got = ops.linear_cross_entropy(x, w, t, b, reduction=reduction, chunk_rows=chunk)
    assert ops.LAST_PATH["linear_cross_entropy"] == _lib.PATH_GENERIC
    whole = F.cross_entropy(F.linear(x, w, b), t, reduction=reduction)
    if chunk >= 11:
        assert torch.equal(got, whole)
    _, bound = ref.reduced(reduction)
    err, err_whole = (got.double() - want64).abs(), (whole.double() - want64).abs()
    assert bool((err <= 2 * err_whole.max() + bound).all())


def test_linear_cross_entropy_gradients_retain_graph_and_upstream():
    from mop_amd import ops
    x, w, b, t = _head()
    leaves = [v.clone().requires_grad_() for v in (x, w, b)]
    ref = [v.double().clone().requires_grad_() for v in (x, w, b)]
    F.cross_entropy(F.linear(*ref[:2], ref[2]), t).backward()
    loss = ops.linear_cross_entropy(leaves[0], leaves[1], t, leaves[2], chunk_rows=4)
    g1 = torch.autograd.grad(loss, leaves, retain_graph=True)
    g2 = torch.autograd.grad(loss, leaves, retain_graph=True)
    g3 = torch.autograd.grad(loss * -3.5, leaves)
    for a, a2, a3, r in zip(g1, g2, g3, ref):
        assert torch.equal(a, a2)
        assert float((a.double() - r.grad).abs().max()) <= 1e-5 * float(r.grad.abs().max())
        assert float((a3.double() + 3.5 * r.grad).abs().max()) <= 1e-5 * 3.5 * float(r.grad.abs().max())


# ---- loss() of the three model families on CPU tensors: the attention cores have no CPU route, so a stand-in takes their place
class _Mix(torch.nn.Module):
    def __init__(self, D):
        super().__init__()
        self.lin = torch.nn.Linear(D, D)

    def forward(self, x, *a, **k):
        return torch.tanh(self.lin(x))


def _without_attention(m, D):
    for mod in list(m.modules()):
        for name, child in list(mod.named_children()):
            if type(child).__name__.endswith("Attention"):
                setattr(mod, name, _Mix(D))
    return m


def _lm(kind):
    from mop_amd.nn import GPT_MoP
    from mop_amd.nn.quartet_attn_patch import TinyTransformerLM, TransformerConfig
    torch.manual_seed(0)
    cfg = TransformerConfig(n_layer=2, n_head=2, n_embd=16, block_size=8, dropout=0.0, bias=True)
    m = GPT_MoP(37, cfg, n_views=2, n_kernels=1) if kind == "mop" else TinyTransformerLM(37, cfg)
    return _without_attention(m, 16)


@pytest.mark.parametrize("kind", ["mop", "quartet", "whisper"])
def test_model_loss_is_forwards_loss_on_cpu(kind):
    from mop_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    if kind == "whisper":
        from mop_amd.nn import WhisperConfig, WhisperMoP
        torch.manual_seed(0)
        m = _without_attention(WhisperMoP(WhisperConfig(n_mels=10, n_audio_ctx=40, vocab_size=37, n_text_ctx=8, n_embd=16, n_head=2,
                                                        n_layer_enc=1, n_layer_dec=2)), 16)
        args = (torch.randn(2, 12, 10, generator=g), torch.randint(0, 37, (2, 8), generator=g))
        targets = torch.randint(0, 37, (2, 8), generator=g)
        fwd = lambda: m(*args, targets)[1]                              # noqa: E731
        loss = lambda c: m.loss(*args, targets, chunk_rows=c)[0]        # noqa: E731
        assert torch.equal(m.loss(*args, targets)[1], m(*args, targets)[2])
    else:
        m = _lm(kind)
        idx, targets = torch.randint(0, 37, (2, 8), generator=g), torch.randint(0, 37, (2, 8), generator=g)
        fwd = lambda: m(idx, targets=targets)[1]                        # noqa: E731
        loss = lambda c: m.loss(idx, targets, chunk_rows=c)             # noqa: E731
    targets[0, 3] = -100
    want = fwd()
    assert torch.equal(loss(16), want) and torch.equal(loss(None), want)
    assert ops.LAST_PATH["linear_cross_entropy"] == _lib.PATH_GENERIC
    logits = m(*args)[0] if kind == "whisper" else m(idx)[0]
    ref = CR.Ref(logits.detach().reshape(16, 37), targets.reshape(16))
    _, bound = ref.reduced("mean")
    assert abs(float(loss(5).detach()) - float(want.detach())) <= 2 * float(bound)
    gw = torch.autograd.grad(want, m.lm_head.weight)[0]
    gl = torch.autograd.grad(loss(5), m.lm_head.weight)[0]
    assert float((gw - gl).abs().max()) <= 1e-5 * float(gw.abs().max())
