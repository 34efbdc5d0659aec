"""torch.autograd bridges from tensors to the C ABI (include/mopk.h).

PyTorch is plumbing here: it owns device memory (caching allocator), the current
HIP stream and the autograd graph.  Every attention core runs in libmopk.so; a CPU
tensor or a missing library raises -- there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib as L

_PRECISION = "auto"  # "auto": fp32 tensors -> exact fp32 kernels, bf16 tensors -> bf16 MFMA


def set_precision(p: str) -> None:
    """'auto' | 'fp32' | 'bf16' -- arithmetic of the contractions (MopkPrecision)."""
    global _PRECISION
    if p not in ("auto", "fp32", "bf16"):
        raise ValueError(p)
    _PRECISION = p


def get_precision() -> str:
    return _PRECISION


_PATH = L.PATH_AUTO


def set_path(p: str) -> None:
    global _PATH
    _PATH = {"auto": L.PATH_AUTO, "generic": L.PATH_GENERIC, "fused": L.PATH_FUSED}[p]


def _prec_for(dtype: torch.dtype) -> int:
    if _PRECISION == "fp32":
        return L.PREC_FP32
    if _PRECISION == "bf16":
        return L.PREC_BF16
    return L.PREC_BF16 if dtype == torch.bfloat16 else L.PREC_FP32


def _io_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.MOPK_F32
    if t.dtype == torch.bfloat16:
        return L.MOPK_BF16
    raise TypeError(f"mop_amd supports float32 / bfloat16 tensors, got {t.dtype}")


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what}: mop_amd runs on MI355X (ROCm) tensors only; got a {t.device} tensor. "
            "There is no CPU fallback -- move the module and inputs to 'cuda'.")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> C.c_void_p:
    """the current stream's handle.  torch.cuda.current_stream() costs ~20 us of host time per call (device-index plumbing + a Stream
    object); the raw accessor behind it ~1 us -- these wrappers are called once or twice per layer and step"""
    if _RAW_STREAM is not None:
        return C.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _once_differentiable(backward):
    """torch's once_differentiable for a backward made of kernel launches, whose outputs carry no graph: differentiating them again
    raises instead of contributing nothing.  torch hangs its error node on the outputs only when an incoming gradient requires
    grad, but these gradients depend on the saved inputs as well (a gradient penalty on d y.sum() / dx meets a gradient of ones),
    so under create_graph -- grad mode is on inside a backward only then -- one incoming gradient goes on as a leaf that requires
    grad (the same storage, no copy)."""
    marked = once_differentiable(backward)

    @functools.wraps(backward)
    def wrapper(ctx, *grads):
        if torch.is_grad_enabled() and not any(isinstance(g, torch.Tensor) and g.requires_grad for g in grads):
            grads = list(grads)
            for i, g in enumerate(grads):
                if isinstance(g, torch.Tensor):
                    grads[i] = g.detach().requires_grad_()
                    break
        return marked(ctx, *grads)
    return wrapper


def _grad_in(dy: torch.Tensor, dtype: torch.dtype, shape=None) -> torch.Tensor:
    """an incoming gradient as the kernels read it: contiguous, of the core's dtype and on a 16-byte boundary, viewed as `shape`.
    Autograd may hand a backward an expanded (stride-0) tensor, a slice of a wider buffer, another dtype, or a contiguous tensor
    whose storage offset puts it off the boundary (`.contiguous()` returns that one unchanged); each is copied into a fresh
    tensor (the allocator's blocks are aligned), anything else is passed on as it is."""
    if dy.dtype != dtype or not dy.is_contiguous() or dy.data_ptr() % 16:
        src, dy = dy, torch.empty(dy.shape, dtype=dtype, device=dy.device)
        dy.copy_(src)
    return dy if shape is None or tuple(shape) == tuple(dy.shape) else dy.view(shape)


def _f32_pack(ts):
    """fp32 contiguous copies of several small parameter tensors.  fp32 inputs are used as they are; otherwise ONE
    concatenation + ONE conversion kernel serve all of them (views of a single buffer) instead of one cast kernel each."""
    if all(t.dtype == torch.float32 for t in ts):
        return [t.detach().contiguous() for t in ts]
    if len({t.dtype for t in ts}) != 1:
        return [_f32c(t) for t in ts]
    flat = torch.cat([t.detach().reshape(-1) for t in ts]).to(torch.float32)
    out, o = [], 0
    for t in ts:
        out.append(flat[o:o + t.numel()].view(t.shape))
        o += t.numel()
    return out


# ---- optional kernel timing (bench.py): HIP events on the stream the kernels are launched on ----
LAST_PATH = {}  # entry point -> MopkPath actually requested on the last call (tests assert on it)
_KEEP_WS = bool(__import__("os").environ.get("MOPK_STAMPS"))  # stamp builds only: keep the last workspace tensors alive for read-back
_TIMING = None  # dict name -> list[(start_event, stop_event)] when enabled


def enable_timing(on: bool = True) -> None:
    global _TIMING
    _TIMING = {} if on else None


def timing_results() -> dict:
    """name -> list of elapsed milliseconds (call after torch.cuda.synchronize())."""
    if _TIMING is None:
        return {}
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in _TIMING.items()}


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _TIMING is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()  # current stream == the stream passed to libmopk

    def __exit__(self, *exc):
        if _TIMING is not None:
            self.b.record()
            _TIMING.setdefault(self.name, []).append((self.a, self.b))
        return False


def _launch(sym: str, a, key: Optional[str] = None) -> None:
    """libmopk's `sym` on the args struct `a` and the current stream; with timing on, HIP events around it under `key`
    (None: never timed)"""
    fn = getattr(L.lib(), sym)
    if _TIMING is None or key is None:
        rc = fn(C.byref(a), _stream())
    else:
        with _timed(key):
            rc = fn(C.byref(a), _stream())
    L.check(rc, sym)


def _bytes(n: int, dev) -> torch.Tensor:
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device=dev)


# --------------------------------------------------------------------------------------
# EdgewiseMSA low-rank core
# --------------------------------------------------------------------------------------
def _ew_views(args: L.EdgewiseArgs, qkv: torch.Tensor, prefix: str):
    """qkv: (B,N,Vq,3,H,dk) contiguous. Fills q/k/v0/vL (or dq/dk_/dv0/dvL) views."""
    B, N, Vq, three, H, dk = qkv.shape
    es = 1  # strides below are in elements
    s_n = Vq * 3 * H * dk
    s_b = N * s_n
    s_v = 3 * H * dk if Vq > 1 else 0
    base = qkv.data_ptr()
    isz = qkv.element_size()
    qn, kn, v0n, vLn = (("q", "k", "v0", "vL") if prefix == "" else ("dq", "dk_", "dv0", "dvL"))
    setattr(args, qn, L.View5(base, s_v, s_b, dk * es, s_n))
    setattr(args, kn, L.View5(base + H * dk * isz, s_v, s_b, dk, s_n))
    setattr(args, v0n, L.View4(base + 2 * H * dk * isz, s_b, dk, s_n))
    last = (Vq - 1) * 3 * H * dk
    setattr(args, vLn, L.View4(base + (last + 2 * H * dk) * isz, s_b, dk, s_n))


def _ew_args(qkv, y, V, r, prec, path, beta_not=0.0, drop=(0.0, 0), small=None, head=None,
             mask=(None, (0, 0, 0))) -> L.EdgewiseArgs:
    """the MopkEdgewiseArgs fields forward and backward share.  y: the (B,N,H,dk) output, or a non-null stand-in where the call
    writes none; small: float32 (sqk, vs0, vsL, chain_logit), None in a support query; head: the low-rank head's float32
    (Wr, br, Wc, bc), None otherwise; mask: (uint8 mask or None, strides) from _mask_u8"""
    B, N, _, _, H, dk = qkv.shape
    a = L.EdgewiseArgs()
    a.B, a.H, a.N, a.dk, a.V, a.r = B, H, N, dk, V, r
    a.io_dtype, a.precision, a.path, a.beta_not = _io_dtype(qkv), prec, path, float(beta_not)
    a.dropout_p, a.dropout_seed = float(drop[0]), int(drop[1])
    a.mask, (a.mask_sb, a.mask_sh, a.mask_si) = _ptr(mask[0]), mask[1]
    _ew_views(a, qkv, "")
    a.y = L.View4(y.data_ptr(), N * H * dk, dk, H * dk)
    if small is not None:
        a.sqk, a.vs0, a.vsL, a.chain_logit = map(torch.Tensor.data_ptr, small)
    if head is not None:
        a.Wr, a.br, a.Wc, a.bc = map(torch.Tensor.data_ptr, head)
    return a


_SAVE_CHAIN_STATE = True


def set_save_chain_state(on: bool) -> None:
    """Fused EdgewiseMSA training forward: export chain prefix products / softmax constants for the backward
    (faster backward, ~1 MB per (b,h) of extra activation memory at N=197, V=5) or let the backward recompute them."""
    global _SAVE_CHAIN_STATE
    _SAVE_CHAIN_STATE = bool(on)


def _ew_lowrank_fwd(ctx, qkv, f, beta_not, V, prec, path, want_bwd, drop, lens_w=None, lens_dil=()):
    """the low-rank core's forward launch, shared by _EdgewiseLowrankFn and _EdgewiseSharedFn.  f: the float32 small tensors by name
    (sqk, vs0, vsL, Wr, br, Wc, bc, logit).  Returns y (B,N,H,dk) and the tensors the backward launch needs (qkv, saved, *f, *extras);
    sets ctx.meta / ctx.lens_*."""
    _require_gpu(qkv, "EdgewiseMSA")
    lib = L.lib()
    B, N, Vq, _, H, dk = qkv.shape
    dev = qkv.device
    n_extra = 0 if lens_w is None else int(lens_w.shape[0] * lens_w.shape[1])
    r = f["Wr"].shape[0] // 4
    y = torch.empty(B, N, H, dk, dtype=qkv.dtype, device=dev)
    a = _ew_args(qkv, y, V, r, prec, path, beta_not, drop, (f["sqk"], f["vs0"], f["vsL"], f["logit"]),
                 (f["Wr"], f["br"], f["Wc"], f["bc"]))
    extras = ()
    ctx.lens_dil, ctx.lens_dtype = tuple(lens_dil), (None if lens_w is None else lens_w.dtype)
    if n_extra:
        lens_w = _f32c(lens_w)
        row_x, col_x = lens_means_hip(qkv, f["sqk"], lens_w, lens_dil)
        extras = (row_x, col_x, lens_w)
        ext = _extra_ext(n_extra, row_x, col_x)
        a.ext = C.pointer(ext)
        if path == L.PATH_GENERIC or not lib.mopk_edgewise_fused_supported(C.byref(a)):
            raise NotImplementedError("extra feature channels are an input of the fused Edgewise kernels only")
        path = L.PATH_FUSED
    if path == L.PATH_AUTO:   # AUTO: fused gfx950 kernels when they cover the shape, generic otherwise
        path = L.PATH_FUSED if lib.mopk_edgewise_fused_supported(C.byref(a)) else L.PATH_GENERIC
    a.path = path
    # training forward of the fused path also exports the chain state its backward would otherwise recompute
    a.save_for_backward = int(bool(want_bwd) and path == L.PATH_FUSED and _SAVE_CHAIN_STATE)
    LAST_PATH["edgewise_fwd"] = path
    saved = _bytes(lib.mopk_edgewise_saved_bytes(C.byref(a)), dev)
    ws = _bytes(256 if path == L.PATH_FUSED else lib.mopk_edgewise_workspace_bytes(C.byref(a)), dev)
    a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
    if _KEEP_WS:
        LAST_PATH["_fwd_ws"] = ws  # diagnostics only (stamp builds read it back): pins the buffer until the next call
    _launch("mopk_edgewise_lowrank_fwd", a, "edgewise_fwd")
    ctx.meta = (beta_not, V, prec, path, r, int(a.save_for_backward), drop)
    return y, (qkv, saved, *f.values(), *extras)


def _ew_lowrank_bwd(ctx, dy, core_saved, head_grads):
    """the low-rank core's backward launch on what _ew_lowrank_fwd returned.  head_grads: float32 (dWr, dbr, dWc, dbc) to write.  Returns the argument struct (its *_part pointers
    are what the batch reduction reads), dqkv, the gradients of the extra channels (or None) and the tensors that own the
    partial sums (keep them alive until the reduction is launched)."""
    lib = L.lib()
    qkv, saved, sqk, vs0, vsL, Wr, br, Wc, bc, logit, *extras = core_saved
    beta_not, V, prec, path, r, sfb, drop = ctx.meta
    B, N, Vq, _, H, dk = qkv.shape
    dev = qkv.device
    dy = _grad_in(dy, qkv.dtype)
    # a.y = dy: unused by bwd, must be non-null
    a = _ew_args(qkv, dy, V, r, prec, path, beta_not, drop, (sqk, vs0, vsL, logit), (Wr, br, Wc, bc))
    a.save_for_backward = sfb
    a.dy = L.View4(dy.data_ptr(), N * H * dk, dk, H * dk)
    # unshared: only v of view 0 and V-1 receive gradient -> zero-fill the rest
    dqkv = (torch.empty_like(qkv) if Vq == 1 else torch.zeros_like(qkv))
    _ew_views(a, dqkv, "d")
    n_extra = extras[0].shape[2] if extras else 0
    d_extras = None
    if n_extra:
        d_extras = (torch.empty_like(extras[0]), torch.empty_like(extras[1]))
        ext = _extra_ext(n_extra, extras[0], extras[1])
        ext.d_row_extra, ext.d_col_extra = d_extras[0].data_ptr(), d_extras[1].data_ptr()
        a.ext = C.pointer(ext)
    # per-batch partials of the small gradients
    n_sqk, n_vs = V * H * dk, H * dk
    parts = torch.empty(B * (n_sqk + 2 * n_vs + H), dtype=torch.float32, device=dev)
    dsqk_p, dvs0_p, dvsL_p, dlg_p = torch.split(parts, [B * n_sqk, B * n_vs, B * n_vs, B * H])
    a.dsqk_part, a.dvs0_part, a.dvsL_part = dsqk_p.data_ptr(), dvs0_p.data_ptr(), dvsL_p.data_ptr()
    a.dWr, a.dbr, a.dWc, a.dbc = map(torch.Tensor.data_ptr, head_grads)
    a.dlogit_part = dlg_p.data_ptr()
    LAST_PATH["edgewise_bwd"] = path
    ws = _bytes(lib.mopk_edgewise_workspace_bytes(C.byref(a)), dev)
    if _KEEP_WS:
        LAST_PATH["_bwd_ws"] = ws  # diagnostics only (stamp builds read it back): pins the buffer until the next call
    a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
    _launch("mopk_edgewise_lowrank_bwd", a, "edgewise_bwd")
    return a, dqkv, d_extras, parts


class _EdgewiseLowrankFn(torch.autograd.Function):
    """y = EdgewiseMSA core(qkv, ...) ; reference attention_variants.py:500-562."""

    @staticmethod
    def forward(ctx, qkv, sqk, vs0, vsL, Wr, br, Wc, bc, logit, beta_not, V, prec, path, want_bwd, drop=(0.0, 0),
                lens_w=None, lens_dil=()):
        """lens_w (L,V,3,3) + lens_dil: the S lens bank.  Its planes reach the head as E = L V extra feature channels given by their
        row / column means (Wr / Wc then have 2V + 2 + E input channels): fused path only (MopkEdgewiseExt.n_extra)."""
        _require_gpu(qkv, "EdgewiseMSA")
        B, N, Vq, _, H, dk = qkv.shape
        f = dict(zip(("sqk", "vs0", "vsL", "Wr", "br", "Wc", "bc", "logit"),
                     _f32_pack([sqk, vs0, vsL, Wr, br, Wc, bc, logit.reshape(1)])))
        ctx.small_dtype = sqk.dtype if len({t.dtype for t in (sqk, vs0, vsL, Wr, br, Wc, bc, logit)}) == 1 else None
        y, core_saved = _ew_lowrank_fwd(ctx, qkv.contiguous(), f, beta_not, V, prec, path, want_bwd, drop, lens_w, lens_dil)
        ctx.save_for_backward(*core_saved)
        return y.view(B, N, H * dk)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        lib = L.lib()
        saved_all = ctx.saved_tensors          # read once: a non-reentrant checkpoint unpacks (recomputes) on every access
        qkv, _, sqk, *_rest = saved_all
        extras = saved_all[10:]
        V, r = ctx.meta[1], ctx.meta[4]
        B, N, Vq, _, H, dk = qkv.shape
        n_extra = extras[0].shape[2] if extras else 0
        C_ = 2 * V + 2 + n_extra
        # ONE buffer for the final values of the small gradients (reduced by the library in a single launch, cast to the
        # parameters' dtype in a single kernel, handed to autograd as views)
        n_sqk, n_vs, n_w, n_b = V * H * dk, H * dk, 4 * r * C_, 4 * r
        small = torch.empty(n_sqk + 2 * n_vs + 2 * n_w + 2 * n_b + 1, dtype=torch.float32, device=qkv.device)
        dsqk, dvs0, dvsL, dWr, dbr, dWc, dbc, dlg = torch.split(small, [n_sqk, n_vs, n_vs, n_w, n_b, n_w, n_b, 1])
        a, dqkv, d_extras, parts = _ew_lowrank_bwd(ctx, dy, saved_all, (dWr, dbr, dWc, dbc))
        L.check(lib.mopk_edgewise_reduce_parts(C.byref(a), dsqk.data_ptr(), dvs0.data_ptr(), dvsL.data_ptr(), dlg.data_ptr(),
                                               _stream()), "mopk_edgewise_reduce_parts")
        dlens = None
        if n_extra:     # the lens means are functions of q, k, sqk and the lens weights: their gradients join the kernels' own
            dsqk_x, dlens = lens_means_bwd_hip(d_extras[0], d_extras[1], qkv, dqkv, sqk, extras[2], ctx.lens_dil)
            dsqk.add_(dsqk_x.reshape(-1))
            dlens = dlens.to(ctx.lens_dtype)
        if ctx.small_dtype is not None and ctx.small_dtype != torch.float32:
            small = small.to(ctx.small_dtype)
            dsqk, dvs0, dvsL, dWr, dbr, dWc, dbc, dlg = torch.split(small, [n_sqk, n_vs, n_vs, n_w, n_b, n_w, n_b, 1])
        return (dqkv, dsqk.view(V, H, dk), dvs0.view(H, dk), dvsL.view(H, dk), dWr.view(4 * r, C_), dbr, dWc.view(4 * r, C_), dbc,
                dlg.reshape(()), None, None, None, None, None, None, dlens, None)


def _ew_param_args(B, q_scale, k_scale, v_scale, Wr, br, Wc, bc, logit) -> L.EdgewiseParamArgs:
    """the MopkEdgewiseParamArgs fields mopk_edgewise_params_fwd and _bwd share: shapes and the parameters themselves"""
    V, H, _, dk = q_scale.shape
    p = L.EdgewiseParamArgs()
    p.B, p.V, p.H, p.dk, p.r, p.C, p.io_dtype = B, V, H, dk, Wr.shape[0] // 4, Wr.shape[1], _io_dtype(q_scale)
    p.q_scale, p.k_scale, p.v_scale, p.Wr, p.br, p.Wc, p.bc, p.chain_logit = map(
        torch.Tensor.data_ptr, (q_scale, k_scale, v_scale, Wr, br, Wc, bc, logit))
    return p


class _EdgewiseSharedFn(torch.autograd.Function):
    """_EdgewiseLowrankFn for a share_qkv layer, taking the layer's small parameters as they are stored: q_scale, k_scale, v_scale
    (V,H,1,dk), the head's Wr, br, Wc, bc and chain_logit, all of one dtype (float32 / bfloat16).  The float32 copies the core
    reads (sqk = q_scale k_scale / sqrt(dk), v_scale[0], v_scale[V-1], ...) come from ONE launch, mopk_edgewise_params_fwd, and the
    parameters' gradients from ONE launch after the core's backward, mopk_edgewise_params_bwd (batch reduction + chain rule +
    cast, each gradient a tensor of its own) -- both bit-identical to the tensor expressions of EdgewiseMSA.forward feeding
    _EdgewiseLowrankFn, which cost about twenty small launches per step."""

    @staticmethod
    def forward(ctx, qkv, q_scale, k_scale, v_scale, Wr, br, Wc, bc, logit, beta_not, V, prec, path, want_bwd, drop=(0.0, 0)):
        _require_gpu(qkv, "EdgewiseMSA")
        B, N, Vq, _, H, dk = qkv.shape
        params = tuple(t.contiguous() for t in (q_scale, k_scale, v_scale, Wr, br, Wc, bc, logit))
        sizes = [V * H * dk, H * dk, H * dk, Wr.numel(), br.numel(), Wc.numel(), bc.numel(), 1]
        pack = torch.empty(sum(sizes), dtype=torch.float32, device=qkv.device)
        p = _ew_param_args(B, *params)
        p.pack = pack.data_ptr()
        _launch("mopk_edgewise_params_fwd", p)
        shapes = ((V, H, dk), (H, dk), (H, dk), Wr.shape, br.shape, Wc.shape, bc.shape, (1,))
        f = {k: t.view(sh) for k, t, sh in zip(("sqk", "vs0", "vsL", "Wr", "br", "Wc", "bc", "logit"), torch.split(pack, sizes), shapes)}
        y, core_saved = _ew_lowrank_fwd(ctx, qkv.contiguous(), f, beta_not, V, prec, path, want_bwd, drop)
        ctx.save_for_backward(*core_saved, *params)
        return y.view(B, N, H * dk)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        saved_all = ctx.saved_tensors          # read once: a non-reentrant checkpoint unpacks (recomputes) on every access
        core_saved, params = saved_all[:10], saved_all[10:]
        qkv = core_saved[0]
        n_w, n_b = params[3].numel(), params[4].numel()
        head = torch.empty(2 * n_w + 2 * n_b, dtype=torch.float32, device=qkv.device)
        a, dqkv, _, parts = _ew_lowrank_bwd(ctx, dy, core_saved, torch.split(head, [n_w, n_b, n_w, n_b]))
        grads = tuple(torch.empty_like(t) for t in params)     # one tensor per parameter: autograd keeps them without a copy
        p = _ew_param_args(qkv.shape[0], *params)
        p.dsqk_part, p.dvs0_part, p.dvsL_part, p.dlogit_part = a.dsqk_part, a.dvs0_part, a.dvsL_part, a.dlogit_part
        p.dWr, p.dbr, p.dWc, p.dbc = a.dWr, a.dbr, a.dWc, a.dbc
        p.gq_scale, p.gk_scale, p.gv_scale, p.gWr, p.gbr, p.gWc, p.gbc, p.glogit = map(torch.Tensor.data_ptr, grads)
        _launch("mopk_edgewise_params_bwd", p)
        return (dqkv, *grads, None, None, None, None, None, None)


class EdgewiseVariant:
    """Static description of a non-default gate head / lens bank (MopkEdgewiseExt, generic path)."""

    def __init__(self, dense: bool = False, use_k3: bool = False, lens_dilations=()):
        self.dense, self.use_k3, self.lens_dilations = bool(dense), bool(use_k3), tuple(int(d) for d in lens_dilations)
        if len(self.lens_dilations) > L.MAX_LENS:
            raise ValueError(f"at most {L.MAX_LENS} lens dilations are supported")


def _extra_ext(n_extra: int, row, col) -> L.EdgewiseExt:
    """MopkEdgewiseExt of a low-rank call whose head takes n_extra lens-mean channels; row / col: their (B,H,E,N) means"""
    ext = L.EdgewiseExt()
    ext.n_extra, ext.row_extra, ext.col_extra = n_extra, row.data_ptr(), col.data_ptr()
    return ext


def _variant_ext(var: EdgewiseVariant, f: dict) -> L.EdgewiseExt:
    """MopkEdgewiseExt of an _EdgewiseGeneralFn call; f: its float32 tensors (head h0..h3, W3, b3, lens_w)"""
    ext = L.EdgewiseExt()
    ext.gate_mode, ext.use_k3, ext.n_lens = int(var.dense), int(var.use_k3), len(var.lens_dilations)
    for i, d in enumerate(var.lens_dilations):
        ext.lens_dil[i] = d
    if var.lens_dilations:
        ext.lens_w = f["lens_w"].data_ptr()
    if var.dense:
        ext.W1, ext.b1, ext.W2, ext.b2 = f["h0"].data_ptr(), f["h1"].data_ptr(), f["h2"].data_ptr(), f["h3"].data_ptr()
        if var.use_k3:
            ext.W3, ext.b3 = f["W3"].data_ptr(), f["b3"].data_ptr()
    return ext


class _EdgewiseGeneralFn(torch.autograd.Function):
    """EdgewiseMSA core with a dense gate head and/or an S lens bank (reference :250-272, :312-318, :425-442, :523-533).

    tensor inputs: qkv, sqk, vs0, vsL, logit, head (4 tensors: low-rank Wr,br,Wc,bc | dense W1,b1,W2,b2), W3, b3, lens_w
    (unused ones are passed as empty tensors)."""

    @staticmethod
    def forward(ctx, qkv, sqk, vs0, vsL, logit, h0, h1, h2, h3, W3, b3, lens_w, beta_not, V, prec, var, wants_grad=True, drop=(0.0, 0),
                mask=None):
        _require_gpu(qkv, "EdgewiseMSA")
        lib = L.lib()
        B, N, Vq, _, H, dk = qkv.shape
        qkv = qkv.contiguous()
        dev = qkv.device
        f = dict(sqk=_f32c(sqk), vs0=_f32c(vs0), vsL=_f32c(vsL), logit=_f32c(logit).reshape(1),
                 h0=_f32c(h0), h1=_f32c(h1), h2=_f32c(h2), h3=_f32c(h3), W3=_f32c(W3), b3=_f32c(b3), lens_w=_f32c(lens_w))
        y = torch.empty(B, N, H, dk, dtype=qkv.dtype, device=dev)
        m8, ms = _mask_u8(mask, B, H, N, dev)
        small, head = (f["sqk"], f["vs0"], f["vsL"], f["logit"]), (f["h0"], f["h1"], f["h2"], f["h3"])
        a = _ew_args(qkv, y, V, 1 if var.dense else f["h0"].shape[0] // 4, prec, L.PATH_GENERIC, beta_not, drop, small,
                     None if var.dense else head, (m8, ms))
        ext = _variant_ext(var, f)
        a.ext = C.pointer(ext)
        # dense head without the 3x3 convolution / lens bank: the fused kernels evaluate it inside their mix loops (the backward
        # keeps dW1[k][:] and db1[k] in one 16-slot row, i.e. covers V <= 6)
        if var.dense and not var.use_k3 and not var.lens_dilations and m8 is None and _PATH != L.PATH_GENERIC and (not wants_grad or V <= 6):
            a.path, a.save_for_backward = L.PATH_FUSED, 1
            if not lib.mopk_edgewise_fused_supported(C.byref(a)):
                a.path, a.save_for_backward = L.PATH_GENERIC, 0
        LAST_PATH["edgewise_fwd"] = int(a.path)
        saved = _bytes(lib.mopk_edgewise_saved_bytes(C.byref(a)), dev)
        ws = _bytes(256 if a.path == L.PATH_FUSED else lib.mopk_edgewise_workspace_bytes(C.byref(a)), dev)
        a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
        _launch("mopk_edgewise_fwd", a, "edgewise_fwd")
        ctx.save_for_backward(qkv, saved, *f.values())
        ctx.keys = list(f.keys())
        ctx.meta = (beta_not, V, prec, var, int(a.r))
        ctx.fwd_path, ctx.drop, ctx.mask = int(a.path), drop, (m8, ms)
        return y.view(B, N, H * dk)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        lib = L.lib()
        qkv, saved, *rest = ctx.saved_tensors
        f = dict(zip(ctx.keys, rest))
        beta_not, V, prec, var, r = ctx.meta
        path = ctx.fwd_path
        B, N, Vq, _, H, dk = qkv.shape
        dev = qkv.device
        dy = _grad_in(dy, qkv.dtype)
        small, head = (f["sqk"], f["vs0"], f["vsL"], f["logit"]), (f["h0"], f["h1"], f["h2"], f["h3"])
        a = _ew_args(qkv, dy, V, r, prec, path, beta_not, ctx.drop, small, None if var.dense else head, ctx.mask)
        a.save_for_backward = int(path == L.PATH_FUSED)
        a.dy = L.View4(dy.data_ptr(), N * H * dk, dk, H * dk)
        dqkv = (torch.empty_like(qkv) if Vq == 1 else torch.zeros_like(qkv))
        _ew_views(a, dqkv, "d")
        f32 = dict(dtype=torch.float32, device=dev)
        dsqk, dvs0, dvsL, dlg = torch.empty(B, V, H, dk, **f32), torch.empty(B, H, dk, **f32), torch.empty(B, H, dk, **f32), torch.empty(B, H, **f32)
        a.dsqk_part, a.dvs0_part, a.dvsL_part, a.dlogit_part = dsqk.data_ptr(), dvs0.data_ptr(), dvsL.data_ptr(), dlg.data_ptr()
        g = {k: torch.zeros_like(f[k]) for k in ("h0", "h1", "h2", "h3", "W3", "b3", "lens_w")}
        ext = _variant_ext(var, f)
        if var.dense:
            ext.dW1, ext.db1, ext.dW2, ext.db2 = g["h0"].data_ptr(), g["h1"].data_ptr(), g["h2"].data_ptr(), g["h3"].data_ptr()
            if var.use_k3:
                ext.dW3, ext.db3 = g["W3"].data_ptr(), g["b3"].data_ptr()
        else:
            a.dWr, a.dbr, a.dWc, a.dbc = g["h0"].data_ptr(), g["h1"].data_ptr(), g["h2"].data_ptr(), g["h3"].data_ptr()
        if var.lens_dilations:
            ext.dlens_w = g["lens_w"].data_ptr()
        a.ext = C.pointer(ext)
        LAST_PATH["edgewise_bwd"] = path
        ws = _bytes(lib.mopk_edgewise_workspace_bytes(C.byref(a)), dev)
        a.saved, a.workspace = saved.data_ptr(), ws.data_ptr()
        _launch("mopk_edgewise_bwd", a, "edgewise_bwd")
        return (dqkv, dsqk.sum(0), dvs0.sum(0), dvsL.sum(0), dlg.sum().reshape(()), g["h0"], g["h1"], g["h2"], g["h3"],
                g["W3"], g["b3"], g["lens_w"], None, None, None, None, None, None, None)


def _half_via_fp32(fn):
    """float16 callers (`module.half()`, fp16 autocast): the kernels take float32 / bfloat16 only, so half tensors go through the
    float32 arithmetic (a superset of fp16) and the result is cast back; autograd carries the casts."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        def is_h(a):
            return isinstance(a, torch.Tensor) and a.dtype == torch.float16
        flat = list(args) + list(kw.values())
        if not any(is_h(a) or (isinstance(a, (tuple, list)) and any(is_h(b) for b in a)) for a in flat):
            return fn(*args, **kw)
        def up(a):
            if is_h(a):
                return a.float()
            if isinstance(a, (tuple, list)):
                return type(a)(up(b) for b in a)
            return a
        out = fn(*[up(a) for a in args], **{k: up(v) for k, v in kw.items()})
        def down(o):
            return o.half() if isinstance(o, torch.Tensor) and o.dtype == torch.float32 and o.dim() == 3 else o
        return tuple(down(o) for o in out) if isinstance(out, tuple) else down(out)
    return wrapped


def _empty_batch(t: torch.Tensor, *shape) -> torch.Tensor:
    """B = 0: the reference's torch ops return an empty result; the C ABI rejects empty shapes.  An empty tensor that still hangs
    on `t` in the autograd graph (its backward hands `t` an empty gradient)."""
    return t.new_zeros(shape) + t.sum() * 0


@_half_via_fp32
def edgewise_general_core(qkv, sqk, vs0, vsL, chain_logit, head, beta_not: float, n_views: int, variant: EdgewiseVariant,
                          W3=None, b3=None, lens_w=None, precision: Optional[int] = None, dropout_p: float = 0.0,
                          seed: Optional[int] = None, attn_mask=None):
    """EdgewiseMSA core for the dense gate head and/or the S lens bank.  head = (Wr, br, Wc, bc) for the low-rank head
    with C = 2V+2+L*V input channels, or (W1 (16,C), b1, W2 (4,16), b2) for the dense head; W3/b3 with use_k3;
    lens_w (L,V,3,3).  qkv as in edgewise_lowrank_core."""
    if qkv.shape[0] == 0:
        return _empty_batch(qkv, 0, qkv.shape[1], qkv.shape[-2] * qkv.shape[-1])
    prec = _prec_for(qkv.dtype) if precision is None else precision
    e = qkv.new_zeros(0, dtype=torch.float32)
    drop = _drop(dropout_p, seed)
    # decided here: inside Function.forward autograd is already switched off
    wants_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                                 for t in (qkv, sqk, vs0, vsL, chain_logit, *head, W3, b3, lens_w))
    return _EdgewiseGeneralFn.apply(qkv, sqk, vs0, vsL, chain_logit, *head, e if W3 is None else W3, e if b3 is None else b3,
                                    e if lens_w is None else lens_w, beta_not, n_views, prec, variant, wants_grad, drop, attn_mask)


def lens_mean_features(qkv, sqk, lens_w, dilations):
    """Row / column means of the S lens bank's planes (reference attention_variants.py:523-533) WITHOUT the planes.

    The bank convolves each score plane S_v = (q * sqk_v) k^T with a depthwise dilated 3x3 kernel w (zero padding = dilation d); the
    low-rank head only ever sees row and column means of the result (:323-326), and those are linear functionals of q and k:
        row mean [i] = 1/N sum_a sum_b w[a][b] R_b[i + (a-1) d],   R_b[i'] = q_v[i'] . sum_{j' in J_b} k[j']
        col mean [j] = 1/N sum_a sum_b w[a][b] C_a[j + (b-1) d],   C_a[j'] = k[j'] . sum_{i' in J_a} q_v[i']
    with J_0 = [0, N-d), J_1 = [0, N), J_2 = [d, N) the source rows / columns a kernel tap can reach.  O(N dk) work per (b, h, v)
    in plain torch ops (autograd carries their backward into q, k, sqk and the lens weights).

    qkv (B,N,1,3,H,dk) shared q / k; sqk (V,H,dk); lens_w (L,V,3,3); -> row, col (B,H,L*V,N) float32, channels l-major as :531."""
    B, N, _, _, H, dk = qkv.shape
    V = sqk.shape[0]
    q = qkv[:, :, 0, 0].permute(0, 2, 1, 3).float()           # (B,H,N,dk)
    k = qkv[:, :, 0, 1].permute(0, 2, 1, 3).float()
    sq = sqk.float()
    L_ = len(dilations)
    dil = [int(d) for d in dilations]
    dmax = max(dil)
    qsum, ksum = q.sum(2), k.sum(2)
    # sums over J_0 = all minus the last d tokens, J_1 = all, J_2 = all minus the first d (slices clamp at N: d >= N leaves nothing)
    ks = torch.stack([torch.stack([ksum - k[:, :, max(N - d, 0):].sum(2), ksum, ksum - k[:, :, :d].sum(2)], 2) for d in dil], 2)    # (B,H,L,3,dk)
    qs = torch.stack([torch.stack([qsum - q[:, :, max(N - d, 0):].sum(2), qsum, qsum - q[:, :, :d].sum(2)], 2) for d in dil], 2)
    w = lens_w.float() / N                                                                  # (L,V,3,3) [a][b]
    # the taps are folded into the (tiny) left operands first: ONE batched GEMM per side then yields, per lens, view and shift, the
    # vector that the shift-and-add below turns into the mean
    ua = torch.einsum("lvst,vhd,nhltd->nhlvsd", w, sq, ks).reshape(B, H, L_ * V * 3, dk)        # row side: shift index a (= s)
    ub = torch.einsum("lvst,vhd,nhlsd->nhlvtd", w, sq, qs).reshape(B, H, L_ * V * 3, dk)        # col side: shift index b (= t)
    Tr = F.pad(torch.matmul(ua, q.transpose(2, 3)).view(B, H, L_, V, 3, N), (dmax, dmax))      # [.., a, dmax + i]
    Tc = F.pad(torch.matmul(ub, k.transpose(2, 3)).view(B, H, L_, V, 3, N), (dmax, dmax))
    def shift_add(T, l, d):                                                                  # sum_a T_a[i + (a-1) d]
        return T[:, :, l, :, 0, dmax - d:dmax - d + N] + T[:, :, l, :, 1, dmax:dmax + N] + T[:, :, l, :, 2, dmax + d:dmax + d + N]
    return (torch.cat([shift_add(Tr, l, d) for l, d in enumerate(dil)], 2),
            torch.cat([shift_add(Tc, l, d) for l, d in enumerate(dil)], 2))


def _lens_set_sums(x, dil):
    """x (B,H,N,dk) -> (B,H,L,3,dk): sums of x over the tokens J_0 = [0, N-d), J_1 = all, J_2 = [d, N) per dilation (all minus the d edge rows)"""
    N = x.shape[2]
    tot = x.sum(2)
    return torch.stack([torch.stack([tot - x[:, :, N - d:].sum(2), tot, tot - x[:, :, :d].sum(2)], 2) for d in dil], 2)


def _lens_set_sums_adjoint(dx, g, dil):
    """dx (B,H,N,dk) += adjoint of _lens_set_sums applied to g (B,H,L,3,dk), in place"""
    N = dx.shape[2]
    dx += g.sum((2, 3))[:, :, None, :]
    for l, d in enumerate(dil):
        dx[:, :, N - d:] -= g[:, :, l, 0][:, :, None, :]
        dx[:, :, :d] -= g[:, :, l, 2][:, :, None, :]
    return dx


def _lens_shift_add(T, dil, dmax, N):
    """T (B,H,L,V,3,N + 2 dmax), zero padded by dmax: -> (B,H,L*V,N)  sum_a T[l,v,a][i + (a-1) d_l]"""
    return torch.cat([T[:, :, l, :, 0, dmax - d:dmax - d + N] + T[:, :, l, :, 1, dmax:dmax + N] + T[:, :, l, :, 2, dmax + d:dmax + d + N]
                      for l, d in enumerate(dil)], 2)


def _lens_unshift(dM, dil, dmax, N, V):
    """adjoint of _lens_shift_add: dM (B,H,L*V,N) -> (B,H,L*V*3,N)  dT[l,v,a][i'] = dM[l,v][i' - (a-1) d_l] (0 outside)"""
    B, H = dM.shape[:2]
    P = F.pad(dM.view(B, H, len(dil), V, N), (dmax, dmax))
    return torch.stack([torch.stack([P[:, :, l, :, dmax + d:dmax + d + N], P[:, :, l, :, dmax:dmax + N], P[:, :, l, :, dmax - d:dmax - d + N]], 3)
                        for l, d in enumerate(dil)], 2).reshape(B, H, -1, N)


def _lens_args(qkv, sqk, lens_w, dilations, V: int = 0) -> L.LensMeansArgs:
    """the call's MopkLensMeansArgs; sqk = lens_w = None (support query): the shape of V views only, no dtype or pointers"""
    B, N, _, _, H, dk = qkv.shape
    a = L.LensMeansArgs()
    a.B, a.H, a.N, a.dk, a.V, a.L = B, H, N, dk, V if sqk is None else sqk.shape[0], len(dilations)
    for i, d in enumerate(dilations):
        a.dil[i] = int(d)
    if sqk is None:
        return a
    a.io_dtype = _io_dtype(qkv)
    s_n = 3 * H * dk
    a.q = L.View4(qkv.data_ptr(), N * s_n, dk, s_n)
    a.k = L.View4(qkv.data_ptr() + H * dk * qkv.element_size(), N * s_n, dk, s_n)
    a.sqk, a.lens_w = sqk.data_ptr(), lens_w.data_ptr()
    return a


def lens_means_hip(qkv, sqk, lens_w, dilations):
    """row / col means of the S lens bank's planes (B,H,L*V,N) fp32 from libmopk's closed-form kernel (mopk_lens_means_fwd);
    qkv (B,N,1,3,H,dk) contiguous on the GPU, sqk (V,H,dk) / lens_w (L,V,3,3) float32 contiguous."""
    _require_gpu(qkv, "lens means")
    B, N, _, _, H, dk = qkv.shape
    E = lens_w.shape[0] * lens_w.shape[1]
    a = _lens_args(qkv, sqk, lens_w, dilations)
    row, col = torch.empty(B, H, E, N, dtype=torch.float32, device=qkv.device), torch.empty(B, H, E, N, dtype=torch.float32, device=qkv.device)
    a.row, a.col = row.data_ptr(), col.data_ptr()
    _launch("mopk_lens_means_fwd", a)
    return row, col


def lens_means_bwd_hip(d_row, d_col, qkv, dqkv, sqk, lens_w, dilations):
    """backward of `lens_means_hip`: ADDS the q / k gradients into dqkv (same layout as qkv) and returns dsqk (V,H,dk), dlens_w (L,V,3,3)"""
    B, N, _, _, H, dk = qkv.shape
    V, Ln = sqk.shape[0], lens_w.shape[0]
    a = _lens_args(qkv, sqk, lens_w, dilations)
    s_n = 3 * H * dk
    a.dq = L.View4(dqkv.data_ptr(), N * s_n, dk, s_n)
    a.dk_ = L.View4(dqkv.data_ptr() + H * dk * dqkv.element_size(), N * s_n, dk, s_n)
    dsqk_p = torch.empty(B, V, H, dk, dtype=torch.float32, device=qkv.device)
    dlens_p = torch.empty(B * H, Ln, V, 3, 3, dtype=torch.float32, device=qkv.device)
    a.d_row, a.d_col, a.dsqk_part, a.dlens_part = d_row.data_ptr(), d_col.data_ptr(), dsqk_p.data_ptr(), dlens_p.data_ptr()
    _launch("mopk_lens_means_bwd", a)
    return dsqk_p.sum(0), dlens_p.sum(0)


def _lens_means_fwd(qkv, sqk, lens_w, dilations):
    """`lens_mean_features` without an autograd graph, in torch ops: -> row, col (B,H,L*V,N), state for `_lens_means_bwd`.  The statement
    the HIP kernels (`lens_means_hip`, mop_amd/csrc/lens_means.hip) are tested against; the product path calls the kernels."""
    B, N, _, _, H, dk = qkv.shape
    V, L_ = sqk.shape[0], len(dilations)
    dil = [min(int(d), N) for d in dilations]
    dmax = max(dil)
    q = qkv[:, :, 0, 0].permute(0, 2, 1, 3).float()
    k = qkv[:, :, 0, 1].permute(0, 2, 1, 3).float()
    ks, qs = _lens_set_sums(k, dil), _lens_set_sums(q, dil)
    w = lens_w.float() / N
    ua = torch.einsum("lvst,vhd,nhltd->nhlvsd", w, sqk, ks).reshape(B, H, L_ * V * 3, dk)
    ub = torch.einsum("lvst,vhd,nhlsd->nhlvtd", w, sqk, qs).reshape(B, H, L_ * V * 3, dk)
    Tr = F.pad(torch.matmul(ua, q.transpose(2, 3)).view(B, H, L_, V, 3, N), (dmax, dmax))
    Tc = F.pad(torch.matmul(ub, k.transpose(2, 3)).view(B, H, L_, V, 3, N), (dmax, dmax))
    return _lens_shift_add(Tr, dil, dmax, N), _lens_shift_add(Tc, dil, dmax, N), (ks, qs, ua, ub)


def _lens_means_bwd(d_row, d_col, qkv, sqk, lens_w, dilations, state):
    """-> dq, dk (B,H,N,dk) float32, dsqk (V,H,dk), dlens_w (L,V,3,3)"""
    B, N, _, _, H, dk = qkv.shape
    V, L_ = sqk.shape[0], len(dilations)
    dil = [min(int(d), N) for d in dilations]
    dmax = max(dil)
    ks, qs, ua, ub = state
    q = qkv[:, :, 0, 0].permute(0, 2, 1, 3).float()
    k = qkv[:, :, 0, 1].permute(0, 2, 1, 3).float()
    w = lens_w.float() / N
    dTr, dTc = _lens_unshift(d_row, dil, dmax, N, V), _lens_unshift(d_col, dil, dmax, N, V)       # (B,H,L*V*3,N)
    dua = torch.matmul(dTr, q).view(B, H, L_, V, 3, dk)
    dub = torch.matmul(dTc, k).view(B, H, L_, V, 3, dk)
    dq = torch.matmul(dTr.transpose(2, 3), ua)
    dk_ = torch.matmul(dTc.transpose(2, 3), ub)
    # through ua = w . sqk . ks and ub = w . sqk . qs
    gs_a, gs_b = dua * sqk.permute(1, 0, 2)[None, :, None, :, None, :], dub * sqk.permute(1, 0, 2)[None, :, None, :, None, :]   # (B,H,L,V,3,dk)
    # contractions over (batch, head, d) with a 3 x 3 result per (l, v): a broadcast product + one reduction (as a GEMM they are
    # K = B H dk deep with a 30 x 3 output -- one workgroup's worth of parallelism)
    dw = ((gs_a[:, :, :, :, :, None, :] * ks[:, :, :, None, None, :, :]).sum((0, 1, 6)) +
          (gs_b[:, :, :, :, None, :, :] * qs[:, :, :, None, :, None, :]).sum((0, 1, 6))) / N
    wks = torch.einsum("lvst,nhltd->nhlvsd", w, ks)
    wqs = torch.einsum("lvst,nhlsd->nhlvtd", w, qs)
    dsqk = (dua * wks + dub * wqs).sum((0, 2, 4)).permute(1, 0, 2)                               # (V,H,dk)
    dks = torch.einsum("nhlvsd,lvst->nhltd", gs_a, w).reshape(B, H, L_ * 3, dk)
    dqs = torch.einsum("nhlvtd,lvst->nhlsd", gs_b, w).reshape(B, H, L_ * 3, dk)
    return _lens_set_sums_adjoint(dq, dqs.view(B, H, L_, 3, dk), dil), _lens_set_sums_adjoint(dk_, dks.view(B, H, L_, 3, dk), dil), dsqk, dw


def lowrank_lens_fused_supported(qkv, n_views: int, rank: int, dilations, precision: Optional[int] = None) -> bool:
    """True when the fused kernels take this low-rank call with an S lens bank of these dilations (as extra mean-feature channels) and
    libmopk's closed-form kernels (mopk_lens_means_*) take the bank"""
    n_lens = len(dilations)
    if not qkv.is_cuda or qkv.shape[2] != 1 or qkv.shape[0] == 0 or _PATH == L.PATH_GENERIC or qkv.dtype == torch.float16:
        return False
    if not 1 <= n_lens <= L.MAX_LENS:
        return False
    if not L.lib().mopk_lens_means_supported(C.byref(_lens_args(qkv, None, None, dilations, n_views)), 1):
        return False
    # qkv: non-null stand-in for y and the extra channels, nothing is read
    a = _ew_args(qkv, qkv, n_views, rank, _prec_for(qkv.dtype) if precision is None else precision, L.PATH_FUSED)
    ext = _extra_ext(n_lens * n_views, qkv, qkv)
    a.ext = C.pointer(ext)
    return bool(L.lib().mopk_edgewise_fused_supported(C.byref(a)))


@_half_via_fp32
def edgewise_lowrank_core(qkv, sqk, vs0, vsL, Wr, br, Wc, bc, chain_logit, beta_not: float,
                          n_views: int, precision: Optional[int] = None, path: Optional[int] = None,
                          dropout_p: float = 0.0, seed: Optional[int] = None, lens_w=None, lens_dilations=()):
    """qkv: (B,N,Vq,3,H,dk) with Vq in {1 (share_qkv), n_views}; returns (B,N,H*dk).  dropout_p > 0: attn_drop on the mixed
    attention weights (:552) inside the fused kernels (see `sdpa_core`).  lens_w (L,V,3,3) + lens_dilations: the S lens bank, fed to
    the fused kernels as extra mean-feature channels (`lens_mean_features` states the closed form; the Function evaluates it and its
    backward with libmopk's kernels, `lens_means_hip` / `lens_means_bwd_hip`; callers check `lowrank_lens_fused_supported` first)."""
    if qkv.shape[0] == 0:
        return _empty_batch(qkv, 0, qkv.shape[1], qkv.shape[-2] * qkv.shape[-1])
    drop = _drop(dropout_p, seed)
    prec = _prec_for(qkv.dtype) if precision is None else precision
    want_bwd = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (qkv, sqk, vs0, vsL, Wr, br, Wc, bc, chain_logit, lens_w))
    return _EdgewiseLowrankFn.apply(qkv, sqk, vs0, vsL, Wr, br, Wc, bc, chain_logit, beta_not,
                                    n_views, prec, _PATH if path is None else path, want_bwd, drop, lens_w, tuple(lens_dilations))


def edgewise_shared_params_supported(qkv, params) -> bool:
    """True when `edgewise_lowrank_core_shared` takes this call: GPU tensors, float32 / bfloat16 qkv of the share_qkv layout
    (B,N,1,3,H,dk) with B > 0, and the small parameters all of one dtype that is float32 or bfloat16"""
    dtypes = {t.dtype for t in params}
    return (qkv.is_cuda and qkv.dim() == 6 and qkv.shape[2] == 1 and qkv.shape[0] > 0 and qkv.dtype in (torch.float32, torch.bfloat16)
            and len(dtypes) == 1 and next(iter(dtypes)) in (torch.float32, torch.bfloat16) and all(t.is_cuda for t in params))


def edgewise_lowrank_core_shared(qkv, q_scale, k_scale, v_scale, Wr, br, Wc, bc, chain_logit, beta_not: float,
                                 n_views: int, precision: Optional[int] = None, path: Optional[int] = None,
                                 dropout_p: float = 0.0, seed: Optional[int] = None):
    """`edgewise_lowrank_core` of a share_qkv layer, fed with the layer's parameters as they are stored instead of the tensors
    derived from them: qkv (B,N,1,3,H,dk); q_scale, k_scale, v_scale (V,H,1,dk) with V = n_views.  Computes what
    `edgewise_lowrank_core(qkv, (q_scale * k_scale).squeeze(2) / sqrt(dk), v_scale[0, :, 0], v_scale[V - 1, :, 0], ...)` computes,
    bit for bit in the output and in every gradient, with one small kernel before the core and one after its backward in place of
    the tensor expressions (see _EdgewiseSharedFn).  Callers check `edgewise_shared_params_supported` first."""
    params = (q_scale, k_scale, v_scale, Wr, br, Wc, bc, chain_logit)
    if not edgewise_shared_params_supported(qkv, params):
        raise NotImplementedError("edgewise_lowrank_core_shared: needs a GPU share_qkv call whose small parameters have one dtype "
                                  "(float32 / bfloat16); use edgewise_lowrank_core")
    if tuple(q_scale.shape) != (n_views, qkv.shape[4], 1, qkv.shape[5]) or k_scale.shape != q_scale.shape or v_scale.shape != q_scale.shape:
        raise ValueError(f"q_scale / k_scale / v_scale must be (n_views, H, 1, dk), got {tuple(q_scale.shape)}")
    drop = _drop(dropout_p, seed)
    prec = _prec_for(qkv.dtype) if precision is None else precision
    want_bwd = torch.is_grad_enabled() and any(t.requires_grad for t in (qkv, *params))
    return _EdgewiseSharedFn.apply(qkv, *params, beta_not, n_views, prec, _PATH if path is None else path, want_bwd, drop)


# --------------------------------------------------------------------------------------
# sibling cores: plain SDPA, dual-path (MultiHopMSA), Quartet
# --------------------------------------------------------------------------------------
def _v4(t: torch.Tensor) -> L.View4:
    """t: (B,N,H,dk) view with unit inner stride -> MopkView4 (strides b,h,n in elements)."""
    assert t.dim() == 4 and t.stride(3) == 1, "inner (head_dim) stride must be 1"
    return L.View4(t.data_ptr(), t.stride(0), t.stride(2), t.stride(1))


def _heads_view(t: torch.Tensor) -> torch.Tensor:
    return t if t.stride(-1) == 1 else t.contiguous()


def _bcast_keys(t: torch.Tensor, B, H, N, Nk) -> torch.Tensor:
    """t, broadcastable to (B,H,N,Nk), as the (B,H,N,Nk) view the kernels index: element (b,h,i,j) at b*sb + h*sh + i*si + j, so the
    key axis has stride 1.  B, H and N stay broadcast by stride 0; a key axis of extent 1 is the one axis written out (Nk copies of
    what t holds, no more), since a stride-0 key axis would make the kernels read t[i + j]."""
    while t.dim() < 4:
        t = t.unsqueeze(0)
    t = t.contiguous()
    if t.shape[3] == 1 and Nk > 1:
        t = t.expand(-1, -1, -1, Nk).contiguous()
    return t.expand(B, H, N, Nk)


def _mask_u8(attn_mask, B, H, N, dev, Nk=None):
    """reference convention: broadcastable to (B,H,N,Nk) (Nk = N unless given), 0 = blocked (attention_variants.py:43-44)."""
    if attn_mask is None:
        return None, (0, 0, 0)
    Nk = N if Nk is None else Nk
    m = _bcast_keys((attn_mask.to(dev) != 0).to(torch.uint8), B, H, N, Nk)
    return m, (m.stride(0), m.stride(1), m.stride(2))


def _refuse_bias_grad(t: Optional[torch.Tensor], what: str) -> None:
    """the cores return no gradient for an additive bias: one that would take part in autograd is an error, not a silent zero"""
    if t is not None and torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(f"{what} requires grad, but the attention cores compute no gradient for it; pass {what}.detach() "
                                  f"or call under torch.no_grad()")


def _bias_f32(bias, B, H, N, dev, Nk=None):
    if bias is None:
        return None, (0, 0, 0)
    Nk = N if Nk is None else Nk
    b = _bcast_keys(bias.to(dev, torch.float32), B, H, N, Nk)
    return b, (b.stride(0), b.stride(1), b.stride(2))


_CORE_OPS = {   # core -> (export stem, support query that resolves PATH_AUTO, LAST_PATH / timing stem, directions LAST_PATH records)
    "sdpa": ("mopk_sdpa", "mopk_sdpa_fused_supported", "sdpa", ("fwd", "bwd")),
    "sdpa_lens": ("mopk_sdpa_lens", "mopk_sdpa_lens_supported", "sdpa", ("fwd", "bwd")),
    "dualpath": ("mopk_dualpath", "mopk_dualpath_fused_supported", "dualpath", ("fwd", "bwd")),
    "quartet": ("mopk_quartet", "mopk_quartet_fused_supported", "quartet", ("fwd",)),
    "quartet_lens": ("mopk_quartet_lens", "mopk_quartet_lens_fused_supported", "quartet", ("fwd",)),
    "crossview": ("mopk_crossview", None, "crossview", ()),       # one path; crossview_core* record it
}


def _core_launch(core: str, a, dev, saved: Optional[torch.Tensor] = None):
    """the tail these cores share, on the args struct `a` (or the one it wraps as .base); forward when `saved` is None, else the
    backward on the forward's `saved`.  Forward: PATH_AUTO is resolved first, so that forward, backward and the size queries agree,
    and `saved` is sized and allocated.  Both: LAST_PATH in the directions `recorded` names, the workspace, the two pointers into
    the struct, the launch (timed under stem_fwd / stem_bwd).  Returns (saved, the resolved path)."""
    stem, query, key, recorded = _CORE_OPS[core]
    lib, base, d = L.lib(), getattr(a, "base", a), ("fwd" if saved is None else "bwd")
    if saved is None and base.path == L.PATH_AUTO:
        base.path = L.PATH_FUSED if getattr(lib, query)(C.byref(a)) else L.PATH_GENERIC
    path = base.path
    if d in recorded:
        LAST_PATH[f"{key}_{d}"] = path
    if saved is None:
        saved = _bytes(getattr(lib, stem + "_saved_bytes")(C.byref(a)), dev)
    ws = _bytes(getattr(lib, stem + "_workspace_bytes")(C.byref(a)), dev)
    base.saved, base.workspace = saved.data_ptr(), ws.data_ptr()
    _launch(f"{stem}_{d}", a, f"{key}_{d}")
    return saved, path


def _sdpa_args(q, k, v, y, mask, bias, causal, prec, path, drop, lens=None):
    """the MopkSdpaArgs fields forward and backward share; mask / bias: (tensor or None, strides) from _mask_u8 / _bias_f32.
    lens: (q_lens or None, kv_lens or None), int32 (B,) device tensors -> the MopkSdpaLensArgs that wraps them"""
    B, N, H, dk = q.shape
    a = L.SdpaArgs()
    a.B, a.H, a.N, a.dk, a.Nk = B, H, N, dk, k.shape[1]
    a.io_dtype, a.precision, a.path, a.causal = _io_dtype(q), prec, path, int(bool(causal))
    a.q, a.k, a.v, a.y = _v4(q), _v4(k), _v4(v), _v4(y)
    a.mask, (a.mask_sb, a.mask_sh, a.mask_si) = _ptr(mask[0]), mask[1]
    a.bias, (a.bias_sb, a.bias_sh, a.bias_si) = _ptr(bias[0]), bias[1]
    a.dropout_p, a.dropout_seed = float(drop[0]), int(drop[1])
    return a if lens is None else L.SdpaLensArgs(base=a, q_lens=_ptr(lens[0]), kv_lens=_ptr(lens[1]))


def _sdpa_fwd(ctx, q, k, v, mask, bias, lens, causal, prec, path, drop):
    """the forward of _SdpaFn (lens None) and _SdpaLensFn (mask = bias = None)"""
    _require_gpu(q, "SDPA")
    # packed form: q is the (B,N,3,H,dk) output of one qkv projection and k = v = None.  The kernels read the three strided views and
    # the backward writes ONE packed gradient -- autograd then has no per-view zero-fill + copy + add to assemble it from three
    ctx.packed = k is None
    if ctx.packed:
        q, k, v = q.contiguous().unbind(2)
    q, k, v = _heads_view(q), _heads_view(k), _heads_view(v)
    B, N, H, dk = q.shape
    Nk = k.shape[1]                # key / value length (cross-attention); N for self-attention
    dev = q.device
    mask, bias = _mask_u8(mask, B, H, N, dev, Nk), _bias_f32(bias, B, H, N, dev, Nk)
    y = torch.empty(B, N, H, dk, dtype=q.dtype, device=dev)
    a = _sdpa_args(q, k, v, y, mask, bias, causal, prec, path, drop, lens)
    saved, path = _core_launch("sdpa" if lens is None else "sdpa_lens", a, dev)
    ctx.save_for_backward(q, k, v, y, saved)
    ctx.meta = (mask, bias, causal, prec, path, drop, lens)
    return y.view(B, N, H * dk)


def _sdpa_bwd(ctx, saved_tensors, dy):
    """the backward of both on dy as _grad_in returns it, (B,N,H,dk): one packed gradient or three, Nk rows for keys and values"""
    q, k, v, y, saved = saved_tensors
    B, N, H, dk = q.shape
    Nk = k.shape[1]
    dev = q.device
    a = _sdpa_args(q, k, v, y, *ctx.meta)
    base = getattr(a, "base", a)
    base.dy = _v4(dy)
    if ctx.packed:
        dqkv = torch.empty(B, N, 3, H, dk, dtype=q.dtype, device=dev)
        dq, dk_, dv = dqkv.unbind(2)
    else:
        dq = torch.empty(B, N, H, dk, dtype=q.dtype, device=dev)
        dk_, dv = (torch.empty(B, Nk, H, dk, dtype=q.dtype, device=dev) for _ in range(2))
    base.dq, base.dk_, base.dv = _v4(dq), _v4(dk_), _v4(dv)
    _core_launch("sdpa" if base is a else "sdpa_lens", a, dev, saved)
    if ctx.packed:
        return dqkv, None, None, None, None, None, None, None, None
    return dq, dk_, dv, None, None, None, None, None, None


class _SdpaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, bias, causal, prec, path, drop=(0.0, 0)):
        return _sdpa_fwd(ctx, q, k, v, mask, bias, None, causal, prec, path, drop)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        ts = ctx.saved_tensors
        return _sdpa_bwd(ctx, ts, _grad_in(dy, ts[0].dtype, ts[0].shape))


class _SdpaLensFn(torch.autograd.Function):
    """_SdpaFn over right-padded rows (mopk_sdpa_lens_*): no mask / bias tensor, per-row lengths read by the kernels"""

    @staticmethod
    def forward(ctx, q, k, v, q_lens, kv_lens, causal, prec, path, drop=(0.0, 0)):
        return _sdpa_fwd(ctx, q, k, v, None, None, (q_lens, kv_lens), causal, prec, path, drop)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        ts = ctx.saved_tensors
        return _sdpa_bwd(ctx, ts, _grad_in(dy, ts[0].dtype, ts[0].shape))


def _check_lens(t, B: int, dev, what: str, op: str = "sdpa_core", beside: str = "q") -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"{op}: {what} must be an int32 (B,) = ({B},) tensor, got "
                         f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{op}: {what} is on {t.device}, {beside} on {dev}")


def sdpa_lens_mask(q_lens, kv_lens, B: int, N: int, Nk: int, device) -> torch.Tensor:
    """the lengths as a (B, 1, N or 1, Nk or 1) bool mask, True = open: query i < q_lens[b] sees key j < kv_lens[b] (torch ops on the
    device, no host sync)"""
    m = torch.ones(B, 1, 1, 1, dtype=torch.bool, device=device)
    if q_lens is not None:
        m = m & (torch.arange(N, device=device).view(1, 1, N, 1) < q_lens.view(B, 1, 1, 1))
    if kv_lens is not None:
        m = m & (torch.arange(Nk, device=device).view(1, 1, 1, Nk) < kv_lens.view(B, 1, 1, 1))
    return m


def dropout_seed() -> int:
    """a fresh 63-bit seed for the in-kernel dropout mask, drawn from torch's CPU generator (so `torch.manual_seed` makes runs
    reproducible, like it does for `nn.Dropout`)"""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _drop(dropout_p: float, seed: Optional[int]) -> tuple:
    """(p, seed) of a core's in-kernel dropout: a fresh seed when none is given, (0.0, 0) when off"""
    return (float(dropout_p), (dropout_seed() if seed is None else int(seed))) if dropout_p > 0 else (0.0, 0)


def dropout_keep_mask(seed: int, p: float, B: int, H: int, N: int, Nk: Optional[int] = None) -> torch.Tensor:
    """the kernels' keep mask as a (B,H,N,Nk) bool tensor, Nk = N unless given (host restatement of `mopk_dropout_keep`, vectorised;
    tests / debugging)"""
    Nk = N if Nk is None else Nk
    import numpy as np
    def h32(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
        x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
        x ^= x >> np.uint64(16)
        return x
    M = np.uint64(0xffffffff)
    lo, hi = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    t = float(p) * 4294967296.0
    thresh = np.uint64(0xffffffff if t >= 4294967295.0 else (1 if t < 1.0 else int(t)))
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i = np.arange(N, dtype=np.uint64)[None, :, None]
    j = np.arange(Nk, dtype=np.uint64)[None, None, :]
    row = h32((i * np.uint64(0x9E3779B1) + bh * np.uint64(0x85EBCA77) + hi) & M) ^ lo
    keep = h32((row ^ ((j * np.uint64(0xC2B2AE3D)) & M)) & M) >= thresh
    return torch.from_numpy(keep.reshape(B, H, N, Nk)) if p > 0 else torch.ones(B, H, N, Nk, dtype=torch.bool)


@_half_via_fp32
def sdpa_core(q, k=None, v=None, attn_mask=None, bias=None, causal=False, dropout_p: float = 0.0, seed: Optional[int] = None,
              q_lens=None, kv_lens=None):
    """q: (B,N,H,dk), k, v: (B,Nk,H,dk) views -- Nk != N is rectangular (cross-)attention: N queries attend to Nk keys -- or packed:
    q = the (B,N,3,H,dk) output of one qkv projection, k = v = None (square; one packed gradient comes back).  Returns (B,N,H*dk).
    attn_mask: 0 = blocked; bias: additive; both broadcastable to (B,H,N,Nk) along any axis, the key axis included (a (N,1) bias, a
    (B,1,N,1) per-query mask; 0-d to 4-d, contiguous or not).  causal needs Nk == N (ValueError otherwise).
    A row with no open key (every key blocked, or a bias of -inf at every key) is 0, as in torch's SDPA.  bias gets no gradient:
    one that requires grad under grad mode raises NotImplementedError.
    dropout_p > 0: the probabilities are multiplied by keep / (1 - p) (mask = `dropout_keep_mask(seed, B, H, N, Nk)`, seed drawn
    when None).
    q_lens / kv_lens: int32 (B,) tensors on q's device for a batch of right-padded rows (values are clamped into [0, N] / [0, Nk]).
    Query i < q_lens[b] attends to keys j < kv_lens[b]; padding query rows give y = 0 and get no gradient, padding keys get
    dk = dv = 0, and padding queries add nothing to dk, dv.  Without attn_mask / bias the kernels read the lengths themselves
    (mopk_sdpa_lens_*: loop bounds, not a mask): rows beyond a length are never loaded, so the result does not depend on what q, k,
    v or the incoming gradient hold there (NaN included), and full lengths are bitwise the call without lengths.  With an attn_mask
    or bias tensor the lengths are folded into the mask (torch ops, no sync) and the call takes the mask route, which multiplies
    padding rows by zero weights: they must then be finite.  No host synchronisation either way."""
    _refuse_bias_grad(bias, "sdpa_core: bias")
    if k is not None:
        if k.dim() != 4 or v is None or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2:] != q.shape[2:]:
            raise ValueError(f"sdpa_core: k, v must be (B, Nk, H, dk) with q's B, H, dk; got q {tuple(q.shape)}, k {tuple(k.shape)}, "
                             f"v {tuple(v.shape) if v is not None else None}")
        if k.shape[1] == 0 and q.shape[1] > 0:        # Nk = 0 means "N" in the C ABI: never pass it through
            raise ValueError("sdpa_core: k, v have no keys (Nk = 0)")
        if causal and k.shape[1] != q.shape[1]:
            raise ValueError(f"sdpa_core: causal attention needs as many keys as queries (N = {q.shape[1]}, Nk = {k.shape[1]})")
    if q_lens is not None or kv_lens is not None:
        for t, what in ((q_lens, "q_lens"), (kv_lens, "kv_lens")):
            if t is not None:
                _check_lens(t, q.shape[0], q.device, what)
    if q.shape[0] == 0:
        if k is None:
            return _empty_batch(q, 0, q.shape[1], q.shape[-2] * q.shape[-1])
        return _empty_batch(q, 0, q.shape[1], q.shape[2] * q.shape[3]) + (k.sum() + v.sum()) * 0
    drop = _drop(dropout_p, seed)
    if q_lens is None and kv_lens is None:
        return _SdpaFn.apply(q, k, v, attn_mask, bias, causal, _prec_for(q.dtype), _PATH, drop)
    if attn_mask is None and bias is None:
        return _SdpaLensFn.apply(q, k, v, q_lens, kv_lens, causal, _prec_for(q.dtype), _PATH, drop)
    B, N, Nk = q.shape[0], q.shape[1], (q.shape[1] if k is None else k.shape[1])
    m = sdpa_lens_mask(q_lens, kv_lens, B, N, Nk, q.device)
    if attn_mask is not None:
        m = m & (attn_mask.to(q.device) != 0)
    return _SdpaFn.apply(q, k, v, m, bias, causal, _prec_for(q.dtype), _PATH, drop)


_ANCHOR_MODES = {"fixed": 0, "argmax_row_sum": 1}          # any other string -> row 0 (reference :141-145)


def _cv_args(ts, mx, y, cfg, mask, causal, prec, drop) -> L.CrossViewArgs:
    """the MopkCrossViewArgs fields forward and backward share; ts: the five (B,N,H,dk) views q1 k1 v1 q2 k2, mx: float32 mix"""
    B, N, H, dk = ts[0].shape
    a = L.CrossViewArgs()
    a.B, a.H, a.N, a.dk = B, H, N, dk
    a.io_dtype, a.precision, a.path, a.causal = _io_dtype(ts[0]), prec, L.PATH_GENERIC, int(bool(causal))
    a.t1, a.t2, a.prior_weight, a.use_prior, a.anchor_mode, a.fixed_k_star = cfg
    a.q1, a.k1, a.v1, a.q2, a.k2 = (_v4(t) for t in ts)
    a.mix, a.y = mx.data_ptr(), _v4(y)
    a.mask, (a.mask_sb, a.mask_sh, a.mask_si) = _ptr(mask[0]), mask[1]
    a.dropout_p, a.dropout_seed = float(drop[0]), int(drop[1])
    return a


class _CrossViewFn(torch.autograd.Function):
    """CrossViewMixerMSA core, reference attention_variants.py:90-153."""

    @staticmethod
    def forward(ctx, q1, k1, v1, q2, k2, mix, cfg, mask, causal, prec, drop=(0.0, 0)):
        _require_gpu(q1, "CrossViewMixerMSA")
        ts = [_heads_view(t) for t in (q1, k1, v1, q2, k2)]
        B, N, H, dk = ts[0].shape
        dev = ts[0].device
        mx = _f32c(mix).reshape(4)
        mask = _mask_u8(mask, B, H, N, dev)
        y = torch.empty(B, N, H, dk, dtype=ts[0].dtype, device=dev)
        a = _cv_args(ts, mx, y, cfg, mask, causal, prec, drop)
        kst = torch.zeros(B, H, dtype=torch.int32, device=dev)
        a.k_star = kst.data_ptr()
        saved, _ = _core_launch("crossview", a, dev)
        LAST_PATH["crossview_k_star"] = kst
        ctx.save_for_backward(*ts, mx, saved)
        ctx.meta = (cfg, causal, prec, mask, drop)
        return y.view(B, N, H * dk)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        *ts, mx, saved = ctx.saved_tensors
        cfg, causal, prec, mask, drop = ctx.meta
        B, N, H, dk = ts[0].shape
        dev = ts[0].device
        dy = _grad_in(dy, ts[0].dtype, (B, N, H, dk))
        a = _cv_args(ts, mx, dy, cfg, mask, causal, prec, drop)          # a.y = dy: unused by bwd, must be non-null
        a.dy = _v4(dy)
        outs = [torch.empty(B, N, H, dk, dtype=ts[0].dtype, device=dev) for _ in range(5)]
        a.dq1, a.dk1, a.dv1, a.dq2, a.dk2 = (_v4(t) for t in outs)
        dmix = torch.empty(B, H, 4, dtype=torch.float32, device=dev)
        a.dmix_part = dmix.data_ptr()
        _core_launch("crossview", a, dev, saved)
        return (*outs, dmix.sum((0, 1)).view(2, 2), None, None, None, None, None)


def _cv_folds(t1, t2, prior_weight, prec, dk) -> bool:
    """the 2x2 mix folds into the dual-path kernels: no transpose cues or prior, fused path allowed, bf16 arithmetic, dk 32 / 64"""
    return (prior_weight <= 0.0 and t1 == 0.0 and t2 == 0.0 and _PATH != L.PATH_GENERIC and prec == L.PREC_BF16
            and dk in (32, 64))


def _cv_mixed_keys(m, k1, k2):
    """S = q1 (m11 k1 + m12 k2)^T + q2 (m21 k1 + m22 k2)^T: the mixed keys k1', k2' (contiguous) from m, the mix in k1's dtype"""
    return (m[0, 0] * k1 + m[0, 1] * k2).contiguous(), (m[1, 0] * k1 + m[1, 1] * k2).contiguous()


@_half_via_fp32
def crossview_core(q1, k1, v1, q2, k2, mix, t1=0.0, t2=0.0, prior_weight=0.0, anchor_mode="argmax_row_sum", fixed_k_star=0,
                   attn_mask=None, causal=False, dropout_p: float = 0.0, seed: Optional[int] = None):
    """q*,k*,v1: (B,N,H,dk) views; mix (2,2).  prior_weight = 0 disables the per-key prior.  Returns (B,N,H*dk)."""
    if q1.shape[0] == 0:
        return _empty_batch(q1, 0, q1.shape[1], q1.shape[2] * q1.shape[3])
    prec = _prec_for(q1.dtype)
    drop = _drop(dropout_p, seed)
    if _cv_folds(t1, t2, prior_weight, prec, q1.shape[-1]) and not any(t.data_ptr() % 16 for t in (q1, k1, v1, q2, k2)):
        # the 2x2 mix folds into two mixed key tensors (autograd carries d mix, d k1, d k2) and the core is the fused two-score
        # attention (dual-path kernels without the transport term), which reads 16-byte vectors: views off that boundary take the
        # generic kernels below
        k1p, k2p = _cv_mixed_keys(mix.to(k1.dtype), k1, k2)
        zero = q1.new_zeros((), dtype=torch.float32)
        LAST_PATH["crossview_fwd"] = L.PATH_FUSED
        return _DualPathFn.apply(q1, k1p, v1, q2, k2p, v1, zero, (1.0, 0.0, 0.0, 0.0), 0.0, 0, attn_mask, causal, prec, L.PATH_FUSED, drop)
    LAST_PATH["crossview_fwd"] = L.PATH_GENERIC
    cfg = (float(t1), float(t2), float(prior_weight), int(prior_weight > 0.0), _ANCHOR_MODES.get(anchor_mode, 2), int(fixed_k_star))
    return _CrossViewFn.apply(q1, k1, v1, q2, k2, mix, cfg, attn_mask, causal, prec, drop)


@_half_via_fp32
def crossview_core_packed(qkv1, qkv2, mix, t1=0.0, t2=0.0, prior_weight=0.0, anchor_mode="argmax_row_sum", fixed_k_star=0,
                          attn_mask=None, causal=False, dropout_p: float = 0.0, seed: Optional[int] = None):
    """`crossview_core` from the packed (B,N,3,H,dk) outputs of the two qkv projections: on the fused route (no transpose cues, no
    prior, bf16 arithmetic, dk 32 / 64) one Function builds the mixed keys, runs the two-score kernels and hands back ONE gradient per
    projection; otherwise the views go to `crossview_core`."""
    if qkv1.shape[0] == 0:
        return _empty_batch(qkv1, 0, qkv1.shape[1], qkv1.shape[-2] * qkv1.shape[-1])
    prec = _prec_for(qkv1.dtype)
    if _cv_folds(t1, t2, prior_weight, prec, qkv1.shape[-1]):
        drop = _drop(dropout_p, seed)
        LAST_PATH["crossview_fwd"] = L.PATH_FUSED
        return _CrossViewFoldedFn.apply(qkv1, qkv2, mix, attn_mask, causal, prec, drop)
    return crossview_core(qkv1[:, :, 0], qkv1[:, :, 1], qkv1[:, :, 2], qkv2[:, :, 0], qkv2[:, :, 1], mix, t1=t1, t2=t2,
                          prior_weight=prior_weight, anchor_mode=anchor_mode, fixed_k_star=fixed_k_star, attn_mask=attn_mask, causal=causal,
                          dropout_p=dropout_p, seed=seed)


def _dp_args(ts, lg, y, gates, beta_not, hops, mask, causal, prec, path, drop) -> L.DualPathArgs:
    """the MopkDualPathArgs fields forward and backward share; ts: the six (B,N,H,dk) views q1 k1 v1 q2 k2 v2"""
    B, N, H, dk = ts[0].shape
    a = L.DualPathArgs()
    a.B, a.H, a.N, a.dk, a.hops = B, H, N, dk, hops
    a.io_dtype, a.precision, a.path, a.causal = _io_dtype(ts[0]), prec, path, int(bool(causal))
    a.g_and, a.g_or, a.g_not, a.g_chain = (float(g) for g in gates)
    a.beta_not = float(beta_not)
    a.q1, a.k1, a.v1, a.q2, a.k2, a.v2 = (_v4(t) for t in ts)
    a.mask, (a.mask_sb, a.mask_sh, a.mask_si) = _ptr(mask[0]), mask[1]
    a.chain_logit, a.y = lg.data_ptr(), _v4(y)
    a.dropout_p, a.dropout_seed = float(drop[0]), int(drop[1])
    return a


def _dp_fwd(ts, lg, gates, beta_not, hops, mask, causal, prec, path, drop):
    """one mopk_dualpath_fwd call on six (B,N,H,dk) views -> (y (B,N,H,dk), saved, resolved path)"""
    B, N, H, dk = ts[0].shape
    dev = ts[0].device
    y = torch.empty(B, N, H, dk, dtype=ts[0].dtype, device=dev)
    a = _dp_args(ts, lg, y, gates, beta_not, hops, mask, causal, prec, path, drop)
    return (y, *_core_launch("dualpath", a, dev))


def _dp_bwd(ts, lg, y, saved, dy, gs, gates, beta_not, hops, mask, causal, prec, path, drop):
    """one mopk_dualpath_bwd call: gradients into the six (B,N,H,dk) views `gs`; -> d chain_logit partials (B,H)"""
    B, N, H, dk = ts[0].shape
    dev = ts[0].device
    a = _dp_args(ts, lg, y, gates, beta_not, hops, mask, causal, prec, path, drop)
    a.dy = _v4(dy)
    a.dq1, a.dk1, a.dv1, a.dq2, a.dk2, a.dv2 = (_v4(g) for g in gs)
    dlg = torch.empty(B, H, dtype=torch.float32, device=dev)
    a.dlogit_part = dlg.data_ptr()
    _core_launch("dualpath", a, dev, saved)
    return dlg


class _DualPathFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q1, k1, v1, q2, k2, v2, logit, gates, beta_not, hops, mask, causal, prec, path, drop=(0.0, 0)):
        _require_gpu(q1, "MultiHopMSA")
        ctx.packed = k1 is None            # packed form: q1 / q2 are the (B,N,3,H,dk) outputs of the two qkv projections (see _SdpaFn)
        if ctx.packed:
            q1, k1, v1 = q1.contiguous().unbind(2)
            q2, k2, v2 = q2.contiguous().unbind(2)
        ts = [_heads_view(t) for t in (q1, k1, v1, q2, k2, v2)]
        B, N, H, dk = ts[0].shape
        lg = _f32c(logit).reshape(1)
        mask = _mask_u8(mask, B, H, N, ts[0].device)
        y, saved, path = _dp_fwd(ts, lg, gates, beta_not, hops, mask, causal, prec, path, drop)
        ctx.save_for_backward(*ts, lg, y, saved)
        ctx.meta = (gates, beta_not, hops, causal, prec, path, mask, drop)
        return y.view(B, N, H * dk)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        *ts, lg, y, saved = ctx.saved_tensors
        gates, beta_not, hops, causal, prec, path, mask, drop = ctx.meta
        B, N, H, dk = ts[0].shape
        dev = ts[0].device
        dy = _grad_in(dy, ts[0].dtype, (B, N, H, dk))
        mk = torch.zeros if hops == 0 else torch.empty          # hops == 0: dv2 is never written
        if ctx.packed:
            packs = [mk(B, N, 3, H, dk, dtype=ts[0].dtype, device=dev) for _ in range(2)]
            gs = [*packs[0].unbind(2), *packs[1].unbind(2)]
        else:
            gs = [mk(B, N, H, dk, dtype=ts[0].dtype, device=dev) for _ in range(6)]
        dlg = _dp_bwd(ts, lg, y, saved, dy, gs, gates, beta_not, hops, mask, causal, prec, path, drop)
        if ctx.packed:
            return (packs[0], None, None, packs[1], None, None, dlg.sum().reshape(()), None, None, None, None, None, None, None, None)
        return (*gs, dlg.sum().reshape(()), None, None, None, None, None, None, None, None)


class _CrossViewFoldedFn(torch.autograd.Function):
    """CrossViewMixerMSA without transpose cues / prior on the fused two-score kernels, from the PACKED projections:
    S = q1 (m11 k1 + m12 k2)^T + q2 (m21 k1 + m22 k2)^T (reference :99-105): the 2x2 mix folds into two mixed key tensors built here
    (no autograd graph), the core is the dual-path kernel pair without the transport term (hops = 0, v2 unused), and the backward
    un-mixes dk1' / dk2' into dk1, dk2 and d mix and writes ONE gradient per projection."""

    @staticmethod
    def forward(ctx, qkv1, qkv2, mix, mask, causal, prec, drop):
        _require_gpu(qkv1, "CrossViewMixerMSA")
        q1, k1, v1 = qkv1.contiguous().unbind(2)
        q2, k2, _ = qkv2.contiguous().unbind(2)
        B, N, H, dk = q1.shape
        k1p, k2p = _cv_mixed_keys(mix.detach().to(k1.dtype), k1, k2)
        ts = [q1, k1p, v1, q2, k2p, v1]
        lg = torch.zeros(1, dtype=torch.float32, device=q1.device)
        mask = _mask_u8(mask, B, H, N, q1.device)
        y, saved, path = _dp_fwd(ts, lg, (1.0, 0.0, 0.0, 0.0), 0.0, 0, mask, causal, prec, L.PATH_FUSED, drop)
        ctx.save_for_backward(qkv1, qkv2, mix, k1p, k2p, lg, y, saved)
        ctx.meta = (causal, prec, path, mask, drop)
        return y.view(B, N, H * dk)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        qkv1, qkv2, mix, k1p, k2p, lg, y, saved = ctx.saved_tensors
        causal, prec, path, mask, drop = ctx.meta
        q1, k1, v1 = qkv1.unbind(2)
        q2, k2, _ = qkv2.unbind(2)
        B, N, H, dk = q1.shape
        dev = q1.device
        dy = _grad_in(dy, q1.dtype, (B, N, H, dk))
        d1, d2 = torch.empty_like(qkv1), torch.zeros_like(qkv2)            # v2 receives no gradient (:98)
        dk1p, dk2p = torch.empty(B, N, H, dk, dtype=q1.dtype, device=dev), torch.empty(B, N, H, dk, dtype=q1.dtype, device=dev)
        dv2 = torch.zeros(B, N, H, dk, dtype=q1.dtype, device=dev)          # hops == 0: never written
        gs = [d1[:, :, 0], dk1p, d1[:, :, 2], d2[:, :, 0], dk2p, dv2]
        _dp_bwd([q1, k1p, v1, q2, k2p, v1], lg, y, saved, dy, gs, (1.0, 0.0, 0.0, 0.0), 0.0, 0, mask, causal, prec, path, drop)
        m = mix.detach().to(q1.dtype)
        d1k, d2k = d1[:, :, 1], d2[:, :, 1]                                  # k1' = m11 k1 + m12 k2, k2' = m21 k1 + m22 k2
        torch.mul(dk1p, m[0, 0], out=d1k); d1k.addcmul_(dk2p, m[1, 0])
        torch.mul(dk1p, m[0, 1], out=d2k); d2k.addcmul_(dk2p, m[1, 1])
        f = lambda x, y_: (x.float() * y_.float()).sum()
        dmix = torch.stack([torch.stack([f(dk1p, k1), f(dk1p, k2)]), torch.stack([f(dk2p, k1), f(dk2p, k2)])]).to(mix.dtype)
        return d1, d2, dmix, None, None, None, None


@_half_via_fp32
def dualpath_core(q1, k1, v1, q2, k2, v2, chain_logit, g_and, g_or, g_not, g_chain, beta_not, hops,
                  attn_mask=None, causal=False, dropout_p: float = 0.0, seed: Optional[int] = None):
    """q*, k*, v*: (B,N,H,dk) views -- or packed: q1 / q2 = the (B,N,3,H,dk) outputs of the two qkv projections, k1 = v1 = k2 = v2 = None"""
    if q1.shape[0] == 0:
        return _empty_batch(q1, 0, q1.shape[1], q1.shape[-2] * q1.shape[-1])
    drop = _drop(dropout_p, seed)
    return _DualPathFn.apply(q1, k1, v1, q2, k2, v2, chain_logit, (g_and, g_or, g_not, g_chain), beta_not,
                             int(hops), attn_mask, causal, _prec_for(q1.dtype), _PATH, drop)


def _qt_args(ts, sc, y, am, eps, prec, path, drop, lens=None):
    """the MopkQuartetArgs fields forward and backward share; ts: the (B,T,H,dh) views q k v, plus q2 k2 with the quartet term,
    whose float32 scalars are sc = (mixture, scale); am: (additive mask or None, strides) from _bias_f32.
    lens: int32 (B,) device tensor -> the MopkQuartetLensArgs that wraps them"""
    B, T, H, dh = ts[0].shape
    a = L.QuartetArgs()
    a.B, a.H, a.T, a.dh = B, H, T, dh
    a.io_dtype, a.precision, a.path = _io_dtype(ts[0]), prec, path
    a.use_quartet, a.eps = int(len(ts) == 5), float(eps)
    a.q, a.k, a.v, a.y = _v4(ts[0]), _v4(ts[1]), _v4(ts[2]), _v4(y)
    if len(ts) == 5:
        a.q2, a.k2 = _v4(ts[3]), _v4(ts[4])
        a.mixture, a.quartet_scale = sc[0].data_ptr(), sc[1].data_ptr()
    a.add_mask, (a.am_sb, a.am_sh, a.am_si) = _ptr(am[0]), am[1]
    a.dropout_p, a.dropout_seed = float(drop[0]), int(drop[1])
    return a if lens is None else L.QuartetLensArgs(base=a, lens=_ptr(lens))


def _qt_fwd(ctx, q, k, v, q2, k2, mixture, qscale, add_mask, lens, eps, use_quartet, need_weights, prec, path, drop):
    """the forward of _QuartetFn (lens None) and _QuartetLensFn (add_mask None)"""
    _require_gpu(q, "CausalSelfAttention")
    ts = [_heads_view(t) for t in ((q, k, v, q2, k2) if use_quartet else (q, k, v))]
    B, T, H, dh = ts[0].shape
    dev = ts[0].device
    sc = [_f32c(mixture).reshape(1), _f32c(qscale).reshape(1)] if use_quartet else []
    am = _bias_f32(add_mask, B, H, T, dev)
    y = torch.empty(B, T, H, dh, dtype=ts[0].dtype, device=dev)
    a = _qt_args(ts, sc, y, am, eps, prec, path, drop, lens)
    attn = torch.empty(B, H, T, T, dtype=torch.float32, device=dev) if need_weights else None
    getattr(a, "base", a).attn = _ptr(attn)
    saved, path = _core_launch("quartet" if lens is None else "quartet_lens", a, dev)
    ctx.save_for_backward(*ts, *sc, y, saved)
    ctx.meta = (eps, use_quartet, prec, path, am, drop)
    ctx.lens = lens
    out = y.view(B, T, H * dh)
    if need_weights:
        ctx.mark_non_differentiable(attn)
        return out, attn
    return out


def _qt_bwd(ctx, dy):
    """the backward of both on dy as _grad_in returns it, (B,T,H,dh): the five (three) input gradients and the two scalar gradients
    (None without the quartet term)"""
    eps, use_quartet, prec, path, am, drop = ctx.meta
    n = 5 if use_quartet else 3
    *ts, y, saved = ctx.saved_tensors
    ts, sc = ts[:n], ts[n:]
    B, T, H, dh = ts[0].shape
    dev = ts[0].device
    a = _qt_args(ts, sc, y, am, eps, prec, path, drop, ctx.lens)
    base = getattr(a, "base", a)
    base.dy = _v4(dy)
    gs = [torch.empty(B, T, H, dh, dtype=ts[0].dtype, device=dev) for _ in range(n)]
    base.dq, base.dk_, base.dv = _v4(gs[0]), _v4(gs[1]), _v4(gs[2])
    if use_quartet:
        base.dq2, base.dk2 = _v4(gs[3]), _v4(gs[4])
        dmix = torch.empty(B, H, dtype=torch.float32, device=dev)
        dqs = torch.empty(B, H, dtype=torch.float32, device=dev)
        base.dmixture_part, base.dqscale_part = dmix.data_ptr(), dqs.data_ptr()
    _core_launch("quartet" if base is a else "quartet_lens", a, dev, saved)
    if use_quartet:
        return gs[0], gs[1], gs[2], gs[3], gs[4], dmix.sum().reshape(1), dqs.sum().reshape(1)
    return gs[0], gs[1], gs[2], None, None, None, None


class _QuartetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, q2, k2, mixture, qscale, add_mask, eps, use_quartet, need_weights, prec, path, drop=(0.0, 0)):
        return _qt_fwd(ctx, q, k, v, q2, k2, mixture, qscale, add_mask, None, eps, use_quartet, need_weights, prec, path, drop)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy, *unused):
        q = ctx.saved_tensors[0]
        return (*_qt_bwd(ctx, _grad_in(dy, q.dtype, q.shape)), None, None, None, None, None, None, None)


# _QuartetLensFn, the Function of the call with per-row lengths, is in mop_amd/gpt_lens_fn.py (imported at the end of this file)


@_half_via_fp32
def quartet_core(q, k, v, q2, k2, mixture, quartet_scale, add_mask, eps, use_quartet, need_weights=False,
                 dropout_p: float = 0.0, seed: Optional[int] = None, lens=None):
    """q, k, v (and q2, k2 with use_quartet): (B,T,H,dk) views.  Returns (B,T,H*dk), and the (B,H,T,T) float32 weights with
    need_weights.  add_mask: additive, broadcastable to (B,H,T,T) along any axis, the key axis included; it gets no gradient.
    lens: int32 (B,) tensor on q's device for a batch of right-padded rows, n_b = clamp(lens[b], 0, T) (mopk_quartet_lens_*;
    `quartet_core_lens_torch` states the semantics).  Row i < n_b normalises both score maps over the keys j < n_b only and attends
    to j <= i, so it comes out as the row alone would; padding rows give y = 0 (zero rows and columns of the returned weights),
    get zero gradients and add nothing to the gradients of mixture / quartet_scale.  Nothing at or beyond a length is read (NaN
    included), the dropout mask is indexed by the padded positions, full lengths are bitwise the call without lengths, and there
    is no host synchronisation.  lens with add_mask raises ValueError."""
    _refuse_bias_grad(add_mask, "quartet_core: add_mask")      # add_mask gets no gradient
    if lens is not None:
        if add_mask is not None:
            raise ValueError("quartet_core: lens and add_mask do not combine (an additive mask acts after the row normalisation)")
        _check_lens(lens, q.shape[0], q.device, "lens", "quartet_core")
    if q.shape[0] == 0:                   # q: (B,T,H,dk)
        out = _empty_batch(q, 0, q.shape[1], q.shape[2] * q.shape[3])
        return (out, q.new_zeros((0, q.shape[2], q.shape[1], q.shape[1]), dtype=torch.float32)) if need_weights else out
    drop = _drop(dropout_p, seed)
    if lens is not None:
        return _gpt_lens_fn._QuartetLensFn.apply(q, k, v, q2, k2, mixture, quartet_scale, lens, eps, use_quartet, need_weights,
                                    _prec_for(q.dtype), _PATH, drop)
    return _QuartetFn.apply(q, k, v, q2, k2, mixture, quartet_scale, add_mask, eps, use_quartet, need_weights,
                            _prec_for(q.dtype), _PATH, drop)


def quartet_core_lens_torch(q, k, v, q2, k2, mixture, quartet_scale, lens, eps, use_quartet, need_weights=False):
    """The semantics of `quartet_core(..., lens=)` in torch ops, on any device and dtype (no dropout): row b is the core on its
    first n_b = clamp(lens[b], 0, T) tokens alone -- statistics over n_b keys, unbiased std with max(n_b - 1, 1) -- padded back
    with zeros.  Reads lens on the host; the statement of the semantics and the tests' reference, not a fast path."""
    B, T, H, dh = q.shape
    y = q.new_zeros(B, T, H * dh)
    attn = q.new_zeros(B, H, T, T)
    for b, n in enumerate(int(x) for x in lens.clamp(0, T).tolist()):
        if n == 0:
            continue
        hv = lambda t: t[b, :n].transpose(0, 1)                        # (H, n, dh)
        def z(a, c, e):
            s = (hv(a) @ hv(c).transpose(-1, -2)) / math.sqrt(dh)
            mu = s.mean(-1, keepdim=True)
            var = ((s - mu) ** 2).sum(-1, keepdim=True).div(max(n - 1, 1))
            pos = var > 0                                              # sd == 0 (a single key): z = 0 with a zero gradient, not 0 * inf
            sd = torch.where(pos, torch.where(pos, var, torch.ones_like(var)).sqrt(), torch.zeros_like(var))
            return (s - mu) / (sd + e)
        if use_quartet:
            z1, z2 = z(q, k, eps), z(q2, k2, eps)
            m = torch.sigmoid(mixture.to(z1.dtype)).reshape(())
            sc = (1 - m) * z1 + m * (z1 * z2) * quartet_scale.to(z1.dtype).reshape(())
        else:
            sc = z(q, k, 1e-5)
        causal = torch.ones(n, n, dtype=torch.bool, device=q.device).tril()
        P = torch.softmax(sc.masked_fill(~causal, float("-inf")), -1)
        y[b, :n] = (P @ hv(v)).transpose(0, 1).reshape(n, H * dh)
        attn[b, :, :n, :n] = P
    return (y, attn.detach().float()) if need_weights else y


# ---- LayerNorm prologue / residual epilogue around the cores (mopk_layernorm_*) ----
def layernorm_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """calls the HIP prologue covers (anything else: the caller keeps torch's LayerNorm): the shapes and dtypes, and an input the
    kernels can read with 16-byte loads -- a contiguous x is passed as it is, so it has to sit on a 16-byte boundary"""
    d = x.shape[-1]
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and weight.dtype in (torch.float32, torch.bfloat16)
            and d % 8 == 0 and d <= 4096 and x.numel() > 0 and (not x.is_contiguous() or x.data_ptr() % 16 == 0))


def _ln_args(xc, w, mean, rstd, y, eps) -> L.LayerNormArgs:
    """the MopkLayerNormArgs fields forward and backward share; xc: contiguous (..., dim) input, y: the output (forward) or its
    gradient (backward), whose dtype is y_dtype"""
    d = xc.shape[-1]
    return L.LayerNormArgs(rows=xc.numel() // d, dim=d, x_dtype=_io_dtype(xc), y_dtype=_io_dtype(y), p_dtype=_io_dtype(w), eps=float(eps),
                           x_ld=d, y_ld=d, x=_ptr(xc), gamma=_ptr(w), mean=_ptr(mean), rstd=_ptr(rstd))


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype, with_residual):
        _require_gpu(x, "layernorm")
        xc = x.contiguous()
        rows = xc.numel() // xc.shape[-1]
        y = torch.empty(xc.shape, dtype=out_dtype, device=x.device)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        w = weight.detach().contiguous()
        b = None if bias is None else bias.detach().to(w.dtype).contiguous()
        a = _ln_args(xc, w, mean, rstd, y, eps)
        a.beta, a.y = _ptr(b), _ptr(y)
        _launch("mopk_layernorm_fwd", a, "layernorm_fwd")
        ctx.save_for_backward(xc, w, mean, rstd)
        ctx.meta = (float(eps), bias is not None, with_residual, weight.dtype, None if bias is None else bias.dtype)
        if with_residual:
            return xc.view_as(xc), y
        return y

    @staticmethod
    @_once_differentiable
    def backward(ctx, *grads):
        xc, w, mean, rstd = ctx.saved_tensors
        eps, has_bias, with_residual, wdt, bdt = ctx.meta
        dres, dy = (grads if with_residual else (None, grads[0]))
        d = xc.shape[-1]
        if dy is None:                                    # only the residual branch carries a gradient
            return (dres, None, None, None, None, None)
        dy = _grad_in(dy, dy.dtype)
        if dres is not None:
            dres = _grad_in(dres, xc.dtype)
        dx = torch.empty_like(xc)
        dg = torch.empty(d, dtype=torch.float32, device=xc.device)
        db = torch.empty(d, dtype=torch.float32, device=xc.device) if has_bias else None
        a = _ln_args(xc, w, mean, rstd, dy, eps)
        a.dy, a.dres, a.dx, a.dgamma, a.dbeta = _ptr(dy), _ptr(dres), _ptr(dx), _ptr(dg), _ptr(db)
        ws = torch.empty(max(1, L.lib().mopk_layernorm_workspace_bytes(C.byref(a))), dtype=torch.uint8, device=xc.device)
        a.workspace = _ptr(ws)
        _launch("mopk_layernorm_bwd", a, "layernorm_bwd")
        return dx, dg.to(wdt), (db.to(bdt) if has_bias else None), None, None, None


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5,
              out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``F.layer_norm(x, (dim,), weight, bias, eps)`` written in ``out_dtype`` (default: x.dtype) by one HIP pass."""
    return _LayerNormFn.apply(x, weight, bias, eps, out_dtype or x.dtype, False)


def layernorm_residual(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], eps: float = 1e-5,
                       out_dtype: Optional[torch.dtype] = None):
    """(x_res, ln(x)) for a pre-norm residual branch ``x_res + f(ln(x))``: ``x_res`` is ``x`` itself, routed through the same
    autograd node so that the backward returns ``d x_res + LN'(d ln)`` from ONE kernel instead of LN backward + an add."""
    return _LayerNormFn.apply(x, weight, bias, eps, out_dtype or x.dtype, True)


# ---- 1-D MoP token gate of the GPT-MoP block (mopk_token_gate_*; reference mop/models/gpt_mop.py:109-123) ----
def token_gate_taps(Wv: torch.Tensor, Wk: torch.Tensor, Wf: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """Fold the gate's linear chain into three taps u (3, D), differentiable in all four parameters.

    views = Wv r ; K_t = sum_j Wk[:,:,j] views_{t+j-1} ; g = Wf [views ; K] ; gate = 1 + alpha0 g0 - alpha1 g1.  With
    w = (alpha0, -alpha1) Wf, w_V = w[:V], w_K = w[V:], c_j = sum_k w_K[k] Wk[k,:,j] and m_j = c_j + [j = 1] w_V:
    gate_t = 1 + sum_j (Wv^T m_j) . r_{t+j-1}.   Wv (V,D) = views.proj.weight, Wk (K,V,3) = kernels.conv.weight,
    Wf (2,V+K,1) = fuse.conv.weight, alpha (2,) = fuse.alpha.  Computed in fp32 (float64 for float64 parameters)."""
    with torch.autocast(device_type=Wv.device.type, enabled=False):
        V = Wv.shape[0]
        ct = torch.float64 if Wv.dtype == torch.float64 else torch.float32
        f32 = lambda t: t.to(ct)
        a = torch.stack((f32(alpha[0]), -f32(alpha[1])))
        w = a @ f32(Wf).reshape(2, -1)                             # (V+K,)
        m = torch.einsum("k,kvj->jv", w[V:], f32(Wk))              # (3, V)
        m = m + torch.stack((torch.zeros_like(w[:V]), w[:V], torch.zeros_like(w[:V])))
        return m @ f32(Wv)                                         # (3, D)


def token_gate_1d_torch(x: torch.Tensor, a: Optional[torch.Tensor], u: torch.Tensor, lens=None) -> torch.Tensor:
    """the folded gate in torch ops (any device / dtype): r = x + a, out_t = r_t (1 + u0.r_{t-1} + u1.r_t + u2.r_{t+1}).
    lens: int (B,) tensor of a right-padded batch -- r_t counts as 0 for t >= lens[b] (whatever it holds, NaN included), so the
    last real token has no u2 term and padding rows come out 0 with zero gradients (torch ops on the device, no host sync)"""
    r = x if a is None else x + a
    if lens is not None:
        keep = torch.arange(r.shape[1], device=r.device).view(1, -1) < lens.to(r.device).view(-1, 1)
        r = torch.where(keep.unsqueeze(-1), r, torch.zeros((), dtype=r.dtype, device=r.device))
    p = torch.einsum("btd,sd->bts", r, u.to(r.dtype))              # (B,T,3)
    gate = 1 + p[..., 1]
    gate = gate + F.pad(p[:, :-1, 0], (1, 0)) + F.pad(p[:, 1:, 2], (0, 1))
    return r * gate.unsqueeze(-1)


def _tg_args(x: torch.Tensor, a: Optional[torch.Tensor], lens=None):
    """the MopkTokenGateArgs fields every call shares; lens: int32 (B,) device tensor -> the MopkTokenGateLensArgs that wraps them"""
    B, T, D = x.shape
    g = L.TokenGateArgs()
    g.B, g.T, g.D = B, T, D
    g.x_dtype = _io_dtype(x)
    g.x, g.x_sb, g.x_st = x.data_ptr(), (x.stride(0) if B > 1 else 0), (x.stride(1) if T > 1 else D)
    f32 = x.dtype == torch.float32
    if a is not None:
        g.a_dtype = _io_dtype(a)
        g.a, g.a_sb, g.a_st = a.data_ptr(), (a.stride(0) if B > 1 else 0), (a.stride(1) if T > 1 else D)
        f32 = f32 or a.dtype == torch.float32
    g.o_dtype = L.MOPK_F32 if f32 else L.MOPK_BF16
    return g if lens is None else L.TokenGateLensArgs(base=g, lens=_ptr(lens))


def token_gate_supported(x: torch.Tensor, a: Optional[torch.Tensor] = None, lens=None) -> bool:
    """True if mopk_token_gate_* take this call: GPU tensors, fp32 / bf16 (mixed pairs included), (B,T,D) with D % 8 == 0 and
    D <= 1024, innermost dimension contiguous, row strides multiples of 8, 16-byte aligned data (the library's own query).
    lens: the same question for mopk_token_gate_lens_* with these int32 (B,) lengths."""
    ts = (x,) if a is None else (x, a)
    if any(not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 3 or t.stride(-1) != 1 for t in ts):
        return False
    if a is not None and a.shape != x.shape:
        return False
    if x.numel() == 0:
        return False
    if lens is not None:
        return bool(L.lib().mopk_token_gate_lens_supported(C.byref(_tg_args(x, a, lens))))
    return bool(L.lib().mopk_token_gate_supported(C.byref(_tg_args(x, a))))


def _tg_fwd(ctx, x, a, u, lens):
    """the forward of _TokenGateFn (lens None) and _TokenGateLensFn"""
    ga = _tg_args(x, a, lens)
    g = getattr(ga, "base", ga)
    stem = "mopk_token_gate" if lens is None else "mopk_token_gate_lens"
    B, T, D = x.shape
    uc = u.detach().to(torch.float32).contiguous()
    odt = torch.float32 if g.o_dtype == L.MOPK_F32 else torch.bfloat16
    out = torch.empty(B, T, D, dtype=odt, device=x.device)
    gate = torch.empty(B, T, dtype=torch.float32, device=x.device)
    g.u, g.out, g.gate = uc.data_ptr(), out.data_ptr(), gate.data_ptr()
    LAST_PATH["token_gate_fwd"] = L.PATH_FUSED
    _launch(stem + "_fwd", ga, "token_gate_fwd")
    ctx.save_for_backward(x, a, uc, gate)
    ctx.u_dtype, ctx.lens, ctx.o_dtype = u.dtype, lens, odt
    return out


def _tg_bwd(ctx, dout):
    """the backward of both on dout as _grad_in returns it: (dx, da, du)"""
    lib = L.lib()
    x, a, uc, gate = ctx.saved_tensors
    ga = _tg_args(x, a, ctx.lens)
    g = getattr(ga, "base", ga)
    stem = "mopk_token_gate" if ctx.lens is None else "mopk_token_gate_lens"
    odt = ctx.o_dtype
    dr = torch.empty(x.shape, dtype=odt, device=x.device)
    du = torch.empty(3, x.shape[2], dtype=torch.float32, device=x.device)
    g.u, g.gate, g.dout, g.dr, g.du = uc.data_ptr(), gate.data_ptr(), dout.data_ptr(), dr.data_ptr(), du.data_ptr()
    ws = _bytes(getattr(lib, stem + "_workspace_bytes")(C.byref(ga)), x.device)
    g.workspace = ws.data_ptr()
    LAST_PATH["token_gate_bwd"] = L.PATH_FUSED
    _launch(stem + "_bwd", ga, "token_gate_bwd")
    dx = dr.to(x.dtype) if ctx.needs_input_grad[0] else None
    da = dr.to(a.dtype) if a is not None and ctx.needs_input_grad[1] else None
    return dx, da, (du.to(ctx.u_dtype) if ctx.needs_input_grad[2] else None)


class _TokenGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, u):
        return _tg_fwd(ctx, x, a, u, None)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dout):
        return _tg_bwd(ctx, _grad_in(dout, ctx.o_dtype))


# _TokenGateLensFn is in mop_amd/gpt_lens_fn.py


def token_gate_1d(x: torch.Tensor, a: Optional[torch.Tensor], u: torch.Tensor, lens=None) -> torch.Tensor:
    """out = r * gate with r = x + a (a may be None) and gate_t = 1 + u0.r_{t-1} + u1.r_t + u2.r_{t+1} (zero padding per sequence):
    the GPT-MoP block's residual add and token gate as one HIP kernel forward and two launches backward.  x, a: (B,T,D); u: (3,D)
    from token_gate_taps.  Output dtype: the promotion of x and a.  Calls the kernels do not take (token_gate_supported) run the
    same formula in torch ops; LAST_PATH["token_gate_fwd"] records which (PATH_FUSED / PATH_GENERIC).
    lens: int32 (B,) tensor on x's device for a batch of right-padded rows, n_b = clamp(lens[b], 0, T) (mopk_token_gate_lens_*):
    r_t counts as 0 for t >= n_b, so the last real token has no u2 term; padding rows come out 0, get dr = 0, add nothing to du
    and are never read (NaN included).  Full lengths are bitwise the call without lengths; no host synchronisation."""
    if lens is not None:
        _check_lens(lens, x.shape[0], x.device, "lens", "token_gate_1d", "x")
    if not token_gate_supported(x, a, lens):
        LAST_PATH["token_gate_fwd"] = L.PATH_GENERIC
        return token_gate_1d_torch(x, a, u, lens)
    if lens is not None:
        return _gpt_lens_fn._TokenGateLensFn.apply(x, a, u, lens)
    return _TokenGateFn.apply(x, a, u)


# ---- MoP mel gate of the WhisperMoP encoder (mopk_mel_gate_*, mopk_gated_residual_*; reference mop/models/whisper_mop.py:91-124) ----
# the two autograd Functions of this family are in mop_amd/mel_gate_fn.py (imported at the end of this file)
def mel_gate_taps(Wv: torch.Tensor, Wk: torch.Tensor, Wf: torch.Tensor, alpha: torch.Tensor, n_mels: int) -> torch.Tensor:
    """Fold the MoP2D chains of L encoder layers into taps W (L, k, n_mels), differentiable in all four parameters.

    views = Wv mel ; K = conv2d(views, Wk, pad k//2) ; g = Wf [views ; K] ; gate = 1 + alpha0 mean_F g0 - alpha1 mean_F g1.  With
    w = (alpha0, -alpha1) Wf, u[i,j] = sum_{kk,v} w[V+kk] Wk[kk,v,i,j] Wv[v] + [i = j = p] sum_v w[v] Wv[v] (p = k // 2) the chain is
    one k x k stencil on the mel map, and its mean over frequency a stencil over time alone:
    gate[t] = 1 + sum_{i,f} mel[t+i-p, f] W[i,f],  W[i,f] = (1/F) sum_{j : 0 <= f-(j-p) < F} u[i,j]  (the zero padding in frequency).
    Wv (L,V,1,1) = views.conv.weight (the stacked conv weights' own (L,V,1,1,1) is taken too), Wk (L,K,V,k,k) = kernels.conv.weight, Wf (L,2,V+K,1,1) = fuse.conv.weight, alpha (L,2) =
    fuse.alpha, each stacked over the layers: the number of launches does not grow with L.  fp32 (float64 for float64 parameters)."""
    if Wv.dim() not in (4, 5) or Wk.dim() != 5 or Wf.dim() != 5 or alpha.dim() != 2:
        raise ValueError(f"mel_gate_taps: expects Wv (L,V,1,1), Wk (L,K,V,k,k), Wf (L,2,V+K,1,1) and alpha (L,2), got "
                         f"{tuple(Wv.shape)}, {tuple(Wk.shape)}, {tuple(Wf.shape)}, {tuple(alpha.shape)}")
    Ln, V = Wv.shape[:2]
    K, k = Wk.shape[1], Wk.shape[-1]
    if (Wv.numel() != Ln * V or tuple(Wk.shape) != (Ln, K, V, k, k) or tuple(Wf.shape) != (Ln, 2, V + K, 1, 1)
            or tuple(alpha.shape) != (Ln, 2) or int(n_mels) < 1):
        raise ValueError(f"mel_gate_taps: inconsistent shapes Wv {tuple(Wv.shape)}, Wk {tuple(Wk.shape)}, Wf {tuple(Wf.shape)}, "
                         f"alpha {tuple(alpha.shape)}, n_mels = {n_mels}")
    with torch.autocast(device_type=Wv.device.type, enabled=False):
        ct = torch.float64 if Wv.dtype == torch.float64 else torch.float32
        Fm, p = int(n_mels), k // 2
        wv = Wv.to(ct).reshape(Ln, V)
        a = torch.stack((alpha[:, 0], -alpha[:, 1]), dim=1).to(ct)                     # (L,2)
        w = torch.einsum("ls,lsc->lc", a, Wf.to(ct).reshape(Ln, 2, V + K))             # (L,V+K)
        u = torch.einsum("lc,lcvij,lv->lij", w[:, V:], Wk.to(ct), wv)                  # (L,k,k)
        j = torch.arange(k, device=Wv.device)
        centre = ((j == p).unsqueeze(1) & (j == p).unsqueeze(0)).to(ct)
        u = u + (w[:, :V] * wv).sum(dim=1).view(Ln, 1, 1) * centre
        src = torch.arange(Fm, device=Wv.device).unsqueeze(0) - (j.unsqueeze(1) - p)   # (k,F): the bin f - (j - p) tap j reads from
        inside = ((src >= 0) & (src < Fm)).to(ct) / Fm
        return u @ inside                                                              # (L,k,F)


def _mg_argcheck(mel: torch.Tensor, W: torch.Tensor, lens: Optional[torch.Tensor]) -> None:
    if mel.dim() != 3 or W.dim() != 3 or W.shape[2] != mel.shape[2] or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError(f"mel_gate: expects mel (B,T,F) and taps W (L,k,F), got {tuple(mel.shape)} and {tuple(W.shape)}")
    if not mel.dtype.is_floating_point or not W.dtype.is_floating_point:
        raise ValueError(f"mel_gate: mel and W must be floating point, got {mel.dtype} and {W.dtype}")
    if W.device != mel.device:
        raise ValueError(f"mel_gate: W is on {W.device}, mel on {mel.device}")
    if lens is not None and (lens.dtype != torch.int32 or tuple(lens.shape) != (mel.shape[0],) or lens.device != mel.device):
        raise ValueError(f"mel_gate: lens must be an int32 ({mel.shape[0]},) tensor on {mel.device}, got {lens.dtype} "
                         f"{tuple(lens.shape)} on {lens.device}")


def mel_gate_torch(mel: torch.Tensor, W: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the folded gates in torch ops (any device / dtype, differentiable in mel and W): gates (B,L,T) in the promotion of the two
    dtypes.  Rows t >= lens[b] of mel are replaced by zeros (whatever they hold), columns t >= lens[b] of the gates are 1."""
    _mg_argcheck(mel, W, lens)
    B, T, Fm = mel.shape
    k = W.shape[1]
    p = k // 2
    ct = torch.promote_types(mel.dtype, W.dtype)
    m = mel.to(ct)
    if lens is not None:
        live = torch.arange(T, device=mel.device).unsqueeze(0) < lens.unsqueeze(1)     # (B,T)
        m = torch.where(live.unsqueeze(-1), m, torch.zeros((), dtype=ct, device=mel.device))
    win = F.pad(m, (0, 0, p, k - 1 - p)).unfold(1, k, 1)                               # (B,T,F,k): frames t-p .. t-p+k-1
    gates = 1 + torch.einsum("btfi,lif->blt", win, W.to(ct))
    if lens is not None:
        gates = torch.where(live.unsqueeze(1), gates, torch.ones((), dtype=ct, device=mel.device))
    return gates


def _mg_args(mel: torch.Tensor, W: torch.Tensor, lens: Optional[torch.Tensor]) -> L.MelGateArgs:
    B, T, Fm = mel.shape
    g = L.MelGateArgs()
    g.B, g.T, g.F, g.L, g.k = B, T, Fm, W.shape[0], W.shape[1]
    g.mel_dtype = _io_dtype(mel)
    g.mel, g.mel_sb, g.mel_st = mel.data_ptr(), (mel.stride(0) if B > 1 else 0), (mel.stride(1) if T > 1 else Fm)
    g.lens = _ptr(lens)
    return g


def mel_gate_supported(mel: torch.Tensor, W: torch.Tensor, lens: Optional[torch.Tensor] = None) -> bool:
    """True if mopk_mel_gate_* take this call: a GPU mel (B,T,F) in fp32 / bf16 that needs no gradient, innermost dimension
    contiguous, fp32 taps (L,k,F) with an odd k <= 7 and F <= 128, lens None or a contiguous int32 (B,) (the library's own query)."""
    if mel.dim() != 3 or W.dim() != 3 or not mel.is_cuda or not W.is_cuda or mel.numel() == 0 or W.numel() == 0:
        return False
    if mel.dtype not in (torch.float32, torch.bfloat16) or W.dtype != torch.float32 or mel.stride(-1) != 1:
        return False
    if W.shape[2] != mel.shape[2] or (mel.requires_grad and torch.is_grad_enabled()):
        return False
    if lens is not None and (not lens.is_cuda or lens.dtype != torch.int32 or lens.dim() != 1 or not lens.is_contiguous()):
        return False
    return bool(L.lib().mopk_mel_gate_supported(C.byref(_mg_args(mel, W, lens))))


def mel_gate(mel: torch.Tensor, W: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gates (B,L,T) fp32 with gates[b,l,t] = 1 + sum_{i,f} mel[b,t+i-p,f] W[l,i,f] (p = k // 2, frames outside [0,T) are zero): the
    MoP2D gates of all L encoder layers from one pass over the mel map, one HIP launch forward (per 8 layers) and two backward
    (dW, bitwise reproducible; the parameters' gradients flow on through mel_gate_taps).  mel: (B,T,F); W: (L,k,F) from
    mel_gate_taps; lens: None or int32 (B,) on the device: rows t >= lens[b] of mel are not read and count as zeros, columns
    t >= lens[b] of the gates are exactly 1.  Calls the kernels do not take (mel_gate_supported: CPU tensors, float64, fp16, an
    even k, a mel that requires grad) run mel_gate_torch; LAST_PATH["mel_gate_fwd"] records which (PATH_FUSED / PATH_GENERIC)."""
    _mg_argcheck(mel, W, lens)
    if not mel_gate_supported(mel, W, lens):
        LAST_PATH["mel_gate_fwd"] = L.PATH_GENERIC
        return mel_gate_torch(mel, W, lens)
    return _mel_gate_fn._MelGateFn.apply(mel, W, lens)


def _gr_argcheck(x: torch.Tensor, a: torch.Tensor, gate: torch.Tensor) -> None:
    if x.dim() != 3 or a.shape != x.shape or tuple(gate.shape) != tuple(x.shape[:2]):
        raise ValueError(f"gated_residual: expects x and a (B,T,D) and gate (B,T), got {tuple(x.shape)}, {tuple(a.shape)} and "
                         f"{tuple(gate.shape)}")
    if not (x.dtype.is_floating_point and a.dtype.is_floating_point and gate.dtype.is_floating_point):
        raise ValueError(f"gated_residual: x, a and gate must be floating point, got {x.dtype}, {a.dtype} and {gate.dtype}")
    if a.device != x.device or gate.device != x.device:
        raise ValueError(f"gated_residual: x is on {x.device}, a on {a.device}, gate on {gate.device}")


def gated_residual_torch(x: torch.Tensor, a: torch.Tensor, gate: torch.Tensor) -> torch.Tensor:
    """(x + a) * gate[..., None] in torch ops (any device / dtype), in the promotion of x's and a's dtypes"""
    _gr_argcheck(x, a, gate)
    r = x + a
    return (r * gate.unsqueeze(-1)).to(r.dtype)


def _gr_args(x: torch.Tensor, a: torch.Tensor, gate: Optional[torch.Tensor]) -> L.GatedResidualArgs:
    """gate: fp32 (B,T) with a contiguous last dimension; None (support query only): a contiguous one yet to be made"""
    B, T, D = x.shape
    g = L.GatedResidualArgs()
    g.B, g.T, g.D = B, T, D
    g.x_dtype, g.a_dtype = _io_dtype(x), _io_dtype(a)
    g.x, g.x_sb, g.x_st = x.data_ptr(), (x.stride(0) if B > 1 else 0), (x.stride(1) if T > 1 else D)
    g.a, g.a_sb, g.a_st = a.data_ptr(), (a.stride(0) if B > 1 else 0), (a.stride(1) if T > 1 else D)
    g.gate, g.gate_sb = _ptr(gate), (gate.stride(0) if gate is not None and B > 1 else T)
    g.o_dtype = L.MOPK_F32 if torch.float32 in (x.dtype, a.dtype) else L.MOPK_BF16
    return g


def gated_residual_supported(x: torch.Tensor, a: torch.Tensor, gate: torch.Tensor) -> bool:
    """True if mopk_gated_residual_* take this call: GPU tensors, x and a (B,T,D) in fp32 / bf16 (mixed pairs included) with
    D % 8 == 0, innermost dimension contiguous, row strides multiples of 8, 16-byte aligned data, gate (B,T) in fp32 / bf16 /
    fp16 (the kernels read it as fp32) (the library's own query)."""
    if any(not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 3 or t.stride(-1) != 1 for t in (x, a)):
        return False
    if a.shape != x.shape or x.numel() == 0 or not gate.is_cuda or tuple(gate.shape) != tuple(x.shape[:2]):
        return False
    if gate.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    as_is = gate.dtype == torch.float32 and gate.stride(-1) == 1                  # else gated_residual makes a fresh fp32 copy
    return bool(L.lib().mopk_gated_residual_supported(C.byref(_gr_args(x, a, gate if as_is else None))))


def gated_residual(x: torch.Tensor, a: torch.Tensor, gate: torch.Tensor) -> torch.Tensor:
    """out = (x + a) * gate[..., None]: the WhisperMoP encoder block's residual add and mel gate as one HIP kernel, and
    dr = dout * gate, dgate = sum_d dout (x + a) as one more.  x, a: (B,T,D); gate: (B,T).  Output dtype: the promotion of x and
    a.  Calls the kernels do not take (gated_residual_supported) run gated_residual_torch; LAST_PATH["gated_residual_fwd"]
    records which (PATH_FUSED / PATH_GENERIC)."""
    _gr_argcheck(x, a, gate)
    if not gated_residual_supported(x, a, gate):
        LAST_PATH["gated_residual_fwd"] = L.PATH_GENERIC
        return gated_residual_torch(x, a, gate)
    if gate.dtype != torch.float32 or gate.stride(-1) != 1:
        gate = gate.to(torch.float32).contiguous()
    return _mel_gate_fn._GatedResidualFn.apply(x, a, gate)


# ---- top-1 routed MoE MLP (mopk_moe_*; reference mop/models/components.py:84-121 MoEMLP) ----
def moe_mlp_torch(x: torch.Tensor, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor], w1s, w2s,
                  residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the reference's dense composition in torch ops: every expert on every token, combined through a constant one-hot of the
    gate's argmax (so the gate receives no gradient and an expert without tokens gets exact zeros)"""
    D = x.shape[-1]
    xf = x.reshape(-1, D)
    logits = F.linear(xf, gate_w, gate_b)
    top = logits.argmax(dim=-1)
    one_hot = torch.zeros_like(logits).scatter_(1, top.unsqueeze(-1), 1.0)
    y = torch.zeros_like(xf)
    for e in range(len(w1s)):
        y = y + one_hot[:, e].unsqueeze(-1) * F.linear(F.gelu(F.linear(xf, w1s[e]), approximate="tanh"), w2s[e])
    y = y.reshape(x.shape)
    return y if residual is None else residual + y


def _moe_dtypes(x: torch.Tensor, w: torch.Tensor):
    """(output dtype, precision) of a kernel call, or None when the kernels do not take the dtypes: under autocast the expert GEMMs
    give the autocast dtype (as nn.Linear does) in bf16 arithmetic; otherwise x and the weights share a dtype"""
    if torch.is_autocast_enabled():
        if torch.get_autocast_dtype("cuda") != torch.bfloat16:
            return None
        return torch.bfloat16, L.PREC_BF16
    if x.dtype != w.dtype:
        return None
    return x.dtype, _prec_for(x.dtype)


def _moe_args(x2: Optional[torch.Tensor], gate_w, gate_b, w1s, w2s, odt: torch.dtype, prec: int, M: int = 0) -> L.MoeArgs:
    """the call's MopkMoeArgs; x2 = None (support query): M rows of w1s' width, x not set"""
    M, D = x2.shape if x2 is not None else (M, w1s[0].shape[1])
    a = L.MoeArgs()
    a.M, a.D, a.F, a.E = M, D, w1s[0].shape[0], len(w1s)
    a.precision = prec
    a.x_dtype = _io_dtype(x2 if x2 is not None else w1s[0])
    a.w_dtype, a.gate_dtype = _io_dtype(w1s[0]), _io_dtype(gate_w)
    a.o_dtype = L.MOPK_F32 if odt == torch.float32 else L.MOPK_BF16
    a.x, a.gate_w, a.gate_b = _ptr(x2), gate_w.data_ptr(), _ptr(gate_b)
    for e in range(len(w1s)):
        a.w1[e], a.w2[e] = w1s[e].data_ptr(), w2s[e].data_ptr()
    return a


def moe_supported(x: torch.Tensor, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor], w1s, w2s) -> bool:
    """True if mopk_moe_* take this call: GPU fp32 / bf16 tensors (bf16 autocast included), contiguous parameters of one dtype,
    D and F multiples of 8, 2 <= E <= 64 (the library's own query decides shape, precision and alignment)"""
    E = len(w1s)
    ts = [x, gate_w] + list(w1s) + list(w2s) + ([] if gate_b is None else [gate_b])
    if E < 2 or E > L.MOE_MAX_EXPERTS or x.numel() == 0:
        return False
    if any(not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16) for t in ts):
        return False
    if any(not w.is_contiguous() or w.dtype != w1s[0].dtype for w in list(w1s) + list(w2s)):
        return False
    if not gate_w.is_contiguous() or (gate_b is not None and (gate_b.dtype != gate_w.dtype or not gate_b.is_contiguous())):
        return False
    dt = _moe_dtypes(x, w1s[0])
    if dt is None:
        return False
    D = x.shape[-1]
    F_ = w1s[0].shape[0]
    if any(w.shape != (F_, D) for w in w1s) or any(w.shape != (D, F_) for w in w2s) or gate_w.shape != (E, D):
        return False
    a = _moe_args(None, gate_w, gate_b, w1s, w2s, *dt, M=x.numel() // D)
    a.x_dtype = _io_dtype(x)
    if x.is_contiguous():       # passed to the kernels as it is (a strided x is copied first): the query sees its alignment
        a.x = x.data_ptr()
    return bool(L.lib().mopk_moe_supported(C.byref(a)))


def _moe_route_buf(M: int, E: int, dev) -> torch.Tensor:
    return torch.empty(2 * M + E + 1, dtype=torch.int32, device=dev)


class _MoeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gate_w, gate_b, n_exp, *ws):
        w1s, w2s = ws[:n_exp], ws[n_exp:]
        D = x.shape[-1]
        x2 = x.detach().reshape(-1, D).contiguous()
        odt, prec = _moe_dtypes(x, w1s[0])
        a = _moe_args(x2, gate_w.detach(), None if gate_b is None else gate_b.detach(), w1s, w2s, odt, prec)
        M, F_ = a.M, a.F
        adt = torch.bfloat16 if prec == L.PREC_BF16 else torch.float32
        y = torch.empty(M, D, dtype=odt, device=x.device)
        u = torch.empty(M, F_, dtype=adt, device=x.device)
        h = torch.empty_like(u)
        route = _moe_route_buf(M, n_exp, x.device)
        res = None
        if residual is not None:
            res = residual.detach().reshape(-1, D).contiguous()
            a.residual = res.data_ptr()
        a.y, a.u, a.h, a.route = y.data_ptr(), u.data_ptr(), h.data_ptr(), route.data_ptr()
        LAST_PATH["moe_fwd"] = L.PATH_FUSED
        _launch("mopk_moe_fwd", a, "moe_fwd")
        ctx.save_for_backward(x2, gate_w, gate_b, u, h, route, *ws)
        ctx.meta = (n_exp, odt, prec, x.shape, x.dtype, residual is not None)
        return y.view(x.shape)

    @staticmethod
    @_once_differentiable
    def backward(ctx, dy):
        x2, gate_w, gate_b, u, h, route, *ws = ctx.saved_tensors
        n_exp, odt, prec, xshape, xdt, has_res = ctx.meta
        w1s, w2s = ws[:n_exp], ws[n_exp:]
        D = x2.shape[1]
        dyc = _grad_in(dy, odt, (-1, D))
        a = _moe_args(x2, gate_w.detach(), None if gate_b is None else gate_b.detach(), w1s, w2s, odt, prec)
        dx = torch.empty(x2.shape, dtype=xdt, device=x2.device)
        dw1 = [torch.empty_like(w) for w in w1s]
        dw2 = [torch.empty_like(w) for w in w2s]
        a.u, a.h, a.route, a.dy, a.dx = u.data_ptr(), h.data_ptr(), route.data_ptr(), dyc.data_ptr(), dx.data_ptr()
        for e in range(n_exp):
            a.dw1[e], a.dw2[e] = dw1[e].data_ptr(), dw2[e].data_ptr()
        ws_buf = _bytes(L.lib().mopk_moe_workspace_bytes(C.byref(a), 1), x2.device)
        a.workspace = ws_buf.data_ptr()
        LAST_PATH["moe_bwd"] = L.PATH_FUSED
        _launch("mopk_moe_bwd", a, "moe_bwd")
        dres = dy if has_res else None
        return (dx.view(xshape), dres, None, None, None, *dw1, *dw2)


def moe_mlp(x: torch.Tensor, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor], w1s, w2s,
            residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Top-1 MoE MLP ``[residual +] W2_e gelu_tanh(W1_e x)`` with ``e = argmax(gate(x))`` per token, the routed expert only (HIP:
    route, grouped fc1 / fc2 GEMMs forward, four grouped GEMMs and a chunk-ordered sum backward; no host sync).  x (..., D);
    gate_w (E, D), gate_b (E,) or None; w1s: E weights (F, D); w2s: E weights (D, F).  gate_w / gate_b get no gradient, as in the
    reference (its one-hot is a constant).  Calls the kernels do not take (moe_supported: fp16, D or F not a multiple of 8, more
    than 64 experts) run the reference's dense composition in torch; LAST_PATH["moe_fwd"] records which (PATH_FUSED / PATH_GENERIC)."""
    _require_gpu(x, "moe_mlp")
    w1s, w2s = list(w1s), list(w2s)
    if not moe_supported(x, gate_w, gate_b, w1s, w2s):
        LAST_PATH["moe_fwd"] = LAST_PATH["moe_bwd"] = L.PATH_GENERIC
        return moe_mlp_torch(x, gate_w, gate_b, w1s, w2s, residual)
    odt, _ = _moe_dtypes(x, w1s[0])
    fold = residual is not None and residual.dtype == odt and residual.shape == x.shape
    y = _MoeFn.apply(x, residual if fold else None, gate_w, gate_b, len(w1s), *w1s, *w2s)
    if residual is not None and not fold:
        y = residual + y
    return y


def moe_route(x: torch.Tensor, gate_w: torch.Tensor, gate_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 expert index per token (x (..., D) -> (M,)): the kernels' fp32-logit argmax (mopk_moe_route), or the same formula in
    fp32 torch for calls the kernels do not take"""
    _require_gpu(x, "moe_route")
    D, E = x.shape[-1], gate_w.shape[0]
    x2 = x.detach().reshape(-1, D).contiguous()
    ok = (2 <= E <= L.MOE_MAX_EXPERTS and x2.shape[0] > 0 and D % 8 == 0 and x2.dtype in (torch.float32, torch.bfloat16)
          and gate_w.dtype in (torch.float32, torch.bfloat16) and (gate_b is None or gate_b.dtype == gate_w.dtype))
    if not ok:
        return F.linear(x2.float(), gate_w.float(), None if gate_b is None else gate_b.float()).argmax(-1).to(torch.int32)
    gw = gate_w.detach().contiguous()
    gb = None if gate_b is None else gate_b.detach().contiguous()
    a = L.MoeArgs()
    a.M, a.D, a.F, a.E, a.precision = x2.shape[0], D, 8, E, L.PREC_BF16
    a.x_dtype = a.w_dtype = a.o_dtype = _io_dtype(x2)
    a.gate_dtype = _io_dtype(gw)
    route = _moe_route_buf(a.M, E, x.device)
    a.x, a.gate_w, a.gate_b, a.route = x2.data_ptr(), gw.data_ptr(), _ptr(gb), route.data_ptr()
    _launch("mopk_moe_route", a)
    return route[:a.M]


# ---- attention of a few new queries against a key / value cache (mopk_decode_attn_*; WhisperMoP incremental decoding) ----
# Four public ops share one validator (_da_check), one torch composition (_da_torch), one acceptance test (_da_accept) and one
# launch tail (_da_run).  An op is its public name; kw below is whichever of kv_len, nk, rows, kv_start, kv_lens it takes.
DECODE_MAX_TQ = 16
_NA = object()                  # _da_check: "the op has no such argument" (None is a value a caller can pass)
_DA_OPS = {                     # op -> (args class, export stem, LAST_PATH key)
    "decode_attention": (L.DecodeAttnArgs, "mopk_decode_attn", "decode_attn"),
    "decode_attention_rows": (L.DecodeAttnRowsArgs, "mopk_decode_attn_rows", "decode_attn_rows"),
    "decode_attention_ragged": (L.DecodeAttnRaggedArgs, "mopk_decode_attn_ragged", "decode_attn_ragged"),
    "decode_attention_lens": (L.DecodeAttnLensArgs, "mopk_decode_attn_lens", "decode_attn_lens"),
}


def _not_row_ints(t: torch.Tensor, B: int) -> bool:
    return t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point or t.dtype == torch.bool


def _da_check(op: str, q, k_cache, v_cache, kv_len=None, nk=None, rows=_NA, kv_start=_NA, kv_lens=_NA, rows_optional=False) -> None:
    """the four ops' argument checks, in one order: shapes, kv_start, kv_lens, rows, kv_len against nk, nk, kv_len.  _NA: the op has
    no such argument; rows_optional: rows may be None (the ragged op)"""
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError(f"{op}: q must be (B, Tq, H, dk) and k_cache, v_cache (B, cap, H, dk) of one shape; got q "
                         f"{tuple(q.shape)}, k {tuple(k_cache.shape)}, v {tuple(v_cache.shape)}")
    if k_cache.shape[0] != q.shape[0] or k_cache.shape[2:] != q.shape[2:]:
        raise ValueError(f"{op}: k_cache / v_cache {tuple(k_cache.shape)} do not match q's B, H, dk {tuple(q.shape)}")
    B, cap = q.shape[0], k_cache.shape[1]
    if kv_start is not _NA and _not_row_ints(kv_start, B):
        raise ValueError(f"{op}: kv_start must be an integer (B,) = ({B},) tensor, got {tuple(kv_start.shape)} {kv_start.dtype}")
    if kv_lens is not _NA and (not isinstance(kv_lens, torch.Tensor) or _not_row_ints(kv_lens, B)):
        raise ValueError(f"{op}: kv_lens must be an integer (B,) = ({B},) tensor, got "
                         f"{(tuple(kv_lens.shape), kv_lens.dtype) if isinstance(kv_lens, torch.Tensor) else type(kv_lens).__name__}")
    if rows is None and rows_optional:
        rows = _NA
    if rows is not _NA and (rows.dim() != 2 or rows.shape[0] != B or rows.shape[1] < cap):
        raise ValueError(f"{op}: rows must be (B, >= cap) = ({B}, >= {cap}), got {tuple(rows.shape)}")
    if kv_len is not None and nk is not None:
        raise ValueError(f"{op}: pass kv_len (device) or nk (host), not both")
    if nk is not None and not 0 < int(nk) <= cap:
        raise ValueError(f"{op}: nk = {nk} outside [1, cap = {cap}]")
    if kv_len is not None and kv_len.numel() != 1:
        raise ValueError(f"{op}: kv_len must hold one element, got shape {tuple(kv_len.shape)}")


def _da_torch(q, k_cache, v_cache, kv_len=None, nk=None, causal=False, rows=None, kv_start=None, kv_lens=None) -> torch.Tensor:
    """the reference composition of the four ops in torch ops (fp32 arithmetic, float64 for float64 tensors).  Row b's key j comes
    from cache row rows[b, j] (clamped into [0, B)); it is open if kv_start[b] <= j < min(L, kv_lens[b]), with L = kv_len (device),
    else nk, else cap.  Every length stays on the device (masks over the whole cache), so there is no host sync either."""
    B, Tq, H, dk = q.shape
    cap = k_cache.shape[1]
    if rows is not None:
        r = rows[:, :cap].to(torch.long).clamp(0, B - 1)
        j = torch.arange(cap, device=k_cache.device).unsqueeze(0)
        k_cache, v_cache = k_cache[r, j], v_cache[r, j]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    s = torch.einsum("bihd,bjhd->bhij", q.to(ct), k_cache.to(ct)) * dk ** -0.5
    j = torch.arange(cap, device=q.device)
    L = kv_len.reshape(()).to(torch.long).clamp(0, cap) if kv_len is not None else (cap if nk is None else int(nk))
    i = torch.arange(Tq, device=q.device)
    lim = L - Tq + i + 1 if causal else L + 0 * i                           # (Tq,): host ints never become device copies
    open_ = (j < L).unsqueeze(0)                                            # (1 or B, cap): the keys a row may see at all
    if kv_start is not None:
        open_ = open_ & (j >= kv_start.reshape(B, 1).to(torch.long))
    if kv_lens is not None:
        open_ = open_ & (j < kv_lens.reshape(B, 1).to(torch.long).clamp_min(0))     # j < L is in open_ already
    ok = open_.unsqueeze(1) & (j.unsqueeze(0) < lim.unsqueeze(1)).unsqueeze(0)  # (1 or B, Tq, cap)
    s = s.masked_fill(~ok.unsqueeze(1), float("-inf"))
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)                            # a query that sees no key gets y = 0, as the kernels
    v = v_cache.to(ct).masked_fill(~open_.view(-1, cap, 1, 1), 0.0)         # rows that are not open may hold anything
    y = torch.einsum("bhij,bjhd->bihd", p, v)
    return y.to(q.dtype).reshape(B, Tq, H * dk)


def _da_args(op: str, q, k_cache, v_cache, kv_len=None, nk=None, causal=False, rows=None, kv_start=None, kv_lens=None):
    """the op's args struct, without y and the workspace"""
    B, Tq, H, dk = q.shape
    base = L.DecodeAttnArgs()
    base.B, base.H, base.Tq, base.dk, base.cap = B, H, Tq, dk, k_cache.shape[1]
    base.Nk = base.cap if (nk is None and kv_len is None) else (0 if nk is None else int(nk))
    base.io_dtype, base.causal = _io_dtype(q), int(bool(causal))
    base.q, base.k, base.v = _v4(q), _v4(k_cache), _v4(v_cache)
    base.kv_len = _ptr(kv_len)
    if op == "decode_attention":
        return base
    a = _DA_OPS[op][0]()
    a.base = base                                                           # a copy: from here on the fields are a.base's
    if rows is not None:
        a.rows, a.rows_ld = rows.data_ptr(), rows.stride(0)
    if kv_start is not None:
        a.kv_start = kv_start.data_ptr()
    if kv_lens is not None:
        a.kv_lens = kv_lens.data_ptr()
    return a


def _row_i32_ok(t: torch.Tensor, B: int) -> bool:
    """a per-row vector the kernels read: int32, CUDA, contiguous, B elements"""
    return t.is_cuda and t.dtype == torch.int32 and t.numel() == B and t.is_contiguous()


def _da_accept(op: str, q, k_cache, v_cache, kv_len=None, nk=None, causal=False, rows=None, kv_start=None, kv_lens=None):
    """the args struct of a call that the op's kernels take, None of one they refuse.  The tensor side is tested here; the library's
    query for the op decides the rest (each variant's query runs the plain op's check on its base first, so that is not asked twice)"""
    if kv_start is not None and not _row_i32_ok(kv_start, q.shape[0]):
        return None
    if kv_lens is not None and not _row_i32_ok(kv_lens, q.shape[0]):
        return None
    if rows is not None and (not rows.is_cuda or rows.dtype != torch.int32 or rows.dim() != 2 or rows.stride(1) != 1):
        return None
    ts = (q, k_cache, v_cache)
    if any(not t.is_cuda or t.dtype != q.dtype or t.dtype not in (torch.float32, torch.bfloat16) or t.stride(-1) != 1 for t in ts):
        return None
    if kv_len is not None and (not kv_len.is_cuda or kv_len.dtype != torch.int32 or kv_len.numel() != 1):
        return None
    if q.numel() == 0 or k_cache.shape[1] == 0:
        return None
    a = _da_args(op, q, k_cache, v_cache, kv_len, nk, causal, rows, kv_start, kv_lens)
    return a if getattr(L.lib(), _DA_OPS[op][1] + "_supported")(C.byref(a)) else None


def _da_run(op: str, q, k_cache, v_cache, causal=False, rows_optional=False, **kw) -> torch.Tensor:
    """a public op's body: validate, then the HIP kernels on the args struct _da_accept built (the one struct serves the library's
    _supported query, its workspace query and the launch), or _da_torch for a call the kernels refuse"""
    _da_check(op, q, k_cache, v_cache, rows_optional=rows_optional, **kw)
    _require_gpu(q, op)
    _, stem, key = _DA_OPS[op]
    with torch.no_grad():
        a = _da_accept(op, q, k_cache, v_cache, causal=causal, **kw)
        if a is None:
            LAST_PATH[key] = L.PATH_GENERIC
            return _da_torch(q, k_cache, v_cache, causal=causal, **kw)
        B, Tq, H, dk = q.shape
        y = torch.empty(B, Tq, H, dk, dtype=q.dtype, device=q.device)
        ws = _bytes(getattr(L.lib(), stem + "_workspace_bytes")(C.byref(a)), q.device)
        base = a if op == "decode_attention" else a.base
        base.y, base.workspace = _v4(y), ws.data_ptr()
        LAST_PATH[key] = L.PATH_FUSED
        _launch(stem + "_fwd", a, key)
        return y.view(B, Tq, H * dk)


def decode_attention_torch(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_len: Optional[torch.Tensor] = None,
                           nk: Optional[int] = None, causal: bool = False) -> torch.Tensor:
    """the reference composition of `decode_attention` in torch ops (fp32 arithmetic, float64 for float64 tensors); the valid length
    stays on the device (a mask over the whole cache), so there is no host sync either"""
    return _da_torch(q, k_cache, v_cache, kv_len, nk, causal)


def decode_attention_supported(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_len: Optional[torch.Tensor] = None,
                               nk: Optional[int] = None, causal: bool = False) -> bool:
    """True if mopk_decode_attn_* take this call: GPU tensors of one dtype (fp32 / bf16), 1 <= Tq <= 16, dk in {32, 64, 128}, unit
    inner strides, 16-byte aligned cache views, an int32 kv_len (the library's own query decides the rest)"""
    return _da_accept("decode_attention", q, k_cache, v_cache, kv_len, nk, causal) is not None


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_len: Optional[torch.Tensor] = None,
                     nk: Optional[int] = None, causal: bool = False) -> torch.Tensor:
    """softmax(q k^T / sqrt(dk) [causal]) v of Tq new queries against the first L keys of a cache; inference only (no autograd).

    q: (B, Tq, H, dk); k_cache, v_cache: (B, cap, H, dk) views (a buffer larger than its fill is passed without a copy).
    L = kv_len, a one-element int32 DEVICE tensor read by the kernels (set it to the length after this step's append: the call's
    arguments then do not change from step to step and can be captured in a graph), else nk (host int), else cap.  causal is
    bottom-right aligned: query i sees keys j < L - Tq + i + 1.  Returns (B, Tq, H * dk) in q's dtype.  Runs the split-KV HIP kernel
    pair when decode_attention_supported() accepts the call, else decode_attention_torch(); LAST_PATH["decode_attn"] records which
    (PATH_FUSED / PATH_GENERIC).  No host synchronisation."""
    return _da_run("decode_attention", q, k_cache, v_cache, causal, kv_len=kv_len, nk=nk)


# ---- decode attention through a source-row table (mopk_decode_attn_rows_*; WhisperMoP beam search) ----
def decode_attention_rows_torch(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, rows: torch.Tensor,
                                kv_len: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """the reference composition of `decode_attention_rows`: gather key / value j of row b from cache row rows[b, j] (clamped into
    [0, B)), then decode_attention_torch"""
    return _da_torch(q, k_cache, v_cache, kv_len, None, causal, rows=rows)


def decode_attention_rows_supported(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, rows: torch.Tensor,
                                    kv_len: Optional[torch.Tensor] = None, causal: bool = False) -> bool:
    """True if mopk_decode_attn_rows_* take this call: what decode_attention_supported asks, and a CUDA int32 (B, >= cap) table with
    unit inner stride"""
    return _da_accept("decode_attention_rows", q, k_cache, v_cache, kv_len, None, causal, rows=rows) is not None


def decode_attention_rows(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, rows: torch.Tensor,
                          kv_len: Optional[torch.Tensor] = None, causal: bool = False) -> torch.Tensor:
    """`decode_attention` whose key / value j of query row b is read from cache row rows[b, j] at position j: a beam's history lives
    in the rows its ancestors wrote, and no cache slot is copied when beams are reordered.  Inference only (no autograd).

    q: (B, Tq, H, dk); k_cache, v_cache: (B, cap, H, dk); rows: int32 (B, >= cap) device table (entries outside [0, B) are clamped);
    kv_len as in decode_attention (else L = cap).  With rows[b, j] = b the result is bitwise that of decode_attention.  Returns
    (B, Tq, H * dk) in q's dtype.  Runs the row-indirect split-KV HIP kernels when decode_attention_rows_supported() accepts the call,
    else decode_attention_rows_torch(); LAST_PATH["decode_attn_rows"] records which.  No host synchronisation."""
    return _da_run("decode_attention_rows", q, k_cache, v_cache, causal, rows=rows, kv_len=kv_len)


# ---- decode attention with a per-row first key (mopk_decode_attn_ragged_*; WhisperMoP decoding of left-padded prompts) ----
def decode_attention_ragged_torch(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_start: torch.Tensor,
                                  rows: Optional[torch.Tensor] = None, kv_len: Optional[torch.Tensor] = None, nk: Optional[int] = None,
                                  causal: bool = False) -> torch.Tensor:
    """the reference composition of `decode_attention_ragged`: decode_attention_torch (after the row gather of
    decode_attention_rows_torch when rows is given) with the keys j < kv_start[b] of row b masked out; no host sync"""
    return _da_torch(q, k_cache, v_cache, kv_len, nk, causal, rows=rows, kv_start=kv_start)


def decode_attention_ragged_supported(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_start: torch.Tensor,
                                      rows: Optional[torch.Tensor] = None, kv_len: Optional[torch.Tensor] = None,
                                      nk: Optional[int] = None, causal: bool = False) -> bool:
    """True if mopk_decode_attn_ragged_* take this call: what decode_attention_supported asks, a contiguous CUDA int32 kv_start of
    B elements, and (with rows) what decode_attention_rows_supported asks of the table"""
    return _da_accept("decode_attention_ragged", q, k_cache, v_cache, kv_len, nk, causal, rows=rows, kv_start=kv_start) is not None


def decode_attention_ragged(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_start: torch.Tensor,
                            rows: Optional[torch.Tensor] = None, kv_len: Optional[torch.Tensor] = None, nk: Optional[int] = None,
                            causal: bool = False) -> torch.Tensor:
    """`decode_attention` (rows None) or `decode_attention_rows` (rows given) in which query row b sees only the keys
    j >= kv_start[b]: prompts of different lengths left-padded in one cache, row b's prompt in columns [kv_start[b], P).
    Inference only (no autograd).

    kv_start: int32 (B,) device tensor (values are clamped into [0, L]); q, k_cache, v_cache, rows, kv_len, nk and causal as in
    decode_attention / decode_attention_rows.  Query i of row b sees kv_start[b] <= j < L (causal: < L - Tq + i + 1); a query that
    sees no key gets y = 0.  With kv_start = 0 the result is bitwise that of decode_attention / decode_attention_rows.  Returns
    (B, Tq, H * dk) in q's dtype.  Runs the split-KV HIP kernels when decode_attention_ragged_supported() accepts the call, else
    decode_attention_ragged_torch(); LAST_PATH["decode_attn_ragged"] records which.  No host synchronisation."""
    return _da_run("decode_attention_ragged", q, k_cache, v_cache, causal, True, kv_start=kv_start, rows=rows, kv_len=kv_len, nk=nk)


# ---- decode attention with a per-row key count (mopk_decode_attn_lens_*; WhisperMoP cross-attention over ragged audio) ----
def decode_attention_lens_torch(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_lens: torch.Tensor,
                                nk: Optional[int] = None) -> torch.Tensor:
    """the reference composition of `decode_attention_lens`: non-causal decode_attention_torch with the keys j >= kv_lens[b] of row b
    masked out; no host sync"""
    return _da_torch(q, k_cache, v_cache, None, nk, False, kv_lens=kv_lens)


def decode_attention_lens_supported(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_lens: torch.Tensor,
                                    nk: Optional[int] = None) -> bool:
    """True if mopk_decode_attn_lens_* take this call: what decode_attention_supported asks, and a contiguous CUDA int32 kv_lens of
    B elements"""
    return _da_accept("decode_attention_lens", q, k_cache, v_cache, None, nk, False, kv_lens=kv_lens) is not None


def decode_attention_lens(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_lens: torch.Tensor,
                          nk: Optional[int] = None) -> torch.Tensor:
    """non-causal `decode_attention` in which row b of q sees only the keys j < kv_lens[b]: the cross-attention of a decode step over
    audio of different lengths right-padded in one cache.  Inference only (no autograd).

    q: (B, Tq, H, dk); k_cache, v_cache: (B, cap, H, dk) views; kv_lens: int32 (B,) device tensor, clamped into [0, nk] (nk: host
    int, else cap).  A row is a row of q: beams or samples of one item that share its cache go in as one row of beams * T queries,
    with one length.  Key rows >= kv_lens[b] are never read; a row with kv_lens[b] = 0 gets y = 0; kv_lens = nk everywhere is
    bitwise decode_attention(q, k_cache, v_cache, nk=nk).  Returns (B, Tq, H * dk) in q's dtype.  Runs the split-KV HIP kernels when
    decode_attention_lens_supported() accepts the call, else decode_attention_lens_torch(); LAST_PATH["decode_attn_lens"] records
    which.  No host synchronisation."""
    return _da_run("decode_attention_lens", q, k_cache, v_cache, kv_lens=kv_lens, nk=nk)


# ---- the ops after the decoder's logits: beam_step, sample_tokens[_ragged], logit_rules, repeat_rules, token_logprob, language_probs, greedy_pick,
# alignment_cost, dtw_align, timestamp_segments, prompt_history_update, window_prompts, alignment_rows, word_spans ----
# Each is its _*_check (every ValueError, once per call), its _*_accept (the tensor-side tests, then the args struct, built once,
# if the library's _supported query takes it, else None), then the torch restatement, or the outputs into that struct and _row_launch.
def _row_launch(a, sym: str, key: str, dev=None, ws_sym: Optional[str] = None) -> None:
    """the tail these ops share: the library's workspace query `ws_sym` where the op has one (the buffer goes into the struct,
    into its base for a struct that wraps one), LAST_PATH, and the launch of `sym` on the accepted struct `a`"""
    if ws_sym is not None:
        n = getattr(L.lib(), ws_sym)(C.byref(a))
        ws = _bytes(n, dev) if n else None
        getattr(a, "base", a).workspace = _ptr(ws)
    LAST_PATH[key] = L.PATH_FUSED
    _launch(sym, a, key)


# ---- batched beam search on device state (mopk_beam_*; WhisperMoP.beam_search) ----
BEAM_MAX_K = 8


class BeamState:
    """Device state of a beam search over B items with K beams each, updated in place by `beam_step` (no host sync, static
    buffers: a step can be captured in a graph).  Rows b * K + k hold item b's beam k.

    scores (B*K,) fp32: live beam log-probabilities, [0, -inf, ...] per item at the start (the prompt is one hypothesis);
    next_ids (B*K, 1) int32: the live beams' newest tokens (the next decoder step's ids); parents (B*K,) int32: the beam each live
    beam extended at the last step; hist (B*K, cap) int32: token histories, the prompt in columns [0, T_p); rows (B*K, cap) int32:
    the cache row holding each history position's keys / values (the prompt's in row b * K, every later one in the row that wrote
    it; entries past a beam's length point at the beam's own row); fin_tokens (B, K, cap) int32, fin_scores (B, K) fp32,
    fin_count (B,) int32: finished hypotheses (eos-filled past their eos, scores length-normalised); done (B,) int32."""

    def __init__(self, prompt_ids: torch.Tensor, num_beams: int, cap: int, eos_token_id: Optional[int] = None,
                 length_penalty: float = 1.0):
        B, T_p = prompt_ids.shape
        K, dev = int(num_beams), prompt_ids.device
        self.B, self.K, self.T, self.prompt_len = B, K, int(cap), T_p
        self.eos, self.length_penalty = eos_token_id, float(length_penalty)
        i32 = dict(dtype=torch.int32, device=dev)
        self.scores = torch.zeros(B, K, dtype=torch.float32, device=dev)
        self.scores[:, 1:] = float("-inf")
        self.scores = self.scores.view(B * K)
        self.next_ids = torch.zeros(B * K, 1, **i32)
        self.parents = torch.zeros(B * K, **i32)
        self.hist = torch.zeros(B * K, self.T, **i32)
        self.hist[:, :T_p] = prompt_ids.to(torch.int32).repeat_interleave(K, 0)
        r = torch.arange(B * K, **i32)
        self.rows = r.unsqueeze(1).repeat(1, self.T)
        self.rows[:, :T_p] = (r // K * K).unsqueeze(1)
        self.fin_tokens = torch.full((B, K, self.T), 0 if eos_token_id is None else int(eos_token_id), **i32)
        self.fin_scores = torch.full((B, K), float("-inf"), dtype=torch.float32, device=dev)
        self.fin_count = torch.zeros(B, **i32)
        self.done = torch.zeros(B, **i32)


def _beam_logits_strides(logits: torch.Tensor, st: BeamState):
    """(item stride, beam stride) of (B*K, V) logits, or of (B, V) logits shared by each item's beams (beam stride 0)"""
    if logits.shape[0] == st.B * st.K:
        return st.K * logits.stride(0), logits.stride(0)
    return logits.stride(0), 0


def _beam_args(logits: torch.Tensor, st: BeamState, pos: torch.Tensor) -> L.BeamArgs:
    a = L.BeamArgs()
    a.B, a.K, a.V, a.T = st.B, st.K, logits.shape[-1], st.T
    a.logits_dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.eos = -1 if st.eos is None else int(st.eos)
    a.prompt_len, a.length_penalty = st.prompt_len, st.length_penalty
    a.logits, (a.logits_sb, a.logits_sk), a.pos = logits.data_ptr(), _beam_logits_strides(logits, st), pos.data_ptr()
    a.scores, a.next_ids, a.parents = st.scores.data_ptr(), st.next_ids.data_ptr(), st.parents.data_ptr()
    a.hist, a.hist_ld, a.rows, a.rows_ld = st.hist.data_ptr(), st.hist.stride(0), st.rows.data_ptr(), st.rows.stride(0)
    a.fin_tokens, a.fin_scores = st.fin_tokens.data_ptr(), st.fin_scores.data_ptr()
    a.fin_count, a.done = st.fin_count.data_ptr(), st.done.data_ptr()
    return a


def _beam_accept(logits: torch.Tensor, state: BeamState, pos: torch.Tensor):
    """the args struct (without the workspace) of a call that mopk_beam_* take, None of one they refuse"""
    if not logits.is_cuda or logits.dtype not in (torch.float32, torch.bfloat16) or logits.stride(-1) != 1:
        return None
    if not pos.is_cuda or pos.dtype != torch.int32 or pos.numel() != 1:
        return None
    a = _beam_args(logits, state, pos)
    return a if L.lib().mopk_beam_supported(C.byref(a)) else None


def beam_step_supported(logits: torch.Tensor, state: BeamState, pos: torch.Tensor) -> bool:
    """True if mopk_beam_* take this call: CUDA fp32 / bf16 logits with unit inner stride, 1 <= K <= 8, V >= 2, an int32 device pos
    (the library's own query decides the rest)"""
    return _beam_accept(logits, state, pos) is not None


def _beam_check(logits: torch.Tensor, state: BeamState, pos: torch.Tensor, what: str):
    if logits.dim() != 2 or logits.shape[0] not in (state.B, state.B * state.K):
        raise ValueError(f"{what}: logits must be (B*K, V) = ({state.B * state.K}, V) or (B, V) = ({state.B}, V), "
                         f"got {tuple(logits.shape)}")
    if not 1 <= state.K <= BEAM_MAX_K or logits.shape[1] < 2:
        raise ValueError(f"{what}: needs 1 <= K <= {BEAM_MAX_K} and V >= 2 (K = {state.K}, V = {logits.shape[1]})")
    if pos.numel() != 1:
        raise ValueError(f"{what}: pos must hold one element, got shape {tuple(pos.shape)}")


def beam_step_torch(logits: torch.Tensor, state: BeamState, pos: torch.Tensor) -> None:
    """the reference composition of `beam_step` in torch ops (CPU or GPU, no host sync): the same candidates, order, walk and
    in-place updates, vectorised over items with a loop over the 2K candidate ranks"""
    _beam_check(logits, state, pos, "beam_step_torch")
    B, K, T = state.B, state.K, state.T
    V, NC, dev = logits.shape[1], 2 * K, logits.device
    x = logits.float()
    if x.shape[0] != B * K:
        x = x.repeat_interleave(K, 0)
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    top, idx = torch.sort(x, dim=-1, descending=True, stable=True)                 # a beam's 2K best, ties to the smaller v
    n = min(NC, V)
    top, idx = top[:, :n], idx[:, :n]
    s0 = state.scores.view(B * K, 1)
    inf = torch.tensor(float("-inf"), device=dev)
    sc = torch.where((top == float("-inf")) | (s0 == float("-inf")), inf, s0 + (top - lse))
    flat = (torch.arange(B * K, device=dev) % K).unsqueeze(1) * V + idx
    sc, flat = sc.view(B, K * n), flat.view(B, K * n)
    o = torch.argsort(flat, dim=1, stable=True)                                     # ties to the smaller flat index ...
    sc, flat = sc.gather(1, o), flat.gather(1, o)
    o = torch.argsort(sc, dim=1, descending=True, stable=True)                      # ... under score descending
    cs, cf = sc.gather(1, o)[:, :NC], flat.gather(1, o)[:, :NC]
    ck, cv = cf // V, cf % V

    p = pos.reshape(()).to(torch.long)
    upd = (state.done == 0) & (p >= state.prompt_len) & (p < T)
    norm = (p - state.prompt_len + 1).to(torch.float32).pow(state.length_penalty)
    eos = -1 if state.eos is None else int(state.eos)
    hist, rows = state.hist.view(B, K, T), state.rows.view(B, K, T)
    j = torch.arange(T, device=dev)
    before, at = j < p, j == p
    nl = torch.zeros(B, dtype=torch.long, device=dev)
    nf = state.fin_count.to(torch.long)
    new_s = state.scores.view(B, K).clone()
    par, tok = torch.zeros(B, K, dtype=torch.long, device=dev), torch.zeros(B, K, dtype=torch.long, device=dev)
    fin_s, fin_t = state.fin_scores.clone(), state.fin_tokens.clone()

    def put(t, i, val, m):                                                          # t[b, i[b]] = val[b] where m[b]
        i = i.unsqueeze(1)
        t.scatter_(1, i, torch.where(m, val.to(t.dtype), t.gather(1, i).squeeze(1)).unsqueeze(1))

    for c in range(NC):
        s, k, v = cs[:, c], ck[:, c], cv[:, c]
        active = nl < K
        is_fin = (v == eos) & torch.isfinite(s)
        store = active & is_fin & (nf < K)
        slot = nf.clamp(max=K - 1)
        put(fin_s, slot, s / norm, store)
        src = hist.gather(1, k.view(B, 1, 1).expand(B, 1, T))                        # the parent's history, before this step
        row = torch.where(before, src, torch.where(at, torch.full_like(src, max(eos, 0)), fin_t.gather(
            1, slot.view(B, 1, 1).expand(B, 1, T))))
        fin_t.scatter_(1, slot.view(B, 1, 1).expand(B, 1, T),
                       torch.where(store.view(B, 1, 1), row, fin_t.gather(1, slot.view(B, 1, 1).expand(B, 1, T))))
        nf = nf + store.to(torch.long)
        live = active & ~is_fin
        li = nl.clamp(max=K - 1)
        put(new_s, li, s, live)
        put(par, li, k, live)
        put(tok, li, v, live)
        nl = nl + live.to(torch.long)

    g = par.unsqueeze(2).expand(B, K, T)
    own = (torch.arange(B * K, device=dev, dtype=torch.int32).view(B, K, 1)).expand(B, K, T)
    new_hist = torch.where(before, hist.gather(1, g), torch.where(at, tok.to(torch.int32).unsqueeze(2).expand(B, K, T), hist))
    new_rows = torch.where(before, rows.gather(1, g), torch.where(at, own, rows))
    u1, u2, u3 = upd.view(B, 1), upd.view(B, 1, 1), upd
    state.hist.copy_(torch.where(u2, new_hist, hist).view(B * K, T))
    state.rows.copy_(torch.where(u2, new_rows, rows).view(B * K, T))
    state.scores.copy_(torch.where(u1, new_s, state.scores.view(B, K)).view(B * K))
    state.parents.copy_(torch.where(u1, par.to(torch.int32), state.parents.view(B, K)).view(B * K))
    state.next_ids.copy_(torch.where(u1, tok.to(torch.int32), state.next_ids.view(B, K)).view(B * K, 1))
    state.fin_scores.copy_(torch.where(u1, fin_s, state.fin_scores))
    state.fin_tokens.copy_(torch.where(u2, fin_t, state.fin_tokens))
    state.fin_count.copy_(torch.where(u3, nf.to(torch.int32), state.fin_count))
    state.done.copy_(torch.where(u3, (nf >= K).to(torch.int32), state.done))


def beam_step(logits: torch.Tensor, state: BeamState, pos: torch.Tensor) -> None:
    """one beam-search step: update `state` in place from the step's last-position logits.  Inference only.

    logits: (B*K, V), or (B, V) shared by each item's beams (the prompt's, at the first step); fp32 or bf16.  pos: (1,) int32 device
    tensor, the history column of the new tokens (the decoder cache's length after the step).  Per item not yet done:
    - candidates (k, v) score scores[k] + log_softmax(logits[k])[v] in fp32; the top 2K in descending score, ties to the smaller
      k * V + v (each beam contributes its 2K largest logits, ties to the smaller v);
    - walk them in order: eos_token_id with a finite score -> a finished hypothesis while the item has fewer than K, stored with
      score / (pos - T_p + 1) ** length_penalty (the generated length, eos counted) and its history + eos; never a live beam.  Any
      other candidate -> the next live beam.  Stop once K live beams are filled;
    - reorder hist / rows in place by parent, write the new tokens at column pos and rows[b*K + k, pos] = b*K + k (the slot the next
      decoder step appends), and mark the item done once it holds K finished hypotheses.
    pos outside [T_p, cap) changes nothing.  Runs the two-launch HIP kernel pair (mopk_beam_step) when beam_step_supported() accepts
    the call, else beam_step_torch(); LAST_PATH["beam_step"] records which.  No host synchronisation."""
    _beam_check(logits, state, pos, "beam_step")
    _require_gpu(logits, "beam_step")
    with torch.no_grad():
        a = _beam_accept(logits, state, pos)
        if a is None:
            LAST_PATH["beam_step"] = L.PATH_GENERIC
            return beam_step_torch(logits, state, pos)
        _row_launch(a, "mopk_beam_step", "beam_step", logits.device, "mopk_beam_workspace_bytes")


def beam_finalize(state: BeamState, n_new: int):
    """the search's answer after n_new steps -> (tokens (B, cap) int32, scores (B,) fp32), on the device without a sync.  An item
    that is not done adds its live beams in beam order (score / n_new ** length_penalty) until it holds K hypotheses; the answer is
    the best normalised score, ties to the earlier stored hypothesis; columns past its eos hold eos."""
    B, K, T = state.B, state.K, state.T
    dev = state.scores.device
    cnt = state.fin_count.to(torch.long).unsqueeze(1)
    j = torch.arange(K, device=dev).unsqueeze(0)
    src = (j - cnt).clamp(0, K - 1)
    fill = (j >= cnt) & (state.done == 0).unsqueeze(1)
    live = state.scores.view(B, K) / float(n_new) ** state.length_penalty
    s = torch.where(fill, live.gather(1, src), state.fin_scores)
    t = torch.where(fill.unsqueeze(2), state.hist.view(B, K, T).gather(1, src.unsqueeze(2).expand(B, K, T)), state.fin_tokens)
    best = s.argmax(dim=1, keepdim=True)
    return t.gather(1, best.unsqueeze(2).expand(B, 1, T)).squeeze(1), s.gather(1, best).squeeze(1)


# ---- temperature / top-k / top-p sampling of one token per row (mopk_sample_*; WhisperMoP.sample) ----
_M32 = 0xFFFFFFFF


def _f32(x: float) -> float:
    """x rounded to fp32 (what the C ABI's float fields carry)"""
    return C.c_float(x).value


def _mul32(a: torch.Tensor, c: int) -> torch.Tensor:
    """(a * c) mod 2^32 for int64 a in [0, 2^32) and a constant c < 2^32, in two 16-bit halves so no product leaves int64"""
    return (a * (c & 0xFFFF) + (((a * (c >> 16)) & 0xFFFF) << 16)) & _M32


def _hash32(x: torch.Tensor) -> torch.Tensor:
    """common.h's fa_hash ("lowbias32") on int64 tensors holding uint32 values"""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def _sample_params(temperature, top_k, top_p, what: str):
    """validate the sampling parameters -> (inv_t (fp32 value, None for temperature 0), top_p (fp32 value))"""
    t = float(temperature)
    if not math.isfinite(t) or t < 0:
        raise ValueError(f"{what}: temperature must be finite and >= 0, got {temperature}")
    inv_t = None if t == 0 else _f32(1.0 / t)
    if inv_t is not None and not (0 < inv_t < math.inf):
        raise ValueError(f"{what}: 1 / temperature = {1.0 / t} is not a finite positive fp32 value")
    if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 0:
        raise ValueError(f"{what}: top_k must be an integer >= 0 (0: off), got {top_k}")
    p = float(top_p)
    if not 0 < p <= 1:
        raise ValueError(f"{what}: top_p must lie in (0, 1] (1: off), got {top_p}")
    return inv_t, _f32(p)


def _sample_check(logits: torch.Tensor, pos: torch.Tensor, temperature, top_k, top_p, out, what: str):
    """validate a sampling call before any device work -> (R, n, inv_t (fp32 value, None for temperature 0), top_p (fp32 value))"""
    inv_t, tp = _sample_params(temperature, top_k, top_p, what)
    if logits.dim() != 2 or logits.shape[1] < 2 or logits.shape[0] < 1:
        raise ValueError(f"{what}: logits must be (rows, V) with V >= 2, got {tuple(logits.shape)}")
    if tuple(pos.shape) != (1,):
        raise ValueError(f"{what}: pos must be a (1,) tensor, got shape {tuple(pos.shape)}")
    R = logits.shape[0]
    if out is not None:
        tok, lp = out
        R = tok.shape[0] if tok.dim() == 1 else -1
        if R < 1 or tuple(lp.shape) != (R,) or tok.dtype != torch.int32 or lp.dtype != torch.float32 or R % logits.shape[0]:
            raise ValueError(f"{what}: out must be (tokens int32 (R,), logprobs fp32 (R,)) with R a multiple of the "
                             f"{logits.shape[0]} logit rows, got {tuple(tok.shape)} {tok.dtype}, {tuple(lp.shape)} {lp.dtype}")
    return R, R // logits.shape[0], inv_t, tp


def sample_tokens_torch(logits: torch.Tensor, pos: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                        seed: int = 0, out=None):
    """the reference composition of `sample_tokens` in torch ops (CPU or GPU, no host sync): the same z, filters, fixed-point top-p
    masses, hash and Gumbel-max, in int64 / fp32 tensors"""
    R, n, inv_t, tp = _sample_check(logits, pos, temperature, top_k, top_p, out, "sample_tokens_torch")
    return _sample_torch(logits, pos, None, R, n, inv_t, tp, top_k, seed, out)


def _sample_torch(logits, pos, pos_off, R, n, inv_t, tp, top_k, seed, out):
    """sample_tokens_torch's body; pos_off (R,): row r draws at pos - pos_off[r]"""
    x = logits.float()
    if n > 1:
        x = x.repeat_interleave(n, 0)
    V, dev = x.shape[1], x.device
    if inv_t is None:
        tok = x.argmax(-1)
    else:
        z = x * torch.tensor(inv_t, dtype=torch.float32, device=dev)
        ninf = torch.tensor(float("-inf"), device=dev)
        keep = torch.ones_like(z, dtype=torch.bool)
        if 0 < top_k < V:
            keep = z >= z.topk(int(top_k), dim=-1).values[:, -1:]
        if tp < 1:
            mz = z.max(-1, keepdim=True).values
            live = keep & (mz != float("-inf"))                                   # a row of -inf only keeps everything
            q = torch.where(live, (torch.exp(z - mz) * 2.0 ** 40).nan_to_num(0.0).to(torch.int64), 0)
            P = torch.ceil(q.sum(-1, keepdim=True).double() * tp).to(torch.int64)
            zs, order = torch.sort(torch.where(keep, z, ninf), dim=-1, descending=True, stable=True)
            first = (q.gather(-1, order).cumsum(-1) >= P).to(torch.int8).argmax(-1, keepdim=True)
            tau = zs.gather(-1, first)                                            # the largest z whose upper mass reaches P
            keep = torch.where(live.any(-1, keepdim=True), keep & (z >= tau), keep)
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        r = torch.arange(R, device=dev, dtype=torch.int64).unsqueeze(1)
        p = pos.reshape(1, 1).to(torch.int64)
        if pos_off is not None:
            p = p - pos_off.reshape(R, 1).to(torch.int64)
        p = p & _M32
        rh = _hash32(_hash32((s & _M32) ^ _mul32(r, 0x9E3779B1)) ^ (s >> 32) ^ _mul32(p, 0x85EBCA77))
        h = _hash32(rh ^ _mul32(torch.arange(V, device=dev, dtype=torch.int64).unsqueeze(0), 0xC2B2AE3D))
        u = ((h >> 9).to(torch.float32) + 0.5) * 2.0 ** -23
        tok = torch.where(keep, z + -torch.log(-torch.log(u)), ninf).argmax(-1)
    lp = torch.log_softmax(x, -1).gather(1, tok.unsqueeze(1)).squeeze(1)
    if out is None:
        return tok.to(torch.int32), lp
    out[0].copy_(tok)
    out[1].copy_(lp)
    return out[0], out[1]


def _sample_args(logits: torch.Tensor, pos: torch.Tensor, R: int, n: int, inv_t, tp: float, top_k: int, seed: int) -> L.SampleArgs:
    a = L.SampleArgs()
    a.R, a.n, a.V = R, n, logits.shape[1]
    a.logits_dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.top_k = min(int(top_k), a.V)
    a.greedy, a.inv_temp, a.top_p = int(inv_t is None), 1.0 if inv_t is None else inv_t, tp
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.logits, a.logits_sb, a.logits_sk, a.pos = logits.data_ptr(), logits.stride(0), 0, pos.data_ptr()
    return a


def _sample_accept(logits, pos, chk, top_k, seed, out, pos_off=None):
    """the args struct of a call that mopk_sample_* (with pos_off: mopk_sample_ragged_*, whose query starts with the plain op's check
    on the same base, so that one is not asked as well) take, None of one they refuse.  chk: _sample_check's (R, n, inv_t, tp)."""
    if not logits.is_cuda or logits.dtype not in (torch.float32, torch.bfloat16) or logits.stride(-1) != 1:
        return None
    if not pos.is_cuda or pos.dtype != torch.int32:
        return None
    if out is not None and not all(t.is_cuda and t.is_contiguous() for t in out):
        return None
    a = _sample_args(logits, pos, *chk, top_k, seed)
    if pos_off is None:
        return a if L.lib().mopk_sample_supported(C.byref(a)) else None
    if not pos_off.is_cuda or pos_off.dtype != torch.int32 or not pos_off.is_contiguous():
        return None
    r = L.SampleRaggedArgs()
    r.base, r.pos_off = a, pos_off.data_ptr()                                      # a copy: from here on the fields are r.base's
    return r if L.lib().mopk_sample_ragged_supported(C.byref(r)) else None


def _sample_run(stem: str, key: str, logits, pos, pos_off, chk, top_k, seed, out):
    """the body sample_tokens and sample_tokens_ragged (pos_off given) share, after their check"""
    with torch.no_grad():
        a = _sample_accept(logits, pos, chk, top_k, seed, out, pos_off)
        if a is None:
            LAST_PATH[key] = L.PATH_GENERIC
            return _sample_torch(logits, pos, pos_off, *chk, top_k, seed, out)
        if out is None:
            out = tuple(torch.empty(chk[0], dtype=dt, device=logits.device) for dt in (torch.int32, torch.float32))
        base = getattr(a, "base", a)
        base.tokens, base.logprobs = out[0].data_ptr(), out[1].data_ptr()
        _row_launch(a, stem + "_step", key, logits.device, stem + "_workspace_bytes")
        return out[0], out[1]


def sample_tokens_supported(logits: torch.Tensor, pos: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                            seed: int = 0, out=None) -> bool:
    """True if mopk_sample_* take this call: CUDA fp32 / bf16 logits with unit inner stride, an int32 device pos, contiguous CUDA
    out buffers (the library's own query decides the rest: 2 <= V <= 2^24).  Raises ValueError on bad arguments."""
    chk = _sample_check(logits, pos, temperature, top_k, top_p, out, "sample_tokens_supported")
    return _sample_accept(logits, pos, chk, top_k, seed, out) is not None


def sample_tokens(logits: torch.Tensor, pos: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                  seed: int = 0, out=None):
    """draw one token per row from last-position logits -> (tokens int32 (R,), logprobs fp32 (R,)).  Inference only.

    logits: (R, V), or (R / n, V) shared by each item's n rows (then pass out buffers of R rows: row r reads logit row r // n);
    fp32 or bf16.  pos: (1,) int32 device tensor, the position of the token being chosen (the decoder cache's length after the step
    that produced the logits).  Per row r:
    - temperature == 0: argmax, ties to the smaller index (torch.argmax);
    - else z = x * inv_t with inv_t = 1 / temperature rounded to fp32 once; top_k > 0 keeps z >= the k-th largest z (counted with
      multiplicity, ties kept; top_k >= V is off); top_p < 1 keeps z >= tau, the largest z_u whose kept upper set
      {z_v >= z_u} holds at least top_p of the kept softmax mass.  The mass is fixed-point, q_v = int(exp(z_v - max z) * 2^40), and
      the test is sum q >= ceil(top_p * Q) in float64, so the threshold does not depend on summation order.  The rule is
      tie-inclusive (HF's top-p cuts a tie group by sort order instead) and never empty;
    - the draw is a Gumbel-max, argmax over the kept v of z_v - log(-log(u_v)) (ties to the smaller v): an exact sample of
      softmax(z) over the kept set.  u_v = ((h >> 9) + 0.5) * 2^-23, with h a hash of (seed, r, pos, v) built on common.h's fa_hash.
      It is a pure function of (logits, pos, seed, r);
    - logprobs[r] = log_softmax(float(x))[token] on the unscaled, unfiltered row (Whisper's sum_logprobs convention).
    out: static (tokens, logprobs) buffers, written in place (graph capture).  Runs the HIP kernel (mopk_sample_step) when
    sample_tokens_supported() accepts the call, else sample_tokens_torch(); LAST_PATH["sample"] records which.  No host sync."""
    chk = _sample_check(logits, pos, temperature, top_k, top_p, out, "sample_tokens")
    return _sample_run("mopk_sample", "sample", logits, pos, None, chk, top_k, seed, out)


# ---- sampling of a left-padded ragged batch (mopk_sample_ragged_*; WhisperMoP.sample with per-row prompt lengths) ----
def _sample_ragged_check(logits, pos, pos_off, temperature, top_k, top_p, out, what: str):
    R, n, inv_t, tp = _sample_check(logits, pos, temperature, top_k, top_p, out, what)
    if pos_off.dim() != 1 or pos_off.shape[0] != R or pos_off.dtype.is_floating_point or pos_off.dtype == torch.bool:
        raise ValueError(f"{what}: pos_off must be an integer ({R},) tensor (one offset per sampled row), got "
                         f"{tuple(pos_off.shape)} {pos_off.dtype}")
    return R, n, inv_t, tp


def sample_tokens_ragged_torch(logits: torch.Tensor, pos: torch.Tensor, pos_off: torch.Tensor, temperature: float = 1.0,
                               top_k: int = 0, top_p: float = 1.0, seed: int = 0, out=None):
    """the reference composition of `sample_tokens_ragged`: sample_tokens_torch with row r's draw at pos - pos_off[r]"""
    R, n, inv_t, tp = _sample_ragged_check(logits, pos, pos_off, temperature, top_k, top_p, out, "sample_tokens_ragged_torch")
    return _sample_torch(logits, pos, pos_off, R, n, inv_t, tp, top_k, seed, out)


def sample_tokens_ragged_supported(logits: torch.Tensor, pos: torch.Tensor, pos_off: torch.Tensor, temperature: float = 1.0,
                                   top_k: int = 0, top_p: float = 1.0, seed: int = 0, out=None) -> bool:
    """True if mopk_sample_ragged_* take this call: what sample_tokens_supported asks, and a contiguous CUDA int32 pos_off.
    Raises ValueError on bad arguments."""
    chk = _sample_ragged_check(logits, pos, pos_off, temperature, top_k, top_p, out, "sample_tokens_ragged_supported")
    return _sample_accept(logits, pos, chk, top_k, seed, out, pos_off) is not None


def sample_tokens_ragged(logits: torch.Tensor, pos: torch.Tensor, pos_off: torch.Tensor, temperature: float = 1.0, top_k: int = 0,
                         top_p: float = 1.0, seed: int = 0, out=None):
    """`sample_tokens` in which row r draws at position pos - pos_off[r] instead of pos: in a batch of prompts left-padded to one
    length, pos_off[r] = the row's padding makes a row's draws depend on its own token index only, so a row samples as it would
    alone.  pos_off: int32 (R,) device tensor, R the number of sampled rows.  With pos_off = 0 the draw is bitwise that of
    sample_tokens.  Runs the HIP kernel (mopk_sample_ragged_step) when sample_tokens_ragged_supported() accepts the call, else
    sample_tokens_ragged_torch(); LAST_PATH["sample_ragged"] records which.  No host sync."""
    chk = _sample_ragged_check(logits, pos, pos_off, temperature, top_k, top_p, out, "sample_tokens_ragged")
    return _sample_run("mopk_sample_ragged", "sample_ragged", logits, pos, pos_off, chk, top_k, seed, out)


# ---- Whisper's logit rules on last-position logits (mopk_logit_rules*; WhisperMoP decoding with logit rules) ----
class LogitRules:
    """Whisper's logit rules (the logit filters of OpenAI Whisper's decoding.py) for a vocabulary of `vocab_size` tokens.

    suppress_tokens: ids never emitted.  suppress_at_begin: ids blocked only at the first generated position (Whisper: blank and
    eot).  timestamp_begin: tb, the first timestamp token (None switches the timestamp rules off); eos_token_id is then required and
    must be < tb.  no_timestamps_token_id: blocked whenever tb is set.  max_initial_timestamp_index: the first timestamp is at most
    tb + this.  `logit_rules` documents the rules.  The constructor validates everything (ValueError) before any device work and
    builds the (V,) uint8 table once (bit 0: never emitted, the no-timestamps token included; bit 1: blocked at the first position);
    table(device) returns its copy on a device, made once per device (pass `device` to make it at construction).
    A row that these lists block completely comes out all -inf: there is no guard."""

    def __init__(self, vocab_size: int, suppress_tokens=(), suppress_at_begin=(), timestamp_begin: Optional[int] = None,
                 eos_token_id: Optional[int] = None, no_timestamps_token_id: Optional[int] = None,
                 max_initial_timestamp_index: Optional[int] = None, device=None):
        def _int(x, name):
            if isinstance(x, bool) or int(x) != x:
                raise ValueError(f"LogitRules: {name} must be an integer, got {x!r}")
            return int(x)

        V = _int(vocab_size, "vocab_size")
        if V < 2:
            raise ValueError(f"LogitRules: vocab_size must be >= 2, got {V}")

        def _id(x, name):
            x = _int(x, name)
            if not 0 <= x < V:
                raise ValueError(f"LogitRules: {name} = {x} outside [0, vocab_size = {V})")
            return x

        self.vocab_size = V
        self.suppress_tokens = tuple(_id(t, "suppress_tokens id") for t in suppress_tokens)
        self.suppress_at_begin = tuple(_id(t, "suppress_at_begin id") for t in suppress_at_begin)
        self.timestamp_begin = None if timestamp_begin is None else _id(timestamp_begin, "timestamp_begin")
        self.eos_token_id = None if eos_token_id is None else _id(eos_token_id, "eos_token_id")
        self.no_timestamps_token_id = None if no_timestamps_token_id is None else _id(no_timestamps_token_id,
                                                                                      "no_timestamps_token_id")
        self.max_initial_timestamp_index = None if max_initial_timestamp_index is None else _int(
            max_initial_timestamp_index, "max_initial_timestamp_index")
        if self.max_initial_timestamp_index is not None and self.max_initial_timestamp_index < 0:
            raise ValueError(f"LogitRules: max_initial_timestamp_index must be >= 0, got {max_initial_timestamp_index}")
        if self.timestamp_begin is not None:
            if self.eos_token_id is None:
                raise ValueError("LogitRules: timestamp_begin needs eos_token_id")
            if not self.eos_token_id < self.timestamp_begin:
                raise ValueError(f"LogitRules: needs eos_token_id < timestamp_begin, got {self.eos_token_id} >= {self.timestamp_begin}")
        mask = torch.zeros(V, dtype=torch.uint8)
        never = list(self.suppress_tokens)
        if self.timestamp_begin is not None and self.no_timestamps_token_id is not None:
            never.append(self.no_timestamps_token_id)
        if never:
            mask[torch.tensor(never, dtype=torch.long)] |= 1
        if self.suppress_at_begin:
            mask[torch.tensor(self.suppress_at_begin, dtype=torch.long)] |= 2
        self._tables = {torch.device("cpu"): mask}
        if device is not None:
            self.table(device)

    def table(self, device) -> torch.Tensor:
        """the (V,) uint8 table on `device` (copied there once, without a host sync)"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._tables.get(device)
        if t is None:
            cpu = self._tables[torch.device("cpu")]
            t = cpu.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else cpu.to(device)
            self._tables[device] = t
        return t


def _lr_check(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules, out, what: str, kind=None) -> None:
    """validate a logit-rules call (or, with kind = RepeatRules, a repeat-rules call: the same arguments) before any device work"""
    kind = LogitRules if kind is None else kind
    if not isinstance(rules, kind):
        raise ValueError(f"{what}: rules must be a {kind.__name__}, got {type(rules).__name__}")
    if logits.dim() != 2 or logits.shape[0] < 1 or not logits.dtype.is_floating_point:
        raise ValueError(f"{what}: logits must be a floating (rows, V) tensor, got {tuple(logits.shape)} {logits.dtype}")
    if logits.shape[1] != rules.vocab_size:
        raise ValueError(f"{what}: logits have V = {logits.shape[1]}, the rules were built for vocab_size = {rules.vocab_size}")
    if hist.dim() != 2 or hist.shape[0] != logits.shape[0] or hist.dtype.is_floating_point or hist.dtype == torch.bool:
        raise ValueError(f"{what}: hist must be an integer ({logits.shape[0]}, T) tensor, got {tuple(hist.shape)} {hist.dtype}")
    if isinstance(t0, bool) or int(t0) != t0 or not 0 <= t0 <= hist.shape[1]:
        raise ValueError(f"{what}: t0 must be an integer in [0, T = {hist.shape[1]}], got {t0}")
    if pos.numel() != 1 or pos.dtype.is_floating_point:
        raise ValueError(f"{what}: pos must hold one integer, got shape {tuple(pos.shape)} {pos.dtype}")
    if out is not None and (out.shape != logits.shape or out.dtype != logits.dtype or out.device != logits.device):
        raise ValueError(f"{what}: out must match logits ({tuple(logits.shape)} {logits.dtype}), got {tuple(out.shape)} {out.dtype}")


def logit_rules_torch(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: LogitRules, out=None):
    """the restatement of `logit_rules` in torch ops (CPU or GPU, vectorised over rows, no host sync): the same rules in the same
    order, rule 3e in fp32 as documented there (L = m + log(sum(exp(x - m))))"""
    _lr_check(logits, hist, pos, t0, rules, out, "logit_rules_torch")
    R, V = logits.shape
    dev, T, t0 = logits.device, hist.shape[1], int(t0)
    mask = rules.table(dev)
    n = (pos.reshape(()).to(torch.long) - t0).clamp(0, T - t0)
    first = n == 0
    blocked = ((mask & 1) != 0) | (first & ((mask & 2) != 0))                      # rules 1 and 2
    blocked = blocked.unsqueeze(0).expand(R, V)
    tb = rules.timestamp_begin
    if tb is not None:
        g = F.pad(hist[:, t0:].to(torch.long), (0, 1))                             # one spare column: the gathers below stay inside
        j = torch.arange(g.shape[1], device=dev)
        at = lambda i: g.index_select(1, i.clamp_min(0).reshape(1)).squeeze(1)     # noqa: E731  g[:, i] at a device index
        last = (n >= 1) & (at(n - 1) >= tb)
        pen = (n < 2) | (at(n - 2) >= tb)
        pair, lone = last & pen, last & ~pen
        li = torch.where((g >= tb) & (j < n), j, -1).max(1).values                 # the last timestamp in sequence order
        t = g.gather(1, li.clamp_min(0).unsqueeze(1)).squeeze(1)
        text_lo = torch.where(lone, rules.eos_token_id, 0)                         # 3b: x[:eos]
        ts_lo = torch.where(li >= 0, torch.where(lone, t, t + 1), tb)              # 3c: x[tb:lim]
        ts_lo = torch.where(pair, V, ts_lo)                                        # 3b: x[tb:]
        text_lo = torch.where(first, tb, text_lo)                                  # 3d: x[:tb]
        k = rules.max_initial_timestamp_index
        ts_hi = torch.where(first, V - 1 if k is None else min(tb + k, V - 1), V - 1)
        v = torch.arange(V, device=dev).unsqueeze(0)
        text = v < tb
        blocked = blocked | torch.where(text, v < text_lo.unsqueeze(1), (v < ts_lo.unsqueeze(1)) | (v > ts_hi))
        x = logits.float().masked_fill(blocked, float("-inf"))                     # 3e, on the row as masked so far
        m = x[:, tb:].max(1).values
        m0 = torch.where(m == float("-inf"), torch.zeros_like(m), m)
        lse = m + torch.log(torch.exp(x[:, tb:] - m0.unsqueeze(1)).sum(1))          # -inf for an all-blocked side
        blocked = blocked | ((lse > x[:, :tb].max(1).values).unsqueeze(1) & text)
    y = logits.masked_fill(blocked, float("-inf"))
    if out is None:
        return y
    out.copy_(y)
    return out


def _lr_args(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: LogitRules, out) -> L.LogitRulesArgs:
    a = L.LogitRulesArgs()
    a.R, a.V, a.T, a.T0 = logits.shape[0], logits.shape[1], hist.shape[1], int(t0)
    a.dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.tb = -1 if rules.timestamp_begin is None else rules.timestamp_begin
    a.eos = 0 if rules.eos_token_id is None else rules.eos_token_id
    k = rules.max_initial_timestamp_index
    a.max_initial = -1 if k is None else min(k, a.V)
    a.logits, a.logits_ld, a.out, a.out_ld = logits.data_ptr(), logits.stride(0), out.data_ptr(), out.stride(0)
    a.hist, a.hist_ld, a.pos, a.mask = hist.data_ptr(), hist.stride(0), pos.data_ptr(), rules.table(logits.device).data_ptr()
    if a.R == 1:                                                                   # a single row: its strides are never used
        a.logits_ld = a.out_ld = a.V
        a.hist_ld = a.T
    return a


def _lr_tensors_ok(logits, o, hist, pos) -> bool:
    """the tensor-side tests that logit_rules and repeat_rules share: CUDA fp32 / bf16 rows, a CUDA int32 history and position"""
    R, V = logits.shape
    for t in (logits, o):
        if not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16) or t.stride(1) != 1 or (R > 1 and t.stride(0) < V):
            return False
    T = hist.shape[1]
    if not hist.is_cuda or hist.dtype != torch.int32 or (T > 1 and hist.stride(1) != 1) or (R > 1 and hist.stride(0) < T):
        return False
    return pos.is_cuda and pos.dtype == torch.int32


def _lr_accept(logits, hist, pos, t0, rules, out):
    """the args struct of a call that mopk_logit_rules takes, None of one it refuses; out None: `logits` stands in for the result"""
    o = logits if out is None else out
    if not _lr_tensors_ok(logits, o, hist, pos):
        return None
    a = _lr_args(logits, hist, pos, t0, rules, o)
    return a if L.lib().mopk_logit_rules_supported(C.byref(a)) else None


def logit_rules_supported(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: LogitRules, out=None) -> bool:
    """True if mopk_logit_rules takes this call: CUDA fp32 / bf16 logits (and out) with unit inner stride and a row stride >= V
    (one row: any), a CUDA int32 hist with unit inner stride and a row stride >= T, an int32 device pos (the library's own query
    decides the rest).  Raises ValueError on bad arguments."""
    _lr_check(logits, hist, pos, t0, rules, out, "logit_rules_supported")
    return _lr_accept(logits, hist, pos, t0, rules, out) is not None


def logit_rules(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: LogitRules, out=None):
    """apply Whisper's logit rules to last-position logits -> the filtered logits, (R, V) in the logits' dtype: every entry is
    the input's bits, or -inf ("blocked").  Inference only.

    logits: (R, V) fp32 or bf16, any row stride.  hist: (R, T) int32 token histories (any row stride: a caller may pass
    hist[::K]).  pos: (1,) int32 device tensor, the column of the token being chosen; t0: the first generated column (the same for
    every row: ragged prompts are left-padded).  Per row, g = hist[r, t0:pos] are the n = pos - t0 tokens generated so far, and,
    in this order:
    1. every id of rules.suppress_tokens is blocked;
    2. n == 0: every id of rules.suppress_at_begin is blocked;
    3. with tb = rules.timestamp_begin set (timestamp tokens are the ids >= tb):
       a. rules.no_timestamps_token_id, if given, is blocked;
       b. last = n >= 1 and g[n-1] >= tb, pen = n < 2 or g[n-2] >= tb.  last and pen: x[tb:] is blocked (a pair is complete, text
          follows); last and not pen: x[:eos] is blocked (a lone timestamp after text is followed by a timestamp or eos);
       c. t = the last g[i] >= tb, if any: x[tb:lim] is blocked, lim = t if last and not pen, else t + 1 (never decreasing);
       d. n == 0: x[:tb] is blocked (the first token is a timestamp), and x[tb + k + 1:] with k = max_initial_timestamp_index;
       e. on the row as masked so far, in fp32: m = max x[tb:], L = m + log(sum(exp(x[tb:] - m))), M = max x[:tb] (an all-blocked
          side gives -inf); L > M: x[:tb] is blocked (the softmax normaliser cancels on both sides).
    A row that the caller's lists block completely comes out all -inf: there is no guard.  out: a static result buffer; it may be
    `logits` itself.  Runs the HIP kernel (mopk_logit_rules: one launch) when logit_rules_supported() accepts the call, else
    logit_rules_torch(); LAST_PATH["logit_rules"] records which.  No host sync; bitwise reproducible."""
    _lr_check(logits, hist, pos, t0, rules, out, "logit_rules")
    with torch.no_grad():
        a = _lr_accept(logits, hist, pos, t0, rules, out)
        if a is None:
            LAST_PATH["logit_rules"] = L.PATH_GENERIC
            return logit_rules_torch(logits, hist, pos, t0, rules, out)
        if out is None:
            out = torch.empty_like(logits, memory_format=torch.contiguous_format)
            a.out, a.out_ld = out.data_ptr(), out.stride(0)                        # in place of the stand-in
        _row_launch(a, "mopk_logit_rules", "logit_rules")
        return out


# ---- repetition penalty and no-repeat n-gram blocking on last-position logits (mopk_repeat_rules*; WhisperMoP decoding) ----
REPEAT_MAX_GENERATED = 4096                                                        # T - t0 the kernel stages in LDS


class RepeatRules:
    """The two per-step controls against repetition loops for a vocabulary of `vocab_size` tokens: `repetition_penalty` (HF's
    RepetitionPenaltyLogitsProcessor; 1.0 is off) and `no_repeat_ngram_size` (HF's NoRepeatNGramLogitsProcessor; 0 is off), both
    over the GENERATED tokens only.  `repeat_rules` documents them.

    exempt_tokens: ids that are never penalised or banned; exempt_from: every id >= it is exempt too (None: none).  The
    constructor validates everything (ValueError) before any device work, builds the (V,) uint8 exemption table once (1: exempt)
    and stores inv_penalty, the fp32 value of 1 / repetition_penalty, computed once on the host; table(device) returns the
    table's copy on a device, made once per device (pass `device` to make it at construction).  neutral: penalty 1.0 and
    n-gram size 0, rules that change nothing."""

    def __init__(self, vocab_size: int, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, exempt_tokens=(),
                 exempt_from: Optional[int] = None, device=None):
        def _int(x, name):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or int(x) != x:
                raise ValueError(f"RepeatRules: {name} must be an integer, got {x!r}")
            return int(x)

        V = _int(vocab_size, "vocab_size")
        if V < 2:
            raise ValueError(f"RepeatRules: vocab_size must be >= 2, got {V}")
        p = repetition_penalty
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or not p > 0:
            raise ValueError(f"RepeatRules: repetition_penalty must be a finite number > 0, got {p!r}")
        p32 = torch.tensor(float(p), dtype=torch.float32)
        inv = 1.0 / p32                                                            # fp32, once, on the host
        if not (math.isfinite(p32.item()) and p32.item() > 0 and math.isfinite(inv.item()) and inv.item() > 0):
            raise ValueError(f"RepeatRules: repetition_penalty = {p!r} or its reciprocal is not a positive finite fp32 number")
        s = _int(no_repeat_ngram_size, "no_repeat_ngram_size")
        if s < 0:
            raise ValueError(f"RepeatRules: no_repeat_ngram_size must be >= 0, got {s}")
        ids = []
        for t in exempt_tokens:
            t = _int(t, "exempt_tokens id")
            if not 0 <= t < V:
                raise ValueError(f"RepeatRules: exempt_tokens id = {t} outside [0, vocab_size = {V})")
            ids.append(t)
        if exempt_from is not None:
            exempt_from = _int(exempt_from, "exempt_from")
            if not 0 <= exempt_from <= V:
                raise ValueError(f"RepeatRules: exempt_from = {exempt_from} outside [0, vocab_size = {V}]")
        self.vocab_size, self.no_repeat_ngram_size = V, s
        self.repetition_penalty, self.inv_penalty = p32.item(), inv.item()         # both as their fp32 values
        self.exempt_tokens, self.exempt_from = tuple(ids), exempt_from
        self.neutral = self.repetition_penalty == 1.0 and s == 0
        table = torch.zeros(V, dtype=torch.uint8)
        if ids:
            table[torch.tensor(ids, dtype=torch.long)] = 1
        if exempt_from is not None:
            table[exempt_from:] = 1
        self._tables = {torch.device("cpu"): table}
        if device is not None:
            self.table(device)

    table = LogitRules.table

    @classmethod
    def for_whisper(cls, logit_rules: LogitRules, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                    extra_exempt=()) -> "RepeatRules":
        """the repeat rules that go with a Whisper `logit_rules`: logit_rules.eos_token_id (when set) and every timestamp token,
        the ids >= logit_rules.timestamp_begin (when set), are exempt, and so are the ids of extra_exempt.  The timestamps must
        be: a segment's closing <|t|> and the next segment's opening <|t|> are legitimately the same token twice, and
        ops.timestamp_segments cuts the segments at exactly such pairs; a penalty or a ban on them would break the grammar that
        transcribe relies on.  Use this constructor for with_logit_rules(...).transcribe."""
        if not isinstance(logit_rules, LogitRules):
            raise ValueError(f"RepeatRules.for_whisper: logit_rules must be a LogitRules, got {type(logit_rules).__name__}")
        exempt = list(extra_exempt)
        if logit_rules.eos_token_id is not None:
            exempt.append(logit_rules.eos_token_id)
        return cls(logit_rules.vocab_size, repetition_penalty, no_repeat_ngram_size, exempt, logit_rules.timestamp_begin)


def _rr_check(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: RepeatRules, out, what: str) -> None:
    """validate a repeat-rules call before any device work: logit_rules' arguments with a RepeatRules"""
    _lr_check(logits, hist, pos, t0, rules, out, what, RepeatRules)


def repeat_rules_torch(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: RepeatRules, out=None):
    """the restatement of `repeat_rules` in torch ops (CPU or GPU, vectorised over rows, no host sync): the same steps in the
    same order, the penalty in fp32 with the same two constants, so it agrees with the kernel bit for bit"""
    _rr_check(logits, hist, pos, t0, rules, out, "repeat_rules_torch")
    R, V = logits.shape
    dev, T, t0 = logits.device, hist.shape[1], int(t0)
    s, G = rules.no_repeat_ngram_size, T - t0
    y = logits
    if G > 0 and not rules.neutral:
        n = (pos.reshape(()).to(torch.long) - t0).clamp(0, G)
        g = hist[:, t0:].to(torch.long)                                            # (R, G), raw values
        j = torch.arange(G, device=dev)
        gc = g.clamp(0, V - 1)
        ok = (j < n) & (g >= 0) & (g < V) & (rules.table(dev)[gc] == 0)            # positions whose token can be changed
        if rules.repetition_penalty != 1.0:
            seen = torch.zeros(R, V, dtype=torch.int32, device=dev).scatter_add_(1, gc, ok.to(torch.int32)) > 0
            x = logits.float()
            pen = torch.where(x < 0, x * rules.repetition_penalty, x * rules.inv_penalty).to(logits.dtype)
            y = torch.where(seen, pen, y)
        W = G - s + 1                                                              # n-gram windows that fit
        if s >= 1 and W >= 1:
            same = (torch.arange(W, device=dev) <= n - s).unsqueeze(0).expand(R, W)
            for k in range(s - 1):                                                 # window i against ctx = g[n - s + 1 : n]
                ctx = g.index_select(1, (n - s + 1 + k).clamp(0, G - 1).reshape(1))
                same = same & (g[:, k:k + W] == ctx)
            hit = (same & ok[:, s - 1:]).to(torch.int32)
            ban = torch.zeros(R, V, dtype=torch.int32, device=dev).scatter_add_(1, gc[:, s - 1:], hit) > 0
            y = y.masked_fill(ban, float("-inf"))
    if out is None:
        return y.clone() if y is logits else y
    if out is not y:
        out.copy_(y)
    return out


def _rr_args(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: RepeatRules, out) -> L.RepeatRulesArgs:
    a = L.RepeatRulesArgs()
    a.R, a.V, a.T, a.T0 = logits.shape[0], logits.shape[1], hist.shape[1], int(t0)
    a.dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.ngram, a.penalty, a.inv_penalty = rules.no_repeat_ngram_size, rules.repetition_penalty, rules.inv_penalty
    a.logits, a.logits_ld, a.out, a.out_ld = logits.data_ptr(), logits.stride(0), out.data_ptr(), out.stride(0)
    a.hist, a.hist_ld, a.pos, a.exempt = hist.data_ptr(), hist.stride(0), pos.data_ptr(), rules.table(logits.device).data_ptr()
    if a.R == 1:                                                                   # a single row: its strides are never used
        a.logits_ld = a.out_ld = a.V
        a.hist_ld = a.T
    return a


def _rr_accept(logits, hist, pos, t0, rules, out):
    """the args struct of a call that mopk_repeat_rules takes, None of one it refuses; out None: `logits` stands in for the result"""
    if not _lr_tensors_ok(logits, logits if out is None else out, hist, pos):
        return None
    a = _rr_args(logits, hist, pos, t0, rules, logits if out is None else out)
    return a if L.lib().mopk_repeat_rules_supported(C.byref(a)) else None


def repeat_rules_supported(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: RepeatRules, out=None) -> bool:
    """True if mopk_repeat_rules takes this call: the tensors that logit_rules_supported asks for, and T - t0 <= 4096 generated
    columns (the library's own query decides that and the rest).  Raises ValueError on bad arguments."""
    _rr_check(logits, hist, pos, t0, rules, out, "repeat_rules_supported")
    return _rr_accept(logits, hist, pos, t0, rules, out) is not None


def repeat_rules(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, t0: int, rules: RepeatRules, out=None):
    """apply a repetition penalty and no-repeat n-gram blocking to last-position logits -> the logits, (R, V) in their dtype.
    Inference only.  The arguments are those of `logit_rules`: logits (R, V) fp32 or bf16, any row stride; hist (R, T) int32
    token histories, any row stride (hist[::K]); pos a (1,) int32 device tensor, the column of the token being chosen; t0 the
    first generated column, the same for every row.

    Per row, n = clamp(pos - t0, 0, T - t0) and g = hist[r, t0 : t0 + n]: only the generated tokens count (the prompt may be
    left padding or the previous window's text).  With p = rules.repetition_penalty and s = rules.no_repeat_ngram_size, in this
    order:
    0. out[r] = logits[r], bit for bit;
    1. p != 1: every distinct v in g with 0 <= v < V that is not exempt gets, in fp32, x = float(logits[r, v]) and
       out[r, v] = x * p if x < 0 else x * rules.inv_penalty, rounded to the logits' dtype (bf16: to nearest even).  A token that
       occurs several times is penalised once; -inf stays -inf and NaN stays NaN.  This is HF's RepetitionPenaltyLogitsProcessor
       with its division written as a multiplication by the fp32 reciprocal that the host computed once (so that the kernel and
       the torch restatement agree bitwise): the result may differ from a true division by one ulp;
    2. s >= 1 and n >= s - 1: with ctx = g[n - s + 1 : n] (s - 1 tokens compared as raw int32 values; empty for s = 1), every i in
       [0, n - s] with g[i : i + s - 1] == ctx names v = g[i + s - 1]; 0 <= v < V and not exempt: out[r, v] = -inf, whether or
       not step 1 penalised it.  This is HF's NoRepeatNGramLogitsProcessor restricted to the generated part.
    Every other entry is the input's bits.  A row that the rules block completely comes out all -inf: there is no guard.  Neutral
    rules are a valid call: the result equals the input.  out: a static result buffer; it may be `logits` itself, and the kernel
    then reads and writes only the entries it changes.  Runs the HIP kernel (mopk_repeat_rules: one launch, one workgroup per
    row) when repeat_rules_supported() accepts the call (T - t0 <= 4096), else repeat_rules_torch(); LAST_PATH["repeat_rules"]
    records which.  No host sync; bitwise reproducible."""
    _rr_check(logits, hist, pos, t0, rules, out, "repeat_rules")
    with torch.no_grad():
        a = _rr_accept(logits, hist, pos, t0, rules, out)
        if a is None:
            LAST_PATH["repeat_rules"] = L.PATH_GENERIC
            return repeat_rules_torch(logits, hist, pos, t0, rules, out)
        if out is None:
            out = torch.empty_like(logits, memory_format=torch.contiguous_format)
            a.out, a.out_ld = out.data_ptr(), out.stride(0)                        # in place of the stand-in
        _row_launch(a, "mopk_repeat_rules", "repeat_rules")
        return out


# ---- per-step decoding statistics (mopk_token_logprob, mopk_greedy_pick; WhisperMoP's return_stats, transcribe's fallback) ----
def _is_index(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, int)


def _stat_logits_check(logits, what: str) -> None:
    if (not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 2
            or not logits.dtype.is_floating_point):
        raise ValueError(f"{what}: logits must be a floating (rows, V) tensor with V >= 2, got "
                         f"{(tuple(logits.shape), logits.dtype) if isinstance(logits, torch.Tensor) else type(logits).__name__}")


def _stat_logits_ok(logits: torch.Tensor) -> bool:
    """the tensor-side tests the two kernels share: CUDA fp32 / bf16, unit inner stride, a row stride >= V (one row: any)"""
    R, V = logits.shape
    return (logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16) and logits.stride(1) == 1
            and (R == 1 or logits.stride(0) >= V))


def _tl_check(logits, tokens, out, what: str) -> None:
    """validate a token_logprob call before any device work"""
    _stat_logits_check(logits, what)
    R, V = logits.shape
    if isinstance(tokens, torch.Tensor):
        if tuple(tokens.shape) != (R,) or tokens.dtype.is_floating_point or tokens.dtype.is_complex or tokens.dtype == torch.bool:
            raise ValueError(f"{what}: tokens must be an integer ({R},) tensor or an int, got {tuple(tokens.shape)} {tokens.dtype}")
        if tokens.device != logits.device:
            raise ValueError(f"{what}: tokens are on {tokens.device}, the logits on {logits.device}")
        if not tokens.is_cuda and bool(((tokens < 0) | (tokens >= V)).any()):          # host values: the host can know
            raise ValueError(f"{what}: a token lies outside [0, V = {V})")
    elif not _is_index(tokens) or not 0 <= tokens < V:
        raise ValueError(f"{what}: tokens must be an integer ({R},) tensor or an int in [0, V = {V}), got {tokens!r}")
    if out is not None and (tuple(out.shape) != (R,) or out.dtype != torch.float32 or out.device != logits.device):
        raise ValueError(f"{what}: out must be an fp32 ({R},) tensor on {logits.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")


def token_logprob_torch(logits: torch.Tensor, tokens, out=None) -> torch.Tensor:
    """the restatement of `token_logprob` in torch ops (no host sync): log_softmax(logits.float(), -1) gathered at the tokens
    (a device token outside [0, V) is clamped, as in the kernel)"""
    _tl_check(logits, tokens, out, "token_logprob_torch")
    R, V = logits.shape
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.full((R,), tokens, dtype=torch.long, device=logits.device)
    lp = torch.log_softmax(logits.float(), -1).gather(1, tokens.to(torch.long).clamp(0, V - 1).unsqueeze(1)).squeeze(1)
    if out is None:
        return lp
    out.copy_(lp)
    return out


def _tl_accept(logits, tokens, out):
    """the args struct of a call that mopk_token_logprob takes, None of one it refuses; out None: the result buffer is left NULL
    (the query looks at its alignment only; the launcher fills it in)"""
    if not _stat_logits_ok(logits):
        return None
    a = L.TokenLogprobArgs()
    a.R, a.V = logits.shape
    a.dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.logits, a.logits_ld = logits.data_ptr(), a.V if a.R == 1 else logits.stride(0)   # a single row: its stride is never used
    if isinstance(tokens, torch.Tensor):
        if not tokens.is_cuda or tokens.dtype != torch.int32 or not tokens.is_contiguous():
            return None
        a.tokens = tokens.data_ptr()
    else:
        a.token = tokens
    if out is not None and not (out.is_cuda and out.is_contiguous()):
        return None
    if out is not None:
        a.out = out.data_ptr()
    return a if L.lib().mopk_token_logprob_supported(C.byref(a)) else None


def token_logprob_supported(logits: torch.Tensor, tokens, out=None) -> bool:
    """True if mopk_token_logprob takes this call: CUDA fp32 / bf16 logits with unit inner stride and a row stride >= V (one
    row: any), tokens an int or a contiguous CUDA int32 tensor, a contiguous CUDA out (the library's own query decides the
    rest).  Raises ValueError on bad arguments."""
    _tl_check(logits, tokens, out, "token_logprob_supported")
    return _tl_accept(logits, tokens, out) is not None


def token_logprob(logits: torch.Tensor, tokens, out=None) -> torch.Tensor:
    """the log-probability of one token per row -> fp32 (R,): out[r] = float(logits[r, tokens[r]]) - lse(logits[r]), in fp32.
    Inference only.

    logits: (R, V) fp32 or bf16, any row stride >= V (a column of a (B, T, V) tensor is one).  tokens: an int32 (R,) tensor on the
    logits' device, or one int for every row.  -inf entries add nothing to the lse; a token whose own entry is -inf gives -inf.  A
    row without a finite entry is outside the contract (its value is unspecified).  A token outside [0, V) is a ValueError where
    the host can see it (an int, a CPU tensor); a device token is clamped into the row.  out: a static fp32 (R,) result buffer.
    Runs the HIP kernel (mopk_token_logprob: one launch) when token_logprob_supported() accepts the call, else
    token_logprob_torch(); LAST_PATH["token_logprob"] records which.  No host sync; bitwise reproducible."""
    _tl_check(logits, tokens, out, "token_logprob")
    with torch.no_grad():
        a = _tl_accept(logits, tokens, out)
        if a is None:
            LAST_PATH["token_logprob"] = L.PATH_GENERIC
            return token_logprob_torch(logits, tokens, out)
        if out is None:
            out = torch.empty(a.R, dtype=torch.float32, device=logits.device)
            a.out = out.data_ptr()
        _row_launch(a, "mopk_token_logprob", "token_logprob")
        return out


# ---- language probabilities on last-position logits (mopk_language_probs; WhisperMoP.detect_language) ----
class LanguageTokens:
    """The language tokens of a vocabulary of `vocab_size` tokens (the tokenizer's share of Whisper's detect_language).

    token_ids: 1 <= n <= 1024 distinct integer ids, each in [0, vocab_size); their order is the column order of the probabilities
    that `language_probs` returns.  The constructor validates everything (ValueError) before any device work and builds the (n,)
    int32 table once; table(device) returns its copy on a device, made once per device (pass `device` to make it at construction)."""

    def __init__(self, vocab_size: int, token_ids, device=None):
        def _int(x, name):
            try:
                ok = not isinstance(x, bool) and int(x) == x
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"LanguageTokens: {name} must be an integer, got {x!r}")
            return int(x)

        V = _int(vocab_size, "vocab_size")
        if V < 2:
            raise ValueError(f"LanguageTokens: vocab_size must be >= 2, got {V}")
        if isinstance(token_ids, torch.Tensor):
            token_ids = token_ids.reshape(-1).tolist()
        try:
            ids = tuple(_int(t, "a token id") for t in token_ids)
        except TypeError:
            raise ValueError(f"LanguageTokens: token_ids must be a sequence of integers, got {type(token_ids).__name__}") from None
        if not 1 <= len(ids) <= L.LANGUAGE_MAX_N:
            raise ValueError(f"LanguageTokens: needs 1 <= n <= {L.LANGUAGE_MAX_N} language tokens, got {len(ids)}")
        for t in ids:
            if not 0 <= t < V:
                raise ValueError(f"LanguageTokens: token id {t} outside [0, vocab_size = {V})")
        if len(set(ids)) != len(ids):
            raise ValueError("LanguageTokens: the token ids must be distinct")
        self.vocab_size, self.token_ids, self.n = V, ids, len(ids)
        self._tables = {torch.device("cpu"): torch.tensor(ids, dtype=torch.int32)}
        if device is not None:
            self.table(device)

    table = LogitRules.table

    @classmethod
    def for_whisper(cls, vocab_size: int, sot_token_id: int, n_languages: int, device=None) -> "LanguageTokens":
        """Whisper's layout: the n_languages language tokens follow <|startoftranscript|>, ids sot + 1 ... sot + n_languages"""
        for name, x in (("sot_token_id", sot_token_id), ("n_languages", n_languages)):
            if not _is_index(x):
                raise ValueError(f"LanguageTokens.for_whisper: {name} must be an int, got {x!r}")
        if n_languages < 1:
            raise ValueError(f"LanguageTokens.for_whisper: n_languages must be >= 1, got {n_languages}")
        return cls(vocab_size, range(sot_token_id + 1, sot_token_id + 1 + n_languages), device)


class LanguageProbs(NamedTuple):
    """what `language_probs` returns: probs (R, n) fp32, the softmax over the language tokens' logits in the LanguageTokens'
    order; tokens (R,) int32, the most probable language token of each row"""
    probs: torch.Tensor
    tokens: torch.Tensor


def _lp_check(logits, languages, out_probs, out_tokens, what: str) -> None:
    """validate a language_probs call before any device work"""
    if not isinstance(languages, LanguageTokens):
        raise ValueError(f"{what}: languages must be a LanguageTokens, got {type(languages).__name__}")
    _stat_logits_check(logits, what)
    R, V = logits.shape
    if V != languages.vocab_size:
        raise ValueError(f"{what}: logits have V = {V}, the languages were built for vocab_size = {languages.vocab_size}")
    n = languages.n
    if out_probs is not None and (not isinstance(out_probs, torch.Tensor) or tuple(out_probs.shape) != (R, n)
                                  or out_probs.dtype != torch.float32 or out_probs.device != logits.device):
        raise ValueError(f"{what}: out_probs must be an fp32 ({R}, {n}) tensor on {logits.device}, got "
                         f"{(tuple(out_probs.shape), out_probs.dtype, out_probs.device) if isinstance(out_probs, torch.Tensor) else type(out_probs).__name__}")
    if out_tokens is not None and (not isinstance(out_tokens, torch.Tensor) or tuple(out_tokens.shape) != (R,)
                                   or out_tokens.dtype != torch.int32 or out_tokens.device != logits.device):
        raise ValueError(f"{what}: out_tokens must be an int32 ({R},) tensor on {logits.device}, got "
                         f"{(tuple(out_tokens.shape), out_tokens.dtype, out_tokens.device) if isinstance(out_tokens, torch.Tensor) else type(out_tokens).__name__}")


def language_probs_torch(logits: torch.Tensor, languages: LanguageTokens, out_probs=None, out_tokens=None) -> LanguageProbs:
    """the restatement of `language_probs` in torch ops (CPU or GPU, no host sync): the language columns gathered and widened to
    fp32, exp(x - logsumexp(x)), and of the columns that hold the row's maximum the smallest token id"""
    _lp_check(logits, languages, out_probs, out_tokens, "language_probs_torch")
    ids = languages.table(logits.device)
    x = logits.index_select(1, ids.to(torch.long)).float()                         # (R, n)
    probs = (x - torch.logsumexp(x, 1, keepdim=True)).exp()
    best = x == x.max(1, keepdim=True).values
    tokens = torch.where(best, ids.unsqueeze(0), torch.full_like(ids, 0x7fffffff).unsqueeze(0)).min(1).values
    if out_probs is not None:
        out_probs.copy_(probs)
        probs = out_probs
    if out_tokens is not None:
        out_tokens.copy_(tokens)
        tokens = out_tokens
    return LanguageProbs(probs, tokens)


def _lp_accept(logits, languages, out_probs, out_tokens):
    """the args struct of a call that mopk_language_probs takes, None of one it refuses; an out_ buffer that is None is left NULL
    (the query looks at alignment and stride only; the launcher fills it in)"""
    if not _stat_logits_ok(logits):
        return None
    a = L.LanguageProbsArgs()
    a.R, a.V = logits.shape
    a.n = languages.n
    a.dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.logits, a.logits_ld = logits.data_ptr(), a.V if a.R == 1 else logits.stride(0)   # a single row: its stride is never used
    a.probs_ld = a.n
    if out_probs is not None:
        if not out_probs.is_cuda or out_probs.stride(1) != 1 or (a.R > 1 and out_probs.stride(0) < a.n):
            return None
        a.probs, a.probs_ld = out_probs.data_ptr(), a.n if a.R == 1 else out_probs.stride(0)
    if out_tokens is not None:
        if not (out_tokens.is_cuda and out_tokens.is_contiguous()):
            return None
        a.tokens = out_tokens.data_ptr()
    a.ids = languages.table(logits.device).data_ptr()
    return a if L.lib().mopk_language_probs_supported(C.byref(a)) else None


def language_probs_supported(logits: torch.Tensor, languages: LanguageTokens, out_probs=None, out_tokens=None) -> bool:
    """True if mopk_language_probs takes this call: CUDA fp32 / bf16 logits with unit inner stride and a row stride >= V (one row:
    any), a CUDA out_probs with unit inner stride and a row stride >= n, a contiguous CUDA out_tokens (the library's own query
    decides the rest).  Raises ValueError on bad arguments."""
    _lp_check(logits, languages, out_probs, out_tokens, "language_probs_supported")
    return _lp_accept(logits, languages, out_probs, out_tokens) is not None


def language_probs(logits: torch.Tensor, languages: LanguageTokens, out_probs=None, out_tokens=None) -> LanguageProbs:
    """the probability of each language and the most probable one -> LanguageProbs(probs (R, n) fp32, tokens (R,) int32): Whisper's
    detect_language on the logits that follow <|startoftranscript|>.  Inference only.

    logits: (R, V) fp32 or bf16, any row stride >= V (a column of a (B, T, V) tensor is one).  languages: a LanguageTokens built
    for V, n tokens t_0 ... t_{n-1}.  Per row, in fp32: x_i = float(logits[r, t_i]); probs[r, i] = exp(x_i - lse(x)), the softmax
    over the language tokens alone (every other token is masked, as in Whisper), 0 where x_i = -inf; tokens[r] = the t_i with the
    largest x_i, ties to the smaller token id (the argmax over the masked vocabulary).  A row without a finite language entry is
    outside the contract (its values are unspecified).  out_probs: a static fp32 (R, n) result buffer, any row stride >= n (what
    lies behind column n of a row is left alone); out_tokens: a static int32 (R,) one.  Runs the HIP kernel (mopk_language_probs:
    one launch, one workgroup per row) when language_probs_supported() accepts the call, else language_probs_torch();
    LAST_PATH["language_probs"] records which.  No host sync; bitwise reproducible."""
    _lp_check(logits, languages, out_probs, out_tokens, "language_probs")
    with torch.no_grad():
        a = _lp_accept(logits, languages, out_probs, out_tokens)
        if a is None:
            LAST_PATH["language_probs"] = L.PATH_GENERIC
            return language_probs_torch(logits, languages, out_probs, out_tokens)
        if out_probs is None:
            out_probs = torch.empty(a.R, a.n, dtype=torch.float32, device=logits.device)
            a.probs = out_probs.data_ptr()
        if out_tokens is None:
            out_tokens = torch.empty(a.R, dtype=torch.int32, device=logits.device)
            a.tokens = out_tokens.data_ptr()
        _row_launch(a, "mopk_language_probs", "language_probs")
        return LanguageProbs(out_probs, out_tokens)


class GreedyState:
    """Device state of a greedy decoding of B rows, updated in place by `greedy_pick` (no host sync, static buffers: a step can be
    captured in a graph).

    next_ids (B, 1) int32: the newest tokens (the next decoder step's ids); done (B,) int32: the row has emitted eos_token_id;
    sum_logprobs (B,) fp32: the sum of log_softmax(logits)[token] over the row's tokens up to and including its first eos;
    n_tokens (B,) int32: how many tokens that sum holds (sum_logprobs / n_tokens is Whisper's avg_logprob); hist (B, cap) int32
    with with_hist, else None: the token history, written at column pos by every pick (a caller fills the prompt's columns)."""

    def __init__(self, B: int, cap: int, eos_token_id: Optional[int] = None, with_hist: bool = False, device=None):
        if not _is_index(B) or not _is_index(cap) or B < 1 or cap < 1:
            raise ValueError(f"GreedyState: B and cap must be ints >= 1, got B = {B!r}, cap = {cap!r}")
        if eos_token_id is not None and (not _is_index(eos_token_id) or eos_token_id < 0):
            raise ValueError(f"GreedyState: eos_token_id must be None or an int >= 0, got {eos_token_id!r}")
        self.B, self.cap, self.eos = B, cap, eos_token_id
        i32 = dict(dtype=torch.int32, device=device)
        self.next_ids = torch.zeros(B, 1, **i32)
        self.done = torch.zeros(B, **i32)
        self.sum_logprobs = torch.zeros(B, dtype=torch.float32, device=device)
        self.n_tokens = torch.zeros(B, **i32)
        self.hist = torch.zeros(B, cap, **i32) if with_hist else None


def _gp_check(logits, state, pos, what: str) -> None:
    """validate a greedy_pick call before any device work"""
    if not isinstance(state, GreedyState):
        raise ValueError(f"{what}: state must be a GreedyState, got {type(state).__name__}")
    _stat_logits_check(logits, what)
    R, V = logits.shape
    if R != state.B:
        raise ValueError(f"{what}: {R} logit rows for a state of B = {state.B} rows")
    if state.eos is not None and state.eos >= V:
        raise ValueError(f"{what}: the state's eos_token_id = {state.eos} outside [0, V = {V})")
    if not isinstance(pos, torch.Tensor) or pos.numel() != 1 or pos.dtype.is_floating_point or pos.dtype == torch.bool:
        raise ValueError(f"{what}: pos must hold one integer, got "
                         f"{(tuple(pos.shape), pos.dtype) if isinstance(pos, torch.Tensor) else type(pos).__name__}")
    h = state.hist
    if h is not None:
        if h.dim() != 2 or h.shape[0] != R or h.dtype != torch.int32:
            raise ValueError(f"{what}: the state's hist must be an int32 ({R}, cap) tensor, got {tuple(h.shape)} {h.dtype}")
        if not pos.is_cuda and not 0 <= int(pos) < h.shape[1]:                        # a host value: the host can know
            raise ValueError(f"{what}: pos = {int(pos)} outside the history's columns [0, {h.shape[1]})")
    for name, t, dt, shape in (("next_ids", state.next_ids, torch.int32, (R, 1)), ("done", state.done, torch.int32, (R,)),
                               ("sum_logprobs", state.sum_logprobs, torch.float32, (R,)), ("n_tokens", state.n_tokens, torch.int32, (R,))):
        if tuple(t.shape) != shape or t.dtype != dt:
            raise ValueError(f"{what}: the state's {name} must be {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    for t in (pos, state.next_ids, state.done, state.sum_logprobs, state.n_tokens) + (() if h is None else (h,)):
        if t.device != logits.device:
            raise ValueError(f"{what}: pos and the state must be on the logits' device {logits.device}, found {t.device}")


def greedy_pick_torch(logits: torch.Tensor, state: GreedyState, pos: torch.Tensor) -> None:
    """the restatement of `greedy_pick` in torch ops (no host sync): log_softmax(logits.float(), -1), argmax, where"""
    _gp_check(logits, state, pos, "greedy_pick_torch")
    x = logits.float()
    lp = torch.log_softmax(x, -1)
    tok = x.argmax(-1)
    add = lp.gather(1, tok.unsqueeze(1)).squeeze(1)
    if state.eos is not None:
        live = state.done == 0
        tok = torch.where(live, tok, torch.full_like(tok, state.eos))
        add = torch.where(live, add, torch.zeros_like(add))
        state.n_tokens.add_(live.to(torch.int32))
        state.done.logical_or_(live & (tok == state.eos))
    else:
        state.n_tokens.add_(1)
    state.sum_logprobs.add_(add)
    state.next_ids.copy_(tok.unsqueeze(1))
    if state.hist is not None:
        cap = state.hist.shape[1]
        p = pos.reshape(1).to(torch.long)
        col = state.hist.index_select(1, p.clamp(0, cap - 1)).squeeze(1)
        inside = ((p >= 0) & (p < cap)).expand_as(col)
        state.hist.index_copy_(1, p.clamp(0, cap - 1), torch.where(inside, tok.to(torch.int32), col).unsqueeze(1))


def _gp_accept(logits, state, pos):
    """the args struct of a call that mopk_greedy_pick takes, None of one it refuses"""
    if not _stat_logits_ok(logits):
        return None
    if not pos.is_cuda or pos.dtype != torch.int32:
        return None
    if not all(t.is_cuda and t.is_contiguous() for t in (state.next_ids, state.done, state.sum_logprobs, state.n_tokens)):
        return None
    a = L.GreedyPickArgs()
    a.R, a.V = logits.shape
    a.dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.eos = -1 if state.eos is None else state.eos
    a.logits, a.logits_ld, a.pos = logits.data_ptr(), a.V if a.R == 1 else logits.stride(0), pos.data_ptr()
    a.next_ids, a.done = state.next_ids.data_ptr(), state.done.data_ptr()
    a.sum_logprobs, a.n_tokens = state.sum_logprobs.data_ptr(), state.n_tokens.data_ptr()
    h = state.hist
    if h is not None:
        cap = h.shape[1]
        if not h.is_cuda or (cap > 1 and h.stride(1) != 1) or (a.R > 1 and h.stride(0) < cap):
            return None
        a.hist, a.hist_cap, a.hist_ld = h.data_ptr(), cap, cap if a.R == 1 else h.stride(0)
    return a if L.lib().mopk_greedy_pick_supported(C.byref(a)) else None


def greedy_pick_supported(logits: torch.Tensor, state: GreedyState, pos: torch.Tensor) -> bool:
    """True if mopk_greedy_pick takes this call: CUDA fp32 / bf16 logits with unit inner stride and a row stride >= V (one row:
    any), an int32 device pos, a CUDA state whose hist (if any) has unit inner stride and a row stride >= cap (the library's own
    query decides the rest).  Raises ValueError on bad arguments."""
    _gp_check(logits, state, pos, "greedy_pick_supported")
    return _gp_accept(logits, state, pos) is not None


def greedy_pick(logits: torch.Tensor, state: GreedyState, pos: torch.Tensor) -> None:
    """one greedy decoding step (Whisper's GreedyDecoder.update): update `state` in place from the step's last-position logits.
    Inference only.

    logits: (B, V) fp32 or bf16, any row stride >= V.  pos: (1,) int32 device tensor, the history column of the new tokens (the
    decoder cache's length after the step that produced the logits; what `logit_rules` takes).  Per row r:
    - state.done[r] != 0 (and the state has an eos): the token is eos; sum_logprobs, n_tokens and done stay;
    - else the token is argmax logits[r], ties to the smaller index (torch.argmax); sum_logprobs[r] += float(logits[r, token]) -
      lse(logits[r]) in fp32; n_tokens[r] += 1; done[r] |= token == eos;
    - next_ids[r] = token, and hist[r, pos] = token when the state has a hist (pos outside its columns writes nothing).
    The first eos is counted in the sum and in the length, nothing behind it.  Runs the HIP kernel (mopk_greedy_pick: one launch)
    when greedy_pick_supported() accepts the call, else greedy_pick_torch(); LAST_PATH["greedy_pick"] records which.  No host
    sync; bitwise reproducible."""
    _gp_check(logits, state, pos, "greedy_pick")
    with torch.no_grad():
        a = _gp_accept(logits, state, pos)
        if a is None:
            LAST_PATH["greedy_pick"] = L.PATH_GENERIC
            return greedy_pick_torch(logits, state, pos)
        _row_launch(a, "mopk_greedy_pick", "greedy_pick")


# --------------------------------------------------------------------------------------
# Token-level timestamps (WhisperMoP.align_tokens): Whisper's alignment filter and its dynamic time warping
ALIGN_MAX_WIDTH = 9            # the filter kernel's odd median widths end here
ALIGN_MAX_ROWS = 1024          # rows of a map the filter kernel holds in LDS / rows of one DTW (one thread each)


def _lens_i32_check(t, B: int, dev, name: str, what: str, beside: str = "the map") -> None:
    if not isinstance(t, torch.Tensor) or t.shape != (B,) or t.dtype.is_floating_point or t.dtype in (torch.bool,) or t.dtype.is_complex:
        raise ValueError(f"{what}: {name} must be an integer ({B},) tensor, got "
                         f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.device != dev:
        raise ValueError(f"{what}: {name} is on {t.device}, {beside} on {dev}")


def _ac_check(probs, n_tokens, n_frames, medfilt_width, what: str) -> None:
    """validate an alignment_cost call before any device work"""
    if not isinstance(probs, torch.Tensor) or probs.dim() != 4 or probs.dtype != torch.float32 or 0 in probs.shape:
        raise ValueError(f"{what}: probs must be a non-empty fp32 (B, S, N, M) tensor, got "
                         f"{(tuple(probs.shape), probs.dtype) if isinstance(probs, torch.Tensor) else type(probs).__name__}")
    if probs.shape[3] > 1 and probs.stride(3) != 1:
        raise ValueError(f"{what}: probs must have a unit inner stride, got strides {probs.stride()}")
    if isinstance(medfilt_width, bool) or int(medfilt_width) != medfilt_width or medfilt_width < 1 or medfilt_width % 2 == 0:
        raise ValueError(f"{what}: medfilt_width must be a positive odd integer, got {medfilt_width}")
    _lens_i32_check(n_tokens, probs.shape[0], probs.device, "n_tokens", what)
    _lens_i32_check(n_frames, probs.shape[0], probs.device, "n_frames", what)


def alignment_cost_torch(probs: torch.Tensor, n_tokens: torch.Tensor, n_frames: torch.Tensor, medfilt_width: int = 7) -> torch.Tensor:
    """the restatement of `alignment_cost` in torch ops (CPU or GPU, vectorised over the batch, no host sync): per head, mean and
    population standard deviation over the item's rows (torch.where keeps everything outside the window out of them), z, a gather
    of the reflect-padded windows, sort, the middle element; the heads are added in index order"""
    _ac_check(probs, n_tokens, n_frames, medfilt_width, "alignment_cost_torch")
    B, S, N, M = probs.shape
    dev, h = probs.device, int(medfilt_width) // 2
    nt = n_tokens.to(torch.long).clamp(0, N)
    nf = n_frames.to(torch.long).clamp(0, M)
    rows = (torch.arange(N, device=dev).unsqueeze(0) < nt.unsqueeze(1)).unsqueeze(2)           # (B, N, 1)
    cnt = nt.to(torch.float32).view(B, 1, 1)
    src = torch.arange(M, device=dev).view(1, M, 1) + torch.arange(-h, h + 1, device=dev).view(1, 1, -1)   # (1, M, width)
    last = (nf - 1).view(B, 1, 1)
    src = torch.where(src < 0, -src, src)
    src = torch.where(src > last, 2 * last - src, src).clamp(0, M - 1)                         # columns >= nf: anything inside
    filt = (nf > h).view(B, 1, 1)
    total = torch.zeros(B, N, M, dtype=torch.float32, device=dev)
    for s in range(S):
        p = probs[:, s]
        mu = torch.where(rows, p, 0.0).sum(1, keepdim=True) / cnt
        d = torch.where(rows, p - mu, 0.0)
        sd = ((d * d).sum(1, keepdim=True) / cnt).sqrt()
        z = (p - mu) / sd
        if h > 0:
            win = torch.stack([z.gather(2, src[:, :, e].unsqueeze(1).expand(B, N, M)) for e in range(2 * h + 1)], dim=3)
            z = torch.where(filt, win.sort(dim=3).values[..., h], z)
        total = total + z
    return -(total / S)


def _ac_args(probs, n_tokens, n_frames, medfilt_width) -> L.AlignCostArgs:
    a = L.AlignCostArgs()
    a.B, a.S, a.N, a.M = probs.shape
    a.width, a.reserved = int(medfilt_width), 0
    a.probs, a.probs_sb, a.probs_ss, a.probs_sn = probs.data_ptr(), probs.stride(0), probs.stride(1), probs.stride(2)
    a.n_tokens, a.n_frames = n_tokens.data_ptr(), n_frames.data_ptr()
    a.cost_sb, a.cost_ld = a.N * a.M, a.M
    return a


def _ac_accept(probs, n_tokens, n_frames, medfilt_width):
    """the args struct of a call that mopk_alignment_cost takes, None of one it refuses; a.cost holds a stand-in"""
    if not probs.is_cuda or n_tokens.dtype != torch.int32 or n_frames.dtype != torch.int32:
        return None
    if medfilt_width > ALIGN_MAX_WIDTH or probs.shape[2] > ALIGN_MAX_ROWS:
        return None
    a = _ac_args(probs, n_tokens, n_frames, medfilt_width)
    a.cost = a.probs                                                               # a stand-in: only its alignment is looked at
    return a if L.lib().mopk_alignment_cost_supported(C.byref(a)) else None


def alignment_cost_supported(probs: torch.Tensor, n_tokens: torch.Tensor, n_frames: torch.Tensor, medfilt_width: int = 7) -> bool:
    """True if mopk_alignment_cost takes this call: CUDA tensors, int32 lengths, an odd width <= 9 and N <= 1024 (the library's own
    query decides the rest).  Raises ValueError on bad arguments."""
    _ac_check(probs, n_tokens, n_frames, medfilt_width, "alignment_cost_supported")
    return _ac_accept(probs, n_tokens, n_frames, medfilt_width) is not None


def alignment_cost(probs: torch.Tensor, n_tokens: torch.Tensor, n_frames: torch.Tensor, medfilt_width: int = 7) -> torch.Tensor:
    """Whisper's alignment filter (timing.py, find_alignment) -> cost (B, N, M) fp32, the input of `dtw_align`.  Inference only.

    probs: (B, S, N, M) fp32 cross-attention probabilities of S heads, rows are tokens and columns audio frames; unit inner stride,
    the other strides are free.  n_tokens, n_frames: int32 (B,) device tensors, clamped into [0, N] and [0, M]: item b uses the rows
    i < n_tokens[b] and the columns j < n_frames[b] only, nothing outside them is read (NaN there does not matter).  Per item, head
    and column: mu and the population standard deviation sd over the item's rows (two passes), z = (p - mu) / sd (no guard for
    sd = 0, as in Whisper); z is median-filtered along the columns with window medfilt_width, reflect-padded by medfilt_width // 2
    inside the item's own n_frames[b] columns (skipped when n_frames[b] <= medfilt_width // 2, as in Whisper);
    cost[b, i, j] = -mean over the heads, added in index order.  Entries outside the item's window are unspecified.
    Runs the HIP kernel (mopk_alignment_cost: one launch) when alignment_cost_supported() accepts the call, else
    alignment_cost_torch(); LAST_PATH["alignment_cost"] records which.  No host sync; bitwise reproducible."""
    _ac_check(probs, n_tokens, n_frames, medfilt_width, "alignment_cost")
    with torch.no_grad():
        a = _ac_accept(probs, n_tokens, n_frames, medfilt_width)
        if a is None:
            LAST_PATH["alignment_cost"] = L.PATH_GENERIC
            return alignment_cost_torch(probs, n_tokens, n_frames, medfilt_width)
        cost = torch.empty(a.B, a.N, a.M, dtype=torch.float32, device=probs.device)
        a.cost = cost.data_ptr()                                                   # in place of the stand-in
        _row_launch(a, "mopk_alignment_cost", "alignment_cost")
        return cost


def _dtw_check(cost, n_rows, n_cols, row0, what: str) -> None:
    """validate a dtw_align call before any device work"""
    if not isinstance(cost, torch.Tensor) or cost.dim() != 3 or cost.dtype != torch.float32 or 0 in cost.shape:
        raise ValueError(f"{what}: cost must be a non-empty fp32 (B, N, M) tensor, got "
                         f"{(tuple(cost.shape), cost.dtype) if isinstance(cost, torch.Tensor) else type(cost).__name__}")
    if cost.shape[2] > 1 and cost.stride(2) != 1:
        raise ValueError(f"{what}: cost must have a unit inner stride, got strides {cost.stride()}")
    if isinstance(row0, bool) or int(row0) != row0 or not 0 <= row0 < cost.shape[1]:
        raise ValueError(f"{what}: row0 must be an integer in [0, N = {cost.shape[1]}), got {row0}")
    _lens_i32_check(n_rows, cost.shape[0], cost.device, "n_rows", what)
    _lens_i32_check(n_cols, cost.shape[0], cost.device, "n_cols", what)


def dtw_align_torch(cost: torch.Tensor, n_rows: torch.Tensor, n_cols: torch.Tensor, row0: int = 0):
    """the restatement of `dtw_align` in torch ops (CPU or GPU, vectorised over the batch, no host sync): one step per
    anti-diagonal over the whole (N - row0, M) rectangle (a cell depends on smaller indices only, so every item's window comes out
    as it would alone), then one step per cell of the longest possible path for the walk back"""
    _dtw_check(cost, n_rows, n_cols, row0, "dtw_align_torch")
    B, N, M = cost.shape
    dev, row0 = cost.device, int(row0)
    R = N - row0
    inf = float("inf")
    D = torch.full((B, R + 1, M + 1), inf, dtype=torch.float32, device=dev)
    D[:, 0, 0] = 0.0
    trace = torch.full((B, R, M), 2, dtype=torch.int8, device=dev)
    x = cost[:, row0:]
    for d in range(R + M - 1):
        i = torch.arange(max(0, d - M + 1), min(R - 1, d) + 1, device=dev)
        j = d - i
        c0, c1, c2 = D[:, i, j], D[:, i, j + 1], D[:, i + 1, j]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        c = torch.where(diag, c0, torch.where(up, c1, c2))
        D[:, i + 1, j + 1] = x[:, i, j] + c
        trace[:, i, j] = torch.where(diag, 0, torch.where(up, 1, 2)).to(torch.int8)
    nr = n_rows.to(torch.long).clamp(0, N) - row0
    nc = n_cols.to(torch.long).clamp(0, M)
    live = (nr > 0) & (nc > 0)
    i, j = (nr - 1).clamp_min(0), (nc - 1).clamp_min(0)
    starts = torch.full((B, R), -1, dtype=torch.long, device=dev)
    ends = torch.full((B, R), -1, dtype=torch.long, device=dev)
    bi = torch.arange(B, device=dev)
    for _ in range(R + M - 1):
        cur_s, cur_e = starts[bi, i], ends[bi, i]
        ends[bi, i] = torch.where(live & (cur_e < 0), j, cur_e)
        starts[bi, i] = torch.where(live, j, cur_s)
        code = trace[bi, i, j].to(torch.long)
        code = torch.where(i == 0, 2, torch.where(j == 0, 1, code))               # the first row goes left, the first column up
        live = live & ((i > 0) | (j > 0))
        i = torch.where(live & (code != 2), i - 1, i)
        j = torch.where(live & (code != 1), j - 1, j)
    out_s = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    out_e = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    out_s[:, row0:] = starts.to(torch.int32)
    out_e[:, row0:] = ends.to(torch.int32)
    return out_s, out_e


def _dtw_args(cost, n_rows, n_cols, row0) -> L.DtwArgs:
    a = L.DtwArgs()
    a.B, a.N, a.M = cost.shape
    a.row0 = int(row0)
    a.cost, a.cost_sb, a.cost_ld = cost.data_ptr(), cost.stride(0), cost.stride(1)
    if a.N == 1:                                                                   # a single row: its stride is never used
        a.cost_ld = a.M
    if a.B == 1:                                                                   # a single item: its stride is never used
        a.cost_sb = a.N * a.cost_ld
    a.n_rows, a.n_cols = n_rows.data_ptr(), n_cols.data_ptr()
    return a


def dtw_workspace_bytes(B: int, N: int, M: int, row0: int = 0) -> int:
    """bytes of step codes one dtw_align call of this shape allocates (mopk_dtw_workspace_bytes; needs no GPU)"""
    a = L.DtwArgs()
    a.B, a.N, a.M, a.row0 = int(B), int(N), int(M), int(row0)
    return int(L.lib().mopk_dtw_workspace_bytes(C.byref(a)))


def _dtw_accept(cost, n_rows, n_cols, row0):
    """the args struct of a call that mopk_dtw_align takes, None of one it refuses; a.starts and a.ends hold stand-ins"""
    if not cost.is_cuda or n_rows.dtype != torch.int32 or n_cols.dtype != torch.int32:
        return None
    B, N, M = cost.shape
    if N - row0 > ALIGN_MAX_ROWS or (N > 1 and cost.stride(1) < M):
        return None
    a = _dtw_args(cost, n_rows, n_cols, row0)
    a.starts = a.ends = a.n_rows                                                   # stand-ins: only their alignment is looked at
    return a if L.lib().mopk_dtw_align_supported(C.byref(a)) else None


def dtw_align_supported(cost: torch.Tensor, n_rows: torch.Tensor, n_cols: torch.Tensor, row0: int = 0) -> bool:
    """True if mopk_dtw_align takes this call: CUDA tensors, int32 lengths, a row stride >= M, item stride >= 0 and
    N - row0 <= 1024 rows (the library's own query decides the rest).  Raises ValueError on bad arguments."""
    _dtw_check(cost, n_rows, n_cols, row0, "dtw_align_supported")
    return _dtw_accept(cost, n_rows, n_cols, row0) is not None


def dtw_align(cost: torch.Tensor, n_rows: torch.Tensor, n_cols: torch.Tensor, row0: int = 0):
    """Whisper's dynamic time warping (timing.py, dtw_cpu) with the walk back on the device -> (starts, ends), both (B, N) int32.
    Inference only.

    cost: (B, N, M) fp32, unit inner stride.  n_rows, n_cols: int32 (B,) device tensors, clamped into [0, N] and [0, M]: item b's
    DTW runs over the rows [row0, n_rows[b]) and the columns [0, n_cols[b]); nothing outside them is read.  Whisper's rules
    exactly, with one fp32 add per cell (1-based, a +inf border, D[0,0] = 0): c0 = D[i-1,j-1], c1 = D[i-1,j], c2 = D[i,j-1];
    c0 < c1 and c0 < c2: the diagonal; else c1 < c0 and c1 < c2: up; else left; D[i,j] = x[i-1,j-1] + c.  The path is walked back
    from the last cell; starts[b, i] / ends[b, i] are its first and last column in row i, so starts[i+1] is ends[i] or
    ends[i] + 1, the first row starts at column 0 and the last row ends at n_cols[b] - 1.  Rows outside the range get -1, and so do
    all rows of an item with no rows or no columns.
    Runs the HIP kernel (mopk_dtw_align: one launch, one workspace of a step code per cell) when dtw_align_supported() accepts the
    call, else dtw_align_torch(); LAST_PATH["dtw_align"] records which.  No host sync, no device-to-host copy."""
    _dtw_check(cost, n_rows, n_cols, row0, "dtw_align")
    with torch.no_grad():
        a = _dtw_accept(cost, n_rows, n_cols, row0)
        if a is None:
            LAST_PATH["dtw_align"] = L.PATH_GENERIC
            return dtw_align_torch(cost, n_rows, n_cols, row0)
        starts = torch.empty(a.B, a.N, dtype=torch.int32, device=cost.device)
        ends = torch.empty(a.B, a.N, dtype=torch.int32, device=cost.device)
        a.starts, a.ends = starts.data_ptr(), ends.data_ptr()                      # in place of the stand-ins
        _row_launch(a, "mopk_dtw_align", "dtw_align", cost.device, "mopk_dtw_workspace_bytes")
        return starts, ends


# --------------------------------------------------------------------------------------
# Long-form transcription (WhisperMoP.transcribe): Whisper's segment and seek arithmetic on decoded token rows
SEGMENTS_MAX_COLS = 1024       # generated columns of a row (one thread each)


class TimestampSegments(NamedTuple):
    """the segments of a batch of decoded windows (`timestamp_segments`), all int32 on the tokens' device.
    starts / ends (R, S): the segments' first and last frame, relative to the window start; tok_begin / tok_end (R, S): the columns
    of `tokens` a segment spans, the end exclusive; all -1 at j >= n_segments[r].  n_segments (R,).  advance (R,): how far the
    next window moves, in [1, max(window[r], 1)]."""
    starts: torch.Tensor
    ends: torch.Tensor
    tok_begin: torch.Tensor
    tok_end: torch.Tensor
    n_segments: torch.Tensor
    advance: torch.Tensor


def _ts_check(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp, what: str) -> None:
    """validate a timestamp_segments call before any device work"""
    def _is_int(x):
        return not isinstance(x, bool) and isinstance(x, int)

    if (not isinstance(tokens, torch.Tensor) or tokens.dim() != 2 or 0 in tokens.shape or tokens.dtype.is_floating_point
            or tokens.dtype.is_complex or tokens.dtype == torch.bool):
        raise ValueError(f"{what}: tokens must be a non-empty integer (R, T) tensor, got "
                         f"{(tuple(tokens.shape), tokens.dtype) if isinstance(tokens, torch.Tensor) else type(tokens).__name__}")
    if not _is_int(t0) or not 0 <= t0 < tokens.shape[1]:
        raise ValueError(f"{what}: t0 must be an int in [0, T = {tokens.shape[1]}), got {t0!r}")
    _lens_i32_check(window, tokens.shape[0], tokens.device, "window", what, "the tokens")
    if not _is_int(timestamp_begin) or not _is_int(eos_token_id) or not 0 <= eos_token_id < timestamp_begin < 2 ** 31:
        raise ValueError(f"{what}: needs ints 0 <= eos_token_id < timestamp_begin < 2^31, got eos_token_id = {eos_token_id!r}, "
                         f"timestamp_begin = {timestamp_begin!r}")
    if not _is_int(frames_per_timestamp) or not 1 <= frames_per_timestamp < 2 ** 31:
        raise ValueError(f"{what}: frames_per_timestamp must be an int >= 1, got {frames_per_timestamp!r}")


def timestamp_segments_torch(tokens: torch.Tensor, t0: int, window: torch.Tensor, timestamp_begin: int, eos_token_id: int,
                             frames_per_timestamp: int = 1) -> TimestampSegments:
    """the restatement of `timestamp_segments` in torch ops (CPU or GPU, vectorised over rows, no host sync): the flags per
    column, a cumulative sum that numbers the cuts, and scatters into buffers with one spare column that takes every write of a
    column that has none to make"""
    _ts_check(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp, "timestamp_segments_torch")
    R, T = tokens.shape
    dev, S, tb, f = tokens.device, T - t0, timestamp_begin, frames_per_timestamp
    g = tokens[:, t0:].to(torch.long)
    j = torch.arange(S, device=dev).unsqueeze(0)
    w = window.to(torch.long).clamp_min(1)
    n = torch.where(g == eos_token_id, j, S).min(1).values
    ts = (j < n.unsqueeze(1)) & (g >= tb)
    cut = torch.zeros_like(ts)
    cut[:, 1:] = ts[:, 1:] & ts[:, :-1]
    at = lambda i: g.gather(1, i.clamp(0, S - 1).unsqueeze(1)).squeeze(1)          # noqa: E731  g[r, i[r]]
    frame = lambda x: ((x - tb) * f).to(torch.int32).to(torch.long)                # noqa: E731  the product in 32 bits
    single_end = (n >= 2) & (at(n - 2) < tb) & (at(n - 1) >= tb)                   # rule 2
    nC = cut.sum(1)
    has = nC > 0
    nseg = torch.where(has, nC + single_end, (n > 0).long())
    rank = cut.cumsum(1) - cut.long()                                              # the exclusive scan: cut c closes segment rank
    col = (t0 + j).expand(R, S)
    starts, ends, tok_begin, tok_end = (torch.full((R, S + 1), -1, dtype=torch.long, device=dev) for _ in range(4))
    prev = F.pad(g, (1, 0))[:, :S]
    close = torch.where(cut, rank, S)                                              # rule 4: a cut closes its segment ...
    ends.scatter_(1, close, frame(prev))
    tok_end.scatter_(1, close, col)
    opens = torch.where(cut & (rank + 1 < nseg.unsqueeze(1)), rank + 1, S)         # ... and opens the next one, if there is one
    starts.scatter_(1, opens, frame(g))
    tok_begin.scatter_(1, opens, col)
    some = nseg > 0
    starts[:, 0] = torch.where(some, torch.where(has & ts[:, 0], frame(g[:, 0]), 0), -1)
    tok_begin[:, 0] = torch.where(some, t0, -1)
    tail = torch.where(has & single_end, nC, S).unsqueeze(1)                       # the cut at n
    ends.scatter_(1, tail, frame(at(n - 1)).unsqueeze(1))
    tok_end.scatter_(1, tail, (t0 + n).unsqueeze(1))
    li = torch.where(ts, j, -1).max(1).values                                      # rule 5: the last timestamp
    s = at(li)
    one = ~has & some
    ends[:, 0] = torch.where(one, torch.where((li >= 0) & (s != tb), frame(s), w), ends[:, 0])
    tok_end[:, 0] = torch.where(one, t0 + n, tok_end[:, 0])
    max_c = torch.where(cut, j, -1).max(1).values
    adv = torch.where(has & ~single_end, frame(at(max_c - 1)), w)
    adv = torch.minimum(adv.clamp_min(1), w)                                       # rule 6
    i32 = lambda t: t.to(torch.int32)                                              # noqa: E731
    return TimestampSegments(i32(starts[:, :S]), i32(ends[:, :S]), i32(tok_begin[:, :S]), i32(tok_end[:, :S]), i32(nseg), i32(adv))


def _ts_args(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp) -> L.TimestampSegmentsArgs:
    a = L.TimestampSegmentsArgs()
    a.R, a.T = tokens.shape
    a.T0, a.tb, a.eos, a.f = t0, timestamp_begin, eos_token_id, frames_per_timestamp
    a.tokens, a.tokens_ld, a.window = tokens.data_ptr(), tokens.stride(0), window.data_ptr()
    if a.R == 1:                                                                   # a single row: its stride is never used
        a.tokens_ld = a.T
    return a


def _ts_accept(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp):
    """the args struct of a call that mopk_timestamp_segments takes, None of one it refuses; the outputs hold stand-ins"""
    R, T = tokens.shape
    if not tokens.is_cuda or tokens.dtype != torch.int32 or (T > 1 and tokens.stride(1) != 1) or (R > 1 and tokens.stride(0) < T):
        return None
    if window.dtype != torch.int32 or (R > 1 and window.stride(0) != 1) or T - t0 > SEGMENTS_MAX_COLS:
        return None
    a = _ts_args(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp)
    a.starts = a.ends = a.tok_begin = a.tok_end = a.n_segments = a.advance = a.window  # stand-ins: only their alignment is looked at
    return a if L.lib().mopk_timestamp_segments_supported(C.byref(a)) else None


def timestamp_segments_supported(tokens: torch.Tensor, t0: int, window: torch.Tensor, timestamp_begin: int, eos_token_id: int,
                                 frames_per_timestamp: int = 1) -> bool:
    """True if mopk_timestamp_segments takes this call: CUDA int32 tokens with unit inner stride and a row stride >= T (one row:
    any), a contiguous int32 window, T - t0 <= 1024 (the library's own query decides the rest).  Raises ValueError on bad
    arguments."""
    _ts_check(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp, "timestamp_segments_supported")
    return _ts_accept(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp) is not None


def timestamp_segments(tokens: torch.Tensor, t0: int, window: torch.Tensor, timestamp_begin: int, eos_token_id: int,
                       frames_per_timestamp: int = 1) -> TimestampSegments:
    """Whisper's segment and seek arithmetic (transcribe.py) for a batch of decoded windows -> TimestampSegments(starts, ends,
    tok_begin, tok_end, n_segments, advance), all int32 on the tokens' device.  Inference only.

    tokens: (R, T) int32 decoder outputs, the prompt in front; unit inner stride, any row stride >= T (one row: any).  t0: the
    first generated column (the same for every row: ragged prompts are left-padded).  window: (R,) int32 device tensor, the frames
    of row r's window, used as w = max(window[r], 1).  tb = timestamp_begin, eos = eos_token_id, 0 <= eos < tb: a token is a
    timestamp when its id is >= tb, and tb + i means frame i * f of the window, f = frames_per_timestamp (this model has no
    convolutional stem: a frame is a mel frame; OpenAI's 20 ms timestamps over 10 ms frames are f = 2).  Per row, e = the first
    column >= t0 that holds eos (T if none), g = tokens[r, t0:e] are its n = e - t0 tokens, ts[i] = g[i] >= tb, and:
    1. n == 0: no segment; advance = w;
    2. single_end = n >= 2 and not ts[n-2] and ts[n-1];
    3. C = the i in [1, n) with ts[i-1] and ts[i], ascending;
    4. C not empty: the cuts are C, then n if single_end; with p the cut before (0 at first), cut c makes the segment of the
       columns tok_begin = t0 + p, tok_end = t0 + c (exclusive), start = (g[p] - tb) * f (0 when g[p] is no timestamp: p = 0 only,
       and never under the logit rules), end = (g[c-1] - tb) * f; advance = w if single_end, else (g[max C - 1] - tb) * f; the
       tokens after the last cut are in no segment (the next window decodes them again);
    5. C empty: one segment [t0, t0 + n), start = 0, end = w, or (s - tb) * f when a timestamp exists and the last one, s, is not
       tb itself; advance = w;
    6. advance is clamped into [1, w].
    Three deviations from Whisper: rule 6 (Whisper has neither clamp; the lower one keeps a loop moving, the upper one guards
    against a timestamp beyond the window, and under the logit rules only the upper one can act), the start = 0 of rule 4, and
    rule 1 (Whisper adds an empty segment there and drops it later).  starts / ends / tok_begin / tok_end are (R, T - t0) with
    -1 at j >= n_segments[r]; the products are taken in 32 bits.
    Runs the HIP kernel (mopk_timestamp_segments: one launch, the -1 tail included) when timestamp_segments_supported() accepts
    the call, else timestamp_segments_torch(); LAST_PATH["timestamp_segments"] records which.  No host sync, no workspace;
    bitwise reproducible."""
    _ts_check(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp, "timestamp_segments")
    with torch.no_grad():
        a = _ts_accept(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp)
        if a is None:
            LAST_PATH["timestamp_segments"] = L.PATH_GENERIC
            return timestamp_segments_torch(tokens, t0, window, timestamp_begin, eos_token_id, frames_per_timestamp)
        seg = torch.empty(4, a.R, a.T - a.T0, dtype=torch.int32, device=tokens.device)
        row = torch.empty(2, a.R, dtype=torch.int32, device=tokens.device)
        a.starts, a.ends, a.tok_begin, a.tok_end = (seg[k].data_ptr() for k in range(4))        # in place of the stand-ins
        a.n_segments, a.advance = row[0].data_ptr(), row[1].data_ptr()
        _row_launch(a, "mopk_timestamp_segments", "timestamp_segments")
        return TimestampSegments(seg[0], seg[1], seg[2], seg[3], row[0], row[1])


# --------------------------------------------------------------------------------------
# Conditioning on the previous text (WhisperMoP.transcribe): the per-clip token history on the device, and the prompts built from it
PROMPT_HISTORY_MAX = 1024      # history entries of a clip (one thread each), and generated columns of a row
WINDOW_PROMPTS_MAX_WIDTH = 2048


class WindowPrompts(NamedTuple):
    """the prompts of a set of windows (`window_prompts`): ids (A, width), left-padded with zeros, and kv_start (A,) int32, the
    first column of each row's own prompt (what WhisperDecodeCache.kv_start takes)"""
    ids: torch.Tensor
    kv_start: torch.Tensor


def _is_int(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, int)


def _hist_state_check(hist, hist_len, what: str) -> None:
    if not isinstance(hist, torch.Tensor) or hist.dim() != 2 or 0 in hist.shape or hist.dtype != torch.int32 or not hist.is_contiguous():
        raise ValueError(f"{what}: hist must be a non-empty contiguous int32 (B, n) tensor, got "
                         f"{(tuple(hist.shape), hist.dtype, hist.stride()) if isinstance(hist, torch.Tensor) else type(hist).__name__}")
    B = hist.shape[0]
    if (not isinstance(hist_len, torch.Tensor) or hist_len.shape != (B,) or hist_len.dtype != torch.int32
            or not hist_len.is_contiguous()):
        raise ValueError(f"{what}: hist_len must be a contiguous int32 ({B},) tensor, got "
                         f"{(tuple(hist_len.shape), hist_len.dtype) if isinstance(hist_len, torch.Tensor) else type(hist_len).__name__}")
    if hist_len.device != hist.device:
        raise ValueError(f"{what}: hist_len is on {hist_len.device}, hist on {hist.device}")


def _ph_check(hist, hist_len, tokens, t0, n_take, item, mode, what: str) -> None:
    """validate a prompt_history_update call before any device work"""
    _hist_state_check(hist, hist_len, what)
    if (not isinstance(tokens, torch.Tensor) or tokens.dim() != 2 or 0 in tokens.shape or tokens.dtype.is_floating_point
            or tokens.dtype.is_complex or tokens.dtype == torch.bool):
        raise ValueError(f"{what}: tokens must be a non-empty integer (A, T) tensor, got "
                         f"{(tuple(tokens.shape), tokens.dtype) if isinstance(tokens, torch.Tensor) else type(tokens).__name__}")
    if tokens.device != hist.device:
        raise ValueError(f"{what}: tokens are on {tokens.device}, hist on {hist.device}")
    if not _is_int(t0) or not 0 <= t0 < tokens.shape[1]:
        raise ValueError(f"{what}: t0 must be an int in [0, T = {tokens.shape[1]}), got {t0!r}")
    for name, t in (("n_take", n_take), ("item", item), ("mode", mode)):
        _lens_i32_check(t, tokens.shape[0], hist.device, name, what, "hist")


def _item_lookup(item: torch.Tensor, B: int):
    """per clip b: whether a row a has item[a] == b, and the first such row"""
    match = item.to(torch.long).unsqueeze(0) == torch.arange(B, device=item.device).unsqueeze(1)         # (B, A)
    return match.any(1), match.to(torch.int32).argmax(1)


def prompt_history_update_torch(hist: torch.Tensor, hist_len: torch.Tensor, tokens: torch.Tensor, t0: int, n_take: torch.Tensor,
                                item: torch.Tensor, mode: torch.Tensor) -> None:
    """the restatement of `prompt_history_update` in torch ops (CPU or GPU, no host sync): every clip looks up the row that names
    it, gathers its new history from (hist, tokens) and keeps its old one where no row, or a row of another mode, does"""
    _ph_check(hist, hist_len, tokens, t0, n_take, item, mode, "prompt_history_update_torch")
    (B, n), S = hist.shape, tokens.shape[1] - t0
    has, a = _item_lookup(item, B)
    md = torch.where(has, mode.to(torch.long)[a], 2)
    L = hist_len.to(torch.long).clamp(0, n)
    m = n_take.to(torch.long)[a].clamp(0, S)
    keep = (L + m).clamp_max(n)
    j = torch.arange(n, device=hist.device).unsqueeze(0)
    src = (L + m - keep).unsqueeze(1) + j                                          # entry j of the last keep of (hist, tokens)
    old = hist.gather(1, src.clamp(0, n - 1))
    new = tokens[:, t0:].to(torch.int32)[a].gather(1, (src - L.unsqueeze(1)).clamp(0, S - 1))
    write = (j < keep.unsqueeze(1)) & (md == 0).unsqueeze(1)
    hist.copy_(torch.where(write, torch.where(src < L.unsqueeze(1), old, new), hist))
    hist_len.copy_(torch.where(md == 0, keep, torch.where(md == 1, 0, hist_len.to(torch.long))).to(torch.int32))


def _ph_accept(hist, hist_len, tokens, t0, n_take, item, mode):
    """the args struct of a call that mopk_prompt_history_update takes, None of one it refuses"""
    A, T = tokens.shape
    if not hist.is_cuda or tokens.dtype != torch.int32 or (T > 1 and tokens.stride(1) != 1) or (A > 1 and tokens.stride(0) < T):
        return None
    if any(t.dtype != torch.int32 or (A > 1 and t.stride(0) != 1) for t in (n_take, item, mode)):
        return None
    if hist.shape[1] > PROMPT_HISTORY_MAX or T - t0 > PROMPT_HISTORY_MAX:
        return None
    a = L.PromptHistoryArgs()
    a.A, a.T, a.T0 = A, T, t0
    a.B, a.n = hist.shape
    a.hist, a.hist_len, a.tokens, a.tokens_ld = hist.data_ptr(), hist_len.data_ptr(), tokens.data_ptr(), tokens.stride(0)
    if A == 1:                                                                     # a single row: its stride is never used
        a.tokens_ld = T
    a.n_take, a.item, a.mode = n_take.data_ptr(), item.data_ptr(), mode.data_ptr()
    return a if L.lib().mopk_prompt_history_update_supported(C.byref(a)) else None


def prompt_history_update_supported(hist: torch.Tensor, hist_len: torch.Tensor, tokens: torch.Tensor, t0: int,
                                    n_take: torch.Tensor, item: torch.Tensor, mode: torch.Tensor) -> bool:
    """True if mopk_prompt_history_update takes this call: CUDA tensors, int32 tokens with unit inner stride and a row stride >= T
    (one row: any), contiguous int32 n_take / item / mode, n <= 1024 and T - t0 <= 1024 (the library's own query decides the
    rest).  Raises ValueError on bad arguments."""
    _ph_check(hist, hist_len, tokens, t0, n_take, item, mode, "prompt_history_update_supported")
    return _ph_accept(hist, hist_len, tokens, t0, n_take, item, mode) is not None


def prompt_history_update(hist: torch.Tensor, hist_len: torch.Tensor, tokens: torch.Tensor, t0: int, n_take: torch.Tensor,
                          item: torch.Tensor, mode: torch.Tensor) -> None:
    """add the tokens a set of decoded windows contributes to their clips' token histories, or clear them, IN PLACE (Whisper's
    all_tokens[prompt_reset_since:], capped: what conditions the next window).  Inference only.

    hist (B, n) int32 contiguous and hist_len (B,) int32: hist[b, :hist_len[b]] holds the last tokens of clip b's transcript since
    its last reset; n is the cap.  tokens: (A, T) int32 decoded rows, unit inner stride, any row stride >= T; t0: the first
    generated column.  n_take, item, mode: (A,) int32 device tensors.  Per row a, with b = item[a], L = hist_len[b] clamped into
    [0, n] and m = n_take[a] clamped into [0, T - t0]:
    mode[a] == 0: c = hist[b, :L] followed by tokens[a, t0:t0+m]; keep = min(n, L + m); hist[b, :keep] = the last keep entries of
                  c; hist_len[b] = keep (hist[b, keep:] keeps its old words);
    mode[a] == 1: hist_len[b] = 0;
    any other value: clip b is left untouched.
    A row whose item lies outside [0, B) is skipped.  The item values of a call must be distinct: two rows of one clip race in the
    kernel (inside the buffers), and the torch path lets the first one win.
    Runs the HIP kernel (mopk_prompt_history_update: one launch, one workgroup per row, the entries held in registers across a
    barrier) when prompt_history_update_supported() accepts the call, else prompt_history_update_torch();
    LAST_PATH["prompt_history_update"] records which.  No host sync, no workspace; bitwise reproducible."""
    _ph_check(hist, hist_len, tokens, t0, n_take, item, mode, "prompt_history_update")
    with torch.no_grad():
        a = _ph_accept(hist, hist_len, tokens, t0, n_take, item, mode)
        if a is None:
            LAST_PATH["prompt_history_update"] = L.PATH_GENERIC
            return prompt_history_update_torch(hist, hist_len, tokens, t0, n_take, item, mode)
        _row_launch(a, "mopk_prompt_history_update", "prompt_history_update")


def _wp_check(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype, what: str) -> None:
    """validate a window_prompts call before any device work"""
    _hist_state_check(hist, hist_len, what)
    B = hist.shape[0]
    if (not isinstance(item, torch.Tensor) or item.dim() != 1 or item.numel() == 0 or item.dtype.is_floating_point
            or item.dtype.is_complex or item.dtype == torch.bool):
        raise ValueError(f"{what}: item must be a non-empty integer (A,) tensor, got "
                         f"{(tuple(item.shape), item.dtype) if isinstance(item, torch.Tensor) else type(item).__name__}")
    if (not isinstance(sot, torch.Tensor) or sot.dim() not in (1, 2) or 0 in sot.shape or sot.dtype.is_floating_point
            or sot.dtype.is_complex or sot.dtype == torch.bool or (sot.dim() == 2 and sot.shape[0] != B)):
        raise ValueError(f"{what}: sot must be an integer (T_s,) or ({B}, T_s) tensor, got "
                         f"{(tuple(sot.shape), sot.dtype) if isinstance(sot, torch.Tensor) else type(sot).__name__}")
    for name, t in (("item", item), ("sot", sot)):
        if t.device != hist.device:
            raise ValueError(f"{what}: {name} is on {t.device}, hist on {hist.device}")
    if not _is_int(sot_prev_token_id) or not 0 <= sot_prev_token_id < 2 ** 31:
        raise ValueError(f"{what}: sot_prev_token_id must be an int in [0, 2^31), got {sot_prev_token_id!r}")
    if not _is_int(width) or width < sot.shape[-1]:
        raise ValueError(f"{what}: width must be an int >= T_s = {sot.shape[-1]}, got {width!r}")
    if out_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: out_dtype must be torch.int32 or torch.int64, got {out_dtype!r}")


def window_prompts_torch(hist: torch.Tensor, hist_len: torch.Tensor, item: torch.Tensor, sot: torch.Tensor,
                         sot_prev_token_id: int, width: int, out_dtype: torch.dtype = torch.int64) -> WindowPrompts:
    """the restatement of `window_prompts` in torch ops (CPU or GPU, vectorised over rows, no host sync): every column finds its
    place relative to the row's first own column and gathers from the history or the sot sequence"""
    _wp_check(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype, "window_prompts_torch")
    (B, n), T_s = hist.shape, sot.shape[-1]
    it = item.to(torch.long)
    b = it.clamp(0, B - 1)
    Ln = torch.where((it >= 0) & (it < B), hist_len.to(torch.long)[b].clamp(0, n), 0)
    room = width - T_s
    h = Ln.clamp_max(room - 1) if room >= 2 else torch.zeros_like(Ln)
    pre = torch.where(h > 0, 1 + h, 0).unsqueeze(1)
    ks = width - T_s - pre
    rel = torch.arange(width, device=hist.device).unsqueeze(0) - ks
    rows = sot.to(torch.long)
    rows = rows[b] if sot.dim() == 2 else rows.unsqueeze(0).expand(b.shape[0], -1)
    from_sot = rows.gather(1, (rel - pre).clamp(0, T_s - 1))
    from_hist = hist.to(torch.long)[b].gather(1, ((Ln - h).unsqueeze(1) + rel - 1).clamp(0, n - 1))
    ids = torch.where(rel >= pre, from_sot, torch.where(rel >= 1, from_hist, torch.where(rel == 0, sot_prev_token_id, 0)))
    return WindowPrompts(ids.to(out_dtype), ks.squeeze(1).to(torch.int32))


def _wp_accept(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype):
    """the args struct of a call that mopk_window_prompts takes, None of one it refuses; the outputs hold stand-ins"""
    A, T_s = item.shape[0], sot.shape[-1]
    if not hist.is_cuda or item.dtype != torch.int32 or (A > 1 and item.stride(0) != 1) or sot.dtype not in (torch.int32, torch.int64):
        return None
    if (T_s > 1 and sot.stride(-1) != 1) or (sot.dim() == 2 and sot.shape[0] > 1 and sot.stride(0) < T_s) or width > WINDOW_PROMPTS_MAX_WIDTH:
        return None
    a = L.WindowPromptsArgs()
    a.A, a.width, a.Ts, a.prev = A, width, T_s, sot_prev_token_id
    a.B, a.n = hist.shape
    a.out_i64, a.sot_i64 = int(out_dtype == torch.int64), int(sot.dtype == torch.int64)
    a.hist, a.hist_len, a.item, a.sot = hist.data_ptr(), hist_len.data_ptr(), item.data_ptr(), sot.data_ptr()
    a.sot_ld = 0 if sot.dim() == 1 else (T_s if sot.shape[0] == 1 else sot.stride(0))
    a.ids = a.kv_start = 8                                                         # stand-ins: only their alignment is looked at
    return a if L.lib().mopk_window_prompts_supported(C.byref(a)) else None


def window_prompts_supported(hist: torch.Tensor, hist_len: torch.Tensor, item: torch.Tensor, sot: torch.Tensor,
                             sot_prev_token_id: int, width: int, out_dtype: torch.dtype = torch.int64) -> bool:
    """True if mopk_window_prompts takes this call: CUDA tensors, a contiguous int32 item, an int32 or int64 sot with unit inner
    stride, width <= 2048 (the library's own query decides the rest).  Raises ValueError on bad arguments."""
    _wp_check(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype, "window_prompts_supported")
    return _wp_accept(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype) is not None


def window_prompts(hist: torch.Tensor, hist_len: torch.Tensor, item: torch.Tensor, sot: torch.Tensor, sot_prev_token_id: int,
                   width: int, out_dtype: torch.dtype = torch.int64) -> WindowPrompts:
    """the prompt matrix of a set of windows, each conditioned on its clip's token history (Whisper's
    [sot_prev] + prompt_tokens[-(n_ctx // 2 - 1):] + sot_sequence) -> WindowPrompts(ids (A, width) of out_dtype, kv_start (A,)
    int32), left-padded as the decoders take a ragged batch.  Inference only.

    hist, hist_len: the state `prompt_history_update` keeps.  item: (A,) int32 device tensor, the clip of row a.  sot: the
    start-of-transcript sequence, an integer (T_s,) tensor, or (B, T_s) indexed by item[a].  width >= T_s is the host's choice
    (the output's shape cannot depend on device values): T_s + 1 + the longest history among the rows holds every row in full.
    Per row a, with b = item[a], L = hist_len[b] clamped into [0, n] and room = width - T_s:
    h = min(L, room - 1) if L > 0 and room >= 2, else 0 (a narrower width keeps the NEWEST h tokens; one too narrow for
    sot_prev_token_id and one token drops the history);  length = T_s + (1 + h if h > 0 else 0);
    ids[a] = width - length zeros, then [sot_prev_token_id, hist[b, L-h:L]] when h > 0, then the sot sequence;
    kv_start[a] = width - length.
    An item outside [0, B) makes a row without history (with a (B, T_s) sot: under the nearest clip's sequence).
    Runs the HIP kernel (mopk_window_prompts: one launch writes both outputs, every word once) when window_prompts_supported()
    accepts the call, else window_prompts_torch(); LAST_PATH["window_prompts"] records which.  No host sync, no workspace;
    bitwise reproducible."""
    _wp_check(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype, "window_prompts")
    with torch.no_grad():
        a = _wp_accept(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype)
        if a is None:
            LAST_PATH["window_prompts"] = L.PATH_GENERIC
            return window_prompts_torch(hist, hist_len, item, sot, sot_prev_token_id, width, out_dtype)
        ids = torch.empty(a.A, width, dtype=out_dtype, device=hist.device)
        ks = torch.empty(a.A, dtype=torch.int32, device=hist.device)
        a.ids, a.kv_start = ids.data_ptr(), ks.data_ptr()                          # in place of the stand-ins
        _row_launch(a, "mopk_window_prompts", "window_prompts")
        return WindowPrompts(ids, ks)


# --------------------------------------------------------------------------------------
# Word timestamps (WhisperMoP.align_words, transcribe(word_timestamps=True)): the tokenizer's part as a table over the vocabulary,
# decoded window rows turned into alignment inputs, and Whisper's word grouping and timing on the aligned text tokens
ALIGNMENT_ROWS_MAX_COLS = 1024 # generated columns of a row (one thread each)
WORD_SPANS_MAX_TOKENS = 1024   # text tokens of a row (one thread each)
WORD_BEGIN, WORD_PREPEND, WORD_APPEND, WORD_SENTENCE_END = 1, 2, 4, 8      # the bits of WordRules.table


class WordRules:
    """what Whisper's word grouping (split_tokens_on_spaces, merge_punctuations, the sentence-end truncation of
    add_word_timestamps) reads from a tokenizer, as a (V,) uint8 table over the token ids: bit 0 (1) the token begins a word,
    bit 1 (2) it is prepend punctuation, bit 2 (4) append punctuation, bit 3 (8) a sentence-end mark.

    word_begin, prepend_punct, append_punct, sentence_end: each an iterable of token ids or a bool (V,) tensor.  The constructor
    validates everything (ValueError) before any device work and builds `table` once, on `device` (default: the CPU);
    `on(device)` returns the table's copy on a device, made once per device.  `from_pieces` builds the rules from the decoded
    text of every token."""

    def __init__(self, vocab_size: int, word_begin, prepend_punct=(), append_punct=(), sentence_end=(), device=None):
        if isinstance(vocab_size, bool) or not isinstance(vocab_size, int) or vocab_size < 1:
            raise ValueError(f"WordRules: vocab_size must be an int >= 1, got {vocab_size!r}")
        V = vocab_size
        mask = torch.zeros(V, dtype=torch.uint8)
        for bit, name, arg in ((WORD_BEGIN, "word_begin", word_begin), (WORD_PREPEND, "prepend_punct", prepend_punct),
                               (WORD_APPEND, "append_punct", append_punct), (WORD_SENTENCE_END, "sentence_end", sentence_end)):
            if isinstance(arg, torch.Tensor):
                if arg.dtype != torch.bool or arg.shape != (V,):
                    raise ValueError(f"WordRules: a tensor {name} must be bool ({V},), got {(tuple(arg.shape), arg.dtype)}")
                mask |= arg.to("cpu", torch.uint8) * bit
                continue
            if isinstance(arg, (str, bytes)) or not hasattr(arg, "__iter__"):
                raise ValueError(f"WordRules: {name} must be an iterable of token ids or a bool ({V},) tensor, got {type(arg).__name__}")
            ids = []
            for x in arg:
                if isinstance(x, bool) or not isinstance(x, int):
                    raise ValueError(f"WordRules: {name} id must be an int, got {x!r}")
                if not 0 <= x < V:
                    raise ValueError(f"WordRules: {name} id = {x} outside [0, vocab_size = {V})")
                ids.append(x)
            if ids:
                mask[torch.tensor(ids, dtype=torch.long)] |= bit
        self.vocab_size = V
        self._tables = {torch.device("cpu"): mask}
        self.table = self.on("cpu" if device is None else device)

    def on(self, device) -> torch.Tensor:
        """the (V,) uint8 table on `device` (copied there once, without a host sync)"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._tables.get(device)
        if t is None:
            cpu = self._tables[torch.device("cpu")]
            t = cpu.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else cpu.to(device)
            self._tables[device] = t
        return t

    @classmethod
    def from_pieces(cls, pieces, prepend="\"'“¿([{-", append="\"'.。,，!！?？:：”)]}、", sentence_end=".。!！?？", device=None):
        """the rules of a vocabulary whose token v decodes to the text pieces[v] (None: a token without text, no bit), after
        Whisper's split_tokens_on_spaces and merge_punctuations:
        begin: the piece starts with " ", or piece.strip() is one character of string.punctuation;
        prepend: the piece starts with " " and piece.strip() is in `prepend`;  append: the piece itself, unstripped, is in `append`
        and not empty;  sentence end: the piece is a single character of `sentence_end`.
        Languages that Whisper splits on unicode code points rather than on spaces are not covered."""
        import string
        pieces = list(pieces)
        if any(p is not None and not isinstance(p, str) for p in pieces):
            raise ValueError("WordRules.from_pieces: every piece must be a str or None")
        if not all(isinstance(s, str) for s in (prepend, append, sentence_end)):
            raise ValueError("WordRules.from_pieces: prepend, append and sentence_end must be str")
        sets = ([], [], [], [])
        for v, p in enumerate(pieces):
            if p is None:
                continue
            core = p.strip()
            if p.startswith(" ") or (len(core) == 1 and core in string.punctuation):
                sets[0].append(v)
            if p.startswith(" ") and core in prepend:               # str containment, as Whisper tests it: " " counts
                sets[1].append(v)
            if p and p in append:
                sets[2].append(v)
            if len(p) == 1 and p in sentence_end:
                sets[3].append(v)
        return cls(len(pieces), *sets, device=device)


class AlignmentRows(NamedTuple):
    """the alignment inputs of a set of decoded windows (`alignment_rows`), W = T_p + 2 + (T - t0) columns: ids (R, W), each row
    [sot, no-timestamps token, text tokens, eos ...]; n_tokens (R,) int32 = T_p + 2 + the row's text tokens; col (R, W) int32, the
    column of `tokens` text token i came from, -1 behind the row's text tokens"""
    ids: torch.Tensor
    n_tokens: torch.Tensor
    col: torch.Tensor


class WordSpans(NamedTuple):
    """the words of a batch of aligned token rows (`word_spans`): starts / ends (R, N) int32 frames, probs (R, N) fp32,
    tok_begin / tok_end (R, N) int32 indices into the row's text tokens (the end exclusive), n_words (R,) int32; at
    j >= n_words[r] the integers are -1 and probs is 0"""
    starts: torch.Tensor
    ends: torch.Tensor
    probs: torch.Tensor
    tok_begin: torch.Tensor
    tok_end: torch.Tensor
    n_words: torch.Tensor


def _int_matrix_check(t, name: str, what: str, shape=None) -> None:
    if (not isinstance(t, torch.Tensor) or t.dim() != 2 or 0 in t.shape or t.dtype.is_floating_point or t.dtype.is_complex
            or t.dtype == torch.bool or (shape is not None and tuple(t.shape) != shape)):
        raise ValueError(f"{what}: {name} must be a non-empty integer {'(R, T)' if shape is None else shape} tensor, got "
                         f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")


def _ar_check(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype, what: str) -> None:
    """validate an alignment_rows call before any device work"""
    _int_matrix_check(tokens, "tokens", what)
    R, T = tokens.shape
    if not _is_int(t0) or not 0 <= t0 < T:
        raise ValueError(f"{what}: t0 must be an int in [0, T = {T}), got {t0!r}")
    _lens_i32_check(n_take, R, tokens.device, "n_take", what, "the tokens")
    if (not isinstance(sot, torch.Tensor) or sot.dim() not in (1, 2) or 0 in sot.shape or sot.dtype not in (torch.int32, torch.int64)
            or (sot.dim() == 2 and sot.shape[0] != R)):
        raise ValueError(f"{what}: sot must be an int32 or int64 (T_p,) or ({R}, T_p) tensor, got "
                         f"{(tuple(sot.shape), sot.dtype) if isinstance(sot, torch.Tensor) else type(sot).__name__}")
    if sot.device != tokens.device:
        raise ValueError(f"{what}: sot is on {sot.device}, the tokens on {tokens.device}")
    for name, x in (("no_timestamps_token_id", no_timestamps_token_id), ("eos_token_id", eos_token_id)):
        if not _is_int(x) or not 0 <= x < 2 ** 31:
            raise ValueError(f"{what}: {name} must be an int in [0, 2^31), got {x!r}")
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: dtype must be torch.int32 or torch.int64, got {dtype!r}")


def alignment_rows_torch(tokens: torch.Tensor, t0: int, n_take: torch.Tensor, sot: torch.Tensor, no_timestamps_token_id: int,
                         eos_token_id: int, dtype: torch.dtype = torch.int64) -> AlignmentRows:
    """the restatement of `alignment_rows` in torch ops (CPU or GPU, vectorised over rows, no host sync): a cumulative sum numbers
    the text tokens, and scatters into buffers with one spare column that takes the write of every column that has none to make"""
    _ar_check(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype, "alignment_rows_torch")
    R, T = tokens.shape
    dev, S, Tp = tokens.device, T - t0, sot.shape[-1]
    W = Tp + 2 + S
    g = tokens[:, t0:].to(torch.long)
    j = torch.arange(S, device=dev).unsqueeze(0)
    text = (j < n_take.to(torch.long).clamp(0, S).unsqueeze(1)) & (g < eos_token_id)
    pos = text.cumsum(1) - text.long()
    ids = torch.full((R, W + 1), eos_token_id, dtype=torch.long, device=dev)
    ids[:, :Tp] = sot.to(torch.long)
    ids[:, Tp] = no_timestamps_token_id
    ids.scatter_(1, torch.where(text, Tp + 1 + pos, W), g)
    col = torch.full((R, W + 1), -1, dtype=torch.long, device=dev)
    col.scatter_(1, torch.where(text, pos, W), (t0 + j).expand(R, S))
    return AlignmentRows(ids[:, :W].to(dtype), (Tp + 2 + text.sum(1)).to(torch.int32), col[:, :W].to(torch.int32))


def _ar_accept(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype):
    """the args struct of a call that mopk_alignment_rows takes, None of one it refuses; the outputs hold stand-ins"""
    R, T = tokens.shape
    Tp = sot.shape[-1]
    if not tokens.is_cuda or tokens.dtype != torch.int32 or (T > 1 and tokens.stride(1) != 1) or (R > 1 and tokens.stride(0) < T):
        return None
    if n_take.dtype != torch.int32 or (R > 1 and n_take.stride(0) != 1) or T - t0 > ALIGNMENT_ROWS_MAX_COLS:
        return None
    if (Tp > 1 and sot.stride(-1) != 1) or (sot.dim() == 2 and R > 1 and sot.stride(0) < Tp):
        return None
    a = L.AlignmentRowsArgs()
    a.R, a.T, a.T0, a.Tp, a.nots, a.eos = R, T, t0, Tp, no_timestamps_token_id, eos_token_id
    a.out_i64, a.sot_i64 = int(dtype == torch.int64), int(sot.dtype == torch.int64)
    a.tokens, a.tokens_ld, a.n_take, a.sot = tokens.data_ptr(), (T if R == 1 else tokens.stride(0)), n_take.data_ptr(), sot.data_ptr()
    a.sot_ld = 0 if sot.dim() == 1 else (Tp if R == 1 else sot.stride(0))
    a.ids = a.n_tokens = a.col = 8                                                 # stand-ins: only their alignment is looked at
    return a if L.lib().mopk_alignment_rows_supported(C.byref(a)) else None


def alignment_rows_supported(tokens: torch.Tensor, t0: int, n_take: torch.Tensor, sot: torch.Tensor, no_timestamps_token_id: int,
                             eos_token_id: int, dtype: torch.dtype = torch.int64) -> bool:
    """True if mopk_alignment_rows takes this call: CUDA int32 tokens with unit inner stride and a row stride >= T (one row: any),
    a contiguous int32 n_take, a sot with unit inner stride, T - t0 <= 1024 (the library's own query decides the rest).  Raises
    ValueError on bad arguments."""
    _ar_check(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype, "alignment_rows_supported")
    return _ar_accept(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype) is not None


def alignment_rows(tokens: torch.Tensor, t0: int, n_take: torch.Tensor, sot: torch.Tensor, no_timestamps_token_id: int,
                   eos_token_id: int, dtype: torch.dtype = torch.int64) -> AlignmentRows:
    """the inputs of the alignment pass behind word timestamps, from the decoded rows of a set of windows (the text_tokens of
    Whisper's find_alignment: no timestamp tokens, no eos, the <|notimestamps|> lead-in) -> AlignmentRows(ids, n_tokens, col).
    Inference only.

    tokens: (R, T) int32 decoder outputs, the rows `timestamp_segments` takes (unit inner stride, any row stride >= T); t0: the
    first generated column.  n_take: (R,) int32 device tensor, how many generated tokens of row r lie inside its segments, clamped
    into [0, T - t0].  sot: the prompt the alignment pass runs under, an int32 or int64 (T_p,) tensor or (R, T_p), one per row.
    With g = tokens[r, t0:] and W = T_p + 2 + (T - t0):
    ids[r] = sot_r, no_timestamps_token_id, the g[j] < eos_token_id among j < n_take[r] in order (n_text[r] of them), then
    eos_token_id to the end of the row;  n_tokens[r] = T_p + 2 + n_text[r];  col[r, i] = t0 + j of text token i for i < n_text[r],
    else -1.  ids has `dtype` (int32 or int64), n_tokens and col are int32.
    Runs the HIP kernel (mopk_alignment_rows: one launch, a stable compaction by wave ballots) when alignment_rows_supported()
    accepts the call, else alignment_rows_torch(); LAST_PATH["alignment_rows"] records which.  No host sync, no workspace; bitwise
    reproducible."""
    _ar_check(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype, "alignment_rows")
    with torch.no_grad():
        a = _ar_accept(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype)
        if a is None:
            LAST_PATH["alignment_rows"] = L.PATH_GENERIC
            return alignment_rows_torch(tokens, t0, n_take, sot, no_timestamps_token_id, eos_token_id, dtype)
        W = a.Tp + 2 + a.T - a.T0
        ids = torch.empty(a.R, W, dtype=dtype, device=tokens.device)
        col = torch.empty(a.R, W, dtype=torch.int32, device=tokens.device)
        n_tokens = torch.empty(a.R, dtype=torch.int32, device=tokens.device)
        a.ids, a.n_tokens, a.col = ids.data_ptr(), n_tokens.data_ptr(), col.data_ptr()     # in place of the stand-ins
        _row_launch(a, "mopk_alignment_rows", "alignment_rows")
        return AlignmentRows(ids, n_tokens, col)


def _ws_check(tokens, times, probs, n_text, word_rules, median_cap, what: str) -> None:
    """validate a word_spans call before any device work"""
    _int_matrix_check(tokens, "tokens", what)
    R, N = tokens.shape
    _int_matrix_check(times, "times", what, (R, N + 1))
    if not isinstance(probs, torch.Tensor) or tuple(probs.shape) != (R, N) or probs.dtype != torch.float32:
        raise ValueError(f"{what}: probs must be an fp32 ({R}, {N}) tensor, got "
                         f"{(tuple(probs.shape), probs.dtype) if isinstance(probs, torch.Tensor) else type(probs).__name__}")
    for name, t in (("times", times), ("probs", probs)):
        if t.device != tokens.device:
            raise ValueError(f"{what}: {name} is on {t.device}, the tokens on {tokens.device}")
    _lens_i32_check(n_text, R, tokens.device, "n_text", what, "the tokens")
    if not isinstance(word_rules, WordRules):
        raise ValueError(f"{what}: word_rules must be a WordRules, got {type(word_rules).__name__}")
    if median_cap is not None and (not _is_int(median_cap) or not 0 <= median_cap < 2 ** 30):
        raise ValueError(f"{what}: median_cap must be None or an int in [0, 2^30), got {median_cap!r}")


def word_spans_torch(tokens: torch.Tensor, times: torch.Tensor, probs: torch.Tensor, n_text: torch.Tensor, word_rules: WordRules,
                     median_cap: Optional[int] = None) -> WordSpans:
    """the restatement of `word_spans` in torch ops (CPU or GPU, vectorised over rows, no host sync): cumulative sums number the
    words and the survivors, a sort finds the median, and scatters into buffers with one spare column place the results.  A
    word's probability is the difference of a float64 running sum, rounded to fp32 once."""
    _ws_check(tokens, times, probs, n_text, word_rules, median_cap, "word_spans_torch")
    R, N = tokens.shape
    dev, V = tokens.device, word_rules.vocab_size
    table = word_rules.on(dev).to(torch.long)
    n = n_text.to(torch.long).clamp(0, N).unsqueeze(1)
    i = torch.arange(N, device=dev).unsqueeze(0)                                   # a token index, and later a word index
    c = torch.where(i < n, table[tokens.to(torch.long).clamp(0, V - 1)], 0)
    begin = (i < n) & ((i == 0) | ((c & WORD_BEGIN) != 0))                         # rule 1
    K = begin.sum(1, keepdim=True)
    o = n.expand(R, N + 2).clone()                                                 # o[k] = n at k >= K
    o.scatter_(1, torch.where(begin, begin.cumsum(1) - 1, N + 1), i.expand(R, N))
    o0, o1 = o[:, :N], o[:, 1:N + 1]
    word = i < K
    tm = times.to(torch.long)
    s, e = tm.gather(1, o0), tm.gather(1, o1)
    cs = F.pad(torch.where(i < n, probs, 0).to(torch.float64).cumsum(1), (1, 0))
    p = ((cs.gather(1, o1) - cs.gather(1, o0)) / (o1 - o0).clamp_min(1)).to(torch.float32)
    fl = torch.where(word & (o1 - o0 == 1), c.gather(1, o0.clamp_max(N - 1)), 0)
    P, A, E = ((fl & b) != 0 for b in (WORD_PREPEND, WORD_APPEND, WORD_SENTENCE_END))
    d = torch.where(word, e - s, 0)
    nz = word & (d != 0)                                                           # rule 2
    M = nz.sum(1, keepdim=True)
    srt = torch.where(nz, d, torch.iinfo(torch.long).max).sort(1).values
    m2 = torch.where(M > 0, srt.gather(1, ((M - 1) // 2).clamp_min(0)) + srt.gather(1, (M // 2).clamp_max(N - 1)), 0)
    max_dur = m2 if median_cap is None else m2.clamp_max(2 * median_cap)
    before = lambda t: F.pad(t, (1, 0))[:, :N]                                     # noqa: E731  the flag of word k - 1
    long_ = word & (i >= 1) & (d > max_dur)                                        # rule 3
    e2 = torch.where(long_ & E, s + max_dur, e)
    s2 = torch.where(long_ & ~E & before(E), e - max_dur, s)
    die1 = P & (i < K - 1)                                                         # rule 4
    die2 = word & (i >= 1) & ~die1 & A & ~before(die1)                             # rule 5
    surv = word & ~die1 & ~die2                                                    # rule 6
    idx = surv.cumsum(1) - surv.long()
    nw = surv.sum(1, keepdim=True)
    tb = n.expand(R, N + 2).clone()                                                # tb[j] = n at j >= n_words
    tb.scatter_(1, torch.where(word & ~before(die1) & (surv | die1), idx, N + 1), o0)
    to = torch.where(surv, idx, N)
    starts, ends = (torch.full((R, N + 1), -1, dtype=torch.long, device=dev).scatter_(1, to, v)[:, :N] for v in (s2, e2))
    out_p = torch.zeros(R, N + 1, dtype=torch.float32, device=dev).scatter_(1, to, p)[:, :N]
    live = i < nw
    i32 = lambda t: t.to(torch.int32)                                              # noqa: E731
    return WordSpans(i32(starts), i32(ends), out_p, i32(torch.where(live, tb[:, :N], -1)), i32(torch.where(live, tb[:, 1:N + 1], -1)),
                     i32(nw.squeeze(1)))


def _ws_accept(tokens, times, probs, n_text, word_rules, median_cap):
    """the args struct of a call that mopk_word_spans takes, None of one it refuses; the outputs hold stand-ins"""
    R, N = tokens.shape
    if not tokens.is_cuda or tokens.dtype != torch.int32 or times.dtype != torch.int32 or N > WORD_SPANS_MAX_TOKENS:
        return None
    if (N > 1 and (tokens.stride(1) != 1 or probs.stride(1) != 1)) or times.stride(1) != 1:
        return None
    if R > 1 and (tokens.stride(0) < N or probs.stride(0) < N or times.stride(0) < N + 1):
        return None
    if n_text.dtype != torch.int32 or (R > 1 and n_text.stride(0) != 1):
        return None
    a = L.WordSpansArgs()
    a.R, a.N, a.V, a.median_cap = R, N, word_rules.vocab_size, (-1 if median_cap is None else median_cap)
    a.tokens, a.times, a.probs = tokens.data_ptr(), times.data_ptr(), probs.data_ptr()
    a.tokens_ld, a.times_ld, a.probs_ld = (N, N + 1, N) if R == 1 else (tokens.stride(0), times.stride(0), probs.stride(0))
    a.n_text, a.table = n_text.data_ptr(), word_rules.on(tokens.device).data_ptr()
    a.starts = a.ends = a.out_probs = a.tok_begin = a.tok_end = a.n_words = 8      # stand-ins: only their alignment is looked at
    return a if L.lib().mopk_word_spans_supported(C.byref(a)) else None


def word_spans_supported(tokens: torch.Tensor, times: torch.Tensor, probs: torch.Tensor, n_text: torch.Tensor,
                         word_rules: WordRules, median_cap: Optional[int] = None) -> bool:
    """True if mopk_word_spans takes this call: CUDA tensors, int32 tokens and times and fp32 probs with unit inner strides and
    row strides that hold a row (one row: any), a contiguous int32 n_text, N <= 1024 (the library's own query decides the rest).
    Raises ValueError on bad arguments."""
    _ws_check(tokens, times, probs, n_text, word_rules, median_cap, "word_spans_supported")
    return _ws_accept(tokens, times, probs, n_text, word_rules, median_cap) is not None


def word_spans(tokens: torch.Tensor, times: torch.Tensor, probs: torch.Tensor, n_text: torch.Tensor, word_rules: WordRules,
               median_cap: Optional[int] = None) -> WordSpans:
    """Whisper's word grouping and timing (find_alignment's split into words, then add_word_timestamps' duration bound and
    merge_punctuations) on a batch of aligned token rows -> WordSpans(starts, ends, probs, tok_begin, tok_end, n_words).
    Inference only.

    tokens: (R, N) int32 text tokens (ids are clamped into [0, V) for the table lookup).  times: (R, N + 1) int32, times[r, i]
    the frame at which text token i begins, times[r, n] the closing frame.  probs: (R, N) fp32 token probabilities.  n_text: (R,)
    int32 device tensor, used as n = clamp(n_text[r], 0, N).  word_rules: the WordRules of the vocabulary.  median_cap: an int
    >= 0 in frames, or None for no cap (Whisper's 0.7 s is 70 at 10 ms frames).  Unit inner strides, free row strides.  Per row:
    1. token i begins a word when i == 0 or its table entry has bit 0; word k covers the tokens [o_k, o_{k+1}), o_K = n;
       s_k = times[o_k], e_k = times[o_{k+1}] (a word ends where the next one starts), p_k = the fp32 mean of its tokens'
       probabilities; the word is prepend / append / sentence-end (P_k / A_k / E_k) when it has exactly one token and that token
       has the bit;
    2. d_k = e_k - s_k; m2 = twice numpy.median of the d_k != 0 (odd count: twice the middle value; even: the sum of the two
       middle values; none: 0); max_dur = m2, or min(m2, 2 * median_cap); integers throughout;
    3. for k >= 1 with d_k > max_dur: if E_k, e_k = s_k + max_dur; else if E_{k-1}, s_k = e_k - max_dur (original values on the
       right-hand sides);
    4. pass 1 (Whisper's right-to-left pass): a word with P_k and k < K - 1 dies; its tokens go in front of the nearest later
       word that does not die in this pass;
    5. pass 2 (left-to-right): a word k >= 1 that survived pass 1, has A_k and received nothing in pass 1 dies, unless every
       earlier word died in pass 1; its tokens go to the back of the nearest earlier word that survives both passes;
    6. the survivors, in order, keep their own s, e, p (Whisper merges text and tokens, not times or probabilities); their token
       ranges [tok_begin, tok_end) include what they absorbed, are contiguous and partition [0, n).
    Two deviations from Whisper: pass 2 does not test `not previous.word.endswith(" ")` (a property of the merged text, not of a
    token id), and punctuation words of more than one token are not recognised.
    Runs the HIP kernel (mopk_word_spans: one launch, one workgroup per row, ballot scans for the word and survivor numbering,
    the per-word values in LDS, the median by ranking) when word_spans_supported() accepts the call, else word_spans_torch()
    (N > 1024 among others); LAST_PATH["word_spans"] records which.  No host sync, no workspace; bitwise reproducible."""
    _ws_check(tokens, times, probs, n_text, word_rules, median_cap, "word_spans")
    with torch.no_grad():
        a = _ws_accept(tokens, times, probs, n_text, word_rules, median_cap)
        if a is None:
            LAST_PATH["word_spans"] = L.PATH_GENERIC
            return word_spans_torch(tokens, times, probs, n_text, word_rules, median_cap)
        seg = torch.empty(4, a.R, a.N, dtype=torch.int32, device=tokens.device)
        out_p = torch.empty(a.R, a.N, dtype=torch.float32, device=tokens.device)
        n_words = torch.empty(a.R, dtype=torch.int32, device=tokens.device)
        a.starts, a.ends, a.tok_begin, a.tok_end = (seg[k].data_ptr() for k in range(4))        # in place of the stand-ins
        a.out_probs, a.n_words = out_p.data_ptr(), n_words.data_ptr()
        _row_launch(a, "mopk_word_spans", "word_spans")
        return WordSpans(seg[0], seg[1], out_p, seg[2], seg[3], n_words)


# --------------------------------------------------------------------------------------
# Audio frontend (LogMelFrontend): Whisper's log-mel spectrogram of a batch of waveforms
LOG_MEL_TILE_FRAMES = L.LOG_MEL_TILE_FRAMES     # frames per workgroup of the tile kernel
LOG_MEL_MIN_FFT, LOG_MEL_MAX_FFT, LOG_MEL_MAX_MELS = 16, 512, 128
_LM_TABLES = {}                # (n_fft, device, dtype) -> (twiddle (n_fft, 2), window (n_fft,))
_LM_BANDS = {}                 # id(filters) -> (weak reference, version, bands (n_mels, 2) int32)


def _slaney_hz_to_mel(f: float) -> float:
    return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0) if f >= 1000.0 else f / (200.0 / 3.0)


def _slaney_mel_to_hz(m: float) -> float:
    return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0)) if m >= 15.0 else m * (200.0 / 3.0)


def mel_filterbank(sample_rate: int, n_fft: int, n_mels: int, device=None) -> torch.Tensor:
    """the Slaney-scale, area-normalised triangular mel filterbank (librosa.filters.mel's default, the matrix Whisper ships as
    mel_filters.npz) -> (n_mels, n_fft/2 + 1) fp32.  The mel scale is linear below 1 kHz (200/3 Hz per mel) and logarithmic above
    (step log(6.4)/27); n_mels + 2 points f_0 .. f_{n_mels+1} are spaced evenly in mel over [0, sample_rate/2]; row m is the
    triangle over [f_m, f_{m+2}] with its peak at f_{m+1}, scaled by 2 / (f_{m+2} - f_m).  Computed in float64 on the host."""
    for name, v in (("sample_rate", sample_rate), ("n_fft", n_fft), ("n_mels", n_mels)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"mel_filterbank: {name} must be an int >= 1, got {v!r}")
    if n_fft % 2:
        raise ValueError(f"mel_filterbank: n_fft must be even, got {n_fft}")
    top = _slaney_hz_to_mel(sample_rate / 2.0)
    pts = torch.tensor([_slaney_mel_to_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)], dtype=torch.float64)
    freqs = torch.arange(n_fft // 2 + 1, dtype=torch.float64) * (sample_rate / 2.0 / (n_fft // 2))
    d = pts[1:] - pts[:-1]
    r = pts.unsqueeze(1) - freqs.unsqueeze(0)
    w = torch.minimum(-r[:-2] / d[:-1].unsqueeze(1), r[2:] / d[1:].unsqueeze(1)).clamp_min(0.0)
    w = w * (2.0 / (pts[2:] - pts[:-2])).unsqueeze(1)
    return w.to(torch.float32).to(device) if device is not None else w.to(torch.float32)


def _lm_tables(n_fft: int, device, dtype):
    """(twiddle (n_fft, 2): cos and sin of 2 pi i / n_fft, window (n_fft,): periodic Hann), computed once per (n_fft, device,
    dtype) in float64 and rounded to dtype"""
    key = (n_fft, str(device), dtype)
    if key not in _LM_TABLES:
        ang = torch.arange(n_fft, dtype=torch.float64) * (2.0 * math.pi / n_fft)
        tw = torch.stack((torch.cos(ang), torch.sin(ang)), dim=1)
        _LM_TABLES[key] = (tw.to(dtype).to(device).contiguous(), (0.5 - 0.5 * torch.cos(ang)).to(dtype).to(device).contiguous())
    return _LM_TABLES[key]


def _lm_bands(filters: torch.Tensor) -> torch.Tensor:
    """(n_mels, 2) int32 on the filters' device: row m of the filters is zero outside [lo, hi) (an empty row: lo = hi = 0).  Built
    with a few torch ops and no host sync, then kept for as long as the same tensor object is passed in unchanged (its version
    counter), so a frontend that holds its filters pays for it once.  A tensor made under torch.inference_mode has no version
    counter and could change unseen, so its table is derived on every call"""
    import weakref
    version = None if filters.is_inference() else filters._version
    hit = _LM_BANDS.get(id(filters))
    if version is not None and hit is not None and hit[0]() is filters and hit[1] == version:
        return hit[2]
    nz = filters != 0
    nb = filters.shape[1]
    lo = nz.to(torch.int32).argmax(1)
    hi = nb - nz.flip(1).to(torch.int32).argmax(1)
    some = nz.any(1)
    bands = torch.stack((torch.where(some, lo, 0), torch.where(some, hi, 0)), dim=1).to(torch.int32).contiguous()
    for k in [k for k, v in _LM_BANDS.items() if v[0]() is None]:
        del _LM_BANDS[k]
    if version is not None:
        _LM_BANDS[id(filters)] = (weakref.ref(filters), version, bands)
    return bands


def _lm_check(audio, filters, n_fft, hop_length, lens, out_dtype, what: str) -> None:
    """validate a log_mel call before any device work"""
    if (not isinstance(audio, torch.Tensor) or audio.dim() != 2 or 0 in audio.shape
            or audio.dtype not in (torch.float32, torch.bfloat16, torch.float16, torch.float64)):
        raise ValueError(f"{what}: audio must be a non-empty (B, L) tensor of float32, bfloat16, float16 or float64 samples, got "
                         f"{(tuple(audio.shape), audio.dtype) if isinstance(audio, torch.Tensor) else type(audio).__name__}")
    if isinstance(n_fft, bool) or not isinstance(n_fft, int) or n_fft < 2 or n_fft % 2:
        raise ValueError(f"{what}: n_fft must be an even int >= 2, got {n_fft!r}")
    if isinstance(hop_length, bool) or not isinstance(hop_length, int) or not 1 <= hop_length <= n_fft:
        raise ValueError(f"{what}: hop_length must be an int in [1, n_fft = {n_fft}], got {hop_length!r}")
    if (not isinstance(filters, torch.Tensor) or filters.dim() != 2 or filters.shape[0] < 1 or filters.shape[1] != n_fft // 2 + 1
            or filters.dtype not in (torch.float32, torch.float64)):
        raise ValueError(f"{what}: filters must be a float32 (or float64) (n_mels, n_fft/2 + 1 = {n_fft // 2 + 1}) tensor, got "
                         f"{(tuple(filters.shape), filters.dtype) if isinstance(filters, torch.Tensor) else type(filters).__name__}")
    if filters.device != audio.device:
        raise ValueError(f"{what}: filters are on {filters.device}, the audio on {audio.device}")
    need = max(hop_length, n_fft // 2 + 1)
    if audio.shape[1] < need:
        raise ValueError(f"{what}: a clip needs at least max(hop_length, n_fft/2 + 1) = {need} samples (one frame, and a "
                         f"reflection that stays inside it), got L = {audio.shape[1]}")
    if lens is not None:
        if not isinstance(lens, torch.Tensor) or lens.dtype != torch.int32 or lens.shape != (audio.shape[0],):
            raise ValueError(f"{what}: lens must be an int32 ({audio.shape[0]},) tensor of sample counts, got "
                             f"{(tuple(lens.shape), lens.dtype) if isinstance(lens, torch.Tensor) else type(lens).__name__}")
        if lens.device != audio.device:
            raise ValueError(f"{what}: lens is on {lens.device}, the audio on {audio.device}")
    allowed = (torch.float32, torch.bfloat16) + ((torch.float64,) if audio.dtype == torch.float64 else ())
    if out_dtype not in allowed:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16 (torch.float64 for float64 audio), got {out_dtype!r}")


def log_mel_torch(audio: torch.Tensor, filters: torch.Tensor, n_fft: int = 400, hop_length: int = 160,
                  lens: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """the restatement of `log_mel` in torch ops (CPU or GPU, no host sync, no FFT library): the frames are gathered at their
    reflected sample indices into a (B, T, n_fft) matrix, windowed, and multiplied with the cos and sin bases read from the same
    (n * k) mod n_fft twiddle table the kernel uses; power, filterbank product, log10, the per-clip clamp over the valid frames,
    the scale, zeros behind T_b.  Computes in float32, in float64 for float64 audio."""
    _lm_check(audio, filters, n_fft, hop_length, lens, out_dtype, "log_mel_torch")
    cd = torch.float64 if audio.dtype == torch.float64 else torch.float32
    dev, (B, Lm), N, nb = audio.device, audio.shape, n_fft, n_fft // 2 + 1
    T = Lm // hop_length
    tw, win = _lm_tables(N, dev, cd)
    ln = torch.full((B,), Lm, dtype=torch.long, device=dev) if lens is None else lens.long().clamp(0, Lm)
    n = torch.arange(N, device=dev)
    idx = (torch.arange(T, device=dev).unsqueeze(1) * hop_length + n.unsqueeze(0) - N // 2).abs().unsqueeze(0)   # (1, T, n_fft)
    lb = ln.view(B, 1, 1)
    idx = torch.where(idx >= lb, 2 * (lb - 1) - idx, idx)
    inside = (idx >= 0) & (idx < lb)
    frames = audio.to(cd).gather(1, idx.clamp(0, Lm - 1).reshape(B, T * N)).view(B, T, N)
    frames = torch.where(inside, frames, 0.0) * win
    kk = (n.unsqueeze(1) * torch.arange(nb, device=dev).unsqueeze(0)) % N
    re, im = frames @ tw[:, 0][kk], frames @ tw[:, 1][kk]
    g = ((re * re + im * im) @ filters.to(cd).t()).clamp_min(1e-10).log10()
    valid = (torch.arange(T, device=dev).unsqueeze(0) < (ln // hop_length).unsqueeze(1)).unsqueeze(2)            # (B, T, 1)
    top = torch.where(valid, g, float("-inf")).amax(dim=(1, 2), keepdim=True)
    out = (torch.maximum(g, top - 8.0) + 4.0) / 4.0
    return torch.where(valid, out, 0.0).to(out_dtype)


def _lm_args(audio, filters, n_fft, hop_length, lens, out_dtype, tables, bands) -> L.LogMelArgs:
    a = L.LogMelArgs()
    a.B, a.L = audio.shape
    a.n_fft, a.hop, a.n_mels = n_fft, hop_length, filters.shape[0]
    a.audio_dtype = {torch.float32: L.MOPK_F32, torch.bfloat16: L.MOPK_BF16, torch.float16: L.LOG_MEL_F16}[audio.dtype]
    a.out_dtype = L.MOPK_BF16 if out_dtype == torch.bfloat16 else L.MOPK_F32
    a.audio, a.audio_ld = audio.data_ptr(), audio.stride(0) if a.B > 1 else a.L       # a single row: its stride is never used
    a.lens, a.filters, a.bands = _ptr(lens), filters.data_ptr(), _ptr(bands)
    a.twiddle, a.window = tables[0].data_ptr(), tables[1].data_ptr()
    return a


def _lm_accept(audio, filters, n_fft, hop_length, lens, out_dtype):
    """the args struct (without the output and the workspace) of a call that mopk_log_mel takes, None of one it refuses"""
    B, Lm = audio.shape
    if not audio.is_cuda or audio.dtype == torch.float64 or (Lm > 1 and audio.stride(1) != 1) or (B > 1 and audio.stride(0) < Lm):
        return None
    if filters.dtype != torch.float32 or not filters.is_contiguous() or out_dtype == torch.float64:
        return None
    if lens is not None and B > 1 and lens.stride(0) != 1:
        return None
    if not (LOG_MEL_MIN_FFT <= n_fft <= LOG_MEL_MAX_FFT and filters.shape[0] <= LOG_MEL_MAX_MELS):
        return None
    a = _lm_args(audio, filters, n_fft, hop_length, lens, out_dtype, _lm_tables(n_fft, audio.device, torch.float32), _lm_bands(filters))
    a.out = a.filters                                                              # a stand-in: only its alignment is looked at
    return a if L.lib().mopk_log_mel_supported(C.byref(a)) else None


def log_mel_supported(audio: torch.Tensor, filters: torch.Tensor, n_fft: int = 400, hop_length: int = 160,
                      lens: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> bool:
    """True if mopk_log_mel takes this call: CUDA float32 / bfloat16 / float16 audio with unit inner stride and a row stride >= L,
    contiguous float32 filters, n_fft even in [16, 512], n_mels <= 128, a contiguous lens, out_dtype float32 or bfloat16 (the
    library's own query decides the rest).  Raises ValueError on bad arguments."""
    _lm_check(audio, filters, n_fft, hop_length, lens, out_dtype, "log_mel_supported")
    return _lm_accept(audio, filters, n_fft, hop_length, lens, out_dtype) is not None


def log_mel(audio: torch.Tensor, filters: torch.Tensor, n_fft: int = 400, hop_length: int = 160,
            lens: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Whisper's log_mel_spectrogram for a batch of clips -> (B, T, n_mels) in out_dtype, T = L // hop_length: what
    WhisperMoP.encode / transcribe take.  Inference only.

    audio: (B, L) float32 / bfloat16 / float16 samples, unit inner stride, any row stride >= L.  filters: (n_mels, n_fft/2 + 1)
    float32 (`mel_filterbank`).  lens: int32 (B,) DEVICE tensor of sample counts (None: L), clamped into [0, L]; clip b has
    len_b samples and T_b = len_b // hop_length frames.  Frame t covers the samples [t * hop - n_fft/2, t * hop + n_fft/2) of the
    clip reflected at its own two ends (torch.stft(center=True, pad_mode="reflect") without its last frame); with w the periodic
    Hann window: P[t,k] = |sum_n w[n] frame_t[n] e^{-2 pi i n k / n_fft}|^2, M = P . filters^T, G = log10(max(M, 1e-10)),
    G = max(G, max_{t < T_b, m} G - 8) per clip, out = (G + 4) / 4; rows t >= T_b are zeros.  L >= max(hop_length, n_fft/2 + 1)
    is checked here; lengths that only the device knows are the caller's to keep in that range (the kernel reads zeros where a
    reflection leaves a shorter clip).
    Runs the HIP kernels (mopk_log_mel: two launches, fp32 on the f32-input MFMA) when log_mel_supported() accepts the call, else
    log_mel_torch(); LAST_PATH["log_mel"] records which.  No host sync; bitwise reproducible.  The twiddle table and the window
    are built once per (n_fft, device).  The filters' band table (the non-zero span of each row) costs about ten small torch
    launches before the two, once per filters tensor OBJECT: a call with the same unchanged tensor (a LogMelFrontend's buffer) is
    two launches, a call with a fresh tensor such as `filters.cuda()`, or with one made under torch.inference_mode, pays them
    again.  Samples are taken to be finite: a NaN or Inf sample lands on the clip's floor here, where log_mel_torch gives NaN."""
    _lm_check(audio, filters, n_fft, hop_length, lens, out_dtype, "log_mel")
    with torch.no_grad():
        a = _lm_accept(audio, filters, n_fft, hop_length, lens, out_dtype)
        if a is None:
            LAST_PATH["log_mel"] = L.PATH_GENERIC
            return log_mel_torch(audio, filters, n_fft, hop_length, lens, out_dtype)
        out = torch.empty(a.B, a.L // a.hop, a.n_mels, dtype=out_dtype, device=audio.device)
        a.out = out.data_ptr()                                                     # in place of the stand-in
        _row_launch(a, "mopk_log_mel", "log_mel", audio.device, "mopk_log_mel_workspace_bytes")
        return out


# --------------------------------------------------------------------------------------
# Audio frontend (Resample, ResampledLogMelFrontend): sample-rate conversion in front of log_mel
RESAMPLE_TILE = 1024            # outputs per workgroup of the kernel (RS_TILE of csrc/resample.hip)
RESAMPLE_MAX_SPAN, RESAMPLE_MAX_CHANNELS, RESAMPLE_MAX_TABLE = 12288, 64, 1 << 22
_RS_I16 = 3                     # MopkResampleArgs.audio_dtype of int16 samples
_RS_FILTERS = {}                # (o, n, lpw, rolloff) -> (w, S, table (n, S) float64, first (n,) int64) on the host
_RS_TABLES = {}                 # (o, n, lpw, rolloff, device, dtype) -> (table (n, S | 1) dtype, first (n,) int32) on the device


def _rs_dims(o: int, n: int, lpw: int, rolloff: float):
    """(w, S) of the reduced rate pair: the centre offset of the tap table and the taps per phase that can be non-zero"""
    if o == n:
        return 0, 1
    base = min(o, n) * rolloff
    return math.ceil(lpw * o / base), math.floor(2 * lpw * o / base) + 1


def _rs_filter(o: int, n: int, lpw: int, rolloff: float):
    """the compact tap table of the reduced rate pair, float64 on the host, kept per (o, n, lpw, rolloff): (w, S, table (n, S),
    first (n,)) with table[p, s] = K[p, first[p] + s] of the definition in `resample`.  first[p] is the first tap of phase p with
    |t| < lpw, moved down where the run would end behind the full row, so a row is a slice of the full table and every tap it
    leaves out has |t| >= lpw: below 2e-49 in float64, a zero in float32.  Only n x (S + 4) taps are ever evaluated.  The
    identity (o == n) is the single tap 1."""
    key = (o, n, lpw, float(rolloff))
    if key not in _RS_FILTERS:
        w, S = _rs_dims(o, n, lpw, rolloff)
        if o == n:
            _RS_FILTERS[key] = (w, S, torch.ones(1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
        else:
            base, width = min(o, n) * rolloff, 2 * w + o
            p = torch.arange(n, dtype=torch.float64).unsqueeze(1)

            def t_of(j):                                     # j: (n, k) int64 tap indices -> the unclamped t
                return (-p / n + (j.to(torch.float64) - w) / o) * base

            lo = (torch.floor(w + o * p / n - lpw * o / base).to(torch.int64) - 1).clamp(0, width - 1)       # at or before the run
            j = lo + torch.arange(S + 4).unsqueeze(0)
            inside = (t_of(j).abs() < lpw) & (j < width)
            first = (lo[:, 0] + inside.to(torch.int64).argmax(1)).clamp(max=width - S)
            t = t_of(first.unsqueeze(1) + torch.arange(S).unsqueeze(0)).clamp(-lpw, lpw)
            table = (base / o) * torch.cos(t * (math.pi / (2 * lpw))) ** 2 * torch.sinc(t)
            _RS_FILTERS[key] = (w, S, table, first)
    return _RS_FILTERS[key]


def _rs_tables(o: int, n: int, lpw: int, rolloff: float, device, dtype):
    """(w, S, table (n, S | 1) in dtype: the float64 taps rounded once, an odd row stride with a zero behind an even S, first
    (n,) int32), on the device, kept per (o, n, lpw, rolloff, device, dtype)"""
    key = (o, n, lpw, float(rolloff), str(device), dtype)
    w, S, table, first = _rs_filter(o, n, lpw, rolloff)
    if key not in _RS_TABLES:
        padded = torch.zeros(n, S | 1, dtype=torch.float64)
        padded[:, :S] = table
        _RS_TABLES[key] = (padded.to(dtype).to(device).contiguous(), first.to(torch.int32).to(device).contiguous())
    return (w, S) + _RS_TABLES[key]


def _rs_param_check(orig_rate, new_rate, lowpass_filter_width, rolloff, what: str) -> None:
    for name, v in (("orig_rate", orig_rate), ("new_rate", new_rate), ("lowpass_filter_width", lowpass_filter_width)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{what}: {name} must be an int >= 1, got {v!r}")
    if isinstance(rolloff, bool) or not isinstance(rolloff, (int, float)) or not 0.0 < rolloff <= 1.0:
        raise ValueError(f"{what}: rolloff must be a number in (0, 1], got {rolloff!r}")


def _rs_check(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype, what: str) -> None:
    """validate a resample call before any device work"""
    _rs_param_check(orig_rate, new_rate, lowpass_filter_width, rolloff, what)
    if (not isinstance(audio, torch.Tensor) or audio.dim() not in (2, 3) or 0 in audio.shape
            or audio.dtype not in (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int16)):
        raise ValueError(f"{what}: audio must be a non-empty (B, L) or (B, C, L) tensor of float32, bfloat16, float16, float64 or "
                         f"int16 samples, got {(tuple(audio.shape), audio.dtype) if isinstance(audio, torch.Tensor) else type(audio).__name__}")
    if lens is not None:
        if not isinstance(lens, torch.Tensor) or lens.dtype != torch.int32 or lens.shape != (audio.shape[0],):
            raise ValueError(f"{what}: lens must be an int32 ({audio.shape[0]},) tensor of sample counts, got "
                             f"{(tuple(lens.shape), lens.dtype) if isinstance(lens, torch.Tensor) else type(lens).__name__}")
        if lens.device != audio.device:
            raise ValueError(f"{what}: lens is on {lens.device}, the audio on {audio.device}")
    allowed = (torch.float32, torch.bfloat16) + ((torch.float64,) if audio.dtype == torch.float64 else ())
    if out_dtype not in allowed:
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16 (torch.float64 for float64 audio), got {out_dtype!r}")


def _rs_mono(audio: torch.Tensor, cd: torch.dtype) -> torch.Tensor:
    """(B, L) or (B, C, L) samples -> (B, L) in cd as the kernel stages them: int16 times 2^-15, the channels summed in ascending
    order and multiplied by the reciprocal of C (rounded to fp32 first when cd is float32, as the kernel's)"""
    x = audio.to(cd)
    if audio.dtype == torch.int16:
        x = x * 2.0 ** -15
    if x.dim() == 2:
        return x
    m = x[:, 0]
    for c in range(1, x.shape[1]):
        m = m + x[:, c]
    inv = 1.0 / x.shape[1] if cd == torch.float64 else float(torch.tensor(1.0) / torch.tensor(float(x.shape[1])))
    return m * inv if x.shape[1] > 1 else m


def resample_torch(audio: torch.Tensor, orig_rate: int, new_rate: int, lens: Optional[torch.Tensor] = None, *,
                   lowpass_filter_width: int = 6, rolloff: float = 0.99, out_dtype: torch.dtype = torch.float32):
    """the restatement of `resample` in torch ops (CPU or GPU, no host sync): the mono samples behind each clip's length set to
    zero and padded by the filter's reach, then one gather, multiply and add per tap over the whole (B, Lout) output, the S taps
    in ascending order as in the kernel (elementwise: a clip's samples do not depend on the batch around it); zeros behind
    len_out_b.  Computes in float32, in float64 for float64 audio.  -> (out, out_lens or None)."""
    _rs_check(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype, "resample_torch")
    cd = torch.float64 if audio.dtype == torch.float64 else torch.float32
    g = math.gcd(orig_rate, new_rate)
    o, n, dev = orig_rate // g, new_rate // g, audio.device
    w, S, table, first = _rs_tables(o, n, lowpass_filter_width, rolloff, dev, cd)
    x = _rs_mono(audio, cd)
    B, Lm = x.shape
    Lout = -(-n * Lm // o)
    out_lens = None
    if lens is not None:
        ln = lens.long().clamp(0, Lm)
        x = torch.where(torch.arange(Lm, device=dev).unsqueeze(0) < ln.unsqueeze(1), x, 0.0)
        out_lens = ((n * ln + (o - 1)) // o).to(torch.int32)
    m = torch.arange(Lout, device=dev)
    f = m // n
    p = m - f * n
    reach = (-(-Lout // n) - 1) * o + 2 * w + o                  # one past the last padded index a tap can touch
    xp = torch.nn.functional.pad(x, (w, max(reach - w - Lm, 0)))
    at = f * o + first.long()[p]                                 # padded index of each output's first tap
    acc = torch.zeros(B, Lout, dtype=cd, device=dev)
    for s in range(S):
        acc = acc + table[:, s][p] * xp[:, at + s]
    if out_lens is not None:
        acc = torch.where(m.unsqueeze(0) < out_lens.unsqueeze(1), acc, 0.0)
    return acc.to(out_dtype), out_lens


def _rs_accept(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype):
    """the args struct (without the outputs) of a call that mopk_resample takes, None of one it refuses"""
    if not audio.is_cuda or audio.dtype == torch.float64 or out_dtype == torch.float64:
        return None
    if lens is not None and lens.shape[0] > 1 and lens.stride(0) != 1:
        return None
    g = math.gcd(orig_rate, new_rate)
    o, n = orig_rate // g, new_rate // g
    B, Cn, Lm = (audio.shape[0], 1, audio.shape[1]) if audio.dim() == 2 else audio.shape
    Lout = -(-n * Lm // o)
    w, S = _rs_dims(o, n, lowpass_filter_width, rolloff)
    # the envelope, before any table is built for a pair far outside it (the library's own query decides the rest)
    if (Lm >= 2 ** 31 or Lout >= 2 ** 31 or Cn > RESAMPLE_MAX_CHANNELS or n * (S | 1) > RESAMPLE_MAX_TABLE
            or ((RESAMPLE_TILE + n - 2) // n) * o + 2 * w + o > RESAMPLE_MAX_SPAN):
        return None
    _, _, table, first = _rs_tables(o, n, lowpass_filter_width, rolloff, audio.device, torch.float32)
    a = L.ResampleArgs()
    a.B, a.C, a.L, a.Lout, a.o, a.n, a.w, a.S, a.table_ld = B, Cn, Lm, Lout, o, n, w, S, table.shape[1]
    a.audio_dtype = {torch.float32: L.MOPK_F32, torch.bfloat16: L.MOPK_BF16, torch.float16: L.LOG_MEL_F16, torch.int16: _RS_I16}[audio.dtype]
    a.out_dtype = L.MOPK_BF16 if out_dtype == torch.bfloat16 else L.MOPK_F32
    a.audio, a.audio_sb, a.audio_sl = audio.data_ptr(), audio.stride(0), audio.stride(-1)
    a.audio_sc = audio.stride(1) if audio.dim() == 3 else 0
    a.lens, a.table, a.first = _ptr(lens), table.data_ptr(), first.data_ptr()
    a.out = a.table                                                                # a stand-in: only its alignment is looked at
    return a if L.lib().mopk_resample_supported(C.byref(a)) else None


def resample_supported(audio: torch.Tensor, orig_rate: int, new_rate: int, lens: Optional[torch.Tensor] = None, *,
                       lowpass_filter_width: int = 6, rolloff: float = 0.99, out_dtype: torch.dtype = torch.float32) -> bool:
    """True if mopk_resample takes this call.  The envelope, with o / n the rates over their gcd, w = ceil(lpw o / base),
    S = floor(2 lpw o / base) + 1 and base = min(o, n) rolloff: CUDA float32 / bfloat16 / float16 / int16 audio of ANY element
    strides (no copy is made), out_dtype float32 or bfloat16, a contiguous lens; B <= 65535, C <= RESAMPLE_MAX_CHANNELS = 64,
    L < 2^31 and ceil(n L / o) < 2^31; a staged span ((RESAMPLE_TILE + n - 2) // n) o + 2 w + o <= RESAMPLE_MAX_SPAN = 12288 samples
    (48 KiB of LDS: o / n up to 11 at the default width, e.g. 176.4 kHz -> 16 kHz; S is bounded with it, S <= 2 w + o); a
    table of n (S | 1) <= RESAMPLE_MAX_TABLE = 2^22 taps (16 MiB; it sits in LDS when span and table fit 64 KiB together, else it is
    read through L2).  Every pair of 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000 -> 16000 is inside, as are the
    abstract pairs (2, 3) and (3, 2), all with the table in LDS.  Raises ValueError on bad arguments."""
    _rs_check(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype, "resample_supported")
    return _rs_accept(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype) is not None


def resample(audio: torch.Tensor, orig_rate: int, new_rate: int, lens: Optional[torch.Tensor] = None, *,
             lowpass_filter_width: int = 6, rolloff: float = 0.99, out_dtype: torch.dtype = torch.float32):
    """Sample-rate conversion of a batch of clips from orig_rate to new_rate -> (out (B, ceil(n L / o)) in out_dtype, out_lens
    int32 (B,) on the device, or None without lens): the stage in front of `log_mel`.  Inference only.

    audio: (B, L), or (B, C, L) whose channels are averaged (summed in ascending order in fp32, times the fp32 reciprocal of C); float32 /
    bfloat16 / float16 samples as they are, int16 times 2^-15 (Whisper's / 32768); any strides, so a channel-first tensor and the
    transposed view of a channel-last one both go to the kernel without a copy.  lens: int32 (B,) DEVICE tensor of sample counts
    (None: L), clamped into [0, L].
    The definition (the windowed-sinc, Hann, polyphase resampler): g = gcd(orig, new), o = orig / g, n = new / g, lpw =
    lowpass_filter_width, base = min(o, n) rolloff, w = ceil(lpw o / base).  Tap j in [0, 2 w + o) of phase p in [0, n):
    t = clamp((-p / n + (j - w) / o) base, -lpw, lpw), K[p, j] = (base / o) cos(t pi / (2 lpw))^2 sinc(pi t), sinc(0) = 1.  Clip b
    of len_b samples, zero outside [0, len_b): y[f n + p] = sum_j K[p, j] x[f o + j - w] for f n + p < len_out_b = ceil(n len_b
    / o); samples >= len_out_b of the row are zeros, out_lens[b] = len_out_b.  orig_rate == new_rate is the identity: the
    converted, downmixed samples exactly.  K is built in float64 on the host and rounded once to fp32, per (o, n, lpw, rolloff,
    device); only the S = floor(2 lpw o / base) + 1 taps per phase with |t| < lpw are kept (the others are zeros in fp32).
    Runs the HIP kernel (mopk_resample: one launch, an fp32 fmaf chain over the S taps in ascending order) when
    resample_supported() accepts the call, else resample_torch(); LAST_PATH["resample"] records which.  No host sync; bitwise
    reproducible; every clip comes out bit for bit as it would alone."""
    _rs_check(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype, "resample")
    with torch.no_grad():
        a = _rs_accept(audio, orig_rate, new_rate, lens, lowpass_filter_width, rolloff, out_dtype)
        if a is None:
            LAST_PATH["resample"] = L.PATH_GENERIC
            return resample_torch(audio, orig_rate, new_rate, lens, lowpass_filter_width=lowpass_filter_width, rolloff=rolloff,
                                  out_dtype=out_dtype)
        out = torch.empty(a.B, a.Lout, dtype=out_dtype, device=audio.device)
        out_lens = torch.empty(a.B, dtype=torch.int32, device=audio.device) if lens is not None else None
        a.out, a.out_lens = out.data_ptr(), _ptr(out_lens)                         # in place of the stand-in
        _row_launch(a, "mopk_resample", "resample")
        return out, out_lens


# ---- cross-entropy of logits, and of a linear head without its (M, V) logits (mopk_cross_entropy_*; the language models' loss()) ----
# the two autograd Functions of this family are in mop_amd/cross_entropy_fn.py (imported at the end of this file)
CE_REDUCTIONS = ("mean", "sum", "none")
# rows of logits that linear_cross_entropy holds at a time by default: of 512 / 1024 / 2048 / 4096 / M the fastest setting whose peak
# memory stayed under a quarter of the unchunked torch head + loss in bf16 at both measured shapes, M = 8192, V = 50304 and
# M = 3584, V = 51865 (tools/bench_cross_entropy.py, profiles/cross_entropy_bench.jsonl)
LINEAR_CE_CHUNK_ROWS = 2048


def _ce_check(logits, targets, ignore_index, reduction, what: str) -> None:
    """validate a cross_entropy call before any device work"""
    _stat_logits_check(logits, what)
    R = logits.shape[0]
    if not isinstance(targets, torch.Tensor) or tuple(targets.shape) != (R,) or targets.dtype != torch.long:
        raise ValueError(f"{what}: targets must be an int64 ({R},) tensor, got "
                         f"{(tuple(targets.shape), targets.dtype) if isinstance(targets, torch.Tensor) else type(targets).__name__}")
    if targets.device != logits.device:
        raise ValueError(f"{what}: targets are on {targets.device}, the logits on {logits.device}")
    if not _is_index(ignore_index):
        raise ValueError(f"{what}: ignore_index must be an int, got {ignore_index!r}")
    if reduction not in CE_REDUCTIONS:
        raise ValueError(f"{what}: reduction must be one of {CE_REDUCTIONS}, got {reduction!r}")


def _ce_counted(targets: torch.Tensor, V: int, ignore_index: int) -> torch.Tensor:
    """the rows that count: a target that is neither ignore_index nor outside [0, V)"""
    return (targets != ignore_index) & (targets >= 0) & (targets < V)


def cross_entropy_torch(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100, reduction: str = "mean") -> torch.Tensor:
    """the restatement of `cross_entropy` in torch ops (no host sync): F.cross_entropy(logits.float(), targets) with every target
    outside [0, V) treated as ignored, as the kernel treats it (torch alone asserts on the device)"""
    _ce_check(logits, targets, ignore_index, reduction, "cross_entropy_torch")
    t = torch.where(_ce_counted(targets, logits.shape[1], ignore_index), targets, torch.full_like(targets, ignore_index))
    return F.cross_entropy(logits.float(), t, ignore_index=ignore_index, reduction=reduction)


def _ce_args(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int, row0: int = 0):
    """the args struct, without outputs, of logits that hold rows [row0, row0 + R) of the problem `targets` spans"""
    a = L.CrossEntropyArgs()
    a.R, a.V = logits.shape
    a.dtype = L.MOPK_BF16 if logits.dtype == torch.bfloat16 else L.MOPK_F32
    a.row0, a.n_rows = row0, targets.shape[0]
    a.ignore_index = max(-2 ** 63, min(2 ** 63 - 1, ignore_index))
    a.logits, a.logits_ld = logits.data_ptr(), a.V if a.R == 1 else logits.stride(0)   # a single row: its stride is never used
    a.targets = targets.data_ptr()
    return a


def _ce_accept(logits, targets, ignore_index):
    """the args struct of a call that mopk_cross_entropy_* take, None of one they refuse"""
    if not _stat_logits_ok(logits) or not (targets.is_cuda and targets.is_contiguous()) or logits.shape[0] >= 2 ** 31:
        return None
    a = _ce_args(logits, targets, ignore_index)
    return a if L.lib().mopk_cross_entropy_supported(C.byref(a)) else None


def _ce_grad_like(logits: torch.Tensor) -> torch.Tensor:
    """an empty (R, V) tensor laid out as the backward kernel needs it: every row sits as its row of `logits` does relative to a
    16-byte boundary (the same row stride, or the smallest one >= V equal to it modulo a vector where the logits are a narrow
    slice of a wide buffer).  Contiguous logits on a boundary get a contiguous tensor."""
    R, V = logits.shape
    epv = 16 // logits.element_size()
    ld = V if R == 1 else logits.stride(0)
    if ld - V >= epv:
        ld = V + (ld - V) % epv
    phase = (logits.data_ptr() % 16) // logits.element_size()
    buf = torch.empty(phase + (R - 1) * ld + V, dtype=logits.dtype, device=logits.device)
    return buf.as_strided((R, V), (ld, 1), buf.storage_offset() + phase)


def cross_entropy_supported(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100, reduction: str = "mean") -> bool:
    """True if mopk_cross_entropy_* take this call: CUDA fp32 / bf16 logits with unit inner stride and a row stride >= V (one row:
    any), CUDA int64 targets (the library's own query decides the rest).  Raises ValueError on bad arguments."""
    _ce_check(logits, targets, ignore_index, reduction, "cross_entropy_supported")
    return _ce_accept(logits, targets.contiguous(), ignore_index) is not None


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100, reduction: str = "mean",
                  inplace_backward: bool = False) -> torch.Tensor:
    """cross-entropy of (R, V) logits against int64 (R,) targets -> fp32: a scalar for "mean" / "sum", (R,) for "none".

    Per row: lse - logits[r, t], lse = logsumexp of the row in fp32 (-inf entries add nothing).  A row whose target is ignore_index
    or lies outside [0, V) is ignored: loss 0, gradient exactly 0, not counted by "mean" (torch asserts on the device for a target
    outside the classes; here it is an ignored row).  "mean" over no counted row is NaN, as in torch.
    logits: fp32 or bf16, unit inner stride, any row stride >= V, rows starting at any element (`logits[:, 1:]`, a padded buffer).
    Differentiable in the logits, once.  The gradient g (softmax - onehot) comes in the logits' dtype, as a new tensor whose rows
    are laid out like the logits'; with inplace_backward=True it is written over the logits themselves: the caller promises that
    nothing reads them after this call (a second backward through the same graph then raises).
    Runs the HIP kernels (mopk_cross_entropy_fwd: a row kernel and, for "mean" / "sum", a one-workgroup reduce; _bwd: one launch)
    when cross_entropy_supported() accepts the call, else cross_entropy_torch() (CPU tensors, fp16, other strides);
    LAST_PATH["cross_entropy_fwd"] / ["cross_entropy_bwd"] record which.  No host sync; bitwise reproducible; a row comes out bit
    for bit as it would alone."""
    _ce_check(logits, targets, ignore_index, reduction, "cross_entropy")
    targets = targets.contiguous()
    if _ce_accept(logits, targets, ignore_index) is None:
        LAST_PATH["cross_entropy_fwd"] = LAST_PATH["cross_entropy_bwd"] = L.PATH_GENERIC
        return cross_entropy_torch(logits, targets, ignore_index, reduction)
    return _cross_entropy_fn._CrossEntropyFn.apply(logits, targets, ignore_index, reduction, bool(inplace_backward))


def _lce_check(x, weight, targets, bias, ignore_index, reduction, chunk_rows, what: str):
    """validate a linear_cross_entropy call -> (M, D, V)"""
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or not x.dtype.is_floating_point or x.numel() == 0:
        raise ValueError(f"{what}: x must be a non-empty floating (..., D) tensor")
    D = x.shape[-1]
    M = x.numel() // D
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2 or weight.shape[1] != D or weight.shape[0] < 2:
        raise ValueError(f"{what}: weight must be a (V >= 2, D = {D}) tensor, got {tuple(getattr(weight, 'shape', ()))}")
    V = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (V,):
        raise ValueError(f"{what}: bias must be a ({V},) tensor, got {tuple(bias.shape)}")
    if not isinstance(targets, torch.Tensor) or targets.numel() != M or targets.dtype != torch.long:
        raise ValueError(f"{what}: targets must be an int64 tensor of {M} elements, one per row of x")
    if any(t is not None and t.device != x.device for t in (weight, bias, targets)):
        raise ValueError(f"{what}: x, weight, bias and targets must be on one device")
    if not _is_index(ignore_index):
        raise ValueError(f"{what}: ignore_index must be an int, got {ignore_index!r}")
    if reduction not in CE_REDUCTIONS:
        raise ValueError(f"{what}: reduction must be one of {CE_REDUCTIONS}, got {reduction!r}")
    if chunk_rows is not None and (not _is_index(chunk_rows) or chunk_rows < 1):
        raise ValueError(f"{what}: chunk_rows must be a positive int or None, got {chunk_rows!r}")
    return M, D, V


def _lce_dtype(x: torch.Tensor, weight: torch.Tensor) -> Optional[torch.dtype]:
    """the dtype F.linear(x, weight) computes and returns in: the autocast dtype under autocast, else the operands' common one
    (None: they differ, and F.linear itself raises)"""
    if x.is_cuda and torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return x.dtype if x.dtype == weight.dtype else None


def linear_cross_entropy_torch(x, weight, targets, bias=None, ignore_index=-100, reduction="mean", chunk_rows=None) -> torch.Tensor:
    """the restatement of `linear_cross_entropy` in torch ops and torch's autograd: F.linear and cross_entropy_torch's row losses
    chunk by chunk, summed once over all rows.  One chunk is F.cross_entropy(F.linear(x, weight, bias).float(), ...) itself.
    Autograd keeps every chunk's logits: this path saves no memory."""
    M, D, V = _lce_check(x, weight, targets, bias, ignore_index, reduction, chunk_rows, "linear_cross_entropy_torch")
    x2, t = x.reshape(M, D), targets.reshape(M)
    c = min(M, chunk_rows or LINEAR_CE_CHUNK_ROWS)
    if c >= M:
        return cross_entropy_torch(F.linear(x2, weight, bias), t, ignore_index, reduction)
    rows = torch.cat([cross_entropy_torch(F.linear(x2[i:i + c], weight, bias), t[i:i + c], ignore_index, "none") for i in range(0, M, c)])
    if reduction == "none":
        return rows
    return rows.sum() if reduction == "sum" else rows.sum() / _ce_counted(t, V, ignore_index).sum()


def linear_cross_entropy(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, bias: Optional[torch.Tensor] = None,
                         ignore_index: int = -100, reduction: str = "mean", chunk_rows: Optional[int] = None) -> torch.Tensor:
    """cross_entropy(F.linear(x, weight, bias), targets) -> fp32, holding at most chunk_rows x V logits at a time.

    x: (..., D), weight: (V, D), bias: (V,) or None, targets: int64, one per row of x; the M rows of x are taken chunk_rows at a
    time (None: LINEAR_CE_CHUNK_ROWS).  Per chunk: one GEMM for the logits (torch; in the autocast dtype under autocast, as F.linear
    would), mopk_cross_entropy_fwd on them and, when x, weight or bias requires grad, mopk_cross_entropy_bwd over the same storage
    (upstream 1, times 1 / n_valid for "mean"), then dx_c = g_c @ W and dW += g_c^T @ x_c, db += sum g_c.  dW and db are accumulated
    in fp32 across the chunks and rounded once to the parameter's dtype.  The loss is the fixed-order sum over all M row losses: it
    depends on the chunking only through what the GEMM itself does.  backward returns the stored gradients times the upstream
    scalar as new tensors (retain_graph works).  Ignored rows as in `cross_entropy`.
    The fused path takes CUDA fp32 / bf16 logits and reduction "mean" / "sum"; anything else ("none", CPU, fp16) runs
    linear_cross_entropy_torch().  LAST_PATH["linear_cross_entropy"] records which; the fused path also records
    LAST_PATH["cross_entropy_fwd"] / ["cross_entropy_bwd"].  No host sync."""
    M, D, V = _lce_check(x, weight, targets, bias, ignore_index, reduction, chunk_rows, "linear_cross_entropy")
    ldt = _lce_dtype(x, weight)
    if (not x.is_cuda or ldt not in (torch.float32, torch.bfloat16) or reduction == "none" or M >= 2 ** 31
            or (bias is not None and not torch.is_autocast_enabled("cuda") and bias.dtype != ldt)):
        LAST_PATH["linear_cross_entropy"] = L.PATH_GENERIC
        return linear_cross_entropy_torch(x, weight, targets, bias, ignore_index, reduction, chunk_rows)
    LAST_PATH["linear_cross_entropy"] = L.PATH_FUSED
    return _cross_entropy_fn._LinearCrossEntropyFn.apply(x, weight, bias, targets.reshape(M).contiguous(), ignore_index, reduction,
                                                         min(M, chunk_rows or LINEAR_CE_CHUNK_ROWS), ldt)


# ---- fused AdamW step: gradient norm, clipping, update, weight EMA (mopk_adamw_*; mop_amd.optim.FusedAdamW holds the state) ----
# A step is a list of groups.  A group is a dict: "params", "grads", "exp_avgs", "exp_avg_sqs", "steps" (lists of equal length;
# exp_avg / exp_avg_sq fp32, step an fp32 scalar tensor), "emas" (a list, or None without an EMA), "lr" (a float or a one-element
# fp32 tensor), "beta1", "beta2", "eps", "weight_decay".  `stats` is the int32 (4,) tensor behind MopkAdamWStats.
ADAMW_GROUP_KEYS = ("params", "grads", "exp_avgs", "exp_avg_sqs", "steps", "emas", "lr", "beta1", "beta2", "eps", "weight_decay")


def _adamw_check(groups, max_grad_norm, ema_decay, stats, what: str) -> None:
    """validate an adamw_step call before any device work"""
    if not isinstance(stats, torch.Tensor) or stats.dtype != torch.int32 or tuple(stats.shape) != (4,) or not stats.is_contiguous():
        raise ValueError(f"{what}: stats must be a contiguous int32 (4,) tensor")
    if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
        raise ValueError(f"{what}: max_grad_norm must be positive, got {max_grad_norm!r}")
    if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
        raise ValueError(f"{what}: ema_decay must lie in [0, 1], got {ema_decay!r}")
    for g in groups:
        missing = [k for k in ADAMW_GROUP_KEYS if k not in g]
        if missing:
            raise ValueError(f"{what}: a group lacks {missing}")
        n = len(g["params"])
        lists = [g["grads"], g["exp_avgs"], g["exp_avg_sqs"], g["steps"]] + ([g["emas"]] if ema_decay is not None else [])
        if any(x is None or len(x) != n for x in lists):
            raise ValueError(f"{what}: the tensor lists of a group must have one entry per parameter ({n})")
        for i, p in enumerate(g["params"]):
            if p.is_complex() or not p.dtype.is_floating_point:
                raise ValueError(f"{what}: parameters must be real floating tensors, got {p.dtype}")
            if g["grads"][i].is_sparse:
                raise ValueError(f"{what}: sparse gradients are not supported")
            if g["grads"][i].shape != p.shape or any(x[i].shape != p.shape for x in lists[1:3] + lists[4:]):
                raise ValueError(f"{what}: gradient, moments and EMA must have the parameter's shape {tuple(p.shape)}")
            if p.device != stats.device:
                raise ValueError(f"{what}: a parameter is on {p.device}, the stats on {stats.device}: one step updates one device")


def _adamw_scalar(x, device) -> torch.Tensor:
    return x.detach().reshape(()).double() if isinstance(x, torch.Tensor) else torch.tensor(float(x), dtype=torch.float64, device=device)


def adamw_step_torch(groups, *, max_grad_norm=None, ema_decay=None, skip_nonfinite=False, stats: torch.Tensor) -> None:
    """the restatement of `adamw_step` in torch ops, tensor by tensor, without a host sync: include/mopk.h's formulae in fp32 with
    the constants rounded from double, the global norm as clip_grad_norm_ takes it (the norm of the tensors' norms), a skipped step
    by torch.where.  exp_avg and exp_avg_sq are fp32; any floating parameter and gradient dtype, any strides."""
    _adamw_check(groups, max_grad_norm, ema_decay, stats, "adamw_step_torch")
    dev, f32 = stats.device, torch.float32
    use_norm = max_grad_norm is not None or skip_nonfinite
    coef = keep = None
    with torch.no_grad():
        if use_norm:
            norms = [torch.linalg.vector_norm(x.detach().float()) for g in groups for x in g["grads"]]
            norm = torch.linalg.vector_norm(torch.stack(norms)) if norms else torch.zeros((), dtype=f32, device=dev)
            coef = torch.ones_like(norm) if max_grad_norm is None else torch.clamp(float(max_grad_norm) / (norm + 1e-6), max=1.0)
            skip = ~torch.isfinite(norm) if skip_nonfinite else torch.zeros((), dtype=torch.bool, device=dev)
            fstats = stats.view(f32)
            fstats[0], fstats[1], stats[2] = norm, coef, skip.to(torch.int32)
            stats[3] += skip.to(torch.int32)
            keep = ~skip if skip_nonfinite else None
        for g in groups:
            lr, b1, b2 = _adamw_scalar(g["lr"], dev), float(g["beta1"]), float(g["beta2"])
            decay = (1.0 - lr * float(g["weight_decay"])).to(f32)
            b1f, omb1, b2f, omb2 = (torch.tensor(x, dtype=torch.float64).to(f32).item() for x in (b1, 1.0 - b1, b2, 1.0 - b2))
            eps = torch.tensor(float(g["eps"]), dtype=torch.float64).to(f32).item()
            for i, p in enumerate(g["params"]):
                p, m, v, step = p.detach(), g["exp_avgs"][i], g["exp_avg_sqs"][i], g["steps"][i]
                k = step.double() + 1.0
                step_size = (lr / (1.0 - torch.pow(torch.tensor(b1, dtype=torch.float64, device=dev), k))).to(f32)
                sqrt_bc2 = torch.sqrt(1.0 - torch.pow(torch.tensor(b2, dtype=torch.float64, device=dev), k)).to(f32)
                gp = g["grads"][i].detach().to(f32)
                if coef is not None:
                    gp = coef * gp
                m_new = b1f * m + omb1 * gp
                v_new = b2f * v + (omb2 * gp) * gp
                pf = p.to(f32) * decay
                p_new = (pf - step_size * (m_new / (torch.sqrt(v_new) / sqrt_bc2 + eps))).to(p.dtype)
                new = [(p, p_new), (m, m_new), (v, v_new), (step, step + 1.0)]
                if ema_decay is not None:
                    d, omd = (torch.tensor(x, dtype=torch.float64).to(f32).item() for x in (float(ema_decay), 1.0 - float(ema_decay)))
                    e = g["emas"][i]
                    new.append((e, (d * e.to(f32) + omd * p_new.to(f32)).to(e.dtype)))
                for old, val in new:
                    old.copy_(val if keep is None else torch.where(keep, val, old))


def _adamw_dtype(t: torch.Tensor):
    return {torch.float32: L.MOPK_F32, torch.bfloat16: L.MOPK_BF16}.get(t.dtype)


def _adamw_accept(groups, max_grad_norm, ema_decay, skip_nonfinite, stats, cache=None):
    """the (args, tensor array) pairs of a step that mopk_adamw_* take -- first the norm call over all tensors when one is needed,
    then one update call per group -- or None of a step they refuse.  `cache` (a dict the caller keeps) saves rebuilding the tensor
    arrays while no pointer changes."""
    if not stats.is_cuda:
        return None
    use_ema, dev = ema_decay is not None, stats.device
    rows = []
    for g in groups:
        lr = g["lr"]
        if isinstance(lr, torch.Tensor) and not (lr.is_cuda and lr.device == dev and lr.dtype == torch.float32 and lr.numel() == 1):
            return None
        for i, p in enumerate(g["params"]):
            gr, m, v, st = g["grads"][i], g["exp_avgs"][i], g["exp_avg_sqs"][i], g["steps"][i]
            e = g["emas"][i] if use_ema else None
            ts = [p, gr, m, v, st] + ([e] if use_ema else [])
            if (_adamw_dtype(p) is None or _adamw_dtype(gr) is None or m.dtype != torch.float32 or v.dtype != torch.float32
                    or st.dtype != torch.float32 or st.numel() != 1 or (use_ema and e.dtype != p.dtype)
                    or not all(t.device == dev and t.layout == torch.strided and t.is_contiguous() for t in ts)):
                return None
            rows.append((p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if use_ema else None, st.data_ptr(),
                         p.numel(), _adamw_dtype(p), _adamw_dtype(gr)))
    key = (tuple(rows), tuple(len(g["params"]) for g in groups))
    if cache is not None and cache.get("key") == key:
        arrays, whole = cache["arrays"], cache["whole"]
    else:
        whole = (L.OptimTensor * max(len(rows), 1))()
        for j, r in enumerate(rows):
            t = whole[j]
            t.p, t.g, t.m, t.v, t.ema, t.step, t.n, t.p_dtype, t.g_dtype = r
        arrays, o = [], 0
        for g in groups:
            n = len(g["params"])
            arrays.append((L.OptimTensor * max(n, 1)).from_buffer(whole, o * C.sizeof(L.OptimTensor)) if n else None)
            o += n
        if cache is not None:
            cache.update(key=key, arrays=arrays, whole=whole, ws=None)
    lib, calls = L.lib(), []
    use_norm = max_grad_norm is not None or skip_nonfinite
    if use_norm:
        a = L.AdamWArgs()
        a.n_tensors, a.phases, a.clip, a.skip_nonfinite = len(rows), L.ADAMW_NORM, max_grad_norm is not None, bool(skip_nonfinite)
        a.max_norm, a.stats = float(max_grad_norm or 0.0), stats.data_ptr()
        ws = cache.get("ws") if cache is not None else None
        if ws is None:
            ws = torch.empty(lib.mopk_adamw_workspace_bytes(C.byref(a), whole) // 4, dtype=torch.float32, device=dev)
            if cache is not None:
                cache["ws"] = ws
        a.workspace = ws.data_ptr()
        calls.append((a, whole, ws))
    for g, arr in zip(groups, arrays):
        if arr is None:
            continue
        a = L.AdamWArgs()
        a.n_tensors, a.phases, a.use_norm, a.use_ema = len(g["params"]), L.ADAMW_UPDATE, use_norm, use_ema
        lr = g["lr"]
        if isinstance(lr, torch.Tensor):
            a.lr_dev = lr.data_ptr()
        else:
            a.lr = float(lr)
        a.beta1, a.beta2, a.eps, a.weight_decay = float(g["beta1"]), float(g["beta2"]), float(g["eps"]), float(g["weight_decay"])
        a.ema_decay, a.stats = float(ema_decay or 0.0), stats.data_ptr()
        calls.append((a, arr, lr))
    if not all(lib.mopk_adamw_supported(C.byref(a), arr) for a, arr, _ in calls):
        return None
    return calls


def adamw_supported(groups, *, max_grad_norm=None, ema_decay=None, skip_nonfinite=False, stats: torch.Tensor) -> bool:
    """True if mopk_adamw_step takes this step: every tensor CUDA, on one device, contiguous; parameters, gradients and EMA fp32
    or bf16; fp32 moments and step counts (the library's own query decides the rest).  Raises ValueError on bad arguments."""
    _adamw_check(groups, max_grad_norm, ema_decay, stats, "adamw_supported")
    return _adamw_accept(groups, max_grad_norm, ema_decay, skip_nonfinite, stats) is not None


def adamw_launches(groups, *, max_grad_norm=None, ema_decay=None, skip_nonfinite=False, stats: torch.Tensor) -> int:
    """kernel launches `adamw_step` makes for this step on the fused path (mopk_adamw_launches), 0 for a step it refuses"""
    calls = _adamw_accept(groups, max_grad_norm, ema_decay, skip_nonfinite, stats)
    return 0 if calls is None else sum(L.lib().mopk_adamw_launches(C.byref(a), arr) for a, arr, _ in calls)


def adamw_step(groups, *, max_grad_norm=None, ema_decay=None, skip_nonfinite=False, stats: torch.Tensor, cache=None) -> None:
    """One AdamW step over all tensors of `groups`, in place: the global gradient norm and clip coefficient when max_grad_norm or
    skip_nonfinite asks for them (stats: norm, coef, skip, skipped), the decoupled-weight-decay update with fp32 moments, the weight
    EMA with ema_decay, step counts + 1.  Gradients are never written.  With skip_nonfinite a non-finite norm leaves every tensor
    and count as it was.  Runs mopk_adamw_step (the launch count is mopk_adamw_launches) when adamw_supported() accepts the step,
    else adamw_step_torch(); LAST_PATH["adamw"] records which.  No host sync, no host-to-device copy."""
    _adamw_check(groups, max_grad_norm, ema_decay, stats, "adamw_step")
    calls = _adamw_accept(groups, max_grad_norm, ema_decay, skip_nonfinite, stats, cache)
    if calls is None:
        LAST_PATH["adamw"] = L.PATH_GENERIC
        return adamw_step_torch(groups, max_grad_norm=max_grad_norm, ema_decay=ema_decay, skip_nonfinite=skip_nonfinite, stats=stats)
    LAST_PATH["adamw"] = L.PATH_FUSED
    st = _stream()
    for a, arr, _ in calls:
        L.check(L.lib().mopk_adamw_step(C.byref(a), arr, st), "mopk_adamw_step")


from . import mel_gate_fn as _mel_gate_fn  # noqa: E402  (it reads this module's helpers, all defined by now)
from . import cross_entropy_fn as _cross_entropy_fn  # noqa: E402  (likewise)
from . import gpt_lens_fn as _gpt_lens_fn  # noqa: E402  (likewise)
