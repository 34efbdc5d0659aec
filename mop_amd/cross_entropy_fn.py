"""The autograd Functions behind `ops.cross_entropy` and `ops.linear_cross_entropy` (mopk_cross_entropy_*).

`mop_amd/ops.py` holds the public ops, their torch twins, the support queries and the argument builders; the two Functions sit
here and reach the shared helpers through the module, so either module may be imported first."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops as O


def _upstream(dloss: torch.Tensor, rows: int):
    """an upstream gradient as the backward kernel reads it -> (fp32 tensor, element stride between rows): a scalar is read by every
    row (stride 0), a per-row vector with its own stride (autograd hands over expanded and strided ones), copied only when it is
    not fp32 or not on a 4-byte boundary"""
    if dloss.dtype != torch.float32 or dloss.data_ptr() % 4 or (dloss.dim() == 1 and dloss.stride(0) < 0):
        dloss = O._grad_in(dloss, torch.float32)
    return dloss, (0 if dloss.dim() == 0 else dloss.stride(0) if rows > 1 else 0)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, ignore_index, reduction, inplace_backward):
        a = O._ce_args(logits, targets, ignore_index)
        dev = logits.device
        lse = torch.empty(a.R, dtype=torch.float32, device=dev)
        row_loss = torch.empty(a.R, dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev) if reduction != "none" else None
        a.lse, a.row_loss, a.out = lse.data_ptr(), row_loss.data_ptr(), O._ptr(out)
        O._row_launch(a, "mopk_cross_entropy_fwd", "cross_entropy_fwd")
        ctx.save_for_backward(logits, targets, lse, out)
        ctx.ignore_index, ctx.reduction, ctx.inplace, ctx.spent = ignore_index, reduction, inplace_backward, False
        return row_loss if reduction == "none" else out[2] if reduction == "mean" else out[0]

    @staticmethod
    @O._once_differentiable
    def backward(ctx, dloss):
        logits, targets, lse, out = ctx.saved_tensors
        if ctx.inplace and ctx.spent:
            raise RuntimeError("cross_entropy(inplace_backward=True): the first backward wrote the gradient over the logits; "
                               "a second one has nothing to read")
        ctx.spent = True
        a = O._ce_args(logits, targets, ctx.ignore_index)
        grad, stride = _upstream(dloss, a.R)
        dlogits = logits.detach() if ctx.inplace else O._ce_grad_like(logits)
        a.lse, a.grad, a.grad_stride = lse.data_ptr(), grad.data_ptr(), stride
        a.dlogits, a.dlogits_ld = dlogits.data_ptr(), a.V if a.R == 1 else dlogits.stride(0)
        if ctx.reduction == "mean":
            a.scale = out.data_ptr() + 3 * out.element_size()           # 1 / n_valid, left there by the forward's reduce
        O._row_launch(a, "mopk_cross_entropy_bwd", "cross_entropy_bwd")
        return dlogits, None, None, None, None


class _LinearCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, targets, ignore_index, reduction, chunk_rows, ldt):
        M, V, D, dev = targets.shape[0], weight.shape[0], weight.shape[1], x.device
        need = any(ctx.needs_input_grad[:3])
        with torch.autocast("cuda", enabled=False):                     # the casts autocast would make are made here, once
            xl, wl = x.detach().reshape(M, D).to(ldt), weight.detach().to(ldt)
            bl = None if bias is None else bias.detach().to(ldt)
            lse = torch.empty(M, dtype=torch.float32, device=dev)
            row_loss = torch.empty(M, dtype=torch.float32, device=dev)
            out = torch.empty(4, dtype=torch.float32, device=dev)
            if need:
                one = torch.ones(1, dtype=torch.float32, device=dev)
                inv_n = O._ce_counted(targets, V, ignore_index).sum().to(torch.float32).reciprocal() if reduction == "mean" else None
                dx = torch.empty(M, D, dtype=ldt, device=dev)
                dw = torch.zeros(V, D, dtype=torch.float32, device=dev)
                db = None if bias is None else torch.zeros(V, dtype=torch.float32, device=dev)
            for i in range(0, M, chunk_rows):
                xc = xl[i:i + chunk_rows]
                logits = F.linear(xc, wl, bl)
                a = O._ce_args(logits, targets, ignore_index, i)
                a.lse, a.row_loss = lse.data_ptr(), row_loss.data_ptr()
                a.out = out.data_ptr() if i + chunk_rows >= M else None  # the last chunk's call sums all M rows
                O._row_launch(a, "mopk_cross_entropy_fwd", "cross_entropy_fwd")
                if not need:
                    continue
                a.dlogits, a.dlogits_ld, a.grad, a.grad_stride, a.scale = a.logits, a.logits_ld, one.data_ptr(), 0, O._ptr(inv_n)
                O._row_launch(a, "mopk_cross_entropy_bwd", "cross_entropy_bwd")
                g = logits                                              # now the gradient of the chunk's logits
                torch.mm(g, wl, out=dx[i:i + chunk_rows])
                if ldt == torch.float32:
                    dw.addmm_(g.t(), xc)
                else:
                    dw += torch.mm(g.t(), xc, out_dtype=torch.float32)
                if db is not None:
                    db += g.sum(0, dtype=torch.float32)
        if need:
            ctx.save_for_backward(dx, dw, db)
        ctx.x_shape, ctx.dtypes = x.shape, (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        return out[2] if reduction == "mean" else out[0]

    @staticmethod
    @O._once_differentiable
    def backward(ctx, dloss):
        dx, dw, db = ctx.saved_tensors
        g = dloss.to(torch.float32)
        need, (xdt, wdt, bdt) = ctx.needs_input_grad, ctx.dtypes
        return ((dx * g).to(xdt).view(ctx.x_shape) if need[0] else None, (dw * g).to(wdt) if need[1] else None,
                (db * g).to(bdt) if need[2] and db is not None else None, None, None, None, None, None)
