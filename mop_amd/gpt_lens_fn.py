"""The autograd Functions behind `ops.quartet_core(lens=)` and `ops.token_gate_1d(lens=)` (mopk_quartet_lens_*,
mopk_token_gate_lens_*): the GPT line over a batch of right-padded rows.

Each is its plain twin in `mop_amd/ops.py` with one more input, the int32 (B,) lengths, and shares that twin's forward and backward
(`ops._qt_fwd` / `_qt_bwd`, `ops._tg_fwd` / `_tg_bwd`), so the signatures of `_QuartetFn` and `_TokenGateFn` stay what they were."""
from __future__ import annotations

import torch

from . import ops as O


class _QuartetLensFn(torch.autograd.Function):
    """_QuartetFn over right-padded rows: no additive mask, per-row lengths read by the kernels"""

    @staticmethod
    def forward(ctx, q, k, v, q2, k2, mixture, qscale, lens, eps, use_quartet, need_weights, prec, path, drop=(0.0, 0)):
        return O._qt_fwd(ctx, q, k, v, q2, k2, mixture, qscale, None, lens, eps, use_quartet, need_weights, prec, path, drop)

    @staticmethod
    @O._once_differentiable
    def backward(ctx, dy, *unused):
        q = ctx.saved_tensors[0]
        return (*O._qt_bwd(ctx, O._grad_in(dy, q.dtype, q.shape)), None, None, None, None, None, None, None)


class _TokenGateLensFn(torch.autograd.Function):
    """_TokenGateFn over right-padded rows: per-row lengths read by the kernels"""

    @staticmethod
    def forward(ctx, x, a, u, lens):
        return O._tg_fwd(ctx, x, a, u, lens)

    @staticmethod
    @O._once_differentiable
    def backward(ctx, dout):
        return (*O._tg_bwd(ctx, O._grad_in(dout, ctx.o_dtype)), None)
