"""The autograd Functions behind `ops.mel_gate` and `ops.gated_residual` (mopk_mel_gate_*, mopk_gated_residual_*).

`mop_amd/ops.py` holds the public ops, their torch twins, the support queries and the argument builders; the two Functions sit
here and reach the shared helpers through the module, so either module may be imported first."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import ops as O


class _MelGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mel, W, lens):
        g = O._mg_args(mel, W, lens)
        Wc = O._f32c(W)
        gates = torch.empty(g.B, g.L, g.T, dtype=torch.float32, device=mel.device)
        g.W, g.gates = Wc.data_ptr(), gates.data_ptr()
        O.LAST_PATH["mel_gate_fwd"] = L.PATH_FUSED
        O._launch("mopk_mel_gate_fwd", g, "mel_gate_fwd")
        ctx.save_for_backward(mel, lens)
        ctx.w_shape = tuple(W.shape)
        return gates

    @staticmethod
    @O._once_differentiable
    def backward(ctx, dgates):
        lib = L.lib()
        mel, lens = ctx.saved_tensors
        dW = torch.empty(ctx.w_shape, dtype=torch.float32, device=mel.device)
        g = O._mg_args(mel, dW, lens)
        dgates = O._grad_in(dgates, torch.float32)
        ws = O._bytes(lib.mopk_mel_gate_workspace_bytes(C.byref(g)), mel.device)
        g.dgates, g.dW, g.workspace = dgates.data_ptr(), dW.data_ptr(), ws.data_ptr()
        O.LAST_PATH["mel_gate_bwd"] = L.PATH_FUSED
        O._launch("mopk_mel_gate_bwd", g, "mel_gate_bwd")
        return None, dW, None


class _GatedResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, gate):
        g = O._gr_args(x, a, gate)
        odt = torch.float32 if g.o_dtype == L.MOPK_F32 else torch.bfloat16
        out = torch.empty(x.shape, dtype=odt, device=x.device)
        g.out = out.data_ptr()
        O.LAST_PATH["gated_residual_fwd"] = L.PATH_FUSED
        O._launch("mopk_gated_residual_fwd", g, "gated_residual_fwd")
        ctx.save_for_backward(x, a, gate)
        return out

    @staticmethod
    @O._once_differentiable
    def backward(ctx, dout):
        x, a, gate = ctx.saved_tensors
        g = O._gr_args(x, a, gate)
        odt = torch.float32 if g.o_dtype == L.MOPK_F32 else torch.bfloat16
        dout = O._grad_in(dout, odt)
        dr = torch.empty(x.shape, dtype=odt, device=x.device)
        dgate = torch.empty(x.shape[:2], dtype=torch.float32, device=x.device)
        g.dout, g.dr, g.dgate = dout.data_ptr(), dr.data_ptr(), dgate.data_ptr()
        O.LAST_PATH["gated_residual_bwd"] = L.PATH_FUSED
        O._launch("mopk_gated_residual_bwd", g, "gated_residual_bwd")
        dx = dr.to(x.dtype) if ctx.needs_input_grad[0] else None
        da = dr.to(a.dtype) if ctx.needs_input_grad[1] else None
        return dx, da, (dgate if ctx.needs_input_grad[2] else None)
