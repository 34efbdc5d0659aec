"""GPT-MoP with the reference's constructors, forward, get_gate_maps and state_dict (mop/models/gpt_mop.py).

Every `MoPBlock` gates the residual stream between attention and MLP.  The reference writes that gate as a Linear, a 3-tap
conv1d, a concatenation, a 1x1 conv1d and the excitatory / inhibitory weights (:89-123); it is linear in the residual stream,
so the block folds it into three taps (`ops.token_gate_taps`, a 3 x D computation under autograd) and runs the residual add,
the gate and the multiply as one HIP kernel (`ops.token_gate_1d`, mopk_token_gate_*).  Calls the kernels do not take (CPU
tensors, fp16, D % 8 != 0, D > 1024) run the reference's composition; `get_gate_maps` always does.

The 3-tap conv is not causal (zero padding 1 on both sides, as in the reference): the gate of token t reads r_{t+1}, so a model
built this way sees one token ahead.  Kept for parity with the reference.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import _lib, ops
from .quartet_attn_patch import MLP, CausalSelfAttention, TinyTransformerLM, TransformerConfig, _LMBase


class ViewsLinear1D(nn.Module):
    """(B,T,D) -> (B,V,T) token views (reference :19-31)"""

    def __init__(self, dim, n_views=5):
        super().__init__()
        self.n_views = n_views
        self.proj = nn.Linear(dim, n_views, bias=False)

    def forward(self, tok):
        return self.proj(tok).transpose(1, 2)


class Kernels1D(nn.Module):
    """(B,V,T) -> (B,K,T), a conv1d with zero padding kernel_size // 2 on both sides (reference :34-45)"""

    def __init__(self, in_ch, n_kernels=3, kernel_size=3):
        super().__init__()
        self.n_kernels = n_kernels
        self.conv = nn.Conv1d(in_ch, n_kernels, kernel_size, padding=kernel_size // 2, bias=False)

    def forward(self, x):
        return self.conv(x)


class FuseExcInh1D(nn.Module):
    """(B,V+K,T) -> (g_pos, g_neg, alpha_pos, alpha_neg): a 1x1 conv1d to two channels and two plain weights (reference :48-68)"""

    def __init__(self, in_ch):
        super().__init__()
        self.conv = nn.Conv1d(in_ch, 2, kernel_size=1, bias=False)
        self.alpha = nn.Parameter(torch.ones(2))

    def forward(self, x):
        g = self.conv(x)
        return g[:, :1], g[:, 1:], self.alpha[0], self.alpha[1]


class MoPBlock(nn.Module):
    """x + attn(ln1(x)), gated by the token gate, then + mlp(ln2(.)) (reference :71-138)"""

    def __init__(self, config: TransformerConfig, n_views=5, n_kernels=3):
        super().__init__()
        self.ln1 = nn.LayerNorm(config.n_embd)
        self.attn = CausalSelfAttention(config)
        self.ln2 = nn.LayerNorm(config.n_embd)
        self.mlp = MLP(config)
        self.views = ViewsLinear1D(config.n_embd, n_views=n_views)
        self.kernels = Kernels1D(in_ch=n_views, n_kernels=n_kernels)
        self.fuse = FuseExcInh1D(in_ch=n_views + n_kernels)
        self.n_views = n_views
        self.n_kernels = n_kernels

    def forward(self, x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = self._gated_residual(x, self.attn(self.ln1(x), attention_mask=attention_mask, lens=lens), lens)
        return x + self.mlp(self.ln2(x))

    def taps(self) -> torch.Tensor:
        """the gate folded into three taps u (3, D) fp32 (ops.token_gate_taps)"""
        return ops.token_gate_taps(self.views.proj.weight, self.kernels.conv.weight, self.fuse.conv.weight, self.fuse.alpha)

    def _gate_torch(self, x):
        V = self.views(x)
        K = self.kernels(V)
        g_pos, g_neg, a_pos, a_neg = self.fuse(torch.cat([V, K], dim=1))
        return 1 + a_pos * g_pos - a_neg * g_neg, V, K                 # (B,1,T)

    @staticmethod
    def _zero_tail(r: torch.Tensor, lens: Optional[torch.Tensor]) -> torch.Tensor:
        """r (B,T,D) with the rows t >= lens[b] set to 0 (whatever they hold): what the gate of a right-padded row reads there"""
        if lens is None:
            return r
        keep = torch.arange(r.shape[1], device=r.device).view(1, -1) < lens.to(r.device).view(-1, 1)
        return torch.where(keep.unsqueeze(-1), r, torch.zeros((), dtype=r.dtype, device=r.device))

    def _gated_residual(self, x: torch.Tensor, a: Optional[torch.Tensor], lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(x + a) * gate(x + a): one kernel where the library takes the call, the reference's composition otherwise.  lens: the
        residual stream counts as 0 beyond a row's length, so its last token reads no padding and padding rows come out 0"""
        if self.kernels.conv.kernel_size[0] == 3 and ops.token_gate_supported(x, a, lens):
            return ops.token_gate_1d(x, a, self.taps(), lens)
        ops.LAST_PATH["token_gate_fwd"] = _lib.PATH_GENERIC
        r = self._zero_tail(x if a is None else x + a, lens)
        return r * self._gate_torch(r)[0].transpose(1, 2)

    def apply_mop(self, x, lens: Optional[torch.Tensor] = None):
        """the token gate applied to x (B,T,D)"""
        return self._gated_residual(x, None, lens)

    def get_gate_maps(self, x, lens: Optional[torch.Tensor] = None):
        """(gate (B,1,T), views (B,V,T), kernels (B,K,T)) of x, in torch ops; lens: of x with the rows beyond a length set to 0"""
        return self._gate_torch(self._zero_tail(x, lens))


class GPT_MoP(_LMBase):
    """GPT-style language model of MoPBlocks (reference :141-249): forward(idx, attention_mask, targets) -> (logits, loss)"""

    def __init__(self, vocab_size: int, config: TransformerConfig, n_views=5, n_kernels=3):
        super().__init__()
        self.config = config
        self.n_views = n_views
        self.n_kernels = n_kernels
        self.wte = nn.Embedding(vocab_size, config.n_embd)
        self.wpe = nn.Embedding(config.block_size, config.n_embd) if config.use_abs_pos_emb else None
        self.drop = nn.Dropout(config.dropout)
        self.blocks = nn.ModuleList([MoPBlock(config, n_views=n_views, n_kernels=n_kernels) for _ in range(config.n_layer)])
        self.ln_f = nn.LayerNorm(config.n_embd)
        self.lm_head = nn.Linear(config.n_embd, vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight
        self.apply(self._init_weights)

    def get_gate_maps(self, x, lens: Optional[torch.Tensor] = None):
        """per-layer gate maps of token ids x (B,T): (gates (B,L,1,T), views (B,L,V,T), kernels (B,L,K,T)); no attention mask.
        x may be a list of 1-D token tensors as in forward, or come with int32 (B,) lengths: positions t < lens[b] are those of
        row b alone"""
        if isinstance(x, (list, tuple)):
            if lens is not None:
                raise ValueError("lens is taken from a list of token tensors: pass one or the other")
            x, _, lens = self._batch(x)
        h = self._embed(x)
        gates, views, kernels = [], [], []
        for block in self.blocks:
            r = h + (block.attn(block.ln1(h)) if lens is None else block.attn(block.ln1(h), lens=lens))
            g, V, K = block.get_gate_maps(r, lens)
            gates.append(g)
            views.append(V)
            kernels.append(K)
            h = block.apply_mop(r, lens)
            h = h + block.mlp(block.ln2(h))
        return torch.stack(gates, dim=1), torch.stack(views, dim=1), torch.stack(kernels, dim=1)


def create_gpt_mop(vocab_size: int, config: TransformerConfig, n_views=5, n_kernels=3):
    """GPT-MoP (reference :253-257)"""
    return GPT_MoP(vocab_size=vocab_size, config=config, n_views=n_views, n_kernels=n_kernels)


def _lm_config(config: TransformerConfig, use_quartet: bool) -> TransformerConfig:
    # the reference copies these six fields only (:260-284): the other fields, use_abs_pos_emb included, take their defaults
    return TransformerConfig(n_layer=config.n_layer, n_head=config.n_head, n_embd=config.n_embd, dropout=config.dropout,
                             block_size=config.block_size, bias=config.bias, use_quartet=use_quartet)


def create_gpt_baseline(vocab_size: int, config: TransformerConfig):
    """TinyTransformerLM without Quartet (z-normalised single-path attention) and without MoP (reference :260-271)"""
    return TinyTransformerLM(vocab_size=vocab_size, config=_lm_config(config, False))


def create_gpt_quartet(vocab_size: int, config: TransformerConfig):
    """TinyTransformerLM with Quartet attention, without MoP (reference :274-285)"""
    return TinyTransformerLM(vocab_size=vocab_size, config=_lm_config(config, True))
