"""Quartet dual-path causal attention with the reference surface (mop/models/quartet_attn_patch.py:19-127), and the
Quartet language model around it (`MLP`, `Block`, `TinyTransformerLM`, :130-213).

The five/three Linear projections stay in PyTorch (hipBLASLt); scores, row z-normalisation, product
mix, causal + additive mask, softmax and AV are one libmopk call (mopk_quartet_*).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .linear import TokenLinear


@dataclass
class TransformerConfig:
    n_layer: int = 6
    n_head: int = 8
    n_embd: int = 512
    dropout: float = 0.1
    block_size: int = 512
    bias: bool = False
    use_quartet: bool = True
    quartet_scale: float = 1.0
    quartet_gate_init: float = -5.0
    score_norm_eps: float = 1e-5
    use_abs_pos_emb: bool = True


class CausalSelfAttention(nn.Module):
    def __init__(self, config: TransformerConfig):
        super().__init__()
        assert config.n_embd % config.n_head == 0
        self.config = config
        self.n_head = config.n_head
        self.head_dim = config.n_embd // config.n_head
        self.scale = 1.0 / math.sqrt(self.head_dim)
        C = config.n_embd
        self.q_proj = TokenLinear(C, C, bias=config.bias)
        self.k_proj = TokenLinear(C, C, bias=config.bias)
        self.v_proj = TokenLinear(C, C, bias=config.bias)
        self.o_proj = TokenLinear(C, C, bias=config.bias)
        if config.use_quartet:
            self.q2_proj = TokenLinear(C, C, bias=config.bias)
            self.k2_proj = TokenLinear(C, C, bias=config.bias)
            self.mixture = nn.Parameter(torch.tensor([config.quartet_gate_init], dtype=torch.float32))
            self.quartet_scale = nn.Parameter(torch.tensor([config.quartet_scale], dtype=torch.float32))
        else:
            self.q2_proj = self.k2_proj = None
            self.register_parameter("mixture", None)
            self.register_parameter("quartet_scale", None)
        self.attn_drop = nn.Dropout(config.dropout)
        self.resid_drop = nn.Dropout(config.dropout)
        # kept for state/buffer parity with the reference (non-persistent); the kernel masks j > i itself
        self.register_buffer("causal_mask", torch.tril(torch.ones(config.block_size, config.block_size))
                             .view(1, 1, config.block_size, config.block_size), persistent=False)

    def forward(self, x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, need_weights: bool = False):
        B, T, C = x.shape
        H, Dh = self.n_head, self.head_dim
        pdrop = float(self.attn_drop.p) if self.training else 0.0      # attn_dropout on the probabilities (:119), inside the kernels
        if T > self.config.block_size:
            raise ValueError("Sequence length > block size")
        q = self.q_proj(x).view(B, T, H, Dh)
        k = self.k_proj(x).view(B, T, H, Dh)
        v = self.v_proj(x).view(B, T, H, Dh)
        uq = bool(self.config.use_quartet)
        q2 = self.q2_proj(x).view(B, T, H, Dh) if uq else None
        k2 = self.k2_proj(x).view(B, T, H, Dh) if uq else None
        out = ops.quartet_core(q, k, v, q2, k2, self.mixture, self.quartet_scale, attention_mask,
                               self.config.score_norm_eps, uq, need_weights, dropout_p=pdrop)
        y, attn = out if need_weights else (out, None)
        y = self.resid_drop(self.o_proj(y))
        return (y, attn) if need_weights else y


class MLP(nn.Module):
    """fc -> GELU(tanh) -> proj -> dropout (reference :130-143)"""

    def __init__(self, config: TransformerConfig):
        super().__init__()
        self.fc = TokenLinear(config.n_embd, 4 * config.n_embd, bias=config.bias)
        self.proj = TokenLinear(4 * config.n_embd, config.n_embd, bias=config.bias)
        self.drop = nn.Dropout(config.dropout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.drop(self.proj(F.gelu(self.fc(x), approximate="tanh")))


class Block(nn.Module):
    """pre-norm block: x + attn(ln1(x)), then x + mlp(ln2(x)) (reference :146-159)"""

    def __init__(self, config: TransformerConfig):
        super().__init__()
        self.ln1 = nn.LayerNorm(config.n_embd)
        self.attn = CausalSelfAttention(config)
        self.ln2 = nn.LayerNorm(config.n_embd)
        self.mlp = MLP(config)

    def forward(self, x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = x + self.attn(self.ln1(x), attention_mask=attention_mask)
        return x + self.mlp(self.ln2(x))


def _init_gpt_weights(module: nn.Module) -> None:
    """N(0, 0.02) for every Linear weight and Embedding, zero Linear biases (reference :177-183); convolutions keep torch's init"""
    if isinstance(module, nn.Linear):
        nn.init.normal_(module.weight, mean=0.0, std=0.02)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.normal_(module.weight, mean=0.0, std=0.02)


class _LMBase(nn.Module):
    """token (+ absolute position) embedding, a stack of blocks, final LayerNorm and the head tied to the token embedding"""

    def _embed(self, idx: torch.Tensor) -> torch.Tensor:
        T = idx.shape[1]
        if T > self.config.block_size:
            raise AssertionError("Sequence length > block size")
        x = self.wte(idx)
        if self.wpe is not None:
            x = x + self.wpe(torch.arange(T, dtype=torch.long, device=idx.device).unsqueeze(0))
        return self.drop(x)

    def _head(self, x: torch.Tensor, targets: Optional[torch.Tensor]):
        logits = self.lm_head(self.ln_f(x))
        loss = None
        if targets is not None:
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1))
        return logits, loss

    def loss(self, idx: torch.Tensor, targets: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, *,
             chunk_rows: Optional[int] = None, ignore_index: int = -100) -> torch.Tensor:
        """the mean cross-entropy that forward(idx, attention_mask, targets)[1] returns, without the (B T, V) logits: the stack as
        in forward, then ops.linear_cross_entropy on the head's input, chunk_rows rows of logits at a time"""
        x = self._embed(idx)
        for block in self.blocks:
            x = block(x, attention_mask=attention_mask)
        return ops.linear_cross_entropy(self.ln_f(x), self.lm_head.weight, targets, self.lm_head.bias,
                                        ignore_index=ignore_index, chunk_rows=chunk_rows)

    def _init_weights(self, module):
        _init_gpt_weights(module)


class TinyTransformerLM(_LMBase):
    """GPT-style LM on Quartet (or plain z-normalised) causal attention (reference :162-213): forward -> (logits, loss)"""

    def __init__(self, vocab_size: int, config: TransformerConfig):
        super().__init__()
        self.config = config
        self.wte = nn.Embedding(vocab_size, config.n_embd)
        self.wpe = nn.Embedding(config.block_size, config.n_embd) if config.use_abs_pos_emb else None
        self.drop = nn.Dropout(config.dropout)
        self.blocks = nn.ModuleList([Block(config) for _ in range(config.n_layer)])
        self.ln_f = nn.LayerNorm(config.n_embd)
        self.lm_head = nn.Linear(config.n_embd, vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight
        self.apply(self._init_weights)

    def forward(self, idx: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None):
        x = self._embed(idx)
        for block in self.blocks:
            x = block(x, attention_mask=attention_mask)
        return self._head(x, targets)
