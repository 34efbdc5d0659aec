"""Quartet dual-path causal attention with the reference surface (mop/models/quartet_attn_patch.py:19-127), and the
Quartet language model around it (`MLP`, `Block`, `TinyTransformerLM`, :130-213).

The five/three Linear projections stay in PyTorch (hipBLASLt); scores, row z-normalisation, product
mix, causal + additive mask, softmax and AV are one libmopk call (mopk_quartet_*).

Right-padded batches: the attention and the blocks take `lens`, an int32 (B,) tensor of per-row lengths (mopk_quartet_lens_*),
and the language models take a list of 1-D token tensors, which they pad themselves (their forward / loss keep the reference's
parameters).  Each row then comes out as it would alone: the row statistics of the attention see the row's own keys only.
`lens` and `attention_mask` do not combine.
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

    def forward(self, x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, need_weights: bool = False,
                lens: Optional[torch.Tensor] = None):
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
                               self.config.score_norm_eps, uq, need_weights, dropout_p=pdrop, lens=lens)
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

    def forward(self, x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = x + self.attn(self.ln1(x), attention_mask=attention_mask, lens=lens)
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

    def _batch(self, idx, targets=None, ignore_index: int = -100):
        """(idx (B,T), targets or None, lens or None) of a call.  A list of B 1-D token tensors is right-padded with token 0 to the
        longest and its lengths go to the device once (pinned, non-blocking: no synchronisation); a list of targets is padded
        with ignore_index.  A list of equal lengths is the stacked tensor without lengths: the tensor path bit for bit.  With
        lengths, tensor targets at positions >= lens[b] count as ignore_index (the logits there are unspecified).  A tensor idx
        is passed through untouched."""
        dev = self.wte.weight.device
        lens = None
        if isinstance(idx, (list, tuple)):
            if len(idx) == 0 or any(t.dim() != 1 for t in idx):
                raise ValueError("a list of token tensors must hold B >= 1 tensors of shape (T_b,)")
            n = [int(t.shape[0]) for t in idx]
            if isinstance(targets, (list, tuple)):
                if [int(t.shape[0]) for t in targets] != n:
                    raise ValueError("targets must have the lengths of the token tensors")
                targets = nn.utils.rnn.pad_sequence(list(targets), batch_first=True, padding_value=ignore_index).to(dev)
            if min(n) != max(n):
                lens = torch.tensor(n, dtype=torch.int32)
                if dev.type == "cuda":
                    lens = lens.pin_memory().to(dev, non_blocking=True)
            idx = nn.utils.rnn.pad_sequence(list(idx), batch_first=True, padding_value=0).to(dev)
        elif isinstance(targets, (list, tuple)):
            raise ValueError("a list of targets goes with a list of token tensors")
        if lens is not None and targets is not None:
            keep = torch.arange(targets.shape[1], device=targets.device).view(1, -1) < lens.to(targets.device).view(-1, 1)
            targets = torch.where(keep, targets, torch.full((), ignore_index, dtype=targets.dtype, device=targets.device))
        return idx, targets, lens

    def _stack(self, idx, attention_mask, lens) -> torch.Tensor:
        """embedding and blocks: the head's input"""
        x = self._embed(idx)
        for block in self.blocks:
            # the call without lengths stays the call of before: a block need not know the argument
            x = block(x, attention_mask=attention_mask) if lens is None else block(x, attention_mask=attention_mask, lens=lens)
        return x

    def _head(self, x: torch.Tensor, targets: Optional[torch.Tensor]):
        logits = self.lm_head(self.ln_f(x))
        loss = None
        if targets is not None:
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1))
        return logits, loss

    def forward(self, idx, attention_mask: Optional[torch.Tensor] = None, targets=None):
        """(logits, loss or None).  idx: (B,T) token ids, or a list of B 1-D token tensors of different lengths (right-padded here,
        see _batch): then every document comes out as it would alone, logits at positions beyond a document's length are
        unspecified but finite, and the loss is the mean over the non-ignored targets of the batch."""
        idx, targets, lens = self._batch(idx, targets)
        return self._head(self._stack(idx, attention_mask, lens), targets)

    def loss(self, idx, targets, attention_mask: Optional[torch.Tensor] = None, *,
             chunk_rows: Optional[int] = None, ignore_index: int = -100) -> torch.Tensor:
        """the mean cross-entropy that forward(idx, attention_mask, targets)[1] returns, without the (B T, V) logits: the stack as
        in forward, then ops.linear_cross_entropy on the head's input, chunk_rows rows of logits at a time.  Lists of documents
        and targets as in forward."""
        idx, targets, lens = self._batch(idx, targets, ignore_index)
        x = self._stack(idx, attention_mask, lens)
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
