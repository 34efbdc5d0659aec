"""Whisper-MoP with the reference's parameter names (mop/models/whisper_mop.py).

`MultiheadSelfAttention` (reference :137-177) and `MultiheadCrossAttention` (:180-221) run their attention cores in libmopk
(plain SDPA: the causal flag and the additive bias for self-attention; rectangular SDPA with Nk = T_audio
keys for cross-attention).  `EncoderBlock` (:241-264), `DecoderBlock` (:267-290), `WhisperMoP` (:296-424) and the factories
`create_whisper_mop` / `create_whisper_baseline` (:427-437) follow the reference's constructors, forward signatures, return values,
`state_dict` names and initialisation.  The mel-map gate `MoP2D` (:91-124, row a17) is linear in the mel map: the encoder folds
all layers' gates into taps and computes them in one launch (`ops.mel_gate`), and every block applies its gate together with the
residual add (`ops.gated_residual`).  The LayerNorms, the MLP and the embeddings are stock PyTorch-ROCm layers.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .linear import TokenLinear


@dataclass
class WhisperConfig:
    """reference :18-37 (same field names and defaults)."""
    n_mels: int = 80
    n_audio_ctx: int = 1500
    vocab_size: int = 51865
    n_text_ctx: int = 448
    n_embd: int = 1024
    n_head: int = 16
    n_layer_enc: int = 12
    n_layer_dec: int = 12
    dropout: float = 0.0
    bias: bool = False
    use_abs_pos_emb: bool = True
    n_views: int = 5
    n_kernels: int = 3
    kernel_size: int = 5


class EncodedAudio(NamedTuple):
    """encoder output of a batch of clips of different lengths (`WhisperMoP.encode` on a list of mel tensors).
    out: (B, T, D), right-padded to T = the longest clip; rows t >= lens[b] of item b are unspecified (finite, never read).
    lens: int32 (B,) device tensor of the clips' frame counts, or None when every clip has T frames (the uniform batch).
    `decode`, `init_decode_cache` and `DecoderBlock.forward` take it wherever they take the plain (B, T, D) tensor."""
    out: torch.Tensor
    lens: Optional[torch.Tensor]


class TokenAlignment(NamedTuple):
    """token-level timestamps of a batch (`WhisperMoP.align_tokens`), in encoder frames, all on the device.
    starts / ends: int32 (B, T): the first and last audio frame of token t of item b; -1 for the prompt, for the final token and
    for the padding.  n_tokens: int32 (B,), the lengths of the token sequences."""
    starts: torch.Tensor
    ends: torch.Tensor
    n_tokens: torch.Tensor


class WordAlignment(NamedTuple):
    """word-level timestamps of a batch (`WhisperMoP.align_words`), all on the device, N = T - prompt_len - 2 columns.
    starts / ends: int32 (B, N), the words' first frame and the frame the next word starts at; probs: fp32 (B, N), the mean
    probability of a word's own tokens; tok_begin / tok_end: int32 (B, N), the positions of the full token sequence a word spans
    (the end exclusive); n_words: int32 (B,).  At j >= n_words[b] the integers are -1 and probs is 0."""
    starts: torch.Tensor
    ends: torch.Tensor
    probs: torch.Tensor
    tok_begin: torch.Tensor
    tok_end: torch.Tensor
    n_words: torch.Tensor


class TranscriptWords(NamedTuple):
    """one clip's words (`transcribe(word_timestamps=True)`), all on the device, one entry per word in order.  starts / ends:
    int32, in frames of the CLIP; probs: fp32; tok_begin / tok_end: int32 indices into Transcript.tokens, the end exclusive (the
    timestamp tokens between two segments fall inside no word); segment: int64, the index of the segment the word begins in."""
    starts: torch.Tensor
    ends: torch.Tensor
    probs: torch.Tensor
    tok_begin: torch.Tensor
    tok_end: torch.Tensor
    segment: torch.Tensor


class _Words(NamedTuple):
    """transcribe's word timestamps, as checked by _words_check"""
    rules: "ops.WordRules"
    heads: List[Tuple[int, int]]
    medfilt_width: int
    median_cap: Optional[int]
    nots: int                            # logit_rules.no_timestamps_token_id


class Transcript(NamedTuple):
    """one clip's long-form transcription (`WhisperMoP.transcribe`), all on the device.  starts / ends: int32 (n,), the segments'
    first and last frame, in frames of the CLIP; tokens: (m,) in prompt_ids' dtype, the segments' tokens end to end, timestamp
    tokens included; offsets: int32 (n + 1,): segment i's tokens are tokens[offsets[i]:offsets[i + 1]]."""
    starts: torch.Tensor
    ends: torch.Tensor
    tokens: torch.Tensor
    offsets: torch.Tensor


class DecodeStats(NamedTuple):
    """a decoding's quality figures (`generate` / `beam_search` / `sample` with return_stats=True), all on the device.
    sum_logprobs: fp32 (B,) ((B, num_samples) from sample), the sum of log_softmax(logits)[token] over the generated tokens up to
    and including the first eos (under logit rules: of the FILTERED rows, Whisper's convention); n_tokens: int32, same shape, how
    many tokens that is: sum_logprobs / n_tokens is Whisper's avg_logprob; no_speech_prob: fp32 (B,), the probability of
    no_speech_token_id at prompt position sot_index, before any logit rule; None without a token id."""
    sum_logprobs: torch.Tensor
    n_tokens: torch.Tensor
    no_speech_prob: Optional[torch.Tensor]


class LanguageDetection(NamedTuple):
    """the language of a batch of clips (`WhisperMoP.detect_language`, and the last element of what `transcribe` returns with
    `languages`), on the device.  tokens: int32 (B,), each clip's most probable language token; probs: fp32 (B, n), the
    probabilities of the n language tokens in the ops.LanguageTokens' order (a softmax over them alone)."""
    tokens: torch.Tensor
    probs: torch.Tensor


class TranscribeLog(NamedTuple):
    """what `transcribe` decided for one clip's windows (return_log=True): host values, one entry per window, in order.
    seek: the window's first frame; temperature: the one whose result was kept; avg_logprob: sum_logprobs / n_tokens of it;
    no_speech_prob: NaN without a no_speech_token_id; compression_ratio: NaN without a callable; skipped: the no-speech skip
    dropped the window."""
    seek: List[int]
    temperature: List[float]
    avg_logprob: List[float]
    no_speech_prob: List[float]
    compression_ratio: List[float]
    skipped: List[bool]


class _Fallback(NamedTuple):
    """transcribe's per-window policy, as checked by _fallback_check"""
    temperatures: Tuple[float, ...]
    logprob_threshold: Optional[float]
    no_speech_threshold: Optional[float]
    no_speech_token_id: Optional[int]
    sot_index: int
    compression_ratio_threshold: Optional[float]
    compression_ratio: Optional[object]
    num_samples: int
    seed: int


class _Conditioning(NamedTuple):
    """transcribe's conditioning on the previous text, as checked by _condition_check"""
    on: bool                             # condition_on_previous_text
    n: int                               # the history cap
    prev: int                            # sot_prev_token_id
    seeds: Optional[List[torch.Tensor]]  # per clip: the initial prompt, or None
    reset_temperature: float


class _PreparedPrompts(NamedTuple):
    """a ragged prompt batch that is already padded (transcribe builds it on the device with ops.window_prompts), for the decoders'
    private entry points in place of the list form: ids (B, P) left-padded, kv_start int32 (B,) or None when every row fills P,
    lens: the rows' lengths on the host, max(lens) == P; every row ends with the same sot_len tokens, inside which sot_index
    counts.  The tokens come back as one (B, P + max_new_tokens) tensor, the padding included."""
    ids: torch.Tensor
    kv_start: Optional[torch.Tensor]
    lens: List[int]
    sot_len: int


class _Batch(NamedTuple):
    """what the prompt checks need to know of the audio batch when the mel is a list: shape[0] and device"""
    shape: Tuple[int, ...]
    device: torch.device


def _enc_parts(enc):
    """(out, lens) of an EncodedAudio; (enc, None) of a plain tensor"""
    return (enc.out, enc.lens) if isinstance(enc, EncodedAudio) else (enc, None)


class ViewsConv2D(nn.Module):
    def __init__(self, n_views: int):
        super().__init__()
        self.conv = nn.Conv2d(1, n_views, kernel_size=1, bias=False)

    def forward(self, mel2d):            # (B,1,T,F) -> (B,V,T,F)
        return self.conv(mel2d)


class Kernels2D(nn.Module):
    def __init__(self, in_ch: int, n_kernels: int, kernel_size: int):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, n_kernels, kernel_size, padding=kernel_size // 2, bias=False)

    def forward(self, x):                # (B,V,T,F) -> (B,K,T,F)
        return self.conv(x)


class FuseExcInh2D(nn.Module):
    def __init__(self, in_ch: int):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, 2, kernel_size=1, bias=False)
        self.alpha = nn.Parameter(torch.ones(2))          # (alpha_pos, alpha_neg), no squashing here (:84-88)

    def forward(self, x):
        g = self.conv(x)
        return g[:, 0:1], g[:, 1:2], self.alpha[0], self.alpha[1]


def _gate_dtype(mel: torch.Tensor) -> torch.dtype:
    """the dtype MoP2D's convolutions give the gate of this mel: autocast's where it is on, else the mel's own"""
    dev = mel.device.type
    return torch.get_autocast_dtype(dev) if torch.is_autocast_enabled(dev) else mel.dtype


def _stacked_taps(mops, n_mels: int) -> torch.Tensor:
    """ops.mel_gate_taps of several MoP2D modules at once -> (len(mops), k, n_mels)"""
    return ops.mel_gate_taps(torch.stack([m.views.conv.weight for m in mops]), torch.stack([m.kernels.conv.weight for m in mops]),
                             torch.stack([m.fuse.conv.weight for m in mops]), torch.stack([m.fuse.alpha for m in mops]), n_mels)


class MoP2D(nn.Module):
    """per-time-step gate 1 + a+ mean_F(g+) - a- mean_F(g-) from the raw mel map (reference :91-124).  The chain has no bias and
    no non-linearity, so `gate` folds it into k x n_mels taps (`ops.mel_gate_taps`) and runs the gate alone on the HIP kernel
    (`ops.mel_gate`); `forward` keeps the reference's convolutions for whoever wants the V / K maps."""

    def __init__(self, n_views: int, n_kernels: int, kernel_size: int):
        super().__init__()
        self.views = ViewsConv2D(n_views)
        self.kernels = Kernels2D(n_views, n_kernels, kernel_size)
        self.fuse = FuseExcInh2D(n_views + n_kernels)

    def taps(self, n_mels: int) -> torch.Tensor:
        """the gate folded into taps (1, k, n_mels) fp32 (ops.mel_gate_taps)"""
        return _stacked_taps([self], n_mels)

    def gate(self, mel2d: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward's gate_t (B,T,1) alone, without the maps: mel2d (B,1,T,F); lens: see ops.mel_gate"""
        g = ops.mel_gate(mel2d[:, 0], self.taps(mel2d.shape[3]), lens)
        return g.transpose(1, 2).to(_gate_dtype(mel2d))

    def forward(self, mel2d) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        V = self.views(mel2d)
        K = self.kernels(V)
        g_pos, g_neg, a_pos, a_neg = self.fuse(torch.cat([V, K], dim=1))
        gate_t = 1 + a_pos * g_pos.mean(dim=3) - a_neg * g_neg.mean(dim=3)      # (B,1,T)
        return gate_t.transpose(1, 2), V, K                                     # (B,T,1)


class MultiheadSelfAttention(nn.Module):
    """separate q/k/v/o Linears; softmax(q k^T / sqrt(dh) [causal] [+ attn_bias]) v in libmopk (reference :137-177)."""

    def __init__(self, dim: int, n_head: int, dropout: float, bias: bool, causal: bool):
        super().__init__()
        assert dim % n_head == 0
        self.dim, self.n_head, self.head_dim, self.causal = dim, n_head, dim // n_head, causal
        self.scale = self.head_dim ** -0.5
        self.q_proj = TokenLinear(dim, dim, bias=bias)
        self.k_proj = TokenLinear(dim, dim, bias=bias)
        self.v_proj = TokenLinear(dim, dim, bias=bias)
        self.o_proj = TokenLinear(dim, dim, bias=bias)
        self.attn_drop = nn.Dropout(dropout)
        self.resid_drop = nn.Dropout(dropout)

    def forward(self, x: torch.Tensor, attn_bias: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None):
        """lens: int32 (B,) device tensor for right-padded rows (tokens t >= lens[b] are padding: neither queries nor keys), or None"""
        pdrop = float(self.attn_drop.p) if self.training else 0.0      # dropout on the probabilities (:172), inside the kernels
        B, T, D = x.shape
        H, Dh = self.n_head, self.head_dim
        q, k, v = (p(x).view(B, T, H, Dh) for p in (self.q_proj, self.k_proj, self.v_proj))
        if lens is None:
            y = ops.sdpa_core(q, k, v, bias=attn_bias, causal=self.causal, dropout_p=pdrop)
        else:
            y = ops.sdpa_core(q, k, v, bias=attn_bias, causal=self.causal, dropout_p=pdrop, q_lens=lens, kv_lens=lens)
        return self.resid_drop(self.o_proj(y))


class MultiheadCrossAttention(nn.Module):
    """queries from x_q, keys / values from x_kv; softmax(q k^T / sqrt(dh) [+ attn_mask]) v in libmopk with Nk = T_kv keys
    (reference :180-221).  attn_mask is ADDITIVE in the reference (:213-214), so it is passed to the core as its bias.
    x_kv may be an `EncodedAudio`: item b's queries then see only the keys j < lens[b]."""

    def __init__(self, dim_q: int, dim_kv: int, n_head: int, dropout: float, bias: bool):
        super().__init__()
        assert dim_q % n_head == 0
        self.n_head, self.head_dim = n_head, dim_q // n_head
        self.scale = self.head_dim ** -0.5
        self.q_proj = TokenLinear(dim_q, dim_q, bias=bias)
        self.k_proj = TokenLinear(dim_kv, dim_q, bias=bias)
        self.v_proj = TokenLinear(dim_kv, dim_q, bias=bias)
        self.o_proj = TokenLinear(dim_q, dim_q, bias=bias)
        self.attn_drop = nn.Dropout(dropout)
        self.resid_drop = nn.Dropout(dropout)

    def forward(self, x_q: torch.Tensor, x_kv: torch.Tensor, attn_mask: Optional[torch.Tensor] = None):
        pdrop = float(self.attn_drop.p) if self.training else 0.0      # dropout on the probabilities (:217), inside the kernels
        x_kv, kv_lens = _enc_parts(x_kv)
        B, Tq, _ = x_q.shape
        Tk = x_kv.shape[1]
        H, Dh = self.n_head, self.head_dim
        q = self.q_proj(x_q).view(B, Tq, H, Dh)
        k = self.k_proj(x_kv).view(B, Tk, H, Dh)
        v = self.v_proj(x_kv).view(B, Tk, H, Dh)
        if kv_lens is None:
            y = ops.sdpa_core(q, k, v, bias=attn_mask, dropout_p=pdrop)
        else:
            y = ops.sdpa_core(q, k, v, bias=attn_mask, dropout_p=pdrop, kv_lens=kv_lens)
        return self.resid_drop(self.o_proj(y))


class MLP(nn.Module):
    def __init__(self, dim: int, dropout: float, bias: bool):
        super().__init__()
        self.fc = TokenLinear(dim, 4 * dim, bias=bias)
        self.proj = TokenLinear(4 * dim, dim, bias=bias)
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        return self.drop(self.proj(F.gelu(self.fc(x), approximate="tanh")))


class EncoderBlock(nn.Module):
    """x + SA(ln1 x); x * gate_t(mel); x + MLP(ln2 x)   (reference :250-275)."""

    def __init__(self, cfg: WhisperConfig):
        super().__init__()
        D = cfg.n_embd
        self.ln1 = nn.LayerNorm(D)
        self.attn = MultiheadSelfAttention(D, cfg.n_head, cfg.dropout, cfg.bias, causal=False)
        self.ln2 = nn.LayerNorm(D)
        self.mlp = MLP(D, cfg.dropout, cfg.bias)
        self.mop = MoP2D(cfg.n_views, cfg.n_kernels, cfg.kernel_size)

    def forward(self, x, mel2d, lens=None, gate_t=None):
        """gate_t: this layer's gate (B,T) where the caller has it already (WhisperMoP computes all layers' in one launch);
        None: the block computes its own from mel2d.  The residual add and the gate are one kernel (ops.gated_residual)."""
        attn_out = self.attn(self.ln1(x)) if lens is None else self.attn(self.ln1(x), lens=lens)
        if gate_t is None:
            gate_t = self.mop.gate(mel2d, lens).squeeze(-1)
        x = ops.gated_residual(x, attn_out, gate_t)
        x = x + self.mlp(self.ln2(x))
        return x, gate_t


class DecoderBlock(nn.Module):
    """x + causal SA(ln1 x); x + CA(ln2 x, enc); x + MLP(ln3 x)   (reference :267-290)."""

    def __init__(self, cfg: WhisperConfig):
        super().__init__()
        D = cfg.n_embd
        self.ln1 = nn.LayerNorm(D)
        self.self_attn = MultiheadSelfAttention(D, cfg.n_head, cfg.dropout, cfg.bias, causal=True)
        self.ln2 = nn.LayerNorm(D)
        self.cross_attn = MultiheadCrossAttention(D, D, cfg.n_head, cfg.dropout, cfg.bias)
        self.ln3 = nn.LayerNorm(D)
        self.mlp = MLP(D, cfg.dropout, cfg.bias)

    def forward(self, x: torch.Tensor, enc: torch.Tensor) -> torch.Tensor:
        """enc: (B, T_audio, D), or an EncodedAudio for clips of different lengths"""
        x = x + self.self_attn(self.ln1(x))
        x = x + self.cross_attn(self.ln2(x), enc)
        x = x + self.mlp(self.ln3(x))
        return x


class WhisperDecodeCache:
    """Key / value cache of one incremental `WhisperMoP` decoding (`init_decode_cache`, `decode_step`, `generate`).

    cross_k / cross_v: per decoder layer, the encoder output projected once to cross-attention keys / values (B, T_audio, H, dh).
    self_k / self_v: per decoder layer, self-attention keys / values (B, max_len, H, dh), filled up to `length`.
    length: the number of cached tokens as a (1,) int32 DEVICE tensor (the kernels read it, so a step's launch arguments do not
    change from step to step); pos: its host mirror (the host drives the loop, so keeping it costs no sync).
    kv_start: None (every row's tokens start at column 0), or an int32 (B,) DEVICE tensor for a ragged batch whose prompts are
    left-padded to one length: row b's tokens start at column kv_start[b] (set it after construction; see decode_step).
    audio_lens: None (every item's cross keys are all T_audio rows), or an int32 (items,) DEVICE tensor for clips of different
    lengths right-padded to T_audio: item b's queries see the cross keys j < audio_lens[b] (set after construction, as kv_start;
    init_decode_cache sets it from an EncodedAudio).  One entry per row of cross_k, i.e. per item where beams / samples share it."""

    def __init__(self, cross_k, cross_v, self_k, self_v, length: torch.Tensor, max_len: int):
        self.cross_k, self.cross_v, self.self_k, self.self_v = cross_k, cross_v, self_k, self_v
        self.length, self.pos, self.max_len = length, 0, int(max_len)
        self.kv_start: Optional[torch.Tensor] = None
        self.audio_lens: Optional[torch.Tensor] = None

    @property
    def dtype(self) -> torch.dtype:
        return self.self_k[0].dtype


class WhisperMoP(nn.Module):
    """Encoder-decoder with the MoP mel gate in every encoder block (reference :296-424).
    forward(mel, dec_input_ids, targets=None) -> (logits, loss, gates); lm_head is tied to wte."""

    def __init__(self, cfg: WhisperConfig):
        super().__init__()
        self.cfg = cfg
        D = cfg.n_embd
        self.audio_proj = nn.Linear(cfg.n_mels, D, bias=cfg.bias)
        self.audio_pos = nn.Embedding(cfg.n_audio_ctx, D) if cfg.use_abs_pos_emb else None
        self.wte = nn.Embedding(cfg.vocab_size, D)
        self.text_pos = nn.Embedding(cfg.n_text_ctx, D) if cfg.use_abs_pos_emb else None
        self.drop = nn.Dropout(cfg.dropout)
        self.encoder = nn.ModuleList([EncoderBlock(cfg) for _ in range(cfg.n_layer_enc)])
        self.decoder = nn.ModuleList([DecoderBlock(cfg) for _ in range(cfg.n_layer_dec)])
        self.enc_ln_f = nn.LayerNorm(D)
        self.dec_ln_f = nn.LayerNorm(D)
        self.lm_head = nn.Linear(D, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.wte.weight
        self.apply(self._init_weights)

    def _init_weights(self, m):                                      # reference :336-346
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, mean=0.0, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, mean=0.0, std=0.02)
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    @torch.no_grad()
    def _pos(self, T: int, device: torch.device) -> torch.Tensor:
        return torch.arange(T, device=device, dtype=torch.long).unsqueeze(0)

    def _audio_check(self, mel, what: str) -> Optional[List[int]]:
        """None for a (B, T_audio, n_mels) tensor; for a list / tuple of B 2-D (T_b, n_mels) tensors (clips of different lengths),
        their frame counts.  Raises ValueError on a malformed list, before any device work."""
        if isinstance(mel, torch.Tensor):
            return None
        if not isinstance(mel, (list, tuple)) or len(mel) == 0:
            raise ValueError(f"{what}: mel must be a (B, T_audio, n_mels) tensor or a non-empty list of B (T_b, n_mels) tensors")
        for b, m in enumerate(mel):
            if not isinstance(m, torch.Tensor) or m.dim() != 2:
                raise ValueError(f"{what}: mel {b} must be a 2-D (T_b, n_mels) tensor, got "
                                 f"{tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__}")
            if m.shape[1] != self.cfg.n_mels:
                raise ValueError(f"{what}: mel {b} has {m.shape[1]} mel bins, the model n_mels = {self.cfg.n_mels}")
            if not 1 <= m.shape[0] <= self.cfg.n_audio_ctx:
                raise ValueError(f"{what}: mel {b} has {m.shape[0]} frames, outside [1, n_audio_ctx = {self.cfg.n_audio_ctx}]")
            if m.dtype != mel[0].dtype or not m.dtype.is_floating_point:
                raise ValueError(f"{what}: mels must share one floating dtype, mel {b} is {m.dtype}")
            if m.device != mel[0].device:
                raise ValueError(f"{what}: mel {b} is on {m.device}, mel 0 on {mel[0].device}")
        return [int(m.shape[0]) for m in mel]

    @staticmethod
    def _audio_pad(mel, lens: Optional[List[int]]):
        """-> (mel (B, T, n_mels), audio_lens): a tensor passes through with audio_lens None; a list is right-padded with ZEROS to
        T = max(lens) (MoP2D's convolutions have no bias and pad with zeros, so a zero tail is what a clip sees when it is alone),
        with audio_lens an int32 (B,) device tensor (None when every length is T: the uniform path)"""
        if lens is None:
            return mel, None
        T = max(lens)
        if min(lens) == T:
            return torch.stack(list(mel)), None
        padded = torch.zeros(len(lens), T, mel[0].shape[1], dtype=mel[0].dtype, device=mel[0].device)
        for b, m in enumerate(mel):
            padded[b, :lens[b]] = m
        audio_lens = torch.tensor(lens, dtype=torch.int32)
        if padded.device.type == "cuda":                               # an asynchronous copy: the host does not wait for it
            return padded, audio_lens.pin_memory().to(padded.device, non_blocking=True)
        return padded, audio_lens

    def _batch_check(self, mel, prompt_ids, what: str):
        """the argument checks generate / beam_search / sample share -> (audio batch info, prompt lengths or None); ValueErrors
        before any device work"""
        alens = self._audio_check(mel, what)
        info = mel if alens is None else _Batch((len(alens),), mel[0].device)
        lens = self._ragged_check(info, prompt_ids, what)
        if alens is not None and lens is None and prompt_ids.shape[0] != len(alens):
            raise ValueError(f"{what}: {prompt_ids.shape[0]} prompts for a batch of {len(alens)} mel inputs")
        return info, lens

    def encode(self, mel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """mel (B, T_audio, n_mels) -> enc_out (B, T_audio, D), gates (B, L_enc, T_audio).

        mel may also be a list of B (T_b, n_mels) tensors, 1 <= T_b <= n_audio_ctx (clips of different lengths).  They are
        right-padded with zeros to T = max T_b; every encoder self-attention then runs with per-row lengths (ops.sdpa_core(q_lens,
        kv_lens): padding frames are neither queries nor keys), so item b comes out as it would alone.  Returns (EncodedAudio(out,
        lens), gates): rows >= lens[b] of out are unspecified, columns >= lens[b] of gates are 1.  A list of equal lengths runs the
        tensor path (lens None)."""
        alens = self._audio_check(mel, "encode")
        if alens is not None:
            mel, audio_lens = self._audio_pad(mel, alens)
            x, gates = self._encode(mel, audio_lens)
            return EncodedAudio(x, audio_lens), gates
        return self._encode(mel, None)

    def _encode(self, mel: torch.Tensor, audio_lens: Optional[torch.Tensor]):
        B, T_a, F_ = mel.shape
        assert F_ == self.cfg.n_mels, "mel dim mismatch"
        x = self.audio_proj(mel)
        if self.audio_pos is not None:
            x = x + self.audio_pos(self._pos(T_a, mel.device))
        x = self.drop(x)
        gates = self._gates(mel, audio_lens)                         # every layer's gate: they depend on the mel map alone
        mel2d = mel.unsqueeze(1)                                     # (B,1,T,F), a view: the blocks are handed their gates
        for blk, gate_t in zip(self.encoder, gates.unbind(1)):
            x, _ = blk(x, mel2d, audio_lens, gate_t)
        x = self.enc_ln_f(x)
        return x, gates.to(_gate_dtype(mel))

    def _gates(self, mel: torch.Tensor, audio_lens: Optional[torch.Tensor]) -> torch.Tensor:
        """the encoder layers' mel gates (B, L_enc, T) fp32: one fold of all layers' MoP2D parameters (ops.mel_gate_taps) and
        one ops.mel_gate launch; with audio_lens the columns >= audio_lens[b] are 1"""
        return ops.mel_gate(mel, _stacked_taps([blk.mop for blk in self.encoder], mel.shape[2]), audio_lens)

    def decode(self, enc_out: torch.Tensor, dec_input_ids: torch.Tensor) -> torch.Tensor:
        """enc_out (B, T_audio, D) or an EncodedAudio, dec_input_ids (B, T_text) -> logits (B, T_text, vocab)."""
        return self.lm_head(self._decode_hidden(enc_out, dec_input_ids))

    def _decode_hidden(self, enc_out, dec_input_ids: torch.Tensor) -> torch.Tensor:
        """the decoder stack up to the head's input (B, T_text, D)"""
        B, T_t = dec_input_ids.shape
        x = self.wte(dec_input_ids)
        if self.text_pos is not None:
            x = x + self.text_pos(self._pos(T_t, dec_input_ids.device))
        x = self.drop(x)
        for blk in self.decoder:
            x = blk(x, enc_out)
        return self.dec_ln_f(x)

    def loss(self, mel: torch.Tensor, dec_input_ids: torch.Tensor, targets: torch.Tensor, *, chunk_rows: Optional[int] = None,
             ignore_index: int = -100):
        """(loss, gates) as forward(mel, dec_input_ids, targets)[1:] returns them, without the (B T_text, vocab) logits: the encoder
        and decoder as in forward, then ops.linear_cross_entropy on the head's input, chunk_rows rows of logits at a time"""
        alens = self._audio_check(mel, "loss")
        if alens is not None and dec_input_ids.shape[0] != len(alens):
            raise ValueError(f"loss: {dec_input_ids.shape[0]} rows of dec_input_ids for a batch of {len(alens)} mel inputs")
        enc_out, gates = self.encode(mel)
        x = self._decode_hidden(enc_out, dec_input_ids)
        loss = ops.linear_cross_entropy(x, self.lm_head.weight, targets, self.lm_head.bias, ignore_index=ignore_index,
                                        chunk_rows=chunk_rows)
        return loss, gates

    def forward(self, mel: torch.Tensor, dec_input_ids: torch.Tensor, targets: Optional[torch.Tensor] = None):
        """mel: (B, T_audio, n_mels), or a list of B (T_b, n_mels) clips of different lengths (see encode): every item's logits
        are then those of the item alone, and the gates' columns >= T_b are 1."""
        alens = self._audio_check(mel, "forward")
        if alens is not None and dec_input_ids.shape[0] != len(alens):
            raise ValueError(f"forward: {dec_input_ids.shape[0]} rows of dec_input_ids for a batch of {len(alens)} mel inputs")
        enc_out, gates = self.encode(mel)
        logits = self.decode(enc_out, dec_input_ids)
        loss = None
        if targets is not None:
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.view(-1))
        return logits, loss, gates

    # ---- incremental (KV-cached) greedy decoding; inference only, dropout off ----
    @torch.no_grad()
    def init_decode_cache(self, enc_out: torch.Tensor, max_len: int) -> WhisperDecodeCache:
        """enc_out (B, T_audio, D) -> a cache for up to max_len text tokens: every decoder layer's cross-attention keys / values are
        projected once here; self-attention buffers (B, max_len, H, dh) are allocated in the dtype the projections produce (bf16
        under bf16 autocast)."""
        if not 0 < int(max_len) <= self.cfg.n_text_ctx:
            raise ValueError(f"init_decode_cache: max_len = {max_len} outside [1, n_text_ctx = {self.cfg.n_text_ctx}]")
        enc_out, audio_lens = _enc_parts(enc_out)                     # an EncodedAudio sets the cache's audio_lens
        B = enc_out.shape[0]
        H, Dh = self.cfg.n_head, self.cfg.n_embd // self.cfg.n_head
        ck, cv = self._cross_kv(enc_out)
        kw = dict(dtype=ck[0].dtype, device=enc_out.device)
        sk = [torch.zeros(B, int(max_len), H, Dh, **kw) for _ in self.decoder]
        sv = [torch.zeros(B, int(max_len), H, Dh, **kw) for _ in self.decoder]
        cache = WhisperDecodeCache(ck, cv, sk, sv, torch.zeros(1, dtype=torch.int32, device=enc_out.device), max_len)
        cache.audio_lens = audio_lens
        return cache

    def _cross_kv(self, enc_out: torch.Tensor):
        """every decoder layer's cross-attention keys / values, (B, T_audio, H, dh) each, projected once"""
        B, T_a, _ = enc_out.shape
        H, Dh = self.cfg.n_head, self.cfg.n_embd // self.cfg.n_head
        ck = [blk.cross_attn.k_proj(enc_out).view(B, T_a, H, Dh) for blk in self.decoder]
        cv = [blk.cross_attn.v_proj(enc_out).view(B, T_a, H, Dh) for blk in self.decoder]
        return ck, cv

    @torch.no_grad()
    def decode_step(self, cache: WhisperDecodeCache, ids: torch.Tensor) -> torch.Tensor:
        """append ids (B, T_new) at positions [len, len + T_new) and run the decoder on them only -> logits (B, T_new, vocab).

        Equals decode(enc_out, all ids so far)[:, -T_new:] in eval().  Attention runs on ops.decode_attention (the split-KV kernels)
        with the device length; a first chunk of more than 16 tokens runs the square causal ops.sdpa_core and writes its keys /
        values into the cache.  Positions, the append and the length update are device-indexed: no host sync, graph-capturable.

        Ragged batches: set cache.kv_start to an int32 (B,) device tensor and pass the prompts left-padded to one length P (any pad
        token), row b's prompt in columns [kv_start[b], P).  Row b's token in column c then takes position c - kv_start[b] (text_pos),
        and its queries see only the keys in columns >= kv_start[b] (ops.decode_attention_ragged; a first chunk of more than 16 tokens
        runs ops.sdpa_core with a key-padding mask), so row b decodes as it would alone; the pad columns are never read.  Every
        later step appends all rows at the same column.  kv_start None is the uniform batch, run exactly as before.

        Clips of different lengths: with cache.audio_lens set (int32 (B,) device tensor), row b's cross-attention sees the keys
        j < audio_lens[b] only (ops.decode_attention_lens; a chunk of more than 16 tokens runs ops.sdpa_core with kv_lens)."""
        return self._decode_tokens(cache, ids)

    def _decode_tokens(self, cache: WhisperDecodeCache, ids: torch.Tensor, rows: Optional[torch.Tensor] = None,
                       beams: int = 1) -> torch.Tensor:
        """decode_step's body.  rows / beams (beam search): self-attention reads row b's key / value j from cache row rows[b, j]
        (ops.decode_attention_rows), and the B = items * beams rows share their item's cross cache (items, T_audio, H, dh): the
        beams' queries of one item go to ops.decode_attention together as one row of beams * T_new queries."""
        B, T = ids.shape
        if cache.pos + T > cache.max_len:
            raise ValueError(f"decode_step: {cache.pos} cached + {T} new tokens exceed the cache's max_len = {cache.max_len}")
        H, Dh = self.cfg.n_head, self.cfg.n_embd // self.cfg.n_head
        idx = cache.length.to(torch.long) + torch.arange(T, device=ids.device)        # positions of the new tokens
        ks = cache.kv_start                                                            # ragged: row b's first column
        x = self.wte(ids)
        if self.text_pos is not None:
            if ks is None:
                x = x + self.text_pos(idx).unsqueeze(0)
            else:                                                                      # per-row positions, pad columns at 0
                x = x + self.text_pos((idx.unsqueeze(0) - ks.to(torch.long).unsqueeze(1)).clamp_min(0))
        new_len = cache.length + T
        long_chunk = T > ops.DECODE_MAX_TQ
        prefill = long_chunk and cache.pos == 0
        for l, blk in enumerate(self.decoder):
            sa, ca = blk.self_attn, blk.cross_attn
            h = blk.ln1(x)
            q, k, v = (p(h).view(B, T, H, Dh) for p in (sa.q_proj, sa.k_proj, sa.v_proj))
            cache.self_k[l].index_copy_(1, idx, k.to(cache.dtype))
            cache.self_v[l].index_copy_(1, idx, v.to(cache.dtype))
            y = self._self_attention(cache, l, q, k, v, idx, new_len, rows, prefill)
            x = x + sa.o_proj(y)
            q = ca.q_proj(blk.ln2(x)).view(B, T, H, Dh)
            y = self._cross_attention(cache, l, q, beams, long_chunk)
            x = x + ca.o_proj(y)
            x = x + blk.mlp.proj(F.gelu(blk.mlp.fc(blk.ln3(x)), approximate="tanh"))
        cache.length.add_(T)
        cache.pos += T
        return self.lm_head(self.dec_ln_f(x))

    @staticmethod
    def _self_attention(cache: WhisperDecodeCache, l: int, q, k, v, idx, new_len, rows, prefill: bool) -> torch.Tensor:
        """layer l's causal self-attention of a decode step, after the step's k / v were appended: prefill (a first chunk of more
        than 16 tokens) runs the square core on the chunk, every other step the decode core the cache asks for"""
        ks = cache.kv_start
        if prefill and ks is not None:                                                # key-padding mask (B, 1, 1, T)
            B, T = q.shape[:2]
            return ops.sdpa_core(q, k, v, attn_mask=(idx.unsqueeze(0) >= ks.unsqueeze(1)).view(B, 1, 1, T), causal=True)
        if prefill:
            return ops.sdpa_core(q, k, v, causal=True)
        if ks is not None:
            return ops.decode_attention_ragged(q, cache.self_k[l], cache.self_v[l], ks, rows=rows, kv_len=new_len, causal=True)
        if rows is not None:
            return ops.decode_attention_rows(q, cache.self_k[l], cache.self_v[l], rows, kv_len=new_len, causal=True)
        return ops.decode_attention(q, cache.self_k[l], cache.self_v[l], kv_len=new_len, causal=True)

    @staticmethod
    def _cross_attention(cache: WhisperDecodeCache, l: int, q, beams: int, long_chunk: bool) -> torch.Tensor:
        """layer l's cross-attention of a decode step over the item's cached audio keys / values"""
        B, T, H, Dh = q.shape
        ck, cv, al = cache.cross_k[l], cache.cross_v[l], cache.audio_lens
        if long_chunk:
            return ops.sdpa_core(q, ck, cv) if al is None else ops.sdpa_core(q, ck, cv, kv_lens=al)
        if al is not None:                                                            # one length per item = per row of q here
            return ops.decode_attention_lens(q.view(B // beams, beams * T, H, Dh), ck, cv, al, nk=ck.shape[1]).view(B, T, H * Dh)
        if beams > 1:
            return ops.decode_attention(q.view(B // beams, beams * T, H, Dh), ck, cv, nk=ck.shape[1]).view(B, T, H * Dh)
        return ops.decode_attention(q, ck, cv, nk=ck.shape[1])

    @staticmethod
    def _ragged_check(mel: torch.Tensor, prompt_ids, what: str) -> Optional[List[int]]:
        """None for a (B, T_p) tensor; for a list / tuple of B 1-D integer tensors (a ragged batch), their lengths.  Raises
        ValueError on a malformed list, before any device work."""
        if isinstance(prompt_ids, torch.Tensor):
            return None
        if isinstance(prompt_ids, _PreparedPrompts):
            if len(prompt_ids.lens) != mel.shape[0]:
                raise ValueError(f"{what}: {len(prompt_ids.lens)} prompts for a batch of {mel.shape[0]} mel inputs")
            return list(prompt_ids.lens)
        if not isinstance(prompt_ids, (list, tuple)) or len(prompt_ids) == 0:
            raise ValueError(f"{what}: prompt_ids must be a (B, T_p) tensor or a non-empty list of B 1-D token tensors")
        if len(prompt_ids) != mel.shape[0]:
            raise ValueError(f"{what}: {len(prompt_ids)} prompts for a batch of {mel.shape[0]} mel inputs")
        for b, p in enumerate(prompt_ids):
            if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.numel() < 1:
                raise ValueError(f"{what}: prompt {b} must be a non-empty 1-D tensor, got "
                                 f"{tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__}")
            if p.dtype.is_floating_point or p.dtype.is_complex or p.dtype == torch.bool or p.dtype != prompt_ids[0].dtype:
                raise ValueError(f"{what}: prompts must share one integer dtype, prompt {b} is {p.dtype}")
            if p.device != mel.device:
                raise ValueError(f"{what}: prompt {b} is on {p.device}, the mel on {mel.device}")
        return [int(p.shape[0]) for p in prompt_ids]

    @staticmethod
    def _ragged_pad(prompt_ids, lens: Optional[List[int]], device):
        """-> (prompts (B, P), kv_start): a tensor passes through with kv_start None; a ragged list is left-padded with token 0 to
        P = max(lens), row b's prompt in columns [P - lens[b], P), with kv_start = P - lens as an int32 (B,) device tensor (None
        when every length is P: the uniform path)"""
        if isinstance(prompt_ids, _PreparedPrompts):
            return prompt_ids.ids, prompt_ids.kv_start
        if lens is None:
            return prompt_ids, None
        P = max(lens)
        if min(lens) == P:
            return torch.stack(list(prompt_ids)), None
        padded = torch.zeros(len(lens), P, dtype=prompt_ids[0].dtype, device=device)
        for b, p in enumerate(prompt_ids):
            padded[b, P - lens[b]:] = p
        kv_start = torch.tensor([P - n for n in lens], dtype=torch.int32)
        if device.type == "cuda":                                      # an asynchronous copy: the host does not wait for it
            return padded, kv_start.pin_memory().to(device, non_blocking=True)
        return padded, kv_start

    def _decode_check(self, mel, prompt_ids, max_new_tokens: int, what: str, count=None, min_vocab: int = 0):
        """the argument checks generate / beam_search / sample share, on top of _batch_check -> (audio batch info, prompt lengths
        or None, B, T_p, rows per item).  count: (argument name, value) of beam_search's num_beams / sample's num_samples.
        ValueErrors before any device work"""
        mel_info, lens = self._batch_check(mel, prompt_ids, what)
        B, T_p = prompt_ids.shape if lens is None else (len(lens), max(lens))
        rep = 1 if count is None else int(count[1])
        if not 1 <= rep <= ops.BEAM_MAX_K:
            raise ValueError(f"{what}: {count[0]} = {count[1]} outside [1, {ops.BEAM_MAX_K}]")
        if self.cfg.vocab_size < min_vocab:
            raise ValueError(f"{what}: needs vocab_size >= {min_vocab}, got {self.cfg.vocab_size}")
        if T_p < 1 or max_new_tokens < 1:
            raise ValueError(f"{what}: needs a prompt and at least one new token (T_p = {T_p}, max_new_tokens = {max_new_tokens})")
        if T_p + max_new_tokens > self.cfg.n_text_ctx:
            raise ValueError(f"{what}: T_p + max_new_tokens = {T_p + max_new_tokens} exceeds n_text_ctx = {self.cfg.n_text_ctx}")
        return mel_info, lens, B, T_p, rep

    def _rules_check(self, rules, eos_token_id, what: str) -> None:
        """the argument checks of a decoding with logit rules (None: nothing to check); ValueErrors before any device work"""
        if rules is None:
            return
        if not isinstance(rules, ops.LogitRules):
            raise ValueError(f"{what}: logit rules must be an ops.LogitRules, got {type(rules).__name__}")
        if rules.vocab_size != self.cfg.vocab_size:
            raise ValueError(f"{what}: the logit rules were built for vocab_size = {rules.vocab_size}, the model has "
                             f"{self.cfg.vocab_size}")
        if rules.eos_token_id is not None and eos_token_id is not None and int(eos_token_id) != rules.eos_token_id:
            raise ValueError(f"{what}: eos_token_id = {eos_token_id}, the logit rules' eos_token_id = {rules.eos_token_id}")

    def _repeat_check(self, rules, what: str):
        """the argument checks of a decoding with repeat rules -> the rules, or None for None and for neutral rules (which then
        cost no launch and no buffer); ValueErrors before any device work"""
        if rules is None:
            return None
        if not isinstance(rules, ops.RepeatRules):
            raise ValueError(f"{what}: repeat rules must be an ops.RepeatRules, got {type(rules).__name__}")
        if rules.vocab_size != self.cfg.vocab_size:
            raise ValueError(f"{what}: the repeat rules were built for vocab_size = {rules.vocab_size}, the model has "
                             f"{self.cfg.vocab_size}")
        return None if rules.neutral else rules

    @staticmethod
    def _filter(lg, hist, pos, t0: int, logit_rules, repeat_rules):
        """a step's last-position logits through the rules, in place: ops.repeat_rules first, then ops.logit_rules, so the
        timestamp grammar's rule 3e and every log-probability see the penalised row; hist: the rows' int32 token histories"""
        if repeat_rules is not None:
            lg = ops.repeat_rules(lg, hist, pos, t0, repeat_rules, out=lg)
        if logit_rules is not None:
            lg = ops.logit_rules(lg, hist, pos, t0, logit_rules, out=lg)
        return lg

    def _stats_check(self, return_stats: bool, no_speech_token_id, sot_index, lens: Optional[List[int]], T_p: int, what: str,
                     eos_token_id=None):
        """the argument checks of a decoding with return_stats -> None when no statistics are asked for, else (no_speech_token_id
        or None, sot_index); ValueErrors before any device work"""
        if not return_stats:
            return None
        V = self.cfg.vocab_size
        if eos_token_id is not None and (isinstance(eos_token_id, bool) or int(eos_token_id) != eos_token_id
                                         or not 0 <= eos_token_id < V):
            raise ValueError(f"{what}: with return_stats, eos_token_id must be None or an int in [0, vocab_size = {V}), got "
                             f"{eos_token_id!r}")
        if no_speech_token_id is not None and (isinstance(no_speech_token_id, bool) or not isinstance(no_speech_token_id, int)
                                               or not 0 <= no_speech_token_id < V):
            raise ValueError(f"{what}: no_speech_token_id must be None or an int in [0, vocab_size = {V}), got {no_speech_token_id!r}")
        shortest = T_p if lens is None else min(lens)
        if isinstance(sot_index, bool) or not isinstance(sot_index, int) or not 0 <= sot_index < shortest:
            raise ValueError(f"{what}: sot_index must be an int inside the shortest prompt, [0, {shortest}), got {sot_index!r}")
        return no_speech_token_id, sot_index

    @staticmethod
    def _prepared(prompt_ids, stats, lens, T_p: int):
        """(stats, lens) as the decoders go on using them.  A _PreparedPrompts batch holds the sot sequence in the last sot_len
        columns of every row: its no-speech column is T_p - sot_len + sot_index for all rows, and its tokens are not cut into a
        list (lens None from here on)"""
        if not isinstance(prompt_ids, _PreparedPrompts):
            return stats, lens
        return (None if stats is None else (stats[0], T_p - prompt_ids.sot_len + stats[1])), None

    @staticmethod
    def _no_speech_prob(prompt_logits: torch.Tensor, stats, lens: Optional[List[int]]) -> Optional[torch.Tensor]:
        """P(no_speech_token_id) at position sot_index of every row's own prompt, from the prompt pass's logits (B, T_p, V) as
        the decoder gave them (call it before a logit rule rewrites the last position in place): one ops.token_logprob launch on
        a column view; a ragged batch first gathers its B rows (B slices and one stack)"""
        tok, sot = stats
        if tok is None:
            return None
        B, T_p = prompt_logits.shape[:2]
        if lens is None or min(lens) == T_p:
            rows = prompt_logits[:, sot]
        else:                                                          # left-padded: row b's prompt starts at T_p - lens[b]
            rows = torch.stack([prompt_logits[b, T_p - lens[b] + sot] for b in range(B)])
        return ops.token_logprob(rows, tok).exp()

    @staticmethod
    def _generated_lengths(tokens: torch.Tensor, T_p: int, eos_token_id: Optional[int]) -> torch.Tensor:
        """int32 (B,): the generated tokens of each (B, cap) row up to and including its first eos, or all of them"""
        gen = tokens[:, T_p:]
        n = gen.shape[1]
        if eos_token_id is None:
            return torch.full((gen.shape[0],), n, dtype=torch.int32, device=tokens.device)
        j = torch.arange(n, device=tokens.device).unsqueeze(0)
        return (torch.where(gen == eos_token_id, j, n - 1).min(1).values + 1).to(torch.int32)

    def with_logit_rules(self, logit_rules: Optional["ops.LogitRules"],
                         repeat_rules: Optional["ops.RepeatRules"] = None) -> "RuledDecoding":
        """this model's decoders under Whisper's logit rules: with_logit_rules(rules).generate / .beam_search / .sample take the
        arguments of generate / beam_search / sample and apply ops.logit_rules(rules) to every step's last-position logits, on the
        device and inside the captured step, before the argmax / beam step / draw.  None: the plain decoders.
        repeat_rules: an ops.RepeatRules (a repetition penalty and / or no-repeat n-gram blocking over the generated tokens),
        applied by ops.repeat_rules to the same logits BEFORE the logit rules; it works with logit_rules None too.  None or
        neutral rules add no launch and no buffer."""
        return RuledDecoding(self, logit_rules, repeat_rules)

    def _replicated_cache(self, mel, mel_info, prompt_ids, lens: Optional[List[int]], cap: int, rep: int):
        """encode, run the prompt once per item and set up the cache of rep rows per item (beams / samples) for the steps after it
        -> (prompt_ids (B, T_p) padded, the prompt pass's logits (B, T_p, V): [:, -1] is shared by the item's rows, the step cache).  The prompt's keys / values
        land in cache row b * rep (a prompt cache over the rows [::rep] of the same buffers); the step cache starts at pos = T_p,
        with the padding's kv_start per row and the audio lengths per item (an item's rows share its cross cache)."""
        H, Dh = self.cfg.n_head, self.cfg.n_embd // self.cfg.n_head
        prompt_ids, kv_start = self._ragged_pad(prompt_ids, lens, mel_info.device)
        B, T_p = prompt_ids.shape
        enc, audio_lens = _enc_parts(self.encode(mel)[0])
        ck, cv = self._cross_kv(enc)
        kw = dict(dtype=ck[0].dtype, device=enc.device)
        sk = [torch.zeros(B * rep, cap, H, Dh, **kw) for _ in self.decoder]
        sv = [torch.zeros(B * rep, cap, H, Dh, **kw) for _ in self.decoder]
        length = torch.zeros(1, dtype=torch.int32, device=enc.device)
        prompt_cache = WhisperDecodeCache(ck, cv, [t[::rep] for t in sk], [t[::rep] for t in sv], length, cap)
        prompt_cache.kv_start, prompt_cache.audio_lens = kv_start, audio_lens
        logits = self.decode_step(prompt_cache, prompt_ids)
        cache = WhisperDecodeCache(ck, cv, sk, sv, length, cap)
        cache.pos = T_p
        cache.kv_start = None if kv_start is None else kv_start.repeat_interleave(rep)
        cache.audio_lens = audio_lens
        return prompt_ids, logits, cache

    @staticmethod
    def _step_loop(cache: WhisperDecodeCache, step, n_steps: int, graph: bool, feed=None) -> None:
        """run step() n_steps times on the cache.  graph: the first step runs eagerly (and warms every kernel up), the second is
        captured in a HIP graph (torch.cuda.graph, one stream, static buffers) and replayed for every further one.  feed(t), if
        given, runs before step t and outside the graph: it puts the step's input where step() reads it (a static buffer for
        t >= 1 when graph is set)."""
        g = None
        for t in range(n_steps):
            if feed is not None:
                feed(t)
            if not graph or t == 0:
                step()
                continue
            if g is None:
                g = torch.cuda.CUDAGraph()
                with torch.autocast(device_type="cuda", dtype=torch.get_autocast_dtype("cuda"),
                                    enabled=torch.is_autocast_enabled("cuda"), cache_enabled=False):
                    with torch.cuda.graph(g):
                        step()
                cache.pos -= 1                           # capture recorded the step without running it
            g.replay()
            cache.pos += 1

    @torch.no_grad()
    def generate(self, mel: torch.Tensor, prompt_ids: torch.Tensor, max_new_tokens: int, eos_token_id: Optional[int] = None,
                 graph: bool = False, *, return_logits: bool = False):
        """greedy decoding: mel (B, T_audio, n_mels), prompt_ids (B, T_p) -> tokens (B, T_p + max_new_tokens), all on the device.

        Rows that have emitted eos_token_id keep emitting it (torch.where: the loop never syncs the host).  graph=True runs the prompt
        and the first single-token step eagerly, captures one single-token decode_step in a HIP graph (torch.cuda.graph, one stream,
        static id / logit buffers) and replays it for every further token.  return_logits=True also returns the last-position logits
        that chose each new token, (B, max_new_tokens, vocab).

        prompt_ids may also be a list of B 1-D tensors of different lengths (a ragged batch): they are left-padded in one cache with
        a per-row start (WhisperDecodeCache.kv_start), each row decodes as it would alone, and the tokens come back as a list of B
        1-D tensors, prompt b followed by its max_new_tokens tokens (views of one device tensor).
        mel may also be a list of B (T_b, n_mels) clips of different lengths (see encode; it combines with a prompt list): every
        row decodes as it would alone.
        Whisper's logit rules and the decoding statistics (return_stats): with_logit_rules(rules).generate(...) takes the same
        arguments and the statistics' keywords; rules None decodes as here."""
        return self._generate(mel, prompt_ids, max_new_tokens, eos_token_id, graph, return_logits, None)

    def _generate(self, mel, prompt_ids, max_new_tokens, eos_token_id, graph, return_logits, logit_rules, return_stats=False,
                  no_speech_token_id=None, sot_index=0, repeat_rules=None):
        """generate's body.  logit_rules: every step's last-position logits pass ops.logit_rules before the argmax, inside the
        captured step, over a (B, cap) int32 device history kept for them only; None runs exactly the code without them.
        repeat_rules: the logits pass ops.repeat_rules before that, over the same history (kept for them alone when logit_rules
        is None).  return_stats: the statistics route (_generate_stats) from the prompt's logits on; False runs exactly the code without it"""
        mel_info, lens, B, T_p, _ = self._decode_check(mel, prompt_ids, max_new_tokens, "generate")
        self._rules_check(logit_rules, eos_token_id, "generate")
        repeat_rules = self._repeat_check(repeat_rules, "generate")
        stats = self._stats_check(return_stats, no_speech_token_id, sot_index, lens, T_p, "generate", eos_token_id)
        stats, lens = self._prepared(prompt_ids, stats, lens, T_p)
        prompt_ids, kv_start = self._ragged_pad(prompt_ids, lens, mel_info.device)
        enc, _ = self.encode(mel)
        cache = self.init_decode_cache(enc, T_p + max_new_tokens)
        cache.kv_start = kv_start
        prompt_logits = self.decode_step(cache, prompt_ids)
        logits = prompt_logits[:, -1]
        if stats is not None:
            return self._generate_stats(cache, prompt_ids, prompt_logits, lens, max_new_tokens, eos_token_id, graph, return_logits,
                                        logit_rules, stats, repeat_rules)
        del prompt_logits
        hist = None
        if logit_rules is not None or repeat_rules is not None:
            hist = torch.zeros(B, T_p + max_new_tokens, dtype=torch.int32, device=prompt_ids.device)
            hist[:, :T_p] = prompt_ids
            logits = self._filter(logits, hist, cache.length, T_p, logit_rules, repeat_rules)
        done = torch.zeros(B, dtype=torch.bool, device=prompt_ids.device) if eos_token_id is not None else None
        toks, steps = [], []
        ids = None

        def pick():                                  # the next token of every row from the last logits; never inside the graph
            nonlocal done
            if return_logits:
                steps.append(logits.clone())
            nxt = logits.argmax(-1)
            if done is not None:
                nxt = torch.where(done, torch.full_like(nxt, eos_token_id), nxt)
                done = done | (nxt == eos_token_id)
            toks.append(nxt)
            if hist is not None:
                hist[:, cache.pos] = nxt             # the host drives the loop: it knows the column
            return nxt.unsqueeze(1)

        def feed(t):
            nonlocal ids
            if graph and t > 1:
                ids.copy_(pick())
            elif graph and t == 1:                   # the buffer the captured step reads from then on
                ids = pick().clone()
            else:
                ids = pick()

        def step():                                  # captured: logits becomes the graph's static output
            nonlocal logits
            logits = self.decode_step(cache, ids)[:, -1]
            if hist is not None:
                logits = self._filter(logits, hist, cache.length, T_p, logit_rules, repeat_rules)

        self._step_loop(cache, step, max_new_tokens - 1, graph, feed)
        pick()
        out = torch.cat([prompt_ids, torch.stack(toks, dim=1).to(prompt_ids.dtype)], dim=1)
        if lens is not None:
            out = [out[b, T_p - lens[b]:] for b in range(B)]
        return (out, torch.stack(steps, dim=1)) if return_logits else out

    def _generate_stats(self, cache, prompt_ids, prompt_logits, lens, max_new_tokens, eos_token_id, graph, return_logits,
                        logit_rules, stats, repeat_rules=None):
        """generate's statistics route, from the prompt pass's logits on: ops.greedy_pick chooses every token on an
        ops.GreedyState whose hist is the logit rules' history and, in the end, the tokens; a step is the decoder step, the
        rules and the pick, all captured with graph=True"""
        B, T_p = prompt_ids.shape
        dev, cap = prompt_ids.device, T_p + max_new_tokens
        no_speech = self._no_speech_prob(prompt_logits, stats, lens)                  # before the rules rewrite [:, -1] in place
        st = ops.GreedyState(B, cap, None if eos_token_id is None else int(eos_token_id), with_hist=True, device=dev)
        st.hist[:, :T_p] = prompt_ids
        steps = None
        if return_logits:
            steps = torch.empty(B, max_new_tokens, prompt_logits.shape[-1], dtype=prompt_logits.dtype, device=dev)

        def pick(lg):
            lg = self._filter(lg, st.hist, cache.length, T_p, logit_rules, repeat_rules)
            if steps is not None:                    # at the device index of the token being chosen: the same launch every step
                steps.index_copy_(1, cache.length.to(torch.long) - T_p, lg.unsqueeze(1))
            ops.greedy_pick(lg, st, cache.length)

        def step():
            pick(self.decode_step(cache, st.next_ids)[:, -1])

        pick(prompt_logits[:, -1])
        self._step_loop(cache, step, max_new_tokens - 1, graph)
        out = torch.cat([prompt_ids, st.hist[:, T_p:].to(prompt_ids.dtype)], dim=1)
        if lens is not None:
            out = [out[b, T_p - lens[b]:] for b in range(B)]
        res = (out, steps) if return_logits else (out,)
        return res + (DecodeStats(st.sum_logprobs, st.n_tokens, no_speech),)

    @torch.no_grad()
    def beam_search(self, mel: torch.Tensor, prompt_ids: torch.Tensor, max_new_tokens: int, num_beams: int,
                    eos_token_id: Optional[int] = None, length_penalty: float = 1.0, graph: bool = False):
        """beam-search decoding: mel (B, T_audio, n_mels), prompt_ids (B, T_p) -> (tokens (B, T_p + max_new_tokens) in prompt_ids'
        dtype, scores (B,) fp32), all on the device; the step loop never syncs the host.

        The prompt runs once per item (its keys / values land in cache row b * K); beam scores start at [0, -inf, ...].  Each step
        (ops.beam_step) ranks the candidates (k, v) by score_k + log_softmax(logits_k)[v] in fp32, takes the top 2K (ties to the
        smaller k * V + v) and walks them in order: eos_token_id with a finite score is stored as a finished hypothesis while the item
        has fewer than K (score / gen_len ** length_penalty, gen_len counting the eos), and is never a live beam; any other candidate
        becomes the next live beam; the walk stops at K live beams.  An item holding K finished hypotheses is done (patience 1) and
        no longer changes.  After max_new_tokens steps an item that is not done adds its live beams in beam order until it holds K;
        the answer is the best normalised score (ties to the earlier stored hypothesis), eos-filled past its eos.  Without
        eos_token_id that is the best live beam.
        Beams never copy cache slots: each step's keys / values are written once into the beam's own row, and the self-attention
        reads a beam's history through the device row table (ops.decode_attention_rows).  graph=True captures one step (decoder
        step + beam_step) after the first eager one and replays it (torch.cuda.graph, one stream, static buffers).
        prompt_ids may also be a list of B 1-D tensors of different lengths (see generate): the tokens then come back as a list of B
        1-D tensors, prompt b followed by max_new_tokens tokens; gen_len counts generated tokens only, as for a tensor.
        mel may also be a list of B (T_b, n_mels) clips of different lengths (see encode): an item's beams share its cross cache and
        its length.
        Whisper's logit rules and the decoding statistics (return_stats): with_logit_rules(rules).beam_search(...) takes the same
        arguments and the statistics' keywords; rules None decodes as here."""
        return self._beam_search(mel, prompt_ids, max_new_tokens, num_beams, eos_token_id, length_penalty, graph, None)

    def _beam_search(self, mel, prompt_ids, max_new_tokens, num_beams, eos_token_id, length_penalty, graph, logit_rules,
                     return_stats=False, no_speech_token_id=None, sot_index=0, repeat_rules=None):
        """beam_search's body.  logit_rules: every step's logits pass ops.logit_rules before ops.beam_step, inside the captured
        step, with the beams' own histories (the first step's shared prompt logits with the rows [::K] of them); None runs exactly
        the code without them.  repeat_rules: ops.repeat_rules before that, on the same histories"""
        mel_info, lens, B, T_p, K = self._decode_check(mel, prompt_ids, max_new_tokens, "beam_search", ("num_beams", num_beams), 2)
        self._rules_check(logit_rules, eos_token_id, "beam_search")
        repeat_rules = self._repeat_check(repeat_rules, "beam_search")
        stats = self._stats_check(return_stats, no_speech_token_id, sot_index, lens, T_p, "beam_search", eos_token_id)
        stats, lens = self._prepared(prompt_ids, stats, lens, T_p)
        cap = T_p + max_new_tokens
        prompt_ids, prompt_logits, cache = self._replicated_cache(mel, mel_info, prompt_ids, lens, cap, K)
        no_speech = None if stats is None else self._no_speech_prob(prompt_logits, stats, lens)
        logits = prompt_logits[:, -1]
        del prompt_logits
        st = ops.BeamState(prompt_ids, K, cap, eos_token_id, length_penalty)
        logits = self._filter(logits, st.hist[::K], cache.length, T_p, logit_rules, repeat_rules)
        ops.beam_step(logits, st, cache.length)

        def step():
            lg = self._decode_tokens(cache, st.next_ids, rows=st.rows, beams=K)[:, -1]
            lg = self._filter(lg, st.hist, cache.length, T_p, logit_rules, repeat_rules)
            ops.beam_step(lg, st, cache.length)

        self._step_loop(cache, step, max_new_tokens - 1, graph)
        tokens, scores = ops.beam_finalize(st, max_new_tokens)
        if stats is not None:
            n_tokens = self._generated_lengths(tokens, T_p, eos_token_id)
            stats = DecodeStats(scores * n_tokens.to(torch.float32) ** float(length_penalty), n_tokens, no_speech)
        tokens = tokens.to(prompt_ids.dtype)
        if lens is not None:
            tokens = [tokens[b, T_p - lens[b]:] for b in range(B)]
        return (tokens, scores) if stats is None else (tokens, scores, stats)

    @torch.no_grad()
    def sample(self, mel: torch.Tensor, prompt_ids: torch.Tensor, max_new_tokens: int, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, num_samples: int = 1, eos_token_id: Optional[int] = None, seed: int = 0, graph: bool = False):
        """sampled decoding: mel (B, T_audio, n_mels), prompt_ids (B, T_p) -> (tokens (B, num_samples, T_p + max_new_tokens) in
        prompt_ids' dtype, sum_logprobs (B, num_samples) fp32), all on the device; the step loop never syncs the host.

        Every token is drawn by ops.sample_tokens (temperature, top_k, top_p and the draw rule are documented there; temperature 0 is
        greedy and equals generate).  Row b * num_samples + s is sample s of item b (Whisper's best_of): the encoder and the prompt
        run once per item (its keys / values land in cache row b * num_samples, the first draw reads the item's prompt logits for
        all its samples), and a constant row table lets the samples read the shared prompt through ops.decode_attention_rows; no
        cache slot is copied.  The draw at position pos of sample row r is a pure function of (logits, seed, r, pos).  A row that has
        emitted eos_token_id keeps emitting it; sum_logprobs adds log_softmax(logits)[token] of every token up to and including the
        first eos.  graph=True captures one step (decoder step + sample_tokens + the eos / sum update) after the first eager one and
        replays it (torch.cuda.graph, one stream, static buffers).
        prompt_ids may also be a list of B 1-D tensors of different lengths (see generate): the tokens then come back as a list of B
        (num_samples, P_b + max_new_tokens) tensors, and row r draws at its own token index (ops.sample_tokens_ragged), so its draws
        are those of a batch in which every prompt has its length.
        mel may also be a list of B (T_b, n_mels) clips of different lengths (see encode): an item's samples share its cross cache
        and its length.
        Whisper's logit rules: with_logit_rules(rules).sample(...) takes the same arguments; sum_logprobs is then the log-softmax
        of the FILTERED row (Whisper's convention: its filters precede the log-probabilities).  The decoding statistics
        (return_stats) are keywords of with_logit_rules(rules).sample(...) as well; rules None decodes as here."""
        return self._sample(mel, prompt_ids, max_new_tokens, temperature, top_k, top_p, num_samples, eos_token_id, seed, graph, None)

    def _sample(self, mel, prompt_ids, max_new_tokens, temperature, top_k, top_p, num_samples, eos_token_id, seed, graph,
                logit_rules, return_stats=False, no_speech_token_id=None, sot_index=0, repeat_rules=None):
        """sample's body.  logit_rules: every step's logits pass ops.logit_rules before the draw, inside the captured step, with
        the samples' own token rows as history (the first draw's shared prompt logits with the rows [::num_samples] of them); the
        log-probabilities are those of the filtered row.  None runs exactly the code without them.  repeat_rules:
        ops.repeat_rules before that, on the same rows"""
        mel_info, lens, B, T_p, n = self._decode_check(mel, prompt_ids, max_new_tokens, "sample", ("num_samples", num_samples))
        ops._sample_params(temperature, top_k, top_p, "sample")                 # argument errors before encoding
        self._rules_check(logit_rules, eos_token_id, "sample")
        repeat_rules = self._repeat_check(repeat_rules, "sample")
        stats = self._stats_check(return_stats, no_speech_token_id, sot_index, lens, T_p, "sample", eos_token_id)
        stats, lens = self._prepared(prompt_ids, stats, lens, T_p)
        cap = T_p + max_new_tokens
        prompt_ids, prompt_logits, cache = self._replicated_cache(mel, mel_info, prompt_ids, lens, cap, n)
        no_speech = None if stats is None else self._no_speech_prob(prompt_logits, stats, lens)
        logits = prompt_logits[:, -1]
        del prompt_logits
        dev = prompt_ids.device
        i32 = dict(dtype=torch.int32, device=dev)
        r = torch.arange(B * n, **i32)
        table = r.unsqueeze(1).repeat(1, cap)                                   # constant: the prompt from row b * n, then own rows
        table[:, :T_p] = (r // n * n).unsqueeze(1)
        tokens = torch.zeros(B * n, cap, **i32)
        tokens[:, :T_p] = prompt_ids.to(torch.int32).repeat_interleave(n, 0)
        tok, lp = torch.zeros(B * n, **i32), torch.zeros(B * n, dtype=torch.float32, device=dev)
        ids = torch.zeros(B * n, 1, **i32)
        sum_lp = torch.zeros(B * n, dtype=torch.float32, device=dev)
        done = torch.zeros(B * n, dtype=torch.bool, device=dev)
        eos = None if eos_token_id is None else int(eos_token_id)
        n_tok = torch.zeros(B * n, **i32) if stats is not None and eos is not None else None

        def draw(lg):
            lg = self._filter(lg, tokens if lg.shape[0] == B * n else tokens[::n], cache.length, T_p, logit_rules, repeat_rules)
            if cache.kv_start is None:
                ops.sample_tokens(lg, cache.length, temperature, top_k, top_p, seed, out=(tok, lp))
            else:
                ops.sample_tokens_ragged(lg, cache.length, cache.kv_start, temperature, top_k, top_p, seed, out=(tok, lp))
            if eos is None:
                sum_lp.add_(lp)
                ids.copy_(tok.unsqueeze(1))
            else:
                sum_lp.add_(torch.where(done, torch.zeros_like(lp), lp))
                if n_tok is not None:
                    n_tok.add_(torch.where(done, 0, 1))
                ids.copy_(torch.where(done, torch.full_like(tok, eos), tok).unsqueeze(1))
                done.logical_or_(ids.squeeze(1) == eos)
            tokens.index_copy_(1, cache.length.to(torch.long), ids)

        def step():
            draw(self._decode_tokens(cache, ids, rows=table, beams=n)[:, -1])

        draw(logits)
        self._step_loop(cache, step, max_new_tokens - 1, graph)
        tokens = tokens.view(B, n, cap).to(prompt_ids.dtype)
        if lens is not None:
            tokens = [tokens[b, :, T_p - lens[b]:] for b in range(B)]
        if stats is None:
            return tokens, sum_lp.view(B, n)
        if n_tok is None:                                                       # no eos: every row holds all its tokens
            n_tok = torch.full((B * n,), max_new_tokens, **i32)
        return tokens, sum_lp.view(B, n), DecodeStats(sum_lp.view(B, n), n_tok.view(B, n), no_speech)

    # ---- token-level timestamps; inference only ----
    def _align_check(self, mel, tokens, prompt_len, alignment_heads, medfilt_width, what: str = "align_tokens"):
        """align_tokens' argument checks -> (audio batch info, token lengths, (layer, head) pairs); ValueErrors before any device
        work"""
        alens = self._audio_check(mel, what)
        info = mel if alens is None else _Batch((len(alens),), mel[0].device)
        if isinstance(tokens, torch.Tensor):
            if tokens.dim() != 2 or tokens.dtype.is_floating_point or tokens.dtype.is_complex or tokens.dtype == torch.bool:
                raise ValueError(f"{what}: tokens must be an integer (B, T) tensor or a list of B 1-D token tensors, got "
                                 f"{tuple(tokens.shape)} {tokens.dtype}")
            if tokens.shape[0] != info.shape[0]:
                raise ValueError(f"{what}: {tokens.shape[0]} token sequences for a batch of {info.shape[0]} mel inputs")
            if tokens.device != info.device:
                raise ValueError(f"{what}: tokens are on {tokens.device}, the mel on {info.device}")
            lens = [int(tokens.shape[1])] * tokens.shape[0]
        else:
            lens = self._ragged_check(info, tokens, what)
        if isinstance(prompt_len, bool) or not isinstance(prompt_len, int) or prompt_len < 0:
            raise ValueError(f"{what}: prompt_len must be a non-negative int (one for the batch), got {prompt_len!r}")
        if min(lens) < prompt_len + 2:
            raise ValueError(f"{what}: every sequence needs the prompt, one token to align and a final token: the shortest has "
                             f"{min(lens)} tokens, prompt_len = {prompt_len}")
        if max(lens) > self.cfg.n_text_ctx:
            raise ValueError(f"{what}: a sequence of {max(lens)} tokens exceeds n_text_ctx = {self.cfg.n_text_ctx}")
        return info, lens, self._align_heads_check(alignment_heads, medfilt_width, what)

    def _align_heads_check(self, alignment_heads, medfilt_width, what: str):
        """the tests of the alignment heads and the median width -> the (layer, head) pairs"""
        if isinstance(medfilt_width, bool) or not isinstance(medfilt_width, int) or medfilt_width < 1 or medfilt_width % 2 == 0:
            raise ValueError(f"{what}: medfilt_width must be a positive odd int, got {medfilt_width!r}")
        Ld, H = self.cfg.n_layer_dec, self.cfg.n_head
        if alignment_heads is None:                                   # Whisper's default: every head of the upper half of the layers
            heads = [(l, h) for l in range(Ld // 2, Ld) for h in range(H)]
        else:
            heads = [tuple(p) for p in alignment_heads]
            if not heads:
                raise ValueError(f"{what}: alignment_heads is empty")
            for p in heads:
                if len(p) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in p) or not (0 <= p[0] < Ld and 0 <= p[1] < H):
                    raise ValueError(f"{what}: alignment head {p} is not a (decoder layer < {Ld}, head < {H}) pair")
        return heads

    @torch.no_grad()
    def align_tokens(self, mel, tokens, prompt_len: int, alignment_heads=None, medfilt_width: int = 7, *, return_cost: bool = False):
        """token-level timestamps, as Whisper's find_alignment computes them -> TokenAlignment(starts, ends, n_tokens), all on the
        device; no host sync.

        mel: as for generate (a tensor, or a list of clips of different lengths).  tokens: a (B, T) integer tensor, or a list of B
        1-D tensors of different lengths (right-padded here): each is the full sequence, the prompt of prompt_len tokens (one int
        for the batch), the generated tokens and a final token.  alignment_heads: a list of (decoder layer, head) pairs; None takes
        every head of the upper half of the decoder layers.
        One teacher-forced decoder pass collects the selected layers' cross-attention queries; their probabilities over the item's
        audio frames are formed in fp32 (softmax(q k^T / sqrt(dh)), frames >= the clip's length blocked), ops.alignment_cost
        z-normalises them over the tokens, median-filters them over the frames (medfilt_width) and averages the heads, and
        ops.dtw_align warps the rows [prompt_len, n_tokens - 1) of the negated map (Whisper drops the prompt and the final token)
        onto the item's frames.  starts / ends (B, T) int32 are each token's first and last ENCODER frame (this model has no
        convolutional downsampling: a frame is a mel frame), -1 outside the aligned rows.  return_cost=True also returns the
        (B, T, T_audio) cost matrix the warping ran on."""
        info, lens, heads = self._align_check(mel, tokens, prompt_len, alignment_heads, medfilt_width)
        ids, n_tokens = self._align_ids(tokens, lens, info.device)
        starts, ends, cost, _ = self._align(mel, ids, n_tokens, prompt_len, heads, medfilt_width)
        out = TokenAlignment(starts, ends, n_tokens)
        return (out, cost) if return_cost else out

    @staticmethod
    def _align_ids(tokens, lens: List[int], dev):
        """the padded (B, T) ids and the device lengths of align_tokens' token argument (a tensor, or a list right-padded here)"""
        B, T = len(lens), max(lens)
        if isinstance(tokens, torch.Tensor):
            ids = tokens
        else:
            ids = torch.zeros(B, T, dtype=tokens[0].dtype, device=dev)
            for b, t in enumerate(tokens):
                ids[b, :lens[b]] = t
        n_tokens = torch.tensor(lens, dtype=torch.int32)
        if dev.type == "cuda":                                         # an asynchronous copy: the host does not wait for it
            n_tokens = n_tokens.pin_memory().to(dev, non_blocking=True)
        return ids, n_tokens

    def _align(self, mel, ids: torch.Tensor, n_tokens: torch.Tensor, prompt_len: int, heads, medfilt_width: int,
               token_probs: bool = False, eot: Optional[int] = None):
        """the alignment pass of align_tokens, align_words and transcribe's word timestamps, on padded ids (B, T) and device
        lengths n_tokens (B,) int32 -> (starts, ends, cost, tok_probs).  tok_probs is None, or with token_probs the fp32 (B, T)
        probability the same teacher-forced pass gives token p + 1 at position p, over the columns below eot (all when None): a
        token at or above eot is read as eot - 1; column T - 1 is unspecified."""
        dev, (B, T) = ids.device, ids.shape
        enc = self.encode(mel)[0]
        enc_out, audio_lens = _enc_parts(enc)
        Ta = enc_out.shape[1]
        layers = sorted({l for l, _ in heads})
        queries, hooks = {}, []
        for l in layers:                                               # cross_attn.q_proj(ln2(x)) of the selected layers
            hooks.append(self.decoder[l].cross_attn.q_proj.register_forward_hook(
                lambda mod, args, out, l=l: queries.__setitem__(l, out)))
        try:
            logits = self.decode(enc, ids)
        finally:
            for h in hooks:
                h.remove()
        H, Dh = self.cfg.n_head, self.cfg.n_embd // self.cfg.n_head
        ck, _ = self._cross_kv(enc_out)
        q = torch.stack([queries[l].view(B, T, H, Dh)[:, :, h] for l, h in heads], dim=1).float()          # (B, S, T, dh)
        k = torch.stack([ck[l][:, :, h] for l, h in heads], dim=1).float()                                 # (B, S, Ta, dh)
        qk = torch.matmul(q, k.transpose(2, 3)) * Dh ** -0.5
        if audio_lens is None:
            n_frames = torch.full((B,), Ta, dtype=torch.int32, device=dev)
        else:
            n_frames = audio_lens
            qk = qk.masked_fill((torch.arange(Ta, device=dev).unsqueeze(0) >= audio_lens.unsqueeze(1)).view(B, 1, 1, Ta), float("-inf"))
        probs = torch.softmax(qk, dim=-1)
        cost = ops.alignment_cost(probs, n_tokens, n_frames, medfilt_width)
        starts, ends = ops.dtw_align(cost, n_tokens - 1, n_frames, row0=prompt_len)
        tok_probs = None
        if token_probs:
            Vr = logits.shape[-1] if eot is None else eot
            nxt = F.pad(ids[:, 1:], (0, 1)).to(torch.int32).clamp(0, Vr - 1).reshape(B * T)
            tok_probs = ops.token_logprob(logits.view(B * T, -1)[:, :Vr], nxt).exp().view(B, T)
        return starts, ends, cost, tok_probs

    @torch.no_grad()
    def align_words(self, mel, tokens, prompt_len: int, word_rules: "ops.WordRules", alignment_heads=None, medfilt_width: int = 7,
                    median_word_frames: Optional[int] = None, *, eot_token_id: Optional[int] = None) -> WordAlignment:
        """word-level timestamps, as Whisper's find_alignment and add_word_timestamps compute them -> WordAlignment(starts, ends,
        probs, tok_begin, tok_end, n_words), all on the device; no host sync.

        mel, tokens, alignment_heads, medfilt_width: as for align_tokens.  Each sequence of n tokens is prompt_len prompt tokens,
        one lead-in token (Whisper's <|notimestamps|>), the text and a final token: the words are formed from
        tokens[prompt_len + 1 : n - 1], and the longest sequence must hold at least one text token.  word_rules: the ops.WordRules
        of the model's vocabulary.  median_word_frames: ops.word_spans' median_cap (Whisper's 0.7 s; None: no cap).
        The alignment pass is align_tokens' own; text token i begins at times[i] = starts[prompt_len + i], i in [0, n_text], with
        starts what align_tokens returns for the same call (Whisper's convention: the cross-attention row at position p times
        token p + 1), and its probability is exp(ops.token_logprob(logits[:, p, :eot_token_id], tokens[:, p + 1])) at
        p = prompt_len + i, from the same teacher-forced pass, over the columns below eot_token_id as Whisper restricts them
        (over all columns when it is None).  Text tokens are expected below eot_token_id, as Whisper's are; the ids live on the
        device, so one at or above it is not refused: its probability is read at column eot_token_id - 1 (the clamp of
        ops.token_logprob) and is meaningless.  ops.word_spans then groups and times the words; tok_begin / tok_end are shifted to
        positions of the full sequence."""
        what = "align_words"
        info, lens, heads = self._align_check(mel, tokens, prompt_len, alignment_heads, medfilt_width, what)
        if not isinstance(word_rules, ops.WordRules) or word_rules.vocab_size != self.cfg.vocab_size:
            raise ValueError(f"{what}: word_rules must be an ops.WordRules of the model's vocabulary ({self.cfg.vocab_size}), got "
                             f"{getattr(word_rules, 'vocab_size', type(word_rules).__name__)!r}")
        if max(lens) < prompt_len + 3:
            raise ValueError(f"{what}: no sequence holds a text token between the lead-in and the final token: the longest has "
                             f"{max(lens)} tokens, prompt_len = {prompt_len}")
        cap = self._median_cap_check(median_word_frames, what)
        if eot_token_id is not None and (isinstance(eot_token_id, bool) or not isinstance(eot_token_id, int)
                                         or not 2 <= eot_token_id <= self.cfg.vocab_size):
            raise ValueError(f"{what}: eot_token_id must be None or an int in [2, vocab_size = {self.cfg.vocab_size}], got {eot_token_id!r}")
        ids, n_tokens = self._align_ids(tokens, lens, info.device)
        w = self._word_pass(mel, ids, n_tokens, prompt_len, heads, medfilt_width, word_rules, cap, eot_token_id)
        shift = lambda t: torch.where(t >= 0, t + (prompt_len + 1), t)                 # noqa: E731
        return WordAlignment(w.starts, w.ends, w.probs, shift(w.tok_begin), shift(w.tok_end), w.n_words)

    @staticmethod
    def _median_cap_check(median_word_frames, what: str) -> Optional[int]:
        if median_word_frames is not None and (isinstance(median_word_frames, bool) or not isinstance(median_word_frames, int)
                                               or not 0 <= median_word_frames < 2 ** 30):
            raise ValueError(f"{what}: median_word_frames must be None or an int in [0, 2^30) of frames, got {median_word_frames!r}")
        return median_word_frames

    def _word_pass(self, mel, ids, n_tokens, prompt_len: int, heads, medfilt_width: int, word_rules, cap, eot) -> "ops.WordSpans":
        """the alignment pass and ops.word_spans on padded ids: the words of ids[:, prompt_len + 1 : n - 1], token indices relative
        to prompt_len + 1"""
        T = ids.shape[1]
        starts, _, _, tok_probs = self._align(mel, ids, n_tokens, prompt_len, heads, medfilt_width, True, eot)
        text = ids.to(torch.int32)[:, prompt_len + 1:T - 1]
        return ops.word_spans(text, starts[:, prompt_len:T - 1], tok_probs[:, prompt_len:T - 2], n_tokens - (prompt_len + 2), word_rules, cap)

    # ---- language detection; inference only ----
    def _language_check(self, mel, sot_ids, languages, what: str) -> torch.Tensor:
        """detect_language's argument checks -> the decoder's ids, (B, T_s) on the mel's device; ValueErrors before any device
        work"""
        V = self.cfg.vocab_size
        if not isinstance(languages, ops.LanguageTokens):
            raise ValueError(f"{what}: languages must be an ops.LanguageTokens, got {type(languages).__name__}")
        if languages.vocab_size != V:
            raise ValueError(f"{what}: the languages were built for vocab_size = {languages.vocab_size}, the model has {V}")
        alens = self._audio_check(mel, what)
        if alens is None:
            if mel.dim() != 3 or mel.shape[0] < 1 or mel.shape[2] != self.cfg.n_mels or not 1 <= mel.shape[1] <= self.cfg.n_audio_ctx:
                raise ValueError(f"{what}: mel must be a (B, T, n_mels = {self.cfg.n_mels}) tensor with 1 <= T <= n_audio_ctx = "
                                 f"{self.cfg.n_audio_ctx} or a non-empty list of B (T_b, n_mels) tensors, got {tuple(mel.shape)}")
            B, dev = mel.shape[0], mel.device
        else:
            B, dev = len(alens), mel[0].device
        if isinstance(sot_ids, torch.Tensor):
            if (sot_ids.dim() not in (1, 2) or sot_ids.dtype.is_floating_point or sot_ids.dtype.is_complex
                    or sot_ids.dtype == torch.bool or sot_ids.shape[-1] < 1):
                raise ValueError(f"{what}: sot_ids must be an int or an integer (T_s,) or (B, T_s) tensor with T_s >= 1, got "
                                 f"{tuple(sot_ids.shape)} {sot_ids.dtype}")
            if sot_ids.dim() == 2 and sot_ids.shape[0] != B:
                raise ValueError(f"{what}: {sot_ids.shape[0]} rows of sot_ids for a batch of {B} mel inputs")
            if sot_ids.shape[-1] > self.cfg.n_text_ctx:
                raise ValueError(f"{what}: T_s = {sot_ids.shape[-1]} exceeds n_text_ctx = {self.cfg.n_text_ctx}")
            if sot_ids.device != dev:
                raise ValueError(f"{what}: sot_ids are on {sot_ids.device}, the mel on {dev}")
            if not sot_ids.is_cuda and bool(((sot_ids < 0) | (sot_ids >= V)).any()):   # host values: the host can know
                raise ValueError(f"{what}: an id of sot_ids lies outside [0, vocab_size = {V})")
            return sot_ids if sot_ids.dim() == 2 else sot_ids.unsqueeze(0).expand(B, -1)
        if isinstance(sot_ids, bool) or not isinstance(sot_ids, int) or not 0 <= sot_ids < V:
            raise ValueError(f"{what}: sot_ids must be an int in [0, vocab_size = {V}) or an integer (T_s,) or (B, T_s) tensor, got "
                             f"{sot_ids!r}")
        return torch.full((B, 1), sot_ids, dtype=torch.long, device=dev)

    @torch.no_grad()
    def detect_language(self, mel, sot_ids, languages: "ops.LanguageTokens") -> LanguageDetection:
        """Whisper's detect_language -> LanguageDetection(tokens (B,) int32, probs (B, n) fp32), on the device.

        mel: as for `encode`, a (B, T, n_mels) tensor or a list of B clips of different lengths, 1 <= T_b <= n_audio_ctx.
        sot_ids: the tokens in front of the language token, an int, a (T_s,) tensor for every clip or a (B, T_s) integer tensor,
        T_s >= 1 (Whisper's is [<|startoftranscript|>]).  languages: the ops.LanguageTokens of the model's vocabulary.
        The result is ops.language_probs(decode(encode(mel)[0], ids)[:, -1], languages): one encoder pass, one teacher-forced
        decoder pass over the T_s tokens (no cache), and one launch that masks everything but the language tokens at the last
        position, takes the softmax over them and their argmax (ties to the smaller token id).  No host synchronisation.
        ValueError before any device work: languages of another type or vocabulary, T_s > n_text_ctx, an id outside the
        vocabulary where the host can see it (an int, a CPU tensor), sot_ids on another device than the mel."""
        ids = self._language_check(mel, sot_ids, languages, "detect_language")
        res = ops.language_probs(self.decode(self.encode(mel)[0], ids)[:, -1], languages)
        return LanguageDetection(res.tokens, res.probs)

    # ---- long-form transcription; inference only ----
    def _transcribe_check(self, mel, prompt_ids, logit_rules, max_new_tokens, window, frames_per_timestamp, num_beams,
                          length_penalty):
        """transcribe's argument checks -> (the clips as a list of (T_b, n_mels) tensors, the window in frames).  What transcribe
        adds is checked here; the clips' first windows and the prompt, one row per clip, then pass _decode_check, as every
        window's decoder call will.  ValueErrors before any device work"""
        what = "transcribe"
        n_ctx = self.cfg.n_audio_ctx
        if isinstance(mel, torch.Tensor):
            if mel.dim() != 3:
                raise ValueError(f"{what}: mel must be a (B, T, n_mels) tensor or a non-empty list of B (T_b, n_mels) tensors, got "
                                 f"{tuple(mel.shape)}")
            mel = list(mel.unbind(0))
        if window is None:
            window = n_ctx
        if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= n_ctx:
            raise ValueError(f"{what}: window must be an int in [1, n_audio_ctx = {n_ctx}], got {window!r}")
        for name, v in (("frames_per_timestamp", frames_per_timestamp), ("max_new_tokens", max_new_tokens), ("num_beams", num_beams)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{what}: {name} must be an int >= 1, got {v!r}")
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or length_penalty != length_penalty:
            raise ValueError(f"{what}: length_penalty must be a number, got {length_penalty!r}")
        if not isinstance(logit_rules, ops.LogitRules) or logit_rules.timestamp_begin is None:
            raise ValueError(f"{what}: logit_rules must be an ops.LogitRules with timestamp_begin set (the segments are cut at "
                             f"the timestamp tokens), got {type(logit_rules).__name__}")
        self._rules_check(logit_rules, None, what)
        if (not isinstance(prompt_ids, torch.Tensor) or prompt_ids.dim() not in (1, 2) or prompt_ids.dtype.is_floating_point
                or prompt_ids.dtype.is_complex or prompt_ids.dtype == torch.bool):
            raise ValueError(f"{what}: prompt_ids must be an integer (T_p,) or (B, T_p) tensor, got "
                             f"{(tuple(prompt_ids.shape), prompt_ids.dtype) if isinstance(prompt_ids, torch.Tensor) else type(prompt_ids).__name__}")
        first = [m[:window] if isinstance(m, torch.Tensor) and m.dim() == 2 else m for m in mel] if isinstance(mel, (list, tuple)) else mel
        B = len(first) if isinstance(first, (list, tuple)) else 0
        prompts = prompt_ids if prompt_ids.dim() == 2 else prompt_ids.unsqueeze(0).expand(B, -1)
        mel_info = self._decode_check(first, prompts, max_new_tokens, what, ("num_beams", num_beams), 2 if num_beams > 1 else 0)[0]
        if prompt_ids.device != mel_info.device:
            raise ValueError(f"{what}: prompt_ids are on {prompt_ids.device}, the mel on {mel_info.device}")
        return list(mel), window

    def _fallback_check(self, T_p: int, temperatures, logprob_threshold, no_speech_threshold, no_speech_token_id, sot_index,
                        compression_ratio_threshold, compression_ratio, num_samples, seed) -> _Fallback:
        """the checks of transcribe's temperature fallback and no-speech skip -> the policy; ValueErrors before any device work"""
        what = "transcribe"

        def _num(x):
            return not isinstance(x, bool) and isinstance(x, (int, float)) and x == x

        if _num(temperatures):
            temperatures = (temperatures,)
        if not isinstance(temperatures, (list, tuple)) or len(temperatures) == 0:
            raise ValueError(f"{what}: temperatures must be a non-empty sequence of numbers, got {temperatures!r}")
        for i, t in enumerate(temperatures):
            if not _num(t) or t < 0 or (i > 0 and not t > temperatures[i - 1]):
                raise ValueError(f"{what}: temperatures must be increasing numbers >= 0, got {tuple(temperatures)!r}")
            if t > 0:
                ops._sample_params(t, 0, 1.0, what)
        for name, v in (("logprob_threshold", logprob_threshold), ("no_speech_threshold", no_speech_threshold),
                        ("compression_ratio_threshold", compression_ratio_threshold)):
            if v is not None and not _num(v):
                raise ValueError(f"{what}: {name} must be None or a number, got {v!r}")
        if no_speech_threshold is not None and no_speech_token_id is None:
            raise ValueError(f"{what}: no_speech_threshold needs no_speech_token_id")
        if compression_ratio is not None and not callable(compression_ratio):
            raise ValueError(f"{what}: compression_ratio must be None or a callable, got {type(compression_ratio).__name__}")
        if compression_ratio_threshold is not None and compression_ratio is None:
            raise ValueError(f"{what}: compression_ratio_threshold needs a compression_ratio callable (the ratio needs a tokenizer "
                             f"and a compressor, which stay outside this library)")
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 1 <= num_samples <= ops.BEAM_MAX_K:
            raise ValueError(f"{what}: num_samples must be an int in [1, {ops.BEAM_MAX_K}], got {num_samples!r}")
        if num_samples > 1 and not temperatures[-1] > 0:
            raise ValueError(f"{what}: num_samples = {num_samples} needs a temperature above 0 (temperature 0 is not sampled)")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"{what}: seed must be an int, got {seed!r}")
        self._stats_check(True, no_speech_token_id, sot_index, None, T_p, what)
        return _Fallback(tuple(float(t) for t in temperatures), logprob_threshold, no_speech_threshold, no_speech_token_id,
                         sot_index, compression_ratio_threshold, compression_ratio, num_samples, seed)

    def _condition_check(self, B: int, T_p: int, max_new_tokens: int, condition_on_previous_text, initial_prompt, sot_prev_token_id,
                         max_prompt_tokens, prompt_reset_temperature) -> Optional[_Conditioning]:
        """the checks of transcribe's conditioning on the previous text -> None with every keyword at its default (the loop then
        runs as it does without them), else the policy; ValueErrors before any device work"""
        what = "transcribe"

        def _int(x):
            return not isinstance(x, bool) and isinstance(x, int)

        if not isinstance(condition_on_previous_text, bool):
            raise ValueError(f"{what}: condition_on_previous_text must be a bool, got {condition_on_previous_text!r}")
        t = prompt_reset_temperature
        if isinstance(t, bool) or not isinstance(t, (int, float)) or t != t:
            raise ValueError(f"{what}: prompt_reset_temperature must be a number, got {t!r}")
        if sot_prev_token_id is not None and (not _int(sot_prev_token_id) or not 0 <= sot_prev_token_id < self.cfg.vocab_size):
            raise ValueError(f"{what}: sot_prev_token_id must be an int in [0, vocab_size = {self.cfg.vocab_size}), got "
                             f"{sot_prev_token_id!r}")
        if max_prompt_tokens is not None and (not _int(max_prompt_tokens) or max_prompt_tokens < 1):
            raise ValueError(f"{what}: max_prompt_tokens must be None or an int >= 1, got {max_prompt_tokens!r}")
        seeds = None
        if initial_prompt is not None:
            seeds = [initial_prompt] * B if isinstance(initial_prompt, torch.Tensor) else initial_prompt
            if not isinstance(seeds, (list, tuple)) or len(seeds) != B:
                raise ValueError(f"{what}: initial_prompt must be a 1-D integer tensor or a list of {B} of them (one per clip), got "
                                 f"{type(initial_prompt).__name__}"
                                 + (f" of {len(seeds)}" if isinstance(seeds, (list, tuple)) else ""))
            for b, p in enumerate(seeds):
                if (not isinstance(p, torch.Tensor) or p.dim() != 1 or p.dtype.is_floating_point or p.dtype.is_complex
                        or p.dtype == torch.bool):
                    raise ValueError(f"{what}: initial_prompt {b} must be a 1-D integer tensor, got "
                                     f"{(tuple(p.shape), p.dtype) if isinstance(p, torch.Tensor) else type(p).__name__}")
            seeds = list(seeds)
        if not condition_on_previous_text and seeds is None:
            return None
        if sot_prev_token_id is None:
            raise ValueError(f"{what}: condition_on_previous_text and initial_prompt need sot_prev_token_id (the token in front of "
                             f"the previous text)")
        n = self.cfg.n_text_ctx // 2 - 1 if max_prompt_tokens is None else max_prompt_tokens
        if n < 1:
            raise ValueError(f"{what}: n_text_ctx = {self.cfg.n_text_ctx} leaves no room for previous text "
                             f"(n_text_ctx // 2 - 1 = {n})")
        if T_p + 1 + n + max_new_tokens > self.cfg.n_text_ctx:
            raise ValueError(f"{what}: T_p + 1 + max_prompt_tokens + max_new_tokens = {T_p} + 1 + {n} + {max_new_tokens} = "
                             f"{T_p + 1 + n + max_new_tokens} exceeds n_text_ctx = {self.cfg.n_text_ctx}")
        return _Conditioning(condition_on_previous_text, n, sot_prev_token_id, seeds, float(t))

    @staticmethod
    def _history_init(cond: _Conditioning, B: int, dev):
        """the token history of B clips -> (hist (B, n) int32, hist_len (B,) int32 on the device, the host's mirror of
        hist_len): empty, or seeded with the last n tokens of each clip's initial prompt"""
        hist = torch.zeros(B, cond.n, dtype=torch.int32, device=dev)
        len_b = [0] * B
        if cond.seeds is None:
            return hist, torch.zeros(B, dtype=torch.int32, device=dev), len_b
        for b, p in enumerate(cond.seeds):
            len_b[b] = min(cond.n, int(p.shape[0]))
            if len_b[b]:
                hist[b, :len_b[b]] = p[p.shape[0] - len_b[b]:].to(device=dev, dtype=torch.int32)
        hist_len = torch.tensor(len_b, dtype=torch.int32)
        if dev.type == "cuda":                                         # an asynchronous copy: the host does not wait for it
            hist_len = hist_len.pin_memory().to(dev, non_blocking=True)
        return hist, hist_len, len_b

    def _decode_with_fallback(self, dec, wins, prompts, max_new_tokens, eos, num_beams, length_penalty, graph, pol: _Fallback,
                              calls: List[int], build=None):
        """one set of windows under transcribe's policy (Whisper's decode_with_fallback, then should_skip) -> (rows (A, cap) on
        the device, and per window, as host lists: the temperature kept, avg_logprob, no_speech_prob, compression ratio, skipped).
        calls: a one-element list, the number of sample calls this transcribe has made so far (call k uses seed + k).
        build: with conditioning on the previous text, build(window indices) makes the _PreparedPrompts of exactly the rows of
        an attempt; its rows come back at the attempt's own width and are cut to the sot sequence and the generated tokens, so
        the rows of every attempt are (T_p + max_new_tokens) wide, T_p the sot sequence's length."""
        A, T_p = len(wins), prompts.shape[1]
        dev, nan = prompts.device, float("nan")
        kw = dict(return_stats=True, no_speech_token_id=pol.no_speech_token_id, sot_index=pol.sot_index)
        kept = [None] * A
        temp, avg, nsp, ratio = [pol.temperatures[0]] * A, [nan] * A, [nan] * A, [nan] * A
        pending = list(range(A))
        for ti, t in enumerate(pol.temperatures):
            sub_w = [wins[i] for i in pending]
            if build is not None:
                sub_p = build(pending)
            else:
                sub_p = prompts if len(pending) == A else torch.stack([prompts[i] for i in pending])
            if t == 0 and num_beams > 1:
                rows, _, st = dec.beam_search(sub_w, sub_p, max_new_tokens, num_beams, eos, length_penalty, graph, **kw)
                a = st.sum_logprobs / st.n_tokens
            elif t == 0:
                rows, st = dec.generate(sub_w, sub_p, max_new_tokens, eos, graph, **kw)
                a = st.sum_logprobs / st.n_tokens
            else:
                toks, _, st = dec.sample(sub_w, sub_p, max_new_tokens, temperature=t, num_samples=pol.num_samples, eos_token_id=eos,
                                         seed=pol.seed + calls[0], graph=graph, **kw)
                calls[0] += 1
                every = st.sum_logprobs / st.n_tokens                  # (rows, num_samples): keep the best, ties to the first
                best = every.argmax(1, keepdim=True)
                a = every.gather(1, best).squeeze(1)
                rows = toks.gather(1, best.unsqueeze(2).expand(-1, 1, toks.shape[2])).squeeze(1)
            if build is not None:
                rows = rows[:, sub_p.ids.shape[1] - T_p:]
            ns = st.no_speech_prob if st.no_speech_prob is not None else torch.full_like(a, nan)
            host = torch.empty(len(pending), 2, dtype=torch.float32)
            if dev.type == "cuda":
                host = host.pin_memory()
            host.copy_(torch.stack((a, ns.to(torch.float32)), dim=1))               # the attempt's one fp32 copy to the host
            gen = rows[:, T_p:].to(torch.int64).cpu() if pol.compression_ratio is not None else None
            for k, (i, (ak, nk)) in enumerate(zip(pending, host.tolist())):
                kept[i], temp[i], avg[i], nsp[i] = rows[k], t, ak, nk
                if gen is not None:
                    hit = (gen[k] == eos).nonzero()
                    ratio[i] = float(pol.compression_ratio(gen[k, :int(hit[0])] if hit.numel() else gen[k]))
            if ti + 1 == len(pol.temperatures):
                break                                                  # the last temperature's result is kept whatever it is
            again = []
            for i in pending:
                need = ((pol.compression_ratio_threshold is not None and ratio[i] > pol.compression_ratio_threshold)
                        or (pol.logprob_threshold is not None and avg[i] < pol.logprob_threshold))
                if (need and pol.no_speech_threshold is not None and pol.logprob_threshold is not None
                        and nsp[i] > pol.no_speech_threshold and avg[i] < pol.logprob_threshold):
                    need = False                                       # silence: a higher temperature would not help
                if need:
                    again.append(i)
            pending = again
            if not pending:
                break
        skipped = [pol.no_speech_threshold is not None and nsp[i] > pol.no_speech_threshold
                   and not (pol.logprob_threshold is not None and avg[i] > pol.logprob_threshold) for i in range(A)]
        rows = kept[0].unsqueeze(0) if A == 1 else torch.stack(kept)
        return rows, temp, avg, nsp, ratio, skipped

    @torch.no_grad()
    def transcribe(self, mel, prompt_ids: torch.Tensor, logit_rules: "ops.LogitRules", max_new_tokens: int, *,
                   window: Optional[int] = None, frames_per_timestamp: int = 1, num_beams: int = 1, length_penalty: float = 1.0,
                   graph: bool = False) -> List[Transcript]:
        """long-form transcription: the window loop that with_logit_rules(logit_rules).transcribe documents, without the
        temperature fallback and the no-speech skip (their keywords are that method's; this signature is pinned)."""
        return self._transcribe(mel, prompt_ids, logit_rules, max_new_tokens, window=window, frames_per_timestamp=frames_per_timestamp,
                                num_beams=num_beams, length_penalty=length_penalty, graph=graph)

    def _transcribe(self, mel, prompt_ids: torch.Tensor, logit_rules: "ops.LogitRules", max_new_tokens: int, *,
                    window: Optional[int] = None, frames_per_timestamp: int = 1, num_beams: int = 1, length_penalty: float = 1.0,
                    graph: bool = False, temperatures=(0.0,), logprob_threshold: Optional[float] = None,
                    no_speech_threshold: Optional[float] = None, no_speech_token_id: Optional[int] = None, sot_index: int = 0,
                    compression_ratio_threshold: Optional[float] = None, compression_ratio=None, num_samples: int = 1,
                    seed: int = 0, return_log: bool = False, word_timestamps: bool = False, word_rules=None, alignment_heads=None,
                    medfilt_width: int = 7, median_word_frames: Optional[int] = None, languages=None, language_index: int = 1,
                    repeat_rules=None, condition_on_previous_text: bool = False, initial_prompt=None, sot_prev_token_id: Optional[int] = None,
                    max_prompt_tokens: Optional[int] = None, prompt_reset_temperature: float = 0.5):
        """long-form transcription, Whisper's transcribe loop over windows for a batch of clips -> a list of B Transcript(starts,
        ends, tokens, offsets), all on the device.

        mel: a list of B (T_b, n_mels) clips, T_b >= 1 and NOT bounded by n_audio_ctx, or a (B, T, n_mels) tensor.  window: the
        frames decoded at a time, at most n_audio_ctx (the default).  prompt_ids: a (T_p,) tensor, or (B, T_p): the same
        start-of-transcript sequence opens every window of an item.  logit_rules: an ops.LogitRules with timestamp_begin set; the
        eos token is its eos_token_id.  frames_per_timestamp: see ops.timestamp_segments.
        Each item keeps a host integer seek_b, 0 at first.  While any seek_b < T_b: the windows mel_b[seek_b:seek_b + window] of
        the items still running go, as a list of clips of different lengths, through with_logit_rules(logit_rules).generate (or
        .beam_search with num_beams > 1; graph is passed on); ops.timestamp_segments cuts the decoded rows into segments and
        gives each row's advance, in one launch; ONE (A, 3) int32 copy to pinned host memory brings advance, n_segments and the
        number of tokens the segments span back (the only synchronisation the loop adds to the decoders' own: with graph=True
        every window's decoder call opens its capture with a device synchronise; the host needs the third to size the token
        views); seek_b += advance, and the window's segments join item b's transcript, their frames shifted by the window's
        seek_b.  advance >= 1, so the loop ends after at most T_b windows.  The tokens behind a
        window's last cut are in no segment: the next window starts at that cut and decodes them again.

        The temperature fallback and the no-speech skip (Whisper's decode_with_fallback and should_skip).  With every argument
        below at its default the loop above is all that runs, and no statistics are asked of the decoders.  Otherwise every
        decoder call runs with return_stats=True, and per set of windows:
        1. all active rows decode at temperatures[0]: temperature 0 is generate (beam_search with num_beams > 1), a temperature
           above 0 is sample(temperature, num_samples), of whose samples the one with the largest avg_logprob = sum_logprobs /
           n_tokens is kept (ties to the smaller index);
        2. a row needs fallback when compression_ratio_threshold is set and its ratio exceeds it, or logprob_threshold is set and
           its avg_logprob is below it;
        3. unless no_speech_threshold and logprob_threshold are both set, its no_speech_prob > no_speech_threshold and its
           avg_logprob < logprob_threshold (silence);
        4. the rows that still need it decode again, as a smaller batch of their own windows, at the next temperature; the last
           temperature's result is kept whatever it is;
        5. with no_speech_threshold set, a row whose final no_speech_prob > no_speech_threshold is skipped, unless
           logprob_threshold is set and its avg_logprob > logprob_threshold: it adds no segments and no tokens, and its seek moves
           by the window's length.
        no_speech_prob: the probability of no_speech_token_id at position sot_index of the prompt, before the logit rules.
        compression_ratio: a callable from a 1-D CPU int64 tensor (the generated tokens before the first eos) to a float (Whisper's
        ratio needs a tokenizer and zlib, which stay outside this library); only with it does a window's token row go to the
        host.  The k-th sample call this transcribe makes uses seed + k.  Sampled results depend on the batch's composition (as
        sample's own do: its draw is a function of the row index), so on which rows fell back together.  Every decoding attempt
        adds ONE (rows, 2) fp32 copy to pinned host memory (avg_logprob, no_speech_prob) to the (A, 3) int32 one per set of
        windows, plus the token rows when compression_ratio is given.  A fallback attempt encodes its windows again (the decoders
        take mel).  return_log=True also returns a list of B TranscribeLog, one entry per window.
        ValueError before any device work: temperatures empty, not increasing, negative or NaN; no_speech_threshold without
        no_speech_token_id; compression_ratio_threshold without compression_ratio; num_samples outside [1, 8], or above 1 with no
        temperature above 0; sot_index outside the prompt; no_speech_token_id outside the vocabulary.

        Conditioning on the previous text (Whisper's condition_on_previous_text and initial_prompt).  With the five keywords
        below at their defaults every window is decoded from prompt_ids alone, by the loop above: no history is allocated and
        no launch is added.  With condition_on_previous_text=True or an initial_prompt, clip b keeps a token history on the
        device, hist (B, n) int32 and hist_len (B,), n = max_prompt_tokens, or n_text_ctx // 2 - 1 when that is None (Whisper's
        n_ctx // 2 - 1), and a window of clip b with a history of len_b > 0 tokens is decoded from [sot_prev_token_id, the
        history, prompt_ids].  sot_prev_token_id (Whisper's <|startofprev|>) is required then.  initial_prompt: a 1-D integer
        tensor for all clips, or a list of B 1-D tensors (an empty one: none for that clip); its last n tokens seed the history,
        and it never appears in the Transcript.
        Before EVERY decoder call, a fallback attempt on some of the rows included, ops.window_prompts builds the prompt matrix
        of exactly that call's rows in one launch, at width = T_p + the largest 1 + len_b among its rows with history (T_p when
        none has any: the host keeps len_b as a mirror of hist_len, updated from the token count the (A, 3) copy brings), and
        the decoders take it as a ragged batch, left-padded with a per-row start, or as a uniform one when every row fills the
        width: exactly what their public list form does with the same prompts, so the result equals a host loop over the public
        decoders bit for bit.  prompt_ids sits in the last T_p columns of every row, so no_speech_prob is read at the one column
        width - T_p + sot_index.  After each set of windows ONE ops.prompt_history_update launch gives every row one of:
        - a skipped window (no speech) leaves its clip's history as it is (Whisper continues before its reset check);
        - with condition_on_previous_text False, or a kept temperature above prompt_reset_temperature, the history is cleared
          (Whisper's prompt_reset_since; so without condition_on_previous_text an initial_prompt conditions each clip's first
          window only);
        - else the tokens that join the transcript, timestamp tokens included, are appended and the newest n kept.
        No host synchronisation is added: the rows' clips and modes ride in the pinned upload that carries the windows'
        lengths, the clips of a decoder call in one of their own, and the (A, 3) download is unchanged.  With graph=True each
        decoder call captures anew at its own width.
        ValueError before any device work: sot_prev_token_id missing or outside the vocabulary; n < 1; T_p + 1 + n +
        max_new_tokens > n_text_ctx; an initial_prompt that is neither form; a prompt_reset_temperature that is not a number.

        Word timestamps (Whisper's word_timestamps=True).  With word_timestamps False the four keywords behind it are not
        looked at, and the loop runs the launches and copies described above.  With it, word_rules must be the ops.WordRules of
        the model's vocabulary and logit_rules.no_timestamps_token_id must be set; alignment_heads and medfilt_width are
        align_tokens', median_word_frames is ops.word_spans' median_cap (transcribe_audio fills in Whisper's 0.7 s).  Per set of
        windows, ops.alignment_rows turns the decoded rows and the device count of the tokens their segments span into the
        alignment pass' ids = [prompt_ids, no-timestamps token, the text tokens (no timestamp tokens, no eos), eos] in one
        launch BEFORE the download, which becomes (A, 4) and carries each row's number of text tokens: no synchronisation is
        added.  The host cuts ids to T_p + 2 + the longest text (the width align_tokens' list form pads to); ONE alignment
        pass (align_words' own, probabilities over the columns below eos) runs over the rows that were not skipped and have
        text, with their windows as the clips, and ONE ops.word_spans call groups and times their words.  The words join the
        clip's list with their frames shifted by the window's seek and their token ranges mapped through alignment_rows' col
        into Transcript.tokens.  A window's word count stays on the device: the padded rows are compacted after the loop by one
        boolean selection per clip (a synchronisation each, outside the loop), and one torch.searchsorted per clip against
        Transcript.offsets gives each word's segment.  Returns (transcripts, words), or (transcripts, logs, words) with
        return_log=True; words is a list of B TranscriptWords, and the transcripts equal those of the same call without word
        timestamps.
        ValueError before any device work: word_rules missing or of another vocabulary; no_timestamps_token_id unset; T_p +
        max_new_tokens + 2 > n_text_ctx; malformed heads, width or median_word_frames.

        Repetition (repeat_rules; on RuledDecoding.transcribe they come from with_logit_rules(logit_rules, repeat_rules)): an
        ops.RepeatRules of the model's vocabulary.  Every decoder call of every window and of every fallback temperature applies
        them before the logit rules, over the window's generated tokens only (never the prompt, so never the previous window's
        text).  Build them with ops.RepeatRules.for_whisper(logit_rules, ...): it exempts eos and the timestamp tokens, which the
        segments need to repeat (one segment's end and the next one's start are the same token).  The alignment pass of the word
        timestamps decodes nothing and is not affected.

        Language detection (Whisper's language=None).  With languages None nothing changes: no launch, no buffer, no copy, and
        language_index is not looked at.  With languages an ops.LanguageTokens of the model's vocabulary, prompt_ids' column
        language_index (1 <= language_index < T_p; Whisper's start-of-transcript sequence has the language token at 1) is a
        placeholder: before the window loop ONE detect_language call runs over the B clips' first windows mel_b[:window], as one
        batch of clips of different lengths, from prompt_ids[..., :language_index]; prompt_ids is expanded to a (B, T_p) copy
        on the device, and a device-side copy writes the detected tokens into its column language_index (no value comes to the
        host, and no host synchronisation is added beyond what a device (B, T_p) prompt tensor costs).  The loop then runs exactly
        as if the caller had passed that matrix: every window, fallback attempt, conditioned prompt and alignment pass opens with
        the detected language.  The LanguageDetection is appended as the LAST element of what is returned: (transcripts,
        detection), (transcripts, logs, detection), (transcripts, words, detection) or (transcripts, logs, words, detection).
        ValueError before any device work: languages of another type or vocabulary; language_index outside [1, T_p).
        Out of scope: reusing the detection's encoder output for the first window (Whisper encodes twice too), detection on
        anything but the first window, a vocabulary projection restricted to the language rows, Whisper's pause and
        segment-boundary heuristics on the words (last_speech_timestamp, preferring the segment-level start / end),
        hallucination_silence_threshold, word splitting on unicode code points, an alignment pass
        fused so that it never materialises the probability maps, top-k / top-p inside transcribe, handing the encoded audio over
        to a fallback attempt or to the alignment pass, a device-side compression ratio, and a vocabulary projection of the prompt
        pass restricted to the columns that are read."""
        clips, W = self._transcribe_check(mel, prompt_ids, logit_rules, max_new_tokens, window, frames_per_timestamp, num_beams,
                                           length_penalty)
        pol = self._fallback_check(prompt_ids.shape[-1], temperatures, logprob_threshold, no_speech_threshold, no_speech_token_id,
                                   sot_index, compression_ratio_threshold, compression_ratio, num_samples, seed)
        cond = self._condition_check(len(clips), prompt_ids.shape[-1], max_new_tokens, condition_on_previous_text, initial_prompt,
                                     sot_prev_token_id, max_prompt_tokens, prompt_reset_temperature)
        wt = self._words_check(prompt_ids.shape[-1], max_new_tokens, logit_rules, word_timestamps, word_rules, alignment_heads,
                               medfilt_width, median_word_frames)
        detection = None
        if languages is not None:
            if (isinstance(language_index, bool) or not isinstance(language_index, int)
                    or not 1 <= language_index < prompt_ids.shape[-1]):
                raise ValueError(f"transcribe: language_index must be an int in [1, T_p = {prompt_ids.shape[-1]}) (the language "
                                 f"token's column of prompt_ids, behind the tokens it is detected from), got {language_index!r}")
            detection = self.detect_language([c[:W] for c in clips], prompt_ids[..., :language_index], languages)
            prompt_ids = (prompt_ids if prompt_ids.dim() == 2 else prompt_ids.unsqueeze(0).expand(len(clips), -1)).clone()
            prompt_ids[:, language_index] = detection.tokens       # a device-side copy: the host never sees the language
        plain = (pol.temperatures == (0.0,) and logprob_threshold is None and no_speech_threshold is None
                 and no_speech_token_id is None and compression_ratio is None and not return_log)
        calls = [0]
        dev, B, dec = clips[0].device, len(clips), self.with_logit_rules(logit_rules, repeat_rules)
        build = None
        if cond is not None:
            hist, hist_len, len_b = self._history_init(cond, B, dev)

            def build(idx):                                            # the prompts of one decoder call: its rows' clips idx
                have = [len_b[b] for b in idx]
                width = T_p + max((1 + n for n in have if n > 0), default=0)
                item = torch.tensor(idx, dtype=torch.int32)
                if dev.type == "cuda":                                 # an asynchronous copy: the host does not wait for it
                    item = item.pin_memory().to(dev, non_blocking=True)
                dt = prompt_ids.dtype if prompt_ids.dtype in (torch.int32, torch.int64) else torch.int64
                ids, kv_start = ops.window_prompts(hist, hist_len, item, prompt_ids, cond.prev, width, dt)
                lens_p = [T_p + (1 + n if n > 0 else 0) for n in have]
                return _PreparedPrompts(ids.to(prompt_ids.dtype), None if min(lens_p) == width else kv_start, lens_p, T_p)
        logs = [TranscribeLog([], [], [], [], [], []) for _ in range(B)]
        tb, eos = logit_rules.timestamp_begin, logit_rules.eos_token_id
        T_p = prompt_ids.shape[-1]
        total = [int(c.shape[0]) for c in clips]
        seek, n_tok = [0] * B, [0] * B
        parts = [([], [], [], []) for _ in range(B)]                   # per item: starts, ends, tokens, offsets of each window
        wparts = [([], [], [], [], [], []) for _ in range(B)]          # per item: starts, ends, probs, tok_begin, tok_end, live
        while True:
            act = [b for b in range(B) if seek[b] < total[b]]
            if not act:
                break
            wins = [clips[b][seek[b]:seek[b] + W] for b in act]
            if prompt_ids.dim() == 1:
                prompts = prompt_ids.unsqueeze(0).expand(len(act), -1)
            else:
                prompts = prompt_ids if len(act) == B else torch.stack([prompt_ids[b] for b in act])
            skipped = None
            if not plain:
                rows, temp, avg, nsp, ratio, skipped = self._decode_with_fallback(
                    dec, wins, prompts, max_new_tokens, eos, num_beams, length_penalty, graph, pol, calls,
                    None if build is None else lambda pending: build([act[i] for i in pending]))
                for a, b in enumerate(act):
                    for field, v in zip(logs[b], (seek[b], temp[a], avg[a], nsp[a], ratio[a], skipped[a])):
                        field.append(v)
            else:
                if build is not None:
                    prompts = build(act)
                if num_beams > 1:
                    rows, _ = dec.beam_search(wins, prompts, max_new_tokens, num_beams, eos, length_penalty, graph)
                else:
                    rows = dec.generate(wins, prompts, max_new_tokens, eos, graph)
                if build is not None:                                  # the sot sequence and the generated tokens
                    rows = rows[:, prompts.ids.shape[1] - T_p:]
            lens = torch.tensor([int(w.shape[0]) for w in wins], dtype=torch.int32)
            if build is not None:                                      # per row: 2 leave the history, 1 clear it, 0 append
                kept_t = temp if skipped is not None else [0.0] * len(act)
                modes = [2 if skipped is not None and skipped[a] else int(not cond.on or kept_t[a] > cond.reset_temperature)
                         for a in range(len(act))]
                lens = torch.stack((lens, torch.tensor(act, dtype=torch.int32), torch.tensor(modes, dtype=torch.int32)))
            meta = torch.empty(len(act), 3 if wt is None else 4, dtype=torch.int32)
            if dev.type == "cuda":                                     # an asynchronous copy: the host does not wait for it
                lens, meta = lens.pin_memory().to(dev, non_blocking=True), meta.pin_memory()
            if build is not None:
                lens, item, mode = lens[0], lens[1], lens[2]
            rows32 = rows.to(torch.int32)
            seg = ops.timestamp_segments(rows32, T_p, lens, tb, eos, frames_per_timestamp)
            last = seg.tok_end.gather(1, (seg.n_segments - 1).clamp_min(0).long().unsqueeze(1)).squeeze(1)
            spanned = torch.where(seg.n_segments > 0, last - T_p, 0)   # a window's segments are contiguous from column T_p on
            cols = (seg.advance, seg.n_segments, spanned.to(torch.int32))
            if wt is not None:
                sot = prompt_ids if prompt_ids.dim() == 1 or len(act) == B else torch.stack([prompt_ids[b] for b in act])
                if sot.dtype not in (torch.int32, torch.int64):
                    sot = sot.to(torch.int64)
                ar = ops.alignment_rows(rows32, T_p, cols[2], sot, wt.nots, eos, torch.int32)
                cols += (ar.n_tokens - (T_p + 2),)
            meta.copy_(torch.stack(cols, dim=1))                       # the one synchronisation
            if build is not None:
                ops.prompt_history_update(hist, hist_len, rows32, T_p, spanned.to(torch.int32), item, mode)
            meta = meta.tolist()
            if wt is not None:
                self._window_words(wt, ar, [r[3] for r in meta], skipped, wins, [seek[b] for b in act], [n_tok[b] for b in act],
                                   [wparts[b] for b in act], T_p, eos)
            for a, (adv, n, m) in enumerate(r[:3] for r in meta):
                b = act[a]
                if skipped is not None and skipped[a]:                 # no speech: nothing joins the transcript, seek moves on
                    adv, n, m = int(wins[a].shape[0]), 0, 0
                if build is not None and modes[a] != 2:                # the host's mirror of hist_len
                    len_b[b] = min(cond.n, len_b[b] + m) if modes[a] == 0 else 0
                st, en, tk, off = parts[b]
                st.append(seg.starts[a, :n] + seek[b])
                en.append(seg.ends[a, :n] + seek[b])
                tk.append(rows[a, T_p:T_p + m])
                off.append(seg.tok_begin[a, :n] + (n_tok[b] - T_p))
                seek[b] += adv
                n_tok[b] += m
        out = []
        for b, (st, en, tk, off) in enumerate(parts):
            off.append(torch.full((1,), n_tok[b], dtype=torch.int32, device=dev))
            out.append(Transcript(torch.cat(st), torch.cat(en), torch.cat(tk), torch.cat(off)))
        tail = () if detection is None else (detection,)
        if wt is None:
            if return_log:
                return (out, logs) + tail
            return (out,) + tail if tail else out
        words = []
        for b, wp in enumerate(wparts):
            if wp[0]:
                live = torch.cat(wp[5])
                st, en, pr, tb_, te_ = (torch.cat(x)[live] for x in wp[:5])
            else:                                                      # no window of this clip had text
                st, en, tb_, te_ = (torch.empty(0, dtype=torch.int32, device=dev) for _ in range(4))
                pr = torch.empty(0, dtype=torch.float32, device=dev)
            words.append(TranscriptWords(st, en, pr, tb_, te_, torch.searchsorted(out[b].offsets, tb_, right=True) - 1))
        return ((out, logs, words) if return_log else (out, words)) + tail

    def _words_check(self, T_p: int, max_new_tokens: int, logit_rules, word_timestamps, word_rules, alignment_heads, medfilt_width,
                     median_word_frames) -> Optional[_Words]:
        """the checks of transcribe's word timestamps -> what the loop needs, None without them; ValueErrors before any device
        work"""
        what = "transcribe"
        if not isinstance(word_timestamps, bool):
            raise ValueError(f"{what}: word_timestamps must be a bool, got {word_timestamps!r}")
        if not word_timestamps:
            return None
        if not isinstance(word_rules, ops.WordRules) or word_rules.vocab_size != self.cfg.vocab_size:
            raise ValueError(f"{what}: word_timestamps needs word_rules, an ops.WordRules of the model's vocabulary "
                             f"({self.cfg.vocab_size}), got {getattr(word_rules, 'vocab_size', type(word_rules).__name__)!r}")
        if logit_rules.no_timestamps_token_id is None:
            raise ValueError(f"{what}: word_timestamps needs logit_rules.no_timestamps_token_id (the alignment pass decodes the "
                             f"text behind it)")
        if T_p + max_new_tokens + 2 > self.cfg.n_text_ctx:
            raise ValueError(f"{what}: word_timestamps aligns up to T_p + max_new_tokens + 2 = {T_p + max_new_tokens + 2} tokens, "
                             f"beyond n_text_ctx = {self.cfg.n_text_ctx}")
        heads = self._align_heads_check(alignment_heads, medfilt_width, what)
        return _Words(word_rules, heads, medfilt_width, self._median_cap_check(median_word_frames, what),
                      logit_rules.no_timestamps_token_id)

    def _window_words(self, wt: _Words, ar, n_text: List[int], skipped, wins, seeks: List[int], n_toks: List[int], wparts, T_p: int,
                      eos: int) -> None:
        """the words of one set of windows: one alignment pass and one ops.word_spans call over the rows that were not skipped
        and have text; each row's padded results and a mask of its live words are appended to its clip's wparts"""
        sel = [a for a in range(len(n_text)) if n_text[a] > 0 and not (skipped is not None and skipped[a])]
        if not sel:
            return
        dev = ar.ids.device
        width = T_p + 2 + max(n_text[a] for a in sel)
        ids, n_tokens, col = ar.ids, ar.n_tokens, ar.col
        shift = torch.tensor([[seeks[a] for a in sel], [n_toks[a] - T_p for a in sel], sel], dtype=torch.int32)
        if dev.type == "cuda":                                         # an asynchronous copy: the host does not wait for it
            shift = shift.pin_memory().to(dev, non_blocking=True)
        if len(sel) < len(n_text):
            pick = shift[2].long()
            ids, n_tokens, col = ids[pick], n_tokens[pick], col[pick]
        w = self._word_pass([wins[a] for a in sel], ids[:, :width], n_tokens, T_p, wt.heads, wt.medfilt_width, wt.rules,
                            wt.median_cap, eos)
        live = w.tok_begin >= 0
        seek, base = shift[0].unsqueeze(1), shift[1].unsqueeze(1)
        at = lambda t: col.gather(1, t.clamp_min(0).long())                            # noqa: E731  text token -> column of the row
        for k, v in enumerate((torch.where(live, w.starts + seek, -1), torch.where(live, w.ends + seek, -1), w.probs,
                               torch.where(live, at(w.tok_begin) + base, -1), torch.where(live, at(w.tok_end - 1) + 1 + base, -1),
                               live)):
            for i, a in enumerate(sel):
                wparts[a][k].append(v[i])

    @torch.no_grad()
    def transcribe_audio(self, audio, frontend: "LogMelFrontend", prompt_ids: torch.Tensor, logit_rules: "ops.LogitRules",
                         max_new_tokens: int, **transcribe_kwargs):
        """`transcribe` from waveforms: audio (a (B, L) tensor or a list of B 1-D clips, see LogMelFrontend.forward) goes through
        frontend, the mel it returns through with_logit_rules(logit_rules).transcribe(mel, prompt_ids, max_new_tokens, **transcribe_kwargs)
        -> a list of Transcript (with return_log=True: that list and the logs).  It runs the loop itself, not through the public
        `transcribe`, whose pinned signature cannot take the policy's keywords: a subclass that overrides `transcribe` overrides
        `_transcribe` for this entry point.
        Every keyword of transcribe passes through (the temperature fallback and the no-speech skip included; with return_log=True
        the logs come back beside the transcripts; with word_timestamps=True the words too, and a median_word_frames the caller
        leaves out becomes round(0.7 / frontend.frame_seconds), Whisper's 0.7 s; with languages the LanguageDetection comes back last).  A segment's frames times frontend.frame_seconds are seconds.  ValueError when frontend.n_mels is not the model's."""
        if not isinstance(frontend, LogMelFrontend) or frontend.n_mels != self.cfg.n_mels:
            raise ValueError(f"transcribe_audio: frontend must be a LogMelFrontend with n_mels = {self.cfg.n_mels} (the model's), got "
                             f"{getattr(frontend, 'n_mels', type(frontend).__name__)!r}")
        if transcribe_kwargs.get("word_timestamps") and transcribe_kwargs.get("median_word_frames") is None:
            transcribe_kwargs["median_word_frames"] = round(0.7 / frontend.frame_seconds)       # Whisper's 0.7 s cap
        return self._transcribe(frontend(audio), prompt_ids, logit_rules, max_new_tokens, **transcribe_kwargs)

    @torch.no_grad()
    def get_gate_maps(self, mel: torch.Tensor):
        """per-layer time gates of the encoder, (B, L_enc, T_audio), as encode returns them; for a list of clips (see encode) the
        columns >= T_b of item b are 1.  The gates depend on the mel map alone, so the encoder is not run."""
        mel, audio_lens = self._audio_pad(mel, self._audio_check(mel, "get_gate_maps"))
        assert mel.shape[2] == self.cfg.n_mels, "mel dim mismatch"
        return self._gates(mel, audio_lens).to(_gate_dtype(mel))


class LogMelFrontend(nn.Module):
    """waveform -> Whisper's log-mel spectrogram (ops.log_mel: the HIP STFT kernel), the stage in front of `WhisperMoP.encode`,
    `generate`, `beam_search`, `sample`, `align_tokens` and `transcribe`.  The Slaney mel filterbank (ops.mel_filterbank) is a
    non-persistent buffer.  Audio must be mono float samples at sample_rate; ResampledLogMelFrontend takes any other rate, int16
    samples and several channels (ops.resample in front).  Out of scope: Whisper's 30 s zero padding, file decoding."""

    def __init__(self, n_mels: int = 80, sample_rate: int = 16000, n_fft: int = 400, hop_length: int = 160):
        super().__init__()
        for name, v in (("n_mels", n_mels), ("sample_rate", sample_rate), ("n_fft", n_fft), ("hop_length", hop_length)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"LogMelFrontend: {name} must be an int >= 1, got {v!r}")
        if n_fft % 2 or hop_length > n_fft:
            raise ValueError(f"LogMelFrontend: needs an even n_fft and hop_length <= n_fft, got n_fft = {n_fft}, hop_length = {hop_length}")
        self.n_mels, self.sample_rate, self.n_fft, self.hop_length = n_mels, sample_rate, n_fft, hop_length
        self.register_buffer("filters", ops.mel_filterbank(sample_rate, n_fft, n_mels), persistent=False)

    @property
    def frame_seconds(self) -> float:
        """the duration of one mel frame"""
        return self.hop_length / self.sample_rate

    @property
    def min_samples(self) -> int:
        """the shortest clip: one frame, and a reflection that stays inside the clip"""
        return max(self.hop_length, self.n_fft // 2 + 1)

    @torch.no_grad()
    def forward(self, audio):
        """audio: a (B, L) tensor of samples -> (B, L // hop_length, n_mels) fp32; or a list of B 1-D clips of different lengths
        -> a list of B (T_b, n_mels) tensors, T_b = L_b // hop_length, views of one padded buffer (what the model's entry points
        take as a list).  The clips are padded into one (B, L_max) buffer and their lengths go to the device as one pinned
        asynchronous copy; every clip is reflected at its own ends and clamped against its own maximum."""
        what = "LogMelFrontend"
        if isinstance(audio, torch.Tensor):
            if audio.dim() != 2:
                raise ValueError(f"{what}: audio must be a (B, L) tensor or a non-empty list of B 1-D clips, got {tuple(audio.shape)}")
            return ops.log_mel(audio, self.filters, self.n_fft, self.hop_length)
        if not isinstance(audio, (list, tuple)) or len(audio) == 0:
            raise ValueError(f"{what}: audio must be a (B, L) tensor or a non-empty list of B 1-D clips")
        for b, x in enumerate(audio):
            if not isinstance(x, torch.Tensor) or x.dim() != 1:
                raise ValueError(f"{what}: clip {b} must be a 1-D tensor of samples, got "
                                 f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
            if x.dtype != audio[0].dtype or not x.dtype.is_floating_point:
                raise ValueError(f"{what}: clips must share one floating dtype, clip {b} is {x.dtype}")
            if x.device != audio[0].device:
                raise ValueError(f"{what}: clip {b} is on {x.device}, clip 0 on {audio[0].device}")
            if x.shape[0] < self.min_samples:
                raise ValueError(f"{what}: clip {b} has {x.shape[0]} samples, fewer than max(hop_length, n_fft/2 + 1) = {self.min_samples}")
        n = [int(x.shape[0]) for x in audio]
        padded = torch.zeros(len(n), max(n), dtype=audio[0].dtype, device=audio[0].device)
        for b, x in enumerate(audio):
            padded[b, :n[b]] = x
        lens = None
        if min(n) != max(n):
            lens = torch.tensor(n, dtype=torch.int32)
            if padded.device.type == "cuda":                           # an asynchronous copy: the host does not wait for it
                lens = lens.pin_memory().to(padded.device, non_blocking=True)
        mel = ops.log_mel(padded, self.filters, self.n_fft, self.hop_length, lens)
        return [mel[b, :n[b] // self.hop_length] for b in range(len(n))]


def _pad_waveforms(audio, min_samples: int, what: str):
    """a non-empty list of clips, each 1-D (L_b,) or 2-D (C_b, L_b), of one dtype and device -> (padded, lens, n): the clips in one
    zero-padded buffer, their lengths as an int32 device tensor (one pinned asynchronous copy; None when all are equal) and as
    Python ints.  Clips of one form stay as they are, (B, L_max) or (B, C, L_max) in their own dtype, and ops.resample converts and
    averages them; a list that mixes channel counts is averaged clip by clip here with the same operations in the same order
    (ops._rs_mono), so a clip comes out as it would alone either way."""
    if not isinstance(audio, (list, tuple)) or len(audio) == 0:
        raise ValueError(f"{what}: audio must be a (B, L) or (B, C, L) tensor or a non-empty list of (L_b,) or (C, L_b) clips")
    for b, x in enumerate(audio):
        if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or 0 in x.shape:
            raise ValueError(f"{what}: clip {b} must be a non-empty 1-D (L,) or 2-D (C, L) tensor of samples, got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        if x.dtype != audio[0].dtype or not (x.dtype.is_floating_point or x.dtype == torch.int16):
            raise ValueError(f"{what}: clips must share one floating or int16 dtype, clip {b} is {x.dtype}")
        if x.device != audio[0].device:
            raise ValueError(f"{what}: clip {b} is on {x.device}, clip 0 on {audio[0].device}")
        if x.shape[-1] < min_samples:
            raise ValueError(f"{what}: clip {b} has {x.shape[-1]} samples, fewer than the {min_samples} it needs")
    n = [int(x.shape[-1]) for x in audio]
    dev = audio[0].device
    if len({tuple(x.shape[:-1]) for x in audio}) == 1:
        padded = torch.zeros(len(n), *audio[0].shape[:-1], max(n), dtype=audio[0].dtype, device=dev)
        for b, x in enumerate(audio):
            padded[b, ..., :n[b]] = x
    else:
        cd = torch.float64 if audio[0].dtype == torch.float64 else torch.float32
        padded = torch.zeros(len(n), max(n), dtype=cd, device=dev)
        for b, x in enumerate(audio):
            padded[b, :n[b]] = ops._rs_mono(x.unsqueeze(0) if x.dim() == 2 else x.reshape(1, 1, -1), cd)[0]
    lens = None
    if min(n) != max(n):
        lens = torch.tensor(n, dtype=torch.int32)
        if dev.type == "cuda":                                         # an asynchronous copy: the host does not wait for it
            lens = lens.pin_memory().to(dev, non_blocking=True)
    return padded, lens, n


class Resample(nn.Module):
    """waveform at orig_rate -> waveform at new_rate (ops.resample: the HIP polyphase kernel; its docstring states the filter),
    mono: the channels of a multi-channel clip are averaged, int16 samples are scaled by 2^-15.  No parameters, no buffers."""

    def __init__(self, orig_rate: int, new_rate: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        super().__init__()
        ops._rs_param_check(orig_rate, new_rate, lowpass_filter_width, rolloff, "Resample")
        self.orig_rate, self.new_rate, self.lowpass_filter_width, self.rolloff = orig_rate, new_rate, lowpass_filter_width, rolloff

    def out_samples(self, samples: int) -> int:
        """the length of a clip of `samples` samples after conversion: ceil(new samples / orig) over the reduced rates"""
        g = math.gcd(self.orig_rate, self.new_rate)
        return -(-(self.new_rate // g) * samples // (self.orig_rate // g))

    @torch.no_grad()
    def forward(self, audio):
        """audio: a (B, L) or (B, C, L) tensor -> (B, ceil(n L / o)) fp32; or a list of B clips, each (L_b,) or (C_b, L_b), of
        different lengths and channel counts -> a list of B (len_out_b,) tensors, views of one padded buffer."""
        kw = dict(lowpass_filter_width=self.lowpass_filter_width, rolloff=self.rolloff)
        if isinstance(audio, torch.Tensor):
            return ops.resample(audio, self.orig_rate, self.new_rate, **kw)[0]
        padded, lens, n = _pad_waveforms(audio, 1, "Resample")
        out = ops.resample(padded, self.orig_rate, self.new_rate, lens, **kw)[0]
        return [out[b, :self.out_samples(n[b])] for b in range(len(n))]


class ResampledLogMelFrontend(LogMelFrontend):
    """a LogMelFrontend for audio at input_sample_rate: ops.resample to sample_rate, then ops.log_mel with the lengths the resampler
    wrote, one device tensor between the two and no host sync.  Takes what `Resample` takes: float or int16 samples, mono or
    multi-channel.  WhisperMoP.transcribe_audio takes it as any LogMelFrontend."""

    def __init__(self, input_sample_rate: int, n_mels: int = 80, sample_rate: int = 16000, n_fft: int = 400, hop_length: int = 160,
                 lowpass_filter_width: int = 6, rolloff: float = 0.99):
        super().__init__(n_mels, sample_rate, n_fft, hop_length)
        ops._rs_param_check(input_sample_rate, sample_rate, lowpass_filter_width, rolloff, "ResampledLogMelFrontend")
        self.input_sample_rate = input_sample_rate
        self.resampler = Resample(input_sample_rate, sample_rate, lowpass_filter_width, rolloff)

    @property
    def min_samples(self) -> int:
        """the shortest clip in INPUT samples: the fewest that resample to LogMelFrontend.min_samples"""
        g = math.gcd(self.input_sample_rate, self.sample_rate)
        return (super().min_samples - 1) * (self.input_sample_rate // g) // (self.sample_rate // g) + 1

    @torch.no_grad()
    def forward(self, audio):
        """audio: a (B, L) or (B, C, L) tensor at input_sample_rate -> (B, ceil(n L / o) // hop_length, n_mels) fp32; or a list of B
        clips, each (L_b,) or (C_b, L_b) -> a list of B (T_b, n_mels) tensors, T_b = ceil(n L_b / o) // hop_length, views of one
        padded buffer."""
        what, rs = "ResampledLogMelFrontend", self.resampler
        kw = dict(lowpass_filter_width=rs.lowpass_filter_width, rolloff=rs.rolloff)
        if isinstance(audio, torch.Tensor):
            if audio.dim() not in (2, 3) or audio.shape[-1] < self.min_samples:
                raise ValueError(f"{what}: audio must be a (B, L) or (B, C, L) tensor with L >= {self.min_samples} or a non-empty list "
                                 f"of clips, got {tuple(audio.shape)}")
            return ops.log_mel(ops.resample(audio, rs.orig_rate, rs.new_rate, **kw)[0], self.filters, self.n_fft, self.hop_length)
        padded, lens, n = _pad_waveforms(audio, self.min_samples, what)
        wave, out_lens = ops.resample(padded, rs.orig_rate, rs.new_rate, lens, **kw)
        mel = ops.log_mel(wave, self.filters, self.n_fft, self.hop_length, out_lens)
        return [mel[b, :rs.out_samples(n[b]) // self.hop_length] for b in range(len(n))]


class RuledDecoding:
    """`WhisperMoP.with_logit_rules(rules)`: the model's three decoders with Whisper's logit rules (ops.LogitRules: the never-emit
    list, blank suppression at the first generated position, the timestamp grammar) applied to every step's last-position logits
    by ops.logit_rules, one HIP launch inside the step.  The decoders' own signatures do not change (their tests pin them); each
    method here takes the arguments of the method it names, and what came later as keywords of its own: the decoding statistics
    (return_stats, no_speech_token_id, sot_index) and, on transcribe, the temperature fallback, the no-speech skip, the
    conditioning on the previous text, the word timestamps and the language detection.  rules.eos_token_id, when set, must equal a call's eos_token_id when that is given too
    (ValueError).  logit_rules None runs the plain decoder: no extra launch, no extra buffer.
    repeat_rules (ops.RepeatRules; for Whisper build them with ops.RepeatRules.for_whisper(logit_rules, ...), which exempts eos
    and the timestamps): a repetition penalty and / or no-repeat n-gram blocking over each row's generated tokens, by
    ops.repeat_rules, one more HIP launch inside the step and BEFORE the logit rules, so everything said above about the filtered
    row (the timestamp grammar's rule 3e, return_logits, the log-probabilities) holds for the row after both filters, while
    no_speech_prob is still read before any filter.  transcribe applies them to every window and every fallback temperature.
    None or neutral rules: no extra launch, no extra buffer."""

    def __init__(self, model: WhisperMoP, logit_rules: Optional["ops.LogitRules"], repeat_rules: Optional["ops.RepeatRules"] = None):
        self.model, self.logit_rules, self.repeat_rules = model, logit_rules, repeat_rules
        model._rules_check(logit_rules, None, "with_logit_rules")
        model._repeat_check(repeat_rules, "with_logit_rules")

    @torch.no_grad()
    def generate(self, mel, prompt_ids, max_new_tokens: int, eos_token_id: Optional[int] = None, graph: bool = False, *,
                 return_logits: bool = False, return_stats: bool = False, no_speech_token_id: Optional[int] = None,
                 sot_index: int = 0):
        """WhisperMoP.generate under the rules: the filter runs before the argmax, over a (B, cap) int32 device history kept for
        it; return_logits returns the FILTERED logits, the ones that chose the token; return_stats adds up the log-softmax of the
        FILTERED rows (Whisper's convention), while no_speech_prob is read before the filter"""
        return self.model._generate(mel, prompt_ids, max_new_tokens, eos_token_id, graph, return_logits, self.logit_rules,
                                    return_stats, no_speech_token_id, sot_index, self.repeat_rules)

    @torch.no_grad()
    def beam_search(self, mel, prompt_ids, max_new_tokens: int, num_beams: int, eos_token_id: Optional[int] = None,
                    length_penalty: float = 1.0, graph: bool = False, *, return_stats: bool = False,
                    no_speech_token_id: Optional[int] = None, sot_index: int = 0):
        """WhisperMoP.beam_search under the rules: the filter runs before ops.beam_step, on the beams' own histories, so the
        candidates' log-probabilities are those of the filtered rows (no_speech_prob is read before the filter)"""
        return self.model._beam_search(mel, prompt_ids, max_new_tokens, num_beams, eos_token_id, length_penalty, graph,
                                       self.logit_rules, return_stats, no_speech_token_id, sot_index, self.repeat_rules)

    @torch.no_grad()
    def sample(self, mel, prompt_ids, max_new_tokens: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
               num_samples: int = 1, eos_token_id: Optional[int] = None, seed: int = 0, graph: bool = False, *,
               return_stats: bool = False, no_speech_token_id: Optional[int] = None, sot_index: int = 0):
        """WhisperMoP.sample under the rules: the filter runs before the draw; sum_logprobs adds the log-softmax of the FILTERED
        row (Whisper's convention: its filters precede the log-probabilities; no_speech_prob is read before the filter)"""
        return self.model._sample(mel, prompt_ids, max_new_tokens, temperature, top_k, top_p, num_samples, eos_token_id, seed,
                                  graph, self.logit_rules, return_stats, no_speech_token_id, sot_index, self.repeat_rules)

    @torch.no_grad()
    def transcribe(self, mel, prompt_ids: torch.Tensor, max_new_tokens: int, *, window: Optional[int] = None,
                   frames_per_timestamp: int = 1, num_beams: int = 1, length_penalty: float = 1.0, graph: bool = False,
                   temperatures=(0.0,), logprob_threshold: Optional[float] = None, no_speech_threshold: Optional[float] = None,
                   no_speech_token_id: Optional[int] = None, sot_index: int = 0, compression_ratio_threshold: Optional[float] = None,
                   compression_ratio=None, num_samples: int = 1, seed: int = 0, return_log: bool = False,
                   word_timestamps: bool = False, word_rules=None, alignment_heads=None, medfilt_width: int = 7,
                   median_word_frames: Optional[int] = None, languages=None, language_index: int = 1,
                   condition_on_previous_text: bool = False, initial_prompt=None, sot_prev_token_id: Optional[int] = None,
                   max_prompt_tokens: Optional[int] = None, prompt_reset_temperature: float = 0.5):
        return self.model._transcribe(
            mel, prompt_ids, self.logit_rules, max_new_tokens, window=window, frames_per_timestamp=frames_per_timestamp,
            num_beams=num_beams, length_penalty=length_penalty, graph=graph, temperatures=temperatures,
            logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold, no_speech_token_id=no_speech_token_id,
            sot_index=sot_index, compression_ratio_threshold=compression_ratio_threshold, compression_ratio=compression_ratio,
            num_samples=num_samples, seed=seed, return_log=return_log, condition_on_previous_text=condition_on_previous_text,
            initial_prompt=initial_prompt, sot_prev_token_id=sot_prev_token_id, max_prompt_tokens=max_prompt_tokens,
            prompt_reset_temperature=prompt_reset_temperature, word_timestamps=word_timestamps, word_rules=word_rules,
            alignment_heads=alignment_heads, medfilt_width=medfilt_width, median_word_frames=median_word_frames,
            languages=languages, language_index=language_index, repeat_rules=self.repeat_rules)


RuledDecoding.transcribe.__doc__ = WhisperMoP._transcribe.__doc__


def create_whisper_mop(cfg: WhisperConfig) -> WhisperMoP:
    return WhisperMoP(cfg)


def create_whisper_baseline(cfg: WhisperConfig) -> WhisperMoP:
    """the same architecture with every encoder gate's alpha at 0: gate = 1 (reference :431-437)."""
    model = WhisperMoP(cfg)
    with torch.no_grad():
        for blk in model.encoder:
            blk.mop.fuse.alpha.zero_()
    return model
