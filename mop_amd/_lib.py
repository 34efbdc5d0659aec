"""ctypes binding of libmopk.so (include/mopk.h).  No torch types cross this boundary."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOPK_LIB") or os.path.join(HERE, "libmopk.so")   # MOPK_LIB: dev builds (tools/build_variant.py)

MOPK_F32, MOPK_BF16 = 0, 1
PREC_FP32, PREC_BF16 = 0, 1
PATH_AUTO, PATH_GENERIC, PATH_FUSED = 0, 1, 2


class View4(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("sb", C.c_int64), ("sh", C.c_int64), ("sn", C.c_int64)]


class View5(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("sv", C.c_int64), ("sb", C.c_int64), ("sh", C.c_int64),
                ("sn", C.c_int64)]


_fp = C.c_void_p  # device pointers travel as void*


MAX_LENS = 4          # MOPK_MAX_LENS
DENSE_HIDDEN = 16     # MOPK_DENSE_HIDDEN


class EdgewiseExt(C.Structure):
    """MopkEdgewiseExt: dense gate head / S lens bank (generic path)."""
    _fields_ = [
        ("gate_mode", C.c_int32), ("use_k3", C.c_int32), ("n_lens", C.c_int32), ("lens_dil", C.c_int32 * MAX_LENS),
        ("lens_w", _fp), ("W1", _fp), ("b1", _fp), ("W3", _fp), ("b3", _fp), ("W2", _fp), ("b2", _fp),
        ("dlens_w", _fp), ("dW1", _fp), ("db1", _fp), ("dW3", _fp), ("db3", _fp), ("dW2", _fp), ("db2", _fp),
        ("n_extra", C.c_int32), ("row_extra", _fp), ("col_extra", _fp), ("d_row_extra", _fp), ("d_col_extra", _fp),
    ]


class EdgewiseArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("dk", C.c_int32),
        ("V", C.c_int32), ("r", C.c_int32), ("io_dtype", C.c_int32), ("precision", C.c_int32),
        ("path", C.c_int32), ("save_for_backward", C.c_int32), ("beta_not", C.c_float),
        ("q", View5), ("k", View5), ("v0", View4), ("vL", View4),
        ("sqk", _fp), ("vs0", _fp), ("vsL", _fp), ("Wr", _fp), ("br", _fp), ("Wc", _fp), ("bc", _fp),
        ("chain_logit", _fp),
        ("y", View4), ("saved", _fp), ("workspace", _fp),
        ("dy", View4), ("dq", View5), ("dk_", View5), ("dv0", View4), ("dvL", View4),
        ("dsqk_part", _fp), ("dvs0_part", _fp), ("dvsL_part", _fp),
        ("dWr", _fp), ("dbr", _fp), ("dWc", _fp), ("dbc", _fp), ("dlogit_part", _fp),
        ("ext", C.POINTER(EdgewiseExt)),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
        ("mask", _fp), ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_si", C.c_int64),
    ]


class EdgewiseParamArgs(C.Structure):
    """MopkEdgewiseParamArgs: the small parameters of a share_qkv EdgewiseMSA layer on their way to the core and their gradients back."""
    _fields_ = [
        ("B", C.c_int32), ("V", C.c_int32), ("H", C.c_int32), ("dk", C.c_int32), ("r", C.c_int32), ("C", C.c_int32),
        ("io_dtype", C.c_int32),
        ("q_scale", _fp), ("k_scale", _fp), ("v_scale", _fp), ("Wr", _fp), ("br", _fp), ("Wc", _fp), ("bc", _fp),
        ("chain_logit", _fp), ("pack", _fp),
        ("dsqk_part", _fp), ("dvs0_part", _fp), ("dvsL_part", _fp), ("dlogit_part", _fp),
        ("dWr", _fp), ("dbr", _fp), ("dWc", _fp), ("dbc", _fp),
        ("gq_scale", _fp), ("gk_scale", _fp), ("gv_scale", _fp), ("gWr", _fp), ("gbr", _fp), ("gWc", _fp), ("gbc", _fp),
        ("glogit", _fp),
    ]


class DualPathArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("dk", C.c_int32), ("hops", C.c_int32),
        ("io_dtype", C.c_int32), ("precision", C.c_int32), ("path", C.c_int32), ("causal", C.c_int32),
        ("g_and", C.c_float), ("g_or", C.c_float), ("g_not", C.c_float), ("g_chain", C.c_float),
        ("beta_not", C.c_float),
        ("q1", View4), ("k1", View4), ("v1", View4), ("q2", View4), ("k2", View4), ("v2", View4),
        ("mask", _fp), ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_si", C.c_int64),
        ("chain_logit", _fp), ("y", View4), ("saved", _fp), ("workspace", _fp),
        ("dy", View4), ("dq1", View4), ("dk1", View4), ("dv1", View4), ("dq2", View4), ("dk2", View4),
        ("dv2", View4), ("dlogit_part", _fp),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
    ]


class QuartetArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("T", C.c_int32), ("dh", C.c_int32),
        ("io_dtype", C.c_int32), ("precision", C.c_int32), ("path", C.c_int32),
        ("use_quartet", C.c_int32), ("eps", C.c_float),
        ("q", View4), ("k", View4), ("v", View4), ("q2", View4), ("k2", View4),
        ("mixture", _fp), ("quartet_scale", _fp),
        ("add_mask", _fp), ("am_sb", C.c_int64), ("am_sh", C.c_int64), ("am_si", C.c_int64),
        ("y", View4), ("attn", _fp), ("saved", _fp), ("workspace", _fp),
        ("dy", View4), ("dq", View4), ("dk_", View4), ("dv", View4), ("dq2", View4), ("dk2", View4),
        ("dmixture_part", _fp), ("dqscale_part", _fp),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
    ]


class SdpaArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("dk", C.c_int32),
        ("io_dtype", C.c_int32), ("precision", C.c_int32), ("path", C.c_int32), ("causal", C.c_int32),
        ("q", View4), ("k", View4), ("v", View4),
        ("mask", _fp), ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_si", C.c_int64),
        ("bias", _fp), ("bias_sb", C.c_int64), ("bias_sh", C.c_int64), ("bias_si", C.c_int64),
        ("y", View4), ("saved", _fp), ("workspace", _fp),
        ("dy", View4), ("dq", View4), ("dk_", View4), ("dv", View4),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
        ("Nk", C.c_int32),                     # key / value length, 0 = N
    ]


class QuartetLensArgs(C.Structure):
    """MopkQuartetLensArgs: the Quartet core over right-padded rows, row b has lens[b] real tokens (NULL = full rows)."""
    _fields_ = [("base", QuartetArgs), ("lens", _fp)]


class SdpaLensArgs(C.Structure):
    """MopkSdpaLensArgs: plain SDPA over right-padded rows, query rows i >= q_lens[b] padding, keys j >= kv_lens[b] blocked."""
    _fields_ = [("base", SdpaArgs), ("q_lens", _fp), ("kv_lens", _fp)]


class CrossViewArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("dk", C.c_int32),
        ("io_dtype", C.c_int32), ("precision", C.c_int32), ("path", C.c_int32), ("causal", C.c_int32),
        ("use_prior", C.c_int32), ("anchor_mode", C.c_int32), ("fixed_k_star", C.c_int32),
        ("t1", C.c_float), ("t2", C.c_float), ("prior_weight", C.c_float),
        ("q1", View4), ("k1", View4), ("v1", View4), ("q2", View4), ("k2", View4),
        ("mix", _fp), ("mask", _fp), ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_si", C.c_int64),
        ("y", View4), ("saved", _fp), ("workspace", _fp), ("k_star", _fp),
        ("dy", View4), ("dq1", View4), ("dk1", View4), ("dv1", View4), ("dq2", View4), ("dk2", View4),
        ("dmix_part", _fp), ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64),
    ]


class LayerNormArgs(C.Structure):
    _fields_ = [
        ("rows", C.c_int64), ("dim", C.c_int32), ("x_dtype", C.c_int32), ("y_dtype", C.c_int32), ("p_dtype", C.c_int32),
        ("eps", C.c_float), ("x_ld", C.c_int64), ("y_ld", C.c_int64),
        ("x", _fp), ("gamma", _fp), ("beta", _fp), ("y", _fp), ("mean", _fp), ("rstd", _fp),
        ("dy", _fp), ("dres", _fp), ("dx", _fp), ("dgamma", _fp), ("dbeta", _fp), ("workspace", _fp),
    ]


class LensMeansArgs(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("dk", C.c_int32), ("V", C.c_int32), ("L", C.c_int32),
        ("io_dtype", C.c_int32), ("dil", C.c_int32 * MAX_LENS),
        ("q", View4), ("k", View4), ("sqk", _fp), ("lens_w", _fp), ("row", _fp), ("col", _fp), ("d_row", _fp), ("d_col", _fp),
        ("dq", View4), ("dk_", View4), ("dsqk_part", _fp), ("dlens_part", _fp),
    ]


class TokenGateArgs(C.Structure):
    """MopkTokenGateArgs: 1-D MoP token gate (GPT-MoP block)."""
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("x_dtype", C.c_int32), ("a_dtype", C.c_int32), ("o_dtype", C.c_int32),
        ("x", _fp), ("x_sb", C.c_int64), ("x_st", C.c_int64), ("a", _fp), ("a_sb", C.c_int64), ("a_st", C.c_int64),
        ("u", _fp), ("out", _fp), ("gate", _fp), ("dout", _fp), ("dr", _fp), ("du", _fp), ("workspace", _fp),
    ]


class TokenGateLensArgs(C.Structure):
    """MopkTokenGateLensArgs: the token gate over right-padded rows, row b has lens[b] real tokens (NULL = full rows)."""
    _fields_ = [("base", TokenGateArgs), ("lens", _fp)]


class MelGateArgs(C.Structure):
    """MopkMelGateArgs: the MoP mel gate of every WhisperMoP encoder layer, folded to taps (L,k,F)."""
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("F", C.c_int32), ("L", C.c_int32), ("k", C.c_int32), ("mel_dtype", C.c_int32),
        ("mel", _fp), ("mel_sb", C.c_int64), ("mel_st", C.c_int64), ("W", _fp), ("lens", _fp), ("gates", _fp), ("dgates", _fp),
        ("dW", _fp), ("workspace", _fp),
    ]


class GatedResidualArgs(C.Structure):
    """MopkGatedResidualArgs: (x + a) * gate[..., None] of the WhisperMoP encoder block."""
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("x_dtype", C.c_int32), ("a_dtype", C.c_int32), ("o_dtype", C.c_int32),
        ("x", _fp), ("x_sb", C.c_int64), ("x_st", C.c_int64), ("a", _fp), ("a_sb", C.c_int64), ("a_st", C.c_int64),
        ("gate", _fp), ("gate_sb", C.c_int64), ("out", _fp), ("dout", _fp), ("dr", _fp), ("dgate", _fp),
    ]


class CrossEntropyArgs(C.Structure):
    """MopkCrossEntropyArgs: cross-entropy of R rows of logits (rows row0 .. of a problem of n_rows) against int64 targets."""
    _fields_ = [
        ("R", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("row0", C.c_int32), ("n_rows", C.c_int32), ("reserved", C.c_int32),
        ("ignore_index", C.c_int64), ("logits", _fp), ("logits_ld", C.c_int64), ("targets", _fp), ("lse", _fp), ("row_loss", _fp),
        ("out", _fp), ("dlogits", _fp), ("dlogits_ld", C.c_int64), ("grad", _fp), ("grad_stride", C.c_int64), ("scale", _fp),
    ]


ADAMW_CHUNK = 4096          # MOPK_ADAMW_CHUNK: elements per chunk
ADAMW_MAX_TENSORS = 40      # MOPK_ADAMW_MAX_TENSORS: tensor parts per launch
ADAMW_MAX_CHUNKS = 4096     # MOPK_ADAMW_MAX_CHUNKS: chunks per launch
ADAMW_NORM, ADAMW_UPDATE = 1, 2


class OptimTensor(C.Structure):
    """MopkOptimTensor: one tensor of a fused optimiser step."""
    _fields_ = [
        ("p", _fp), ("g", _fp), ("m", _fp), ("v", _fp), ("ema", _fp), ("step", _fp), ("n", C.c_int64),
        ("p_dtype", C.c_int32), ("g_dtype", C.c_int32),
    ]


class AdamWStats(C.Structure):
    """MopkAdamWStats: the 16 device bytes a FusedAdamW keeps between steps."""
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("skip", C.c_int32), ("skipped", C.c_int32)]


class AdamWArgs(C.Structure):
    """MopkAdamWArgs: the phases and hyper-parameters of one mopk_adamw_step call."""
    _fields_ = [
        ("n_tensors", C.c_int32), ("phases", C.c_int32), ("clip", C.c_int32), ("skip_nonfinite", C.c_int32), ("use_norm", C.c_int32),
        ("use_ema", C.c_int32),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
        ("ema_decay", C.c_double), ("max_norm", C.c_double),
        ("lr_dev", _fp), ("stats", _fp), ("workspace", _fp),
    ]


MOE_MAX_EXPERTS = 64


class MoeArgs(C.Structure):
    """MopkMoeArgs: top-1 routed MoE MLP (ViT_MoP(use_moe=True))."""
    _fields_ = [
        ("M", C.c_int32), ("D", C.c_int32), ("F", C.c_int32), ("E", C.c_int32), ("precision", C.c_int32),
        ("x_dtype", C.c_int32), ("w_dtype", C.c_int32), ("gate_dtype", C.c_int32), ("o_dtype", C.c_int32), ("reserved", C.c_int32),
        ("x", _fp), ("gate_w", _fp), ("gate_b", _fp), ("w1", _fp * MOE_MAX_EXPERTS), ("w2", _fp * MOE_MAX_EXPERTS),
        ("residual", _fp), ("y", _fp), ("u", _fp), ("h", _fp), ("route", _fp), ("dy", _fp), ("dx", _fp),
        ("dw1", _fp * MOE_MAX_EXPERTS), ("dw2", _fp * MOE_MAX_EXPERTS), ("workspace", _fp),
    ]


class DecodeAttnArgs(C.Structure):
    """MopkDecodeAttnArgs: a few new queries against a key / value cache (WhisperMoP incremental decoding)."""
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("Tq", C.c_int32), ("dk", C.c_int32), ("cap", C.c_int32), ("Nk", C.c_int32),
        ("io_dtype", C.c_int32), ("causal", C.c_int32),
        ("q", View4), ("k", View4), ("v", View4), ("y", View4), ("kv_len", _fp), ("workspace", _fp),
    ]


class DecodeAttnRowsArgs(C.Structure):
    """MopkDecodeAttnRowsArgs: decode attention whose keys / values are read through a (B, cap) source-row table (beam search)."""
    _fields_ = [("base", DecodeAttnArgs), ("rows", _fp), ("rows_ld", C.c_int64)]


class DecodeAttnRaggedArgs(C.Structure):
    """MopkDecodeAttnRaggedArgs: decode attention in which query row b sees only the keys j >= kv_start[b] (left-padded prompts of
    different lengths), optionally through a row table."""
    _fields_ = [("base", DecodeAttnArgs), ("rows", _fp), ("rows_ld", C.c_int64), ("kv_start", _fp)]


class DecodeAttnLensArgs(C.Structure):
    """MopkDecodeAttnLensArgs: decode attention in which row b of q sees the keys j < kv_lens[b] (cross-attention over right-padded
    audio of unequal length)."""
    _fields_ = [("base", DecodeAttnArgs), ("kv_lens", _fp)]


class BeamArgs(C.Structure):
    """MopkBeamArgs: one step of batched beam search over device state (WhisperMoP.beam_search)."""
    _fields_ = [
        ("B", C.c_int32), ("K", C.c_int32), ("V", C.c_int32), ("T", C.c_int32), ("logits_dtype", C.c_int32), ("eos", C.c_int32),
        ("prompt_len", C.c_int32), ("length_penalty", C.c_float),
        ("logits", _fp), ("logits_sb", C.c_int64), ("logits_sk", C.c_int64), ("pos", _fp),
        ("scores", _fp), ("next_ids", _fp), ("parents", _fp), ("hist", _fp), ("hist_ld", C.c_int64), ("rows", _fp),
        ("rows_ld", C.c_int64), ("fin_tokens", _fp), ("fin_scores", _fp), ("fin_count", _fp), ("done", _fp), ("workspace", _fp),
    ]


class SampleArgs(C.Structure):
    """MopkSampleArgs: temperature / top-k / top-p sampling of one token per row (WhisperMoP.sample)."""
    _fields_ = [
        ("R", C.c_int32), ("n", C.c_int32), ("V", C.c_int32), ("logits_dtype", C.c_int32), ("top_k", C.c_int32), ("greedy", C.c_int32),
        ("inv_temp", C.c_float), ("top_p", C.c_float), ("seed", C.c_uint64),
        ("logits", _fp), ("logits_sb", C.c_int64), ("logits_sk", C.c_int64), ("pos", _fp), ("tokens", _fp), ("logprobs", _fp),
        ("workspace", _fp),
    ]


class SampleRaggedArgs(C.Structure):
    """MopkSampleRaggedArgs: sampling in which row r draws at position *pos - pos_off[r] (a left-padded ragged batch)."""
    _fields_ = [("base", SampleArgs), ("pos_off", _fp)]


class LogitRulesArgs(C.Structure):
    """MopkLogitRulesArgs: Whisper's suppression and timestamp rules on last-position logits (WhisperMoP's logit_rules)."""
    _fields_ = [
        ("R", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("T", C.c_int32), ("T0", C.c_int32), ("tb", C.c_int32),
        ("eos", C.c_int32), ("max_initial", C.c_int32),
        ("logits", _fp), ("logits_ld", C.c_int64), ("out", _fp), ("out_ld", C.c_int64), ("hist", _fp), ("hist_ld", C.c_int64),
        ("pos", _fp), ("mask", _fp),
    ]


class RepeatRulesArgs(C.Structure):
    """MopkRepeatRulesArgs: repetition penalty and no-repeat n-gram blocking on last-position logits (WhisperMoP's repeat_rules)."""
    _fields_ = [
        ("R", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("T", C.c_int32), ("T0", C.c_int32), ("ngram", C.c_int32),
        ("penalty", C.c_float), ("inv_penalty", C.c_float),
        ("logits", _fp), ("logits_ld", C.c_int64), ("out", _fp), ("out_ld", C.c_int64), ("hist", _fp), ("hist_ld", C.c_int64),
        ("pos", _fp), ("exempt", _fp),
    ]


class AlignCostArgs(C.Structure):
    """MopkAlignCostArgs: Whisper's alignment filter (z-normalise, median-filter, average the heads) on cross-attention maps."""
    _fields_ = [
        ("B", C.c_int32), ("S", C.c_int32), ("N", C.c_int32), ("M", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
        ("probs", _fp), ("probs_sb", C.c_int64), ("probs_ss", C.c_int64), ("probs_sn", C.c_int64),
        ("n_tokens", _fp), ("n_frames", _fp), ("cost", _fp), ("cost_sb", C.c_int64), ("cost_ld", C.c_int64),
    ]


class DtwArgs(C.Structure):
    """MopkDtwArgs: Whisper's dynamic time warping over per-item windows of a cost matrix, walked back on the device."""
    _fields_ = [
        ("B", C.c_int32), ("N", C.c_int32), ("M", C.c_int32), ("row0", C.c_int32),
        ("cost", _fp), ("cost_sb", C.c_int64), ("cost_ld", C.c_int64), ("n_rows", _fp), ("n_cols", _fp),
        ("starts", _fp), ("ends", _fp), ("workspace", _fp),
    ]


class TimestampSegmentsArgs(C.Structure):
    """MopkTimestampSegmentsArgs: Whisper's segment and seek arithmetic on decoded token rows (WhisperMoP.transcribe)."""
    _fields_ = [
        ("R", C.c_int32), ("T", C.c_int32), ("T0", C.c_int32), ("tb", C.c_int32), ("eos", C.c_int32), ("f", C.c_int32),
        ("tokens", _fp), ("tokens_ld", C.c_int64), ("window", _fp), ("starts", _fp), ("ends", _fp),
        ("tok_begin", _fp), ("tok_end", _fp), ("n_segments", _fp), ("advance", _fp),
    ]


class PromptHistoryArgs(C.Structure):
    """MopkPromptHistoryArgs: the in-place update of the per-clip token history (WhisperMoP.transcribe's conditioning)."""
    _fields_ = [
        ("A", C.c_int32), ("B", C.c_int32), ("n", C.c_int32), ("T", C.c_int32), ("T0", C.c_int32), ("reserved", C.c_int32),
        ("hist", _fp), ("hist_len", _fp), ("tokens", _fp), ("tokens_ld", C.c_int64), ("n_take", _fp), ("item", _fp), ("mode", _fp),
    ]


class WindowPromptsArgs(C.Structure):
    """MopkWindowPromptsArgs: the left-padded prompt matrix of a set of windows, built from the token history."""
    _fields_ = [
        ("A", C.c_int32), ("B", C.c_int32), ("n", C.c_int32), ("width", C.c_int32), ("Ts", C.c_int32), ("prev", C.c_int32),
        ("out_i64", C.c_int32), ("sot_i64", C.c_int32),
        ("hist", _fp), ("hist_len", _fp), ("item", _fp), ("sot", _fp), ("sot_ld", C.c_int64), ("ids", _fp), ("kv_start", _fp),
    ]


class AlignmentRowsArgs(C.Structure):
    """MopkAlignmentRowsArgs: decoded window rows turned into the padded ids of the alignment pass (transcribe's word timestamps)."""
    _fields_ = [
        ("R", C.c_int32), ("T", C.c_int32), ("T0", C.c_int32), ("Tp", C.c_int32), ("nots", C.c_int32), ("eos", C.c_int32),
        ("out_i64", C.c_int32), ("sot_i64", C.c_int32),
        ("tokens", _fp), ("tokens_ld", C.c_int64), ("n_take", _fp), ("sot", _fp), ("sot_ld", C.c_int64), ("ids", _fp),
        ("n_tokens", _fp), ("col", _fp),
    ]


class WordSpansArgs(C.Structure):
    """MopkWordSpansArgs: aligned text tokens grouped into timed words (Whisper's add_word_timestamps)."""
    _fields_ = [
        ("R", C.c_int32), ("N", C.c_int32), ("V", C.c_int32), ("median_cap", C.c_int32),
        ("tokens", _fp), ("tokens_ld", C.c_int64), ("times", _fp), ("times_ld", C.c_int64), ("probs", _fp), ("probs_ld", C.c_int64),
        ("n_text", _fp), ("table", _fp), ("starts", _fp), ("ends", _fp), ("out_probs", _fp), ("tok_begin", _fp), ("tok_end", _fp),
        ("n_words", _fp),
    ]


class LogMelArgs(C.Structure):
    """MopkLogMelArgs: Whisper's log-mel spectrogram of a batch of waveforms (LogMelFrontend)."""
    _fields_ = [
        ("B", C.c_int32), ("L", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32),
        ("audio_dtype", C.c_int32), ("out_dtype", C.c_int32), ("reserved", C.c_int32),
        ("audio", _fp), ("audio_ld", C.c_int64), ("lens", _fp), ("filters", _fp), ("bands", _fp), ("twiddle", _fp),
        ("window", _fp), ("out", _fp), ("workspace", _fp),
    ]


class ResampleArgs(C.Structure):
    """MopkResampleArgs: polyphase sample-rate conversion of a batch of waveforms (ops.resample)."""
    _fields_ = [
        ("B", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("Lout", C.c_int32), ("o", C.c_int32), ("n", C.c_int32),
        ("w", C.c_int32), ("S", C.c_int32), ("table_ld", C.c_int32), ("audio_dtype", C.c_int32), ("out_dtype", C.c_int32),
        ("reserved", C.c_int32),
        ("audio", _fp), ("audio_sb", C.c_int64), ("audio_sc", C.c_int64), ("audio_sl", C.c_int64), ("lens", _fp), ("table", _fp),
        ("first", _fp), ("out", _fp), ("out_lens", _fp),
    ]


class TokenLogprobArgs(C.Structure):
    """MopkTokenLogprobArgs: the log-probability of one token per row of last-position logits (WhisperMoP's no_speech_prob)."""
    _fields_ = [
        ("R", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("token", C.c_int32),
        ("logits", _fp), ("logits_ld", C.c_int64), ("tokens", _fp), ("out", _fp),
    ]


class GreedyPickArgs(C.Structure):
    """MopkGreedyPickArgs: one greedy decoding step on device state (WhisperMoP.generate)."""
    _fields_ = [
        ("R", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("eos", C.c_int32), ("hist_cap", C.c_int32), ("reserved", C.c_int32),
        ("logits", _fp), ("logits_ld", C.c_int64), ("pos", _fp), ("next_ids", _fp), ("done", _fp), ("sum_logprobs", _fp),
        ("n_tokens", _fp), ("hist", _fp), ("hist_ld", C.c_int64),
    ]


class LanguageProbsArgs(C.Structure):
    """MopkLanguageProbsArgs: the softmax over the language tokens' logits and its argmax (WhisperMoP.detect_language)."""
    _fields_ = [
        ("R", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("n", C.c_int32),
        ("logits", _fp), ("logits_ld", C.c_int64), ("ids", _fp), ("probs", _fp), ("probs_ld", C.c_int64), ("tokens", _fp),
    ]


LANGUAGE_MAX_N = 1024      # MOPK_LANGUAGE_MAX_N
LOG_MEL_TILE_FRAMES = 32   # MOPK_LOG_MEL_TILE_FRAMES
LOG_MEL_F16 = 2            # MOPK_LOG_MEL_F16


# every symbol include/mopk.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mopk_version": (C.c_int, []),
    "mopk_strerror": (C.c_char_p, [C.c_int]),
    "mopk_edgewise_fused_supported": (C.c_int, [C.POINTER(EdgewiseArgs)]),
    "mopk_edgewise_dominant_kernel": (C.c_char_p, [C.POINTER(EdgewiseArgs), C.c_int]),
    "mopk_edgewise_saved_bytes": (C.c_size_t, [C.POINTER(EdgewiseArgs)]),
    "mopk_edgewise_workspace_bytes": (C.c_size_t, [C.POINTER(EdgewiseArgs)]),
    "mopk_edgewise_lowrank_fwd": (C.c_int, [C.POINTER(EdgewiseArgs), C.c_void_p]),
    "mopk_edgewise_lowrank_bwd": (C.c_int, [C.POINTER(EdgewiseArgs), C.c_void_p]),
    "mopk_edgewise_reduce_parts": (C.c_int, [C.POINTER(EdgewiseArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mopk_edgewise_params_fwd": (C.c_int, [C.POINTER(EdgewiseParamArgs), C.c_void_p]),
    "mopk_edgewise_params_bwd": (C.c_int, [C.POINTER(EdgewiseParamArgs), C.c_void_p]),
    "mopk_edgewise_fwd": (C.c_int, [C.POINTER(EdgewiseArgs), C.c_void_p]),
    "mopk_edgewise_bwd": (C.c_int, [C.POINTER(EdgewiseArgs), C.c_void_p]),
    "mopk_dualpath_saved_bytes": (C.c_size_t, [C.POINTER(DualPathArgs)]),
    "mopk_dualpath_workspace_bytes": (C.c_size_t, [C.POINTER(DualPathArgs)]),
    "mopk_dualpath_fused_supported": (C.c_int, [C.POINTER(DualPathArgs)]),
    "mopk_dualpath_fwd": (C.c_int, [C.POINTER(DualPathArgs), C.c_void_p]),
    "mopk_dualpath_bwd": (C.c_int, [C.POINTER(DualPathArgs), C.c_void_p]),
    "mopk_quartet_saved_bytes": (C.c_size_t, [C.POINTER(QuartetArgs)]),
    "mopk_quartet_workspace_bytes": (C.c_size_t, [C.POINTER(QuartetArgs)]),
    "mopk_quartet_fused_supported": (C.c_int, [C.POINTER(QuartetArgs)]),
    "mopk_quartet_fwd": (C.c_int, [C.POINTER(QuartetArgs), C.c_void_p]),
    "mopk_quartet_bwd": (C.c_int, [C.POINTER(QuartetArgs), C.c_void_p]),
    "mopk_quartet_lens_saved_bytes": (C.c_size_t, [C.POINTER(QuartetLensArgs)]),
    "mopk_quartet_lens_workspace_bytes": (C.c_size_t, [C.POINTER(QuartetLensArgs)]),
    "mopk_quartet_lens_fused_supported": (C.c_int, [C.POINTER(QuartetLensArgs)]),
    "mopk_quartet_lens_fwd": (C.c_int, [C.POINTER(QuartetLensArgs), C.c_void_p]),
    "mopk_quartet_lens_bwd": (C.c_int, [C.POINTER(QuartetLensArgs), C.c_void_p]),
    "mopk_crossview_saved_bytes": (C.c_size_t, [C.POINTER(CrossViewArgs)]),
    "mopk_crossview_workspace_bytes": (C.c_size_t, [C.POINTER(CrossViewArgs)]),
    "mopk_crossview_fwd": (C.c_int, [C.POINTER(CrossViewArgs), C.c_void_p]),
    "mopk_crossview_bwd": (C.c_int, [C.POINTER(CrossViewArgs), C.c_void_p]),
    "mopk_sdpa_saved_bytes": (C.c_size_t, [C.POINTER(SdpaArgs)]),
    "mopk_sdpa_workspace_bytes": (C.c_size_t, [C.POINTER(SdpaArgs)]),
    "mopk_sdpa_fused_supported": (C.c_int, [C.POINTER(SdpaArgs)]),
    "mopk_sdpa_fwd": (C.c_int, [C.POINTER(SdpaArgs), C.c_void_p]),
    "mopk_sdpa_bwd": (C.c_int, [C.POINTER(SdpaArgs), C.c_void_p]),
    "mopk_dropout_keep": (C.c_int, [C.c_uint64, C.c_float, C.c_int64, C.c_int64, C.c_int64]),
    "mopk_layernorm_workspace_bytes": (C.c_size_t, [C.POINTER(LayerNormArgs)]),
    "mopk_layernorm_fwd": (C.c_int, [C.POINTER(LayerNormArgs), C.c_void_p]),
    "mopk_lens_means_supported": (C.c_int, [C.POINTER(LensMeansArgs), C.c_int]),
    "mopk_lens_means_fwd": (C.c_int, [C.POINTER(LensMeansArgs), C.c_void_p]),
    "mopk_lens_means_bwd": (C.c_int, [C.POINTER(LensMeansArgs), C.c_void_p]),
    "mopk_layernorm_bwd": (C.c_int, [C.POINTER(LayerNormArgs), C.c_void_p]),
    "mopk_token_gate_supported": (C.c_int, [C.POINTER(TokenGateArgs)]),
    "mopk_token_gate_workspace_bytes": (C.c_size_t, [C.POINTER(TokenGateArgs)]),
    "mopk_token_gate_fwd": (C.c_int, [C.POINTER(TokenGateArgs), C.c_void_p]),
    "mopk_token_gate_bwd": (C.c_int, [C.POINTER(TokenGateArgs), C.c_void_p]),
    "mopk_token_gate_lens_supported": (C.c_int, [C.POINTER(TokenGateLensArgs)]),
    "mopk_token_gate_lens_workspace_bytes": (C.c_size_t, [C.POINTER(TokenGateLensArgs)]),
    "mopk_token_gate_lens_fwd": (C.c_int, [C.POINTER(TokenGateLensArgs), C.c_void_p]),
    "mopk_token_gate_lens_bwd": (C.c_int, [C.POINTER(TokenGateLensArgs), C.c_void_p]),
    "mopk_moe_supported": (C.c_int, [C.POINTER(MoeArgs)]),
    "mopk_moe_workspace_bytes": (C.c_size_t, [C.POINTER(MoeArgs), C.c_int]),
    "mopk_moe_route": (C.c_int, [C.POINTER(MoeArgs), C.c_void_p]),
    "mopk_moe_fwd": (C.c_int, [C.POINTER(MoeArgs), C.c_void_p]),
    "mopk_moe_bwd": (C.c_int, [C.POINTER(MoeArgs), C.c_void_p]),
    "mopk_decode_attn_supported": (C.c_int, [C.POINTER(DecodeAttnArgs)]),
    "mopk_decode_attn_workspace_bytes": (C.c_size_t, [C.POINTER(DecodeAttnArgs)]),
    "mopk_decode_attn_fwd": (C.c_int, [C.POINTER(DecodeAttnArgs), C.c_void_p]),
    "mopk_decode_attn_rows_supported": (C.c_int, [C.POINTER(DecodeAttnRowsArgs)]),
    "mopk_decode_attn_rows_workspace_bytes": (C.c_size_t, [C.POINTER(DecodeAttnRowsArgs)]),
    "mopk_decode_attn_rows_fwd": (C.c_int, [C.POINTER(DecodeAttnRowsArgs), C.c_void_p]),
    "mopk_beam_supported": (C.c_int, [C.POINTER(BeamArgs)]),
    "mopk_beam_workspace_bytes": (C.c_size_t, [C.POINTER(BeamArgs)]),
    "mopk_beam_step": (C.c_int, [C.POINTER(BeamArgs), C.c_void_p]),
    "mopk_sample_supported": (C.c_int, [C.POINTER(SampleArgs)]),
    "mopk_sample_workspace_bytes": (C.c_size_t, [C.POINTER(SampleArgs)]),
    "mopk_sample_step": (C.c_int, [C.POINTER(SampleArgs), C.c_void_p]),
    "mopk_decode_attn_ragged_supported": (C.c_int, [C.POINTER(DecodeAttnRaggedArgs)]),
    "mopk_decode_attn_ragged_workspace_bytes": (C.c_size_t, [C.POINTER(DecodeAttnRaggedArgs)]),
    "mopk_decode_attn_ragged_fwd": (C.c_int, [C.POINTER(DecodeAttnRaggedArgs), C.c_void_p]),
    "mopk_sample_ragged_supported": (C.c_int, [C.POINTER(SampleRaggedArgs)]),
    "mopk_sample_ragged_workspace_bytes": (C.c_size_t, [C.POINTER(SampleRaggedArgs)]),
    "mopk_sample_ragged_step": (C.c_int, [C.POINTER(SampleRaggedArgs), C.c_void_p]),
    "mopk_sdpa_lens_supported": (C.c_int, [C.POINTER(SdpaLensArgs)]),
    "mopk_sdpa_lens_saved_bytes": (C.c_size_t, [C.POINTER(SdpaLensArgs)]),
    "mopk_sdpa_lens_workspace_bytes": (C.c_size_t, [C.POINTER(SdpaLensArgs)]),
    "mopk_sdpa_lens_fwd": (C.c_int, [C.POINTER(SdpaLensArgs), C.c_void_p]),
    "mopk_sdpa_lens_bwd": (C.c_int, [C.POINTER(SdpaLensArgs), C.c_void_p]),
    "mopk_decode_attn_lens_supported": (C.c_int, [C.POINTER(DecodeAttnLensArgs)]),
    "mopk_decode_attn_lens_workspace_bytes": (C.c_size_t, [C.POINTER(DecodeAttnLensArgs)]),
    "mopk_decode_attn_lens_fwd": (C.c_int, [C.POINTER(DecodeAttnLensArgs), C.c_void_p]),
    "mopk_logit_rules_supported": (C.c_int, [C.POINTER(LogitRulesArgs)]),
    "mopk_logit_rules": (C.c_int, [C.POINTER(LogitRulesArgs), C.c_void_p]),
    "mopk_repeat_rules_supported": (C.c_int, [C.POINTER(RepeatRulesArgs)]),
    "mopk_repeat_rules": (C.c_int, [C.POINTER(RepeatRulesArgs), C.c_void_p]),
    "mopk_alignment_cost_supported": (C.c_int, [C.POINTER(AlignCostArgs)]),
    "mopk_alignment_cost": (C.c_int, [C.POINTER(AlignCostArgs), C.c_void_p]),
    "mopk_dtw_align_supported": (C.c_int, [C.POINTER(DtwArgs)]),
    "mopk_dtw_workspace_bytes": (C.c_size_t, [C.POINTER(DtwArgs)]),
    "mopk_dtw_align": (C.c_int, [C.POINTER(DtwArgs), C.c_void_p]),
    "mopk_timestamp_segments_supported": (C.c_int, [C.POINTER(TimestampSegmentsArgs)]),
    "mopk_timestamp_segments": (C.c_int, [C.POINTER(TimestampSegmentsArgs), C.c_void_p]),
    "mopk_prompt_history_update_supported": (C.c_int, [C.POINTER(PromptHistoryArgs)]),
    "mopk_prompt_history_update": (C.c_int, [C.POINTER(PromptHistoryArgs), C.c_void_p]),
    "mopk_window_prompts_supported": (C.c_int, [C.POINTER(WindowPromptsArgs)]),
    "mopk_window_prompts": (C.c_int, [C.POINTER(WindowPromptsArgs), C.c_void_p]),
    "mopk_alignment_rows_supported": (C.c_int, [C.POINTER(AlignmentRowsArgs)]),
    "mopk_alignment_rows": (C.c_int, [C.POINTER(AlignmentRowsArgs), C.c_void_p]),
    "mopk_word_spans_supported": (C.c_int, [C.POINTER(WordSpansArgs)]),
    "mopk_word_spans": (C.c_int, [C.POINTER(WordSpansArgs), C.c_void_p]),
    "mopk_log_mel_supported": (C.c_int, [C.POINTER(LogMelArgs)]),
    "mopk_log_mel_workspace_bytes": (C.c_size_t, [C.POINTER(LogMelArgs)]),
    "mopk_log_mel": (C.c_int, [C.POINTER(LogMelArgs), C.c_void_p]),
    "mopk_resample_supported": (C.c_int, [C.POINTER(ResampleArgs)]),
    "mopk_resample": (C.c_int, [C.POINTER(ResampleArgs), C.c_void_p]),
    "mopk_token_logprob_supported": (C.c_int, [C.POINTER(TokenLogprobArgs)]),
    "mopk_token_logprob": (C.c_int, [C.POINTER(TokenLogprobArgs), C.c_void_p]),
    "mopk_greedy_pick_supported": (C.c_int, [C.POINTER(GreedyPickArgs)]),
    "mopk_greedy_pick": (C.c_int, [C.POINTER(GreedyPickArgs), C.c_void_p]),
    "mopk_language_probs_supported": (C.c_int, [C.POINTER(LanguageProbsArgs)]),
    "mopk_language_probs": (C.c_int, [C.POINTER(LanguageProbsArgs), C.c_void_p]),
    "mopk_mel_gate_supported": (C.c_int, [C.POINTER(MelGateArgs)]),
    "mopk_mel_gate_workspace_bytes": (C.c_size_t, [C.POINTER(MelGateArgs)]),
    "mopk_mel_gate_fwd": (C.c_int, [C.POINTER(MelGateArgs), C.c_void_p]),
    "mopk_mel_gate_bwd": (C.c_int, [C.POINTER(MelGateArgs), C.c_void_p]),
    "mopk_gated_residual_supported": (C.c_int, [C.POINTER(GatedResidualArgs)]),
    "mopk_gated_residual_workspace_bytes": (C.c_size_t, [C.POINTER(GatedResidualArgs)]),
    "mopk_gated_residual_fwd": (C.c_int, [C.POINTER(GatedResidualArgs), C.c_void_p]),
    "mopk_gated_residual_bwd": (C.c_int, [C.POINTER(GatedResidualArgs), C.c_void_p]),
    "mopk_cross_entropy_supported": (C.c_int, [C.POINTER(CrossEntropyArgs)]),
    "mopk_cross_entropy_fwd": (C.c_int, [C.POINTER(CrossEntropyArgs), C.c_void_p]),
    "mopk_cross_entropy_bwd": (C.c_int, [C.POINTER(CrossEntropyArgs), C.c_void_p]),
    "mopk_adamw_supported": (C.c_int, [C.POINTER(AdamWArgs), C.POINTER(OptimTensor)]),
    "mopk_adamw_workspace_bytes": (C.c_size_t, [C.POINTER(AdamWArgs), C.POINTER(OptimTensor)]),
    "mopk_adamw_launches": (C.c_int, [C.POINTER(AdamWArgs), C.POINTER(OptimTensor)]),
    "mopk_adamw_step": (C.c_int, [C.POINTER(AdamWArgs), C.POINTER(OptimTensor), C.c_void_p]),
}

_lib = None


def lib():
    """Load libmopk.so; fail loudly if the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m mop_amd.build` "
                "(mop_amd has no CPU or PyTorch fallback for the attention cores)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the ABI drifted
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib().mopk_strerror(rc).decode()} (status {rc})")
