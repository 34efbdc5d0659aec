/*
 * mopk.h -- C ABI of libmopk.so, the MI355X (gfx950) MoP-attention kernel library.
 *
 * The reference (Eran-BA/MoP) is pure PyTorch and has no FFI of its own; the
 * drop-in boundary is the nn.Module surface (mop_amd/nn mirrors it).  This
 * header is the boundary BELOW those modules: one entry point per reference
 * attention core, each citing the reference code it replaces.  Plain pointers,
 * sizes and element strides only; no torch types.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless stated; the caller owns every
 *    buffer (inputs, outputs, `saved`, `workspace`); the library never
 *    allocates or frees device memory and keeps no state between calls.
 *  - Kernels are enqueued on `stream` (a hipStream_t passed as void*); no call
 *    synchronises the host.  All entry points are graph-capturable.
 *  - Strides are in ELEMENTS of the tensor's dtype; the innermost (dk) dimension
 *    must be contiguous.
 *  - Return value: 0 = ok, negative = MopkStatus; mopk_strerror() names it.
 *  - `*_part` outputs are per-batch partial sums with leading dimension B; the
 *    caller reduces them over dim 0 (keeps the kernels free of global atomics
 *    and bit-reproducible).
 */
#ifndef MOPK_H
#define MOPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOPK_VERSION 118 /* 118: mopk_decode_attn_ragged_*, MopkDecodeAttnRaggedArgs, mopk_sample_ragged_* and MopkSampleRaggedArgs (added later without a bump: new exports only, detect with mopk_decode_attn_ragged_supported / mopk_sample_ragged_supported), mopk_sample_* and MopkSampleArgs (added later without a bump: new exports only, detect with mopk_sample_supported), mopk_decode_attn_rows_*, MopkDecodeAttnRowsArgs, mopk_beam_* and MopkBeamArgs (added later without a bump: new exports only, detect with mopk_decode_attn_rows_supported / mopk_beam_supported), mopk_decode_attn_* and MopkDecodeAttnArgs (added later without a bump: new exports only, detect with mopk_decode_attn_supported), mopk_moe_* and MopkMoeArgs (added later without a bump: new exports only, detect with mopk_moe_supported), MopkSdpaArgs.Nk appended (rectangular plain SDPA, 0 = N; added later without a bump, the number is pinned by the ABI tests: callers must be built against this header), mopk_token_gate_* (added later without a bump: new exports only, detect with mopk_token_gate_supported), attention dropout on every generic path, MopkCrossViewArgs.{dropout_p,dropout_seed}; 117: mopk_lens_means_{fwd,bwd}; 116: MopkEdgewiseExt.{n_extra,row_extra,col_extra,d_row_extra,d_col_extra}; 115: mask tensors on the fused dual-path kernels; 114: MopkEdgewiseArgs.mask (generic path), fused dense gate head; 113: attention dropout in the fused SDPA / Quartet kernels (dropout_p, dropout_seed, mopk_dropout_keep); 112: mopk_layernorm_*; 0.1.1: MopkEdgewiseArgs.{save_for_backward, ext}, MopkCrossViewArgs, *_fused_supported, y read by the sibling _bwd; 111: mopk_edgewise_reduce_parts */

typedef enum MopkStatus {
    MOPK_OK = 0,
    MOPK_ERR_BAD_SHAPE = -1,    /* non-positive or unsupported dimension */
    MOPK_ERR_BAD_ARG = -2,      /* null pointer / bad stride / bad enum */
    MOPK_ERR_UNSUPPORTED = -3,  /* variant not implemented by the requested path */
    MOPK_ERR_LAUNCH = -4,       /* hipGetLastError() != hipSuccess after a launch */
    MOPK_ERR_NO_DEVICE = -5     /* no gfx950 device visible */
} MopkStatus;

typedef enum MopkDtype { MOPK_F32 = 0, MOPK_BF16 = 1 } MopkDtype;

/* Arithmetic of the contractions.  FP32: exact fp32 FMA accumulation (parity
 * <= 1e-3 vs the reference CPU path, in practice ~1e-5).  BF16: bf16 MFMA
 * operands, fp32 accumulate, fp32 softmax/log/LSE/sigmoid (parity <= 1e-2). */
typedef enum MopkPrecision { MOPK_PREC_FP32 = 0, MOPK_PREC_BF16 = 1 } MopkPrecision;

/* Which implementation to run.  AUTO picks FUSED when the shape is supported
 * by the fused gfx950 kernels and GENERIC (multi-kernel, any shape) otherwise. */
typedef enum MopkPath { MOPK_PATH_AUTO = 0, MOPK_PATH_GENERIC = 1, MOPK_PATH_FUSED = 2 } MopkPath;

/* A (B,H,N,dk) tensor view: element (b,h,n,d) at ptr + b*sb + h*sh + n*sn + d. */
typedef struct MopkView4 {
    void *ptr;
    int64_t sb, sh, sn;
} MopkView4;

/* A per-view (V,B,H,N,dk) tensor view; sv == 0 means "one tensor shared by all views". */
typedef struct MopkView5 {
    void *ptr;
    int64_t sv, sb, sh, sn;
} MopkView5;

/* --------------------------------------------------------------------------
 * EdgewiseMSA attention core (low-rank gate head; dense head / lens banks through MopkEdgewiseExt).
 * Replaces reference mop/models/attention_variants.py:
 *   EdgewiseMSA.forward :500-562 (scores, per-view softmax, chain products,
 *   log features, gate head :319-331, score-space mix, re-normalise, value
 *   aggregation + transport) for attn_mask=None, no lens banks, dropout 0.
 * The qkv / proj Linear layers (:459, :564) stay outside (hipBLASLt GEMMs).
 *
 * Scale folding (verified identity):
 *   S_v = ((q * q_scale_v) (k * k_scale_v)^T) / sqrt(dk) = ((q * sqk_v) k^T),
 *   sqk_v = q_scale_v * k_scale_v / sqrt(dk).
 * For share_qkv=False pass per-view q/k (sv != 0) and sqk = 1/sqrt(dk).
 * -------------------------------------------------------------------------- */
/* Optional gate-head / feature variants (NULL ext = low-rank head, no lens bank).  The plain dense head (use_k3 = 0, n_lens = 0,
 * shared q/k, V <= 8 forward / V <= 6 backward, save_for_backward = 1) also runs on the fused kernels (MOPK_PATH_FUSED); the 3x3
 * convolution and the lens banks are generic-path only.
 *   dense head  : reference EdgewiseGateHead dense branch :250-272, :312-318 (Conv2d 1x1 C->16, GELU(tanh),
 *                 [use_k3: GELU again, Conv2d 3x3 16->16 pad 1], Conv2d 1x1 16->4, sigmoid)
 *   S lens bank : depthwise dilated 3x3 convolutions of the score planes appended to the feature stack :425-442, :523-533
 * Feature channel order (C = 2V + 2 + n_lens*V): S_0..S_{V-1}, S_0^T..S_{V-1}^T, Cr, Cl, lens[l*V+v]   :522-533
 * With the low-rank head and a lens bank, Wr/Wc (and dWr/dWc) are (4r, C) with this C. */
#define MOPK_MAX_LENS 4
#define MOPK_DENSE_HIDDEN 16
typedef struct MopkEdgewiseExt {
    int32_t gate_mode;          /* 0 = low-rank (row_proj/col_proj), 1 = dense                     :243 */
    int32_t use_k3;             /* dense only                                                       :253 */
    int32_t n_lens;             /* number of lens dilations L (0 = no lens bank), <= MOPK_MAX_LENS */
    int32_t lens_dil[MOPK_MAX_LENS]; /* dilation == padding of each 3x3 depthwise conv             :430-436 */
    const float *lens_w;        /* (L,V,3,3) = lens_bank.{l}.weight[:,0]                            */
    const float *W1, *b1;       /* edge_head.conv1 (16,C) / (16)                                    :251 */
    const float *W3, *b3;       /* edge_head.mid3 (16,16,3,3) / (16), use_k3 only                   :254 */
    const float *W2, *b2;       /* edge_head.conv2 (4,16) / (4)                                     :255 */
    /* backward outputs, fully reduced on device (any may be NULL when the matching input is unused) */
    float *dlens_w, *dW1, *db1, *dW3, *db3, *dW2, *db2;
    /* Extra feature channels of the LOW-RANK head on the FUSED path (gate_mode = 0, n_lens = 0): n_extra channels appended to the head's
     * input behind the 2V + 2 built-in ones, given directly as their row / column means -- row_extra, col_extra: (B,H,n_extra,N) fp32,
     * contiguous; Wr / Wc (dWr / dWc) are (4r, 2V + 2 + n_extra).  _bwd writes the gradient with respect to those values into
     * d_row_extra / d_col_extra (same shape).  This is how the S lens bank :425-442, :523-533 reaches the fused kernels with the
     * low-rank head: the row / column means of a depthwise dilated 3x3 convolution of S_v = Qe_v k^T are linear functionals of q and k
     * (row sums of S over three column ranges, shifted by the dilation), which the caller evaluates without ever forming a plane
     * (mop_amd/ops.py: lens_mean_features).  2V + 2 + n_extra <= 26. */
    int32_t n_extra;
    const float *row_extra, *col_extra;
    float *d_row_extra, *d_col_extra;
} MopkEdgewiseExt;

typedef struct MopkEdgewiseArgs {
    int32_t B, H, N, dk;
    int32_t V;          /* number of score views (>= 2)            :362 */
    int32_t r;          /* gate_rank                               :277 */
    int32_t io_dtype;   /* MopkDtype of q,k,v,y,dy,dq,dk,dv        */
    int32_t precision;  /* MopkPrecision                           */
    int32_t path;       /* MopkPath                                */
    int32_t save_for_backward; /* fused path: 1 = fwd also exports the chain state (prefix products, softmax constants,
                                * log-means) and the mix state (mixed logits, view log-sum-exp in fp32, softmax row statistics,
                                * P v0) into `saved`, and _bwd reads them.  0 = small `saved` (w * y_chain only); _bwd then
                                * re-runs the forward kernel into its workspace first to obtain that record (workspace_bytes()
                                * grows by the record's size).  Must have the same value in the fwd call, the bwd call and
                                * both *_bytes() queries.  The fused _bwd is three launches on `stream` (mix backward, the two
                                * D-chains, per-view gradients) that hand packed N x N slabs to each other through `workspace`. */
    float beta_not;     /* :361, used at :546 */

    MopkView5 q, k;          /* per-view (sv!=0) or shared (sv==0) queries / keys  :461-470 */
    MopkView4 v0, vL;        /* values of view 0 and of the last view :553-557 (before v_scale) */
    const float *sqk;        /* (V,H,dk) fp32, see above */
    const float *vs0, *vsL;  /* (H,dk) fp32: v_scale[0], v_scale[V-1] (ones when unshared) */
    const float *Wr, *br;    /* edge_head.row_proj weight (4r, 2V+2) / bias (4r)  :277 */
    const float *Wc, *bc;    /* edge_head.col_proj                                 :278 */
    const float *chain_logit;/* chain_value_logit, 1 fp32 on device                :451 */

    MopkView4 y;             /* out: (B,H,N,dk) view of the (B,N,D) tensor fed to proj :563 */

    void *saved;             /* out (fwd) / in (bwd): mopk_edgewise_saved_bytes() bytes */
    void *workspace;         /* scratch: mopk_edgewise_workspace_bytes() bytes */

    /* ---- backward only (ignored by _fwd) ---- */
    MopkView4 dy;            /* in : dL/dy, same geometry as y */
    MopkView5 dq, dk_;       /* out: dL/dq, dL/dk; sv==0 -> summed over views */
    MopkView4 dv0, dvL;      /* out: dL/dv0, dL/dvL (v_scale applied); dv0.ptr == dvL.ptr -> their sum is written once */
    float *dsqk_part;        /* out: (B,V,H,dk) */
    float *dvs0_part, *dvsL_part; /* out: (B,H,dk) */
    float *dWr, *dbr, *dWc, *dbc; /* out: (4r,2V+2),(4r),(4r,2V+2),(4r) -- fully reduced */
    float *dlogit_part;      /* out: (B,H) */

    const MopkEdgewiseExt *ext; /* host pointer; NULL = low-rank head without lens bank (the only form the fused path takes) */
    float dropout_p;         /* attn_drop on the mixed attention weights (:552); see MopkSdpaArgs.dropout_p */
    uint64_t dropout_seed;
    /* Optional attention mask, 1 = keep (generic path only).  EXTENSION: the reference's masked EdgewiseMSA is NaN for any blocking
     * mask (-inf scores enter the feature stack, :504-506 -> :518-546).  Here the mask acts on the probabilities only -- the per-view
     * softmaxes (:507) and the final one (:549-551); gate features see the unmasked scores.  Every row must keep at least one key. */
    const uint8_t *mask;
    int64_t mask_sb, mask_sh, mask_si;
} MopkEdgewiseArgs;

size_t mopk_edgewise_saved_bytes(const MopkEdgewiseArgs *a);
size_t mopk_edgewise_workspace_bytes(const MopkEdgewiseArgs *a);
int mopk_edgewise_lowrank_fwd(const MopkEdgewiseArgs *a, void *stream);   /* requires ext == NULL or ext->gate_mode == 0 */
int mopk_edgewise_lowrank_bwd(const MopkEdgewiseArgs *a, void *stream);
int mopk_edgewise_fwd(const MopkEdgewiseArgs *a, void *stream);           /* any head / lens variant (ext) */
int mopk_edgewise_bwd(const MopkEdgewiseArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * MultiHopMSA (dual-path, scalar gates) attention core.
 * Replaces reference mop/models/attention_variants.py:200-229
 * (and experiments/cifar10_twohop_gates.py:55-99 `dual_path_mix`).
 * mask: optional uint8 (1 = keep, 0 = blocked), element (b,h,i,j) at
 * mask + b*mask_sb + h*mask_sh + i*mask_si + j (strides may be 0 to broadcast);
 * `causal` != 0 adds the lower-triangular mask without reading memory.
 * -------------------------------------------------------------------------- */
typedef struct MopkDualPathArgs {
    int32_t B, H, N, dk;
    int32_t hops;            /* >= 2  :174 ; 0 = no value-transport term (two-score attention only; fused kernels only,
                              * v2 / dv2 / chain_logit unused) -- CrossViewMixerMSA's 2x2 mix folds into (k1', k2') */
    int32_t io_dtype, precision, path;
    int32_t causal;
    float g_and, g_or, g_not, g_chain; /* python-float gates :188 */
    float beta_not;
    MopkView4 q1, k1, v1, q2, k2, v2;
    const uint8_t *mask;
    int64_t mask_sb, mask_sh, mask_si;
    const float *chain_logit;
    MopkView4 y;
    void *saved, *workspace;
    /* backward */
    MopkView4 dy, dq1, dk1, dv1, dq2, dk2, dv2;
    float *dlogit_part;      /* (B,H) */
    float dropout_p;         /* attn_drop on the mixed attention weights (attention_variants.py:222; the transport term uses the
                              * undropped A1, A2 :224-227); fused path only, see MopkSdpaArgs.dropout_p */
    uint64_t dropout_seed;
} MopkDualPathArgs;

size_t mopk_dualpath_saved_bytes(const MopkDualPathArgs *a);
size_t mopk_dualpath_workspace_bytes(const MopkDualPathArgs *a);
int mopk_dualpath_fwd(const MopkDualPathArgs *a, void *stream);
int mopk_dualpath_bwd(const MopkDualPathArgs *a, void *stream);
/* 1 if MOPK_PATH_AUTO runs this call on the fused kernels: bf16 arithmetic, dk 32/64, chain gate 0 (causal flag and mask tensor ok) */
int mopk_dualpath_fused_supported(const MopkDualPathArgs *a);

/* --------------------------------------------------------------------------
 * Quartet CausalSelfAttention core.
 * Replaces reference mop/models/quartet_attn_patch.py:88-121 (scores, row
 * z-norm with unbiased std over the full row, product mix, causal mask,
 * additive attention_mask, softmax, AV).  use_quartet==0 -> :108-110.
 * add_mask: optional fp32 additive mask, element (b,h,i,j) at
 * add_mask + b*am_sb + h*am_sh + i*am_si + j.
 * -------------------------------------------------------------------------- */
typedef struct MopkQuartetArgs {
    int32_t B, H, T, dh;
    int32_t io_dtype, precision, path;
    int32_t use_quartet;
    float eps;               /* score_norm_eps :31 */
    MopkView4 q, k, v, q2, k2;
    const float *mixture;        /* 1 fp32 on device :52 */
    const float *quartet_scale;  /* 1 fp32 on device :55 */
    const float *add_mask;
    int64_t am_sb, am_sh, am_si;
    MopkView4 y;
    float *attn;             /* optional out (B,H,T,T) fp32 for need_weights=True :125 */
    void *saved, *workspace;
    /* backward */
    MopkView4 dy, dq, dk_, dv, dq2, dk2;
    float *dmixture_part, *dqscale_part; /* (B,H) */
    float dropout_p;         /* attn_dropout on the probabilities (quartet_attn_patch.py:119); see MopkSdpaArgs.dropout_p */
    uint64_t dropout_seed;
} MopkQuartetArgs;

size_t mopk_quartet_saved_bytes(const MopkQuartetArgs *a);
size_t mopk_quartet_workspace_bytes(const MopkQuartetArgs *a);
int mopk_quartet_fwd(const MopkQuartetArgs *a, void *stream);
int mopk_quartet_bwd(const MopkQuartetArgs *a, void *stream);  /* needs q,k,v,(q2,k2), y (forward output), dy */
/* 1 if MOPK_PATH_AUTO runs this call on the fused kernels: bf16 arithmetic, dh 32/64, no add_mask, attn == NULL */
int mopk_quartet_fused_supported(const MopkQuartetArgs *a);

/* The Quartet core over a batch of right-padded rows.  (Added under version 118: new exports only, no layout of an existing
 * struct changes; callers detect them with mopk_quartet_lens_fused_supported.)
 * lens: device (B) int32 or NULL (= full rows); n_b = clamp(lens[b], 0, T).  Row i < n_b z-normalises both score maps over the
 * keys j < n_b only -- mean, unbiased std with max(n_b - 1, 1), the same sd == 0 guard -- and attends to j <= i: it comes out
 * as the row alone at T = n_b would.  Nothing at or beyond a length is used, NaN / Inf included.  Padding queries get y = 0 and
 * dq = dq2 = 0 written, padding keys dk = dk2 = dv = 0; padding rows add nothing to dmixture_part / dqscale_part.  The dropout
 * mask is indexed by the padded positions (b,h,i,j).  With need_weights (base.attn, generic path) rows and columns beyond a
 * length of the returned map are 0.  With all lengths equal to T the results are bitwise those of mopk_quartet_fwd / _bwd on
 * the same path.  base.add_mask must be NULL (MOPK_ERR_BAD_ARG otherwise).  Sizes, the path decision, argument checks and the
 * path == FUSED refusals are those of mopk_quartet_* on base.  Pass the same lengths to _fwd and _bwd. */
typedef struct MopkQuartetLensArgs {
    MopkQuartetArgs base;    /* unchanged meaning; base.add_mask must be NULL */
    const int32_t *lens;     /* device (B) int32, 4-byte aligned, or NULL */
} MopkQuartetLensArgs;
size_t mopk_quartet_lens_saved_bytes(const MopkQuartetLensArgs *a);
size_t mopk_quartet_lens_workspace_bytes(const MopkQuartetLensArgs *a);
int mopk_quartet_lens_fwd(const MopkQuartetLensArgs *a, void *stream);
int mopk_quartet_lens_bwd(const MopkQuartetLensArgs *a, void *stream);
int mopk_quartet_lens_fused_supported(const MopkQuartetLensArgs *a);

/* --------------------------------------------------------------------------
 * Plain scaled-dot-product attention core.
 * Replaces BaselineMSA.forward attention_variants.py:42-46, MSA.forward
 * components.py:61-64, MultiheadSelfAttention.forward whisper_mop.py:163-175
 * and MultiheadCrossAttention.forward whisper_mop.py:198-228 (Nk != N).
 * path: MOPK_PATH_AUTO picks the fused kernels (sdpa_flash.hip: no N x N map in HBM) when they cover the call.
 * -------------------------------------------------------------------------- */
typedef struct MopkSdpaArgs {
    int32_t B, H, N, dk;
    int32_t io_dtype, precision, path;
    int32_t causal;
    MopkView4 q, k, v;
    const uint8_t *mask;     /* optional, 1 = keep */
    int64_t mask_sb, mask_sh, mask_si;
    const float *bias;       /* optional additive fp32 */
    int64_t bias_sb, bias_sh, bias_si;
    MopkView4 y;
    void *saved, *workspace;
    MopkView4 dy, dq, dk_, dv;
    /* attention dropout (`self.attn_drop(A)` components.py:62, attention_variants.py:45, `self.attn_dropout` quartet_attn_patch.py:119):
     * probabilities are multiplied by keep(b,h,i,j) / (1 - dropout_p) after the softmax, keep = mopk_dropout_keep(); the same
     * function is evaluated again in _bwd (nothing is stored), so pass the same p and seed to both.  0 = off.  Both paths draw the
     * same mask from a seed (the generic path multiplies its N x N map by it in a workspace plane). */
    float dropout_p;
    uint64_t dropout_seed;
    /* key / value length (cross-attention, whisper_mop.py:180-228); 0 = N.  With Nk != N, N is the query length: q, y, dy, dq are
     * (B, N, H, dk), k, v, dk_, dv are (B, Nk, H, dk), mask and bias are (., ., N, Nk) with the row strides above.  causal with
     * Nk != N is MOPK_ERR_UNSUPPORTED. */
    int32_t Nk;
} MopkSdpaArgs;

size_t mopk_sdpa_saved_bytes(const MopkSdpaArgs *a);
size_t mopk_sdpa_workspace_bytes(const MopkSdpaArgs *a);
int mopk_sdpa_fwd(const MopkSdpaArgs *a, void *stream);
int mopk_sdpa_bwd(const MopkSdpaArgs *a, void *stream);  /* needs q,k,v, y (forward output), dy; mask/bias as in the forward */
/* 1 if the fused (flash-style) gfx950 kernels take this call under MOPK_PATH_AUTO: bf16 arithmetic, dk 32/64, no mask/bias tensor */
int mopk_sdpa_fused_supported(const MopkSdpaArgs *a);
/* The dropout mask of the fused kernels as a host function (tests / reproducibility): 1 if edge (query i, key j) of head-batch
 * index bh = b * H + h is kept under (seed, p).  Counter-based: lowbias32(lowbias32(i * 0x9E3779B1 + bh * 0x85EBCA77 + seed_hi)
 * ^ seed_lo ^ j * 0xC2B2AE3D) >= p * 2^32. */
int mopk_dropout_keep(uint64_t seed, float p, int64_t bh, int64_t i, int64_t j);

/* --------------------------------------------------------------------------
 * Plain SDPA with per-row lengths: a batch of right-padded sequences (WhisperMoP with audio clips of unequal length).  (Added
 * under version 118: new exports only, MopkSdpaArgs is unchanged.)  base.mask and base.bias must be NULL.
 * q_lens[b] / kv_lens[b] are clamped into [0, N] / [0, Nk]; a NULL pointer means the full length.
 *   query i < q_lens[b] attends to keys j < kv_lens[b] (and j <= i with causal); a query with no open key gives y = 0, dq = 0;
 *   padding queries (i >= q_lens[b]): y = 0 and dq = 0 are written, and they add nothing to dk, dv whatever dy holds there;
 *   padding keys (j >= kv_lens[b]): dk = dv = 0 are written;
 *   nothing beyond a length is used: the result does not depend on what q, k, v, dy hold there (NaN and Inf included);
 *   dropout: keep(seed, b*H+h, i, j) is indexed by the padded positions, so a seed gives the mask of mopk_sdpa_fwd;
 *   with every length full (or both pointers NULL) y, dq, dk, dv are bitwise those of mopk_sdpa_fwd / _bwd on base.
 * Fused path (what mopk_sdpa_fused_supported(&base) takes): the length is a loop bound of the flash kernels, read once per
 * workgroup -- key tiles beyond kv_lens[b] and query blocks beyond q_lens[b] are skipped, only the last tile is edge-masked, no
 * mask bytes are read.  Generic path: the lengths block edges in the softmax kernel and zero the gathered padding rows.
 * Saved / workspace sizes are those of base.  Pass the same lengths to _fwd and _bwd. */
typedef struct MopkSdpaLensArgs {
    MopkSdpaArgs base;       /* unchanged meaning; base.mask and base.bias must be NULL */
    const int32_t *q_lens;   /* device (B) int32, 4-byte aligned, or NULL: query rows i >= q_lens[b] are padding */
    const int32_t *kv_lens;  /* device (B) int32, 4-byte aligned, or NULL: keys j >= kv_lens[b] are blocked */
} MopkSdpaLensArgs;
int mopk_sdpa_lens_supported(const MopkSdpaLensArgs *a);     /* 1 if the fused kernels take this call under MOPK_PATH_AUTO */
size_t mopk_sdpa_lens_saved_bytes(const MopkSdpaLensArgs *a);
size_t mopk_sdpa_lens_workspace_bytes(const MopkSdpaLensArgs *a);
int mopk_sdpa_lens_fwd(const MopkSdpaLensArgs *a, void *stream);
int mopk_sdpa_lens_bwd(const MopkSdpaLensArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * CrossViewMixerMSA attention core.
 * Replaces reference mop/models/attention_variants.py:90-110 (`_compute_logits`: S1, S2, S12, S21, 2x2 mix,
 * transpose cues) and :120-153 (mask, softmax, optional per-key prior sharpening, A v1).
 * anchor_mode: 0 = "fixed" (row clamp(fixed_k_star)), 1 = "argmax_row_sum" (argmax over the row sums of
 * softmax(S2) -- all ~1, i.e. decided by rounding; reproduced as written), 2 = any other string (row 0).
 * -------------------------------------------------------------------------- */
typedef struct MopkCrossViewArgs {
    int32_t B, H, N, dk;
    int32_t io_dtype, precision, path;
    int32_t causal;
    int32_t use_prior;       /* enable_per_key_prior && prior_weight > 0   :126 */
    int32_t anchor_mode, fixed_k_star;
    float t1, t2;            /* transpose-cue weights; 0 when use_transpose_cues is False :106-110 */
    float prior_weight;
    MopkView4 q1, k1, v1, q2, k2;
    const float *mix;        /* (2,2) fp32 on device :78 */
    const uint8_t *mask;     /* optional, 1 = keep */
    int64_t mask_sb, mask_sh, mask_si;
    MopkView4 y;
    void *saved, *workspace;
    int32_t *k_star;         /* optional out (B,H) int32: anchor row used by the prior */
    /* backward */
    MopkView4 dy, dq1, dk1, dv1, dq2, dk2;
    float *dmix_part;        /* (B,H,4) */
    float dropout_p;         /* attn_drop on the final attention weights (:151), see MopkSdpaArgs.dropout_p */
    uint64_t dropout_seed;
} MopkCrossViewArgs;

size_t mopk_crossview_saved_bytes(const MopkCrossViewArgs *a);
size_t mopk_crossview_workspace_bytes(const MopkCrossViewArgs *a);
int mopk_crossview_fwd(const MopkCrossViewArgs *a, void *stream);
int mopk_crossview_bwd(const MopkCrossViewArgs *a, void *stream);

/* Sum the per-batch partial gradients an Edgewise backward left in a->dsqk_part (B,V,H,dk), a->dvs0_part, a->dvsL_part
 * (B,H,dk) and a->dlogit_part (B,H) over the batch, in a fixed order (bitwise reproducible), into dsqk (V,H,dk), dvs0, dvsL
 * (H,dk) and dlogit (1): one launch in place of the four reductions `q_scale.grad`, `v_scale.grad` and
 * `chain_value_logit.grad` would otherwise need on the host side (attention_variants.py:374-378, :451 are the parameters).
 * Reads only B, V, H, dk and the four *_part pointers of `a`. */
int mopk_edgewise_reduce_parts(const MopkEdgewiseArgs *a, float *dsqk, float *dvs0, float *dvsL, float *dlogit, void *stream);

/* Small-parameter prologue / epilogue of a share_qkv EdgewiseMSA layer with the low-rank head (added without a version bump: new
 * exports only).  The layer's small parameters -- q_scale, k_scale, v_scale (V,H,1,dk) :374-378, the head's Wr, br, Wc, bc and
 * chain_value_logit :451 -- are stored in `io_dtype` (one dtype for all of them, contiguous); the core reads float32 copies.
 *   _params_fwd: ONE launch writes `pack`, n_pack = V H dk + 2 H dk + 2 (4r C) + 2 (4r) + 1 floats laid out as
 *     sqk (V,H,dk) | vs0 (H,dk) | vsL (H,dk) | Wr (4r,C) | br | Wc | bc | logit, with sqk = rnd(rnd(q_scale k_scale) inv),
 *     inv = (float)(1 / sqrt(dk)), rnd = round-to-nearest-even to io_dtype, every product a separate float32 multiply: the values
 *     `(q_scale * k_scale) * inv` has when evaluated tensor by tensor in io_dtype.  vs0 / vsL = v_scale[0] / v_scale[V-1].
 *   _params_bwd: ONE launch after mopk_edgewise_lowrank_bwd, in place of mopk_edgewise_reduce_parts.  Sums the per-batch partials
 *     in that function's order, then finishes the chain rule with the roundings a tensor-by-tensor evaluation in io_dtype has:
 *     g = rnd(dsqk), g2 = rnd(g inv), dq_scale = rnd(g2 k_scale), dk_scale = rnd(g2 q_scale); dv_scale[0] = rnd(dvs0),
 *     dv_scale[V-1] = rnd(dvsL), rows between zero; gWr .. gbc = rnd(dWr .. dbc) (the float32 values _bwd left), glogit = rnd(dlogit).
 *     Every output is a separate contiguous array of the parameter's shape.
 * Neither allocates nor synchronises (safe under stream capture). */
typedef struct MopkEdgewiseParamArgs {
    int32_t B, V, H, dk, r;
    int32_t C;               /* input channels of the head: 2V + 2 */
    int32_t io_dtype;        /* MopkDtype of the parameters and of their gradients */
    const void *q_scale, *k_scale, *v_scale;       /* (V,H,1,dk) */
    const void *Wr, *br, *Wc, *bc;                 /* (4r,C), (4r), (4r,C), (4r) */
    const void *chain_logit;                       /* 1 */
    float *pack;                                   /* _fwd out: n_pack floats */
    /* ---- _params_bwd only ---- */
    const float *dsqk_part, *dvs0_part, *dvsL_part, *dlogit_part;   /* as in MopkEdgewiseArgs: (B,V,H,dk), (B,H,dk) x 2, (B,H) */
    const float *dWr, *dbr, *dWc, *dbc;            /* float32, fully reduced (MopkEdgewiseArgs.dWr ..) */
    void *gq_scale, *gk_scale, *gv_scale;          /* out, io_dtype: (V,H,1,dk) */
    void *gWr, *gbr, *gWc, *gbc, *glogit;          /* out, io_dtype */
} MopkEdgewiseParamArgs;
int mopk_edgewise_params_fwd(const MopkEdgewiseParamArgs *p, void *stream);
int mopk_edgewise_params_bwd(const MopkEdgewiseParamArgs *p, void *stream);

/* -------------------------------------------------------------------------- */
/* LayerNorm prologue / residual epilogue of the attention path.
 *
 * Replaces, around the core, the `self.ln1(x)` of `x = x + self.dp1(self.attn(self.ln1(x)))`
 * (experiments/cifar100_edgewise_gates.py:371-374; mop/models/components.py:96-98 is the same block): the forward applies
 * torch.nn.LayerNorm (biased variance, eps inside the sqrt, fp32 statistics) to `rows` token rows of width `dim` and writes the
 * result in `y_dtype` -- the dtype the qkv GEMM consumes -- in one pass; mean / rstd are kept for the backward.  The backward
 * returns dx = dres + LN'(dy): `dres` is the gradient arriving on the residual branch (NULL: none), so the `x + ...` add of the
 * block costs no extra pass.  dgamma / dbeta are summed over rows in a fixed order (bitwise reproducible).
 * Rows are contiguous with leading dimensions x_ld / y_ld (elements, multiples of 8); dim % 8 == 0, dim <= 4096, pointers
 * 16-byte aligned; anything else returns MOPK_ERR_UNSUPPORTED / MOPK_ERR_BAD_ARG. */
typedef struct MopkLayerNormArgs {
    int64_t rows;
    int32_t dim;
    int32_t x_dtype, y_dtype, p_dtype;   /* MopkDtype of x/dx/dres, of y/dy, of gamma/beta */
    float eps;
    int64_t x_ld, y_ld;
    const void *x, *gamma, *beta;        /* beta may be NULL */
    void *y;                             /* forward out */
    float *mean, *rstd;                  /* (rows) fp32: forward out (both or neither), backward in */
    const void *dy, *dres;               /* backward in; dres may be NULL */
    void *dx;                            /* backward out (may alias dres) */
    float *dgamma, *dbeta;               /* (dim) fp32 backward out; either may be NULL */
    void *workspace;                     /* backward: mopk_layernorm_workspace_bytes() */
} MopkLayerNormArgs;
size_t mopk_layernorm_workspace_bytes(const MopkLayerNormArgs *a);
int mopk_layernorm_fwd(const MopkLayerNormArgs *a, void *stream);
int mopk_layernorm_bwd(const MopkLayerNormArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Row / column means of the S lens bank's planes in closed form -- the values MopkEdgewiseExt.row_extra / col_extra take.
 * The bank (attention_variants.py:425-442, :523-533) convolves every score plane S_v = (q * sqk_v) k^T with a depthwise dilated
 * 3x3 kernel (zero padding = dilation); the low-rank head reads only row / column means of the result (:323-326), which are
 * linear functionals of q and k (O(N dk) per (b, h, view); see mop_amd/csrc/lens_means.hip).  N <= 224, dk in {16, 32, 64},
 * L * V <= 16, and a working set (grows with the largest dilation) within the CU's 160 KB of LDS: mopk_lens_means_supported.  q / k: the shared (sv == 0) queries / keys of the Edgewise call.
 *   _fwd: row, col (B,H,L*V,N) fp32, channel l * V + v (the reference's order, :531).
 *   _bwd: given d_row / d_col, ADDS the q / k gradients into dq / dk_ (the buffers the Edgewise backward has already written,
 *         io_dtype elements) and writes per-(b) / per-(b,h) partials of the scale and weight gradients for the caller to sum:
 *         dsqk_part (B,V,H,dk), dlens_part (B*H,L,V,3,3). */
typedef struct MopkLensMeansArgs {
    int32_t B, H, N, dk, V, L;
    int32_t io_dtype;              /* MopkDtype of q, k, dq, dk_ */
    int32_t dil[MOPK_MAX_LENS];    /* dilation == padding of each lens   :430-436 */
    MopkView4 q, k;
    const float *sqk;              /* (V,H,dk) fp32, as MopkEdgewiseArgs.sqk */
    const float *lens_w;           /* (L,V,3,3) fp32: lens_bank[l].weight[:, 0] */
    float *row, *col;              /* fwd out */
    const float *d_row, *d_col;    /* bwd in  */
    MopkView4 dq, dk_;             /* bwd in/out: += */
    float *dsqk_part, *dlens_part; /* bwd out */
} MopkLensMeansArgs;
int mopk_lens_means_supported(const MopkLensMeansArgs *a, int backward);   /* 1 if the kernels take this shape (dimensions and dil only) */
int mopk_lens_means_fwd(const MopkLensMeansArgs *a, void *stream);
int mopk_lens_means_bwd(const MopkLensMeansArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * 1-D MoP token gate of the GPT-MoP block (mop/models/gpt_mop.py:109-123), residual add included.  (Added under version 118:
 * new exports only, no existing layout changes; callers detect it with mopk_token_gate_supported.)
 * The reference gate  views = Wv r ; K = conv1d(views, Wk, pad 1) ; g = Wf [views ; K] ; gate = 1 + a0 g0 - a1 g1  is linear
 * in r, so it folds (mop_amd/ops.py token_gate_taps, in torch) into three taps u (3,D):
 *     r_t = x_t + a_t ,   gate_t = 1 + u[0] . r_{t-1} + u[1] . r_t + u[2] . r_{t+1}   (zero outside [0,T), never across b),
 *     out_t = r_t * gate_t .
 *   _fwd: out (o_dtype) and gate (B,T) fp32 (kept for the backward).
 *   _bwd: with delta_t = dout_t . r_t (r recomputed from x, a):
 *         dr_t = dout_t gate_t + u[0] delta_{t+1} + u[1] delta_t + u[2] delta_{t-1}    (the gradient of both x and a),
 *         du[s] = sum_{b,t} delta_t r_{t+s-1}, per-workgroup partials in `workspace`, summed by a second launch in a fixed order.
 * x / a: (B,T,D) with element strides (sb, st), innermost contiguous; a may be NULL (r = x).  o_dtype must be the promotion of
 * x_dtype and a_dtype (F32 if either is F32, else BF16).  out / dout / dr: contiguous (B,T,D) o_dtype.  D % 8 == 0, D <= 1024,
 * strides multiples of 8, 16-byte aligned pointers; mopk_token_gate_supported says whether a call is taken. */
typedef struct MopkTokenGateArgs {
    int32_t B, T, D;
    int32_t x_dtype, a_dtype, o_dtype;   /* MopkDtype; a_dtype is ignored when a == NULL */
    const void *x;
    int64_t x_sb, x_st;
    const void *a;                       /* NULL: no residual branch */
    int64_t a_sb, a_st;
    const float *u;                      /* (3,D) fp32 contiguous: taps of r_{t-1}, r_t, r_{t+1} */
    void *out;                           /* fwd out */
    float *gate;                         /* (B,T) fp32: fwd out, bwd in */
    const void *dout;                    /* bwd in */
    void *dr;                            /* bwd out */
    float *du;                           /* bwd out (3,D) fp32 */
    void *workspace;                     /* bwd: mopk_token_gate_workspace_bytes() */
} MopkTokenGateArgs;
int mopk_token_gate_supported(const MopkTokenGateArgs *a);                /* 1 if the kernels take this call (shape, dtypes, strides, alignment) */
size_t mopk_token_gate_workspace_bytes(const MopkTokenGateArgs *a);
int mopk_token_gate_fwd(const MopkTokenGateArgs *a, void *stream);
int mopk_token_gate_bwd(const MopkTokenGateArgs *a, void *stream);

/* The token gate over right-padded rows (new exports under version 118; detect with mopk_token_gate_lens_supported).
 * lens: device (B) int32 or NULL (= full rows); n_b = clamp(lens[b], 0, T).  r_t counts as 0 for t >= n_b, so gate_{n_b - 1} has
 * no u2 term.  Rows t >= n_b get out = 0, dr = 0 and gate = 1 written and add nothing to du; they are never read (a NaN there
 * changes nothing).  Full lengths are bitwise the call without lengths, du included.  Checks and the workspace size are base's. */
typedef struct MopkTokenGateLensArgs {
    MopkTokenGateArgs base;
    const int32_t *lens;     /* device (B) int32, 4-byte aligned, or NULL */
} MopkTokenGateLensArgs;
int mopk_token_gate_lens_supported(const MopkTokenGateLensArgs *a);
size_t mopk_token_gate_lens_workspace_bytes(const MopkTokenGateLensArgs *a);
int mopk_token_gate_lens_fwd(const MopkTokenGateLensArgs *a, void *stream);
int mopk_token_gate_lens_bwd(const MopkTokenGateLensArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Top-1 routed mixture-of-experts MLP (mop/models/components.py:84-121 MoEMLP), optional residual add.  (Added under version 118:
 * new exports only, no existing layout changes; callers detect it with mopk_moe_supported.)
 *   e_t = argmax_e (gate_w[e] . x_t + gate_b[e])   (fp32 FMA logits whatever the dtypes; ties -> lowest e, as torch.argmax)
 *   y_t = W2_{e_t} gelu_tanh(W1_{e_t} x_t) [+ residual_t]
 * Only the routed expert runs on a token.  Per-expert token counts stay on the device; every launch is graph-capturable.
 * route: int32, 2 M + E + 1 entries = [expert of each token (M) | perm (M): sorted position -> token, experts in index order,
 *        tokens ascending inside an expert (stable) | offsets (E + 1): expert e owns sorted positions [off[e], off[e+1])].
 *   _route: writes route (used by _fwd, callable alone).
 *   _fwd:   route, then u = W1_e x (pre-activation) and h = gelu(u), both (M,F) in sorted order and the activation dtype (BF16 under
 *           PREC_BF16, else F32; kept for _bwd), then y (M,D) o_dtype in token order.
 *   _bwd:   with route, u, h from _fwd and dy (M,D) o_dtype: dx (M,D) x_dtype (the residual's gradient is dy itself, not written),
 *           dw1[e] (F,D) and dw2[e] (D,F) in w_dtype, zeros for an expert without tokens.  Weight gradients are fp32 partial slabs per
 *           fixed-size row chunk summed in chunk order: no atomics, bitwise reproducible.
 * x, y, residual, dy, dx: contiguous (M,D); gate_w (E,D), gate_b (E) or NULL in gate_dtype; w1[e] (F,D), w2[e] (D,F) contiguous in
 * w_dtype, read in place.  PREC_FP32 (exact fp32 MFMA) needs x, w and o all F32; PREC_BF16 (bf16 MFMA operands, fp32 accumulation)
 * takes any F32 / BF16 mix.  D % 8 == 0, F % 8 == 0, 2 <= E <= MOPK_MOE_MAX_EXPERTS, 16-byte aligned pointers. */
#define MOPK_MOE_MAX_EXPERTS 64
typedef struct MopkMoeArgs {
    int32_t M, D, F, E;                  /* tokens, model width, hidden width, experts */
    int32_t precision;                   /* MopkPrecision */
    int32_t x_dtype, w_dtype, gate_dtype, o_dtype;   /* MopkDtype: x / dx; w1, w2, dw1, dw2; gate_w, gate_b; y, residual, dy */
    int32_t reserved;
    const void *x;
    const void *gate_w;
    const void *gate_b;                  /* NULL: no gate bias */
    const void *w1[MOPK_MOE_MAX_EXPERTS];
    const void *w2[MOPK_MOE_MAX_EXPERTS];
    const void *residual;                /* NULL: no residual add */
    void *y;                             /* fwd out */
    void *u, *h;                         /* fwd out, bwd in: (M,F) activation dtype, sorted order */
    int32_t *route;                      /* fwd / route out, bwd in */
    const void *dy;                      /* bwd in */
    void *dx;                            /* bwd out */
    void *dw1[MOPK_MOE_MAX_EXPERTS];     /* bwd out */
    void *dw2[MOPK_MOE_MAX_EXPERTS];     /* bwd out */
    void *workspace;                     /* bwd: mopk_moe_workspace_bytes(a, 1) */
} MopkMoeArgs;
int mopk_moe_supported(const MopkMoeArgs *a);                       /* 1 if the kernels take this call (shape, dtypes, precision, alignment) */
size_t mopk_moe_workspace_bytes(const MopkMoeArgs *a, int backward); /* 0 for the forward */
int mopk_moe_route(const MopkMoeArgs *a, void *stream);
int mopk_moe_fwd(const MopkMoeArgs *a, void *stream);
int mopk_moe_bwd(const MopkMoeArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Attention of a few new queries against a key / value cache: incremental (KV-cached) decoding of the WhisperMoP decoder
 * (mop/models/whisper_mop.py:137-221 attention cores, one step at a time).  Inference only, no backward.  (Added under version 118:
 * new exports only, no existing layout changes; callers detect it with mopk_decode_attn_supported.)
 *   y_i = softmax_j(q_i . k_j / sqrt(dk)) v_j  over the keys j < L (and j < L - Tq + i + 1 with causal)
 * L = *kv_len when kv_len != NULL (device memory, read by the kernels: the caller sets it to the length after this step's append, so
 * the launch arguments do not change from step to step and a step can be captured once in a graph), else L = Nk.  L is clamped to
 * [0, cap].  causal is BOTTOM-RIGHT aligned: the Tq queries are the last Tq positions of the L keys, query i (0-based) sees keys
 * j < L - Tq + i + 1.  A query that sees no key gets y = 0.
 * q, y: (B, Tq, H, dk) views; k, v: (B, cap, H, dk) views of a cache buffer (only the first L rows are read).  1 <= Tq <= 16,
 * dk in {32, 64, 128}, 0 <= Nk <= cap (Nk >= 1 without kv_len).  k / v: 16-byte aligned pointers and strides that are whole 16-byte
 * vectors; q / y: any element strides.  F32: exact fp32 arithmetic; BF16: bf16 io, fp32 arithmetic.
 * Split-KV: one workgroup per (b, h, chunk of 64 or 128 keys), chunk count fixed by cap; a second launch merges the per-chunk
 * partials in chunk order.  No atomics: bitwise reproducible.  workspace: mopk_decode_attn_workspace_bytes(). */
typedef struct MopkDecodeAttnArgs {
    int32_t B, H, Tq, dk;                /* batch, heads, new queries per row, head size */
    int32_t cap;                         /* rows of the k / v cache views */
    int32_t Nk;                          /* valid keys when kv_len is NULL */
    int32_t io_dtype;                    /* MopkDtype of q, k, v and y */
    int32_t causal;                      /* 0 / 1, bottom-right aligned (above) */
    MopkView4 q, k, v;
    MopkView4 y;                         /* out */
    const int32_t *kv_len;               /* device: valid keys (one int32), or NULL for Nk */
    void *workspace;
} MopkDecodeAttnArgs;
int mopk_decode_attn_supported(const MopkDecodeAttnArgs *a);         /* 1 if the kernels take this call (shape, dtype, strides, alignment) */
size_t mopk_decode_attn_workspace_bytes(const MopkDecodeAttnArgs *a);
int mopk_decode_attn_fwd(const MopkDecodeAttnArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Row-indirect decode attention: beam search over a cache whose slots are written once.  (Added under version 118: new exports
 * only; callers detect it with mopk_decode_attn_rows_supported.)  Exactly mopk_decode_attn_fwd, except that key / value j of query
 * row b is read from cache row rows[b * rows_ld + j] at position j instead of from row b.  rows: device int32 (B, >= cap) table,
 * rows_ld >= cap; an entry outside [0, B) is clamped into it.  With rows[b, j] = b the result is bitwise that of
 * mopk_decode_attn_fwd (same chunks, softmax, merge order and fp32 arithmetic).  Cost: one int32 read per key.  Workspace:
 * mopk_decode_attn_rows_workspace_bytes() (that of base). */
typedef struct MopkDecodeAttnRowsArgs {
    MopkDecodeAttnArgs base;             /* unchanged meaning; base.k / base.v: (B, cap, H, dk) views of the cache */
    const int32_t *rows;                 /* device: (B, rows_ld) int32 source-row table */
    int64_t rows_ld;                     /* elements between table rows, >= cap */
} MopkDecodeAttnRowsArgs;
int mopk_decode_attn_rows_supported(const MopkDecodeAttnRowsArgs *a);
size_t mopk_decode_attn_rows_workspace_bytes(const MopkDecodeAttnRowsArgs *a);
int mopk_decode_attn_rows_fwd(const MopkDecodeAttnRowsArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Ragged decode attention: prompts of different lengths left-padded in one cache.  (Added under version 118: new exports only;
 * callers detect it with mopk_decode_attn_ragged_supported.)  Exactly mopk_decode_attn_fwd (rows == NULL) or
 * mopk_decode_attn_rows_fwd (rows != NULL), except that query row b sees only the keys j >= s_b, s_b = kv_start[b] clamped into
 * [0, L]: query i of row b sees s_b <= j < L (causal: < L - Tq + i + 1).  Key rows below s_b are not read; a query that sees no
 * key gets y = 0.  With kv_start[b] = 0 the result is bitwise that of mopk_decode_attn_fwd / mopk_decode_attn_rows_fwd.
 * kv_start: device int32 (B), 4-byte aligned, required.  Workspace: mopk_decode_attn_ragged_workspace_bytes() (that of base). */
typedef struct MopkDecodeAttnRaggedArgs {
    MopkDecodeAttnArgs base;             /* unchanged meaning */
    const int32_t *rows;                 /* NULL: row b reads its own cache row; else as MopkDecodeAttnRowsArgs.rows */
    int64_t rows_ld;                     /* as MopkDecodeAttnRowsArgs.rows_ld when rows != NULL */
    const int32_t *kv_start;             /* device (B) int32, required: query row b sees keys j >= kv_start[b] */
} MopkDecodeAttnRaggedArgs;
int mopk_decode_attn_ragged_supported(const MopkDecodeAttnRaggedArgs *a);
size_t mopk_decode_attn_ragged_workspace_bytes(const MopkDecodeAttnRaggedArgs *a);
int mopk_decode_attn_ragged_fwd(const MopkDecodeAttnRaggedArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Decode attention with per-row key counts: the cross-attention of a decode step over right-padded audio of unequal length.
 * (Added under version 118: new exports only; callers detect it with mopk_decode_attn_lens_supported.)  Exactly
 * mopk_decode_attn_fwd with L = kv_lens[b] clamped into [0, base.Nk] for row b of q: chunks beyond L leave at once and the merge
 * ignores them, key rows >= L are never read, a row with L = 0 gets y = 0.  kv_lens[b] = Nk for every b is bitwise
 * mopk_decode_attn_fwd.  base.kv_len must be NULL and base.causal 0.  kv_lens: device int32 (B), 4-byte aligned, required.
 * Workspace: mopk_decode_attn_lens_workspace_bytes() (that of base). */
typedef struct MopkDecodeAttnLensArgs {
    MopkDecodeAttnArgs base;             /* base.kv_len NULL, base.causal 0 */
    const int32_t *kv_lens;              /* device (B) int32, required: row b of q sees keys j < kv_lens[b] */
} MopkDecodeAttnLensArgs;
int mopk_decode_attn_lens_supported(const MopkDecodeAttnLensArgs *a);
size_t mopk_decode_attn_lens_workspace_bytes(const MopkDecodeAttnLensArgs *a);
int mopk_decode_attn_lens_fwd(const MopkDecodeAttnLensArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * One step of batched beam search (WhisperMoP.beam_search): updates the device beam state in place from the step's last-position
 * logits, with no host synchronisation, so a step can be captured once in a graph.  (Added under version 118: new exports only;
 * callers detect it with mopk_beam_supported.)  Per batch item b that is not done (done[b] == 0):
 *   candidates (k, v), score = scores[b*K + k] + (logit[b, k, v] - lse[b, k]) in fp32, k < K, v < V; a beam's candidates are its 2K
 *   largest logits (ties: smaller v);  the item's top 2K candidates by score descending, ties to the smaller k * V + v;
 *   walk them in order: token eos with a finite score -> stored as finished hypothesis fin_count[b] (while fin_count[b] < K) with
 *   score / (pos - prompt_len + 1) ** length_penalty and tokens hist[b*K + k, :pos], eos; never a live beam.  Any other candidate
 *   -> the next live beam k': scores, parents (k), next_ids (v).  The walk stops when K live beams are filled.
 *   then hist and rows are reordered in place: row b*K + k' takes columns [0, pos) of row b*K + parents[k'], hist[., pos] = next_ids,
 *   rows[., pos] = b*K + k';  done[b] = fin_count[b] >= K.
 * pos = *pos: the history column of the new token (the cache length after the step's decode).  Done items are left untouched.
 * logits: row (b, k) at logits + b * logits_sb + k * logits_sk elements (logits_sk = 0: one row per item shared by its beams, the
 * first step), F32 or BF16, element-aligned; finite or -inf values.  1 <= K <= 8, 2 <= V, K * V < 2^31, pos in [prompt_len, T).
 * Launch A: one workgroup per (beam row, vocab slice): (max, sum-exp) and the top 2K of the slice, 16-byte loads;  launch B: one
 * workgroup per item: lse by a fixed-order merge, candidate merge, the walk and the reorder.  No atomics: bitwise reproducible. */
#define MOPK_BEAM_MAX_K 8
typedef struct MopkBeamArgs {
    int32_t B, K, V;                     /* batch items, beams per item, vocabulary */
    int32_t T;                           /* columns of hist, rows and fin_tokens */
    int32_t logits_dtype;                /* MopkDtype */
    int32_t eos;                         /* eos token id, or -1: no eos */
    int32_t prompt_len;                  /* history columns before the first new token */
    float length_penalty;
    const void *logits;
    int64_t logits_sb, logits_sk;        /* element strides of an item's and of a beam's logit row */
    const int32_t *pos;                  /* device: the new token's history column (one int32) */
    float *scores;                       /* (B*K) in / out: live beam log-probabilities */
    int32_t *next_ids;                   /* (B*K) out: the live beams' new tokens (the next decoder step's ids) */
    int32_t *parents;                    /* (B*K) out: beam index (0..K-1) each live beam extends */
    int32_t *hist;                       /* (B*K, hist_ld) in / out: token history */
    int64_t hist_ld;
    int32_t *rows;                       /* (B*K, rows_ld) in / out: MopkDecodeAttnRowsArgs.rows */
    int64_t rows_ld;
    int32_t *fin_tokens;                 /* (B, K, T) out: finished hypotheses; columns past their eos are not written */
    float *fin_scores;                   /* (B, K) out: length-normalised scores */
    int32_t *fin_count;                  /* (B) in / out */
    int32_t *done;                       /* (B) in / out */
    void *workspace;
} MopkBeamArgs;
int mopk_beam_supported(const MopkBeamArgs *a);                      /* 1 if the kernels take this call (K, V, T, dtype, strides) */
size_t mopk_beam_workspace_bytes(const MopkBeamArgs *a);
int mopk_beam_step(const MopkBeamArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Temperature / top-k / top-p sampling of one token per row (WhisperMoP.sample; inference only).  (Added under version 118: new
 * exports only; callers detect it with mopk_sample_supported.)  Row r (0 <= r < R) reads logits x at
 * logits + (r / n) * logits_sb + (r % n) * logits_sk elements (logits_sk = 0: one row shared by the n rows of an item), F32 or BF16,
 * element-aligned, finite or -inf values.  pos = *pos (device memory: one set of launch arguments serves every decoding step).
 *   greedy:  tokens[r] = argmax_v x_v, ties to the smaller v.
 *   else:    z_v = x_v * inv_temp (fp32);  top_k in (0, V): keep z_v >= the k-th largest z (counted with multiplicity, ties kept);
 *            top_p < 1: q_v = (uint64)(expf(z_v - max z) * 2^40) over the kept set, Q = sum q_v, P = ceil((double)top_p * Q),
 *            tau = the largest z_u with sum_{kept, z_v >= z_u} q_v >= P; keep z_v >= tau (tie-inclusive, never empty);
 *            tokens[r] = argmax_{v kept} z_v + G_v, ties to the smaller v, G_v = -logf(-logf(u)), u = ((h >> 9) + 0.5) * 2^-23,
 *            h = fa_hash(rh ^ v * 0xC2B2AE3D), rh = fa_hash(fa_hash(seed_lo ^ r * 0x9E3779B1) ^ seed_hi ^ pos * 0x85EBCA77)
 *            (common.h's fa_hash; all products mod 2^32).
 *   logprobs[r] = log_softmax(x)[tokens[r]] on the unscaled, unfiltered row.
 * One workgroup of 1024 threads per row streams the row once per pass (it stays in L2); the top-k and top-p thresholds are found by a
 * radix walk over the order-preserving uint32 key of z with integer LDS counts / fixed-point masses, so no result depends on the
 * order of an atomic.  No host synchronisation; bitwise reproducible.  workspace: mopk_sample_workspace_bytes() (0 today). */
#define MOPK_SAMPLE_MAX_V (1 << 24)       /* the fixed-point masses of a row sum exactly in 64 bits */
typedef struct MopkSampleArgs {
    int32_t R;                           /* rows sampled */
    int32_t n;                           /* rows per item: row r reads the logit row of item r / n */
    int32_t V;                           /* vocabulary, 2 <= V <= MOPK_SAMPLE_MAX_V */
    int32_t logits_dtype;                /* MopkDtype: F32 or BF16 */
    int32_t top_k;                       /* 0: off */
    int32_t greedy;                      /* 1: temperature 0 (argmax; inv_temp, top_k, top_p and seed unused) */
    float inv_temp;                      /* 1 / temperature rounded to fp32 once, finite and > 0 */
    float top_p;                         /* 1: off, else in (0, 1) */
    uint64_t seed;
    const void *logits;
    int64_t logits_sb, logits_sk;        /* element strides of an item's and of a row-in-item's logit row */
    const int32_t *pos;                  /* device: the sampled token's position (one int32) */
    int32_t *tokens;                     /* (R) out */
    float *logprobs;                     /* (R) out */
    void *workspace;                     /* may be NULL while mopk_sample_workspace_bytes() is 0 */
} MopkSampleArgs;
int mopk_sample_supported(const MopkSampleArgs *a);                  /* 1 if the kernel takes this call (V, dtype, filters, strides) */
size_t mopk_sample_workspace_bytes(const MopkSampleArgs *a);
int mopk_sample_step(const MopkSampleArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Sampling of a ragged batch (prompts left-padded in one cache).  (Added under version 118: new exports only; callers detect it
 * with mopk_sample_ragged_supported.)  Exactly mopk_sample_step, except that row r draws at position *pos - pos_off[r] instead of
 * *pos (the hash's pos), so a row's draws depend on its own token index and not on its batch's padding.  With pos_off[r] = 0 the
 * draw is bitwise that of mopk_sample_step.  pos_off: device int32 (R), 4-byte aligned, required. */
typedef struct MopkSampleRaggedArgs {
    MopkSampleArgs base;                 /* unchanged meaning */
    const int32_t *pos_off;              /* device (R) int32, required: row r draws at *pos - pos_off[r] */
} MopkSampleRaggedArgs;
int mopk_sample_ragged_supported(const MopkSampleRaggedArgs *a);
size_t mopk_sample_ragged_workspace_bytes(const MopkSampleRaggedArgs *a);
int mopk_sample_ragged_step(const MopkSampleRaggedArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Whisper's logit rules on last-position logits (WhisperMoP.generate / beam_search / sample with logit_rules; inference only).
 * (Added under version 118: new exports only; callers detect it with mopk_logit_rules_supported.)  Row r (0 <= r < R) reads x at
 * logits + r * logits_ld elements and writes out + r * out_ld (F32 or BF16, element-aligned); every written entry is the input's
 * bits or -inf ("blocked").  g = hist[r * hist_ld + T0 ...] holds the n = clamp(*pos - T0, 0, T - T0) tokens generated so far
 * (*pos in device memory: one set of launch arguments serves every decoding step).  In this order:
 *   1. mask[v] & 1: blocked (the never-emit list; callers fold the no-timestamps token in when tb >= 0);
 *   2. n == 0 and mask[v] & 2: blocked (blank / eot at the first generated position);
 *   3. tb >= 0 (timestamp tokens are v >= tb), with last = n >= 1 && g[n-1] >= tb and pen = n < 2 || g[n-2] >= tb:
 *      last && pen: x[tb:] blocked; last && !pen: x[:eos] blocked;
 *      t = the last g[i] >= tb, if any: x[tb:lim] blocked, lim = t when last && !pen, else t + 1 (timestamps never decrease);
 *      n == 0: x[:tb] blocked, and x[tb + max_initial + 1:] when max_initial >= 0;
 *      then, over what is left, in fp32: L = m + logf(sum expf(x[tb:] - m)), m = max x[tb:], M = max x[:tb] (-inf for an empty
 *      side); L > M: x[:tb] blocked.
 * A row that the caller's lists block completely comes out all -inf: no guard.  One workgroup of 1024 threads per row: one wave
 * scans g, one streaming pass merges (m, sum, M) in a fixed order, one writes the result; bitwise reproducible, no workspace, no
 * host synchronisation.  out may be logits (the same rows); any other overlap is undefined. */
typedef struct MopkLogitRulesArgs {
    int32_t R;                           /* rows */
    int32_t V;                           /* vocabulary, >= 2 */
    int32_t dtype;                       /* MopkDtype of logits and out: F32 or BF16 */
    int32_t T;                           /* columns of hist (g is never read past them) */
    int32_t T0;                          /* first generated column, 0 <= T0 <= T */
    int32_t tb;                          /* first timestamp token, or -1: rule 3 off */
    int32_t eos;                         /* 0 <= eos < tb when tb >= 0 (unused otherwise) */
    int32_t max_initial;                 /* max_initial_timestamp_index, or -1: off */
    const void *logits;
    int64_t logits_ld;                   /* element stride between rows, >= V */
    void *out;
    int64_t out_ld;                      /* >= V */
    const int32_t *hist;                 /* device (R rows of T) int32 */
    int64_t hist_ld;                     /* element stride between hist rows, >= T */
    const int32_t *pos;                  /* device: one int32 */
    const uint8_t *mask;                 /* device (V): bit 0 rule 1, bit 1 rule 2 */
} MopkLogitRulesArgs;
int mopk_logit_rules_supported(const MopkLogitRulesArgs *a);         /* 1 if the kernel takes this call (V, dtype, strides, ids) */
int mopk_logit_rules(const MopkLogitRulesArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Token-level timestamps (WhisperMoP.align_tokens; inference only): Whisper's alignment filter and its dynamic time warping.
 * (Added under version 118: new exports only; callers detect them with the _supported queries.)
 *
 * mopk_alignment_cost: probs (B, S, N, M) fp32, the cross-attention probabilities of S heads (rows: tokens, columns: audio frames),
 * element (b, s, i, j) at probs + b * probs_sb + s * probs_ss + i * probs_sn + j.  nt = clamp(n_tokens[b], 0, N), nf =
 * clamp(n_frames[b], 0, M): item b uses the rows i < nt and the columns j < nf only; nothing else is loaded.  Per head and column:
 * mu = sum_i p / nt, sd = sqrt(sum_i (p - mu)^2 / nt) (two passes, fp32), z = (p - mu) / sd (no guard for sd = 0); z is
 * median-filtered along j over `width` columns, reflect-padded by width / 2 inside the item's own nf columns (skipped when
 * nf <= width / 2); cost[b, i, j] = -(sum_s filtered) / S, heads added in index order.  cost outside the window is not written.
 * One workgroup of 1024 threads per (column tile, item) keeps one head's slab in LDS; no atomics, fixed reduction orders: bitwise
 * reproducible.  Takes odd width <= 9 and N <= 1024.
 *
 * mopk_dtw_align: Whisper's dtw_cpu over rows [row0, clamp(n_rows[b], 0, N)) and columns [0, clamp(n_cols[b], 0, M)) of cost
 * (B, N, M) fp32 (element (b, i, j) at cost + b * cost_sb + i * cost_ld + j).  1-based with a +inf border and D[0,0] = 0:
 * c0 = D[i-1,j-1], c1 = D[i-1,j], c2 = D[i,j-1]; c0 < c1 && c0 < c2: step 0 (diagonal); else c1 < c0 && c1 < c2: step 1 (up); else
 * step 2 (left); D[i,j] = x[i-1,j-1] + c, one fp32 add.  The path is walked back from the last cell (the first row goes left to
 * column 0 and the first column up to the first row, which is what the rules give for finite costs).  starts[b, i] / ends[b, i]
 * (B, N) int32: the first and last column of the path in row i; -1 for rows outside the range and for an item without rows or
 * columns.  One workgroup per item, one thread per row over the anti-diagonals, a step code per cell in the workspace
 * (mopk_dtw_workspace_bytes), the walk back on the device; no host synchronisation.  Takes N - row0 <= 1024. */
typedef struct MopkAlignCostArgs {
    int32_t B, S, N, M;
    int32_t width;                       /* median filter width, odd */
    int32_t reserved;                    /* 0 */
    const float *probs;
    int64_t probs_sb, probs_ss, probs_sn;   /* element strides of item, head and row; unit column stride */
    const int32_t *n_tokens;             /* device (B) */
    const int32_t *n_frames;             /* device (B) */
    float *cost;                         /* (B, N, M) out */
    int64_t cost_sb, cost_ld;            /* element strides of item and row, cost_ld >= M */
} MopkAlignCostArgs;
int mopk_alignment_cost_supported(const MopkAlignCostArgs *a);       /* 1 if the kernel takes this call (N, width, alignment) */
int mopk_alignment_cost(const MopkAlignCostArgs *a, void *stream);

typedef struct MopkDtwArgs {
    int32_t B, N, M;
    int32_t row0;                        /* first row of every item's range, 0 <= row0 < N */
    const float *cost;
    int64_t cost_sb, cost_ld;            /* element strides of item and row, cost_ld >= M */
    const int32_t *n_rows;               /* device (B): the range's end row */
    const int32_t *n_cols;               /* device (B) */
    int32_t *starts;                     /* (B, N) out, contiguous */
    int32_t *ends;                       /* (B, N) out, contiguous */
    void *workspace;                     /* mopk_dtw_workspace_bytes(): one step code per cell */
} MopkDtwArgs;
int mopk_dtw_align_supported(const MopkDtwArgs *a);                  /* 1 if the kernel takes this call (N - row0, alignment) */
size_t mopk_dtw_workspace_bytes(const MopkDtwArgs *a);               /* from B, N, M, row0 alone (no pointer is looked at) */
int mopk_dtw_align(const MopkDtwArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Whisper's segment and seek arithmetic on decoded token rows (WhisperMoP.transcribe; the rules of OpenAI Whisper's
 * transcribe.py).  (Added under version 118: new exports only; callers detect it with mopk_timestamp_segments_supported.)
 * Row r (0 <= r < R) reads tokens + r * tokens_ld + T0 ...: S = T - T0 generated columns.  e = the first column that holds eos
 * (S if none), g = the n = e tokens before it, ts[i] = g[i] >= tb (a timestamp token: tb + i is frame i * f of the window),
 * w = max(window[r], 1).
 *   1. n == 0: no segment, advance = w.
 *   2. single_end = n >= 2 && !ts[n-2] && ts[n-1];  C = { i : 1 <= i < n, ts[i-1] && ts[i] }, ascending.
 *   3. C not empty: the cuts are C, then n if single_end.  With p the cut before (0 at first), cut c closes the segment of the
 *      token columns [T0 + p, T0 + c): start = (g[p] - tb) * f (0 when g[p] is no timestamp: p = 0 only), end = (g[c-1] - tb) * f.
 *      advance = w if single_end, else (g[max C - 1] - tb) * f; the tokens after the last cut are in no segment.
 *   4. C empty: one segment [T0, T0 + n), start = 0, end = w, or (s - tb) * f when a timestamp exists and the last one, s, is
 *      not tb itself; advance = w.
 *   5. advance is clamped into [1, w].
 * starts / ends / tok_begin / tok_end (R, S) int32, contiguous: row r's n_segments[r] segments in order, -1 behind them (written by
 * the same launch).  The products are taken in 32 bits (callers keep (id - tb) * f below 2^31).  One workgroup per row, one
 * thread per generated column: wave ballots and one LDS exchange per block reduction and for the exclusive scan that numbers
 * the cuts; every output word has one writer; integers only, no atomics, no workspace, no host synchronisation.
 * Takes T - T0 <= 1024. */
typedef struct MopkTimestampSegmentsArgs {
    int32_t R;                           /* rows */
    int32_t T;                           /* columns of tokens */
    int32_t T0;                          /* first generated column, 0 <= T0 < T */
    int32_t tb;                          /* first timestamp token */
    int32_t eos;                         /* 0 <= eos < tb */
    int32_t f;                           /* frames per timestamp step, >= 1 */
    const int32_t *tokens;               /* device (R rows of T) int32 */
    int64_t tokens_ld;                   /* element stride between rows, >= T */
    const int32_t *window;               /* device (R): frames of row r's window */
    int32_t *starts, *ends;              /* (R, T - T0) out: frames relative to the window start */
    int32_t *tok_begin, *tok_end;        /* (R, T - T0) out: columns of tokens, the end exclusive */
    int32_t *n_segments;                 /* (R) out */
    int32_t *advance;                    /* (R) out: frames to move the window by, in [1, w] */
} MopkTimestampSegmentsArgs;
int mopk_timestamp_segments_supported(const MopkTimestampSegmentsArgs *a);   /* 1 if the kernel takes this call (T - T0, alignment) */
int mopk_timestamp_segments(const MopkTimestampSegmentsArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Conditioning a window on the previous text (WhisperMoP.transcribe with condition_on_previous_text / initial_prompt; Whisper's
 * all_tokens[prompt_reset_since:] and its n_ctx // 2 - 1 cap).  (Added under version 118: new exports only; callers detect them
 * with the _supported queries.)  The state: hist (B, n) int32, contiguous, and hist_len (B) int32: hist[b, :hist_len[b]] holds
 * the last tokens of clip b's transcript since its last reset, n is the cap.  Everywhere L = hist_len[b] clamped into [0, n].
 *
 * mopk_prompt_history_update, in place.  Row a (0 <= a < A) reads tokens + a * tokens_ld + T0 ...; b = item[a]; a row with b outside
 * [0, B) is skipped.  m = n_take[a] clamped into [0, T - T0].
 *   mode[a] == 0: c = hist[b, :L] followed by tokens[a, T0 : T0 + m];  keep = min(n, L + m);  hist[b, :keep] = the last keep
 *                 entries of c;  hist_len[b] = keep.  hist[b, keep:] is left as it is.
 *   mode[a] == 1: hist_len[b] = 0 (hist is left as it is).
 *   any other value: clip b is left untouched.
 * The item values of one call must be distinct (two rows of one clip race; every access stays inside the buffers).  One workgroup
 * per row, one thread per history entry: thread j reads the entry that ends up at hist[b, j] into a register, a barrier follows
 * the last read, then every thread writes (the shift is in place).  Takes n <= 1024 and T - T0 <= 1024.
 *
 * mopk_window_prompts builds the left-padded prompt matrix ids (A, width) and kv_start (A) of a set of windows.  Row a: b = item[a]
 * (outside [0, B): the row has no history and reads the sot row of the nearest clip), room = width - Ts,
 *   h = min(L, room - 1) if L > 0 and room >= 2, else 0;   length = Ts + (h > 0 ? 1 + h : 0);   kv_start[a] = width - length;
 *   ids[a] = kv_start[a] zeros, then prev and hist[b, L - h : L] when h > 0, then the Ts tokens sot + b * sot_ld ...
 * (sot_ld == 0: one sot sequence for every clip).  One workgroup per row strides over the columns; thread 0 writes kv_start.
 * Takes width <= 2048.
 * Both: integers only, every word has one writer, no atomics, no workspace, no host synchronisation. */
typedef struct MopkPromptHistoryArgs {
    int32_t A;                           /* rows of tokens */
    int32_t B;                           /* clips */
    int32_t n;                           /* history cap, >= 1 */
    int32_t T;                           /* columns of tokens */
    int32_t T0;                          /* first generated column, 0 <= T0 < T */
    int32_t reserved;
    int32_t *hist;                       /* device (B, n) int32, contiguous, in place */
    int32_t *hist_len;                   /* device (B), in place */
    const int32_t *tokens;               /* device (A rows of T) int32 */
    int64_t tokens_ld;                   /* element stride between rows, >= T */
    const int32_t *n_take;               /* device (A): tokens of row a that join the history */
    const int32_t *item;                 /* device (A): the clip of row a, distinct */
    const int32_t *mode;                 /* device (A): 0 append, 1 reset, else leave */
} MopkPromptHistoryArgs;
int mopk_prompt_history_update_supported(const MopkPromptHistoryArgs *a);    /* 1 if the kernel takes this call (n, T - T0, alignment) */
int mopk_prompt_history_update(const MopkPromptHistoryArgs *a, void *stream);

typedef struct MopkWindowPromptsArgs {
    int32_t A;                           /* rows of ids */
    int32_t B;                           /* clips */
    int32_t n;                           /* history cap, >= 1 */
    int32_t width;                       /* columns of ids, >= Ts */
    int32_t Ts;                          /* tokens of the sot sequence, >= 1 */
    int32_t prev;                        /* the token in front of the history (Whisper's sot_prev) */
    int32_t out_i64;                     /* ids holds int64 (1) or int32 (0) */
    int32_t sot_i64;                     /* sot holds int64 (1) or int32 (0) */
    const int32_t *hist;                 /* device (B, n) int32, contiguous */
    const int32_t *hist_len;             /* device (B) */
    const int32_t *item;                 /* device (A): the clip of row a */
    const void *sot;                     /* device (Ts), or (B rows of Ts) with sot_ld */
    int64_t sot_ld;                      /* element stride between the clips' sot rows, >= Ts, or 0: one row for all */
    void *ids;                           /* (A, width) out, contiguous */
    int32_t *kv_start;                   /* (A) out */
} MopkWindowPromptsArgs;
int mopk_window_prompts_supported(const MopkWindowPromptsArgs *a);           /* 1 if the kernel takes this call (width, alignment) */
int mopk_window_prompts(const MopkWindowPromptsArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Word timestamps (WhisperMoP.align_words and transcribe(word_timestamps=True); Whisper's find_alignment and add_word_timestamps
 * with the tokenizer's part as a table over the vocabulary).  (Added under version 118: new exports only; callers detect them with
 * the _supported queries.)
 *
 * mopk_alignment_rows turns decoded window rows into the inputs of the alignment pass.  Row r reads g[j] = tokens[r, T0 + j],
 * S = T - T0 generated columns, m = n_take[r] clamped into [0, S]; the text tokens are the g[j] < eos with j < m, in order, n_text
 * of them.  W = Tp + 2 + S.
 *   ids[r]      = the Tp tokens sot + r * sot_ld ... (sot_ld == 0: one sequence for every row), nots, the text tokens, then eos to
 *                 the end of the row (at least once);
 *   n_tokens[r] = Tp + 2 + n_text;
 *   col[r, i]   = T0 + j of text token i for i < n_text, else -1 (W columns).
 * One workgroup per row, one thread per generated column: a stable compaction by wave ballots and one LDS exchange of the waves'
 * counts; the block then strides over what the compaction did not write.  Takes S <= 1024.
 *
 * mopk_word_spans groups a row of text tokens into words and times them.  Row r: n = n_text[r] clamped into [0, N]; c_i =
 * table[tokens[r, i] clamped into [0, V)] (bit 0 begins a word, bit 1 prepend punctuation, bit 2 append punctuation, bit 3 sentence
 * end); times[r, i] is the frame at which token i begins and times[r, n] the closing frame.
 *   1. token i begins a word when i == 0 or c_i & 1; word k covers [o_k, o_{k+1}), o_K = n; s_k = times[o_k], e_k = times[o_{k+1}],
 *      p_k = the fp32 mean of its tokens' probabilities (summed in token order); P_k / A_k / E_k: the word has exactly one token and
 *      that token has bit 1 / 2 / 3.
 *   2. d_k = e_k - s_k; m2 = twice the median of the d_k != 0 (odd count: twice the middle value; even: the sum of the two middle
 *      values; none: 0); max_dur = m2, or min(m2, 2 * median_cap) with median_cap >= 0.
 *   3. k >= 1 with d_k > max_dur: E_k: e_k = s_k + max_dur; else E_{k-1}: s_k = e_k - max_dur (original values on the right).
 *   4. pass 1: a word with P_k and k < K - 1 dies; its tokens go in front of the nearest later word that does not die here.
 *   5. pass 2: a word k >= 1 that survived pass 1, has A_k and received nothing in pass 1 dies when word k - 1 survived pass 1; its
 *      tokens go to the back of the nearest earlier word that survives both passes (one exists then).
 *   6. the survivors, in order, keep their own s, e, p; their token ranges [tok_begin, tok_end) are the unions with what they
 *      absorbed, contiguous, a partition of [0, n).  starts / ends / tok_begin / tok_end (R, N) int32 and probs (R, N) fp32,
 *      contiguous; behind the n_words[r] survivors the integers are -1 and probs 0 (written by the same launch).
 * One workgroup per row, one thread per token and then per word: the word and the survivor numbering are ballot scans with one LDS
 * exchange each, the per-word values live in LDS, and for the median every word ranks its own duration against the others (ties to
 * the smaller index).  Takes N <= 1024.
 * Both: every output word has one writer, no atomics, no workspace, no host synchronisation. */
typedef struct MopkAlignmentRowsArgs {
    int32_t R;                           /* rows */
    int32_t T;                           /* columns of tokens */
    int32_t T0;                          /* first generated column, 0 <= T0 < T */
    int32_t Tp;                          /* tokens of the sot sequence, >= 1 */
    int32_t nots;                        /* the token behind the sot sequence (Whisper's <|notimestamps|>) */
    int32_t eos;                         /* text tokens are below it; it closes and pads the row */
    int32_t out_i64;                     /* ids holds int64 (1) or int32 (0) */
    int32_t sot_i64;                     /* sot holds int64 (1) or int32 (0) */
    const int32_t *tokens;               /* device (R rows of T) int32 */
    int64_t tokens_ld;                   /* element stride between rows, >= T */
    const int32_t *n_take;               /* device (R): generated tokens of row r that are inside its segments */
    const void *sot;                     /* device (Tp), or (R rows of Tp) with sot_ld */
    int64_t sot_ld;                      /* element stride between the rows' sot sequences, >= Tp, or 0: one for all */
    void *ids;                           /* (R, Tp + 2 + T - T0) out, contiguous */
    int32_t *n_tokens;                   /* (R) out */
    int32_t *col;                        /* (R, Tp + 2 + T - T0) out, contiguous */
} MopkAlignmentRowsArgs;
int mopk_alignment_rows_supported(const MopkAlignmentRowsArgs *a);           /* 1 if the kernel takes this call (T - T0, alignment) */
int mopk_alignment_rows(const MopkAlignmentRowsArgs *a, void *stream);

typedef struct MopkWordSpansArgs {
    int32_t R;                           /* rows */
    int32_t N;                           /* text tokens per row */
    int32_t V;                           /* entries of table */
    int32_t median_cap;                  /* frames, >= 0, or -1: no cap */
    const int32_t *tokens;               /* device (R rows of N) int32 */
    int64_t tokens_ld;                   /* element stride between rows, >= N */
    const int32_t *times;                /* device (R rows of N + 1) int32 */
    int64_t times_ld;                    /* element stride between rows, >= N + 1 */
    const float *probs;                  /* device (R rows of N) fp32 */
    int64_t probs_ld;                    /* element stride between rows, >= N */
    const int32_t *n_text;               /* device (R) */
    const uint8_t *table;                /* device (V) */
    int32_t *starts, *ends;              /* (R, N) out: frames */
    float *out_probs;                    /* (R, N) out */
    int32_t *tok_begin, *tok_end;        /* (R, N) out: indices into the row's text tokens, the end exclusive */
    int32_t *n_words;                    /* (R) out */
} MopkWordSpansArgs;
int mopk_word_spans_supported(const MopkWordSpansArgs *a);                   /* 1 if the kernel takes this call (N, alignment) */
int mopk_word_spans(const MopkWordSpansArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Whisper's log-mel spectrogram of a batch of waveforms (audio.py's log_mel_spectrogram; the stage in front of the encoder).
 * (Added under version 118: new exports only; callers detect it with mopk_log_mel_supported.)
 * Clip b holds len_b = min(lens[b], L) samples (L without lens) and T_b = len_b / hop frames; T = L / hop rows are written.
 * Frame t covers the samples [t * hop - n_fft/2, t * hop + n_fft/2) of the clip reflected at ITS OWN two ends (index -i reads i,
 * index len_b - 1 + i reads len_b - 1 - i).  With w the periodic Hann window and F the filters:
 *   P[t,k] = | sum_n w[n] * frame_t[n] * e^{-2 pi i n k / n_fft} |^2, k = 0 .. n_fft/2;   M[t,m] = sum_k F[m,k] * P[t,k];
 *   G = log10(max(M, 1e-10));   G = max(G, max over the clip's own t < T_b and all m of G, minus 8);   out = (G + 4) / 4.
 * Rows t >= T_b of out are written as zeros by the same call.  All arithmetic is fp32.
 * Two launches.  (1) One workgroup per (tile of MOPK_LOG_MEL_TILE_FRAMES frames, clip): the windowed frames and the twiddles
 * sit in LDS, the DFT is a (32 x n_fft) . (n_fft x 2 . 32) product per 32 bins on the f32-input MFMA (twiddle n * k mod n_fft:
 * an exact integer index into the table), the power and the filterbank product stay in LDS and registers, G goes to out (fp32)
 * or to the workspace (bf16 out), and the tile's maximum to one workspace word of its own.  (2) Every workgroup reduces its
 * clip's tile maxima in a fixed order (no atomics: bit-repeatable), clamps, scales and writes the zero tail.
 * No host synchronisation.  The first call raises the kernel's LDS limit (not inside a stream capture: run once before).
 * Takes n_fft even in [16, 512], 1 <= hop <= n_fft, 1 <= n_mels <= 128, L >= max(hop, n_fft/2 + 1), B <= 65535.  A device
 * length below n_fft/2 + 1 cannot be refused here: such a clip reads zeros where the reflection leaves it (never out of bounds). */
#define MOPK_LOG_MEL_TILE_FRAMES 32
#define MOPK_LOG_MEL_F16 2               /* audio_dtype only: IEEE half samples (beside MOPK_F32 and MOPK_BF16) */
typedef struct MopkLogMelArgs {
    int32_t B;                           /* clips */
    int32_t L;                           /* samples per row of audio */
    int32_t n_fft;
    int32_t hop;
    int32_t n_mels;
    int32_t audio_dtype;                 /* MOPK_F32, MOPK_BF16 or MOPK_LOG_MEL_F16 */
    int32_t out_dtype;                   /* MOPK_F32 or MOPK_BF16 */
    int32_t reserved;
    const void *audio;                   /* device (B rows of L), unit inner stride */
    int64_t audio_ld;                    /* element stride between rows, >= L */
    const int32_t *lens;                 /* device (B) sample counts, clamped into [0, L]; NULL: every clip has L */
    const float *filters;                /* device (n_mels, n_fft/2 + 1) fp32, contiguous */
    const int32_t *bands;                /* device (n_mels, 2): filters[m][k] == 0 outside lo <= k < hi; NULL: 0 .. n_fft/2 + 1 */
    const float *twiddle;                /* device (n_fft, 2): cos and sin of 2 pi i / n_fft */
    const float *window;                 /* device (n_fft): 0.5 - 0.5 cos(2 pi n / n_fft) */
    void *out;                           /* (B, L / hop, n_mels) out, contiguous */
    void *workspace;                     /* mopk_log_mel_workspace_bytes() */
} MopkLogMelArgs;
int mopk_log_mel_supported(const MopkLogMelArgs *a);             /* 1 if the kernel takes this call (shape, dtypes, alignment) */
size_t mopk_log_mel_workspace_bytes(const MopkLogMelArgs *a);    /* from the shape and out_dtype alone (no pointer is looked at) */
int mopk_log_mel(const MopkLogMelArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Sample-rate conversion of a batch of waveforms (the stage in front of mopk_log_mel; inference only): the windowed-sinc (Hann)
 * polyphase resampler.  (Added under version 118: new exports only; callers detect it with mopk_resample_supported.)
 * With o / n the reduced input / output rates, K the caller's tap table and w its centre offset, clip b of len_b = min(lens[b], L)
 * samples (L without lens), taken as zero outside [0, len_b), gives len_out_b = ceil(n * len_b / o) samples (64-bit product):
 *   y[f * n + p] = sum_{s < S} K[p][s] * x[f * o + first[p] + s - w],   0 <= p < n,   f * n + p < len_out_b,
 * an fmaf chain in ascending s from 0, fp32.  Row p of K holds the S consecutive taps of phase p that can be non-zero, first[p]
 * is the index of its first tap in the full (n, 2 w + o) table; first[p] is clamped into [0, 2 w + o - S] on the device, so no
 * table content makes the kernel read outside the span it staged.  A sample x[q] is the mean over the C channels, summed in
 * ascending channel order in fp32 and multiplied by the fp32 reciprocal of C, of the converted input: fp32, bf16 and fp16 exactly, int16 times 2^-15.
 * The identity (orig == new) is the table n = o = S = 1, w = 0, K = 1, first = 0.
 * One launch.  A workgroup takes one clip's tile of 1024 consecutive outputs, stages the contiguous input span the tile reads
 * (conversion, channel mean and the [0, len_b) bound applied once, reads outside the bound never issued) and, when span and
 * table fit 64 KiB together, the table into LDS; otherwise the table is read through L2.  Outputs m >= len_out_b of the row are
 * written as zeros and out_lens[b] = len_out_b by the same launch.  A sample depends on its own clip only: bit-identical to the
 * clip run alone.  No workspace, no host synchronisation, no raised LDS limit (capturable without a warm-up).
 * Takes 1 <= B <= 65535, 1 <= C <= 64, 1 <= S <= 2 w + o, S <= table_ld, n * table_ld <= 2^22, Lout = ceil(n * L / o) < 2^31
 * and a span ((1024 + n - 2) / n) * o + 2 w + o <= 12288 samples (o / n up to 11 at the default filter width). */
typedef struct MopkResampleArgs {
    int32_t B;                           /* clips */
    int32_t C;                           /* channels, averaged */
    int32_t L;                           /* samples per channel and row of audio */
    int32_t Lout;                        /* samples per row of out: ceil(n * L / o) */
    int32_t o, n;                        /* input / output rate over their gcd */
    int32_t w;                           /* centre offset of the tap table */
    int32_t S;                           /* taps per phase */
    int32_t table_ld;                    /* element stride between rows of table, >= S (odd: conflict-free in LDS) */
    int32_t audio_dtype;                 /* MOPK_F32, MOPK_BF16, MOPK_LOG_MEL_F16 (IEEE half) or 3: int16 */
    int32_t out_dtype;                   /* MOPK_F32 or MOPK_BF16 (one rounding of the fp32 result) */
    int32_t reserved;
    const void *audio;                   /* device; sample (b, c, q) at audio + b * audio_sb + c * audio_sc + q * audio_sl elements */
    int64_t audio_sb, audio_sc, audio_sl;
    const int32_t *lens;                 /* device (B) sample counts, clamped into [0, L]; NULL: every clip has L */
    const float *table;                  /* device (n, table_ld) fp32, contiguous; columns >= S are copied along and never used */
    const int32_t *first;                /* device (n) */
    void *out;                           /* (B, Lout) out, contiguous */
    int32_t *out_lens;                   /* (B) out, or NULL */
} MopkResampleArgs;
int mopk_resample_supported(const MopkResampleArgs *a);          /* 1 if the kernel takes this call (shape, dtypes, alignment) */
int mopk_resample(const MopkResampleArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Per-step decoding statistics on last-position logits (WhisperMoP.generate / beam_search / sample with return_stats, and the
 * temperature fallback and no-speech skip of WhisperMoP.transcribe; inference only).  (Added under version 118: new exports only;
 * callers detect them with the _supported queries.)  Row r (0 <= r < R) reads x at logits + r * logits_ld elements, F32 or BF16,
 * element-aligned, finite or -inf values; lse = m + logf(sum expf(x - m)), m = max x, in fp32 (-inf entries add nothing).  A row
 * without a finite entry is outside the contract: nothing faults, its results are unspecified.
 *
 * mopk_token_logprob: out[r] = (float)x[t] - lse, t = tokens[r], or `token` for every row when tokens is NULL; t is clamped into
 * [0, V) (callers refuse what they can see).  x[t] = -inf gives -inf.
 *
 * mopk_greedy_pick: one greedy decoding step (Whisper's GreedyDecoder.update) on device state, in place.  p = *pos.
 *   eos >= 0 and done[r] != 0:  t = eos; sum_logprobs, n_tokens and done are left as they are;
 *   else:  t = argmax_v x_v, ties to the smaller v;  sum_logprobs[r] += x[t] - lse;  n_tokens[r] += 1;  done[r] |= (t == eos).
 *   next_ids[r] = t;  hist[r * hist_ld + p] = t when hist is given and 0 <= p < hist_cap.
 * The first eos is counted in the sum and in the length, nothing behind it: sum_logprobs / n_tokens is Whisper's avg_logprob.
 *
 * Both: one workgroup of 1024 threads per row, one pass over the row in 16-byte loads (scalar elements before the row's first
 * 16-byte boundary and behind its last whole vector), the (max, sum-exp) pairs and the best (value, index) merged by wave shuffles
 * and then in wave order; static LDS only, no atomics, no workspace, no host synchronisation: bitwise reproducible, and a first
 * call may be inside a stream capture. */
typedef struct MopkTokenLogprobArgs {
    int32_t R;                           /* rows */
    int32_t V;                           /* vocabulary, >= 2 */
    int32_t dtype;                       /* MopkDtype of logits: F32 or BF16 */
    int32_t token;                       /* the token of every row when tokens is NULL */
    const void *logits;
    int64_t logits_ld;                   /* element stride between rows, >= V */
    const int32_t *tokens;               /* device (R) int32, contiguous, or NULL */
    float *out;                          /* (R) out */
} MopkTokenLogprobArgs;
int mopk_token_logprob_supported(const MopkTokenLogprobArgs *a);     /* 1 if the kernel takes this call (V, dtype, stride, alignment) */
int mopk_token_logprob(const MopkTokenLogprobArgs *a, void *stream);

typedef struct MopkGreedyPickArgs {
    int32_t R;                           /* rows */
    int32_t V;                           /* vocabulary, >= 2 */
    int32_t dtype;                       /* MopkDtype of logits: F32 or BF16 */
    int32_t eos;                         /* eos token id, or -1: no eos */
    int32_t hist_cap;                    /* columns of hist (0 without hist) */
    int32_t reserved;                    /* 0 */
    const void *logits;
    int64_t logits_ld;                   /* element stride between rows, >= V */
    const int32_t *pos;                  /* device: the new token's history column (one int32) */
    int32_t *next_ids;                   /* (R) out: the next decoder step's ids */
    int32_t *done;                       /* (R) in / out */
    float *sum_logprobs;                 /* (R) in / out */
    int32_t *n_tokens;                   /* (R) in / out */
    int32_t *hist;                       /* (R rows of hist_cap) in / out, or NULL */
    int64_t hist_ld;                     /* element stride between hist rows, >= hist_cap */
} MopkGreedyPickArgs;
int mopk_greedy_pick_supported(const MopkGreedyPickArgs *a);         /* 1 if the kernel takes this call (V, dtype, strides, alignment) */
int mopk_greedy_pick(const MopkGreedyPickArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Repetition penalty and no-repeat n-gram blocking on last-position logits (WhisperMoP decoding with repeat rules; inference
 * only).  (Added under version 118: new exports only; callers detect it with mopk_repeat_rules_supported.)  The conventions are
 * mopk_logit_rules': row r (0 <= r < R) reads x at logits + r * logits_ld elements and writes out + r * out_ld (F32 or BF16,
 * element-aligned); g = hist[r * hist_ld + T0 ...] holds the n = clamp(*pos - T0, 0, T - T0) tokens generated so far (*pos in
 * device memory: one set of launch arguments serves every decoding step).  Tokens before T0 (the prompt) never count.  In this
 * order:
 *   0. out[v] = x[v], bit for bit;
 *   1. penalty != 1: every distinct v in g with 0 <= v < V and exempt[v] == 0 gets, in fp32, f = (float)x[v],
 *      out[v] = f < 0 ? f * penalty : f * inv_penalty, rounded to the dtype (BF16: to nearest even).
 *      -inf stays -inf and NaN stays NaN.  inv_penalty is the caller's fp32 1 / penalty: the product may differ from a true quotient by one ulp;
 *   2. ngram = s >= 1 and n >= s - 1: for every i in [0, n - s] with g[i : i + s - 1] == g[n - s + 1 : n] (raw int32 values),
 *      v = g[i + s - 1]; 0 <= v < V and exempt[v] == 0: out[v] = -inf, whether or not step 1 touched it.
 * Every other entry of out is the input's bits; a row that the rules block completely comes out all -inf: no guard.
 * One workgroup of 1024 threads per row, one launch; g is staged in LDS once (T - T0 <= 4096).  out == logits (the same rows):
 * the kernel touches only the entries that it changes; every x[g[i]] is read before a barrier and written after it, so duplicate
 * tokens write equal values, and the bans are written behind a second barrier.  Any other overlap is undefined.  Bitwise
 * reproducible, no workspace, no host synchronisation. */
typedef struct MopkRepeatRulesArgs {
    int32_t R;                           /* rows */
    int32_t V;                           /* vocabulary, >= 2 */
    int32_t dtype;                       /* MopkDtype of logits and out: F32 or BF16 */
    int32_t T;                           /* columns of hist (g is never read past them) */
    int32_t T0;                          /* first generated column, 0 <= T0 <= T, T - T0 <= 4096 */
    int32_t ngram;                       /* no_repeat_ngram_size, >= 0 (0: off) */
    float penalty;                       /* repetition_penalty, finite and > 0 (1: off) */
    float inv_penalty;                   /* the caller's fp32 1 / penalty */
    const void *logits;
    int64_t logits_ld;                   /* element stride between rows, >= V */
    void *out;
    int64_t out_ld;                      /* >= V */
    const int32_t *hist;                 /* device (R rows of T) int32 */
    int64_t hist_ld;                     /* element stride between hist rows, >= T */
    const int32_t *pos;                  /* device: one int32 */
    const uint8_t *exempt;               /* device (V): non-zero entries are never penalised or banned */
} MopkRepeatRulesArgs;
int mopk_repeat_rules_supported(const MopkRepeatRulesArgs *a);       /* 1 if the kernel takes this call (V, dtype, strides, T - T0) */
int mopk_repeat_rules(const MopkRepeatRulesArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Language probabilities on last-position logits (WhisperMoP.detect_language, and transcribe with `languages`; inference only):
 * Whisper's detect_language after the decoder pass.  (Added under version 118: new exports only; callers detect it with
 * mopk_language_probs_supported.)  Row r (0 <= r < R) reads x_i = (float)logits[r * logits_ld + ids[i]], 0 <= i < n, F32 or BF16,
 * element-aligned, finite or -inf values; each ids[i] is clamped into [0, V) before the read, so no read leaves the row (callers
 * refuse what they can see).  In fp32:
 *   lse = m + logf(sum_i expf(x_i - m)), m = max_i x_i (-inf entries add nothing);
 *   probs[r * probs_ld + i] = expf(x_i - lse), which is 0 for x_i = -inf;
 *   tokens[r] = ids[i*], i* the largest x_i, ties to the smaller token id (what an argmax over the masked vocabulary gives).
 * A row without a finite language entry is outside the contract: nothing faults, its values are unspecified.  Entries of probs
 * behind column n of a row are not written.
 * One launch, one workgroup of 256 threads per row; a thread gathers up to four entries and keeps them in registers, the
 * (max, sum-exp) pairs and the best (value, id) are merged by wave shuffles and then in wave order; static LDS only, no atomics,
 * no workspace, no host synchronisation: bitwise reproducible, and a first call may be inside a stream capture. */
#define MOPK_LANGUAGE_MAX_N 1024
typedef struct MopkLanguageProbsArgs {
    int32_t R;                           /* rows */
    int32_t V;                           /* vocabulary, >= 2 */
    int32_t dtype;                       /* MopkDtype of logits: F32 or BF16 */
    int32_t n;                           /* languages, 1 <= n <= MOPK_LANGUAGE_MAX_N */
    const void *logits;
    int64_t logits_ld;                   /* element stride between rows, >= V */
    const int32_t *ids;                  /* device (n) int32, contiguous: the language tokens */
    float *probs;                        /* (R, n) out */
    int64_t probs_ld;                    /* element stride between probs rows, >= n */
    int32_t *tokens;                     /* (R) out: the most probable language token of each row */
} MopkLanguageProbsArgs;
int mopk_language_probs_supported(const MopkLanguageProbsArgs *a);   /* 1 if the kernel takes this call (V, n, dtype, strides, alignment) */
int mopk_language_probs(const MopkLanguageProbsArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * The MoP mel gate of every WhisperMoP encoder layer (mop/models/whisper_mop.py:91-124 MoP2D), all layers in one launch.  (Added
 * under version 118: new exports only; callers detect it with mopk_mel_gate_supported.)
 * MoP2D (1x1 conv -> kxk conv -> cat -> 1x1 conv -> mean over frequency -> 1 + a0 g0 - a1 g1) has no bias and no non-linearity,
 * so it folds (mop_amd/ops.py mel_gate_taps, in torch) into a 1-D stencil over time with F input channels, p = k / 2:
 *     gates[b,l,t] = 1 + sum_{i<k} sum_{f<F} mel[b, t+i-p, f] W[l,i,f]       (frames outside [0, T) are zero).
 * With lens (device int32 (B)): rows t >= lens[b] of mel are NOT READ and count as zeros, gates[b,l,t >= lens[b]] = 1 exactly.
 *   _fwd: a workgroup stages MOPK_MEL_GATE_TILE frames plus the 2p halo of one item in LDS once (converted to fp32) and writes
 *         every layer's gate of the tile from it; the taps sit in LDS too, and more than MOPK_MEL_GATE_LAYERS layers go in
 *         chunks of that many (one launch per chunk).  Each gate is one fp32 sum in a fixed order (i outer, f inner) that does
 *         not depend on T or B, so a clip's columns are bitwise those of the clip alone.
 *   _bwd: dW[l,i,f] = sum_{b,t < lens[b]} dgates[b,l,t] mel[b,t+i-p,f].  Workgroup j sums the tiles j, j + P, ... (P =
 *         min(tiles, 256)) into registers and writes one partial row of `workspace`; a second launch sums the P rows in a fixed
 *         order.  No atomics: bitwise reproducible.  No gradient of mel.
 * mel: element strides (mel_sb, mel_st), innermost contiguous, element-aligned (16-byte aligned rows take vector loads, others
 * scalar loads).  W, gates, dgates, dW: contiguous fp32.  Odd k <= 7, F <= 128, any B, T, L >= 1. */
#define MOPK_MEL_GATE_TILE 32
#define MOPK_MEL_GATE_LAYERS 8
#define MOPK_MEL_GATE_MAX_K 7
#define MOPK_MEL_GATE_MAX_F 128
typedef struct MopkMelGateArgs {
    int32_t B, T, F, L, k;
    int32_t mel_dtype;                   /* MopkDtype: F32 or BF16 */
    const void *mel;                     /* (B,T,F) */
    int64_t mel_sb, mel_st;              /* element strides, mel_st >= F */
    const float *W;                      /* (L,k,F) fp32 contiguous */
    const int32_t *lens;                 /* device (B) int32 or NULL; values are clamped into [0, T] */
    float *gates;                        /* fwd out (B,L,T) fp32 contiguous */
    const float *dgates;                 /* bwd in  (B,L,T) fp32 contiguous */
    float *dW;                           /* bwd out (L,k,F) fp32 contiguous */
    void *workspace;                     /* bwd: mopk_mel_gate_workspace_bytes() */
} MopkMelGateArgs;
int mopk_mel_gate_supported(const MopkMelGateArgs *a);                /* 1 if the kernels take this call (shape, dtype, strides, alignment) */
size_t mopk_mel_gate_workspace_bytes(const MopkMelGateArgs *a);
int mopk_mel_gate_fwd(const MopkMelGateArgs *a, void *stream);
int mopk_mel_gate_bwd(const MopkMelGateArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Residual add and per-token gate of the WhisperMoP encoder block in one launch.  (Added under version 118: new exports only;
 * callers detect it with mopk_gated_residual_supported.)
 *   _fwd: out[b,t,:] = (x[b,t,:] + a[b,t,:]) gate[b,t].
 *   _bwd: dr[b,t,:] = dout[b,t,:] gate[b,t] (the gradient of both x and a), dgate[b,t] = sum_d dout[b,t,d] (x + a)[b,t,d] with
 *         r recomputed from x and a.  One wave owns a row and reduces it by shuffles: no atomics, bitwise reproducible.
 * x / a: (B,T,D) with element strides (sb, st), innermost contiguous.  gate: (B,T) fp32 with batch stride gate_sb, t contiguous.
 * o_dtype must be the promotion of x_dtype and a_dtype.  out / dout / dr: contiguous (B,T,D) o_dtype; dgate contiguous (B,T) fp32.
 * D % 8 == 0, strides multiples of 8, 16-byte aligned x / a / out / dout / dr; no workspace. */
typedef struct MopkGatedResidualArgs {
    int32_t B, T, D;
    int32_t x_dtype, a_dtype, o_dtype;   /* MopkDtype */
    const void *x;
    int64_t x_sb, x_st;
    const void *a;
    int64_t a_sb, a_st;
    const float *gate;                   /* (B,T) fp32 */
    int64_t gate_sb;                     /* element stride between the gate's rows, >= T */
    void *out;                           /* fwd out */
    const void *dout;                    /* bwd in */
    void *dr;                            /* bwd out */
    float *dgate;                        /* bwd out (B,T) fp32 */
} MopkGatedResidualArgs;
int mopk_gated_residual_supported(const MopkGatedResidualArgs *a);    /* 1 if the kernels take this call (shape, dtypes, strides, alignment) */
size_t mopk_gated_residual_workspace_bytes(const MopkGatedResidualArgs *a);   /* 0: the kernels need none */
int mopk_gated_residual_fwd(const MopkGatedResidualArgs *a, void *stream);
int mopk_gated_residual_bwd(const MopkGatedResidualArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Cross-entropy of rows of logits against int64 class targets (ops.cross_entropy, ops.linear_cross_entropy, the language models'
 * loss()).  (Added under version 118: new exports only; callers detect them with mopk_cross_entropy_supported.)
 *
 * A call holds R rows of a problem of n_rows rows: launch row r (0 <= r < R) is problem row row0 + r.  logits / dlogits are indexed
 * by the launch row (row r at logits + r * logits_ld elements, F32 or BF16, element-aligned, unit inner stride); targets, lse,
 * row_loss and grad by the problem row.  A whole problem in one call has row0 = 0, n_rows = R; a caller that holds only a chunk of
 * the logits at a time (ops.linear_cross_entropy) walks row0 and keeps the per-row arrays whole.
 *
 * A row is IGNORED when its target t is ignore_index or lies outside [0, V) (torch asserts on the device for the latter): its loss
 * is 0, its gradient is 0, it is not counted.  No read leaves a row for any target value.
 *
 * _fwd: lse[row] = m + logf(sum expf(x - m)), m = max x, in fp32 (-inf entries add nothing; a row without a finite entry is
 *   outside the contract);  row_loss[row] = lse - x[t], 0 for an ignored row.  With `out`, a second launch (one workgroup) follows:
 *   out[0] = sum of row_loss over the counted rows of [0, n_rows), accumulated in double in a fixed order;  out[1] = n_valid, their
 *   number;  out[2] = sum / n_valid (NaN when no row counts);  out[3] = 1 / n_valid.  The sum reads row_loss of EVERY problem row:
 *   the call with `out` is the last of a chunked problem.
 * _bwd: dlogits[r, j] = g (expf(x_j - lse[row]) - [j == t]) in the logits' dtype, g = grad[row * grad_stride] (grad_stride 0: one
 *   upstream scalar), times *scale when scale is given (out + 3 of the forward for a mean).  An ignored row is written as exact
 *   zeros; grad and scale are not read for it.  Columns [V, ld) are not touched.  dlogits may be logits itself (same pointer and
 *   stride); otherwise the two must not overlap, and each row of dlogits must sit as its row of logits does relative to 16 bytes
 *   (pointers equal mod 16, strides equal mod 16 bytes; MOPK_ERR_UNSUPPORTED otherwise).
 *
 * One workgroup of 1024 threads per row; 16-byte loads and stores with scalar elements before a row's first 16-byte boundary and
 * behind its last whole vector; the (max, sum-exp) pairs merged by wave shuffles and then in wave order.  Static LDS only, no float
 * atomics, no workspace, no host synchronisation: bitwise reproducible, and a first call may be inside a stream capture. */
typedef struct MopkCrossEntropyArgs {
    int32_t R;                           /* rows of this call */
    int32_t V;                           /* classes, >= 2 */
    int32_t dtype;                       /* MopkDtype of logits and dlogits: F32 or BF16 */
    int32_t row0;                        /* problem row of launch row 0, >= 0 */
    int32_t n_rows;                      /* rows of the problem, >= row0 + R */
    int32_t reserved;                    /* 0 */
    int64_t ignore_index;
    const void *logits;
    int64_t logits_ld;                   /* element stride between rows, >= V */
    const int64_t *targets;              /* device (n_rows) int64 */
    float *lse;                          /* (n_rows): fwd out, bwd in */
    float *row_loss;                     /* (n_rows): fwd out */
    float *out;                          /* fwd: (4) out, or NULL: no reduce launch */
    void *dlogits;                       /* bwd out */
    int64_t dlogits_ld;                  /* element stride between its rows, >= V */
    const float *grad;                   /* bwd: upstream gradient, one float or one per problem row */
    int64_t grad_stride;                 /* element stride between its rows, >= 0; 0: one scalar for all */
    const float *scale;                  /* bwd: one float that multiplies grad, or NULL */
} MopkCrossEntropyArgs;
int mopk_cross_entropy_supported(const MopkCrossEntropyArgs *a);      /* 1 if the kernels take this call (V, dtype, strides, alignment) */
int mopk_cross_entropy_fwd(const MopkCrossEntropyArgs *a, void *stream);
int mopk_cross_entropy_bwd(const MopkCrossEntropyArgs *a, void *stream);

/* --------------------------------------------------------------------------
 * Fused AdamW step over a list of tensors (mop_amd.optim.FusedAdamW, ops.adamw_step): global gradient norm, clipping, the update,
 * an optional weight EMA.  (Added under version 118: new exports only; callers detect them with mopk_adamw_supported.)
 *
 * A call takes one MopkAdamWArgs and a HOST array of n_tensors MopkOptimTensor.  The hyper-parameters of a call hold for all its
 * tensors; an optimiser with several parameter groups makes one call with phases = MOPK_ADAMW_NORM over all tensors and one call
 * with phases = MOPK_ADAMW_UPDATE per group.  Per element, in fp32, every product and sum rounded once (no contraction):
 *   g' = coef * g                                     coef = stats.coef when use_norm, else 1;  g itself is never written
 *   p  = p * decay                                    decay = fl(1 - lr * weight_decay)
 *   m  = fl(b1) * m + fl(1 - b1) * g'
 *   v  = fl(b2) * v + (fl(1 - b2) * g') * g'
 *   p  = p - fl(lr / bc1) * (m / (sqrtf(v) / fl(sqrt(bc2)) + fl(eps)))       bc_i = 1 - b_i^(step + 1)
 *   ema = fl(d) * ema + fl(1 - d) * p                 only with use_ema
 * The constants fl(.) are computed in double (lr, the betas, eps, weight_decay and ema_decay travel as doubles; b^(step + 1) by
 * repeated squaring in double, from the tensor's own device step count) and rounded to fp32 once.  With lr_dev, lr is read from
 * that device float.  p, g and ema are F32 or BF16 (p and ema share p_dtype; g_dtype may differ); m and v are always fp32.  A
 * BF16 p or ema is rounded to nearest even once, from the fp32 result.
 *
 * Launches.  The tensors are cut into chunks of MOPK_ADAMW_CHUNK elements (the last chunk of a tensor may be short; an empty
 * tensor has none) and the chunk list into slices that travel as kernel arguments: a slice holds at most MOPK_ADAMW_MAX_TENSORS
 * tensor parts and at most MOPK_ADAMW_MAX_CHUNKS chunks, is filled greedily in tensor order, and a tensor with more chunks than
 * fit continues in the next slice.  With S slices (mopk_adamw_launches; a slice of empty tensors only launches its count kernel):
 *   MOPK_ADAMW_NORM    S launches (one workgroup of 256 threads per chunk: each thread sums the squares of its elements in fp32 in
 *                      index order, the workgroup merges by the wave shuffle tree and then the waves in wave order, one partial per
 *                      chunk goes to the workspace; no atomics) + 1 launch (one workgroup sums the partials in double, thread-
 *                      strided, same merge order; stats.norm = fl(sqrt(sum)), stats.coef = min(1, max_norm / (norm + 1e-6)) when
 *                      clip, else 1 (a NaN norm gives a NaN coef, as torch's clamp does); stats.skip = skip_nonfinite and the norm
 *                      is not finite; stats.skipped += stats.skip)
 *   MOPK_ADAMW_UPDATE  S launches (grid min(chunks of the slice, 2048), grid-stride over chunks) + S launches that add 1 to the
 *                      step counts (stream-ordered behind every update launch: no launch reads a count that it writes).
 * With stats.skip set and use_norm, an update call writes nothing and advances no count.
 * A chunk is read in 16-byte vectors from p's first 16-byte boundary on; the elements before it and behind the last whole vector
 * are handled one by one, and a stream that does not share p's alignment is read or written element by element.
 * No host synchronisation, no host-to-device copy, no allocation: a call may be captured in a HIP graph (the pointers are then
 * fixed; step counts, bias corrections, lr_dev and the stats are read on the device at replay). */
#define MOPK_ADAMW_CHUNK 4096            /* elements per chunk */
#define MOPK_ADAMW_MAX_TENSORS 40        /* tensor parts per launch */
#define MOPK_ADAMW_MAX_CHUNKS 4096       /* chunks per launch */
#define MOPK_ADAMW_NORM 1                /* phases */
#define MOPK_ADAMW_UPDATE 2
typedef struct MopkOptimTensor {
    void *p;                             /* (n) parameter, in / out */
    const void *g;                       /* (n) gradient */
    float *m;                            /* (n) fp32 first moment, in / out */
    float *v;                            /* (n) fp32 second moment, in / out */
    void *ema;                           /* (n) EMA of p in p_dtype, in / out; NULL without use_ema */
    float *step;                         /* device fp32 scalar: steps taken so far, in / out */
    int64_t n;                           /* elements, >= 0; 0: only step is touched, the other pointers may be NULL */
    int32_t p_dtype;                     /* MopkDtype of p and ema */
    int32_t g_dtype;                     /* MopkDtype of g */
} MopkOptimTensor;
typedef struct MopkAdamWStats {         /* 16 device bytes that outlive a call */
    float norm;                          /* total gradient norm before clipping */
    float coef;                          /* clip coefficient */
    int32_t skip;                        /* 1: the step that follows is skipped */
    int32_t skipped;                     /* steps skipped so far */
} MopkAdamWStats;
typedef struct MopkAdamWArgs {
    int32_t n_tensors;
    int32_t phases;                      /* MOPK_ADAMW_NORM | MOPK_ADAMW_UPDATE */
    int32_t clip;                        /* norm: compute the clip coefficient from max_norm */
    int32_t skip_nonfinite;              /* norm: set stats.skip on a non-finite norm */
    int32_t use_norm;                    /* update: read coef and skip from stats (implied by MOPK_ADAMW_NORM in the same call) */
    int32_t use_ema;
    double lr, beta1, beta2, eps, weight_decay, ema_decay, max_norm;
    const float *lr_dev;                 /* device float that replaces lr, or NULL */
    MopkAdamWStats *stats;               /* device; needed by the norm phase and by use_norm */
    float *workspace;                    /* device, mopk_adamw_workspace_bytes; norm phase only */
} MopkAdamWArgs;
int mopk_adamw_supported(const MopkAdamWArgs *a, const MopkOptimTensor *t);   /* 1 if the kernels take this call (dtypes, alignment, counts) */
size_t mopk_adamw_workspace_bytes(const MopkAdamWArgs *a, const MopkOptimTensor *t);   /* one fp32 partial per chunk; reads only n */
int mopk_adamw_launches(const MopkAdamWArgs *a, const MopkOptimTensor *t);    /* kernel launches mopk_adamw_step makes for this call */
int mopk_adamw_step(const MopkAdamWArgs *a, const MopkOptimTensor *t, void *stream);

/* -------------------------------------------------------------------------- */
int mopk_version(void);
const char *mopk_strerror(int status);
/* 1 if the fused gfx950 kernels cover this Edgewise shape (N, dk, V, r). */
int mopk_edgewise_fused_supported(const MopkEdgewiseArgs *a);
/* name prefix of the dominant kernel(s) an edgewise fwd/bwd with these arguments launches (static string; bench.py matches
 * rocprofv3 kernel-trace rows with it -- the fused backward is three launches of one template, `ew_fused_bwd_kernel<.., 0|1|2>`,
 * and all three rows are summed). */
const char *mopk_edgewise_dominant_kernel(const MopkEdgewiseArgs *a, int backward);

#ifdef __cplusplus
}
#endif
#endif /* MOPK_H */
