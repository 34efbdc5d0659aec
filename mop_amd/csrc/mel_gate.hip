// The MoP mel gate of the WhisperMoP encoder (mop/models/whisper_mop.py:91-124 MoP2D), all layers from one pass over the mel map,
// and the encoder block's residual add + gate multiply.
//
// MoP2D's 1x1 conv -> kxk conv -> cat -> 1x1 conv -> mean over frequency -> alpha chain is linear in the mel map, so the host folds
// every layer into taps W (L, k, F) (mop_amd/ops.py mel_gate_taps) and gate[b,l,t] = 1 + sum_i sum_f mel[b,t+i-p,f] W[l,i,f].
//
// Layout: a workgroup of MG_THREADS threads owns MG_TILE consecutive frames of one item.  It stages the tile and its 2p halo rows
// in LDS as fp32 (row stride MG_FS, odd: the 32 frames a wave reads in one step fall into 32 different banks) and the taps of up
// to MG_LC layers beside them; thread (l, t) then runs the k*F-term sum of one gate from LDS, i outer and f inner, an order that
// depends on neither T nor B.  More than MG_LC layers: one launch per chunk of layers.  Frames behind lens[b] are staged as zeros
// without being read; their gates are written as exactly 1.
// Backward: thread j of a workgroup owns the taps j, j + MG_THREADS, ... of the chunk in registers and adds dgate[l,t] * mel row
// products tile after tile (workgroup w takes the tiles w, w + P, ...); one partial row per workgroup goes to the workspace and a
// second launch sums the rows in a fixed order (no atomics: bitwise reproducible).
// Algorithmic traffic: B*T*F*sizeof(mel) (+ the halo rows, 2p per tile) + L*k*F*4 per workgroup from L2 + B*L*T*4 written;
// backward the same mel bytes + B*L*T*4 read + the partial rows.  Static LDS only (48.3 KB forward, 20.2 KB backward).
//
// gated_residual: one wave per token row, 16-byte vector loads and stores, lane l owns the 8-element chunks l, l + 64, ...;
// the backward's row sum is a wave reduction (no atomics).
#include "common.h"

namespace mopk {
namespace {

constexpr int MG_TILE = MOPK_MEL_GATE_TILE;              // frames per workgroup tile
constexpr int MG_LC = MOPK_MEL_GATE_LAYERS;              // layers per launch (their taps fit in LDS)
constexpr int MG_MAXK = MOPK_MEL_GATE_MAX_K;
constexpr int MG_MAXF = MOPK_MEL_GATE_MAX_F;
constexpr int MG_THREADS = MG_TILE * MG_LC;              // 256: thread (l, t) of the forward
constexpr int MG_ROWS = MG_TILE + MG_MAXK - 1;           // tile + halo
constexpr int MG_FS = MG_MAXF + 1;                       // LDS row stride (odd)
constexpr int MG_MAX_PARTS = 256;                        // backward workgroups (dW partial rows)
constexpr int MG_OPT = MG_LC * MG_MAXK * MG_MAXF / MG_THREADS;   // taps per thread of the backward (28)
constexpr int GR_WAVES = 4;                              // gated_residual: token rows per workgroup

template <typename T> __device__ __forceinline__ void mg_ld8(const T *p, float (&v)[8]);
template <> __device__ __forceinline__ void mg_ld8<float>(const float *p, float (&v)[8]) {
    const float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> __device__ __forceinline__ void mg_ld8<unsigned short>(const unsigned short *p, float (&v)[8]) {
    const uint4 u = *(const uint4 *)p;
    const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __builtin_bit_cast(float, w[i] << 16); v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u); }
}
template <typename T> __device__ __forceinline__ void mg_st8(T *p, const float (&v)[8]);
template <> __device__ __forceinline__ void mg_st8<float>(float *p, const float (&v)[8]) {
    *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <> __device__ __forceinline__ void mg_st8<unsigned short>(unsigned short *p, const float (&v)[8]) {
    *(uint4 *)p = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
}

__device__ __forceinline__ int mg_len(const MopkMelGateArgs &a, int b) {
    if (!a.lens) return a.T;
    const int n = a.lens[b];
    return n < 0 ? 0 : (n > a.T ? a.T : n);
}

// LDS row r = frame t0 - p + r of item b, r < MG_TILE + 2p; frames outside [0, len) are zeros and are not read.
// VEC: 8 elements per load (rows start on 16-byte boundaries and F % 8 == 0), else one element per load.
template <typename MT, bool VEC>
__device__ __forceinline__ void mg_stage(const MopkMelGateArgs &a, int b, int t0, int len, float *sm) {
    const int p = a.k >> 1, rows = MG_TILE + 2 * p;
    const MT *base = (const MT *)a.mel + (int64_t)b * a.mel_sb;
    if (VEC) {
        const int nv = a.F >> 3;
        for (int idx = threadIdx.x; idx < rows * nv; idx += MG_THREADS) {
            const int r = idx / nv, c = idx - r * nv, t = t0 - p + r;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
            if (t >= 0 && t < len) mg_ld8<MT>(base + (int64_t)t * a.mel_st + 8 * c, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) sm[r * MG_FS + 8 * c + e] = v[e];
        }
    } else {
        for (int idx = threadIdx.x; idx < rows * a.F; idx += MG_THREADS) {
            const int r = idx / a.F, f = idx - r * a.F, t = t0 - p + r;
            sm[r * MG_FS + f] = (t >= 0 && t < len) ? ld_as_f32<MT>(base + (int64_t)t * a.mel_st + f) : 0.f;
        }
    }
}

// gates[b, l0 + l, t] for the layers l < min(MG_LC, L - l0)
template <typename MT, bool VEC>
__global__ __launch_bounds__(MG_THREADS) void mg_fwd_kernel(MopkMelGateArgs a, int l0) {
    __shared__ float sm[MG_ROWS * MG_FS];
    __shared__ float sw[MG_LC * MG_MAXK * MG_MAXF];
    const int tiles = (a.T + MG_TILE - 1) / MG_TILE;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * MG_TILE;
    const int lc = a.L - l0 < MG_LC ? a.L - l0 : MG_LC;
    const int len = mg_len(a, b);
    const int tl = threadIdx.x % MG_TILE, ll = threadIdx.x / MG_TILE, t = t0 + tl;
    float *gp = a.gates + ((int64_t)b * a.L + l0 + ll) * a.T + t;
    if (t0 >= len) {                              // the whole tile lies behind the clip: nothing to read
        if (ll < lc && t < a.T) *gp = 1.f;
        return;
    }
    const int kF = a.k * a.F;
    for (int idx = threadIdx.x; idx < lc * kF; idx += MG_THREADS) sw[idx] = a.W[(size_t)l0 * kF + idx];
    mg_stage<MT, VEC>(a, b, t0, len, sm);
    __syncthreads();
    if (ll >= lc || t >= a.T) return;
    float g = 1.f;
    if (t < len) {
        float acc = 0.f;
        for (int i = 0; i < a.k; ++i) {
            const float *mr = sm + (tl + i) * MG_FS, *wr = sw + (ll * a.k + i) * a.F;
            for (int f = 0; f < a.F; ++f) acc = fmaf(mr[f], wr[f], acc);
        }
        g = 1.f + acc;
    }
    *gp = g;
}

// part[blockIdx.x][(l0 + l) k F + i F + f] = sum over this workgroup's tiles of dgates[b,l0+l,t] mel[b,t+i-p,f]
template <typename MT, bool VEC>
__global__ __launch_bounds__(MG_THREADS) void mg_bwd_kernel(MopkMelGateArgs a, int l0, float *part) {
    __shared__ float sm[MG_ROWS * MG_FS];
    __shared__ float sg[MG_LC * MG_TILE];
    const int tiles = (a.T + MG_TILE - 1) / MG_TILE, ntiles = a.B * tiles;
    const int lc = a.L - l0 < MG_LC ? a.L - l0 : MG_LC;
    const int kF = a.k * a.F, n = lc * kF;
    float acc[MG_OPT];
    int off[MG_OPT];                              // (LDS offset of mel[i][f]) | (l << 16) of the tap o = threadIdx.x + j MG_THREADS
#pragma unroll
    for (int j = 0; j < MG_OPT; ++j) {
        const int o = threadIdx.x + j * MG_THREADS;
        const int l = o / kF, rem = o - l * kF, i = rem / a.F, f = rem - i * a.F;
        acc[j] = 0.f;
        off[j] = (i * MG_FS + f) | (l << 16);
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / tiles, t0 = (tile % tiles) * MG_TILE;
        const int len = mg_len(a, b);
        if (t0 >= len) continue;                  // uniform in the workgroup: gates behind the clip are constants
        mg_stage<MT, VEC>(a, b, t0, len, sm);
        for (int idx = threadIdx.x; idx < lc * MG_TILE; idx += MG_THREADS) {
            const int l = idx / MG_TILE, t = t0 + idx % MG_TILE;
            sg[idx] = t < len ? a.dgates[((int64_t)b * a.L + l0 + l) * a.T + t] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MG_OPT; ++j) {
            if (threadIdx.x + j * MG_THREADS < n) {
                const float *mr = sm + (off[j] & 0xffff), *gr = sg + (off[j] >> 16) * MG_TILE;
                float s = acc[j];
#pragma unroll 8
                for (int tl = 0; tl < MG_TILE; ++tl) s = fmaf(gr[tl], mr[tl * MG_FS], s);
                acc[j] = s;
            }
        }
        __syncthreads();                          // sm and sg are rewritten by the next tile
    }
    float *prow = part + (size_t)blockIdx.x * a.L * kF + (size_t)l0 * kF;
#pragma unroll
    for (int j = 0; j < MG_OPT; ++j) {
        const int o = threadIdx.x + j * MG_THREADS;
        if (o < n) prow[o] = acc[j];
    }
}

// dW[c] = sum over partial rows p of part[p][c], p in a fixed order: 16 waves per 64 columns, each sums every 16th row, then LDS
__global__ __launch_bounds__(1024) void mg_reduce_kernel(const float *part, int nparts, int n, float *dW) {
    __shared__ float red[16][64];
    const int c = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c;
    float acc = 0.f;
    if (col < n)
        for (int p = s; p < nparts; p += 16) acc += part[(size_t)p * n + col];
    red[s][c] = acc;
    __syncthreads();
    if (s == 0 && col < n) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i][c];
        dW[col] = t;
    }
}

// out = (x + a) gate
template <typename XT, typename AT, typename OT>
__global__ __launch_bounds__(GR_WAVES * 64) void gr_fwd_kernel(MopkGatedResidualArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * GR_WAVES + w;
    if (row >= (int64_t)a.B * a.T) return;
    const int b = (int)(row / a.T), t = (int)(row % a.T), nvec = a.D >> 3;
    const float g = a.gate[(int64_t)b * a.gate_sb + t];
    const XT *xp = (const XT *)a.x + (int64_t)b * a.x_sb + (int64_t)t * a.x_st;
    const AT *ap = (const AT *)a.a + (int64_t)b * a.a_sb + (int64_t)t * a.a_st;
    OT *op = (OT *)a.out + row * a.D;
    for (int c = lane; c < nvec; c += 64) {
        float x[8], r[8];
        mg_ld8<XT>(xp + 8 * c, x);
        mg_ld8<AT>(ap + 8 * c, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (x[e] + r[e]) * g;
        mg_st8<OT>(op + 8 * c, r);
    }
}

// dr = dout gate ; dgate = sum_d dout (x + a)
template <typename XT, typename AT, typename OT>
__global__ __launch_bounds__(GR_WAVES * 64) void gr_bwd_kernel(MopkGatedResidualArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * GR_WAVES + w;
    if (row >= (int64_t)a.B * a.T) return;        // whole waves leave: the shuffles below see full waves
    const int b = (int)(row / a.T), t = (int)(row % a.T), nvec = a.D >> 3;
    const float g = a.gate[(int64_t)b * a.gate_sb + t];
    const XT *xp = (const XT *)a.x + (int64_t)b * a.x_sb + (int64_t)t * a.x_st;
    const AT *ap = (const AT *)a.a + (int64_t)b * a.a_sb + (int64_t)t * a.a_st;
    const OT *gp = (const OT *)a.dout + row * a.D;
    OT *op = (OT *)a.dr + row * a.D;
    float s = 0.f;
    for (int c = lane; c < nvec; c += 64) {
        float x[8], r[8], go[8];
        mg_ld8<XT>(xp + 8 * c, x);
        mg_ld8<AT>(ap + 8 * c, r);
        mg_ld8<OT>(gp + 8 * c, go);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s = fmaf(go[e], x[e] + r[e], s); go[e] *= g; }
        mg_st8<OT>(op + 8 * c, go);
    }
    s = wave_sum(s);
    if (lane == 0) a.dgate[row] = s;
}

bool mg_dtype_ok(int d) { return d == MOPK_F32 || d == MOPK_BF16; }

// shape / dtype / stride / alignment rules shared by the support query and the entry points (pointers checked when non-null)
int mg_check(const MopkMelGateArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->T <= 0 || a->F <= 0 || a->L <= 0 || a->k <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->k % 2 == 0 || a->k > MG_MAXK || a->F > MG_MAXF) return MOPK_ERR_UNSUPPORTED;
    if (!mg_dtype_ok(a->mel_dtype)) return MOPK_ERR_BAD_ARG;
    const int64_t tiles = (a->T + MG_TILE - 1) / MG_TILE;
    if (a->B * tiles > ((int64_t)1 << 31) - 1 || (int64_t)a->L * a->k * a->F > ((int64_t)1 << 31) - 1) return MOPK_ERR_UNSUPPORTED;
    if (a->mel_st < a->F || a->mel_sb < 0) return MOPK_ERR_BAD_ARG;
    const uintptr_t es = a->mel_dtype == MOPK_F32 ? 4 : 2;
    if (misaligned(es - 1, a->mel) || misaligned(3, a->W, a->lens, a->gates, a->dgates, a->dW, a->workspace)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

// rows of 8-element chunks on 16-byte boundaries
bool mg_vec(const MopkMelGateArgs *a) {
    return a->F % 8 == 0 && a->mel_st % 8 == 0 && a->mel_sb % 8 == 0 && !misaligned(15, a->mel);
}

int mg_parts(const MopkMelGateArgs *a) {
    const int64_t tiles = (int64_t)a->B * ((a->T + MG_TILE - 1) / MG_TILE);
    return (int)(tiles < MG_MAX_PARTS ? tiles : MG_MAX_PARTS);
}

template <typename MT, bool VEC>
void mg_launch(const MopkMelGateArgs *a, bool bwd, hipStream_t st) {
    const unsigned fwd_grid = (unsigned)(a->B * ((a->T + MG_TILE - 1) / MG_TILE));
    for (int l0 = 0; l0 < a->L; l0 += MG_LC) {
        if (!bwd) hipLaunchKernelGGL((mg_fwd_kernel<MT, VEC>), dim3(fwd_grid), dim3(MG_THREADS), 0, st, *a, l0);
        else hipLaunchKernelGGL((mg_bwd_kernel<MT, VEC>), dim3(mg_parts(a)), dim3(MG_THREADS), 0, st, *a, l0, (float *)a->workspace);
    }
}

void mg_dispatch(const MopkMelGateArgs *a, bool bwd, hipStream_t st) {
    const bool bf = a->mel_dtype == MOPK_BF16, vec = mg_vec(a);
    if (bf && vec) mg_launch<unsigned short, true>(a, bwd, st);
    else if (bf) mg_launch<unsigned short, false>(a, bwd, st);
    else if (vec) mg_launch<float, true>(a, bwd, st);
    else mg_launch<float, false>(a, bwd, st);
}

int gr_check(const MopkGatedResidualArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->T <= 0 || a->D <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->D % 8 != 0) return MOPK_ERR_UNSUPPORTED;
    if ((int64_t)a->B * a->T > (((int64_t)1 << 31) - 1) * GR_WAVES) return MOPK_ERR_UNSUPPORTED;
    if (!mg_dtype_ok(a->x_dtype) || !mg_dtype_ok(a->a_dtype) || !mg_dtype_ok(a->o_dtype)) return MOPK_ERR_BAD_ARG;
    const int promo = (a->x_dtype == MOPK_F32 || a->a_dtype == MOPK_F32) ? MOPK_F32 : MOPK_BF16;
    if (a->o_dtype != promo) return MOPK_ERR_UNSUPPORTED;
    if (a->x_sb % 8 || a->x_st % 8 || a->x_st < a->D || a->x_sb < 0) return MOPK_ERR_UNSUPPORTED;
    if (a->a_sb % 8 || a->a_st % 8 || a->a_st < a->D || a->a_sb < 0) return MOPK_ERR_UNSUPPORTED;
    if (a->gate_sb < 0 || (a->B > 1 && a->gate_sb < a->T)) return MOPK_ERR_BAD_ARG;
    if (misaligned(15, a->x, a->a, a->out, a->dout, a->dr) || misaligned(3, a->gate, a->dgate)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <typename XT, typename AT, typename OT>
void gr_launch(const MopkGatedResidualArgs *a, bool bwd, hipStream_t st) {
    const unsigned grid = (unsigned)(((int64_t)a->B * a->T + GR_WAVES - 1) / GR_WAVES);
    if (!bwd) hipLaunchKernelGGL((gr_fwd_kernel<XT, AT, OT>), dim3(grid), dim3(GR_WAVES * 64), 0, st, *a);
    else hipLaunchKernelGGL((gr_bwd_kernel<XT, AT, OT>), dim3(grid), dim3(GR_WAVES * 64), 0, st, *a);
}

void gr_dispatch(const MopkGatedResidualArgs *a, bool bwd, hipStream_t st) {
    const bool xb = a->x_dtype == MOPK_BF16, ab = a->a_dtype == MOPK_BF16;
    if (xb && ab) gr_launch<unsigned short, unsigned short, unsigned short>(a, bwd, st);
    else if (xb) gr_launch<unsigned short, float, float>(a, bwd, st);
    else if (ab) gr_launch<float, unsigned short, float>(a, bwd, st);
    else gr_launch<float, float, float>(a, bwd, st);
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_mel_gate_supported(const MopkMelGateArgs *a) { return mg_check(a) == MOPK_OK; }

size_t mopk_mel_gate_workspace_bytes(const MopkMelGateArgs *a) {
    if (mg_check(a) != MOPK_OK) return 0;
    return (size_t)mg_parts(a) * a->L * a->k * a->F * sizeof(float);
}

int mopk_mel_gate_fwd(const MopkMelGateArgs *a, void *stream) {
    const int rc = mg_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->mel, a->W, a->gates)) return MOPK_ERR_BAD_ARG;
    mg_dispatch(a, false, (hipStream_t)stream);
    return launch_status();
}

int mopk_mel_gate_bwd(const MopkMelGateArgs *a, void *stream) {
    const int rc = mg_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->mel, a->dgates, a->dW, a->workspace)) return MOPK_ERR_BAD_ARG;
    mg_dispatch(a, true, (hipStream_t)stream);
    const int n = a->L * a->k * a->F;
    hipLaunchKernelGGL(mg_reduce_kernel, dim3((n + 63) / 64), dim3(1024), 0, (hipStream_t)stream, (const float *)a->workspace,
                       mg_parts(a), n, a->dW);
    return launch_status();
}

int mopk_gated_residual_supported(const MopkGatedResidualArgs *a) { return gr_check(a) == MOPK_OK; }

size_t mopk_gated_residual_workspace_bytes(const MopkGatedResidualArgs *) { return 0; }

int mopk_gated_residual_fwd(const MopkGatedResidualArgs *a, void *stream) {
    const int rc = gr_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->a, a->gate, a->out)) return MOPK_ERR_BAD_ARG;
    gr_dispatch(a, false, (hipStream_t)stream);
    return launch_status();
}

int mopk_gated_residual_bwd(const MopkGatedResidualArgs *a, void *stream) {
    const int rc = gr_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->a, a->gate, a->dout, a->dr, a->dgate)) return MOPK_ERR_BAD_ARG;
    gr_dispatch(a, true, (hipStream_t)stream);
    return launch_status();
}

}  // extern "C"
