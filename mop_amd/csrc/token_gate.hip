// 1-D MoP token gate of the GPT-MoP block (mop/models/gpt_mop.py:109-123) with the residual add of the block folded in.
//
// The reference's Linear -> conv1d(k=3) -> cat -> 1x1 conv1d -> alpha chain is linear in the residual stream r, so the host folds
// it into three taps u (3, D) (mop_amd/ops.py token_gate_taps) and the gate of token t is 1 + u0.r_{t-1} + u1.r_t + u2.r_{t+1}.
//
// Layout: a workgroup of TG_WAVES waves owns a tile of TG_TILE consecutive tokens of one sequence; wave w holds TG_TPW token rows in
// registers (16-byte vector loads, lane l owns the 8-element chunks l, l+64, ...; r = x + a formed on load).  The three dot
// products of every token (and the one each halo token contributes) go through LDS, so each row is read once and the multiply
// runs from registers.  Backward: delta_t = dout_t . r_t the same way, then dr from registers and du accumulated per lane; per-
// workgroup du partials go to the workspace and a second launch sums them in a fixed order (no atomics: bitwise reproducible).
// Algorithmic traffic: forward B*T*D*(sizeof x + sizeof a + sizeof out), backward B*T*D*(dout + x + a + dr) plus the halo rows
// (2 per tile) and the du partials.  Static LDS only (< 3 KB forward, < 17 KB backward): nothing to set before a graph capture.
//
// Per-row lengths (LENS = true, mopk_token_gate_lens_*): right-padded rows, n_b = clamp(lens[b], 0, T).  r_t counts as 0 for
// t >= n_b: "t < n_b" replaces "t < T" for every load, halo included, so gate_{n_b - 1} has no u2 term; rows t >= n_b are never
// read and get out = 0, gate = 1, dr = 0 written, and add nothing to du.  Full lengths run the instructions of LENS = false on the
// same operands (bitwise equal, du included).  The LENS = true instantiations are a unit of their own (-DMOPK_TOKEN_GATE_LENS).
#include "common.h"
#include <type_traits>

namespace mopk {
namespace {

constexpr int TG_WAVES = 8;                      // waves per workgroup
constexpr int TG_TPW = 2;                        // token rows per wave
constexpr int TG_TILE = TG_WAVES * TG_TPW;       // tokens per tile (16)
constexpr int TG_MAX_VPL = 2;                    // 8-element chunks per lane: D <= 64 * 8 * 2 = 1024
constexpr int TG_MAX_PARTS = 512;                // backward workgroups (du partial rows)

// the kernels' argument struct: MopkTokenGateArgs itself, or (LENS) the struct that wraps it with the lengths
template <bool LENS> using TgArgs = std::conditional_t<LENS, MopkTokenGateLensArgs, MopkTokenGateArgs>;
__host__ __device__ __forceinline__ const MopkTokenGateArgs &tg_base(const MopkTokenGateArgs &a) { return a; }
__host__ __device__ __forceinline__ const MopkTokenGateArgs &tg_base(const MopkTokenGateLensArgs &a) { return a.base; }
__device__ __forceinline__ int tg_len(const MopkTokenGateArgs &a, int) { return a.T; }
__device__ __forceinline__ int tg_len(const MopkTokenGateLensArgs &a, int b) {      // b is workgroup-uniform: a scalar load
    if (!a.lens) return a.base.T;
    const int n = a.lens[b];
    return n < 0 ? 0 : (n > a.base.T ? a.base.T : n);
}
template <typename T> __device__ __forceinline__ void tg_ld8(const T *p, float (&v)[8]);
template <> __device__ __forceinline__ void tg_ld8<float>(const float *p, float (&v)[8]) {
    const float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> __device__ __forceinline__ void tg_ld8<unsigned short>(const unsigned short *p, float (&v)[8]) {
    const uint4 u = *(const uint4 *)p;
    const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __builtin_bit_cast(float, w[i] << 16); v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u); }
}
template <typename T> __device__ __forceinline__ void tg_st8(T *p, const float (&v)[8]);
template <> __device__ __forceinline__ void tg_st8<float>(float *p, const float (&v)[8]) {
    *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
template <> __device__ __forceinline__ void tg_st8<unsigned short>(unsigned short *p, const float (&v)[8]) {
    *(uint4 *)p = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
}
// zeros for the chunks this lane owns of one (D) output row
template <typename OT, int VPL>
__device__ __forceinline__ void tg_store_zero(OT *op, int lane, int nvec) {
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) tg_st8<OT>(op + 8 * c, z);
    }
}

// r[i] = x + a for the chunks this lane owns (zeros past D)
template <typename XT, typename AT, int VPL>
__device__ __forceinline__ void tg_load_r(const MopkTokenGateArgs &a, int b, int t, int lane, float (&r)[VPL][8]) {
    const int nvec = a.D >> 3;
    const XT *xp = (const XT *)a.x + (int64_t)b * a.x_sb + (int64_t)t * a.x_st;
    const AT *ap = a.a ? (const AT *)a.a + (int64_t)b * a.a_sb + (int64_t)t * a.a_st : nullptr;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[i][e] = 0.f;
        if (c < nvec) {
            tg_ld8<XT>(xp + 8 * c, r[i]);
            if (ap) {
                float v[8];
                tg_ld8<AT>(ap + 8 * c, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) r[i][e] += v[e];
            }
        }
    }
}

template <int VPL>
__device__ __forceinline__ float tg_dot(const float (&p)[VPL][8], const float (&q)[VPL][8]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(p[i][e], q[i][e], s);
    return wave_sum(s);
}

template <typename OT, int VPL>
__device__ __forceinline__ void tg_load_o(const OT *p, int lane, int nvec, float (&v)[VPL][8]) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int c = lane + 64 * i;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        if (c < nvec) tg_ld8<OT>(p + 8 * c, v[i]);
    }
}

template <int VPL>
__device__ __forceinline__ void tg_load_u(const float *u, int lane, int nvec, int D, float (&uu)[3][VPL][8]) {
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int c = lane + 64 * i;
#pragma unroll
            for (int e = 0; e < 8; ++e) uu[s][i][e] = 0.f;
            if (c < nvec) tg_ld8<float>(u + (size_t)s * D + 8 * c, uu[s][i]);
        }
}

// gate_t = 1 + u0.r_{t-1} + u1.r_t + u2.r_{t+1} ; out_t = r_t gate_t
template <typename XT, typename AT, typename OT, int VPL, bool LENS = false>
__global__ __launch_bounds__(TG_WAVES * 64) void tg_fwd_kernel(TgArgs<LENS> al) {
    const MopkTokenGateArgs &a = tg_base(al);
    __shared__ float q[TG_TILE + 2][4];          // slot j = token t0 - 1 + j: (u0.r, u1.r, u2.r)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tiles = (a.T + TG_TILE - 1) / TG_TILE;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * TG_TILE;
    const int n = tg_len(al, b);                 // LENS: the real tokens of this row; else T
    const int nvec = a.D >> 3;
    float uu[3][VPL][8];
    tg_load_u<VPL>(a.u, lane, nvec, a.D, uu);
    float r[TG_TPW][VPL][8];
#pragma unroll
    for (int j = 0; j < TG_TPW; ++j) {
        const int slot = 1 + w * TG_TPW + j, t = t0 + slot - 1;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (t < n) {
            tg_load_r<XT, AT, VPL>(a, b, t, lane, r[j]);
            d0 = tg_dot<VPL>(r[j], uu[0]); d1 = tg_dot<VPL>(r[j], uu[1]); d2 = tg_dot<VPL>(r[j], uu[2]);
        }
        if (lane == 0) { q[slot][0] = d0; q[slot][1] = d1; q[slot][2] = d2; }
    }
    if (w < 2) {                                 // halo: wave 0 the token before the tile (its u0 term), wave 1 the one after (u2)
        const int slot = w ? TG_TILE + 1 : 0, t = t0 + slot - 1;
        float d = 0.f;
        if (t >= 0 && t < n) {
            float h[VPL][8];
            tg_load_r<XT, AT, VPL>(a, b, t, lane, h);
            d = tg_dot<VPL>(h, w ? uu[2] : uu[0]);
        }
        if (lane == 0) { q[slot][0] = w ? 0.f : d; q[slot][1] = 0.f; q[slot][2] = w ? d : 0.f; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TG_TPW; ++j) {
        const int slot = 1 + w * TG_TPW + j, t = t0 + slot - 1;
        if (t >= a.T) continue;
        if (LENS && t >= n) {                    // a padding row: out = 0, gate = 1 (wave-uniform)
            if (lane == 0) a.gate[(int64_t)b * a.T + t] = 1.f;
            tg_store_zero<OT, VPL>((OT *)a.out + ((int64_t)b * a.T + t) * a.D, lane, nvec);
            continue;
        }
        const float g = 1.f + q[slot - 1][0] + q[slot][1] + q[slot + 1][2];
        const int64_t row = (int64_t)b * a.T + t;
        if (lane == 0) a.gate[row] = g;
        OT *op = (OT *)a.out + row * a.D;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int c = lane + 64 * i;
            if (c < nvec) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = r[j][i][e] * g;
                tg_st8<OT>(op + 8 * c, o);
            }
        }
    }
}

// dr_t = dout_t gate_t + u0 delta_{t+1} + u1 delta_t + u2 delta_{t-1} ;  du_s += delta_{t+1-s} r_t   (s = 0, 1, 2)
template <typename XT, typename AT, typename OT, int VPL, bool LENS = false>
__global__ __launch_bounds__(TG_WAVES * 64) void tg_bwd_kernel(TgArgs<LENS> al, float *part) {
    const MopkTokenGateArgs &a = tg_base(al);
    __shared__ float dl[TG_TILE + 2];
    __shared__ float red[TG_WAVES][64 * 8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tiles = (a.T + TG_TILE - 1) / TG_TILE;
    const int ntiles = a.B * tiles;
    const int nvec = a.D >> 3;
    float uu[3][VPL][8], du[3][VPL][8];
    tg_load_u<VPL>(a.u, lane, nvec, a.D, uu);
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int i = 0; i < VPL; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) du[s][i][e] = 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / tiles, t0 = (tile % tiles) * TG_TILE;
        const int n = tg_len(al, b);
        float r[TG_TPW][VPL][8], go[TG_TPW][VPL][8];
#pragma unroll
        for (int j = 0; j < TG_TPW; ++j) {
            const int slot = 1 + w * TG_TPW + j, t = t0 + slot - 1;
            float d = 0.f;
            if (t < n) {
                tg_load_r<XT, AT, VPL>(a, b, t, lane, r[j]);
                tg_load_o<OT, VPL>((const OT *)a.dout + ((int64_t)b * a.T + t) * a.D, lane, nvec, go[j]);
                d = tg_dot<VPL>(r[j], go[j]);
            }
            if (lane == 0) dl[slot] = d;
        }
        if (w < 2) {
            const int slot = w ? TG_TILE + 1 : 0, t = t0 + slot - 1;
            float d = 0.f;
            if (t >= 0 && t < n) {
                float h[VPL][8], g[VPL][8];
                tg_load_r<XT, AT, VPL>(a, b, t, lane, h);
                tg_load_o<OT, VPL>((const OT *)a.dout + ((int64_t)b * a.T + t) * a.D, lane, nvec, g);
                d = tg_dot<VPL>(h, g);
            }
            if (lane == 0) dl[slot] = d;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TG_TPW; ++j) {
            const int slot = 1 + w * TG_TPW + j, t = t0 + slot - 1;
            if (t >= a.T) continue;
            const int64_t row = (int64_t)b * a.T + t;
            OT *op = (OT *)a.dr + row * a.D;
            if (LENS && t >= n) { tg_store_zero<OT, VPL>(op, lane, nvec); continue; }       // a padding row: dr = 0, nothing for du
            const float g = a.gate[row], dn = dl[slot + 1], dc = dl[slot], dp = dl[slot - 1];
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const int c = lane + 64 * i;
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    o[e] = fmaf(uu[0][i][e], dn, fmaf(uu[1][i][e], dc, fmaf(uu[2][i][e], dp, go[j][i][e] * g)));
                    du[0][i][e] = fmaf(dn, r[j][i][e], du[0][i][e]);
                    du[1][i][e] = fmaf(dc, r[j][i][e], du[1][i][e]);
                    du[2][i][e] = fmaf(dp, r[j][i][e], du[2][i][e]);
                }
                if (c < nvec) tg_st8<OT>(op + 8 * c, o);
            }
        }
        __syncthreads();                          // dl is rewritten by the next tile
    }
    // one partial (3, D) row per workgroup: the waves' accumulators summed through LDS in a fixed order
    float *prow = part + (size_t)blockIdx.x * 3 * a.D;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[w][lane * 8 + e] = du[s][i][e];
            __syncthreads();
            for (int c = threadIdx.x; c < 64 * 8; c += TG_WAVES * 64) {
                const int col = 64 * 8 * i + c;
                if (col < a.D) {
                    float acc = 0.f;
#pragma unroll
                    for (int ww = 0; ww < TG_WAVES; ++ww) acc += red[ww][c];
                    prow[s * a.D + col] = acc;
                }
            }
            __syncthreads();
        }
}

// du[c] = sum over partial rows p of part[p][c], p in a fixed order: 16 waves per 64 columns, each sums every 16th row, then LDS
__global__ __launch_bounds__(1024) void tg_reduce_kernel(const float *part, int nparts, int n, float *du) {
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
        du[col] = t;
    }
}

bool tg_dtype_ok(int d) { return d == MOPK_F32 || d == MOPK_BF16; }

// shape / dtype / stride / alignment rules shared by the support query and the entry points (pointers checked when non-null)
int tg_check(const MopkTokenGateArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->T <= 0 || a->D <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->D % 8 != 0 || a->D > 64 * 8 * TG_MAX_VPL) return MOPK_ERR_UNSUPPORTED;
    if ((int64_t)a->B * a->T > ((int64_t)1 << 31) - 1) return MOPK_ERR_UNSUPPORTED;
    if (!tg_dtype_ok(a->x_dtype) || !tg_dtype_ok(a->o_dtype) || (a->a && !tg_dtype_ok(a->a_dtype))) return MOPK_ERR_BAD_ARG;
    const int promo = (a->x_dtype == MOPK_F32 || (a->a && a->a_dtype == MOPK_F32)) ? MOPK_F32 : MOPK_BF16;
    if (a->o_dtype != promo) return MOPK_ERR_UNSUPPORTED;
    if (a->x_sb % 8 || a->x_st % 8 || a->x_st < a->D) return MOPK_ERR_UNSUPPORTED;
    if (a->a && (a->a_sb % 8 || a->a_st % 8 || a->a_st < a->D)) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(15, a->x, a->a, a->u, a->out, a->dout, a->dr, a->du, a->workspace)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

int tg_parts(const MopkTokenGateArgs *a) {
    const int64_t tiles = (int64_t)a->B * ((a->T + TG_TILE - 1) / TG_TILE);
    return (int)(tiles < TG_MAX_PARTS ? tiles : TG_MAX_PARTS);
}

template <typename XT, typename AT, typename OT, bool LENS>
void tg_launch(const TgArgs<LENS> *al, bool bwd, hipStream_t st) {
    const MopkTokenGateArgs *a = &tg_base(*al);
    const int vpl = (a->D / 8 + 63) / 64;
    const dim3 block(TG_WAVES * 64);
    const unsigned fwd_grid = (unsigned)(a->B * ((a->T + TG_TILE - 1) / TG_TILE));
#define MOPK_TG(V_) do {                                                                                                       \
        if (!bwd) hipLaunchKernelGGL((tg_fwd_kernel<XT, AT, OT, V_, LENS>), dim3(fwd_grid), block, 0, st, *al);                    \
        else hipLaunchKernelGGL((tg_bwd_kernel<XT, AT, OT, V_, LENS>), dim3(tg_parts(a)), block, 0, st, *al, (float *)a->workspace); \
    } while (0)
    if (vpl == 1) MOPK_TG(1); else MOPK_TG(2);
#undef MOPK_TG
}

template <bool LENS>
void tg_dispatch(const TgArgs<LENS> *al, bool bwd, hipStream_t st) {
    const MopkTokenGateArgs *a = &tg_base(*al);
    const bool xb = a->x_dtype == MOPK_BF16;
    const bool ab = a->a ? a->a_dtype == MOPK_BF16 : xb;         // no branch: AT is never read, instantiate as x's type
    if (xb && ab) tg_launch<unsigned short, unsigned short, unsigned short, LENS>(al, bwd, st);
    else if (xb) tg_launch<unsigned short, float, float, LENS>(al, bwd, st);
    else if (ab) tg_launch<float, unsigned short, float, LENS>(al, bwd, st);
    else tg_launch<float, float, float, LENS>(al, bwd, st);
}

// the reduction launch that ends either backward
int tg_reduce(const MopkTokenGateArgs *a, hipStream_t st) {
    const int n = 3 * a->D;
    hipLaunchKernelGGL(tg_reduce_kernel, dim3((n + 63) / 64), dim3(1024), 0, st, (const float *)a->workspace, tg_parts(a), n, a->du);
    return launch_status();
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

#ifndef MOPK_TOKEN_GATE_LENS
int mopk_token_gate_supported(const MopkTokenGateArgs *a) { return tg_check(a) == MOPK_OK; }

size_t mopk_token_gate_workspace_bytes(const MopkTokenGateArgs *a) {
    if (!a || a->B <= 0 || a->T <= 0 || a->D <= 0 || (int64_t)a->B * a->T > ((int64_t)1 << 31) - 1) return 0;   // as tg_check
    return (size_t)tg_parts(a) * 3 * a->D * sizeof(float);
}

int mopk_token_gate_fwd(const MopkTokenGateArgs *a, void *stream) {
    const int rc = tg_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->u, a->out, a->gate)) return MOPK_ERR_BAD_ARG;
    tg_dispatch<false>(a, false, (hipStream_t)stream);
    return launch_status();
}

int mopk_token_gate_bwd(const MopkTokenGateArgs *a, void *stream) {
    const int rc = tg_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->u, a->gate, a->dout, a->dr, a->du, a->workspace)) return MOPK_ERR_BAD_ARG;
    tg_dispatch<false>(a, true, (hipStream_t)stream);
    return tg_reduce(a, (hipStream_t)stream);
}
#else   // MOPK_TOKEN_GATE_LENS: the unit of the LENS = true instantiations; checks and sizes are those of base
static int tg_lens_check(const MopkTokenGateLensArgs *l) {
    if (!l) return MOPK_ERR_BAD_ARG;
    const int rc = tg_check(&l->base);
    if (rc != MOPK_OK) return rc;
    return misaligned(3, l->lens) ? MOPK_ERR_UNSUPPORTED : MOPK_OK;
}
int mopk_token_gate_lens_supported(const MopkTokenGateLensArgs *l) { return tg_lens_check(l) == MOPK_OK; }

size_t mopk_token_gate_lens_workspace_bytes(const MopkTokenGateLensArgs *l) {
    if (!l || l->base.B <= 0 || l->base.T <= 0 || l->base.D <= 0 || (int64_t)l->base.B * l->base.T > ((int64_t)1 << 31) - 1) return 0;
    return (size_t)tg_parts(&l->base) * 3 * l->base.D * sizeof(float);
}

int mopk_token_gate_lens_fwd(const MopkTokenGateLensArgs *l, void *stream) {
    const int rc = tg_lens_check(l);
    if (rc != MOPK_OK) return rc;
    const MopkTokenGateArgs *a = &l->base;
    if (any_null(a->x, a->u, a->out, a->gate)) return MOPK_ERR_BAD_ARG;
    tg_dispatch<true>(l, false, (hipStream_t)stream);
    return launch_status();
}

int mopk_token_gate_lens_bwd(const MopkTokenGateLensArgs *l, void *stream) {
    const int rc = tg_lens_check(l);
    if (rc != MOPK_OK) return rc;
    const MopkTokenGateArgs *a = &l->base;
    if (any_null(a->x, a->u, a->gate, a->dout, a->dr, a->du, a->workspace)) return MOPK_ERR_BAD_ARG;
    tg_dispatch<true>(l, true, (hipStream_t)stream);
    return tg_reduce(a, (hipStream_t)stream);
}
#endif  // MOPK_TOKEN_GATE_LENS

}  // extern "C"
