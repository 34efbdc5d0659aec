// Top-1 routed mixture-of-experts MLP (mop/models/components.py:84-121): y_t = W2_e gelu(W1_e x_t) with e = argmax(gate(x_t)).
//
// The reference runs every expert on every token and keeps one result through a one-hot product; here each token runs through
// its own expert only (1/E of the expert FLOPs) and no per-expert count ever reaches the host, so every launch is graph-capturable.
//
// Route (2 launches): moe_logits_kernel computes the gate logits in fp32 FMA from x, gate.weight, gate.bias (one wave per token,
// a fixed butterfly order) and the argmax (strict >, ties to the lowest index as torch.argmax); moe_scan_kernel (one workgroup)
// counts tokens per expert with integer counters in LDS, scans them and writes a stable permutation: sorted position p -> token,
// experts in index order, tokens ascending inside an expert.  route = [expert (M) | perm (M) | offsets (E + 1)] int32.
//
// Grouped GEMM (moe_gemm_kernel, one template, six modes): rows are sorted positions, so expert e owns rows [off_e, off_{e+1}).
// The row-tile grid is sized from the upper bound ceil(M / TM) + E - 1 (sum_e ceil(c_e / TM) never exceeds it); a workgroup finds
// its expert by walking the E + 1 offsets and exits when it is past the last tile.  Operands are staged through registers into
// LDS as [row][k] images (bf16, or fp32 for the exact path), gathered rows included: the token row of a sorted position is read
// through perm while the tile is staged.  Edges are zero-filled (M any, D and F multiples of 8).
//   FC1: U = X_e W1_e^T (A rows gathered), epilogue stores U and H = gelu(U) (both in sorted order, kept for the backward)
//   FC2: Y = H_e W2_e^T, epilogue scatters each row to its token (+ residual): every token is written exactly once
//   DU : dU = (dY_e W2_e) * gelu'(U) (A rows gathered)
//   DX : dX = dU_e W1_e, scattered to the token rows
//   WG2: dW2_e = dY_e^T H_e, WG1: dW1_e = dU_e^T X_e -- the reduction runs over an expert's rows, cut into chunks of `chunk`
//        rows; each (chunk, tile) writes an fp32 partial slab and moe_wsum_kernel adds an expert's slabs in chunk order
//        (no atomics: bitwise reproducible).  An expert without tokens owns no chunk and gets zeros.
// Arithmetic: PREC_BF16 rounds operands to bf16 while staging and runs v_mfma_f32_16x16x32_bf16; PREC_FP32 keeps fp32 in LDS and
// runs v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  Both accumulate in fp32 and share the 16x16 C layout.
#include "common.h"

namespace mopk {
namespace {

constexpr int MOE_BK = 32;                   // k per staged tile
constexpr int MOE_LDH = MOE_BK + 8;          // bf16 LDS row stride (16-byte fragment reads)
constexpr int MOE_LDF = MOE_BK + 4;          // fp32 LDS row stride (16-byte fragment reads)

enum MoeMode { FC1 = 0, FC2 = 1, DU = 2, DX = 3, WG2 = 4, WG1 = 5 };

__device__ __forceinline__ float gelu_tanh(float u) {
    const float c = 0.7978845608028654f;
    return 0.5f * u * (1.f + tanhf(c * fmaf(0.044715f * u, u * u, u)));
}
__device__ __forceinline__ float gelu_tanh_grad(float u) {
    const float c = 0.7978845608028654f;
    const float t = tanhf(c * fmaf(0.044715f * u, u * u, u));
    return 0.5f * (1.f + t) + 0.5f * u * (1.f - t * t) * c * fmaf(3.f * 0.044715f, u * u, 1.f);
}

// 8 consecutive elements of a fp32 / bf16 buffer (element offset a multiple of 8, 16-byte aligned base)
__device__ __forceinline__ void moe_ld8(const void *base, int64_t off, int dt, float (&v)[8]) {
    if (dt == MOPK_BF16) {
        const uint4 u = *(const uint4 *)((const unsigned short *)base + off);
        const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __builtin_bit_cast(float, w[i] << 16); v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u); }
    } else {
        const float4 a = *(const float4 *)((const float *)base + off), b = *(const float4 *)((const float *)base + off + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}
__device__ __forceinline__ float moe_ld1(const void *base, int64_t off, int dt) {
    return dt == MOPK_BF16 ? bf2f(((const unsigned short *)base)[off]) : ((const float *)base)[off];
}
__device__ __forceinline__ void moe_st1(void *base, int64_t off, int dt, float v) {
    if (dt == MOPK_BF16) ((unsigned short *)base)[off] = f2bf(v);
    else ((float *)base)[off] = v;
}

// One operand tile: ROWS rows x MOE_BK k of X(r, k), staged to an LDS image [r][k].
//  KC (k contiguous): element (r, k) at base[roff_r + k]; roff_r is fixed over the k loop (a gathered token row, a sorted row or a
//      weight row), -1 for rows outside the tile's range.  Thread t: rows t/4 + 64 j, k = 8 (t % 4) .. +7 (16-byte loads).
//  RC (r contiguous): element (r, k) at base[src(k) * ld + c0 + r], src(k) = perm[k] for gathered rows.  Thread t: k = t / 8,
//      r = 8 (t % 8) + 64 j .. +7 (16-byte loads along r, scalar LDS stores).
template <int ROWS, bool BF16>
struct MoeStage {
    static constexpr int NJ = ROWS / 64;
    float v[NJ][8];
    __device__ __forceinline__ void load_kc(const void *base, int dt, const int64_t (&roff)[NJ], int k0, int K) {
        const int k = k0 + (threadIdx.x & 3) * 8;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (roff[j] >= 0 && k < K) moe_ld8(base, roff[j] + k, dt, v[j]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
            }
        }
    }
    // k rows [k0, k1) of the source (sorted positions; through perm when perm != nullptr), columns [c0, c0 + ROWS) below R
    __device__ __forceinline__ void load_rc(const void *base, int dt, int64_t ld, const int *perm, int k0, int k1, int c0, int R) {
        const int kk = k0 + (threadIdx.x >> 3);
        int64_t srow = -1;
        if (kk < k1) srow = perm ? perm[kk] : kk;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = c0 + (threadIdx.x & 7) * 8 + 64 * j;
            if (srow >= 0 && c < R) moe_ld8(base, srow * ld + c, dt, v[j]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
            }
        }
    }
    __device__ __forceinline__ void store_kc(void *lds) const {
        const int r = threadIdx.x >> 2, k = (threadIdx.x & 3) * 8;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (BF16) {
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(v[j][e]);
                *(bf16x8 *)((unsigned short *)lds + (r + 64 * j) * MOE_LDH + k) = o;
            } else {
                float *p = (float *)lds + (r + 64 * j) * MOE_LDF + k;
                *(float4 *)p = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
                *(float4 *)(p + 4) = make_float4(v[j][4], v[j][5], v[j][6], v[j][7]);
            }
        }
    }
    __device__ __forceinline__ void store_rc(void *lds) const {
        const int k = threadIdx.x >> 3, r = (threadIdx.x & 7) * 8;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (BF16) ((unsigned short *)lds)[(r + 64 * j + e) * MOE_LDH + k] = f2bf(v[j][e]);
                else ((float *)lds)[(r + 64 * j + e) * MOE_LDF + k] = v[j][e];
            }
    }
};

// which operand layouts a mode stages: A is KC for the four row-block GEMMs, RC for the weight gradients; B is KC where the weight
// is read as W[n][k] (FC1, FC2), RC where it is read as W[k][n] (DU, DX) and for the weight gradients
template <int MODE> struct MoeLayout {
    static constexpr bool A_KC = MODE <= DX;
    static constexpr bool B_KC = MODE == FC1 || MODE == FC2;
};

// expert and row range of row tile t of width TM: experts' tiles are laid end to end in expert order.  false: surplus workgroup.
__device__ __forceinline__ bool moe_find_tile(const int *off, int E, int TMr, int t, int &e, int &r0, int &r1) {
    int base = 0;
    for (int x = 0; x < E; ++x) {
        const int o0 = off[x], o1 = off[x + 1];
        const int n = (o1 - o0 + TMr - 1) / TMr;
        if (t < base + n) { e = x; r0 = o0 + (t - base) * TMr; r1 = min(o1, r0 + TMr); return true; }
        base += n;
    }
    return false;
}

template <int MODE, bool BF16, int TM, int TN>
__global__ __launch_bounds__(256) void moe_gemm_kernel(MopkMoeArgs a, int chunk, float *slab) {
    constexpr int LD = BF16 ? MOE_LDH : MOE_LDF, ES = BF16 ? 2 : 4;
    __shared__ __attribute__((aligned(16))) char smem[(TM + TN) * LD * ES];
    void *Al = smem, *Bl = smem + TM * LD * ES;
    constexpr int MI = TM / 32, NI = TN / 32;
    constexpr bool WG = MODE >= WG2;
    using L = MoeLayout<MODE>;
    const int M = a.M, D = a.D, F = a.F, E = a.E;
    const int *perm = a.route + M;
    const int *off = a.route + 2 * M;
    const int act_dt = BF16 ? MOPK_BF16 : MOPK_F32;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;

    // ---- the tile: expert e, output rows [m0, m0 + TM) x columns [n0, n0 + TN) and the k range
    int e, r0, r1;
    int m0, n0, Mo, No, K;                        // output rows / columns bound, reduction length
    if (!WG) {
        if (!moe_find_tile(off, E, TM, blockIdx.x, e, r0, r1)) return;
        m0 = r0; Mo = r1;
        n0 = blockIdx.y * TN;
        No = (MODE == FC1 || MODE == DU) ? F : D;
        K = (MODE == FC1 || MODE == DU) ? D : F;
    } else {
        if (!moe_find_tile(off, E, chunk, blockIdx.y, e, r0, r1)) return;
        const int I = MODE == WG2 ? D : F, J = MODE == WG2 ? F : D;
        const int tj = (J + TN - 1) / TN;
        m0 = (blockIdx.x / tj) * TM; n0 = (blockIdx.x % tj) * TN;
        Mo = I; No = J; K = r1 - r0;
    }

    // ---- operand sources
    const void *Ab, *Bb;
    int adt, bdt;
    int64_t lda = 0, ldb = 0;
    switch (MODE) {
        case FC1: Ab = a.x; adt = a.x_dtype; lda = D; Bb = a.w1[e]; bdt = a.w_dtype; ldb = D; break;
        case FC2: Ab = a.h; adt = act_dt; lda = F; Bb = a.w2[e]; bdt = a.w_dtype; ldb = F; break;
        case DU:  Ab = a.dy; adt = a.o_dtype; lda = D; Bb = a.w2[e]; bdt = a.w_dtype; ldb = F; break;
        case DX:  Ab = a.workspace; adt = act_dt; lda = F; Bb = a.w1[e]; bdt = a.w_dtype; ldb = D; break;
        case WG2: Ab = a.dy; adt = a.o_dtype; lda = D; Bb = a.h; bdt = act_dt; ldb = F; break;
        default:  Ab = a.workspace; adt = act_dt; lda = F; Bb = a.x; bdt = a.x_dtype; ldb = D; break;
    }
    const bool a_gather = MODE == FC1 || MODE == DU || MODE == WG2;
    const bool b_gather = MODE == WG1;

    MoeStage<TM, BF16> sa;
    MoeStage<TN, BF16> sb;
    int64_t aoff[TM / 64], boff[TN / 64];
    if (L::A_KC) {
#pragma unroll
        for (int j = 0; j < TM / 64; ++j) {
            const int m = m0 + (tid >> 2) + 64 * j;
            aoff[j] = m < Mo ? (int64_t)(a_gather ? perm[m] : m) * lda : -1;
        }
    }
    if (L::B_KC) {
#pragma unroll
        for (int j = 0; j < TN / 64; ++j) {
            const int n = n0 + (tid >> 2) + 64 * j;
            boff[j] = n < No ? (int64_t)n * ldb : -1;
        }
    }
    // k0 runs over [0, K); for the weight gradients the k index is the sorted row r0 + k
    auto load = [&](int k0) {
        if (L::A_KC) sa.load_kc(Ab, adt, aoff, k0, K);
        else sa.load_rc(Ab, adt, lda, a_gather ? perm : nullptr, r0 + k0, r1, m0, Mo);
        if (L::B_KC) sb.load_kc(Bb, bdt, boff, k0, K);
        else if (WG) sb.load_rc(Bb, bdt, ldb, b_gather ? perm : nullptr, r0 + k0, r1, n0, No);
        else sb.load_rc(Bb, bdt, ldb, nullptr, k0, K, n0, No);     // DU / DX: B(n, k) = W[k][n]
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int k0 = 0; k0 < K; k0 += MOE_BK) {
        if (L::A_KC) sa.store_kc(Al); else sa.store_rc(Al);
        if (L::B_KC) sb.store_kc(Bl); else sb.store_rc(Bl);
        __syncthreads();
        if (k0 + MOE_BK < K) load(k0 + MOE_BK);
        if (BF16) {
            const unsigned short *Ah = (const unsigned short *)Al, *Bh = (const unsigned short *)Bl;
            bf16x8 af[MI], bfr[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *(const bf16x8 *)&Ah[(wm * (TM / 2) + i * 16 + (lane & 15)) * LD + 8 * (lane >> 4)];
#pragma unroll
            for (int j = 0; j < NI; ++j) bfr[j] = *(const bf16x8 *)&Bh[(wn * (TN / 2) + j * 16 + (lane & 15)) * LD + 8 * (lane >> 4)];
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        } else {
            // lane group g = lane / 16 reads k = 16 h + 4 g .. +3 as one float4 and feeds them to four MFMAs; A and B use the same
            // k order, so the four steps of both halves cover k = 0 .. 31 exactly once
            const float *As = (const float *)Al, *Bs = (const float *)Bl;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float4 af[MI], bfr[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) af[i] = *(const float4 *)&As[(wm * (TM / 2) + i * 16 + (lane & 15)) * LD + 16 * h + 4 * (lane >> 4)];
#pragma unroll
                for (int j = 0; j < NI; ++j) bfr[j] = *(const float4 *)&Bs[(wn * (TN / 2) + j * 16 + (lane & 15)) * LD + 16 * h + 4 * (lane >> 4)];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bfr[j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bfr[j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bfr[j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bfr[j].w, acc[i][j], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }

    // ---- epilogue: lane holds rows (lane / 16) * 4 + r, column lane % 16 of each 16 x 16 tile
    if (WG) slab += (size_t)blockIdx.y * (size_t)D * F;         // this chunk's (I, J) partial
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * (TM / 2) + i * 16 + (lane >> 4) * 4 + r;
            if (m >= Mo) continue;
            int64_t tok = m;
            if (MODE == FC2 || MODE == DX) tok = perm[m];
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int n = n0 + wn * (TN / 2) + j * 16 + (lane & 15);
                if (n >= No) continue;
                const float v = acc[i][j][r];
                switch (MODE) {
                    case FC1: {
                        const int64_t o = (int64_t)m * F + n;
                        moe_st1(a.u, o, act_dt, v);
                        moe_st1(a.h, o, act_dt, gelu_tanh(v));
                        break;
                    }
                    case FC2: {
                        const int64_t o = tok * D + n;
                        moe_st1(a.y, o, a.o_dtype, a.residual ? v + moe_ld1(a.residual, o, a.o_dtype) : v);
                        break;
                    }
                    case DU: {
                        const int64_t o = (int64_t)m * F + n;
                        moe_st1(a.workspace, o, act_dt, v * gelu_tanh_grad(moe_ld1(a.u, o, act_dt)));
                        break;
                    }
                    case DX: moe_st1(a.dx, tok * D + n, a.x_dtype, v); break;
                    default: slab[(int64_t)m * No + n] = v; break;
                }
            }
        }
}

}  // namespace
}  // namespace mopk

namespace mopk {
namespace {

// gate logits in fp32 FMA (lane d-strided partial sums, a fixed butterfly) and the argmax: one wave per token
__global__ __launch_bounds__(256) void moe_logits_kernel(MopkMoeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.M) return;
    const int64_t xo = t * a.D;
    int best = 0;
    float bv = 0.f;
    for (int e = 0; e < a.E; ++e) {
        float s = 0.f;
        for (int d = lane; d < a.D; d += 64) s = fmaf(moe_ld1(a.x, xo + d, a.x_dtype), moe_ld1(a.gate_w, (int64_t)e * a.D + d, a.gate_dtype), s);
        s = wave_sum(s);
        if (a.gate_b) s += moe_ld1(a.gate_b, e, a.gate_dtype);
        if (e == 0 || s > bv) { bv = s; best = e; }
    }
    if (lane == 0) a.route[t] = best;
}

// counts, offsets and the stable permutation, one workgroup: thread i owns tokens [i C, (i + 1) C); cnt[e][i] counts its tokens of
// expert e, a per-expert scan over threads turns the counts into first positions, and a second pass over the same tokens in the
// same order places them.  Integer arithmetic only: the permutation is a pure function of the expert indices.
constexpr int MOE_SCAN_THREADS = 256;
__global__ __launch_bounds__(MOE_SCAN_THREADS) void moe_scan_kernel(MopkMoeArgs a) {
    __shared__ int cnt[MOPK_MOE_MAX_EXPERTS][MOE_SCAN_THREADS];
    __shared__ int tot[MOPK_MOE_MAX_EXPERTS + 1];
    const int i = threadIdx.x, E = a.E;
    const int64_t M = a.M, C = (M + MOE_SCAN_THREADS - 1) / MOE_SCAN_THREADS;
    const int64_t t0 = i * C, t1 = t0 + C < M ? t0 + C : M;
    const int *ex = a.route;
    int *perm = a.route + M, *off = a.route + 2 * M;
    for (int e = 0; e < E; ++e) cnt[e][i] = 0;
    for (int64_t t = t0; t < t1; ++t) cnt[ex[t]][i] += 1;
    __syncthreads();
    if (i < E) {
        int s = 0;
        for (int j = 0; j < MOE_SCAN_THREADS; ++j) { const int c = cnt[i][j]; cnt[i][j] = s; s += c; }
        tot[i] = s;
    }
    __syncthreads();
    if (i == 0) {
        int s = 0;
        for (int e = 0; e < E; ++e) { const int c = tot[e]; tot[e] = s; off[e] = s; s += c; }
        off[E] = s;
    }
    __syncthreads();
    for (int64_t t = t0; t < t1; ++t) {
        const int e = ex[t];
        const int p = tot[e] + cnt[e][i];
        cnt[e][i] += 1;
        perm[p] = (int)t;
    }
}

// dW_e = sum of expert e's chunk slabs in chunk order (zeros without tokens), written in the weights' dtype; z = 0: dW1, 1: dW2
__global__ __launch_bounds__(256) void moe_wsum_kernel(MopkMoeArgs a, int chunk, const float *slab1, const float *slab2) {
    const int e = blockIdx.y, which = blockIdx.z;
    const int64_t n = (int64_t)a.D * a.F;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const int *off = a.route + 2 * (int64_t)a.M;
    int c0 = 0;
    for (int x = 0; x < e; ++x) c0 += (off[x + 1] - off[x] + chunk - 1) / chunk;
    const int nc = (off[e + 1] - off[e] + chunk - 1) / chunk;
    const float *s = which ? slab2 : slab1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = c0; c < c0 + nc; ++c) {
        const float4 v = *(const float4 *)(s + (size_t)c * n + i);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    void *dst = which ? a.dw2[e] : a.dw1[e];
    if (a.w_dtype == MOPK_BF16) {
        *(uint2 *)((unsigned short *)dst + i) = make_uint2(pack_bf16(acc.x, acc.y), pack_bf16(acc.z, acc.w));
    } else {
        *(float4 *)((float *)dst + i) = acc;
    }
}

// ---- host side
constexpr int MOE_CHUNK_MIN = 256;
constexpr int MOE_TARGET_CHUNKS = 16;

// rows per weight-gradient chunk: about M / 16, a multiple of 256 (a pure function of M, so results do not depend on the routing)
int moe_chunk(int64_t M) {
    int64_t c = (M + MOE_TARGET_CHUNKS - 1) / MOE_TARGET_CHUNKS;
    c = (c + MOE_CHUNK_MIN - 1) / MOE_CHUNK_MIN * MOE_CHUNK_MIN;
    return (int)c;
}
int64_t moe_tiles_bound(int64_t M, int E, int T) { return (M + T - 1) / T + E - 1; }
int moe_act_dt(const MopkMoeArgs *a) { return a->precision == MOPK_PREC_BF16 ? MOPK_BF16 : MOPK_F32; }
size_t moe_dsize(int dt) { return dt == MOPK_BF16 ? 2 : 4; }
size_t moe_du_bytes(const MopkMoeArgs *a) { return (size_t)round_up((int64_t)a->M * a->F * moe_dsize(moe_act_dt(a)), 256); }
size_t moe_slab_bytes(const MopkMoeArgs *a) {
    return (size_t)moe_tiles_bound(a->M, a->E, moe_chunk(a->M)) * a->D * a->F * sizeof(float);
}

bool moe_dt_ok(int d) { return d == MOPK_F32 || d == MOPK_BF16; }

// argument rules shared by the support query and the entry points (pointers checked when non-null)
int moe_check(const MopkMoeArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->M <= 0 || a->D <= 0 || a->F <= 0 || a->E < 2) return MOPK_ERR_BAD_SHAPE;
    if (a->precision != MOPK_PREC_FP32 && a->precision != MOPK_PREC_BF16) return MOPK_ERR_BAD_ARG;
    if (!moe_dt_ok(a->x_dtype) || !moe_dt_ok(a->w_dtype) || !moe_dt_ok(a->gate_dtype) || !moe_dt_ok(a->o_dtype)) return MOPK_ERR_BAD_ARG;
    if (a->E > MOPK_MOE_MAX_EXPERTS || a->D % 8 || a->F % 8) return MOPK_ERR_UNSUPPORTED;
    if ((int64_t)a->M * a->F > ((int64_t)1 << 31) - 1 || (int64_t)a->M * a->D > ((int64_t)1 << 31) - 1) return MOPK_ERR_UNSUPPORTED;
    if (a->precision == MOPK_PREC_FP32 && (a->x_dtype | a->w_dtype | a->o_dtype) != MOPK_F32) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(15, a->x, a->residual, a->y, a->u, a->h, a->dy, a->dx, a->route, a->workspace)) return MOPK_ERR_UNSUPPORTED;
    for (int e = 0; e < a->E; ++e)
        if (misaligned(15, a->w1[e], a->w2[e], a->dw1[e], a->dw2[e])) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <int MODE, bool BF16, int TM, int TN>
void moe_gemm(const MopkMoeArgs *a, int chunk, float *slab, hipStream_t st) {
    dim3 grid;
    if (MODE >= WG2) {
        const int I = MODE == WG2 ? a->D : a->F, J = MODE == WG2 ? a->F : a->D;
        grid = dim3((unsigned)(((I + TM - 1) / TM) * ((J + TN - 1) / TN)), (unsigned)moe_tiles_bound(a->M, a->E, chunk));
    } else {
        const int N = (MODE == FC1 || MODE == DU) ? a->F : a->D;
        grid = dim3((unsigned)moe_tiles_bound(a->M, a->E, TM), (unsigned)((N + TN - 1) / TN));
    }
    hipLaunchKernelGGL((moe_gemm_kernel<MODE, BF16, TM, TN>), grid, dim3(256), 0, st, *a, chunk, slab);
}

// tiles: bf16 128 x 128 where the output is F wide (FC1, DU) and for the weight gradients, 64 x 64 where it is D wide (FC2, DX:
// four times the workgroups at D = 384); fp32 64 x 64 throughout (LDS and registers of the fp32 operand images)
template <int MODE>
void moe_gemm_p(const MopkMoeArgs *a, int chunk, float *slab, hipStream_t st) {
    constexpr bool WIDE = MODE == FC1 || MODE == DU || MODE >= WG2;
    if (a->precision == MOPK_PREC_BF16) {
        if (WIDE) moe_gemm<MODE, true, 128, 128>(a, chunk, slab, st);
        else moe_gemm<MODE, true, 64, 64>(a, chunk, slab, st);
    } else {
        moe_gemm<MODE, false, 64, 64>(a, chunk, slab, st);
    }
}

int moe_route(const MopkMoeArgs *a, hipStream_t st) {
    hipLaunchKernelGGL(moe_logits_kernel, dim3((unsigned)((a->M + 3) / 4)), dim3(256), 0, st, *a);
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(MOE_SCAN_THREADS), 0, st, *a);
    return launch_status();
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_moe_supported(const MopkMoeArgs *a) { return moe_check(a) == MOPK_OK; }

size_t mopk_moe_workspace_bytes(const MopkMoeArgs *a, int backward) {
    if (!a || a->M <= 0 || a->D <= 0 || a->F <= 0 || a->E < 2 || a->E > MOPK_MOE_MAX_EXPERTS) return 0;
    if (!backward) return 0;
    return moe_du_bytes(a) + 2 * moe_slab_bytes(a);
}

int mopk_moe_route(const MopkMoeArgs *a, void *stream) {
    const int rc = moe_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->gate_w, a->route)) return MOPK_ERR_BAD_ARG;
    return moe_route(a, (hipStream_t)stream);
}

int mopk_moe_fwd(const MopkMoeArgs *a, void *stream) {
    const int rc = moe_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->gate_w, a->route, a->u, a->h, a->y)) return MOPK_ERR_BAD_ARG;
    for (int e = 0; e < a->E; ++e)
        if (any_null(a->w1[e], a->w2[e])) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (moe_route(a, st) != MOPK_OK) return MOPK_ERR_LAUNCH;
    moe_gemm_p<FC1>(a, 0, nullptr, st);
    moe_gemm_p<FC2>(a, 0, nullptr, st);
    return launch_status();
}

int mopk_moe_bwd(const MopkMoeArgs *a, void *stream) {
    const int rc = moe_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->x, a->route, a->u, a->h, a->dy, a->dx, a->workspace)) return MOPK_ERR_BAD_ARG;
    for (int e = 0; e < a->E; ++e)
        if (any_null(a->w1[e], a->w2[e], a->dw1[e], a->dw2[e])) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int chunk = moe_chunk(a->M);
    float *slab1 = (float *)((char *)a->workspace + moe_du_bytes(a));
    float *slab2 = (float *)((char *)slab1 + moe_slab_bytes(a));
    moe_gemm_p<DU>(a, chunk, nullptr, st);         // dU -> workspace[0, du_bytes)
    moe_gemm_p<DX>(a, chunk, nullptr, st);
    moe_gemm_p<WG2>(a, chunk, slab2, st);
    moe_gemm_p<WG1>(a, chunk, slab1, st);
    const int64_t n = (int64_t)a->D * a->F;
    hipLaunchKernelGGL(moe_wsum_kernel, dim3((unsigned)((n / 4 + 255) / 256), (unsigned)a->E, 2), dim3(256), 0, st, *a, chunk,
                       (const float *)slab1, (const float *)slab2);
    return launch_status();
}

}  // extern "C"
