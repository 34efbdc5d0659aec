// Temperature / top-k / top-p sampling of one token per row (WhisperMoP.sample; inference only).  One launch, one workgroup of
// 1024 threads per row, no atomics whose order can change a result, no host synchronisation: the position is read from device
// memory, so one set of launch arguments serves every step and a step can be captured once in a HIP graph.
//
// Each pass streams the row (thread t reads elements v = t + 1024 i) and recomputes z = x * inv_temp; the row (104 KB in bf16 at
// V = 51865) stays in L2 between passes.  Pass 1 merges the unscaled (max, sum-exp) for the log-probability and the min / max key.
// The filters are thresholds on the order-preserving uint32 key of z, found by a radix walk: each level histograms the keys inside
// the current window [lo, hi] into <= 256 power-of-two bins (LDS integer atomics: counts for top-k, fixed-point masses
// exp(z - max z) * 2^40 for top-p, both order-independent sums), one wave scans the bins from the top to find the bin where the
// running total reaches the target, and the window shrinks to that bin; at most four levels reach a single key.  The draw is a
// Gumbel-max over the kept set with a counter-based hash, so it needs no prefix scan.  Every block reduction has a fixed order:
// tokens and log-probabilities are bitwise reproducible.
//
// Ragged batches (mopk_sample_ragged_*): OFF = true draws row r at position *pos - pos_off[r], the row's own token index in a
// left-padded batch; nothing else changes.  That instantiation is compiled in a unit of its own (-DMOPK_SAMPLE_RAGGED, a second
// object of this file), so the OFF = false kernel's code is the same as before the flag existed.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int SP_THREADS = 1024;
constexpr int SP_WAVES = SP_THREADS / WAVE;
constexpr int SP_BINS = 256;
#define SP_UNROLL 16                                            // loads in flight per thread: each pass is bound by L2 latency
constexpr float SP_MASS_SCALE = 1099511627776.f;               // 2^40: masses sum exactly in 64 bits for V <= 2^24

__device__ __forceinline__ uint32_t sp_row_hash(uint64_t seed, int r, int pos) {
    return fa_hash(fa_hash((uint32_t)seed ^ (uint32_t)r * 0x9E3779B1u) ^ (uint32_t)(seed >> 32) ^ (uint32_t)pos * 0x85EBCA77u);
}
// Gumbel noise of element v: u is an odd multiple of 2^-24 in (0, 1), exact in fp32 (a 24-bit form would round its top values to 1)
__device__ __forceinline__ float sp_gumbel(uint32_t rh, int v) {
    const uint32_t h = fa_hash(rh ^ (uint32_t)v * 0xC2B2AE3Du);
    const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}
// order-preserving key: a < b as floats <=> key(a) < key(b); -0 is folded into +0 first
__device__ __forceinline__ uint32_t sp_key(float z) {
    const uint32_t u = __float_as_uint(z == 0.f ? 0.f : z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t sp_mass(float z, float mz) { return (uint64_t)(expf(z - mz) * SP_MASS_SCALE); }

struct SpLds {
    uint64_t hist[SP_BINS];
    union {                                                     // used one after the other: a barrier follows every get()
        RowLseLds<SP_WAVES> lse;
        RowBestLds<SP_WAVES> best;
    };
    uint64_t wu[SP_WAVES];
    uint32_t wk[SP_WAVES], wk2[SP_WAVES];
    uint32_t sel, exact;
    uint64_t above;
};

// block-wide reductions: shuffles inside a wave, then the SP_WAVES wave results in wave order (every thread gets the result);
// row_helpers.h has the (max, sum-exp) and best (score, index) ones
__device__ __forceinline__ uint64_t sp_block_sum(uint64_t x, SpLds &s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0) s.wu[threadIdx.x / WAVE] = x;
    __syncthreads();
    x = 0;
    for (int i = 0; i < SP_WAVES; ++i) x += s.wu[i];
    __syncthreads();
    return x;
}
__device__ __forceinline__ void sp_block_minmax(uint32_t &lo, uint32_t &hi, SpLds &s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor(lo, o, 64));
        hi = max(hi, (uint32_t)__shfl_xor(hi, o, 64));
    }
    const int w = threadIdx.x / WAVE;
    if ((threadIdx.x & 63) == 0) { s.wk[w] = lo; s.wk2[w] = hi; }
    __syncthreads();
    for (int i = 0; i < SP_WAVES; ++i) { lo = min(lo, s.wk[i]); hi = max(hi, s.wk2[i]); }
    __syncthreads();
}

template <typename T>
struct SpRow {                                                  // one logit row; z(v) = x_v * inv_temp (x_v when greedy)
    const T *x;
    int V;
    float it;
    bool greedy;
    __device__ __forceinline__ float x_at(int v) const { return ld_as_f32<T>(x + v); }
    __device__ __forceinline__ float z(int v) const { return greedy ? x_at(v) : x_at(v) * it; }
};

// the largest key t in [lo, hi] with (weight of the keys >= t) >= target, where weight = 1 per element (MASS = false) or the
// element's fixed-point mass (MASS = true; mz = max z).  The caller guarantees that the total weight in [lo, hi] reaches target.
template <bool MASS, typename T>
__device__ __forceinline__ uint32_t sp_select(const SpRow<T> &row, uint32_t lo, uint32_t hi, uint64_t target, float mz, SpLds &s) {
    const int tid = threadIdx.x;
    uint64_t above = 0;                                         // weight of the keys above the window
    for (;;) {
        const uint32_t span = hi - lo;
        const int bits = span ? 32 - __clz(span) : 0;
        const int sh = bits > 8 ? bits - 8 : 0;                 // (span >> sh) < 256
        if (tid < SP_BINS) s.hist[tid] = 0;
        if (tid == 0) { s.sel = 0; s.above = above; s.exact = 0; }     // never used: some bin always reaches the target
        __syncthreads();
#pragma unroll SP_UNROLL
        for (int v = tid; v < row.V; v += SP_THREADS) {
            const float z = row.z(v);
            const uint32_t k = sp_key(z);
            if (k >= lo && k <= hi) {
                const uint64_t w = MASS ? sp_mass(z, mz) : 1;
                if (w) atomicAdd((unsigned long long *)&s.hist[(k - lo) >> sh], (unsigned long long)w);
            }
        }
        __syncthreads();
        if (tid < WAVE) {                                       // lane l owns bins 4l .. 4l + 3; suffix sums from bin 255 down
            uint64_t h[4], own = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = s.hist[4 * tid + j]; own += h[j]; }
            uint64_t incl = own;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint64_t t = __shfl_down(incl, o, 64);
                if (tid + o < WAVE) incl += t;
            }
            uint64_t cum = above + incl - own;                  // weight above this lane's bins
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                if (cum < target && cum + h[j] >= target) { s.sel = 4 * tid + j; s.above = cum; s.exact = cum + h[j] == target; }
                cum += h[j];
            }
        }
        __syncthreads();
        const uint32_t b = s.sel;
        const bool exact = !MASS && s.exact;                    // the bin's elements are exactly the last ones counted: key >= its
        above = s.above;                                        // lower edge keeps the same set as its smallest key
        __syncthreads();                                        // every thread has read sel / above before the next level
        const uint64_t nlo = (uint64_t)lo + ((uint64_t)b << sh);
        const uint64_t nhi = nlo + (((uint64_t)1 << sh) - 1);
        if (sh == 0 || exact) return (uint32_t)nlo;
        lo = (uint32_t)nlo;
        hi = nhi < hi ? (uint32_t)nhi : hi;
    }
}

// OFF: row r draws at *pos - pos_off[r] (a ragged batch); else at *pos
template <typename T, bool OFF>
__global__ __launch_bounds__(SP_THREADS) void sp_row_kernel(MopkSampleArgs a, const int32_t *pos_off) {
    __shared__ SpLds s;
    const int tid = threadIdx.x, r = blockIdx.x, V = a.V;
    const int item = r / a.n, sub = r - item * a.n;
    const SpRow<T> row{(const T *)a.logits + (int64_t)item * a.logits_sb + (int64_t)sub * a.logits_sk, V, a.inv_temp, a.greedy != 0};

    // pass 1: unscaled (max, sum-exp); greedy: the argmax; else the key range
    float m0 = -INFINITY, l0 = 0.f, best = -INFINITY;
    int bv = ROW_NONE;
    uint32_t thr = 0xffffffffu, kmax = 0;                       // kept: key(z) >= thr (all of [0, V) before any filter)
#pragma unroll SP_UNROLL
    for (int v = tid; v < V; v += SP_THREADS) {
        const float f = row.x_at(v);
        row_lse_add(m0, l0, f);
        if (row.greedy) {
            if (f > best || bv == ROW_NONE) { best = f; bv = v; }         // v rises: the first maximum of this thread
        } else {
            const uint32_t k = sp_key(f * row.it);
            thr = min(thr, k);
            kmax = max(kmax, k);
        }
    }
    row_wave_lse(m0, l0);
    s.lse.put(m0, l0);
    __syncthreads();
    s.lse.get(m0, l0);
    __syncthreads();
    if (!row.greedy) {
        sp_block_minmax(thr, kmax, s);
        if (a.top_k > 0 && a.top_k < V) thr = sp_select<false>(row, thr, kmax, (uint64_t)a.top_k, 0.f, s);
        const float mz = m0 * row.it;                           // max z = z of the max logit (x -> x * inv_temp is monotone)
        if (a.top_p < 1.f && mz != -INFINITY) {
            uint64_t q = 0;
#pragma unroll SP_UNROLL
            for (int v = tid; v < V; v += SP_THREADS) {
                const float z = row.z(v);
                if (sp_key(z) >= thr) q += sp_mass(z, mz);
            }
            const uint64_t Q = sp_block_sum(q, s);
            const uint64_t P = (uint64_t)ceil((double)a.top_p * (double)Q);
            thr = sp_select<true>(row, thr, kmax, P, mz, s);
        }
        // the draw: Gumbel-max over the kept set
        uint32_t rh;
        if constexpr (OFF) rh = sp_row_hash(a.seed, r, *a.pos - pos_off[r]);
        else rh = sp_row_hash(a.seed, r, *a.pos);
#pragma unroll SP_UNROLL
        for (int v = tid; v < V; v += SP_THREADS) {
            const float z = row.z(v);
            if (sp_key(z) >= thr) {
                const float sc = z + sp_gumbel(rh, v);
                if (row_before(sc, v, best, bv)) { best = sc; bv = v; }
            }
        }
    }
    row_wave_best(best, bv);
    s.best.put(best, bv);
    __syncthreads();
    s.best.get(best, bv);
    __syncthreads();
    if (bv >= V) bv = 0;                                        // only reachable with NaN logits: keep the read inside the row
    if (tid == 0) {
        a.tokens[r] = bv;
        a.logprobs[r] = row.x_at(bv) - (m0 + logf(l0));
    }
}

int sp_check(const MopkSampleArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->n <= 0 || a->V < 2) return MOPK_ERR_BAD_SHAPE;
    if (a->V > MOPK_SAMPLE_MAX_V) return MOPK_ERR_UNSUPPORTED;
    if (a->logits_dtype != MOPK_F32 && a->logits_dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->logits_sb < 0 || a->logits_sk < 0) return MOPK_ERR_BAD_ARG;
    if (a->greedy != 0 && a->greedy != 1) return MOPK_ERR_BAD_ARG;
    if (!a->greedy) {
        if (!(a->inv_temp > 0.f) || a->inv_temp == INFINITY) return MOPK_ERR_BAD_ARG;
        if (a->top_k < 0 || !(a->top_p > 0.f) || !(a->top_p <= 1.f)) return MOPK_ERR_BAD_ARG;
    }
    const int es = a->logits_dtype == MOPK_BF16 ? 2 : 4;
    if (misaligned(es - 1, a->logits)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

#ifdef MOPK_SAMPLE_RAGGED
int sp_ragged_check(const MopkSampleRaggedArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    const int rc = sp_check(&a->base);
    if (rc != MOPK_OK) return rc;
    if (!a->pos_off) return MOPK_ERR_BAD_ARG;
    if (misaligned(3, a->pos_off)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}
#endif

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

#ifndef MOPK_SAMPLE_RAGGED
int mopk_sample_supported(const MopkSampleArgs *a) { return sp_check(a) == MOPK_OK; }

size_t mopk_sample_workspace_bytes(const MopkSampleArgs *a) {
    (void)a;
    return 0;
}

int mopk_sample_step(const MopkSampleArgs *a, void *stream) {
    const int rc = sp_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->pos, a->tokens, a->logprobs)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->logits_dtype == MOPK_BF16)
        hipLaunchKernelGGL((sp_row_kernel<unsigned short, false>), dim3((unsigned)a->R), dim3(SP_THREADS), 0, st, *a, nullptr);
    else hipLaunchKernelGGL((sp_row_kernel<float, false>), dim3((unsigned)a->R), dim3(SP_THREADS), 0, st, *a, nullptr);
    return launch_status();
}
#else   // the ragged exports: this file compiled a second time with -DMOPK_SAMPLE_RAGGED (mop_amd/build.py)
int mopk_sample_ragged_supported(const MopkSampleRaggedArgs *a) { return sp_ragged_check(a) == MOPK_OK; }

size_t mopk_sample_ragged_workspace_bytes(const MopkSampleRaggedArgs *a) {
    return sp_ragged_check(a) == MOPK_OK ? mopk_sample_workspace_bytes(&a->base) : 0;
}

int mopk_sample_ragged_step(const MopkSampleRaggedArgs *a, void *stream) {
    const int rc = sp_ragged_check(a);
    if (rc != MOPK_OK) return rc;
    const MopkSampleArgs *b = &a->base;
    if (any_null(b->logits, b->pos, b->tokens, b->logprobs)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (b->logits_dtype == MOPK_BF16)
        hipLaunchKernelGGL((sp_row_kernel<unsigned short, true>), dim3((unsigned)b->R), dim3(SP_THREADS), 0, st, *b, a->pos_off);
    else hipLaunchKernelGGL((sp_row_kernel<float, true>), dim3((unsigned)b->R), dim3(SP_THREADS), 0, st, *b, a->pos_off);
    return launch_status();
}
#endif

}  // extern "C"
