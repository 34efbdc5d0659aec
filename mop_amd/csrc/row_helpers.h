// Helpers of the kernels that walk a row of logits or of a key / value cache (beam_search.hip, sample.hip, logit_rules.hip,
// repeat_rules.hip, token_logprob.hip, language.hip, decode_attn.hip): their bitwise-reproducibility claims rest on all of them doing
// these steps the same way, so each is here once.  That includes the order in which a workgroup merges its threads' results: the
// shuffle tree inside a wave (row_wave_*), then the waves in wave order (Row*Lds).  A kernel whose results rest on another order
// (beam_search.hip's pairwise trees through LDS) keeps it in its own file and says so.
#pragma once
#include "common.h"

namespace mopk {

constexpr int ROW_NONE = 0x7fffffff;                            // index of "no element yet": every real index ranks before it (row_before)

template <typename T> __device__ __forceinline__ T row_ninf();  // -inf in the row's element type
template <> __device__ __forceinline__ float row_ninf<float>() { return -INFINITY; }
template <> __device__ __forceinline__ unsigned short row_ninf<unsigned short>() { return 0xFF80; }

// online (max, sum-exp) of a row: add one element (-inf entries add nothing; m = -inf: l = 0 * 0 + 1) ...
__device__ __forceinline__ void row_lse_add(float &m, float &l, float f) {
    if (f > m) { l = l * expf(m - f) + 1.f; m = f; }
    else if (f != -INFINITY) l += expf(f - m);
}
// ... and merge a second pair (m2, l2) into (m, l)
__device__ __forceinline__ void row_lse_merge(float &m, float &l, float m2, float l2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;
    l = (m == -INFINITY ? 0.f : l * expf(m - M)) + (m2 == -INFINITY ? 0.f : l2 * expf(m2 - M));
    m = M;
}

// (as, ai) ranks before (bs, bi): larger score, ties to the smaller index
__device__ __forceinline__ bool row_before(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

// 16 bytes -> 8 bf16 or 4 fp32 widened to fp32 (the tag argument picks the element type)
__device__ __forceinline__ void row_unpack(const uint4 &u, float (&f)[8], unsigned short) {
    const unsigned int w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __builtin_bit_cast(float, w[i] << 16);
        f[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ void row_unpack(const uint4 &u, float (&f)[4], float) {
    f[0] = __builtin_bit_cast(float, u.x); f[1] = __builtin_bit_cast(float, u.y);
    f[2] = __builtin_bit_cast(float, u.z); f[3] = __builtin_bit_cast(float, u.w);
}

// Row x[0, V) read in 16-byte vectors (a row may start at any element): elements [0, head) lie before the row's first 16-byte
// boundary (all of a row that ends before it), nvec vectors of EPV elements start at x + head, [tail0, V) lie behind the last.
template <typename T>
struct RowSpan {
    static constexpr int EPV = 16 / (int)sizeof(T);
    int head, nvec, tail0;
    __device__ __forceinline__ RowSpan(const T *x, int V) {
        head = min((int)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(T)), V);
        nvec = (V - head) / EPV;
        tail0 = head + nvec * EPV;
    }
};

// Workgroup-wide merges, in two steps with the kernel's own __syncthreads() between them (a kernel that merges both kinds pays one
// barrier).  Step 1, inside a wave: the xor-shuffle tree with offsets 32, 16, ... 1; every lane gets the wave's result.
__device__ __forceinline__ void row_best_xor(float &s, int &i, int o) {
    const float s2 = __shfl_xor(s, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (row_before(s2, i2, s, i)) { s = s2; i = i2; }
}
// A kernel that merges two quantities runs one tree for both, so that a level's shuffles travel together: one tree after the other
// cost gp_row_kernel 0.6 % and lr_row_kernel 1.2 %.  logit_rules.hip, which pairs lse with a maximum, has that loop.
__device__ __forceinline__ void row_wave_lse(float &m, float &l) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) row_lse_merge(m, l, __shfl_xor(m, o, 64), __shfl_xor(l, o, 64));
}
__device__ __forceinline__ void row_wave_best(float &s, int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) row_best_xor(s, i, o);
}
__device__ __forceinline__ void row_wave_lse_best(float &m, float &l, float &s, int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { row_lse_merge(m, l, __shfl_xor(m, o, 64), __shfl_xor(l, o, 64)); row_best_xor(s, i, o); }
}
// Step 2, across the workgroup's NW waves, through LDS: lane 0 of each wave put()s its wave's result, the kernel's barrier follows,
// and every thread get()s waves 0 .. NW - 1 merged in that order.  A kernel that reuses the LDS adds a barrier behind get().
template <int NW>
struct RowLseLds {
    float wm[NW], wl[NW];
    __device__ __forceinline__ void put(float m, float l) {
        if ((threadIdx.x & (WAVE - 1)) == 0) { wm[threadIdx.x / WAVE] = m; wl[threadIdx.x / WAVE] = l; }
    }
    __device__ __forceinline__ void get(float &m, float &l) const {
        m = wm[0];
        l = wl[0];
        for (int w = 1; w < NW; ++w) row_lse_merge(m, l, wm[w], wl[w]);
    }
};
template <int NW>
struct RowBestLds {
    float ws[NW];
    int wi[NW];
    __device__ __forceinline__ void put(float s, int i) {
        if ((threadIdx.x & (WAVE - 1)) == 0) { ws[threadIdx.x / WAVE] = s; wi[threadIdx.x / WAVE] = i; }
    }
    __device__ __forceinline__ void get(float &s, int &i) const {
        s = ws[0];
        i = wi[0];
        for (int w = 1; w < NW; ++w)
            if (row_before(ws[w], wi[w], s, i)) { s = ws[w]; i = wi[w]; }
    }
};

}  // namespace mopk
