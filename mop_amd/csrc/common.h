// Shared device helpers for libmopk (gfx950 only); the host side of a launch is host_launch.h, included at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mopk.h"

namespace mopk {

typedef __attribute__((ext_vector_type(8))) short bf16x8;   // MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;    // 16x16 accumulator
typedef __attribute__((ext_vector_type(16))) float f32x16;  // 32x32 accumulator

constexpr int WAVE = 64;

__device__ __forceinline__ unsigned short f2bf(float f) {
    // round-to-nearest-even; plain cast keeps NaN a NaN (v_cvt_pk_bf16_f32 at -O3)
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short u) {
    return __builtin_bit_cast(float, ((unsigned int)u) << 16);
}
// pack two floats into one dword of 2 x bf16 (lo = a, hi = b)
__device__ __forceinline__ unsigned int pack_bf16(float a, float b) {
    return (unsigned int)f2bf(a) | ((unsigned int)f2bf(b) << 16);
}

template <typename T> __device__ __forceinline__ float ld_as_f32(const T *p);
template <> __device__ __forceinline__ float ld_as_f32<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float ld_as_f32<unsigned short>(const unsigned short *p) {
    return bf2f(*p);
}
template <typename T> __device__ __forceinline__ void st_from_f32(T *p, float v);
template <> __device__ __forceinline__ void st_from_f32<float>(float *p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_from_f32<unsigned short>(unsigned short *p, float v) {
    *p = f2bf(v);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// Natural logarithm of an argument that is known to be a NORMAL positive float: x >= 2^-126, finite or +inf (NaN stays NaN).
// __logf() guards v_log_f32 against subnormal arguments (compare, two selects, v_ldexp_f32: five instructions around the
// logarithm) and ends in fma(log2 x, ln 2, 0 or -32 ln 2); with the guard never taken that is this product, bit for bit.
// The product is made opaque, so -ffast-math cannot contract it into a consumer's add or re-associate it with a consumer's
// multiply: callers get the value __logf() gave them.  Every call site states why its argument cannot be subnormal.
__device__ __forceinline__ float log_pos(float x) {
    float v = __builtin_amdgcn_logf(x) * 0.6931471805599453f;
    asm("" : "+v"(v));
    return v;
}
// max(a, b) as ONE v_max_f32.  fmaxf() quiets signalling NaNs first (a `v_max_f32 x, x, x` in front of every operand the
// compiler cannot prove canonical: loop-carried values, matrix-core results); the hardware instruction returns the other
// operand for a quiet NaN exactly like fmaxf(), so the results differ only for a SIGNALLING NaN operand, which no
// arithmetic instruction produces.  The compiler pads no hazards of an asm statement: BOTH OPERANDS MUST COME FROM AN
// ORDINARY VALU INSTRUCTION (or from another vmax) -- never straight from an MFMA or from v_exp / v_log / v_rcp -- and the
// result must go to ordinary VALU code, not into an MFMA operand.
__device__ __forceinline__ float vmax(float a, float b) {
    asm("v_max_f32 %0, %0, %1" : "+v"(a) : "v"(b));
    return a;
}
// max(m, x[0], .., x[15]) as eight v_max3_f32 in ONE statement (between two dependent asm statements the compiler pads a wait
// state; inside one the hardware interlocks).  NaN handling and operand contract as vmax.
__device__ __forceinline__ float vmax16(float m, const f32x16 &x) {
    asm("v_max3_f32 %0, %0, %1, %2\n\tv_max3_f32 %0, %0, %3, %4\n\tv_max3_f32 %0, %0, %5, %6\n\tv_max3_f32 %0, %0, %7, %8\n\t"
        "v_max3_f32 %0, %0, %9, %10\n\tv_max3_f32 %0, %0, %11, %12\n\tv_max3_f32 %0, %0, %13, %14\n\tv_max3_f32 %0, %0, %15, %16"
        : "+v"(m)
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(x[8]), "v"(x[9]), "v"(x[10]),
          "v"(x[11]), "v"(x[12]), "v"(x[13]), "v"(x[14]), "v"(x[15]));
    return m;
}
// key / value length of a plain SDPA call: N queries attend to Nk keys (cross-attention); Nk = 0 means N (square)
__host__ __device__ inline int sdpa_nk(const MopkSdpaArgs &a) { return a.Nk > 0 ? a.Nk : a.N; }
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- attention dropout: counter-based keep mask, a pure function of (seed, b*H+h, query, key) -- evaluated again in the backward
__host__ __device__ inline uint32_t fa_hash(uint32_t x) {          // "lowbias32" integer finalizer
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
struct FaDrop { uint32_t thresh, seed_lo, seed_hi; float inv_keep; };      // thresh == 0: dropout off
__host__ __device__ inline FaDrop fa_drop(float p, uint64_t seed) {
    FaDrop d{0u, (uint32_t)seed, (uint32_t)(seed >> 32), 1.f};
    if (p > 0.f) {
        const double t = (double)p * 4294967296.0;
        d.thresh = t >= 4294967295.0 ? 0xffffffffu : (t < 1.0 ? 1u : (uint32_t)t);
        d.inv_keep = 1.f / (1.f - p);
    }
    return d;
}
__host__ __device__ inline uint32_t fa_drop_row(const FaDrop &d, int bh, int i) {
    return fa_hash((uint32_t)i * 0x9E3779B1u + (uint32_t)bh * 0x85EBCA77u + d.seed_hi) ^ d.seed_lo;
}
__host__ __device__ inline bool fa_drop_keep(const FaDrop &d, uint32_t rowh, int j) {
    return fa_hash(rowh ^ ((uint32_t)j * 0xC2B2AE3Du)) >= d.thresh;
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// bump allocator over a caller-provided buffer (256-byte aligned carve-outs)
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *p) : base((char *)p) {}
    template <typename T> T *take(size_t n) {
        size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
        T *r = base ? (T *)(base + off) : nullptr;
        off += bytes;
        return r;
    }
};

}  // namespace mopk

#include "host_launch.h"   // every unit here holds both kernels and their entry points
