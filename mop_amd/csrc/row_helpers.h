// Helpers of the kernels that walk a row of logits or of a key / value cache (beam_search.hip, sample.hip, logit_rules.hip,
// decode_attn.hip): their bitwise-reproducibility claims rest on all of them doing these steps the same way, so each is here once.
#pragma once
#include "common.h"

namespace mopk {

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

}  // namespace mopk
