// Language detection on last-position logits (WhisperMoP.detect_language and transcribe with `languages`; inference only): the
// softmax over the n language tokens' logits of each row and the most probable language token (mopk_language_probs; Whisper's
// detect_language after its mask).  include/mopk.h states it.  One launch, one workgroup of 256 threads per row, static LDS, no
// atomics, no workspace, no host synchronisation.
//
// It is a gather of at most 1024 scalars per row: a thread reads up to four of them (entries tid, tid + 256, ...) and keeps them
// in registers for the second step, so a logit is read once.  A thread merges what it reads into its (max, sum-exp) pair and its
// best (value, token id); ranking by row_before is a total order, so the argmax does not depend on who read what, and the pairs
// are merged in a fixed order (wave shuffles, then the waves in order): results are bitwise reproducible.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_WAVES = LG_THREADS / WAVE;
constexpr int LG_PER = MOPK_LANGUAGE_MAX_N / LG_THREADS;        // entries per thread
constexpr int LG_NONE = 0x7fffffff;                             // id of "no entry yet": every real id ranks before it
static_assert(LG_PER * LG_THREADS == MOPK_LANGUAGE_MAX_N, "a thread's share covers the table");

struct LgLds {
    float wm[LG_WAVES], wl[LG_WAVES], ws[LG_WAVES];
    int wi[LG_WAVES];
};

template <typename T>
__global__ __launch_bounds__(LG_THREADS) void lg_row_kernel(MopkLanguageProbsArgs a) {
    __shared__ LgLds s;
    const int r = blockIdx.x, V = a.V, n = a.n, tid = threadIdx.x;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    float f[LG_PER];
    float m = -INFINITY, l = 0.f, bs = -INFINITY;
    int bi = LG_NONE;
#pragma unroll
    for (int k = 0; k < LG_PER; ++k) {
        const int i = tid + k * LG_THREADS;
        f[k] = -INFINITY;
        if (i < n) {
            const int t = min(max(a.ids[i], 0), V - 1);         // no read leaves the row
            f[k] = ld_as_f32<T>(x + t);
            row_lse_add(m, l, f[k]);
            if (row_before(f[k], t, bs, bi)) { bs = f[k]; bi = t; }
        }
    }
    // block-wide merge: shuffles inside a wave, then the wave results in wave order (every thread gets the result)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        row_lse_merge(m, l, __shfl_xor(m, o, 64), __shfl_xor(l, o, 64));
        const float s2 = __shfl_xor(bs, o, 64);
        const int i2 = __shfl_xor(bi, o, 64);
        if (row_before(s2, i2, bs, bi)) { bs = s2; bi = i2; }
    }
    const int w = tid / WAVE;
    if ((tid & 63) == 0) { s.wm[w] = m; s.wl[w] = l; s.ws[w] = bs; s.wi[w] = bi; }
    __syncthreads();
    m = s.wm[0];
    l = s.wl[0];
    bs = s.ws[0];
    bi = s.wi[0];
#pragma unroll
    for (int i = 1; i < LG_WAVES; ++i) {
        row_lse_merge(m, l, s.wm[i], s.wl[i]);
        if (row_before(s.ws[i], s.wi[i], bs, bi)) { bs = s.ws[i]; bi = s.wi[i]; }
    }
    const float lse = m + logf(l);
    float *p = a.probs + (int64_t)r * a.probs_ld;
#pragma unroll
    for (int k = 0; k < LG_PER; ++k) {
        const int i = tid + k * LG_THREADS;
        if (i < n) p[i] = expf(f[k] - lse);
    }
    // bi == LG_NONE is only reachable with NaN logits: the first language stands in
    if (tid == 0) a.tokens[r] = bi != LG_NONE ? bi : min(max(a.ids[0], 0), V - 1);
}

int lg_check(const MopkLanguageProbsArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->V < 2 || a->n < 1 || a->n > MOPK_LANGUAGE_MAX_N) return MOPK_ERR_BAD_SHAPE;
    if (a->dtype != MOPK_F32 && a->dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->logits_ld < a->V || a->probs_ld < a->n) return MOPK_ERR_BAD_ARG;
    if (misaligned(a->dtype == MOPK_BF16 ? 1 : 3, a->logits)) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(3, a->ids, a->probs, a->tokens)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_language_probs_supported(const MopkLanguageProbsArgs *a) { return lg_check(a) == MOPK_OK; }

int mopk_language_probs(const MopkLanguageProbsArgs *a, void *stream) {
    const int rc = lg_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->ids, a->probs, a->tokens)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((lg_row_kernel<unsigned short>), dim3((unsigned)a->R), dim3(LG_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((lg_row_kernel<float>), dim3((unsigned)a->R), dim3(LG_THREADS), 0, st, *a);
    return launch_status();
}

}  // extern "C"
