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
static_assert(LG_PER * LG_THREADS == MOPK_LANGUAGE_MAX_N, "a thread's share covers the table");

template <typename T>
__global__ __launch_bounds__(LG_THREADS) void lg_row_kernel(MopkLanguageProbsArgs a) {
    __shared__ RowLseLds<LG_WAVES> sl;
    __shared__ RowBestLds<LG_WAVES> sb;
    const int r = blockIdx.x, V = a.V, n = a.n, tid = threadIdx.x;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    float f[LG_PER];
    float m = -INFINITY, l = 0.f, bs = -INFINITY;
    int bi = ROW_NONE;                                          // a token id here: every real id ranks before it
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
    row_wave_lse_best(m, l, bs, bi);
    sl.put(m, l);
    sb.put(bs, bi);
    __syncthreads();
    sl.get(m, l);
    sb.get(bs, bi);
    const float lse = m + logf(l);
    float *p = a.probs + (int64_t)r * a.probs_ld;
#pragma unroll
    for (int k = 0; k < LG_PER; ++k) {
        const int i = tid + k * LG_THREADS;
        if (i < n) p[i] = expf(f[k] - lse);
    }
    // bi == ROW_NONE is only reachable with NaN logits: the first language stands in
    if (tid == 0) a.tokens[r] = bi != ROW_NONE ? bi : min(max(a.ids[0], 0), V - 1);
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
