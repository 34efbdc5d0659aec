// Per-step decoding statistics on last-position logits (WhisperMoP's return_stats and the temperature fallback / no-speech skip of
// transcribe; inference only): the log-probability of one token per row (mopk_token_logprob) and one greedy decoding step on device
// state (mopk_greedy_pick: argmax, log-probability sum, length, eos bookkeeping and the history column).  include/mopk.h states
// both.  One launch, one workgroup of 1024 threads per row, static LDS, no atomics, no host synchronisation: the position is read
// from device memory, so one set of launch arguments serves every step and a step can be captured once in a HIP graph.
//
// One pass streams the row in 16-byte loads: the elements before the row's first 16-byte boundary and behind its last whole
// vector are read one by one (a row may start at any element).  A thread merges what it reads into its (max, sum-exp) pair and its
// best (value, index); ranking by row_before is a total order, so the argmax does not depend on who read what, and the pairs are
// merged in a fixed order (wave shuffles, then the waves in order): results are bitwise reproducible.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int TL_THREADS = 1024;
constexpr int TL_WAVES = TL_THREADS / WAVE;

// this thread's share of row x[0, V): (m, l) and, with BEST, the best (bs, bi)
template <typename T, bool BEST>
__device__ __forceinline__ void tl_scan(const T *x, int V, float &m, float &l, float &bs, int &bi) {
    constexpr int EPV = RowSpan<T>::EPV;
    const int tid = threadIdx.x;
    const RowSpan<T> sp(x, V);
    const int head = sp.head, tail0 = sp.tail0;                 // head + (V - tail0) < 2 * EPV scalar elements
    const uint4 *xv = (const uint4 *)(x + head);
#pragma unroll 4
    for (int u = tid; u < sp.nvec; u += TL_THREADS) {
        float f[EPV];
        row_unpack(xv[u], f, T());
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            row_lse_add(m, l, f[e]);
            if (BEST && row_before(f[e], head + u * EPV + e, bs, bi)) { bs = f[e]; bi = head + u * EPV + e; }
        }
    }
    if (tid < head + (V - tail0)) {
        const int e = tid < head ? tid : tail0 + (tid - head);
        const float f = ld_as_f32<T>(x + e);
        row_lse_add(m, l, f);
        if (BEST && row_before(f, e, bs, bi)) { bs = f; bi = e; }
    }
}

template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tl_row_kernel(MopkTokenLogprobArgs a) {
    __shared__ RowLseLds<TL_WAVES> s;
    const int r = blockIdx.x, V = a.V;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    float m = -INFINITY, l = 0.f, bs = -INFINITY;
    int bi = ROW_NONE;
    tl_scan<T, false>(x, V, m, l, bs, bi);
    row_wave_lse(m, l);
    s.put(m, l);
    __syncthreads();
    s.get(m, l);
    if (threadIdx.x == 0) {
        const int t = min(max(a.tokens ? a.tokens[r] : a.token, 0), V - 1);        // no read leaves the row
        a.out[r] = ld_as_f32<T>(x + t) - (m + logf(l));
    }
}

template <typename T>
__global__ __launch_bounds__(TL_THREADS) void gp_row_kernel(MopkGreedyPickArgs a) {
    __shared__ RowLseLds<TL_WAVES> sl;
    __shared__ RowBestLds<TL_WAVES> sb;
    const int r = blockIdx.x, V = a.V;
    const int p = *a.pos;
    const bool hist_on = a.hist != nullptr && p >= 0 && p < a.hist_cap;
    if (a.eos >= 0 && a.done[r] != 0) {                         // the whole workgroup takes this branch: no barrier is skipped
        if (threadIdx.x == 0) {
            a.next_ids[r] = a.eos;
            if (hist_on) a.hist[(int64_t)r * a.hist_ld + p] = a.eos;
        }
        return;
    }
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    float m = -INFINITY, l = 0.f, bs = -INFINITY;
    int bi = ROW_NONE;
    tl_scan<T, true>(x, V, m, l, bs, bi);
    row_wave_lse_best(m, l, bs, bi);
    sl.put(m, l);
    sb.put(bs, bi);
    __syncthreads();
    sl.get(m, l);
    sb.get(bs, bi);
    if (threadIdx.x == 0) {
        const int t = bi < V ? bi : 0;                          // only reachable with NaN logits: keep the read inside the row
        a.sum_logprobs[r] += ld_as_f32<T>(x + t) - (m + logf(l));
        a.n_tokens[r] += 1;
        a.next_ids[r] = t;
        if (t == a.eos) a.done[r] = 1;
        if (hist_on) a.hist[(int64_t)r * a.hist_ld + p] = t;
    }
}

int tl_row_check(int R, int V, int dtype, const void *logits, int64_t ld) {
    if (R <= 0 || V < 2) return MOPK_ERR_BAD_SHAPE;
    if (dtype != MOPK_F32 && dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (ld < V) return MOPK_ERR_BAD_ARG;
    if (misaligned(dtype == MOPK_BF16 ? 1 : 3, logits)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

int tl_check(const MopkTokenLogprobArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    const int rc = tl_row_check(a->R, a->V, a->dtype, a->logits, a->logits_ld);
    if (rc != MOPK_OK) return rc;
    if (!a->tokens && (a->token < 0 || a->token >= a->V)) return MOPK_ERR_BAD_ARG;
    if (misaligned(3, a->tokens, a->out)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

int gp_check(const MopkGreedyPickArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    const int rc = tl_row_check(a->R, a->V, a->dtype, a->logits, a->logits_ld);
    if (rc != MOPK_OK) return rc;
    if (a->eos < -1 || a->eos >= a->V || a->reserved != 0) return MOPK_ERR_BAD_ARG;
    if (a->hist_cap < 0 || (a->hist && a->hist_ld < a->hist_cap)) return MOPK_ERR_BAD_ARG;
    if (misaligned(3, a->pos, a->next_ids, a->done, a->sum_logprobs, a->n_tokens, a->hist)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_token_logprob_supported(const MopkTokenLogprobArgs *a) { return tl_check(a) == MOPK_OK; }

int mopk_token_logprob(const MopkTokenLogprobArgs *a, void *stream) {
    const int rc = tl_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->out)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((tl_row_kernel<unsigned short>), dim3((unsigned)a->R), dim3(TL_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((tl_row_kernel<float>), dim3((unsigned)a->R), dim3(TL_THREADS), 0, st, *a);
    return launch_status();
}

int mopk_greedy_pick_supported(const MopkGreedyPickArgs *a) { return gp_check(a) == MOPK_OK; }

int mopk_greedy_pick(const MopkGreedyPickArgs *a, void *stream) {
    const int rc = gp_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->pos, a->next_ids, a->done, a->sum_logprobs, a->n_tokens)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((gp_row_kernel<unsigned short>), dim3((unsigned)a->R), dim3(TL_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((gp_row_kernel<float>), dim3((unsigned)a->R), dim3(TL_THREADS), 0, st, *a);
    return launch_status();
}

}  // extern "C"
