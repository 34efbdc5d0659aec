// Repetition penalty and no-repeat n-gram blocking on last-position logits (WhisperMoP.generate / beam_search / sample with repeat
// rules; inference only).  include/mopk.h states the rules.  One launch, one workgroup of 1024 threads per row, no atomics, no host
// synchronisation: the position is read from device memory, so one set of launch arguments serves every step and a step can be
// captured once in a HIP graph.
//
// The generated tokens g (at most 4096) are staged in LDS once.  With out == logits the kernel touches only the entries that it
// changes: thread t reads x[g[t + 1024 k]] for its (at most four) positions, a workgroup barrier follows, and only then is anything
// written, so every read sees the input and the threads that hold the same token write the same value.  The bans are written behind
// a second barrier, so a banned token is -inf whichever thread penalised it.  With a separate out the row is copied first (16-byte
// accesses where both rows are aligned alike, elements at the ragged ends), before the first barrier.  The kernel waits on latency
// (g, then x[g], then the writes), not on bandwidth.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int RR_THREADS = 1024;
constexpr int RR_MAX_G = 4096;                                  // generated tokens held in LDS (16 KB)
constexpr int RR_PER = RR_MAX_G / RR_THREADS;                   // history positions per thread

// y[0:V] = x[0:V], bit for bit
template <typename T>
__device__ __forceinline__ void rr_copy_row(const T *x, T *y, int V, int tid) {
    if (((uintptr_t)x ^ (uintptr_t)y) & 15) {                   // the rows are aligned differently: elements
        for (int v = tid; v < V; v += RR_THREADS) y[v] = x[v];
        return;
    }
    const RowSpan<T> sp(x, V);
    const int head = sp.head, nvec = sp.nvec, tail = sp.tail0;
    if (tid < head) y[tid] = x[tid];
    const uint4 *xv = (const uint4 *)(x + head);
    uint4 *yv = (uint4 *)(y + head);
    int i = tid;
    for (; i + 3 * RR_THREADS < nvec; i += 4 * RR_THREADS) {    // four loads in flight, then their stores
        const uint4 a = xv[i], b = xv[i + RR_THREADS], c = xv[i + 2 * RR_THREADS], d = xv[i + 3 * RR_THREADS];
        yv[i] = a;
        yv[i + RR_THREADS] = b;
        yv[i + 2 * RR_THREADS] = c;
        yv[i + 3 * RR_THREADS] = d;
    }
    for (; i < nvec; i += RR_THREADS) yv[i] = xv[i];
    if (tail + tid < V) y[tail + tid] = x[tail + tid];          // fewer than EPV elements
}

template <typename T>
__global__ __launch_bounds__(RR_THREADS) void rr_row_kernel(MopkRepeatRulesArgs a) {
    __shared__ int32_t sg[RR_MAX_G];
    const int tid = threadIdx.x, r = blockIdx.x, V = a.V;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    T *y = (T *)a.out + (int64_t)r * a.out_ld;
    const int32_t *g = a.hist + (int64_t)r * a.hist_ld + a.T0;
    const int n = min(min(max(*a.pos - a.T0, 0), a.T - a.T0), RR_MAX_G);
    const bool pen = a.penalty != 1.f;

    // the history into LDS, and step 1's reads: thread t owns the positions t + 1024 k
    int tok[RR_PER];
    float f[RR_PER];
#pragma unroll
    for (int k = 0; k < RR_PER; ++k) {                          // each loop's loads are independent: they fly together
        const int i = tid + k * RR_THREADS;
        tok[k] = i < n ? g[i] : -1;
    }
#pragma unroll
    for (int k = 0; k < RR_PER; ++k) {
        const int i = tid + k * RR_THREADS;
        if (i < n) sg[i] = tok[k];
        if (!pen || (unsigned)tok[k] >= (unsigned)V || a.exempt[tok[k]]) tok[k] = -1;
    }
#pragma unroll
    for (int k = 0; k < RR_PER; ++k) f[k] = tok[k] >= 0 ? ld_as_f32<T>(x + tok[k]) : 0.f;

    if ((const T *)y != x) rr_copy_row<T>(x, y, V, tid);        // step 0
    __syncthreads();                                            // every read above is done, the row is copied, sg is whole

    // step 1: the penalty
#pragma unroll
    for (int k = 0; k < RR_PER; ++k)
        if (tok[k] >= 0) st_from_f32<T>(y + tok[k], f[k] < 0.f ? f[k] * a.penalty : f[k] * a.inv_penalty);

    // step 2: ban the token that followed each earlier occurrence of the last s - 1 tokens
    const int s = a.ngram;
    if (s >= 1 && n >= s) {                                     // the same for the whole workgroup
        __syncthreads();                                        // the bans land on top of the penalties
        const int c0 = n - s + 1;
        for (int i = tid; i <= n - s; i += RR_THREADS) {
            bool same = true;
            for (int k = s - 2; k >= 0 && same; --k) same = sg[i + k] == sg[c0 + k];
            if (same) {
                const int v = sg[i + s - 1];
                if ((unsigned)v < (unsigned)V && !a.exempt[v]) y[v] = row_ninf<T>();
            }
        }
    }
}

int rr_check(const MopkRepeatRulesArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->V < 2) return MOPK_ERR_BAD_SHAPE;
    if (a->dtype != MOPK_F32 && a->dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->T < 0 || a->T0 < 0 || a->T0 > a->T) return MOPK_ERR_BAD_ARG;
    if (a->logits_ld < a->V || a->out_ld < a->V || a->hist_ld < a->T) return MOPK_ERR_BAD_ARG;
    if (a->ngram < 0) return MOPK_ERR_BAD_ARG;
    if (!(a->penalty > 0.f) || !(a->penalty < INFINITY) || !(a->inv_penalty > 0.f) || !(a->inv_penalty < INFINITY))
        return MOPK_ERR_BAD_ARG;
    if (a->out == a->logits && a->R > 1 && a->out_ld != a->logits_ld) return MOPK_ERR_BAD_ARG;   // in place: the same rows
    if (a->T - a->T0 > RR_MAX_G) return MOPK_ERR_UNSUPPORTED;
    const int es = a->dtype == MOPK_BF16 ? 2 : 4;
    if (misaligned(es - 1, a->logits, a->out) || misaligned(3, a->hist, a->pos))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_repeat_rules_supported(const MopkRepeatRulesArgs *a) { return rr_check(a) == MOPK_OK; }

int mopk_repeat_rules(const MopkRepeatRulesArgs *a, void *stream) {
    const int rc = rr_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->out, a->hist, a->pos, a->exempt)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((rr_row_kernel<unsigned short>), dim3((unsigned)a->R), dim3(RR_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((rr_row_kernel<float>), dim3((unsigned)a->R), dim3(RR_THREADS), 0, st, *a);
    return launch_status();
}

}  // extern "C"
