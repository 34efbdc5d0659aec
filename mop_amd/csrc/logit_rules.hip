// Whisper's logit rules on last-position logits (WhisperMoP.generate / beam_search / sample with logit_rules; inference only): the
// never-emit list, blank suppression at the first generated position and the timestamp grammar (pairs, monotone, a bounded first
// timestamp, and a forced timestamp when the timestamp tokens together outweigh the best text token).  include/mopk.h states the
// rules.  One launch, one workgroup of 1024 threads per row, no atomics, no host synchronisation: the position is read from device
// memory, so one set of launch arguments serves every step and a step can be captured once in a HIP graph.
//
// Rules 1-3d reduce to four row constants: text tokens v < text_lo are blocked, timestamp tokens are kept inside [ts_lo, ts_hi]
// only, and the mask table's bits are tested against `mbits`.  Wave 0 finds them from the token history (at most T <= a few hundred
// tokens).  Pass 1 streams the row (thread t reads v = t + 1024 i) and merges (max, sum-exp) of the kept timestamps and the max of
// the kept text tokens; every block reduction has a fixed order, so the result is bitwise reproducible.  Pass 2 streams it again
// (it is in L2) and writes each entry's own bits or -inf; a thread rewrites only elements that it read itself, so out may be logits.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int LR_THREADS = 1024;
constexpr int LR_WAVES = LR_THREADS / WAVE;
#define LR_UNROLL 16                                            // loads in flight per thread: each pass is bound by L2 latency

struct LrRow {                                                  // rules 1-3d of one row
    int tb;                                                     // V when rule 3 is off: every token is a text token
    int text_lo, ts_lo, ts_hi;
    uint32_t mbits;
    __device__ __forceinline__ bool blocked(int v, uint32_t mk) const {
        return (mk & mbits) || (v < tb ? v < text_lo : (v < ts_lo || v > ts_hi));
    }
};

struct LrLds {
    RowLseLds<LR_WAVES> lse;
    float wt[LR_WAVES];
    int last_ts;
};

template <typename T>
__global__ __launch_bounds__(LR_THREADS) void lr_row_kernel(MopkLogitRulesArgs a) {
    __shared__ LrLds s;
    const int tid = threadIdx.x, r = blockIdx.x, V = a.V;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    T *y = (T *)a.out + (int64_t)r * a.out_ld;
    const int32_t *g = a.hist + (int64_t)r * a.hist_ld + a.T0;
    const int n = min(max(*a.pos - a.T0, 0), a.T - a.T0);
    const bool ts_on = a.tb >= 0;

    // the history: index of the last timestamp token (wave 0; lane l reads g[l], g[l + 64], ...)
    if (ts_on && tid < WAVE) {
        int li = -1;
        for (int i = tid; i < n; i += WAVE)
            if (g[i] >= a.tb) li = i;                           // i rises: the lane's last one
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) li = max(li, __shfl_xor(li, o, 64));
        if (tid == 0) s.last_ts = li;
    }
    __syncthreads();
    LrRow row{V, 0, 0, V - 1, n == 0 ? 3u : 1u};
    if (ts_on) {
        row.tb = a.tb;
        row.ts_lo = a.tb;
        const bool last = n >= 1 && g[n - 1] >= a.tb;
        const bool pen = n < 2 || g[n - 2] >= a.tb;
        if (last && !pen) row.text_lo = a.eos;
        const int li = s.last_ts;
        if (li >= 0) {
            const int t = min(g[li], V - 1);                    // an id past the vocabulary blocks no more than V - 1 does
            row.ts_lo = last && !pen ? t : t + 1;
        }
        if (last && pen) row.ts_lo = V;
        if (n == 0) {
            row.text_lo = a.tb;
            if (a.max_initial >= 0 && a.max_initial < V - 1 - a.tb) row.ts_hi = a.tb + a.max_initial;
        }
    }

    // pass 1 (rule 3e): (max, sum-exp) of the kept timestamps, max of the kept text tokens
    if (ts_on) {
        float m = -INFINITY, l = 0.f, mt = -INFINITY;
#pragma unroll LR_UNROLL
        for (int v = tid; v < V; v += LR_THREADS) {
            const float f = ld_as_f32<T>(x + v);
            if (!row.blocked(v, a.mask[v])) {
                if (v >= row.tb) row_lse_add(m, l, f);
                else mt = fmaxf(mt, f);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                      // row_wave_lse and wave_max in one tree (row_helpers.h says why)
            row_lse_merge(m, l, __shfl_xor(m, o, 64), __shfl_xor(l, o, 64));
            mt = fmaxf(mt, __shfl_xor(mt, o, 64));
        }
        s.lse.put(m, l);
        if ((tid & 63) == 0) s.wt[tid / WAVE] = mt;
        __syncthreads();
        s.lse.get(m, l);
        mt = s.wt[0];
        for (int i = 1; i < LR_WAVES; ++i) mt = fmaxf(mt, s.wt[i]);
        const float L = m == -INFINITY ? -INFINITY : m + logf(l);
        if (L > mt) row.text_lo = row.tb;
    }

    // pass 2: the entry's own bits, or -inf
#pragma unroll LR_UNROLL
    for (int v = tid; v < V; v += LR_THREADS) {
        const T e = x[v];
        y[v] = row.blocked(v, a.mask[v]) ? row_ninf<T>() : e;
    }
}

int lr_check(const MopkLogitRulesArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->V < 2) return MOPK_ERR_BAD_SHAPE;
    if (a->dtype != MOPK_F32 && a->dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->T < 0 || a->T0 < 0 || a->T0 > a->T) return MOPK_ERR_BAD_ARG;
    if (a->logits_ld < a->V || a->out_ld < a->V || a->hist_ld < a->T) return MOPK_ERR_BAD_ARG;
    if (a->tb < -1 || a->max_initial < -1) return MOPK_ERR_BAD_ARG;
    if (a->tb >= 0 && (a->tb >= a->V || a->eos < 0 || a->eos >= a->tb)) return MOPK_ERR_BAD_ARG;
    const int es = a->dtype == MOPK_BF16 ? 2 : 4;
    if (misaligned(es - 1, a->logits, a->out) || misaligned(3, a->hist, a->pos))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_logit_rules_supported(const MopkLogitRulesArgs *a) { return lr_check(a) == MOPK_OK; }

int mopk_logit_rules(const MopkLogitRulesArgs *a, void *stream) {
    const int rc = lr_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->out, a->hist, a->pos, a->mask)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((lr_row_kernel<unsigned short>), dim3((unsigned)a->R), dim3(LR_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((lr_row_kernel<float>), dim3((unsigned)a->R), dim3(LR_THREADS), 0, st, *a);
    return launch_status();
}

}  // extern "C"
