// Conditioning a window on the previous text (WhisperMoP.transcribe; inference only): the per-clip token history on the device and
// the prompt matrix of a set of windows built from it.  include/mopk.h states the rules.  Each op is one launch, one workgroup per
// row, integers only, no atomics, no workspace, no host synchronisation: every length is read from device memory and every word has
// one writer, so both can be captured in a HIP graph and are bitwise reproducible.
//
// mopk_prompt_history_update shifts a clip's history in place: the block is n rounded up to whole waves (n <= 1024), thread j holds
// the entry that ends up at hist[b, j] in a register, and a barrier separates the last read of the row from its first write.
// mopk_window_prompts strides a block of up to 1024 threads over the width columns of its row; thread 0 writes kv_start.
#include "common.h"

namespace mopk {
namespace {

constexpr int PH_MAXN = 1024;          // history entries of a clip (one thread each)
constexpr int PH_MAXS = 1024;          // generated columns of a row
constexpr int WP_MAXW = 2048;          // columns of a prompt row
constexpr int WP_THREADS = 1024;

__device__ __forceinline__ int ph_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }

__global__ __launch_bounds__(PH_MAXN) void ph_row_kernel(MopkPromptHistoryArgs a) {
    const int j = threadIdx.x, r = blockIdx.x;
    const int b = a.item[r], mode = a.mode[r];
    if (b < 0 || b >= a.B || (mode != 0 && mode != 1)) return;  // the whole block: no thread reaches the barrier
    int32_t *h = a.hist + (int64_t)b * a.n;
    if (mode == 1) {
        if (j == 0) a.hist_len[b] = 0;
        return;
    }
    const int L = ph_clamp(a.hist_len[b], 0, a.n), m = ph_clamp(a.n_take[r], 0, a.T - a.T0);
    const int keep = min(a.n, L + m), src = L + m - keep + j;   // entry j of the last keep of (hist[b, :L], tokens[r, T0:T0+m])
    const bool mine = j < keep;
    int v = 0;
    if (mine) v = src < L ? h[src] : a.tokens[(int64_t)r * a.tokens_ld + a.T0 + (src - L)];   // src - L < m <= T - T0
    __syncthreads();                                            // every source entry is in a register before any is overwritten
    if (mine) h[j] = v;
    if (j == 0) a.hist_len[b] = keep;
}

template <typename OUT, typename SOT>
__device__ __forceinline__ void wp_row(const MopkWindowPromptsArgs &a) {
    const int r = blockIdx.x, W = a.width, Ts = a.Ts;
    const int b = a.item[r];
    const bool in = b >= 0 && b < a.B;
    const int bc = ph_clamp(b, 0, a.B - 1);
    const int L = in ? ph_clamp(a.hist_len[bc], 0, a.n) : 0, room = W - Ts;
    const int hh = L > 0 && room >= 2 ? min(L, room - 1) : 0;
    const int pre = hh > 0 ? 1 + hh : 0, ks = W - Ts - pre;
    const int32_t *h = a.hist + (int64_t)bc * a.n + (L - hh);
    const SOT *sot = (const SOT *)a.sot + (int64_t)bc * a.sot_ld;
    OUT *out = (OUT *)a.ids + (int64_t)r * W;
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        const int rel = c - ks;                                 // < pre + Ts
        int64_t v = 0;
        if (rel >= pre) v = (int64_t)sot[rel - pre];
        else if (rel >= 1) v = h[rel - 1];                      // rel - 1 < hh <= L
        else if (rel == 0) v = a.prev;                          // pre > 0 here
        out[c] = (OUT)v;
    }
    if (threadIdx.x == 0) a.kv_start[r] = ks;
}

__global__ __launch_bounds__(WP_THREADS) void wp_row_kernel(MopkWindowPromptsArgs a) {
    if (a.out_i64) {
        if (a.sot_i64) wp_row<int64_t, int64_t>(a);
        else wp_row<int64_t, int32_t>(a);
    } else {
        if (a.sot_i64) wp_row<int32_t, int64_t>(a);
        else wp_row<int32_t, int32_t>(a);
    }
}

int ph_check(const MopkPromptHistoryArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->A <= 0 || a->B <= 0 || a->n <= 0 || a->T <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->T0 < 0 || a->T0 >= a->T || a->tokens_ld < a->T) return MOPK_ERR_BAD_ARG;
    if (a->n > PH_MAXN || a->T - a->T0 > PH_MAXS) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(3, a->hist, a->hist_len, a->tokens, a->n_take, a->item, a->mode)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

int wp_check(const MopkWindowPromptsArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->A <= 0 || a->B <= 0 || a->n <= 0 || a->Ts <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->width < a->Ts || a->sot_ld < 0 || (a->sot_ld > 0 && a->sot_ld < a->Ts)) return MOPK_ERR_BAD_ARG;
    if ((a->out_i64 != 0 && a->out_i64 != 1) || (a->sot_i64 != 0 && a->sot_i64 != 1)) return MOPK_ERR_BAD_ARG;
    if (a->width > WP_MAXW) return MOPK_ERR_UNSUPPORTED;
    const uintptr_t om = a->out_i64 ? 7 : 3, sm = a->sot_i64 ? 7 : 3;
    if (misaligned(3, a->hist, a->hist_len, a->item) || misaligned(sm, a->sot) || misaligned(om, a->ids) || misaligned(3, a->kv_start))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_prompt_history_update_supported(const MopkPromptHistoryArgs *a) { return ph_check(a) == MOPK_OK; }

int mopk_prompt_history_update(const MopkPromptHistoryArgs *a, void *stream) {
    const int rc = ph_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->hist, a->hist_len, a->tokens, a->n_take, a->item, a->mode)) return MOPK_ERR_BAD_ARG;
    const int threads = (a->n + WAVE - 1) / WAVE * WAVE;
    hipLaunchKernelGGL(ph_row_kernel, dim3((unsigned)a->A), dim3(threads), 0, (hipStream_t)stream, *a);
    return launch_status();
}

int mopk_window_prompts_supported(const MopkWindowPromptsArgs *a) { return wp_check(a) == MOPK_OK; }

int mopk_window_prompts(const MopkWindowPromptsArgs *a, void *stream) {
    const int rc = wp_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->hist, a->hist_len, a->item, a->sot, a->ids, a->kv_start)) return MOPK_ERR_BAD_ARG;
    const int threads = min((a->width + WAVE - 1) / WAVE * WAVE, WP_THREADS);
    hipLaunchKernelGGL(wp_row_kernel, dim3((unsigned)a->A), dim3(threads), 0, (hipStream_t)stream, *a);
    return launch_status();
}

}  // extern "C"
