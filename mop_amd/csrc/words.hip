// Word timestamps on decoded token rows (WhisperMoP.align_words and transcribe(word_timestamps=True); inference only): the rows of
// a set of windows turned into alignment inputs, and the aligned text tokens grouped into timed words.  include/mopk.h states the
// rules.  Each op is one launch, one workgroup per row, one thread per column (at most 1024), no atomics, no workspace, no host
// synchronisation: every length is read from device memory and every output word has exactly one writer, so both can be captured
// in a HIP graph and are bitwise reproducible.
//
// Every flag is one bit per thread, so a wave's share of a scan is a ballot (the scheme of ts_row_kernel): the flags before a lane
// are the population count under it, the waves exchange their counts through LDS once, and a thread adds the counts of the waves
// before its own.  mopk_alignment_rows needs one such scan (the text tokens), mopk_word_spans three (the word begins, the nonzero
// durations, of which only the total is used, and the surviving words).  In mopk_word_spans thread i is token i up to the first
// scan and word i after it; the words' first tokens, durations and class bits live in LDS.  For the median every word counts the
// nonzero durations that rank before its own (smaller, or equal with a smaller index): K reads of one LDS word per thread, all
// lanes the same address, so each read is a broadcast; the one or two words whose rank is in the middle write the result.
#include "common.h"

namespace mopk {
namespace {

constexpr int WS_MAXN = 1024;
constexpr int WS_WAVES = WS_MAXN / WAVE;

enum : int { WS_BEGIN = 1, WS_PREPEND = 2, WS_APPEND = 4, WS_SENT_END = 8, WS_DIE1 = 16 };   // bits 0-3: the table's; 4: dies in pass 1

__device__ __forceinline__ int ws_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }

// exclusive scan of one flag per thread over the block; returns the flags before this thread and sets total.  cnt: WS_WAVES ints of
// LDS that no other scan is using (two barriers inside: the second one frees cnt again)
__device__ __forceinline__ int ws_scan(bool flag, int *cnt, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) cnt[wv] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < nw; ++k) {
        const int c = cnt[k];
        if (k < wv) before += c;
        total += c;
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

template <typename OUT, typename SOT>
__device__ __forceinline__ void ar_row(const MopkAlignmentRowsArgs &a, int *cnt) {
    const int j = threadIdx.x, r = blockIdx.x;
    const int S = a.T - a.T0, Tp = a.Tp, W = Tp + 2 + S;
    const int m = ws_clamp(a.n_take[r], 0, S);
    const int g = j < S ? a.tokens[(int64_t)r * a.tokens_ld + a.T0 + j] : 0;
    const bool text = j < m && g < a.eos;
    int n_text;
    const int pos = ws_scan(text, cnt, n_text);                 // pos < n_text <= S
    OUT *ids = (OUT *)a.ids + (int64_t)r * W;
    int32_t *col = a.col + (int64_t)r * W;
    if (text) {
        ids[Tp + 1 + pos] = (OUT)g;
        col[pos] = a.T0 + j;
    }
    const SOT *sot = (const SOT *)a.sot + (int64_t)r * a.sot_ld;
    for (int c = j; c < W; c += blockDim.x) {
        if (c < Tp) ids[c] = (OUT)sot[c];
        else if (c == Tp) ids[c] = (OUT)a.nots;
        else if (c > Tp + n_text) ids[c] = (OUT)a.eos;         // the text tokens are at Tp + 1 ... Tp + n_text
        if (c >= n_text) col[c] = -1;
    }
    if (j == 0) a.n_tokens[r] = Tp + 2 + n_text;
}

__global__ __launch_bounds__(WS_MAXN) void ar_row_kernel(MopkAlignmentRowsArgs a) {
    __shared__ int cnt[WS_WAVES];
    if (a.out_i64) {
        if (a.sot_i64) ar_row<int64_t, int64_t>(a, cnt);
        else ar_row<int64_t, int32_t>(a, cnt);
    } else {
        if (a.sot_i64) ar_row<int32_t, int64_t>(a, cnt);
        else ar_row<int32_t, int32_t>(a, cnt);
    }
}

struct WsLds {
    int cnt[WS_WAVES];
    int o[WS_MAXN + 1];                  // first token of word k; o[K] = n
    int d[WS_MAXN];                      // e_k - s_k
    int tb[WS_MAXN + 1];                 // first token of survivor j; tb[n_words] = n
    unsigned char cls[WS_MAXN];          // of word k: P / A / E (single-token words only) and WS_DIE1
    int med[2];
};

__global__ __launch_bounds__(WS_MAXN) void ws_row_kernel(MopkWordSpansArgs a) {
    __shared__ WsLds s;
    const int i = threadIdx.x, r = blockIdx.x, N = a.N;
    const int n = ws_clamp(a.n_text[r], 0, N);
    const int32_t *times = a.times + (int64_t)r * a.times_ld;
    const float *pr = a.probs + (int64_t)r * a.probs_ld;

    // 1. words: number the begins
    const bool valid = i < n;
    const int c = valid ? a.table[ws_clamp(a.tokens[(int64_t)r * a.tokens_ld + i], 0, a.V - 1)] : 0;
    const bool begin = valid && (i == 0 || (c & WS_BEGIN));
    int K;
    const int k_tok = ws_scan(begin, s.cnt, K);                 // K <= n <= N
    if (begin) {
        s.o[k_tok] = i;
        s.cls[k_tok] = (unsigned char)c;
    }
    if (i == 0) s.o[K] = n;
    __syncthreads();

    // from here on thread i is word i
    const bool word = i < K;
    int st = 0, en = 0, d = 0, fl = 0, o0 = 0;
    float p = 0.f;
    if (word) {
        o0 = s.o[i];
        const int o1 = s.o[i + 1];                              // o0 < o1 <= n
        st = times[o0];
        en = times[o1];
        d = en - st;
        fl = o1 - o0 == 1 ? (s.cls[i] & (WS_PREPEND | WS_APPEND | WS_SENT_END)) : 0;
        if ((fl & WS_PREPEND) && i < K - 1) fl |= WS_DIE1;
        float sum = 0.f;
        for (int t = o0; t < o1; ++t) sum += pr[t];
        p = sum / (float)(o1 - o0);
        s.d[i] = d;
        s.cls[i] = (unsigned char)fl;                           // thread i alone read s.cls[i] above
    }

    // 2. twice the median of the nonzero durations
    const bool nz = word && d != 0;
    int M;
    ws_scan(nz, s.cnt, M);                                      // its barriers publish s.d and s.cls as well
    if (nz) {
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const int dj = s.d[j];
            rank += dj != 0 && (dj < d || (dj == d && j < i));
        }
        if (rank == (M - 1) / 2) s.med[0] = d;
        if (rank == M / 2) s.med[1] = d;
    }
    __syncthreads();
    const int m2 = M > 0 ? s.med[0] + s.med[1] : 0;             // odd M: the middle value twice
    const int max_dur = a.median_cap >= 0 ? min(m2, 2 * a.median_cap) : m2;

    // 3. truncation at sentence ends (original values only)
    bool die2 = false;
    if (word && i >= 1) {
        const int prev = s.cls[i - 1];
        if (d > max_dur) {
            if (fl & WS_SENT_END) en = st + max_dur;
            else if (prev & WS_SENT_END) st = en - max_dur;
        }
        // 5. pass 2: word i - 1 survived pass 1, so this word received nothing and a survivor of both passes is before it
        die2 = !(fl & WS_DIE1) && (fl & WS_APPEND) && !(prev & WS_DIE1);
    }

    // 6. survivors; a survivor's range opens at the head of the run of pass-1 deaths in front of it
    const bool surv = word && !(fl & WS_DIE1) && !die2;
    int n_words;
    const int idx = ws_scan(surv, s.cnt, n_words);              // n_words <= K
    const bool after_die1 = i >= 1 && (s.cls[i - 1] & WS_DIE1);
    if (word && !after_die1 && (surv || (fl & WS_DIE1))) s.tb[idx] = o0;
    if (i == 0) s.tb[n_words] = n;
    const int64_t ob = (int64_t)r * N;
    if (surv) {
        a.starts[ob + idx] = st;
        a.ends[ob + idx] = en;
        a.out_probs[ob + idx] = p;
    }
    __syncthreads();
    if (i < n_words) {
        a.tok_begin[ob + i] = s.tb[i];
        a.tok_end[ob + i] = s.tb[i + 1];
    } else if (i < N) {
        a.starts[ob + i] = a.ends[ob + i] = a.tok_begin[ob + i] = a.tok_end[ob + i] = -1;
        a.out_probs[ob + i] = 0.f;
    }
    if (i == 0) a.n_words[r] = n_words;
}

int ar_check(const MopkAlignmentRowsArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->T <= 0 || a->Tp <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->T0 < 0 || a->T0 >= a->T || a->tokens_ld < a->T) return MOPK_ERR_BAD_ARG;
    if (a->sot_ld < 0 || (a->sot_ld > 0 && a->sot_ld < a->Tp)) return MOPK_ERR_BAD_ARG;
    if ((a->out_i64 != 0 && a->out_i64 != 1) || (a->sot_i64 != 0 && a->sot_i64 != 1)) return MOPK_ERR_BAD_ARG;
    if (a->T - a->T0 > WS_MAXN) return MOPK_ERR_UNSUPPORTED;
    const uintptr_t om = a->out_i64 ? 7 : 3, sm = a->sot_i64 ? 7 : 3;
    if (misaligned(3, a->tokens, a->n_take) || misaligned(sm, a->sot) || misaligned(om, a->ids) || misaligned(3, a->n_tokens, a->col))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

int ws_check(const MopkWordSpansArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->N <= 0 || a->V <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->tokens_ld < a->N || a->times_ld < (int64_t)a->N + 1 || a->probs_ld < a->N || a->median_cap < -1) return MOPK_ERR_BAD_ARG;
    if (a->N > WS_MAXN) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(3, a->tokens, a->times, a->probs, a->n_text, a->starts, a->ends, a->out_probs, a->tok_begin, a->tok_end, a->n_words))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_alignment_rows_supported(const MopkAlignmentRowsArgs *a) { return ar_check(a) == MOPK_OK; }

int mopk_alignment_rows(const MopkAlignmentRowsArgs *a, void *stream) {
    const int rc = ar_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->tokens, a->n_take, a->sot, a->ids, a->n_tokens, a->col)) return MOPK_ERR_BAD_ARG;
    const int threads = (a->T - a->T0 + WAVE - 1) / WAVE * WAVE;
    hipLaunchKernelGGL(ar_row_kernel, dim3((unsigned)a->R), dim3(threads), 0, (hipStream_t)stream, *a);
    return launch_status();
}

int mopk_word_spans_supported(const MopkWordSpansArgs *a) { return ws_check(a) == MOPK_OK; }

int mopk_word_spans(const MopkWordSpansArgs *a, void *stream) {
    const int rc = ws_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->tokens, a->times, a->probs, a->n_text, a->table, a->starts, a->ends, a->out_probs, a->tok_begin, a->tok_end, a->n_words))
        return MOPK_ERR_BAD_ARG;
    const int threads = (a->N + WAVE - 1) / WAVE * WAVE;
    hipLaunchKernelGGL(ws_row_kernel, dim3((unsigned)a->R), dim3(threads), 0, (hipStream_t)stream, *a);
    return launch_status();
}

}  // extern "C"
