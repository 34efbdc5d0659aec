// Whisper's segment and seek arithmetic on decoded token rows (WhisperMoP.transcribe; inference only): the timestamp tokens of a
// decoded window cut it into segments and say how far the next window moves.  include/mopk.h states the rules.  One launch, one
// workgroup per row, one thread per generated column (T - T0 <= 1024), integers only, no atomics, no workspace, no host
// synchronisation: the window lengths are read from device memory and every output word has exactly one writer, so the call can be
// captured in a HIP graph and is bitwise reproducible.
//
// Every flag is one bit per thread, so a wave's share of each block reduction is a ballot: the first eos is the lowest set bit,
// the last cut and the last timestamp the highest, the cuts before a lane the population count under it.  The waves exchange
// their shares through LDS once for n and once for (cut count, last cut, last timestamp); a thread adds the counts of the waves
// before its own, which completes the exclusive scan that numbers the cuts.  The thread of cut c closes segment k (end, tok_end)
// and opens segment k + 1 (start, tok_begin), thread 0 opens segment 0, closes what no cut closes and writes the row's two
// scalars; thread j >= n_segments writes the -1 tail at j.
#include "common.h"

namespace mopk {
namespace {

constexpr int TS_MAXS = 1024;
constexpr int TS_WAVES = TS_MAXS / WAVE;

struct TsLds {
    int first_eos[TS_WAVES];
    int cuts[TS_WAVES], last_cut[TS_WAVES], last_ts[TS_WAVES];
};

__device__ __forceinline__ int ts_hi_bit(unsigned long long b, int base) { return b ? base + 63 - __clzll((long long)b) : -1; }

__global__ __launch_bounds__(TS_MAXS) void ts_row_kernel(MopkTimestampSegmentsArgs a) {
    __shared__ TsLds s;
    const int i = threadIdx.x, r = blockIdx.x, lane = i & 63, wv = i >> 6, nw = blockDim.x >> 6;
    const int S = a.T - a.T0, tb = a.tb;
    const uint32_t f = (uint32_t)a.f;
    const int32_t *g = a.tokens + (int64_t)r * a.tokens_ld + a.T0;
    const bool col = i < S;                                     // the block is S rounded up to whole waves
    const int tok = col ? g[i] : 0;
    const int prev = col && i > 0 ? g[i - 1] : 0;
    auto frame = [&](int id) { return (int32_t)((uint32_t)(id - tb) * f); };   // of a timestamp token id >= tb

    // n: the first column that holds eos, S if none
    const unsigned long long be = __ballot(col && tok == a.eos);
    if (lane == 0) s.first_eos[wv] = be ? wv * WAVE + __ffsll((long long)be) - 1 : S;
    __syncthreads();
    int n = S;
    for (int k = 0; k < nw; ++k) n = min(n, s.first_eos[k]);

    // timestamp flags, pair flags (the cuts C), and the exclusive scan of the pair flags
    const bool ts = i < n && tok >= tb;
    const bool cut = ts && i > 0 && prev >= tb;                 // i - 1 < n as well
    const unsigned long long bc = __ballot(cut), bt = __ballot(ts);
    if (lane == 0) {
        s.cuts[wv] = __popcll(bc);
        s.last_cut[wv] = ts_hi_bit(bc, wv * WAVE);
        s.last_ts[wv] = ts_hi_bit(bt, wv * WAVE);
    }
    __syncthreads();
    int before = 0, nC = 0, maxC = -1, li = -1;
    for (int k = 0; k < nw; ++k) {
        const int c = s.cuts[k];
        if (k < wv) before += c;
        nC += c;
        maxC = max(maxC, s.last_cut[k]);
        li = max(li, s.last_ts[k]);
    }
    const int rank = before + __popcll(bc & ((1ull << lane) - 1ull));
    const bool single_end = n >= 2 && g[n - 2] < tb && g[n - 1] >= tb;
    const int nseg = nC > 0 ? nC + (single_end ? 1 : 0) : (n > 0 ? 1 : 0);       // <= n <= S

    const int64_t o = (int64_t)r * S;
    int32_t *starts = a.starts + o, *ends = a.ends + o, *tok_begin = a.tok_begin + o, *tok_end = a.tok_end + o;
    if (cut) {                                                  // rank < nC <= nseg <= S
        ends[rank] = frame(prev);
        tok_end[rank] = a.T0 + i;
        if (rank + 1 < nseg) {
            starts[rank + 1] = frame(tok);
            tok_begin[rank + 1] = a.T0 + i;
        }
    }
    if (i == 0) {
        const int w = max(a.window[r], 1);
        int adv = w;
        if (nC > 0) {
            starts[0] = tok >= tb ? frame(tok) : 0;
            tok_begin[0] = a.T0;
            if (single_end) {
                ends[nC] = frame(g[n - 1]);
                tok_end[nC] = a.T0 + n;
            } else {
                adv = frame(g[maxC - 1]);
            }
        } else if (n > 0) {
            starts[0] = 0;
            tok_begin[0] = a.T0;
            ends[0] = li >= 0 && g[li] != tb ? frame(g[li]) : w;
            tok_end[0] = a.T0 + n;
        }
        a.n_segments[r] = nseg;
        a.advance[r] = min(max(adv, 1), w);
    }
    if (col && i >= nseg) starts[i] = ends[i] = tok_begin[i] = tok_end[i] = -1;
}

int ts_check(const MopkTimestampSegmentsArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->T <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->T0 < 0 || a->T0 >= a->T || a->tokens_ld < a->T) return MOPK_ERR_BAD_ARG;
    if (a->eos < 0 || a->eos >= a->tb || a->f < 1) return MOPK_ERR_BAD_ARG;
    if (a->T - a->T0 > TS_MAXS) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(3, a->tokens, a->window, a->starts, a->ends, a->tok_begin, a->tok_end, a->n_segments, a->advance))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_timestamp_segments_supported(const MopkTimestampSegmentsArgs *a) { return ts_check(a) == MOPK_OK; }

int mopk_timestamp_segments(const MopkTimestampSegmentsArgs *a, void *stream) {
    const int rc = ts_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->tokens, a->window, a->starts, a->ends, a->tok_begin, a->tok_end, a->n_segments, a->advance)) return MOPK_ERR_BAD_ARG;
    const int threads = (a->T - a->T0 + WAVE - 1) / WAVE * WAVE;
    hipLaunchKernelGGL(ts_row_kernel, dim3((unsigned)a->R), dim3(threads), 0, (hipStream_t)stream, *a);
    return launch_status();
}

}  // extern "C"
