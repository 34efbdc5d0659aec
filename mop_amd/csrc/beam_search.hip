// One step of batched beam search (WhisperMoP.beam_search; inference only).  Two launches, no atomics, no host synchronisation:
// the step reads its position from device memory, so one set of launch arguments serves every step and a step can be captured once
// in a HIP graph.
//
// Launch A (bs_rows_kernel): one workgroup per (beam row, vocab slice).  The slice is streamed with 16-byte loads (the elements
// before a row's first 16-byte boundary and after its last whole vector are read one by one by the first / last slice), and each
// thread keeps an online (max, sum-exp) pair and a sorted register list of its NC = 2K best (logit, index) entries.  The pairs are
// combined and the lists merged pairwise through LDS in a fixed tree order; the slice writes (m, l) and its NC best entries (padded
// with sentinels, index ROW_NONE, which rank after every real entry, -inf ones included) to the workspace.  The slice count is chosen
// so that B * K * slices reaches about two workgroups per CU even at B = 1, K = 5.
// Launch B (bs_item_kernel): one workgroup per batch item.  Each beam's log-sum-exp is merged from its slices in slice order; every
// slice candidate becomes (score = scores[k] + (logit - lse[k]), flat index k * V + v) and the item's NC best are selected by the same
// list-and-tree merge.  Thread 0 walks them (eos with a finite score -> a finished hypothesis while fewer than K are stored; anything
// else -> the next live beam; stop at K live beams).  Then the item's K history rows and row-table rows are reordered in place,
// a column block at a time: all K rows of the block are loaded into LDS, barrier, written from their parents.  Only this workgroup
// touches those rows, so the step needs no second buffer (whose pointers would alternate between steps and break graph replay).
// Ranking: larger score first, ties to the smaller flat index -- the same comparison in every list and merge, so the result does not
// depend on how the vocabulary is sliced or on thread timing.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int BS_A_THREADS = 128;       // launch A workgroup
constexpr int BS_B_THREADS = 256;       // launch B workgroup
constexpr int BS_MIN_VEC = 128;         // 16-byte vectors per slice at least: one per launch-A thread
constexpr int BS_TARGET_WG = 512;       // launch-A workgroups aimed for (two per CU on a 256-CU MI355X)
constexpr int BS_COLS = 256;            // history columns per reorder block

// insert into a sorted register list of NC entries (dropped when it ranks after the last one)
template <int NC>
__device__ __forceinline__ void bs_insert(float (&ls)[NC], int (&li)[NC], float s, int i) {
    if (!row_before(s, i, ls[NC - 1], li[NC - 1])) return;
    ls[NC - 1] = s;
    li[NC - 1] = i;
#pragma unroll
    for (int j = NC - 1; j > 0; --j) {
        if (row_before(ls[j], li[j], ls[j - 1], li[j - 1])) {
            const float ts = ls[j]; ls[j] = ls[j - 1]; ls[j - 1] = ts;
            const int ti = li[j]; li[j] = li[j - 1]; li[j - 1] = ti;
        }
    }
}

// merge the NT threads' lists into the workgroup's NC best: lists to LDS, then log2(NT) pairwise levels (thread t < n merges lists
// t and t + n into list t; list t + n is never written at that level, so one barrier per level suffices).  Result: ws[0 .. NC).
template <int NC, int NT>
__device__ __forceinline__ void bs_block_merge(const float (&ls)[NC], const int (&li)[NC], float *ws, int *wi) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NC; ++j) { ws[tid * NC + j] = ls[j]; wi[tid * NC + j] = li[j]; }
    __syncthreads();
#pragma unroll 1
    for (int n = NT / 2; n >= 1; n >>= 1) {
        if (tid < n) {
            const float *as = ws + tid * NC, *bs = ws + (tid + n) * NC;
            const int *ai = wi + tid * NC, *bi = wi + (tid + n) * NC;
            float ms[NC];
            int mi[NC];
            int p = 0, q = 0;                                   // p + q = o < NC before each output: both stay in their lists
            float hs = as[0], gs = bs[0];                       // the two lists' current heads
            int hi = ai[0], gi = bi[0];
#pragma unroll
            for (int o = 0; o < NC; ++o) {
                const bool ta = row_before(hs, hi, gs, gi);
                ms[o] = ta ? hs : gs;
                mi[o] = ta ? hi : gi;
                if (o + 1 < NC) {
                    if (ta) { ++p; hs = as[p]; hi = ai[p]; }
                    else { ++q; gs = bs[q]; gi = bi[q]; }
                }
            }
#pragma unroll
            for (int o = 0; o < NC; ++o) { ws[tid * NC + o] = ms[o]; wi[tid * NC + o] = mi[o]; }
        }
        __syncthreads();
    }
}

struct BsWs {                                                   // workspace layout, rows = B * K
    float *ml;                                                  // (rows, nslice, 2): slice max, sum-exp
    float *cs;                                                  // (rows, nslice, NC): slice candidates' logits
    int *ci;                                                    // (rows, nslice, NC): their vocabulary indices
};
__host__ __device__ inline BsWs bs_ws(const MopkBeamArgs &a, int nslice) {
    const size_t n = (size_t)a.B * a.K * nslice;
    float *base = (float *)a.workspace;
    return BsWs{base, base + n * 2, (int *)(base + n * 2 + n * 2 * a.K)};
}

// launch A: one (beam row, vocabulary slice).  The lists hold LN >= NC entries and the first NC are written: LN = 16 for NC = 14,
// whose own form hipcc compiles to 256 VGPRs and AGPR copies (a longer sorted list only adds entries after the first NC).
template <typename T, int NC>
__global__ __launch_bounds__(BS_A_THREADS) void bs_rows_kernel(MopkBeamArgs a, int nslice) {
    constexpr int EPV = RowSpan<T>::EPV;
    constexpr int LN = NC == 14 ? 16 : NC;
    __shared__ float ws[BS_A_THREADS * LN];
    __shared__ int wi[BS_A_THREADS * LN];
    __shared__ float rm[BS_A_THREADS], rl[BS_A_THREADS];
    const int tid = threadIdx.x, row = blockIdx.x, slice = blockIdx.y;
    const int b = row / a.K, k = row - b * a.K;
    if (a.done[b]) return;                                      // launch B leaves a done item untouched as well
    const int V = a.V;
    const T *x = (const T *)a.logits + (int64_t)b * a.logits_sb + (int64_t)k * a.logits_sk;
    const RowSpan<T> sp(x, V);
    const int head = sp.head, nvec = sp.nvec, tail0 = sp.tail0;
    const int u0 = (int)((int64_t)nvec * slice / nslice), u1 = (int)((int64_t)nvec * (slice + 1) / nslice);

    float ls[LN];
    int li[LN];
#pragma unroll
    for (int j = 0; j < LN; ++j) { ls[j] = -INFINITY; li[j] = ROW_NONE; }
    float m = -INFINITY, l = 0.f;
    const uint4 *xv = (const uint4 *)(x + head);
    for (int u = u0 + tid; u < u1; u += BS_A_THREADS) {
        float f[EPV];
        row_unpack(xv[u], f, T());
        float fm = f[0];
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            row_lse_add(m, l, f[e]);
            fm = fmaxf(fm, f[e]);
        }
        if (fm < ls[LN - 1]) continue;                          // the common case once the list is full: nothing to insert
#pragma unroll 1
        for (int e = 0; e < EPV; ++e) {                         // one insert body, fed by shifting the vector down
            bs_insert(ls, li, f[0], head + u * EPV + e);
#pragma unroll
            for (int j = 0; j + 1 < EPV; ++j) f[j] = f[j + 1];
        }
    }
    const int nh = slice == 0 ? head : 0, nt = slice == nslice - 1 ? V - tail0 : 0;     // scalar head / tail elements
    for (int t = tid; t < nh + nt; t += BS_A_THREADS) {
        const int e = t < nh ? t : tail0 + (t - nh);
        const float f = ld_as_f32<T>(x + e);
        row_lse_add(m, l, f);
        bs_insert(ls, li, f, e);
    }

    rm[tid] = m;                                                // pairwise trees through LDS, not row_helpers.h's wave-then-waves
    rl[tid] = l;                                                // order: the step's results depend on this one
    bs_block_merge<LN, BS_A_THREADS>(ls, li, ws, wi);           // its first barrier also publishes rm / rl
#pragma unroll 1
    for (int n = BS_A_THREADS / 2; n >= 1; n >>= 1) {
        if (tid < n) {
            float mm = rm[tid], ll = rl[tid];
            row_lse_merge(mm, ll, rm[tid + n], rl[tid + n]);
            rm[tid] = mm;
            rl[tid] = ll;
        }
        __syncthreads();
    }
    const BsWs w = bs_ws(a, nslice);
    const size_t part = (size_t)row * nslice + slice;
    if (tid == 0) { w.ml[part * 2] = rm[0]; w.ml[part * 2 + 1] = rl[0]; }
    if (tid < NC) { w.cs[part * NC + tid] = ws[tid]; w.ci[part * NC + tid] = wi[tid]; }
}

// launch B: one batch item
template <int NC>
__global__ __launch_bounds__(BS_B_THREADS) void bs_item_kernel(MopkBeamArgs a, int nslice) {
    constexpr int K = NC / 2;
    __shared__ float ws[BS_B_THREADS * NC];
    __shared__ int wi[BS_B_THREADS * NC];
    __shared__ int cols[2][K][BS_COLS];                         // history / row-table block of the item's K rows
    __shared__ float lse[K], sc[K];
    __shared__ int par[K], tok[K], fpar[K], fslot[K];
    __shared__ int nfin;
    const int tid = threadIdx.x, b = blockIdx.x, V = a.V;
    if (a.done[b]) return;
    const int pos = *a.pos;
    if (pos < a.prompt_len || pos >= a.T) return;               // out of range: the call changes nothing
    const BsWs w = bs_ws(a, nslice);
    if (tid < K) {
        const float *ml = w.ml + (size_t)(b * K + tid) * nslice * 2;
        float M = -INFINITY;
        for (int s = 0; s < nslice; ++s) M = fmaxf(M, ml[2 * s]);
        float l = 0.f;
        if (M != -INFINITY)
            for (int s = 0; s < nslice; ++s)
                if (ml[2 * s] != -INFINITY) l = fmaf(expf(ml[2 * s] - M), ml[2 * s + 1], l);
        lse[tid] = M == -INFINITY ? -INFINITY : M + logf(l);
        sc[tid] = a.scores[b * K + tid];
        par[tid] = tid;                                         // defaults: every LDS row index below stays inside [0, K)
        tok[tid] = 0;
    }
    __syncthreads();

    // ---- the item's NC best candidates by score
    float ls[NC];
    int li[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) { ls[j] = -INFINITY; li[j] = ROW_NONE; }
    const int per_row = nslice * NC;
    const size_t c0 = (size_t)b * K * per_row;
    for (int i = tid; i < K * per_row; i += BS_B_THREADS) {
        const int k = i / per_row;
        const float x = w.cs[c0 + i];
        const int v = w.ci[c0 + i];
        if (v == ROW_NONE) continue;
        const float s = (x == -INFINITY || sc[k] == -INFINITY) ? -INFINITY : sc[k] + (x - lse[k]);
        bs_insert(ls, li, s, k * V + v);
    }
    bs_block_merge<NC, BS_B_THREADS>(ls, li, ws, wi);

    // ---- the walk
    if (tid == 0) {
        int nl = 0, nf = a.fin_count[b], nn = 0;
        const float norm = powf((float)(pos - a.prompt_len + 1), a.length_penalty);
        for (int c = 0; c < NC && nl < K; ++c) {
            const float s = ws[c];
            const int flat = wi[c];
            if (flat == ROW_NONE) break;                        // unreachable: K * V >= NC real candidates
            const int k = flat / V, v = flat - k * V;
            if (v == a.eos && isfinite(s)) {
                if (nf < K) {
                    a.fin_scores[b * K + nf] = s / norm;
                    fpar[nn] = k;
                    fslot[nn] = nf;
                    ++nf;
                    ++nn;
                }
            } else {
                sc[nl] = s;                                     // every beam's old score was read before the merge above
                par[nl] = k;
                tok[nl] = v;
                ++nl;
            }
        }
        nfin = nn;
        a.fin_count[b] = nf;
        a.done[b] = nf >= K;
    }
    __syncthreads();

    // ---- reorder columns [0, pos) of the K history / row-table rows in place; copy finished hypotheses' histories
    const int nn = nfin;
    int32_t *hist = a.hist + (int64_t)b * K * a.hist_ld, *rows = a.rows + (int64_t)b * K * a.rows_ld;
    int32_t *fin = a.fin_tokens + (int64_t)b * K * a.T;
    for (int cb = 0; cb < pos; cb += BS_COLS) {
        const int nc = pos - cb < BS_COLS ? pos - cb : BS_COLS;
        for (int i = tid; i < K * nc; i += BS_B_THREADS) {
            const int k = i / nc, c = i - k * nc;
            cols[0][k][c] = hist[k * a.hist_ld + cb + c];
            cols[1][k][c] = rows[k * a.rows_ld + cb + c];
        }
        __syncthreads();
        for (int i = tid; i < K * nc; i += BS_B_THREADS) {
            const int k = i / nc, c = i - k * nc;
            hist[k * a.hist_ld + cb + c] = cols[0][par[k]][c];
            rows[k * a.rows_ld + cb + c] = cols[1][par[k]][c];
        }
        for (int i = tid; i < nn * nc; i += BS_B_THREADS) {
            const int f = i / nc, c = i - f * nc;
            fin[(int64_t)fslot[f] * a.T + cb + c] = cols[0][fpar[f]][c];
        }
        __syncthreads();
    }
    if (tid < K) {
        hist[tid * a.hist_ld + pos] = tok[tid];
        rows[tid * a.rows_ld + pos] = b * K + tid;
        a.next_ids[b * K + tid] = tok[tid];
        a.parents[b * K + tid] = par[tid];
        a.scores[b * K + tid] = sc[tid];
    }
    if (tid < nn) fin[(int64_t)fslot[tid] * a.T + pos] = a.eos;
}

int bs_nslice(const MopkBeamArgs *a) {
    const int epv = a->logits_dtype == MOPK_BF16 ? 8 : 4;
    const int64_t rows = (int64_t)a->B * a->K;
    const int64_t want = (BS_TARGET_WG + rows - 1) / rows;
    const int64_t most = a->V / epv / BS_MIN_VEC;
    int64_t n = want < most ? want : most;
    return n < 1 ? 1 : (int)n;
}

int bs_check(const MopkBeamArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->K <= 0 || a->V < 2 || a->T <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->K > MOPK_BEAM_MAX_K) return MOPK_ERR_UNSUPPORTED;
    if ((int64_t)a->K * a->V >= ROW_NONE || (int64_t)a->B * a->K > 0x7fffffff) return MOPK_ERR_UNSUPPORTED;
    if (a->prompt_len < 1 || a->prompt_len >= a->T) return MOPK_ERR_BAD_SHAPE;
    if (a->hist_ld < a->T || a->rows_ld < a->T) return MOPK_ERR_BAD_SHAPE;
    if (a->logits_dtype != MOPK_F32 && a->logits_dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->logits_sb < 0 || a->logits_sk < 0) return MOPK_ERR_BAD_ARG;
    if (a->eos < -1 || a->eos >= a->V) return MOPK_ERR_BAD_ARG;
    if (!(a->length_penalty == a->length_penalty) || a->length_penalty == INFINITY || a->length_penalty == -INFINITY)
        return MOPK_ERR_BAD_ARG;
    const int es = a->logits_dtype == MOPK_BF16 ? 2 : 4;
    if (misaligned(es - 1, a->logits) || misaligned(15, a->workspace)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <int NC>
void bs_launch(const MopkBeamArgs *a, hipStream_t st) {
    const int ns = bs_nslice(a);
    const dim3 ga((unsigned)(a->B * a->K), (unsigned)ns);
    if (a->logits_dtype == MOPK_BF16) hipLaunchKernelGGL((bs_rows_kernel<unsigned short, NC>), ga, dim3(BS_A_THREADS), 0, st, *a, ns);
    else hipLaunchKernelGGL((bs_rows_kernel<float, NC>), ga, dim3(BS_A_THREADS), 0, st, *a, ns);
    hipLaunchKernelGGL(bs_item_kernel<NC>, dim3((unsigned)a->B), dim3(BS_B_THREADS), 0, st, *a, ns);
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_beam_supported(const MopkBeamArgs *a) { return bs_check(a) == MOPK_OK; }

size_t mopk_beam_workspace_bytes(const MopkBeamArgs *a) {
    if (bs_check(a) != MOPK_OK) return 0;
    return (size_t)a->B * a->K * bs_nslice(a) * (2 + 2 * 2 * a->K) * sizeof(float);
}

int mopk_beam_step(const MopkBeamArgs *a, void *stream) {
    const int rc = bs_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->pos, a->scores, a->next_ids, a->parents, a->hist, a->rows, a->fin_tokens, a->fin_scores, a->fin_count, a->done, a->workspace))
        return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    switch (a->K) {
        case 1: bs_launch<2>(a, st); break;
        case 2: bs_launch<4>(a, st); break;
        case 3: bs_launch<6>(a, st); break;
        case 4: bs_launch<8>(a, st); break;
        case 5: bs_launch<10>(a, st); break;
        case 6: bs_launch<12>(a, st); break;
        case 7: bs_launch<14>(a, st); break;
        default: bs_launch<16>(a, st); break;
    }
    return launch_status();
}

}  // extern "C"
