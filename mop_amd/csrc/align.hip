// Token-level timestamps (WhisperMoP.align_tokens; inference only): Whisper's alignment filter and its dynamic time warping.
// include/mopk.h states both ops.  Neither kernel uses an atomic, every reduction has a fixed order (bitwise reproducible), and
// the per-item lengths are read from device memory: no host synchronisation.
//
// ac_cost_kernel, one workgroup of 1024 threads per (column tile, item), loops over the S heads.  The head's n_tokens x (tile + 2 halo)
// slab lives in LDS (the halo columns are the reflect-padded neighbours inside the item's own n_frames columns).  Thread t owns
// slab column t % W and the rows t / W, t / W + parts, ... through the load, both statistics passes (the mean first, then the
// squared deviations from it) and the normalisation, so only the two column reductions need a barrier.  In the filter pass a thread
// owns up to AC_KMAX fixed outputs (column t % tile, rows t / tile + k * 1024 / tile), takes each median by compare-exchanges in
// registers and adds the heads up in registers in index order.  tile is 64 columns up to N = 448 rows, 32 up to 896, 16 up to 1024:
// the slab stays within 144 KB and a thread within AC_KMAX outputs.
//
// dtw_kernel, one workgroup per item with one thread per row, walks the anti-diagonals: thread i takes cell (i, d - i) of diagonal
// d.  Its left neighbour D[i, j-1] is its own last value and D[i-1, j-1] is the D[i-1, j] it read one diagonal earlier, so one value
// per diagonal crosses threads, through two LDS rows indexed by the diagonal's parity with one barrier per diagonal.  The costs of
// eight diagonals are fetched ahead into registers.  Every cell's step code goes to the workspace; wave 0 then walks the path back
// from the last cell, reading up to 64 codes of a row at once to jump over a run of left steps, and lane 0 writes starts / ends.
#include "common.h"

namespace mopk {
namespace {

constexpr int AC_THREADS = 1024;
constexpr int AC_KMAX = 28;                                     // filter outputs per thread: N * tile <= AC_KMAX * AC_THREADS
constexpr int AC_MAXN = 1024, AC_MAXWIDTH = 9;
constexpr int AC_MAXW = 64 + AC_MAXWIDTH - 1;                   // slab columns

__host__ __device__ inline int ac_tile_log2(int N) { return N <= 448 ? 6 : N <= 896 ? 5 : 4; }
inline size_t ac_lds_bytes(int N, int width) {
    const int W = (1 << ac_tile_log2(N)) + width - 1;
    return ((size_t)N * W + AC_THREADS + 2 * AC_MAXW) * sizeof(float);
}

// the median of w[0..WIDTH): WIDTH / 2 + 1 bubble passes leave the largest values in order at the top
template <int WIDTH> __device__ __forceinline__ float ac_median(float (&w)[WIDTH]) {
#pragma unroll
    for (int p = 0; p <= WIDTH / 2; ++p)
#pragma unroll
        for (int e = 0; e + 1 < WIDTH - p; ++e) {
            const float lo = fminf(w[e], w[e + 1]), hi = fmaxf(w[e], w[e + 1]);
            w[e] = lo;
            w[e + 1] = hi;
        }
    return w[WIDTH / 2];
}

template <int WIDTH>
__global__ __launch_bounds__(AC_THREADS) void ac_cost_kernel(MopkAlignCostArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int H = WIDTH / 2;
    const int tl = ac_tile_log2(a.N), tile = 1 << tl, W = tile + 2 * H;
    const int t = threadIdx.x, b = blockIdx.y, j0 = blockIdx.x * tile;
    const int nt = min(max(a.n_tokens[b], 0), a.N), nf = min(max(a.n_frames[b], 0), a.M);
    if (nt == 0 || j0 >= nf) return;                            // the same for the whole workgroup
    float *slab = (float *)smem;                                // nt rows of W
    float *red = slab + (size_t)a.N * W;                        // AC_THREADS partial sums, red[part * W + c]
    float *mu = red + AC_THREADS, *sd = mu + AC_MAXW;
    const bool filt = nf > H;                                   // Whisper skips the filter on a map of <= width / 2 columns

    // statistics ownership: slab column c, rows part, part + parts, ...
    const int parts = AC_THREADS / W, c = t % W, part = t / W;
    int src = j0 - H + c;                                       // the column of probs behind slab column c
    bool own = part < parts;
    if (filt) {
        own = own && src <= nf - 1 + H;
        src = src < 0 ? -src : src >= nf ? 2 * (nf - 1) - src : src;        // reflect: nf > H keeps it inside [0, nf)
    } else {
        own = own && src >= 0 && src < nf;
    }
    // filter ownership: output column j0 + jo, rows io, io + rpp, ...
    const int jo = t & (tile - 1), io = t >> tl, rpp = AC_THREADS >> tl;
    const bool out_col = j0 + jo < nf;
    float acc[AC_KMAX];
#pragma unroll
    for (int k = 0; k < AC_KMAX; ++k) acc[k] = 0.f;
    const float fn = (float)nt;

    for (int s = 0; s < a.S; ++s) {
        const float *p = a.probs + (int64_t)b * a.probs_sb + (int64_t)s * a.probs_ss + src;
        float sum = 0.f;
        if (own)
            for (int i = part; i < nt; i += parts) {
                const float v = p[(int64_t)i * a.probs_sn];
                slab[i * W + c] = v;
                sum += v;
            }
        red[t] = sum;
        __syncthreads();
        if (t < W) {
            float m = red[t];
            for (int q = 1; q < parts; ++q) m += red[q * W + t];
            mu[t] = m / fn;
        }
        __syncthreads();
        const float m = mu[c];
        float sq = 0.f;
        if (own)
            for (int i = part; i < nt; i += parts) {
                const float d = slab[i * W + c] - m;
                sq += d * d;
            }
        red[t] = sq;
        __syncthreads();
        if (t < W) {
            float v = red[t];
            for (int q = 1; q < parts; ++q) v += red[q * W + t];
            sd[t] = sqrtf(v / fn);
        }
        __syncthreads();
        const float dv = sd[c];
        if (own)
            for (int i = part; i < nt; i += parts) slab[i * W + c] = (slab[i * W + c] - m) / dv;
        __syncthreads();
        if (out_col) {
#pragma unroll
            for (int k = 0; k < AC_KMAX; ++k) {
                const int i = io + k * rpp;
                if (i < nt) {
                    const float *z = slab + i * W + jo;
                    if (filt) {
                        float w[WIDTH];
#pragma unroll
                        for (int e = 0; e < WIDTH; ++e) w[e] = z[e];
                        acc[k] += ac_median<WIDTH>(w);
                    } else {
                        acc[k] += z[H];
                    }
                }
            }
        }
        __syncthreads();                                        // the next head overwrites the slab
    }
    if (out_col) {
        float *y = a.cost + (int64_t)b * a.cost_sb + j0 + jo;
        const float S = (float)a.S;
#pragma unroll
        for (int k = 0; k < AC_KMAX; ++k) {
            const int i = io + k * rpp;
            if (i < nt) y[(int64_t)i * a.cost_ld] = -(acc[k] / S);
        }
    }
}

int ac_check(const MopkAlignCostArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->S <= 0 || a->N <= 0 || a->M <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->width < 1 || a->width % 2 == 0) return MOPK_ERR_BAD_ARG;
    if (a->cost_ld < a->M) return MOPK_ERR_BAD_ARG;
    if (a->N > AC_MAXN || a->width > AC_MAXWIDTH || a->B > 65535) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(3, a->probs, a->cost, a->n_tokens, a->n_frames)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <int WIDTH> int ac_launch(const MopkAlignCostArgs *a, hipStream_t st) {
    const size_t lds = ac_lds_bytes(a->N, WIDTH);
    const int tile = 1 << ac_tile_log2(a->N);
    // the raised dynamic-LDS limit is kept per (instantiation, device) by launch_big_lds: it may not be set during stream capture
    return launch_big_lds<ac_cost_kernel<WIDTH>>(dim3((unsigned)((a->M + tile - 1) / tile), (unsigned)a->B), dim3(AC_THREADS), lds, st, *a);
}

// ---- dynamic time warping ----
constexpr int DTW_MAXR = 1024;
constexpr int DTW_AHEAD = 8;                                    // diagonals whose costs are fetched ahead

__global__ __launch_bounds__(DTW_MAXR) void dtw_kernel(MopkDtwArgs a) {
    __shared__ float diag[2][DTW_MAXR];
    const int i = threadIdx.x, b = blockIdx.x, lane = i & 63;
    const int Rw = a.N - a.row0;                                // rows of the workspace of one item
    const int R = min(max(a.n_rows[b], 0), a.N) - a.row0, Cn = min(max(a.n_cols[b], 0), a.M);
    int32_t *starts = a.starts + (int64_t)b * a.N, *ends = a.ends + (int64_t)b * a.N;
    for (int r = i; r < a.N; r += blockDim.x) starts[r] = ends[r] = -1;
    if (R <= 0 || Cn <= 0) return;                              // the same for the whole workgroup
    uint8_t *trace = (uint8_t *)a.workspace + (int64_t)b * Rw * a.M;
    const bool row = i < R;
    const float *x = a.cost + (int64_t)b * a.cost_sb + (int64_t)(a.row0 + (row ? i : 0)) * a.cost_ld;
    uint8_t *tr = trace + (int64_t)(row ? i : 0) * a.M;

    float left = INFINITY;                                      // D[i, j-1]
    float corner = i == 0 ? 0.f : INFINITY;                     // D[i-1, j-1]: the D[i-1, j] of the diagonal before
    const int nd = R + Cn - 1;
    for (int d0 = 0; d0 < nd; d0 += DTW_AHEAD) {
        float xr[DTW_AHEAD];
#pragma unroll
        for (int k = 0; k < DTW_AHEAD; ++k) {
            const int j = d0 + k - i;
            xr[k] = row && j >= 0 && j < Cn ? x[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < DTW_AHEAD; ++k) {
            const int d = d0 + k, j = d - i;
            if (row && j >= 0 && j < Cn) {
                const float c0 = corner, c1 = i > 0 ? diag[(d - 1) & 1][i - 1] : INFINITY, c2 = left;
                float cmin;
                int step;
                if (c0 < c1 && c0 < c2) { cmin = c0; step = 0; }
                else if (c1 < c0 && c1 < c2) { cmin = c1; step = 1; }
                else { cmin = c2; step = 2; }
                left = xr[k] + cmin;
                corner = c1;
                diag[d & 1][i] = left;
                tr[j] = (uint8_t)step;
            }
            __syncthreads();
        }
    }
    // the walk back (wave 0): row 0 goes left to column 0 and column 0 goes up to row 0, as Whisper's borders say
    if (i >= 64) return;
    int r = R - 1, j = Cn - 1;
    if (lane == 0) ends[a.row0 + r] = j;
    while (r > 0) {
        const int jj = j - lane;
        const int code = jj > 0 ? trace[(int64_t)r * a.M + jj] : 1;          // lanes past column 0 stop at it, too
        const unsigned long long stop = __ballot(code != 2);
        if (stop == 0) { j -= 64; continue; }
        const int l = __ffsll((long long)stop) - 1;
        const int cl = __shfl(code, l, 64);
        j = max(j - l, 0);
        if (lane == 0) starts[a.row0 + r] = j;
        if (cl == 0) --j;
        --r;
        if (lane == 0) ends[a.row0 + r] = j;
    }
    if (lane == 0) starts[a.row0] = 0;
}

int dtw_check(const MopkDtwArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->N <= 0 || a->M <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->row0 < 0 || a->row0 >= a->N || a->cost_ld < a->M) return MOPK_ERR_BAD_ARG;
    if (a->N - a->row0 > DTW_MAXR) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(3, a->cost, a->n_rows, a->n_cols, a->starts, a->ends)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_alignment_cost_supported(const MopkAlignCostArgs *a) { return ac_check(a) == MOPK_OK; }

int mopk_alignment_cost(const MopkAlignCostArgs *a, void *stream) {
    const int rc = ac_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->probs, a->cost, a->n_tokens, a->n_frames)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    switch (a->width) {
        case 1: return ac_launch<1>(a, st);
        case 3: return ac_launch<3>(a, st);
        case 5: return ac_launch<5>(a, st);
        case 7: return ac_launch<7>(a, st);
        default: return ac_launch<9>(a, st);
    }
}

int mopk_dtw_align_supported(const MopkDtwArgs *a) { return dtw_check(a) == MOPK_OK; }

size_t mopk_dtw_workspace_bytes(const MopkDtwArgs *a) {
    if (!a || a->B <= 0 || a->N <= 0 || a->M <= 0 || a->row0 < 0 || a->row0 >= a->N) return 0;
    return (size_t)a->B * (size_t)(a->N - a->row0) * (size_t)a->M;
}

int mopk_dtw_align(const MopkDtwArgs *a, void *stream) {
    const int rc = dtw_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->cost, a->n_rows, a->n_cols, a->starts, a->ends, a->workspace)) return MOPK_ERR_BAD_ARG;
    const int threads = (a->N - a->row0 + WAVE - 1) / WAVE * WAVE;
    hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)a->B), dim3(threads), 0, (hipStream_t)stream, *a);
    return launch_status();
}

}  // extern "C"
