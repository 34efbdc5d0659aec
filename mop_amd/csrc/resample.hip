// Sample-rate conversion of a batch of waveforms (ops.resample, the stage in front of the log-mel kernels; inference only):
// the windowed-sinc polyphase resampler.  include/mopk.h states the definition.  One launch, fp32, no atomics, no workspace.
//
// rs_kernel: one workgroup (4 waves) per (tile of RS_TILE consecutive outputs, clip).
//   1. The tile's outputs m0 .. m0 + live - 1 belong to the input frames f0 .. f0 + nf (f = m / n); together they read the
//      contiguous samples [f0 o - w, (f0 + nf) o - w + 2 w + o) of the clip.  That span goes to LDS once, a lane taking 16 bytes
//      of consecutive samples per channel in one load where the sample stride is 1 and all of them lie inside the clip, and
//      sample by sample elsewhere (the clip's ends, a strided view).  The dtype conversion, the channel mean (ascending
//      channels, fp32, one product with the fp32 reciprocal of C) and the [0, len_b) bound happen here; a sample outside the
//      bound is a zero that is never loaded.
//   2. The compact tap table (n rows of S taps, an odd row stride so that consecutive phases fall into different banks) and the
//      first-tap indices go to LDS beside the span when both fit 64 KiB; otherwise they are read where they are (L2).
//   3. Output i of the tile: r = p0 + i, df = r / n, p = r mod n (32-bit: one 64-bit division per workgroup gave f0 and p0), an
//      fmaf chain over the S taps of phase p in ascending order on the span at df o + first[p].  first[p] is clamped so that
//      the chain stays inside the span whatever the table says.  Neighbouring lanes take neighbouring outputs: contiguous stores.
//   Outputs >= len_out_b of the tile are written as zeros; workgroup 0 of a clip writes out_lens[b].
// Nothing a workgroup computes depends on another clip or on the grid: a clip's samples are bit-identical to the clip run alone.
#include "common.h"

namespace mopk {
namespace {

constexpr int RS_TILE = 1024;                       // outputs per workgroup (ops.RESAMPLE_TILE)
constexpr int RS_THREADS = 256;
constexpr int RS_MAX_SPAN = 12288;                  // staged samples per workgroup: 48 KiB
constexpr int RS_MAX_C = 64;
constexpr int RS_MAX_TABLE = 1 << 22;               // n * table_ld
constexpr int RS_LDS_BYTES = 65536;                 // the default limit of a launch: no attribute to raise
constexpr int RS_I16 = 3;                           // audio_dtype: int16 (beside MOPK_F32, MOPK_BF16, MOPK_LOG_MEL_F16)

__device__ __forceinline__ float rs_cvt(float v) { return v; }
__device__ __forceinline__ float rs_cvt(unsigned short v) { return bf2f(v); }
__device__ __forceinline__ float rs_cvt(_Float16 v) { return (float)v; }
__device__ __forceinline__ float rs_cvt(short v) { return (float)v * 0x1p-15f; }

// 16 bytes of consecutive samples in one load.  The address is only element-aligned (a span starts where its tile's first tap
// falls): gfx950 global loads take any alignment, and the copy below tells the compiler no more than that.
template <typename TIN> struct RsRaw { TIN e[16 / sizeof(TIN)]; };
template <typename TIN> __device__ __forceinline__ RsRaw<TIN> rs_ld16(const TIN *p) {
    RsRaw<TIN> r;
    __builtin_memcpy(&r, p, 16);
    return r;
}

// the largest span a tile stages: its outputs touch at most (RS_TILE + n - 2) / n + 1 input frames
inline int64_t rs_span(const MopkResampleArgs *a) { return (int64_t)((RS_TILE + a->n - 2) / a->n) * a->o + 2 * (int64_t)a->w + a->o; }
inline int64_t rs_table_bytes(const MopkResampleArgs *a) { return ((int64_t)a->n * a->table_ld + a->n) * 4; }

template <typename TIN, typename TOUT, bool TAB_LDS>
__global__ __launch_bounds__(RS_THREADS) void rs_kernel(MopkResampleArgs a, int span_max, float inv_c) {
    extern __shared__ __align__(16) float rs_smem[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int len = a.lens ? min(max(a.lens[b], 0), a.L) : a.L;
    const int len_out = (int)(((int64_t)a.n * len + a.o - 1) / a.o);           // <= Lout
    const int64_t m0 = (int64_t)blockIdx.x * RS_TILE;
    const int cnt = (int)min((int64_t)RS_TILE, (int64_t)a.Lout - m0);           // outputs of this tile, >= 1
    const int live = (int)min((int64_t)cnt, max((int64_t)0, (int64_t)len_out - m0));
    TOUT *out = (TOUT *)a.out + (int64_t)b * a.Lout + m0;
    if (blockIdx.x == 0 && tid == 0 && a.out_lens) a.out_lens[b] = len_out;
    for (int i = live + tid; i < cnt; i += RS_THREADS) st_from_f32<TOUT>(out + i, 0.f);
    if (live == 0) return;                                                      // the whole workgroup: a tile of padding

    // 1. the span of input samples this tile reads
    const int64_t f0 = m0 / a.n;
    const int p0 = (int)(m0 - f0 * a.n);
    const int nf = (p0 + live - 1) / a.n;                                       // <= (RS_TILE + n - 2) / n
    const int taps = 2 * a.w + a.o, nspan = nf * a.o + taps;                    // <= span_max
    const int64_t x0 = f0 * a.o - a.w;
    float *xs = rs_smem;
    const TIN *x = (const TIN *)a.audio + (int64_t)b * a.audio_sb;
    constexpr int V = 16 / (int)sizeof(TIN);                                    // samples per 16-byte load
    const bool unit = a.audio_sl == 1;
    for (int g = tid * V; g < nspan; g += RS_THREADS * V) {
        const int64_t q = x0 + g;
        if (unit && q >= 0 && q + V <= len && g + V <= nspan) {                 // V samples inside the clip: one load per channel
            float v[V];
            const TIN *px = x + q;
            const RsRaw<TIN> r0 = rs_ld16<TIN>(px);
#pragma unroll
            for (int u = 0; u < V; ++u) v[u] = rs_cvt(r0.e[u]);
            for (int c = 1; c < a.C; ++c) {
                const RsRaw<TIN> r = rs_ld16<TIN>(px + c * a.audio_sc);
#pragma unroll
                for (int u = 0; u < V; ++u) v[u] += rs_cvt(r.e[u]);
            }
#pragma unroll
            for (int u = 0; u < V; ++u) xs[g + u] = a.C > 1 ? v[u] * inv_c : v[u];
        } else {                                                                // the clip's ends, the span's end, a sample stride
            for (int u = 0; u < V && g + u < nspan; ++u) {
                const int64_t qu = q + u;
                float v = 0.f;
                if (qu >= 0 && qu < len) {
                    const TIN *px = x + qu * a.audio_sl;
                    v = rs_cvt(*px);
                    for (int c = 1; c < a.C; ++c) v += rs_cvt(px[c * a.audio_sc]);
                    if (a.C > 1) v *= inv_c;
                }
                xs[g + u] = v;
            }
        }
    }

    // 2. the table
    const float *tab = a.table;
    const int *fs = a.first;
    if (TAB_LDS) {
        float *t = rs_smem + span_max;
        int *f = (int *)(t + a.n * a.table_ld);
        for (int i = tid; i < a.n * a.table_ld; i += RS_THREADS) t[i] = a.table[i];
        for (int i = tid; i < a.n; i += RS_THREADS) f[i] = a.first[i];
        tab = t;
        fs = f;
    }
    __syncthreads();

    // 3. the outputs
    const int jmax = taps - a.S;                                                // >= 0
    for (int i = tid; i < live; i += RS_THREADS) {
        const int r = p0 + i, df = r / a.n, p = r - df * a.n;                   // df <= nf
        const int j0 = min(max(fs[p], 0), jmax);
        const float *xr = xs + df * a.o + j0, *kr = tab + (int64_t)p * a.table_ld;      // xr[S - 1] is at most xs[nspan - 1]
        float acc = 0.f;
        for (int s = 0; s < a.S; ++s) acc = fmaf(kr[s], xr[s], acc);
        st_from_f32<TOUT>(out + i, acc);
    }
}

int rs_check(const MopkResampleArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->C <= 0 || a->L <= 0 || a->Lout <= 0 || a->o <= 0 || a->n <= 0 || a->w < 0 || a->S <= 0 || a->table_ld <= 0)
        return MOPK_ERR_BAD_SHAPE;
    if (a->B > 65535 || a->C > RS_MAX_C || a->S > a->table_ld || (int64_t)a->n * a->table_ld > RS_MAX_TABLE) return MOPK_ERR_BAD_SHAPE;
    if (2 * (int64_t)a->w + a->o < a->S || rs_span(a) > RS_MAX_SPAN) return MOPK_ERR_BAD_SHAPE;
    if (((int64_t)a->n * a->L + a->o - 1) / a->o != a->Lout) return MOPK_ERR_BAD_SHAPE;         // which also keeps it below 2^31
    if (a->audio_dtype != MOPK_F32 && a->audio_dtype != MOPK_BF16 && a->audio_dtype != MOPK_LOG_MEL_F16 && a->audio_dtype != RS_I16)
        return MOPK_ERR_BAD_ARG;
    if (a->out_dtype != MOPK_F32 && a->out_dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    const uintptr_t am = a->audio_dtype == MOPK_F32 ? 3 : 1, om = a->out_dtype == MOPK_F32 ? 3 : 1;
    if (misaligned(am, a->audio) || misaligned(om, a->out) || misaligned(3, a->lens, a->table, a->first, a->out_lens))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <typename TIN, typename TOUT> int rs_launch(const MopkResampleArgs *a, hipStream_t st) {
    const int span_max = (int)rs_span(a);
    const bool tab_lds = (int64_t)span_max * 4 + rs_table_bytes(a) <= RS_LDS_BYTES;
    const size_t lds = (size_t)span_max * 4 + (tab_lds ? (size_t)rs_table_bytes(a) : 0);
    const dim3 grid((unsigned)(((int64_t)a->Lout + RS_TILE - 1) / RS_TILE), (unsigned)a->B);
    const float inv_c = 1.0f / (float)a->C;                                     // rounded once, on the host
    if (tab_lds) hipLaunchKernelGGL((rs_kernel<TIN, TOUT, true>), grid, dim3(RS_THREADS), lds, st, *a, span_max, inv_c);
    else hipLaunchKernelGGL((rs_kernel<TIN, TOUT, false>), grid, dim3(RS_THREADS), lds, st, *a, span_max, inv_c);
    return launch_status();
}

template <typename TIN> int rs_launch_out(const MopkResampleArgs *a, hipStream_t st) {
    return a->out_dtype == MOPK_F32 ? rs_launch<TIN, float>(a, st) : rs_launch<TIN, unsigned short>(a, st);
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_resample_supported(const MopkResampleArgs *a) { return rs_check(a) == MOPK_OK; }

int mopk_resample(const MopkResampleArgs *a, void *stream) {
    const int rc = rs_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->audio, a->table, a->first, a->out)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->audio_dtype == MOPK_F32) return rs_launch_out<float>(a, st);
    if (a->audio_dtype == MOPK_BF16) return rs_launch_out<unsigned short>(a, st);
    if (a->audio_dtype == MOPK_LOG_MEL_F16) return rs_launch_out<_Float16>(a, st);
    return rs_launch_out<short>(a, st);
}

}  // extern "C"
