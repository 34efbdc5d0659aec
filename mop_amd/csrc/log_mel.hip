// Whisper's log-mel spectrogram of a batch of waveforms (LogMelFrontend; inference only).  include/mopk.h states the definition.
// Two launches, fp32 throughout, no atomics, no host synchronisation.
//
// lm_tile_kernel: one workgroup (4 waves) per (tile of 32 frames, clip).
//   1. The twiddle table (n_fft x (cos, sin)) and the tile's 32 windowed frames go to LDS.  The frames are stored as a matrix
//      [frame][n] with a row stride of n_fft + 1 dwords although neighbouring frames share samples: a lane of the MFMA's A operand
//      is a frame, and 32 frames at one n then fall into 32 different banks (the raw samples, hop apart, would not).  A sample index
//      is reflected at the clip's own ends, from len_b read on the device; a frame >= T_b is a row of zeros.
//   2. DFT: per 32 bins two 32x32 accumulators (re, im) on v_mfma_f32_32x32x2_f32, n_fft / 2 steps of k = 2.  A = frames
//      (row = frame, k = n), B = twiddles (k = n, column = bin), read at (n * bin) mod n_fft, an integer kept per lane and advanced
//      by (2 * bin) mod n_fft per step: no angle is ever rounded.  Wave w owns the bin tiles w, w + 4, w + 8 (n_fft = 400: seven
//      tiles), all in flight at once so one read of A feeds them all.  The MFMA is an exact fp32 fma chain in n order.
//   3. P = re^2 + im^2 goes to LDS over the frames (one barrier), [frame][bin] with an odd row stride.
//   4. Filterbank: output e = frame * n_mels + m of the tile belongs to thread e mod 256, so the stores are contiguous; the sum
//      runs over the filter's band [lo, hi) in ascending k (the caller's band table, or every bin without one).  G = log10(max(M,
//      1e-10)) goes to the output (fp32) or the workspace (bf16 output), the tile's maximum over its valid frames to the
//      workspace word of this (clip, tile): a tile without a valid frame writes -inf and does nothing else.
// lm_finish_kernel: one workgroup per (4096 outputs, clip): the maximum of the clip's tile words (a fixed order: bit-repeatable),
//   then out = (max(G, max - 8) + 4) / 4 for t < T_b and 0 behind.
#include "common.h"

namespace mopk {
namespace {

constexpr int LM_F = MOPK_LOG_MEL_TILE_FRAMES;      // frames per tile = rows of the 32x32 MFMA
constexpr int LM_THREADS = 256, LM_WAVES = LM_THREADS / WAVE;
constexpr int LM_CHUNK = 4096;                      // outputs per workgroup of the second launch
constexpr int LM_MAX_FFT = 512, LM_MIN_FFT = 16, LM_MAX_MELS = 128;

template <typename T> __device__ __forceinline__ float lm_ld(const T *p);
template <> __device__ __forceinline__ float lm_ld<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float lm_ld<unsigned short>(const unsigned short *p) { return bf2f(*p); }
template <> __device__ __forceinline__ float lm_ld<_Float16>(const _Float16 *p) { return (float)*p; }

__host__ __device__ inline int lm_bins(int n_fft) { return n_fft / 2 + 1; }
__host__ __device__ inline int lm_bin_tiles(int n_fft) { return (lm_bins(n_fft) + 31) / 32; }
__host__ __device__ inline int lm_p_stride(int n_fft) { return lm_bin_tiles(n_fft) * 32 + 1; }
__host__ __device__ inline int lm_tiles(int T) { return (T + LM_F - 1) / LM_F; }
inline size_t lm_lds_bytes(int n_fft) {             // twiddles, then the frames / the power (the larger of the two)
    const int buf = LM_F * (n_fft + 1) > LM_F * lm_p_stride(n_fft) ? LM_F * (n_fft + 1) : LM_F * lm_p_stride(n_fft);
    return sizeof(float) * (size_t)(2 * n_fft + buf);
}
__device__ __forceinline__ int lm_len(const MopkLogMelArgs &a, int b) { return a.lens ? min(max(a.lens[b], 0), a.L) : a.L; }

template <typename TIN, int TPW>
__global__ __launch_bounds__(LM_THREADS) void lm_tile_kernel(MopkLogMelArgs a, float *g_out, float *part) {
    extern __shared__ __align__(16) float lm_smem[];
    __shared__ float red[LM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tile = blockIdx.x, b = blockIdx.y, t0 = tile * LM_F;
    const int N = a.n_fft, nb = lm_bins(N), nbt = lm_bin_tiles(N), AS = N + 1, PS = lm_p_stride(N);
    const int T = a.L / a.hop, len = lm_len(a, b), Tb = len / a.hop;
    if (t0 >= Tb) {                                             // the whole workgroup: a tile of padding frames
        if (tid == 0) part[(int64_t)b * gridDim.x + tile] = -INFINITY;
        return;
    }
    float2 *tw = (float2 *)lm_smem;
    float *buf = lm_smem + 2 * N;

    // 1. twiddles and windowed frames
    for (int i = tid; i < N; i += LM_THREADS) tw[i] = ((const float2 *)a.twiddle)[i];
    const TIN *x = (const TIN *)a.audio + (int64_t)b * a.audio_ld;
    for (int r = 0; r < LM_F / LM_WAVES; ++r) {
        const int t = wv * (LM_F / LM_WAVES) + r;
        const int64_t first = (int64_t)(t0 + t) * a.hop - N / 2;
        for (int n = lane; n < N; n += WAVE) {
            int64_t q = first + n;
            q = q < 0 ? -q : q;
            q = q >= len ? 2 * (int64_t)(len - 1) - q : q;
            const bool in = t0 + t < Tb && q >= 0 && q < len;
            buf[t * AS + n] = in ? a.window[n] * lm_ld<TIN>(x + q) : 0.f;
        }
    }
    __syncthreads();

    // 2. the DFT of the tile's frames
    const int kh = lane >> 5, j = lane & 31;
    f32x16 re[TPW], im[TPW];
    int idx[TPW], inc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int k = (wv + LM_WAVES * i) * 32 + j;             // bins past n_fft / 2 are computed (valid twiddles) and never used
        inc[i] = (2 * k) % N;
        idx[i] = (kh * k) % N;
#pragma unroll
        for (int c = 0; c < 16; ++c) re[i][c] = im[i][c] = 0.f;
    }
    const float *ap = buf + j * AS + kh;
    for (int s = 0; s < N / 2; ++s) {
        const float av = ap[2 * s];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            if (wv + LM_WAVES * i < nbt) {                      // the same for the whole wave
                const float2 c = tw[idx[i]];
                re[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, c.x, re[i], 0, 0, 0);
                im[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, c.y, im[i], 0, 0, 0);
                idx[i] += inc[i];
                idx[i] -= idx[i] >= N ? N : 0;
            }
        }
    }
    __syncthreads();                                            // every wave is done with the frames: the power takes their place

    // 3. the power, [frame][bin]
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        if (wv + LM_WAVES * i < nbt) {
            const int k = (wv + LM_WAVES * i) * 32 + j;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int t = (c & 3) + 8 * (c >> 2) + 4 * kh;
                buf[t * PS + k] = re[i][c] * re[i][c] + im[i][c] * im[i][c];
            }
        }
    }
    __syncthreads();

    // 4. filterbank, log, the tile's maximum
    const int M = a.n_mels, rows = min(LM_F, Tb - t0);          // rows >= 1
    float *g = g_out + ((int64_t)b * T + t0) * M;
    float mx = -INFINITY;
    for (int e = tid; e < rows * M; e += LM_THREADS) {
        const int t = e / M, m = e - t * M;
        const int lo = a.bands ? min(max(a.bands[2 * m], 0), nb) : 0, hi = a.bands ? min(max(a.bands[2 * m + 1], lo), nb) : nb;
        const float *f = a.filters + (int64_t)m * nb, *p = buf + t * PS;
        float acc = 0.f;
        for (int k = lo; k < hi; ++k) acc = fmaf(f[k], p[k], acc);
        // log10(max(M, 1e-10)), the floor itself exact.  Samples are taken to be finite: a NaN power lands on the floor here and
        // is dropped by the fmaxf below, where the torch composition would carry the NaN through the clip.
        const float v = acc > 1e-10f ? log10f(acc) : -10.f;
        g[e] = v;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LM_WAVES; ++w) mx = fmaxf(mx, red[w]);
        part[(int64_t)b * gridDim.x + tile] = mx;
    }
}

template <typename TOUT>
__global__ __launch_bounds__(LM_THREADS) void lm_finish_kernel(MopkLogMelArgs a, const float *g_in, const float *part, int ntiles) {
    __shared__ float red[LM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    const int T = a.L / a.hop, Tb = lm_len(a, b) / a.hop;
    float mx = -INFINITY;
    for (int i = tid; i < ntiles; i += LM_THREADS) mx = fmaxf(mx, part[(int64_t)b * ntiles + i]);
    mx = wave_max(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < LM_WAVES; ++w) mx = fmaxf(mx, red[w]);
    const float floor_ = mx - 8.f;
    const int64_t total = (int64_t)T * a.n_mels, valid = (int64_t)Tb * a.n_mels, base = (int64_t)b * total;
    const int64_t e0 = (int64_t)blockIdx.x * LM_CHUNK;
    TOUT *out = (TOUT *)a.out + base;
    for (int64_t e = e0 + tid; e < min(e0 + LM_CHUNK, total); e += LM_THREADS)
        st_from_f32<TOUT>(out + e, e < valid ? (fmaxf(g_in[base + e], floor_) + 4.f) * 0.25f : 0.f);
}

int lm_check(const MopkLogMelArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->L <= 0 || a->n_mels <= 0 || a->n_fft <= 0 || a->hop <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->n_fft % 2 || a->n_fft < LM_MIN_FFT || a->n_fft > LM_MAX_FFT || a->hop > a->n_fft || a->n_mels > LM_MAX_MELS)
        return MOPK_ERR_BAD_SHAPE;
    if (a->L < a->hop || a->L < a->n_fft / 2 + 1 || a->B > 65535) return MOPK_ERR_BAD_SHAPE;
    if (a->audio_dtype != MOPK_F32 && a->audio_dtype != MOPK_BF16 && a->audio_dtype != MOPK_LOG_MEL_F16) return MOPK_ERR_BAD_ARG;
    if (a->out_dtype != MOPK_F32 && a->out_dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->audio_ld < a->L) return MOPK_ERR_BAD_ARG;
    const uintptr_t am = a->audio_dtype == MOPK_F32 ? 3 : 1, om = a->out_dtype == MOPK_F32 ? 3 : 1;
    if (misaligned(am, a->audio) || misaligned(om, a->out) || misaligned(3, a->lens, a->filters, a->bands, a->window, a->workspace) ||
        misaligned(7, a->twiddle))
        return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <typename TIN> int lm_launch_tiles(const MopkLogMelArgs *a, float *g, float *part, int ntiles, hipStream_t st) {
    const size_t lds = lm_lds_bytes(a->n_fft);
    const int tpw = (lm_bin_tiles(a->n_fft) + LM_WAVES - 1) / LM_WAVES;        // 1 .. 3
    const dim3 grid((unsigned)ntiles, (unsigned)a->B), block(LM_THREADS);
    // the raised dynamic-LDS limit is kept per (instantiation, device) by launch_big_lds: it may not be set during stream capture
    // (named in the order 2, 3, 1: the order in which the code object has always held the three kernels)
    return tpw == 2 ? launch_big_lds<lm_tile_kernel<TIN, 2>>(grid, block, lds, st, *a, g, part)
         : tpw == 3 ? launch_big_lds<lm_tile_kernel<TIN, 3>>(grid, block, lds, st, *a, g, part)
                    : launch_big_lds<lm_tile_kernel<TIN, 1>>(grid, block, lds, st, *a, g, part);
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_log_mel_supported(const MopkLogMelArgs *a) { return lm_check(a) == MOPK_OK; }

size_t mopk_log_mel_workspace_bytes(const MopkLogMelArgs *a) {
    if (!a || a->B <= 0 || a->B > 65535 || a->L <= 0 || a->hop <= 0 || a->n_mels <= 0) return 0;      // B: the grid's y extent, as lm_check
    const int T = a->L / a->hop;
    Carver c(nullptr);
    c.take<float>((size_t)a->B * lm_tiles(T));
    if (a->out_dtype != MOPK_F32) c.take<float>((size_t)a->B * T * a->n_mels);
    return c.off;
}

int mopk_log_mel(const MopkLogMelArgs *a, void *stream) {
    const int rc = lm_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->audio, a->filters, a->twiddle, a->window, a->out, a->workspace)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int T = a->L / a->hop, ntiles = lm_tiles(T);
    Carver c(a->workspace);
    float *part = c.take<float>((size_t)a->B * ntiles);
    float *g = a->out_dtype == MOPK_F32 ? (float *)a->out : c.take<float>((size_t)a->B * T * a->n_mels);
    int rc1;
    if (a->audio_dtype == MOPK_F32) rc1 = lm_launch_tiles<float>(a, g, part, ntiles, st);
    else if (a->audio_dtype == MOPK_BF16) rc1 = lm_launch_tiles<unsigned short>(a, g, part, ntiles, st);
    else rc1 = lm_launch_tiles<_Float16>(a, g, part, ntiles, st);
    if (rc1 != MOPK_OK) return rc1;
    const dim3 grid((unsigned)(((int64_t)T * a->n_mels + LM_CHUNK - 1) / LM_CHUNK), (unsigned)a->B);
    if (a->out_dtype == MOPK_F32) hipLaunchKernelGGL(lm_finish_kernel<float>, grid, dim3(LM_THREADS), 0, st, *a, (const float *)g, (const float *)part, ntiles);
    else hipLaunchKernelGGL(lm_finish_kernel<unsigned short>, grid, dim3(LM_THREADS), 0, st, *a, (const float *)g, (const float *)part, ntiles);
    return launch_status();
}

}  // extern "C"
