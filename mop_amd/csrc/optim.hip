// Fused AdamW step over a list of tensors (mop_amd.optim.FusedAdamW, ops.adamw_step): the sum of squares of all gradients, the
// finalise that turns it into a norm, a clip coefficient and a skip flag, the update with an optional weight EMA, and the step
// counts.  include/mopk.h states the arithmetic and the launch count.  The tensor table travels as kernel arguments, one slice per
// launch; every quantity a later launch needs (norm, coefficient, skip flag, step counts, lr_dev) is read from device memory, so a
// call makes no host synchronisation and no copy, can be captured in a HIP graph, and its results are bitwise reproducible.
// Built without fast-math and with contraction off: the rounding count of every formula is the one the header states, and the
// vector and the element-by-element paths give the same bits.
#include "common.h"
#include "row_helpers.h"

#pragma clang fp contract(off)

namespace mopk {
namespace {

constexpr int AW_THREADS = 256;
constexpr int AW_WAVES = AW_THREADS / WAVE;
constexpr int AW_FIN_THREADS = 1024;
constexpr int AW_GRID_CAP = 2048;                               // update launches: capped grid, grid-stride over chunks
constexpr int64_t AW_CHUNK = MOPK_ADAMW_CHUNK;
constexpr int AW_TCAP = MOPK_ADAMW_MAX_TENSORS;
constexpr int AW_CCAP = MOPK_ADAMW_MAX_CHUNKS;

// one launch's share of the tensor list: part i covers chunks [chunk0[i], chunk0[i] + cstart[i + 1] - cstart[i]) of tensor t[i]
struct AwSlice {
    MopkOptimTensor t[AW_TCAP];
    int64_t chunk0[AW_TCAP];
    int32_t cstart[AW_TCAP + 1];                                // slice-relative prefix of the parts' chunk counts
    uint8_t last[AW_TCAP];                                      // this part holds its tensor's last chunk (or the tensor is empty)
    int32_t nt;
    int32_t reserved;
    int64_t partial0;                                           // index of the slice's first chunk among all chunks of the call
};
struct AwHyper {
    double lr, beta1, beta2, weight_decay;
    float eps, ema_b, ema_omb, reserved;
    const float *lr_dev;
    const MopkAdamWStats *stats;                                // NULL: coef 1, never skipped
};
static_assert(sizeof(AwSlice) + sizeof(AwHyper) + 64 <= 4096, "a slice and the hyper-parameters must fit the kernel-argument segment");

inline int64_t aw_chunks(int64_t n) { return (n + AW_CHUNK - 1) / AW_CHUNK; }

// part of slice s that holds slice-relative chunk c (nt <= 40 entries read through the scalar cache; c is uniform)
__device__ __forceinline__ int aw_part(const AwSlice &s, int c) {
    int i = 0;
    while (i + 1 < s.nt && s.cstart[i + 1] <= c) ++i;
    return i;
}

// ---- 1. sum of squares of all gradients: one workgroup per chunk, one fp32 partial per chunk ----
template <typename T>
__device__ __forceinline__ float aw_sumsq_chunk(const T *g, int len) {
    constexpr int EPV = RowSpan<T>::EPV;
    const int tid = threadIdx.x;
    const RowSpan<T> sp(g, len);
    const int head = sp.head, tail0 = sp.tail0;
    const uint4 *gv = (const uint4 *)(g + head);
    float acc = 0.f;
    if (tid < head) { const float f = ld_as_f32<T>(g + tid); acc += f * f; }
#pragma unroll 4
    for (int u = tid; u < sp.nvec; u += AW_THREADS) {
        float f[EPV];
        row_unpack(gv[u], f, T());
#pragma unroll
        for (int e = 0; e < EPV; ++e) acc += f[e] * f[e];
    }
    if (tid >= head && tid < head + (len - tail0)) { const float f = ld_as_f32<T>(g + tail0 + (tid - head)); acc += f * f; }
    return acc;
}

__global__ __launch_bounds__(AW_THREADS) void aw_sumsq_kernel(AwSlice s, float *partials) {
    __shared__ float ws[AW_WAVES];
    const int c = blockIdx.x;
    const int i = aw_part(s, c);
    const MopkOptimTensor &t = s.t[i];
    const int64_t off = (s.chunk0[i] + (c - s.cstart[i])) * AW_CHUNK;
    const int len = (int)min(AW_CHUNK, t.n - off);
    float acc = t.g_dtype == MOPK_BF16 ? aw_sumsq_chunk((const unsigned short *)t.g + off, len)
                                        : aw_sumsq_chunk((const float *)t.g + off, len);
    acc = wave_sum(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) ws[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = ws[0];
        for (int w = 1; w < AW_WAVES; ++w) acc += ws[w];
        partials[s.partial0 + c] = acc;
    }
}

// ---- 2. finalise: one workgroup ----
__global__ __launch_bounds__(AW_FIN_THREADS) void aw_finalise_kernel(const float *partials, int64_t n_partials, int clip, double max_norm,
                                                                     int skip_nonfinite, MopkAdamWStats *stats) {
    __shared__ double ws[AW_FIN_THREADS / WAVE];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t i = tid; i < n_partials; i += AW_FIN_THREADS) s += (double)partials[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & (WAVE - 1)) == 0) ws[tid / WAVE] = s;
    __syncthreads();
    if (tid == 0) {
        s = ws[0];
        for (int w = 1; w < AW_FIN_THREADS / WAVE; ++w) s += ws[w];
        const float norm = (float)sqrt(s);
        float coef = 1.f;
        if (clip) {
            const float c = (float)max_norm / (norm + 1e-6f);
            coef = c < 1.f ? c : (c != c ? c : 1.f);            // a NaN norm stays a NaN coefficient
        }
        const int skip = skip_nonfinite && !(fabsf(norm) <= 3.402823466e+38f);
        stats->norm = norm;
        stats->coef = coef;
        stats->skip = skip;
        stats->skipped += skip;
    }
}

// ---- 3. update ----
// G consecutive elements of one stream as floats: vector loads where the stream shares p's alignment, else one by one
template <typename T, int G>
__device__ __forceinline__ void aw_load(const T *x, bool vec, float (&f)[G]) {
    if (vec) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < G / 4; ++k) {
                float q[4];
                row_unpack(((const uint4 *)x)[k], q, float());
#pragma unroll
                for (int e = 0; e < 4; ++e) f[4 * k + e] = q[e];
            }
        } else if constexpr (G == 8) {
            row_unpack(*(const uint4 *)x, f, (unsigned short)0);
        } else {                                                // 4 bf16 beside an fp32 p: 8 bytes
            const uint2 u = *(const uint2 *)x;
            f[0] = __builtin_bit_cast(float, u.x << 16); f[1] = __builtin_bit_cast(float, u.x & 0xffff0000u);
            f[2] = __builtin_bit_cast(float, u.y << 16); f[3] = __builtin_bit_cast(float, u.y & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int e = 0; e < G; ++e) f[e] = ld_as_f32<T>(x + e);
    }
}
template <typename T, int G>
__device__ __forceinline__ void aw_store(T *x, bool vec, const float (&f)[G]) {
    if (vec) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < G / 4; ++k)
                ((uint4 *)x)[k] = make_uint4(__builtin_bit_cast(unsigned int, f[4 * k]), __builtin_bit_cast(unsigned int, f[4 * k + 1]),
                                             __builtin_bit_cast(unsigned int, f[4 * k + 2]), __builtin_bit_cast(unsigned int, f[4 * k + 3]));
        } else {
            static_assert(G == 8, "a bf16 parameter is walked in groups of 8");
            *(uint4 *)x = make_uint4(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7]));
        }
    } else {
#pragma unroll
        for (int e = 0; e < G; ++e) st_from_f32<T>(x + e, f[e]);
    }
}

// the constants of one tensor's update, from its step count
struct AwConst { float coef, decay, b1, omb1, b2, omb2, step_size, sqrt_bc2, eps, ema_b, ema_omb; };

__device__ __forceinline__ double aw_powi(double b, unsigned int k) {       // b^k by repeated squaring
    double r = 1.0;
    while (k) {
        if (k & 1u) r *= b;
        b *= b;
        k >>= 1;
    }
    return r;
}

__device__ __forceinline__ void aw_elem(const AwConst &k, float &p, float g, float &m, float &v) {
    const float gp = k.coef * g;
    p = p * k.decay;
    m = k.b1 * m + k.omb1 * gp;
    v = k.b2 * v + (k.omb2 * gp) * gp;
    const float denom = sqrtf(v) / k.sqrt_bc2 + k.eps;
    p = p - k.step_size * (m / denom);
}
__device__ __forceinline__ float aw_ema(const AwConst &k, float ema, float p) { return k.ema_b * ema + k.ema_omb * p; }

// PT: what is stored for p and ema, and what the next step reads back
template <typename PT> __device__ __forceinline__ float aw_stored(float p);
template <> __device__ __forceinline__ float aw_stored<float>(float p) { return p; }
template <> __device__ __forceinline__ float aw_stored<unsigned short>(float p) { return bf2f(f2bf(p)); }

template <typename PT, typename GT, bool EMA>
__device__ __forceinline__ void aw_update_chunk(const AwConst &k, PT *p, const GT *g, float *m, float *v, PT *ema, int len) {
    constexpr int G = RowSpan<PT>::EPV;
    const int tid = threadIdx.x;
    const RowSpan<PT> sp(p, len);
    const int head = sp.head, tail0 = sp.tail0;
    // a stream is read in vectors when its element `head` lies on the vector's boundary (16 bytes; 8 for 4 bf16 gradients)
    const bool gvec = (((uintptr_t)(g + head)) & (G * sizeof(GT) >= 16 ? 15 : 7)) == 0;
    const bool mvec = (((uintptr_t)(m + head)) & 15) == 0, vvec = (((uintptr_t)(v + head)) & 15) == 0;
    const bool evec = EMA && (((uintptr_t)(ema + head)) & 15) == 0;
    for (int u = tid; u < sp.nvec; u += AW_THREADS) {
        const int e0 = head + u * G;
        float fp[G], fg[G], fm[G], fv[G], fe[G];
        aw_load<PT, G>(p + e0, true, fp);
        aw_load<GT, G>(g + e0, gvec, fg);
        aw_load<float, G>(m + e0, mvec, fm);
        aw_load<float, G>(v + e0, vvec, fv);
        if (EMA) aw_load<PT, G>(ema + e0, evec, fe);
#pragma unroll
        for (int e = 0; e < G; ++e) {
            aw_elem(k, fp[e], fg[e], fm[e], fv[e]);
            if (EMA) fe[e] = aw_ema(k, fe[e], aw_stored<PT>(fp[e]));
        }
        aw_store<PT, G>(p + e0, true, fp);
        aw_store<float, G>(m + e0, mvec, fm);
        aw_store<float, G>(v + e0, vvec, fv);
        if (EMA) aw_store<PT, G>(ema + e0, evec, fe);
    }
    if (tid < head + (len - tail0)) {
        const int e = tid < head ? tid : tail0 + (tid - head);
        float fp = ld_as_f32<PT>(p + e), fm = m[e], fv = v[e];
        aw_elem(k, fp, ld_as_f32<GT>(g + e), fm, fv);
        st_from_f32<PT>(p + e, fp);
        m[e] = fm;
        v[e] = fv;
        if (EMA) st_from_f32<PT>(ema + e, aw_ema(k, ld_as_f32<PT>(ema + e), aw_stored<PT>(fp)));
    }
}

template <typename PT, bool EMA>
__device__ __forceinline__ void aw_update_g(const AwConst &k, const MopkOptimTensor &t, int64_t off, int len) {
    if (t.g_dtype == MOPK_BF16)
        aw_update_chunk<PT, unsigned short, EMA>(k, (PT *)t.p + off, (const unsigned short *)t.g + off, t.m + off, t.v + off,
                                                 EMA ? (PT *)t.ema + off : nullptr, len);
    else
        aw_update_chunk<PT, float, EMA>(k, (PT *)t.p + off, (const float *)t.g + off, t.m + off, t.v + off,
                                        EMA ? (PT *)t.ema + off : nullptr, len);
}

template <bool EMA>
__global__ __launch_bounds__(AW_THREADS) void aw_update_kernel(AwSlice s, AwHyper h) {
    float coef = 1.f;
    if (h.stats) {
        if (h.stats->skip) return;
        coef = h.stats->coef;
    }
    const double lr = h.lr_dev ? (double)*h.lr_dev : h.lr;
    const int n_chunks = s.cstart[s.nt];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int i = aw_part(s, c);
        const MopkOptimTensor &t = s.t[i];
        const int64_t off = (s.chunk0[i] + (c - s.cstart[i])) * AW_CHUNK;
        const int len = (int)min(AW_CHUNK, t.n - off);
        const unsigned int step = (unsigned int)*t.step + 1u;   // the count is advanced by a later launch
        const double bc1 = 1.0 - aw_powi(h.beta1, step), bc2 = 1.0 - aw_powi(h.beta2, step);
        AwConst k;
        k.coef = coef;
        k.decay = (float)(1.0 - lr * h.weight_decay);
        k.b1 = (float)h.beta1; k.omb1 = (float)(1.0 - h.beta1);
        k.b2 = (float)h.beta2; k.omb2 = (float)(1.0 - h.beta2);
        k.step_size = (float)(lr / bc1);
        k.sqrt_bc2 = (float)sqrt(bc2);
        k.eps = h.eps; k.ema_b = h.ema_b; k.ema_omb = h.ema_omb;
        if (t.p_dtype == MOPK_BF16) aw_update_g<unsigned short, EMA>(k, t, off, len);
        else aw_update_g<float, EMA>(k, t, off, len);
    }
}

// ---- 4. step counts: one thread per tensor part; only the part with a tensor's last chunk counts ----
__global__ __launch_bounds__(WAVE) void aw_advance_kernel(AwSlice s, const MopkAdamWStats *stats) {
    if (stats && stats->skip) return;
    const int i = threadIdx.x;
    if (i < s.nt && s.last[i]) *s.t[i].step += 1.f;
}

int aw_check(const MopkAdamWArgs *a, const MopkOptimTensor *t) {
    if (!a || (a->n_tensors > 0 && !t)) return MOPK_ERR_BAD_ARG;
    if (a->n_tensors < 0 || (a->phases & ~(MOPK_ADAMW_NORM | MOPK_ADAMW_UPDATE)) || a->phases == 0) return MOPK_ERR_BAD_ARG;
    for (int i = 0; i < a->n_tensors; ++i) {
        const MopkOptimTensor &x = t[i];
        if (x.n < 0) return MOPK_ERR_BAD_SHAPE;
        if ((x.p_dtype != MOPK_F32 && x.p_dtype != MOPK_BF16) || (x.g_dtype != MOPK_F32 && x.g_dtype != MOPK_BF16)) return MOPK_ERR_UNSUPPORTED;
        const bool upd = a->phases & MOPK_ADAMW_UPDATE;
        if (upd && (!x.step || misaligned(3, x.step))) return MOPK_ERR_BAD_ARG;
        if (x.n == 0) continue;                                 // an empty tensor has no chunk: only its count is touched
        if (any_null(x.g) || misaligned(x.g_dtype == MOPK_BF16 ? 1 : 3, x.g)) return MOPK_ERR_UNSUPPORTED;
        if (!upd) continue;
        if (any_null(x.p, x.m, x.v) || (a->use_ema && !x.ema)) return MOPK_ERR_BAD_ARG;
        if (misaligned(x.p_dtype == MOPK_BF16 ? 1 : 3, x.p, x.ema) || misaligned(3, x.m, x.v, x.step)) return MOPK_ERR_UNSUPPORTED;
    }
    return MOPK_OK;
}

// walk the slices of a tensor list in order: fn(slice) for each; the slice's partial0 counts the chunks before it
template <typename Fn>
int64_t aw_for_each_slice(const MopkOptimTensor *t, int n, Fn &&fn) {
    AwSlice s = {};
    int64_t done = 0;                                           // chunks in flushed slices
    int n_slices = 0;
    auto flush = [&]() {
        if (s.nt == 0) return;
        s.partial0 = done;
        fn(s);
        done += s.cstart[s.nt];
        ++n_slices;
        s = AwSlice{};
    };
    for (int i = 0; i < n; ++i) {
        int64_t rem = aw_chunks(t[i].n), c0 = 0;
        do {
            if (s.nt == AW_TCAP || s.cstart[s.nt] == AW_CCAP) flush();
            const int take = (int)(rem < (int64_t)(AW_CCAP - s.cstart[s.nt]) ? rem : (int64_t)(AW_CCAP - s.cstart[s.nt]));
            s.t[s.nt] = t[i];
            s.chunk0[s.nt] = c0;
            s.cstart[s.nt + 1] = s.cstart[s.nt] + take;
            s.last[s.nt] = rem == take;
            ++s.nt;
            c0 += take;
            rem -= take;
        } while (rem > 0);
    }
    flush();
    return n_slices;
}

int64_t aw_total_chunks(const MopkOptimTensor *t, int n) {
    int64_t c = 0;
    for (int i = 0; i < n; ++i) c += t[i].n > 0 ? aw_chunks(t[i].n) : 0;
    return c;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_adamw_supported(const MopkAdamWArgs *a, const MopkOptimTensor *t) { return aw_check(a, t) == MOPK_OK; }

size_t mopk_adamw_workspace_bytes(const MopkAdamWArgs *a, const MopkOptimTensor *t) {
    if (!a || a->n_tensors < 0 || (a->n_tensors > 0 && !t)) return 0;
    const int64_t c = aw_total_chunks(t, a->n_tensors);
    return (size_t)round_up((c > 0 ? c : 1) * (int64_t)sizeof(float), 256);
}

int mopk_adamw_launches(const MopkAdamWArgs *a, const MopkOptimTensor *t) {
    if (!a || a->n_tensors < 0 || (a->n_tensors > 0 && !t)) return 0;
    int64_t S1 = 0;                                             // slices that hold a chunk (a slice of empty tensors holds none)
    const int64_t S = aw_for_each_slice(t, a->n_tensors, [&](const AwSlice &s) { S1 += s.cstart[s.nt] > 0; });
    return (int)(((a->phases & MOPK_ADAMW_NORM) ? S1 + 1 : 0) + ((a->phases & MOPK_ADAMW_UPDATE) ? S1 + S : 0));
}

int mopk_adamw_step(const MopkAdamWArgs *a, const MopkOptimTensor *t, void *stream) {
    const int rc = aw_check(a, t);
    if (rc != MOPK_OK) return rc;
    const bool norm = a->phases & MOPK_ADAMW_NORM, update = a->phases & MOPK_ADAMW_UPDATE;
    const bool use_stats = norm || a->use_norm;
    if ((use_stats && !a->stats) || (norm && !a->workspace)) return MOPK_ERR_BAD_ARG;
    if (misaligned(3, a->stats, a->workspace, a->lr_dev)) return MOPK_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (norm) {
        float *partials = a->workspace;
        aw_for_each_slice(t, a->n_tensors, [&](const AwSlice &s) {
            if (s.cstart[s.nt] > 0) hipLaunchKernelGGL(aw_sumsq_kernel, dim3((unsigned)s.cstart[s.nt]), dim3(AW_THREADS), 0, st, s, partials);
        });
        hipLaunchKernelGGL(aw_finalise_kernel, dim3(1), dim3(AW_FIN_THREADS), 0, st, (const float *)partials,
                           aw_total_chunks(t, a->n_tensors), a->clip, a->max_norm, a->skip_nonfinite, a->stats);
    }
    if (update) {
        AwHyper h = {};
        h.lr = a->lr; h.beta1 = a->beta1; h.beta2 = a->beta2; h.weight_decay = a->weight_decay;
        h.eps = (float)a->eps; h.ema_b = (float)a->ema_decay; h.ema_omb = (float)(1.0 - a->ema_decay);
        h.lr_dev = a->lr_dev;
        h.stats = use_stats ? a->stats : nullptr;
        aw_for_each_slice(t, a->n_tensors, [&](const AwSlice &s) {
            const int nc = s.cstart[s.nt];
            if (nc == 0) return;
            const dim3 grid((unsigned)(nc < AW_GRID_CAP ? nc : AW_GRID_CAP));
            if (a->use_ema) hipLaunchKernelGGL(aw_update_kernel<true>, grid, dim3(AW_THREADS), 0, st, s, h);
            else hipLaunchKernelGGL(aw_update_kernel<false>, grid, dim3(AW_THREADS), 0, st, s, h);
        });
        aw_for_each_slice(t, a->n_tensors, [&](const AwSlice &s) {
            hipLaunchKernelGGL(aw_advance_kernel, dim3(1), dim3(WAVE), 0, st, s, (const MopkAdamWStats *)h.stats);
        });
    }
    return launch_status();
}

}  // extern "C"
