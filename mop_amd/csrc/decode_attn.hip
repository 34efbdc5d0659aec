// Attention of a few new queries against a key / value cache (incremental decoding of the WhisperMoP decoder; inference only).
//
// softmax(q k^T / sqrt(dk) [causal]) v for Tq <= 16 queries per (batch, head) row against the first L keys of a (B, cap, H, dk) cache.
// L is read from device memory (MopkDecodeAttnArgs.kv_len) when given, so one set of launch arguments serves every decoding step
// and a single-token step can be captured once in a HIP graph and replayed.
//
// Split-KV ("flash-decoding"): launch 1 has one workgroup per (b*H + h, chunk of CH keys); the chunk count is fixed from cap, not
// from L, and a workgroup whose chunk lies past L only writes an empty partial (m = -inf).  Per workgroup:
//   stage   K chunk -> LDS and V chunk -> registers with 16-byte loads (rows past L are never read), q -> LDS in fp32;
//   scores  thread (key j, query group) forms q_i . k_j from LDS in fp32 FMAs, masks, scales by 1/sqrt(dk);
//   softmax one wave per query: chunk max m, p = exp(s - m), l = sum p;
//   PV      V registers -> LDS (the K tile's space), thread (8-column slice, query, key group) accumulates p v over its keys,
//           the key groups are summed in a fixed order through LDS;
//   and writes (m, l) and acc (Tq x dk fp32) for its chunk to the workspace.
// Launch 2 (one workgroup per row) merges the partials in chunk order: out = sum_s e^(m_s - M) acc_s / sum_s e^(m_s - M) l_s.
// No atomics anywhere: results are bitwise reproducible.  All arithmetic is fp32 (bf16 operands are widened on load), so fp32 io
// is exact fp32 and bf16 io has fp32 accumulation; the only bf16 rounding is the final store of y.
// Algorithmic traffic: 2 * B * L * H * dk * sizeof(T) bytes of K and V (read once), plus q, y and the fp32 partials
// (B * H * chunks * Tq * (dk + 2) * 4 bytes, written and read back once).  Static LDS only (<= 59 KB): nothing to set before a
// graph capture.
//
// Row-indirect variant (mopk_decode_attn_rows_*, beam search): the same kernels with ROWS = true, where key / value j of query row b
// comes from cache row rows[b * rows_ld + j] (clamped into [0, B)) at position j.  Only the staging address changes: one int32 table
// read per key, the key's dk elements still one run of 16-byte vectors, and every later step is the same code, so an identity table
// gives bitwise the result of the plain kernels.
//
// Ragged variant (mopk_decode_attn_ragged_*, prompts of different lengths left-padded in one cache): START = true adds a per-row
// first key, s = kv_start[b] clamped into [0, L]; query row b sees keys s <= j < its limit.  A chunk that lies wholly below s writes
// the empty partial (as a chunk past L does), key rows below s are neither loaded nor scored, and a query with no open key ends as
// y = 0 in the merge.  With kv_start = 0 every step is the plain code, so the result is bitwise that of the plain kernels; the
// START = false instantiations compile to the same instructions as before the flag existed (kv_start is an unused argument there).
//
// Per-row key counts (mopk_decode_attn_lens_*, cross-attention over right-padded audio of unequal length): LENS = true reads the
// row's own L = kv_lens[b] (clamped into [0, Nk]) where the plain kernel takes one L for the batch; everything after that is the
// plain code, so a chunk past the row's L writes the empty partial and leaves, key rows >= L are never read, and kv_lens = Nk is
// bitwise the plain result.  The per-row pointer travels in the kv_start argument (START and LENS are never set together).  These
// instantiations are built in a unit of their own (-DMOPK_DECODE_LENS, mop_amd/build.py), which leaves the code of the others as
// it was.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_MAX_TQ = 16;

template <typename T, int DK, int TQB>
struct DaCfg {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int CH = (32768 / (DK * ES)) < 128 ? (32768 / (DK * ES)) : 128;   // keys per chunk (K/V tile <= 32 KB)
    static constexpr int R16 = DK * ES / 16;                    // 16-byte vectors per key row
    static constexpr int PITCH = R16 + 1;                       // LDS row pitch in 16-byte units (odd: conflict-free row reads)
    static constexpr int VPT = CH * R16 / DA_THREADS;           // staged vectors per thread and tensor
    static constexpr int EPV = 16 / ES;                         // elements per 16-byte vector
    static constexpr int NG = DA_THREADS / CH;                  // query groups of the score phase
    static constexpr int QPT = (TQB + NG - 1) / NG;             // queries per thread in the score phase
    static constexpr int S = DK / 8;                            // 8-column slices of the PV phase
    static constexpr int KG = DA_THREADS / S / TQB;             // key groups of the PV phase
    static_assert(CH * R16 % DA_THREADS == 0, "staging must divide evenly");
    static_assert(KG >= 1, "PV phase needs one key group");
};

// launch 1: one (row, chunk) partial; ROWS: keys / values through the row table; START: keys from kv_start[b] on; LENS: keys up to
// kv_start[b] (the row's key count in the same argument)
template <typename T, int DK, int TQB, bool ROWS, bool START, bool LENS = false>
__global__ __launch_bounds__(DA_THREADS) void da_split_kernel(MopkDecodeAttnArgs a, int nsplit, const int32_t *rows, int64_t rows_ld,
                                                              const int32_t *kv_start) {
    using C = DaCfg<T, DK, TQB>;
    __shared__ uint4 tile[C::CH * C::PITCH];
    __shared__ float4 qs4[TQB * DK / 4];
    __shared__ float sc[TQB * C::CH];
    __shared__ float4 red4[C::KG * TQB * DK / 4];
    float *qs = (float *)qs4, *red = (float *)red4;

    const int tid = threadIdx.x;
    const int bh = blockIdx.x, split = blockIdx.y;
    const int b = bh / a.H, h = bh - b * a.H;
    const int tq = a.Tq;
    int L = a.kv_len ? *a.kv_len : a.Nk;
    L = L < 0 ? 0 : (L > a.cap ? a.cap : L);
    if constexpr (LENS) {
        const int n = kv_start[b];                                  // uniform: one scalar load per workgroup
        L = n < 0 ? 0 : (n > L ? L : n);
    }
    const int c0 = split * C::CH;
    const size_t part = (size_t)bh * nsplit + split;
    float *ml = (float *)a.workspace + part * tq * 2;
    float *acc_out = (float *)a.workspace + (size_t)a.B * a.H * nsplit * tq * 2 + part * tq * DK;
    const int nv = L - c0 < C::CH ? L - c0 : C::CH;             // keys of this chunk any query can see (causal limits are <= L)
    int s0 = 0;                                                 // first key any query of this row can see
    if constexpr (START) {
        s0 = kv_start[b];
        s0 = s0 < 0 ? 0 : (s0 > L ? L : s0);
    }
    if (nv <= 0 || (START && c0 + C::CH <= s0)) {
        if (tid < tq) { ml[2 * tid] = -INFINITY; ml[2 * tid + 1] = 0.f; }
        return;
    }

    // ---- stage: K, V chunk rows [c0, c0 + nv) with 16-byte loads (zeros past nv), q in fp32
    const char *kb = (const char *)a.k.ptr + ((int64_t)b * a.k.sb + (int64_t)h * a.k.sh) * C::ES;
    const char *vb = (const char *)a.v.ptr + ((int64_t)b * a.v.sb + (int64_t)h * a.v.sh) * C::ES;
    uint4 kreg[C::VPT], vreg[C::VPT];
#pragma unroll
    for (int u = 0; u < C::VPT; ++u) {
        const int idx = tid + DA_THREADS * u, row = idx / C::R16, col = idx - row * C::R16;
        kreg[u] = vreg[u] = make_uint4(0u, 0u, 0u, 0u);
        if (row < nv && (!START || c0 + row >= s0)) {
            int64_t kro = 0, vro = 0;                               // element offset of the source row from row b
            if constexpr (ROWS) {
                int r = rows[(int64_t)b * rows_ld + c0 + row];
                r = r < 0 ? 0 : (r >= a.B ? a.B - 1 : r);
                kro = (int64_t)(r - b) * a.k.sb;
                vro = (int64_t)(r - b) * a.v.sb;
            }
            kreg[u] = *(const uint4 *)(kb + ((int64_t)(c0 + row) * a.k.sn + kro) * C::ES + col * 16);
            vreg[u] = *(const uint4 *)(vb + ((int64_t)(c0 + row) * a.v.sn + vro) * C::ES + col * 16);
        }
    }
    const T *qb = (const T *)a.q.ptr + (int64_t)b * a.q.sb + (int64_t)h * a.q.sh;
    for (int idx = tid; idx < TQB * DK; idx += DA_THREADS) {
        const int i = idx / DK, d = idx - i * DK;
        qs[idx] = i < tq ? ld_as_f32<T>(qb + (int64_t)i * a.q.sn + d) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < C::VPT; ++u) {
        const int idx = tid + DA_THREADS * u, row = idx / C::R16, col = idx - row * C::R16;
        tile[row * C::PITCH + col] = kreg[u];
    }
    __syncthreads();

    // ---- scores: thread (key j, query group g) for queries g, g + NG, ...
    const float scale = 1.0f / sqrtf((float)DK);
    {
        const int j = tid % C::CH, g = tid / C::CH;
        float s[C::QPT];
#pragma unroll
        for (int qi = 0; qi < C::QPT; ++qi) s[qi] = 0.f;
        if (j < nv && (!START || c0 + j >= s0)) {
#pragma unroll 4
            for (int c = 0; c < C::R16; ++c) {
                float kf[C::EPV];
                row_unpack(tile[j * C::PITCH + c], kf, T());
#pragma unroll
                for (int qi = 0; qi < C::QPT; ++qi) {
                    const int i = g + qi * C::NG;
                    if (i < TQB && i < tq) {
                        const float *qp = qs + i * DK + c * C::EPV;
#pragma unroll
                        for (int e = 0; e < C::EPV; ++e) s[qi] = fmaf(qp[e], kf[e], s[qi]);
                    }
                }
            }
        }
#pragma unroll
        for (int qi = 0; qi < C::QPT; ++qi) {
            const int i = g + qi * C::NG;
            if (i < TQB) {
                const int lim = a.causal ? L - tq + i + 1 : L;          // bottom-right aligned causal limit (global key index)
                sc[i * C::CH + j] = (i < tq && j < nv && c0 + j < lim && (!START || c0 + j >= s0)) ? s[qi] * scale : -INFINITY;
            }
        }
    }
    __syncthreads();

    // ---- V registers -> the K tile's space (every thread is past its last K read); chunk softmax, one wave per query
#pragma unroll
    for (int u = 0; u < C::VPT; ++u) {
        const int idx = tid + DA_THREADS * u, row = idx / C::R16, col = idx - row * C::R16;
        tile[row * C::PITCH + col] = vreg[u];
    }
    {
        const int lane = tid & 63, w = tid >> 6;
        for (int i = w; i < tq; i += DA_THREADS / 64) {
            float m = -INFINITY;
            for (int j = lane; j < C::CH; j += 64) m = fmaxf(m, sc[i * C::CH + j]);
            m = wave_max(m);
            float l = 0.f;
            for (int j = lane; j < C::CH; j += 64) {
                const float p = m == -INFINITY ? 0.f : expf(sc[i * C::CH + j] - m);
                sc[i * C::CH + j] = p;
                l += p;
            }
            l = wave_sum(l);
            if (lane == 0) { ml[2 * i] = m; ml[2 * i + 1] = l; }
        }
    }
    __syncthreads();

    // ---- PV: thread (slice s, query i, key group kg) over keys kg, kg + KG, ... < nv
    {
        const int s = tid % C::S, r = tid / C::S, i = r % TQB, kg = r / TQB;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        if (i < tq) {
            for (int j = kg; j < nv; j += C::KG) {
                const float p = sc[i * C::CH + j];
                const uint4 *vp = tile + j * C::PITCH + s * (8 / C::EPV);
                float vf[8];
                if constexpr (C::EPV == 8) {
                    row_unpack(vp[0], vf, T());
                } else {
                    float lo[4], hi[4];
                    row_unpack(vp[0], lo, T());
                    row_unpack(vp[1], hi, T());
#pragma unroll
                    for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = hi[e]; }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, vf[e], acc[e]);
            }
        }
        float4 *rp = red4 + ((kg * TQB + i) * DK + s * 8) / 4;
        rp[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        rp[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    __syncthreads();
    for (int idx = tid; idx < tq * DK; idx += DA_THREADS) {
        const int i = idx / DK, d = idx - i * DK;
        float t = 0.f;
#pragma unroll
        for (int kg = 0; kg < C::KG; ++kg) t += red[(kg * TQB + i) * DK + d];
        acc_out[idx] = t;
    }
}

// launch 2: merge the chunk partials of one (b, h) row in chunk order
template <typename T>
__global__ __launch_bounds__(DA_THREADS) void da_merge_kernel(MopkDecodeAttnArgs a, int nsplit) {
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
    const int tq = a.Tq, dk = a.dk;
    const float *ml = (const float *)a.workspace + (size_t)bh * nsplit * tq * 2;
    const float *acc = (const float *)a.workspace + (size_t)a.B * a.H * nsplit * tq * 2 + (size_t)bh * nsplit * tq * dk;
    T *yb = (T *)a.y.ptr + (int64_t)b * a.y.sb + (int64_t)h * a.y.sh;
    for (int idx = threadIdx.x; idx < tq * dk; idx += DA_THREADS) {
        const int i = idx / dk, d = idx - i * dk;
        float M = -INFINITY;
        for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ml[(s * tq + i) * 2]);
        float l = 0.f, o = 0.f;
        if (M != -INFINITY) {
            for (int s = 0; s < nsplit; ++s) {
                const float ms = ml[(s * tq + i) * 2];
                if (ms == -INFINITY) continue;
                const float f = expf(ms - M);
                l = fmaf(f, ml[(s * tq + i) * 2 + 1], l);
                o = fmaf(f, acc[((size_t)s * tq + i) * dk + d], o);
            }
        }
        st_from_f32<T>(yb + (int64_t)i * a.y.sn + d, l > 0.f ? o / l : 0.f);
    }
}

int da_esize(const MopkDecodeAttnArgs *a) { return a->io_dtype == MOPK_BF16 ? 2 : 4; }

int da_chunk(const MopkDecodeAttnArgs *a) {
    const int c = 32768 / (a->dk * da_esize(a));
    return c < 128 ? c : 128;
}

int da_nsplit(const MopkDecodeAttnArgs *a) { return (a->cap + da_chunk(a) - 1) / da_chunk(a); }

int da_check(const MopkDecodeAttnArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->B <= 0 || a->H <= 0 || a->Tq <= 0 || a->dk <= 0 || a->cap <= 0) return MOPK_ERR_BAD_SHAPE;
    if (a->io_dtype != MOPK_F32 && a->io_dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->causal != 0 && a->causal != 1) return MOPK_ERR_BAD_ARG;
    if (a->Tq > DA_MAX_TQ) return MOPK_ERR_UNSUPPORTED;
    if (a->dk != 32 && a->dk != 64 && a->dk != 128) return MOPK_ERR_UNSUPPORTED;
    if (a->Nk < 0 || a->Nk > a->cap || (!a->kv_len && a->Nk == 0)) return MOPK_ERR_BAD_SHAPE;
    if (da_nsplit(a) > 65535 || (int64_t)a->B * a->H > 0x7fffffff) return MOPK_ERR_UNSUPPORTED;
    const int vec = 16 / da_esize(a);                             // elements per 16-byte vector: K / V row strides
    for (const MopkView4 *t : {&a->k, &a->v})
        if (t->sb % vec || t->sh % vec || t->sn % vec || misaligned(15, t->ptr)) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(15, a->workspace) || misaligned(3, a->kv_len)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <typename T, int DK, int TQB, bool ROWS>
void da_launch_split(const dim3 &grid, const dim3 &block, hipStream_t st, const MopkDecodeAttnArgs *a, int ns, const int32_t *rows,
                     int64_t rows_ld, const int32_t *kv_start) {
    if (kv_start) hipLaunchKernelGGL((da_split_kernel<T, DK, TQB, ROWS, true>), grid, block, 0, st, *a, ns, rows, rows_ld, kv_start);
    else hipLaunchKernelGGL((da_split_kernel<T, DK, TQB, ROWS, false>), grid, block, 0, st, *a, ns, rows, rows_ld, kv_start);
}

template <typename T, int DK, bool ROWS>
void da_launch_dk(const MopkDecodeAttnArgs *a, const int32_t *rows, int64_t rows_ld, const int32_t *kv_start, hipStream_t st) {
    const int ns = da_nsplit(a);
    const dim3 grid((unsigned)(a->B * a->H), (unsigned)ns), block(DA_THREADS);
    if (a->Tq <= 1) da_launch_split<T, DK, 1, ROWS>(grid, block, st, a, ns, rows, rows_ld, kv_start);
    else if (a->Tq <= 4) da_launch_split<T, DK, 4, ROWS>(grid, block, st, a, ns, rows, rows_ld, kv_start);
    else da_launch_split<T, DK, 16, ROWS>(grid, block, st, a, ns, rows, rows_ld, kv_start);
    hipLaunchKernelGGL(da_merge_kernel<T>, dim3((unsigned)(a->B * a->H)), block, 0, st, *a, ns);
}

template <typename T, bool ROWS>
void da_launch(const MopkDecodeAttnArgs *a, const int32_t *rows, int64_t rows_ld, hipStream_t st, const int32_t *kv_start = nullptr) {
    if (a->dk == 32) da_launch_dk<T, 32, ROWS>(a, rows, rows_ld, kv_start, st);
    else if (a->dk == 64) da_launch_dk<T, 64, ROWS>(a, rows, rows_ld, kv_start, st);
    else da_launch_dk<T, 128, ROWS>(a, rows, rows_ld, kv_start, st);
}

int da_rows_check(const MopkDecodeAttnRowsArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    const int rc = da_check(&a->base);
    if (rc != MOPK_OK) return rc;
    if (a->rows_ld < a->base.cap) return MOPK_ERR_BAD_SHAPE;
    if (misaligned(3, a->rows)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

int da_ragged_check(const MopkDecodeAttnRaggedArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    const int rc = da_check(&a->base);
    if (rc != MOPK_OK) return rc;
    if (!a->kv_start) return MOPK_ERR_BAD_ARG;
    if (misaligned(3, a->kv_start)) return MOPK_ERR_UNSUPPORTED;
    if (a->rows) {
        if (a->rows_ld < a->base.cap) return MOPK_ERR_BAD_SHAPE;
        if (misaligned(3, a->rows)) return MOPK_ERR_UNSUPPORTED;
    }
    return MOPK_OK;
}

#ifdef MOPK_DECODE_LENS
int da_lens_check(const MopkDecodeAttnLensArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    const int rc = da_check(&a->base);
    if (rc != MOPK_OK) return rc;
    if (a->base.kv_len || a->base.causal || !a->kv_lens) return MOPK_ERR_BAD_ARG;
    if (misaligned(3, a->kv_lens)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

template <typename T, int DK>
void da_launch_lens_dk(const MopkDecodeAttnArgs *a, const int32_t *kv_lens, hipStream_t st) {
    const int ns = da_nsplit(a);
    const dim3 grid((unsigned)(a->B * a->H), (unsigned)ns), block(DA_THREADS);
    if (a->Tq <= 1) hipLaunchKernelGGL((da_split_kernel<T, DK, 1, false, false, true>), grid, block, 0, st, *a, ns, (const int32_t *)nullptr, (int64_t)0, kv_lens);
    else if (a->Tq <= 4) hipLaunchKernelGGL((da_split_kernel<T, DK, 4, false, false, true>), grid, block, 0, st, *a, ns, (const int32_t *)nullptr, (int64_t)0, kv_lens);
    else hipLaunchKernelGGL((da_split_kernel<T, DK, 16, false, false, true>), grid, block, 0, st, *a, ns, (const int32_t *)nullptr, (int64_t)0, kv_lens);
    hipLaunchKernelGGL(da_merge_kernel<T>, dim3((unsigned)(a->B * a->H)), block, 0, st, *a, ns);
}

template <typename T>
void da_launch_lens(const MopkDecodeAttnArgs *a, const int32_t *kv_lens, hipStream_t st) {
    if (a->dk == 32) da_launch_lens_dk<T, 32>(a, kv_lens, st);
    else if (a->dk == 64) da_launch_lens_dk<T, 64>(a, kv_lens, st);
    else da_launch_lens_dk<T, 128>(a, kv_lens, st);
}
#endif

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

#ifndef MOPK_DECODE_LENS
int mopk_decode_attn_supported(const MopkDecodeAttnArgs *a) { return da_check(a) == MOPK_OK; }

size_t mopk_decode_attn_workspace_bytes(const MopkDecodeAttnArgs *a) {
    if (da_check(a) != MOPK_OK) return 0;
    return (size_t)a->B * a->H * da_nsplit(a) * a->Tq * (a->dk + 2) * sizeof(float);
}

int mopk_decode_attn_fwd(const MopkDecodeAttnArgs *a, void *stream) {
    const int rc = da_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->q.ptr, a->k.ptr, a->v.ptr, a->y.ptr, a->workspace)) return MOPK_ERR_BAD_ARG;
    if (a->io_dtype == MOPK_BF16) da_launch<unsigned short, false>(a, nullptr, 0, (hipStream_t)stream);
    else da_launch<float, false>(a, nullptr, 0, (hipStream_t)stream);
    return launch_status();
}

int mopk_decode_attn_rows_supported(const MopkDecodeAttnRowsArgs *a) { return da_rows_check(a) == MOPK_OK; }

size_t mopk_decode_attn_rows_workspace_bytes(const MopkDecodeAttnRowsArgs *a) {
    return da_rows_check(a) == MOPK_OK ? mopk_decode_attn_workspace_bytes(&a->base) : 0;
}

int mopk_decode_attn_rows_fwd(const MopkDecodeAttnRowsArgs *a, void *stream) {
    const int rc = da_rows_check(a);
    if (rc != MOPK_OK) return rc;
    const MopkDecodeAttnArgs *b = &a->base;
    if (any_null(b->q.ptr, b->k.ptr, b->v.ptr, b->y.ptr, b->workspace, a->rows)) return MOPK_ERR_BAD_ARG;
    if (b->io_dtype == MOPK_BF16) da_launch<unsigned short, true>(b, a->rows, a->rows_ld, (hipStream_t)stream);
    else da_launch<float, true>(b, a->rows, a->rows_ld, (hipStream_t)stream);
    return launch_status();
}

int mopk_decode_attn_ragged_supported(const MopkDecodeAttnRaggedArgs *a) { return da_ragged_check(a) == MOPK_OK; }

size_t mopk_decode_attn_ragged_workspace_bytes(const MopkDecodeAttnRaggedArgs *a) {
    return da_ragged_check(a) == MOPK_OK ? mopk_decode_attn_workspace_bytes(&a->base) : 0;
}

int mopk_decode_attn_ragged_fwd(const MopkDecodeAttnRaggedArgs *a, void *stream) {
    const int rc = da_ragged_check(a);
    if (rc != MOPK_OK) return rc;
    const MopkDecodeAttnArgs *b = &a->base;
    if (any_null(b->q.ptr, b->k.ptr, b->v.ptr, b->y.ptr, b->workspace)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->rows) {
        if (b->io_dtype == MOPK_BF16) da_launch<unsigned short, true>(b, a->rows, a->rows_ld, st, a->kv_start);
        else da_launch<float, true>(b, a->rows, a->rows_ld, st, a->kv_start);
    } else {
        if (b->io_dtype == MOPK_BF16) da_launch<unsigned short, false>(b, nullptr, 0, st, a->kv_start);
        else da_launch<float, false>(b, nullptr, 0, st, a->kv_start);
    }
    return launch_status();
}

#else  // MOPK_DECODE_LENS: the unit of the per-row key counts
int mopk_decode_attn_lens_supported(const MopkDecodeAttnLensArgs *a) { return da_lens_check(a) == MOPK_OK; }

size_t mopk_decode_attn_lens_workspace_bytes(const MopkDecodeAttnLensArgs *a) {
    if (da_lens_check(a) != MOPK_OK) return 0;
    const MopkDecodeAttnArgs *b = &a->base;
    return (size_t)b->B * b->H * da_nsplit(b) * b->Tq * (b->dk + 2) * sizeof(float);      // = mopk_decode_attn_workspace_bytes(base)
}

int mopk_decode_attn_lens_fwd(const MopkDecodeAttnLensArgs *a, void *stream) {
    const int rc = da_lens_check(a);
    if (rc != MOPK_OK) return rc;
    const MopkDecodeAttnArgs *b = &a->base;
    if (any_null(b->q.ptr, b->k.ptr, b->v.ptr, b->y.ptr, b->workspace)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (b->io_dtype == MOPK_BF16) da_launch_lens<unsigned short>(b, a->kv_lens, st);
    else da_launch_lens<float>(b, a->kv_lens, st);
    return launch_status();
}
#endif

}  // extern "C"
