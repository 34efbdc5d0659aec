// Cross-entropy of rows of logits against int64 targets (ops.cross_entropy, ops.linear_cross_entropy, the models' loss()):
// forward, reduce and backward.  include/mopk.h states the three.  One workgroup of 1024 threads per row, static LDS, no float
// atomics, no workspace, no host synchronisation: every quantity a later launch needs (lse, the row losses, 1 / n_valid) is read
// from device memory, so a call can be captured in a HIP graph, and results are bitwise reproducible.
//
// Forward: one pass streams the row in 16-byte loads; the elements before the row's first 16-byte boundary and behind its last whole
// vector are read one by one (a row may start at any element).  A thread merges what it reads into its (max, sum-exp) pair; the
// pairs are merged in the fixed order of row_helpers.h (wave shuffles, then the waves in order).  Reduce: one workgroup sums the row
// losses of the rows that count, in double, thread-strided, then by the same two-step order.  Backward: elementwise from the saved
// lse, the same head / vector / tail split; a thread stores only where it loaded, and loads before it stores, so the gradient may
// be written over the logits.
#include "common.h"
#include "row_helpers.h"

namespace mopk {
namespace {

constexpr int CE_THREADS = 1024;
constexpr int CE_WAVES = CE_THREADS / WAVE;
constexpr int CE_BWD_BATCH = 4;                                 // vectors a backward thread loads before it stores the first

// a row whose target is ignore_index or no class at all adds nothing: loss 0, gradient 0, not counted
__device__ __forceinline__ bool ce_ignored(int64_t t, const MopkCrossEntropyArgs &a) {
    return t == a.ignore_index || t < 0 || t >= (int64_t)a.V;
}

// this thread's share of row x[0, V): the walk of token_logprob.hip's tl_scan
template <typename T>
__device__ __forceinline__ void ce_scan(const T *x, int V, float &m, float &l) {
    constexpr int EPV = RowSpan<T>::EPV;
    const int tid = threadIdx.x;
    const RowSpan<T> sp(x, V);
    const int head = sp.head, tail0 = sp.tail0;                 // head + (V - tail0) < 2 * EPV scalar elements
    const uint4 *xv = (const uint4 *)(x + head);
#pragma unroll 4
    for (int u = tid; u < sp.nvec; u += CE_THREADS) {
        float f[EPV];
        row_unpack(xv[u], f, T());
#pragma unroll
        for (int e = 0; e < EPV; ++e) row_lse_add(m, l, f[e]);
    }
    if (tid < head + (V - tail0)) {
        const int e = tid < head ? tid : tail0 + (tid - head);
        row_lse_add(m, l, ld_as_f32<T>(x + e));
    }
}

template <typename T>
__global__ __launch_bounds__(CE_THREADS) void ce_fwd_kernel(MopkCrossEntropyArgs a) {
    __shared__ RowLseLds<CE_WAVES> s;
    const int r = blockIdx.x, V = a.V;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    float m = -INFINITY, l = 0.f;
    ce_scan<T>(x, V, m, l);
    row_wave_lse(m, l);
    s.put(m, l);
    __syncthreads();
    s.get(m, l);
    if (threadIdx.x == 0) {
        const int64_t row = (int64_t)a.row0 + r;
        const int64_t t = a.targets[row];
        const float lse = m + logf(l);
        a.lse[row] = lse;
        a.row_loss[row] = ce_ignored(t, a) ? 0.f : lse - ld_as_f32<T>(x + t);        // t in [0, V): no read leaves the row
    }
}

// out[0 .. 3] = sum, n_valid, sum / n_valid, 1 / n_valid over rows [0, n_rows)
__global__ __launch_bounds__(CE_THREADS) void ce_reduce_kernel(MopkCrossEntropyArgs a) {
    __shared__ double ws[CE_WAVES];
    __shared__ int wn[CE_WAVES];
    const int tid = threadIdx.x;
    double s = 0.0;
    int n = 0;
    for (int i = tid; i < a.n_rows; i += CE_THREADS)
        if (!ce_ignored(a.targets[i], a)) { s += (double)a.row_loss[i]; ++n; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); n += __shfl_xor(n, o, 64); }
    if ((tid & (WAVE - 1)) == 0) { ws[tid / WAVE] = s; wn[tid / WAVE] = n; }
    __syncthreads();
    if (tid == 0) {
        s = ws[0];
        n = wn[0];
        for (int w = 1; w < CE_WAVES; ++w) { s += ws[w]; n += wn[w]; }
        a.out[0] = (float)s;
        a.out[1] = (float)n;
        a.out[2] = (float)(s / (double)n);                      // no row counts: 0 / 0 = NaN, as torch's mean
        a.out[3] = 1.f / (float)n;
    }
}

__device__ __forceinline__ uint4 ce_pack(const float (&f)[8], unsigned short) {
    return make_uint4(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7]));
}
__device__ __forceinline__ uint4 ce_pack(const float (&f)[4], float) {
    return make_uint4(__builtin_bit_cast(unsigned int, f[0]), __builtin_bit_cast(unsigned int, f[1]),
                      __builtin_bit_cast(unsigned int, f[2]), __builtin_bit_cast(unsigned int, f[3]));
}

// g (softmax(x)_j - [j == t]) of element j
__device__ __forceinline__ float ce_grad(float x, float lse, float g, int j, int t) { return g * (expf(x - lse) - (j == t ? 1.f : 0.f)); }

template <typename T>
__device__ __forceinline__ uint4 ce_grad_vec(const uint4 &v, float lse, float g, int j0, int t) {
    constexpr int EPV = RowSpan<T>::EPV;
    float f[EPV];
    row_unpack(v, f, T());
#pragma unroll
    for (int e = 0; e < EPV; ++e) f[e] = ce_grad(f[e], lse, g, j0 + e, t);
    return ce_pack(f, T());
}

template <typename T>
__global__ __launch_bounds__(CE_THREADS) void ce_bwd_kernel(MopkCrossEntropyArgs a) {
    constexpr int EPV = RowSpan<T>::EPV;
    const int r = blockIdx.x, V = a.V, tid = threadIdx.x;
    const int64_t row = (int64_t)a.row0 + r;
    const T *x = (const T *)a.logits + (int64_t)r * a.logits_ld;
    T *d = (T *)a.dlogits + (int64_t)r * a.dlogits_ld;
    const RowSpan<T> sp(x, V);                                  // d's rows lie as x's do relative to 16 bytes (ce_bwd_check)
    const int head = sp.head, tail0 = sp.tail0, nvec = sp.nvec;
    const uint4 *xv = (const uint4 *)(x + head);
    uint4 *dv = (uint4 *)(d + head);
    const int e1 = tid < head ? tid : tail0 + (tid - head);     // this thread's scalar element, if tid < head + (V - tail0)
    const int64_t t64 = a.targets[row];
    if (ce_ignored(t64, a)) {                                   // the whole workgroup: exact zeros, no product with grad or scale
        for (int u = tid; u < nvec; u += CE_THREADS) dv[u] = make_uint4(0u, 0u, 0u, 0u);
        if (tid < head + (V - tail0)) st_from_f32<T>(d + e1, 0.f);
        return;
    }
    const int t = (int)t64;
    const float lse = a.lse[row];
    float g = a.grad[row * a.grad_stride];
    if (a.scale) g *= *a.scale;
    int u = tid;
    for (; u + (CE_BWD_BATCH - 1) * CE_THREADS < nvec; u += CE_BWD_BATCH * CE_THREADS) {
        uint4 v[CE_BWD_BATCH];
#pragma unroll
        for (int k = 0; k < CE_BWD_BATCH; ++k) v[k] = xv[u + k * CE_THREADS];
#pragma unroll
        for (int k = 0; k < CE_BWD_BATCH; ++k) dv[u + k * CE_THREADS] = ce_grad_vec<T>(v[k], lse, g, head + (u + k * CE_THREADS) * EPV, t);
    }
    for (; u < nvec; u += CE_THREADS) dv[u] = ce_grad_vec<T>(xv[u], lse, g, head + u * EPV, t);
    if (tid < head + (V - tail0)) st_from_f32<T>(d + e1, ce_grad(ld_as_f32<T>(x + e1), lse, g, e1, t));
}

int ce_check(const MopkCrossEntropyArgs *a) {
    if (!a) return MOPK_ERR_BAD_ARG;
    if (a->R <= 0 || a->V < 2) return MOPK_ERR_BAD_SHAPE;
    if (a->dtype != MOPK_F32 && a->dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (a->logits_ld < a->V || (a->dlogits && a->dlogits_ld < a->V)) return MOPK_ERR_BAD_ARG;
    if (a->row0 < 0 || (int64_t)a->row0 + a->R > (int64_t)a->n_rows || a->grad_stride < 0 || a->reserved != 0) return MOPK_ERR_BAD_ARG;
    if (misaligned(a->dtype == MOPK_BF16 ? 1 : 3, a->logits, a->dlogits)) return MOPK_ERR_UNSUPPORTED;
    if (misaligned(7, a->targets) || misaligned(3, a->lse, a->row_loss, a->out, a->grad, a->scale)) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

// the backward's 16-byte stores follow the loads' split: every row of dlogits must sit as its row of logits does
int ce_bwd_check(const MopkCrossEntropyArgs *a) {
    const int64_t epv = a->dtype == MOPK_BF16 ? 8 : 4;
    if ((((uintptr_t)a->logits ^ (uintptr_t)a->dlogits) & 15) != 0) return MOPK_ERR_UNSUPPORTED;
    if (a->R > 1 && (a->logits_ld - a->dlogits_ld) % epv != 0) return MOPK_ERR_UNSUPPORTED;
    return MOPK_OK;
}

}  // namespace
}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_cross_entropy_supported(const MopkCrossEntropyArgs *a) { return ce_check(a) == MOPK_OK; }

int mopk_cross_entropy_fwd(const MopkCrossEntropyArgs *a, void *stream) {
    const int rc = ce_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->targets, a->lse, a->row_loss)) return MOPK_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((ce_fwd_kernel<unsigned short>), dim3((unsigned)a->R), dim3(CE_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((ce_fwd_kernel<float>), dim3((unsigned)a->R), dim3(CE_THREADS), 0, st, *a);
    if (a->out) hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(CE_THREADS), 0, st, *a);
    return launch_status();
}

int mopk_cross_entropy_bwd(const MopkCrossEntropyArgs *a, void *stream) {
    int rc = ce_check(a);
    if (rc != MOPK_OK) return rc;
    if (any_null(a->logits, a->targets, a->lse, a->dlogits, a->grad)) return MOPK_ERR_BAD_ARG;
    if ((rc = ce_bwd_check(a)) != MOPK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == MOPK_BF16) hipLaunchKernelGGL((ce_bwd_kernel<unsigned short>), dim3((unsigned)a->R), dim3(CE_THREADS), 0, st, *a);
    else hipLaunchKernelGGL((ce_bwd_kernel<float>), dim3((unsigned)a->R), dim3(CE_THREADS), 0, st, *a);
    return launch_status();
}

}  // extern "C"
