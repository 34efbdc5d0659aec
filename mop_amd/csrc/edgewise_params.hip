// Small-parameter prologue / epilogue of a share_qkv EdgewiseMSA layer (low-rank head): mopk_edgewise_params_{fwd,bwd}.
//
// The layer's small parameters (q_scale, k_scale, v_scale, the head's Wr / br / Wc / bc, chain_value_logit: a few thousand
// numbers) reach the core as one float32 buffer and their gradients leave it through one batch reduction plus a short chain
// rule.  Evaluated tensor by tensor that is some twenty 4 - 8 us launches per step; here it is one launch each way.  Both kernels
// restate the tensor-by-tensor arithmetic exactly: every intermediate a tensor expression would round to the parameters' dtype is
// rounded here (rnd<T>), every product is a separate float32 multiply (__fmul_rn: no contraction), and the batch reduction keeps
// the order of ew_reduce_parts_kernel (edgewise_generic.hip).
#include "common.h"

namespace mopk {

// the value a float has after a round trip through T (round-to-nearest-even)
template <typename T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<unsigned short>(float v) { return bf2f(f2bf(v)); }

struct EwParamDims {
    int B, V, H, dk, n_sqk, n_vs, n_w, n_b;
    float inv;      // (float)(1 / sqrt(dk))
};

// pack = sqk | vs0 | vsL | Wr | br | Wc | bc | logit, one thread per float
template <typename T>
__global__ void __launch_bounds__(256) ew_params_fwd_kernel(const T *q_scale, const T *k_scale, const T *v_scale, const T *Wr,
                                                           const T *br, const T *Wc, const T *bc, const T *logit, float *pack,
                                                           EwParamDims d) {
    int i = blockIdx.x * 256 + threadIdx.x;
    const int o = i;
    float v;
    if (i < d.n_sqk) {
        const float qk = rnd<T>(__fmul_rn(ld_as_f32(q_scale + i), ld_as_f32(k_scale + i)));
        v = rnd<T>(__fmul_rn(qk, d.inv));
    } else if ((i -= d.n_sqk) < d.n_vs) v = ld_as_f32(v_scale + i);
    else if ((i -= d.n_vs) < d.n_vs) v = ld_as_f32(v_scale + (size_t)(d.V - 1) * d.n_vs + i);
    else if ((i -= d.n_vs) < d.n_w) v = ld_as_f32(Wr + i);
    else if ((i -= d.n_w) < d.n_b) v = ld_as_f32(br + i);
    else if ((i -= d.n_b) < d.n_w) v = ld_as_f32(Wc + i);
    else if ((i -= d.n_w) < d.n_b) v = ld_as_f32(bc + i);
    else if ((i -= d.n_b) < 1) v = ld_as_f32(logit);
    else return;
    pack[o] = v;
}

struct EwParamGrads {       // outputs of the backward, each an array of its own
    void *q_scale, *k_scale, *v_scale, *Wr, *br, *Wc, *bc, *logit;
};

// blocks [0, n_red): 16 outputs x 16 batch slices each, slices combined in a fixed order (ew_reduce_parts_kernel's), and the thread
// that holds a finished sum applies the chain rule; block n_red: dlogit by the 256-thread tree; blocks behind it: the head's
// float32 gradients rounded to T and the zero rows 1 .. V-2 of dv_scale
template <typename T>
__global__ void __launch_bounds__(256) ew_params_bwd_kernel(const float *dsqk_p, const float *dvs0_p, const float *dvsL_p,
                                                           const float *dlg_p, const float *dWr, const float *dbr, const float *dWc,
                                                           const float *dbc, const T *q_scale, const T *k_scale, EwParamGrads g,
                                                           EwParamDims d, int n_red) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int n_lg = d.B * d.H;
    if ((int)blockIdx.x == n_red) {
        float s = 0.f;
        for (int i = tid; i < n_lg; i += 256) s += dlg_p[i];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
        if (tid == 0) st_from_f32((T *)g.logit, red[0]);
        return;
    }
    if ((int)blockIdx.x > n_red) {
        int i = ((int)blockIdx.x - n_red - 1) * 256 + tid;
        if (i < d.n_w) st_from_f32((T *)g.Wr + i, dWr[i]);
        else if ((i -= d.n_w) < d.n_b) st_from_f32((T *)g.br + i, dbr[i]);
        else if ((i -= d.n_b) < d.n_w) st_from_f32((T *)g.Wc + i, dWc[i]);
        else if ((i -= d.n_w) < d.n_b) st_from_f32((T *)g.bc + i, dbc[i]);
        else if ((i -= d.n_b) < (d.V - 2) * d.n_vs) st_from_f32((T *)g.v_scale + d.n_vs + i, 0.f);
        return;
    }
    const int o = blockIdx.x * 16 + (tid & 15), sl = tid >> 4, total = d.n_sqk + 2 * d.n_vs;
    float s = 0.f;
    if (o < total) {
        const float *src; int w, c;
        if (o < d.n_sqk) { src = dsqk_p; w = d.n_sqk; c = o; }
        else if (o < d.n_sqk + d.n_vs) { src = dvs0_p; w = d.n_vs; c = o - d.n_sqk; }
        else { src = dvsL_p; w = d.n_vs; c = o - d.n_sqk - d.n_vs; }
#pragma unroll 4
        for (int b = sl; b < d.B; b += 16) s += src[(size_t)b * w + c];
    }
    red[tid] = s;
    __syncthreads();
    if (sl == 0 && o < total) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k * 16 + tid];
        if (o < d.n_sqk) {          // sqk = (q_scale k_scale) inv: d(q_scale) = (dsqk inv) k_scale, d(k_scale) = (dsqk inv) q_scale
            const float g2 = rnd<T>(__fmul_rn(rnd<T>(t), d.inv));
            st_from_f32((T *)g.q_scale + o, __fmul_rn(g2, ld_as_f32(k_scale + o)));
            st_from_f32((T *)g.k_scale + o, __fmul_rn(g2, ld_as_f32(q_scale + o)));
        } else {                    // v_scale[0] / v_scale[V-1]; + 0: the sum with the other row's zeros (-0 becomes +0)
            const bool last = o >= d.n_sqk + d.n_vs;
            const int c = o - d.n_sqk - (last ? d.n_vs : 0);
            st_from_f32((T *)g.v_scale + (last ? (size_t)(d.V - 1) * d.n_vs : 0) + c, rnd<T>(t) + 0.f);
        }
    }
}

static EwParamDims ew_param_dims(const MopkEdgewiseParamArgs *p) {
    EwParamDims d;
    d.B = p->B; d.V = p->V; d.H = p->H; d.dk = p->dk;
    d.n_sqk = p->V * p->H * p->dk; d.n_vs = p->H * p->dk; d.n_w = 4 * p->r * p->C; d.n_b = 4 * p->r;
    d.inv = (float)(1.0 / sqrt((double)p->dk));
    return d;
}

template <typename T> static int ew_params_fwd_t(const MopkEdgewiseParamArgs *p, hipStream_t st) {
    const EwParamDims d = ew_param_dims(p);
    const int n_pack = d.n_sqk + 2 * d.n_vs + 2 * d.n_w + 2 * d.n_b + 1;
    hipLaunchKernelGGL((ew_params_fwd_kernel<T>), dim3((n_pack + 255) / 256), dim3(256), 0, st, (const T *)p->q_scale,
                       (const T *)p->k_scale, (const T *)p->v_scale, (const T *)p->Wr, (const T *)p->br, (const T *)p->Wc,
                       (const T *)p->bc, (const T *)p->chain_logit, p->pack, d);
    return launch_status();
}

template <typename T> static int ew_params_bwd_t(const MopkEdgewiseParamArgs *p, hipStream_t st) {
    const EwParamDims d = ew_param_dims(p);
    const int n_red = (d.n_sqk + 2 * d.n_vs + 15) / 16;
    const int n_cvt = (2 * d.n_w + 2 * d.n_b + (d.V - 2) * d.n_vs + 255) / 256;
    const EwParamGrads g{p->gq_scale, p->gk_scale, p->gv_scale, p->gWr, p->gbr, p->gWc, p->gbc, p->glogit};
    hipLaunchKernelGGL((ew_params_bwd_kernel<T>), dim3(n_red + 1 + n_cvt), dim3(256), 0, st, p->dsqk_part, p->dvs0_part,
                       p->dvsL_part, p->dlogit_part, p->dWr, p->dbr, p->dWc, p->dbc, (const T *)p->q_scale, (const T *)p->k_scale, g,
                       d, n_red);
    return launch_status();
}

static int ew_params_validate(const MopkEdgewiseParamArgs *p, bool bwd) {
    if (!p) return MOPK_ERR_BAD_ARG;
    if (p->B <= 0 || p->V < 2 || p->H <= 0 || p->dk <= 0 || p->r < 1 || p->C < 1) return MOPK_ERR_BAD_SHAPE;
    if (p->io_dtype != MOPK_F32 && p->io_dtype != MOPK_BF16) return MOPK_ERR_BAD_ARG;
    if (any_null(p->q_scale, p->k_scale)) return MOPK_ERR_BAD_ARG;
    if (!bwd && any_null(p->v_scale, p->Wr, p->br, p->Wc, p->bc, p->chain_logit, p->pack)) return MOPK_ERR_BAD_ARG;
    if (bwd && any_null(p->dsqk_part, p->dvs0_part, p->dvsL_part, p->dlogit_part, p->dWr, p->dbr, p->dWc, p->dbc, p->gq_scale, p->gk_scale, p->gv_scale, p->gWr, p->gbr, p->gWc, p->gbc, p->glogit))
        return MOPK_ERR_BAD_ARG;
    return MOPK_OK;
}

}  // namespace mopk

using namespace mopk;

extern "C" {

int mopk_edgewise_params_fwd(const MopkEdgewiseParamArgs *p, void *stream) {
    const int rc = ew_params_validate(p, false);
    if (rc) return rc;
    return p->io_dtype == MOPK_BF16 ? ew_params_fwd_t<unsigned short>(p, (hipStream_t)stream) : ew_params_fwd_t<float>(p, (hipStream_t)stream);
}

int mopk_edgewise_params_bwd(const MopkEdgewiseParamArgs *p, void *stream) {
    const int rc = ew_params_validate(p, true);
    if (rc) return rc;
    return p->io_dtype == MOPK_BF16 ? ew_params_bwd_t<unsigned short>(p, (hipStream_t)stream) : ew_params_bwd_t<float>(p, (hipStream_t)stream);
}

}  // extern "C"
