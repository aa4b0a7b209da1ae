// Multi-coil (SENSE) data consistency for gfx950, float and double: the pointwise kernels around the coil transforms and the batched
// conjugate-gradient updates of the x-step  G x^ = A^H y + La2 (z - w),  G p = sum_c conj(S_c) ifft2(m fft2(S_c p)) + La2 p.
//
// One application of G is three launches of the any-size kernels (kernels_anysize.hip: coil-expanding rows, masked columns over B * C
// pseudo-slices, coil-combining rows, which also leave the row partials of Re<p, Gp>).  The kernels here are the rest of a CG iteration:
//   k_cg_init  r0 = aty + La2 v - G v, p0 = r0, partials of <r0, r0> and of ||aty + La2 v||^2
//   k_cg_xr    alpha = <r, r> / Re<p, Gp>;  x^ += alpha p;  r -= alpha Gp;  partials of the new <r, r>;  last iteration: x = |Re x^|
//              (complex images, pnp_set_image: x = x^, and k_cg_begin reads a complex z - w; the CX roles of both kernels)
//   k_cg_p     beta = <r+, r+> / <r, r>;  p = r+ + beta p
// Every scalar is formed on the device, by EVERY workgroup of a slice for itself from the slice's partials (a few hundred doubles, in the
// fixed order of coil_plan.h): no atomics, no host round trip, and nothing that depends on the batch or on a slice's place in it.
// Grid: (cg_blocks(N), B); a workgroup owns CG_SPAN consecutive elements of one slice, thread t the elements t, t + 256, ...
#include "internal.h"
#include "coil_plan.h"
#include "prox_ops.h"

namespace pnp {

// the sum of v[0 .. n) by the whole workgroup, in cg_tree_sum's order; sh: CG_THREADS doubles of LDS, free again on return
__device__ __forceinline__ double block_sum(const double* v, int n, double* sh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += CG_THREADS) s += v[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = CG_THREADS / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// the same tree over one value per thread (a thread's own elements already added in order)
__device__ __forceinline__ double block_sum_own(double s, double* sh) {
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = CG_THREADS / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_expand_ids(const int32_t* mask_id, int32_t* out, int n, int C) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) out[s] = mask_id[coil_pseudo_slice(s, C)];
}

// CX: the state is complex (pnp_set_image): z - w keeps its imaginary part
template <typename R, bool CX>
__global__ __launch_bounds__(CG_THREADS) void k_cg_begin(const CoilState<R, CX>* z, const CoilState<R, CX>* w, typename CxOf<R>::type* xh, size_t N) {
    const size_t base = (size_t)blockIdx.y * N, lo = (size_t)blockIdx.x * CG_SPAN;
    for (size_t i = lo + threadIdx.x; i < lo + CG_SPAN && i < N; i += CG_THREADS) {
        typename CxOf<R>::type v;
        if constexpr (CX) {
            const typename CxOf<R>::type zv = z[base + i], wv = w[base + i];
            v.x = zv.x - wv.x; v.y = zv.y - wv.y;
        } else {
            v.x = z[base + i] - w[base + i]; v.y = R(0);
        }
        xh[base + i] = v;
    }
}

template <typename R>
__global__ __launch_bounds__(CG_THREADS) void k_cg_init(const typename CxOf<R>::type* aty, const typename CxOf<R>::type* xh,
                                                        const typename CxOf<R>::type* gp, typename CxOf<R>::type* r,
                                                        typename CxOf<R>::type* p, R la2, double* part_rr, double* part_bb, size_t N) {
    using C = typename CxOf<R>::type;
    __shared__ double sh[CG_THREADS];
    const size_t base = (size_t)blockIdx.y * N, lo = (size_t)blockIdx.x * CG_SPAN;
    double rr = 0.0, bb = 0.0;
    for (size_t i = lo + threadIdx.x; i < lo + CG_SPAN && i < N; i += CG_THREADS) {
        const C a = aty[base + i], v = xh[base + i], g = gp[base + i];
        C rhs, rv;
        rhs.x = fma_r(la2, v.x, a.x); rhs.y = fma_r(la2, v.y, a.y);
        rv.x = rhs.x - g.x; rv.y = rhs.y - g.y;
        r[base + i] = rv;
        p[base + i] = rv;
        rr += (double)rv.x * (double)rv.x + (double)rv.y * (double)rv.y;
        bb += (double)rhs.x * (double)rhs.x + (double)rhs.y * (double)rhs.y;
    }
    const double srr = block_sum_own(rr, sh), sbb = block_sum_own(bb, sh);
    if (threadIdx.x == 0) {
        const size_t at = cg_partial_index(blockIdx.y, blockIdx.x, gridDim.x);
        part_rr[at] = srr;
        part_bb[at] = sbb;
    }
}

// CX: the last iteration stores x = x^ (complex) instead of |Re x^|
template <typename R, bool CX>
__global__ __launch_bounds__(CG_THREADS) void k_cg_xr(typename CxOf<R>::type* xh, typename CxOf<R>::type* r, const typename CxOf<R>::type* p,
                                                      const typename CxOf<R>::type* gp, const double* part_rr, const double* part_pgp,
                                                      double* part_rr_next, double* scal, CoilState<R, CX>* x_out, size_t N, int H) {
    using C = typename CxOf<R>::type;
    __shared__ double sh[CG_THREADS];
    const int b = blockIdx.y, nblk = gridDim.x;
    const double rr = block_sum(part_rr + cg_partial_index(b, 0, nblk), nblk, sh);
    const double pgp = block_sum(part_pgp + cg_partial_index(b, 0, cg_row_partials(H)), cg_row_partials(H), sh);
    const double alpha = cg_ratio(rr, pgp);
    const R a = (R)alpha;
    const size_t base = (size_t)b * N, lo = (size_t)blockIdx.x * CG_SPAN;
    double rn = 0.0;
    for (size_t i = lo + threadIdx.x; i < lo + CG_SPAN && i < N; i += CG_THREADS) {
        const C pv = p[base + i], gv = gp[base + i];
        C xv = xh[base + i], rv = r[base + i];
        xv.x = fma_r(a, pv.x, xv.x); xv.y = fma_r(a, pv.y, xv.y);
        rv.x = fma_r(-a, gv.x, rv.x); rv.y = fma_r(-a, gv.y, rv.y);
        xh[base + i] = xv;
        r[base + i] = rv;
        if constexpr (CX) { if (x_out) x_out[base + i] = xv; }
        else              { if (x_out) x_out[base + i] = fabs(xv.x); }
        rn += (double)rv.x * (double)rv.x + (double)rv.y * (double)rv.y;
    }
    const double srn = block_sum_own(rn, sh);
    if (threadIdx.x == 0) {
        part_rr_next[cg_partial_index(b, blockIdx.x, nblk)] = srn;
        if (blockIdx.x == 0) { scal[4 * b + 0] = alpha; scal[4 * b + 2] = rr; }
    }
}

template <typename R>
__global__ __launch_bounds__(CG_THREADS) void k_cg_p(const typename CxOf<R>::type* r, typename CxOf<R>::type* p, const double* part_rr,
                                                     const double* part_rr_next, double* scal, size_t N) {
    using C = typename CxOf<R>::type;
    __shared__ double sh[CG_THREADS];
    const int b = blockIdx.y, nblk = gridDim.x;
    const double rr = block_sum(part_rr + cg_partial_index(b, 0, nblk), nblk, sh);
    const double rn = block_sum(part_rr_next + cg_partial_index(b, 0, nblk), nblk, sh);
    const double beta = cg_ratio(rn, rr);
    const R bt = (R)beta;
    const size_t base = (size_t)b * N, lo = (size_t)blockIdx.x * CG_SPAN;
    for (size_t i = lo + threadIdx.x; i < lo + CG_SPAN && i < N; i += CG_THREADS) {
        const C rv = r[base + i];
        C pv = p[base + i];
        pv.x = fma_r(bt, pv.x, rv.x); pv.y = fma_r(bt, pv.y, rv.y);
        p[base + i] = pv;
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) scal[4 * b + 1] = beta;
}

// rel[b] = ||r|| / ||aty + La2 v|| of the x-step just done (0 for a zero right-hand side); one workgroup per slice
__global__ __launch_bounds__(CG_THREADS) void k_cg_residual(const double* part_rr, const double* part_bb, double* rel, int nblk) {
    __shared__ double sh[CG_THREADS];
    const int b = blockIdx.x;
    const double rr = block_sum(part_rr + cg_partial_index(b, 0, nblk), nblk, sh);
    const double bb = block_sum(part_bb + cg_partial_index(b, 0, nblk), nblk, sh);
    if (threadIdx.x == 0) rel[b] = bb > 0.0 ? sqrt(rr / bb) : 0.0;
}

template <typename R>
__global__ __launch_bounds__(256) void k_cabs(const typename CxOf<R>::type* in, R* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const typename CxOf<R>::type v = in[i]; out[i] = sqrt(v.x * v.x + v.y * v.y); }
}

// the pixel prox of the loops in double (float: launch_prox, kernels_generic.hip)
template <bool CNC>
__global__ __launch_bounds__(256) void k_prox_f64(const double* x, double* z, double* w, ProxParamsT<double> p, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double zv = z[i], wv = w[i];
    if (CNC) prox_cnc(x[i], zv, wv, p); else prox_l1(x[i], zv, wv, p);
    z[i] = zv;
    w[i] = wv;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static dim3 cg_grid(int B, size_t N) { return dim3((unsigned)cg_blocks(N), (unsigned)B); }
static unsigned pw_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_expand_ids(hipStream_t s, const int32_t* mask_id, int32_t* out, int B, int C) {
    hipLaunchKernelGGL(k_expand_ids, dim3(pw_blocks((size_t)B * C)), dim3(256), 0, s, mask_id, out, B * C, C);
    return hipGetLastError();
}

template <typename R, bool CX>
hipError_t launch_cg_begin(hipStream_t s, const CoilState<R, CX>* z, const CoilState<R, CX>* w, typename CxOf<R>::type* xh, int B, size_t N) {
    hipLaunchKernelGGL((k_cg_begin<R, CX>), cg_grid(B, N), dim3(CG_THREADS), 0, s, z, w, xh, N);
    return hipGetLastError();
}
template <typename R>
hipError_t launch_cg_init(hipStream_t s, const typename CxOf<R>::type* aty, const typename CxOf<R>::type* xh, const typename CxOf<R>::type* gp,
                          typename CxOf<R>::type* r, typename CxOf<R>::type* p, R la2, double* part_rr, double* part_bb, int B, size_t N) {
    hipLaunchKernelGGL(k_cg_init<R>, cg_grid(B, N), dim3(CG_THREADS), 0, s, aty, xh, gp, r, p, la2, part_rr, part_bb, N);
    return hipGetLastError();
}
template <typename R, bool CX>
hipError_t launch_cg_xr(hipStream_t s, typename CxOf<R>::type* xh, typename CxOf<R>::type* r, const typename CxOf<R>::type* p,
                        const typename CxOf<R>::type* gp, const double* part_rr, const double* part_pgp, double* part_rr_next, double* scal,
                        CoilState<R, CX>* x_out, int B, size_t N, int H) {
    hipLaunchKernelGGL((k_cg_xr<R, CX>), cg_grid(B, N), dim3(CG_THREADS), 0, s, xh, r, p, gp, part_rr, part_pgp, part_rr_next, scal, x_out, N, H);
    return hipGetLastError();
}
template <typename R>
hipError_t launch_cg_p(hipStream_t s, const typename CxOf<R>::type* r, typename CxOf<R>::type* p, const double* part_rr,
                       const double* part_rr_next, double* scal, int B, size_t N) {
    hipLaunchKernelGGL(k_cg_p<R>, cg_grid(B, N), dim3(CG_THREADS), 0, s, r, p, part_rr, part_rr_next, scal, N);
    return hipGetLastError();
}
hipError_t launch_cg_residual(hipStream_t s, const double* part_rr, const double* part_bb, double* rel, int B, size_t N) {
    hipLaunchKernelGGL(k_cg_residual, dim3((unsigned)B), dim3(CG_THREADS), 0, s, part_rr, part_bb, rel, cg_blocks(N));
    return hipGetLastError();
}
template <typename R> hipError_t launch_cabs(hipStream_t s, const typename CxOf<R>::type* in, R* out, size_t n) {
    hipLaunchKernelGGL(k_cabs<R>, dim3(pw_blocks(n)), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}
hipError_t launch_prox_f64(hipStream_t s, bool cnc, const double* x, double* z, double* w, ProxParamsT<double> p, size_t n) {
    if (cnc) hipLaunchKernelGGL(k_prox_f64<true>, dim3(pw_blocks(n)), dim3(256), 0, s, x, z, w, p, n);
    else     hipLaunchKernelGGL(k_prox_f64<false>, dim3(pw_blocks(n)), dim3(256), 0, s, x, z, w, p, n);
    return hipGetLastError();
}

#define COIL_INST(R)                                                                                                                        \
    template hipError_t launch_cg_begin<R, false>(hipStream_t, const R*, const R*, CxOf<R>::type*, int, size_t);                            \
    template hipError_t launch_cg_begin<R, true>(hipStream_t, const CxOf<R>::type*, const CxOf<R>::type*, CxOf<R>::type*, int, size_t);     \
    template hipError_t launch_cg_xr<R, true>(hipStream_t, CxOf<R>::type*, CxOf<R>::type*, const CxOf<R>::type*, const CxOf<R>::type*,      \
                                              const double*, const double*, double*, double*, CxOf<R>::type*, int, size_t, int);            \
    template hipError_t launch_cg_init<R>(hipStream_t, const CxOf<R>::type*, const CxOf<R>::type*, const CxOf<R>::type*, CxOf<R>::type*,    \
                                          CxOf<R>::type*, R, double*, double*, int, size_t);                                                \
    template hipError_t launch_cg_xr<R, false>(hipStream_t, CxOf<R>::type*, CxOf<R>::type*, const CxOf<R>::type*, const CxOf<R>::type*,     \
                                               const double*, const double*, double*, double*, R*, int, size_t, int);                       \
    template hipError_t launch_cg_p<R>(hipStream_t, const CxOf<R>::type*, CxOf<R>::type*, const double*, const double*, double*, int, size_t); \
    template hipError_t launch_cabs<R>(hipStream_t, const CxOf<R>::type*, R*, size_t);
COIL_INST(float)
COIL_INST(double)
#undef COIL_INST

}  // namespace pnp
