// The z / w update of the generic iteration (S1:123-126 / S4:127-132), shared by the row epilogues of kernels_generic.hip and
// kernels_anysize.hip.
#pragma once
#include "internal.h"

namespace pnp {

__device__ __forceinline__ float  fma_r(float a, float b, float c)    { return fmaf(a, b, c); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return fma(a, b, c); }

template <typename R> __device__ __forceinline__ R soft(R a, R c) {
    const R m = fabs(a) - c;
    const R r = m > R(0) ? m : R(0);
    return a < R(0) ? -r : r;
}
template <typename R> __device__ __forceinline__ void prox_l1(R x, R& z, R& w, const ProxParamsT<R>& p) {
    const R u = x + w;
    z = soft(u, p.thr);
    w = u - z;
}
template <typename R> __device__ __forceinline__ void prox_cnc(R x, R& z, R& w, const ProxParamsT<R>& p) {
    const R u = x + w;
    const R clipz = z < -p.ib ? -p.ib : (z > p.ib ? p.ib : z);          // z - soft(z, 1/b)
    const R t = fma_r(p.c1, z, fma_r(p.c2, u, p.c3 * clipz));
    z = soft(t, p.thr);
    w = u - z;
}

}  // namespace pnp
