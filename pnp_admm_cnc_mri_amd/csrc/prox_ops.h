// The z / w update of the generic iteration (S1:123-126 / S4:127-132), applied by the row epilogues of c2c_roles.h -- and its complex form
// (include/pnp_mri.h, "complex-valued images"): csoft, cclip and the two steps on a complex state.  Host- and device-callable without
// HIP, so tests/host/c2c_roles_emulation.cpp and tests/host/complex_emulation.cpp run the same text under g++ and the sanitizers.
#pragma once
#include <math.h>
#include "prox_params.h"
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROX_HD __host__ __device__
#else
#define PROX_HD
#endif

namespace pnp {

// the fused multiply-add of the c2c roles, the real prox, the coil and the wavelet kernels (-ffp-contract=off: only such calls fuse);
// the complex and temporal code below keeps its own name for the same call, cpx_fma
PROX_HD inline float  fma_r(float a, float b, float c)    { return fmaf(a, b, c); }
PROX_HD inline double fma_r(double a, double b, double c) { return fma(a, b, c); }

template <typename R> PROX_HD inline R soft(R a, R c) {
    const R m = fabs(a) - c;
    const R r = m > R(0) ? m : R(0);
    return a < R(0) ? -r : r;
}
template <typename R> PROX_HD inline void prox_l1(R x, R& z, R& w, const ProxParamsT<R>& p) {
    const R u = x + w;
    z = soft(u, p.thr);
    w = u - z;
}
template <typename R> PROX_HD inline void prox_cnc(R x, R& z, R& w, const ProxParamsT<R>& p) {
    const R u = x + w;
    const R clipz = z < -p.ib ? -p.ib : (z > p.ib ? p.ib : z);          // z - soft(z, 1/b)
    const R t = fma_r(p.c1, z, fma_r(p.c2, u, p.c3 * clipz));
    z = soft(t, p.thr);
    w = u - z;
}

// ---- complex state: a value is two components of S (float | double) --------------------------------------------------------------
template <typename S> struct alignas(2 * sizeof(S)) Cpx {
    S re, im;
    Cpx() = default;
    PROX_HD constexpr Cpx(S r, S i) : re(r), im(i) {}
    PROX_HD explicit constexpr Cpx(double v) : re((S)v), im((S)v) {}      // a real factor for both components (the wavelet filters' taps)
};
// component-wise: what a real-linear map does to a complex value (NOT the complex product)
template <typename S> PROX_HD inline Cpx<S> operator+(Cpx<S> a, Cpx<S> b) { return {a.re + b.re, a.im + b.im}; }
template <typename S> PROX_HD inline Cpx<S> operator-(Cpx<S> a, Cpx<S> b) { return {a.re - b.re, a.im - b.im}; }
template <typename S> PROX_HD inline Cpx<S> operator*(Cpx<S> a, Cpx<S> b) { return {a.re * b.re, a.im * b.im}; }

PROX_HD inline float  cpx_fma(float a, float b, float c)    { return fmaf(a, b, c); }
PROX_HD inline double cpx_fma(double a, double b, double c) { return fma(a, b, c); }
PROX_HD inline float  cpx_sqrt(float a)  { return sqrtf(a); }
PROX_HD inline double cpx_sqrt(double a) { return sqrt(a); }

// the item functions of wavelet_plan.h instantiated on Cpx<S> find this by argument-dependent lookup: Psi is real-linear, so a tap
// is one fma per component, in the order of the real instance
template <typename S> PROX_HD inline Cpx<S> wv_fma(Cpx<S> a, Cpx<S> b, Cpx<S> c) { return {cpx_fma(a.re, b.re, c.re), cpx_fma(a.im, b.im, c.im)}; }

// |u|: two rounded products, one sum (no fma: -ffp-contract=off), one square root
template <typename S> PROX_HD inline S cpx_abs(Cpx<S> u) {
    const S a = u.re * u.re, b = u.im * u.im;
    return cpx_sqrt(a + b);
}
// the prox of c |.|: u (|u| - c) / |u| where |u| > c, 0 elsewhere (|u| = 0 included)
template <typename S> PROX_HD inline Cpx<S> csoft(Cpx<S> u, S c) {
    const S m = cpx_abs(u);
    const S s = m > c ? (m - c) / m : S(0);
    return {s * u.re, s * u.im};
}
// the projection onto the disc of radius ib: z - csoft(z, ib)
template <typename S> PROX_HD inline Cpx<S> cclip(Cpx<S> z, S ib) {
    const S m = cpx_abs(z);
    if (!(m > ib)) return z;
    const S f = ib / m;
    return {z.re * f, z.im * f};
}
// t = c1 z + c2 u + c3 cclip(z, ib), component-wise with prox_cnc's fma chain
template <typename S> PROX_HD inline Cpx<S> cnc_combine_cx(Cpx<S> z, Cpx<S> u, const ProxParamsT<S>& p) {
    const Cpx<S> cl = cclip(z, p.ib);
    return {cpx_fma(p.c1, z.re, cpx_fma(p.c2, u.re, p.c3 * cl.re)), cpx_fma(p.c1, z.im, cpx_fma(p.c2, u.im, p.c3 * cl.im))};
}
template <typename S> PROX_HD inline void prox_l1_cx(Cpx<S> x, Cpx<S>& z, Cpx<S>& w, const ProxParamsT<S>& p) {
    const Cpx<S> u = x + w;
    z = csoft(u, p.thr);
    w = u - z;
}
template <typename S> PROX_HD inline void prox_cnc_cx(Cpx<S> x, Cpx<S>& z, Cpx<S>& w, const ProxParamsT<S>& p) {
    const Cpx<S> u = x + w;
    z = csoft(cnc_combine_cx(z, u, p), p.thr);
    w = u - z;
}

}  // namespace pnp
