// A real denoiser on a complex image (include/pnp_mri.h, "PnP denoisers on complex images"): the glue between the complex state of a
// coil context in complex image mode and the real planes [n,1,H,W] a CNN takes.  Float only.  The item functions are pnp_cx_ops.h's.
//   k_cx_den_in<MODE>        v = a (+ b) -> the planes: |v| ('modulus', one plane) or 0.5 + g Re v, 0.5 + g Im v ('parts', the second plane
//                            n floats behind the first)
//   k_cx_den_out<MODE>       the network's planes q and the value v = a (+ b) it was asked about -> complex z
//   k_cx_den_out_dual<MODE>  the same join, then w+ = w + x - z from the unclipped values and the projection of x, z, w+ onto the unit disc:
//                            the last launch of an iteration.  x and w are updated in place; a and b may be x and w (a thread reads
//                            all of its elements before it writes any, and no two threads share an element)
// Streaming kernels: a thread of the vector arm takes 4 complex elements, 16 bytes per access on every array (two on a complex array, one
// on a plane); the thread behind the last group takes the n % 4 tail elements one by one.  The second plane of 'parts' lies on a 16-byte
// boundary only when n % 4 == 0; for the other residues the scalar arm runs: one element per thread, 8-byte and 4-byte accesses,
// consecutive over the lanes (cx_den_vector, the choice pw_shape makes for the real pointwise kernels).  Every element is written exactly
// once and nothing beyond n (2 n on the planes of 'parts').
// Bytes per pixel, b null / b given:   in 'modulus' 12 / 20, 'parts' 16 / 24;   out 'modulus' 20 / 28, 'parts' 16 (its join does not look at
// a, b: the loads are not emitted);   out_dual 'modulus' 52 / 60, 'parts' 48.
// The complex S6:301 is k_combine (kernels_generic.hip) on 2 n floats: the expression is component-wise.
// -ffp-contract=off (Makefile): no fma.  Vector stores only, no atomics.
#include "internal.h"
#include "pnp_cx_ops.h"

namespace pnp {

namespace {

using Cf = Cpx<float>;
struct alignas(16) Cf2 { Cf v[2]; };
struct alignas(16) Fl4 { float v[4]; };

__device__ __forceinline__ Cf cx_sum1(const Cf* a, const Cf* b, size_t e) {
    const Cf v = a[e];
    return b ? v + b[e] : v;
}
__device__ __forceinline__ void cx_load4(const Cf* a, size_t e, Cf (&v)[4]) {
    const Cf2 lo = *(const Cf2*)(a + e), hi = *(const Cf2*)(a + e + 2);
    v[0] = lo.v[0]; v[1] = lo.v[1]; v[2] = hi.v[0]; v[3] = hi.v[1];
}
__device__ __forceinline__ void cx_store4(Cf* a, size_t e, const Cf (&v)[4]) {
    Cf2 lo, hi;
    lo.v[0] = v[0]; lo.v[1] = v[1]; hi.v[0] = v[2]; hi.v[1] = v[3];
    *(Cf2*)(a + e) = lo;
    *(Cf2*)(a + e + 2) = hi;
}
__device__ __forceinline__ void cx_sum4(const Cf* a, const Cf* b, size_t e, Cf (&v)[4]) {
    cx_load4(a, e, v);
    if (b) {
        Cf u[4];
        cx_load4(b, e, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] + u[k];
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void k_cx_den_in(const Cf* a, const Cf* b, float* p, float g, size_t n) {
    size_t e; int cnt;
    cx_den_span(VEC, n, (size_t)blockIdx.x * 256 + threadIdx.x, e, cnt);
    if (VEC && cnt == 4) {
        Cf v[4];
        cx_sum4(a, b, e, v);
        Fl4 p0, p1 = {};
#pragma unroll
        for (int k = 0; k < 4; ++k) cx_den_split<MODE>(v[k], g, p0.v[k], p1.v[k]);
        *(Fl4*)(p + e) = p0;
        if (MODE == CXD_PARTS) *(Fl4*)(p + n + e) = p1;
        return;
    }
    for (int k = 0; k < cnt; ++k) {
        float p0, p1 = 0.0f;
        cx_den_split<MODE>(cx_sum1(a, b, e + k), g, p0, p1);
        p[e + k] = p0;
        if (MODE == CXD_PARTS) p[n + e + k] = p1;
    }
}

// DUAL: x, w are read and written, z is written; otherwise x and w are not touched
template <int MODE, bool VEC, bool DUAL>
__global__ __launch_bounds__(256) void k_cx_den_out(const float* q, const Cf* a, const Cf* b, Cf* x, Cf* z, Cf* w, float g, size_t n) {
    size_t e; int cnt;
    cx_den_span(VEC, n, (size_t)blockIdx.x * 256 + threadIdx.x, e, cnt);
    if (VEC && cnt == 4) {
        Cf v[4], zv[4];
        cx_sum4(a, b, e, v);
        const Fl4 q0 = *(const Fl4*)(q + e);
        Fl4 q1 = {};
        if (MODE == CXD_PARTS) q1 = *(const Fl4*)(q + n + e);
        if (DUAL) {
            Cf xv[4], wv[4];
            cx_load4(x, e, xv);
            cx_load4(w, e, wv);
#pragma unroll
            for (int k = 0; k < 4; ++k) cx_den_join_dual<MODE>(q0.v[k], q1.v[k], v[k], g, xv[k], zv[k], wv[k]);
            cx_store4(x, e, xv);
            cx_store4(z, e, zv);
            cx_store4(w, e, wv);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) zv[k] = cx_den_join<MODE>(q0.v[k], q1.v[k], v[k], g);
            cx_store4(z, e, zv);
        }
        return;
    }
    for (int k = 0; k < cnt; ++k) {
        const size_t i = e + k;
        const Cf v = cx_sum1(a, b, i);
        const float q0 = q[i], q1 = MODE == CXD_PARTS ? q[n + i] : 0.0f;
        if (DUAL) {
            Cf xv = x[i], zv, wv = w[i];
            cx_den_join_dual<MODE>(q0, q1, v, g, xv, zv, wv);
            x[i] = xv; z[i] = zv; w[i] = wv;
        } else {
            z[i] = cx_den_join<MODE>(q0, q1, v, g);
        }
    }
}

bool off16(std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* q : ptrs) bits |= (uintptr_t)q;
    return (bits & 15) != 0;
}
dim3 cx_den_grid(bool vec, size_t n) { return dim3((unsigned)((cx_den_threads(vec, n) + 255) / 256)); }

template <int MODE, bool VEC, bool DUAL>
void den_out_launch(hipStream_t s, const float* q, const float2* a, const float2* b, float2* x, float2* z, float2* w, float g, size_t n) {
    hipLaunchKernelGGL((k_cx_den_out<MODE, VEC, DUAL>), cx_den_grid(VEC, n), dim3(256), 0, s, q, (const Cf*)a, (const Cf*)b, (Cf*)x, (Cf*)z,
                       (Cf*)w, g, n);
}
template <bool DUAL>
hipError_t den_out_any(hipStream_t s, int mode, const float* q, const float2* a, const float2* b, float2* x, float2* z, float2* w, float g, size_t n) {
    if (n < 1 || (mode != CXD_MODULUS && mode != CXD_PARTS) || off16({ q, a, b, x, z, w })) return hipErrorInvalidValue;
    const bool vec = cx_den_vector(mode, n);
    if (mode == CXD_MODULUS) den_out_launch<CXD_MODULUS, true, DUAL>(s, q, a, b, x, z, w, g, n);
    else if (vec)            den_out_launch<CXD_PARTS, true, DUAL>(s, q, a, b, x, z, w, g, n);
    else                     den_out_launch<CXD_PARTS, false, DUAL>(s, q, a, b, x, z, w, g, n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cx_den_in(hipStream_t s, int mode, const float2* a, const float2* b, float* planes, float g, size_t n) {
    if (n < 1 || (mode != CXD_MODULUS && mode != CXD_PARTS) || off16({ a, b, planes })) return hipErrorInvalidValue;
    const Cf *ca = (const Cf*)a, *cb = (const Cf*)b;
    if (mode == CXD_MODULUS)          hipLaunchKernelGGL((k_cx_den_in<CXD_MODULUS, true>), cx_den_grid(true, n), dim3(256), 0, s, ca, cb, planes, g, n);
    else if (cx_den_vector(mode, n))  hipLaunchKernelGGL((k_cx_den_in<CXD_PARTS, true>), cx_den_grid(true, n), dim3(256), 0, s, ca, cb, planes, g, n);
    else                              hipLaunchKernelGGL((k_cx_den_in<CXD_PARTS, false>), cx_den_grid(false, n), dim3(256), 0, s, ca, cb, planes, g, n);
    return hipGetLastError();
}
hipError_t launch_cx_den_out(hipStream_t s, int mode, const float* q, const float2* a, const float2* b, float2* z, float g, size_t n) {
    return den_out_any<false>(s, mode, q, a, b, nullptr, z, nullptr, g, n);
}
hipError_t launch_cx_den_out_dual(hipStream_t s, int mode, const float* q, const float2* a, const float2* b, float2* x, float2* z, float2* w,
                                  float g, size_t n) {
    if (!x || !w) return hipErrorInvalidValue;
    return den_out_any<true>(s, mode, q, a, b, x, z, w, g, n);
}

}  // namespace pnp
