// A real denoiser on a complex image (include/pnp_mri.h, "PnP denoisers on complex images"): the item functions between a complex state
// and the real planes a CNN takes, host- and device-callable without HIP like prox_ops.h, so tests/host/pnp_cx_emulation.cpp runs the same
// text under g++ and the sanitizers.  Float only, as the PnP path is.  No fma anywhere: every +, *, /, sqrt is one correctly rounded
// float operation in the order written (-ffp-contract=off), which is what tests/pnp_complex_oracle.py restates in NumPy.
//   'modulus'  one plane  m = |v|;            D(v) = (d / m) v where m != 0, (d, 0) where m == 0        (d = the network's answer to m)
//   'parts'    two planes 0.5 + g Re v, 0.5 + g Im v;   D(v) = ((q0 - 0.5) / g, (q1 - 0.5) / g)
#pragma once
#include <stddef.h>
#include "prox_ops.h"

namespace pnp {

enum { CXD_MODULUS = 0, CXD_PARTS = 1 };                 // PNP_CX_DENOISE_* of include/pnp_mri.h

// v -> the plane values; 'modulus' leaves p1 alone (there is no second plane)
template <int MODE> PROX_HD inline void cx_den_split(Cpx<float> v, float g, float& p0, float& p1) {
    if (MODE == CXD_MODULUS) {
        p0 = cpx_abs(v);
    } else {
        const float a = g * v.re, b = g * v.im;
        p0 = 0.5f + a;
        p1 = 0.5f + b;
    }
}

// the network's planes and the value v it was asked about -> the denoised complex value.  'modulus': one division, then two products;
// d may be negative and is not clamped; m == 0 (both signs of zero, squares that underflow) has no phase to keep: (d, 0), never 0 / 0.
// A NaN in v or d comes out as NaN.  'parts' does not look at v
template <int MODE> PROX_HD inline Cpx<float> cx_den_join(float q0, float q1, Cpx<float> v, float g) {
    if (MODE == CXD_MODULUS) {
        const float m = cpx_abs(v);
        if (m == 0.0f) return {q0, 0.0f};
        const float f = q0 / m;
        return {f * v.re, f * v.im};
    } else {
        const float a = q0 - 0.5f, b = q1 - 0.5f;
        return {a / g, b / g};
    }
}

// the join fused with the dual update and the three projections onto the unit disc (the complex clamp(0, 1) of S6:305-308): w is formed
// from the unclipped x and z, left to right as k_dual_clamp does
template <int MODE> PROX_HD inline void cx_den_join_dual(float q0, float q1, Cpx<float> v, float g, Cpx<float>& x, Cpx<float>& z, Cpx<float>& w) {
    const Cpx<float> zn = cx_den_join<MODE>(q0, q1, v, g);
    const Cpx<float> wn = (w + x) - zn;
    x = cclip(x, 1.0f);
    z = cclip(zn, 1.0f);
    w = cclip(wn, 1.0f);
}

// ---- the index map of the kernels: n complex elements, a thread of the vector arm takes 4 (two 16-byte accesses on a complex array, one
// per plane), the thread behind the last full group takes the n % 4 elements of the tail one by one; the scalar arm takes one element per
// thread.  The vector arm needs the second plane on a 16-byte boundary: it starts n floats behind the first, so 'parts' takes it only
// when n % 4 == 0 (then there is no tail either); 'modulus' has one plane and always takes it.
PROX_HD inline bool cx_den_vector(int mode, size_t n) { return mode == CXD_MODULUS || (n & 3) == 0; }
PROX_HD inline size_t cx_den_threads(bool vec, size_t n) { return vec ? n / 4 + ((n & 3) ? 1 : 0) : n; }
// the elements [first, first + count) of thread i
PROX_HD inline void cx_den_span(bool vec, size_t n, size_t i, size_t& first, int& count) {
    if (!vec) { first = i; count = i < n ? 1 : 0; return; }
    const size_t n4 = n / 4;
    first = 4 * i;
    count = i < n4 ? 4 : (i == n4 ? (int)(n & 3) : 0);
}

}  // namespace pnp
