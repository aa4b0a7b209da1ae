// The row and column roles of the c2c kernels, stated once.
//
// Every operator outside the fused and slice engines is two launches: a row launch (RowIn, inverse, RowEpi) and a column launch
// (pre, ColMid, post).  This header holds what such a triple MEANS -- the element forms of the inputs, epilogues and k-space ops -- and
// which triples exist; the kernels of kernels_generic.hip (k_rows, k_cols, k_cols16, k_cols32) and kernels_anysize.hip (k_any_rows,
// k_any_cols) supply the transforms, tiles and operand fetches around them.  Plain C++17, host- and device-callable without HIP
// (CxOf<R> is specialised by internal.h for float2 / double2): tests/host/c2c_roles_emulation.cpp runs this text under g++.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include "prox_ops.h"

#if defined(__HIPCC__)
#define C2C_HD __host__ __device__ __forceinline__
#else
#define C2C_HD inline
#endif

namespace pnp {

enum RowIn  { IN_COMPLEX = 0, IN_REAL = 1, IN_REAL_DIFF = 2 };
enum RowEpi { EPI_COMPLEX = 0, EPI_ABS_REAL = 1, EPI_ABS_COMPLEX = 2, EPI_L1 = 3, EPI_CNC = 4 };
enum ColMid { MID_NONE = 0, MID_BLEND = 1, MID_MASK = 2, MID_RESID = 3, MID_MASK_ADD = 4 };

// complex type per precision: any struct with members x, y of type R
template <typename R> struct CxOf;

template <typename R>
struct RowArgsT {
    using C = typename CxOf<R>::type;
    const C* cin;      // IN_COMPLEX
    const R* rin0;     // IN_REAL / IN_REAL_DIFF (minuend)
    const R* rin1;     // IN_REAL_DIFF (subtrahend)
    C*       cout;     // EPI_COMPLEX
    R*       x_out;    // EPI_ABS_* (required) / EPI_L1, EPI_CNC (optional, may be null)
    R*       z;        // EPI_L1 / EPI_CNC: read old, write new
    R*       w;
    R        scale;    // applied to the transform output
    ProxParamsT<R> prox;
    int      nrows;    // B*H
};

template <typename R>
struct ColArgsT {
    using C = typename CxOf<R>::type;
    const C*       in;
    C*             out;        // may alias in
    const C*       y;          // MID_BLEND / MID_RESID: measurements; MID_MASK_ADD: noise
    const uint8_t* mask_bank;  // [K][H][W]
    const int32_t* mask_id;    // [B] or null
    R              c;          // MID_BLEND: 1/(1+La2)
    int            y_per_slice;// MID_MASK_ADD: 0 = one [H][W] noise array for all slices
    int            B;
};

// ---- complex arithmetic on C = float2 / double2 / cxT<R> / any {x, y} (the cxT operators of fft16.h belong to the fused engines) ----
template <typename C, typename R> C2C_HD C mkc(R x, R y) { C r; r.x = x; r.y = y; return r; }
template <typename C> C2C_HD C cmul(C a, C b)  { return mkc<C>(fma_r(a.x, b.x, -(a.y * b.y)), fma_r(a.x, b.y, a.y * b.x)); }
template <typename C> C2C_HD C cmulc(C a, C b) { return mkc<C>(fma_r(a.x, b.x, a.y * b.y), fma_r(a.y, b.x, -(a.x * b.y))); }   // a * conj(b)
template <typename C> C2C_HD C cadd(C a, C b)  { return mkc<C>(a.x + b.x, a.y + b.y); }
template <typename C> C2C_HD C csub(C a, C b)  { return mkc<C>(a.x - b.x, a.y - b.y); }
template <typename C> C2C_HD C cconj(C a)      { return mkc<C>(a.x, -a.y); }

// ---- rows: element e of the input of a row transform, and what becomes of element e of its output v ----
template <int IN, typename R> C2C_HD typename CxOf<R>::type row_load(const RowArgsT<R>& p, size_t e) {
    using C = typename CxOf<R>::type;
    if (IN == IN_COMPLEX) return p.cin[e];
    if (IN == IN_REAL) return mkc<C>(p.rin0[e], R(0));
    return mkc<C>(p.rin0[e] - p.rin1[e], R(0));
}

template <int EPI, typename R> C2C_HD void row_store(const RowArgsT<R>& p, size_t e, typename CxOf<R>::type v) {
    using C = typename CxOf<R>::type;
    if (EPI == EPI_COMPLEX) {
        p.cout[e] = mkc<C>(v.x * p.scale, v.y * p.scale);
    } else if (EPI == EPI_ABS_REAL) {
        p.x_out[e] = fabs(v.x * p.scale);
    } else if (EPI == EPI_ABS_COMPLEX) {
        p.x_out[e] = sqrt(v.x * v.x + v.y * v.y) * p.scale;
    } else {
        const R x = fabs(v.x * p.scale);
        R z = p.z[e], w = p.w[e];
        if (EPI == EPI_L1) prox_l1(x, z, w, p.prox); else prox_cnc(x, z, w, p.prox);
        p.z[e] = z;
        p.w[e] = w;
        if (p.x_out) p.x_out[e] = x;
    }
}

// ---- columns: the k-space op on one element X; m: the mask byte is set; y: the element's measurement (BLEND, RESID) or noise
// (MASK_ADD) -- a value the kernel already holds in a register (k_cols16 fetches at kernel start), or a pointer to it in global memory,
// read only where this function asks: where m is set (BLEND, RESID), always (MASK_ADD), never (MASK).
// An unsampled measurement is SELECTED away, never multiplied: a NaN there cannot reach the result.
template <typename C> C2C_HD C col_operand(C y)        { return y; }
template <typename C> C2C_HD C col_operand(const C* y) { return *y; }

template <int MID, typename C, typename R, typename Y> C2C_HD C col_mid(C X, bool m, Y y, R c) {
    if (MID == MID_BLEND) {
        if (m) { const C yv = col_operand(y); X.x = fma_r(yv.x - X.x, c, X.x); X.y = fma_r(yv.y - X.y, c, X.y); }
    } else if (MID == MID_MASK) {
        if (!m) X = mkc<C>(R(0), R(0));
    } else if (MID == MID_RESID) {
        if (m) { const C yv = col_operand(y); X.x -= yv.x; X.y -= yv.y; } else X = mkc<C>(R(0), R(0));
    } else if (MID == MID_MASK_ADD) {
        const C nv = col_operand(y);
        X = m ? cadd(X, nv) : nv;
    }
    return X;
}

// ---- the legal triples.  f receives the triple as three std::integral_constants and returns what its launch returns; any other
// triple returns `invalid` without calling f.  Every kernel family instantiates exactly this list.
template <int V> using role_c = std::integral_constant<int, V>;

template <typename Ret, typename F>
inline Ret row_roles(RowIn in, bool inv, RowEpi epi, Ret invalid, F&& f) {
    constexpr std::false_type fwd{};
    constexpr std::true_type  bwd{};
    if (!inv && epi == EPI_COMPLEX) {
        if (in == IN_COMPLEX)   return f(role_c<IN_COMPLEX>{}, fwd, role_c<EPI_COMPLEX>{});        // fft2
        if (in == IN_REAL)      return f(role_c<IN_REAL>{}, fwd, role_c<EPI_COMPLEX>{});           // A, synthesis
        if (in == IN_REAL_DIFF) return f(role_c<IN_REAL_DIFF>{}, fwd, role_c<EPI_COMPLEX>{});      // the iteration: z - w
    }
    if (inv && in == IN_COMPLEX) {
        if (epi == EPI_COMPLEX)     return f(role_c<IN_COMPLEX>{}, bwd, role_c<EPI_COMPLEX>{});    // ifft2
        if (epi == EPI_ABS_REAL)    return f(role_c<IN_COMPLEX>{}, bwd, role_c<EPI_ABS_REAL>{});   // the iteration's x
        if (epi == EPI_ABS_COMPLEX) return f(role_c<IN_COMPLEX>{}, bwd, role_c<EPI_ABS_COMPLEX>{});// the initial state
        if (epi == EPI_L1)          return f(role_c<IN_COMPLEX>{}, bwd, role_c<EPI_L1>{});
        if (epi == EPI_CNC)         return f(role_c<IN_COMPLEX>{}, bwd, role_c<EPI_CNC>{});
    }
    return invalid;
}

template <typename Ret, typename F>
inline Ret col_roles(bool pre, ColMid mid, bool post, Ret invalid, F&& f) {
    constexpr std::false_type no{};
    constexpr std::true_type  yes{};
    if (pre && !post && mid == MID_NONE)      return f(yes, role_c<MID_NONE>{}, no);
    if (!pre && post && mid == MID_NONE)      return f(no, role_c<MID_NONE>{}, yes);
    if (pre && post && mid == MID_BLEND)      return f(yes, role_c<MID_BLEND>{}, yes);
    if (pre && !post && mid == MID_MASK)      return f(yes, role_c<MID_MASK>{}, no);
    if (pre && post && mid == MID_MASK)       return f(yes, role_c<MID_MASK>{}, yes);      // the coil columns of G (any-size kernels only)
    if (!pre && post && mid == MID_MASK)      return f(no, role_c<MID_MASK>{}, yes);
    if (pre && post && mid == MID_RESID)      return f(yes, role_c<MID_RESID>{}, yes);
    if (pre && !post && mid == MID_MASK_ADD)  return f(yes, role_c<MID_MASK_ADD>{}, no);
    return invalid;
}

}  // namespace pnp
