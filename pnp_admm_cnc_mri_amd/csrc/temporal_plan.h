// Temporal sparsity (pnp_set_temporal; kernels_temporal.hip; include/pnp_mri.h, "temporal sparsity"): the argument check, the run of
// pixels a workgroup owns, its LDS layout and -- as work-item functions -- every load, sum and store of the prox.  Host- and
// device-callable code without HIP: the kernel runs these functions one item per thread, tests/host/temporal_emulation.cpp runs them
// one item after another under g++ and the sanitizers.
//
// The batch is S series of T frames, slice b = s T + t, every slice N = H W values V (V = R, or Cpx<R> with complex images).  For every
// series and pixel, u_t = x_t + w_t,
//     U_k = T^(-1/2) sum_t u_t e^(-2 pi i k t / T),   Z_k = csoft(U_k, thr)  (L1)  |  csoft(c1 z^_k + c2 U_k + c3 cclip(z^_k, ib), thr)  (CNC, z^ = F z),
//     z+_t = T^(-1/2) sum_k Z_k e^(+2 pi i k t / T),  w+_t = u_t - z+_t,       and with keep_dc  Z_0 = U_0 (NOT the CNC combination).
// Real images form k = 0 .. T/2 only and rebuild z+_t = T^(-1/2) [Z_0 + 2 sum_{0<k<T/2} Re(Z_k e^(+2 pi i k t / T)) + (T even) Z_(T/2) (-1)^t];
// the coefficients 0 and T/2 are real there and take soft / clip on their real part alone.
//
// Arithmetic: direct sums, t (analysis) and k (synthesis) ascending, every product one explicit fma onto the running sum, the scale
// T^(-1/2) (rounded once to R) applied once per sum.  Twiddles: a table cos, sin (2 pi j / T), j < T, computed in double and rounded once
// to R (tp_twiddles); term (k, t) uses entry j = (k t) mod T.  The kernel reads them from the table laid out as the matrix
// E[r][c] = (cos, sin)(2 pi ((r c) mod T) / T) (tp_twiddle_matrix: the same T values, T x T places), so that a sum walks a row: no index
// arithmetic, and a row index that is uniform over a wavefront makes the reads scalar.
//
// A workgroup owns a RUN of P consecutive pixels of one series across its T frames (the last run of a slice is shorter).  There is one
// layout, TP_LDS: the run lies in LDS as two tiles [T][P] -- u, and z (CNC's input, later z+) -- and the coefficients as [K][P] complex,
// K = T/2 + 1 (real) or T (complex) -- a complex-double series of T = 64 is 2 KiB a pixel, beyond a lane's registers, and one form serves
// every (T, value type).  Four passes with a barrier between them:
//     load    item (t, g): 16 bytes of x, w (CNC: z) of frame t -> u, z tiles
//     coef    item (block of TP_KB coefficients, pixel): U_k (and z^_k) by one walk over t that serves the whole block, thresholded -> Z tile
//     synth   item (block of TP_FB frames, pixel): z+_t by one walk over k that serves the whole block -> z tile
//     store   item (t, g): 16 bytes of z+ and of w+ = u - z+ of frame t leave for memory
// A group g is VP consecutive pixels, VP sizeof(V) <= 16 bytes: the unit of every global access.  Frames lie N values apart, so a group of
// frame t is aligned to its VP sizeof(V) bytes only if N is a multiple of VP (and the arrays are aligned so): tp_group picks the widest VP
// for which that holds -- 128 x 130 x 129 floats (N % 4 = 2) run on 8-byte accesses, an odd N on single values.
// The two middle passes put consecutive pixels on the 64 lanes of a wavefront and give the whole wavefront one block (tp_slot): item =
// 64 slot + lane, slot = (block, 64 pixels).  The block index is uniform over the wavefront (TP_UNIFORM says so to the compiler: the
// twiddle rows are then addressed by scalars), a lane reads its pixel's u once per term for the whole block, and a lane behind the run's
// last pixel does nothing.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include "prox_ops.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TP_HD __host__ __device__
#else
#define TP_HD
#endif

// a value that is the same on every lane of the wavefront, for the compiler to keep in a scalar register
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define TP_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define TP_UNIFORM(x) (x)
#endif

namespace pnp {

constexpr int TP_MIN_FRAMES = 2, TP_MAX_FRAMES = 64;
constexpr int TP_WAVE = 64;                                        // lanes of a slot of the coef and synth passes
constexpr int TP_KB = 4, TP_FB = 4;                                // coefficients resp. frames served by one walk
constexpr int TP_THREADS = 256;
constexpr int TP_MIN_RUN = 16, TP_MAX_RUN = 1024;
constexpr size_t TP_LDS_BUDGET = 40 * 1024;                        // aim of one workgroup's LDS: four workgroups share a compute unit's 160 KiB
enum { TP_LDS = 1 };                                               // layouts (tp_layout): the one there is

// Argument check of pnp_set_temporal / pnp_temporal_check: 0 = valid, else which rule fails
enum { TP_OK = 0, TP_BAD_FRAMES = 1, TP_BAD_BATCH = 2 };
TP_HD constexpr int tp_check(int frames, int B) {
    if (frames < TP_MIN_FRAMES || frames > TP_MAX_FRAMES) return TP_BAD_FRAMES;
    if (B < 1 || B % frames) return TP_BAD_BATCH;
    return TP_OK;
}

// ---- the plan per (T, value type) ------------------------------------------------------------------------------------------------
TP_HD constexpr int tp_layout(int /*T*/, size_t /*value_bytes*/) { return TP_LDS; }
// coefficients formed per pixel
TP_HD constexpr int tp_coefs(int T, bool cx) { return cx ? T : T / 2 + 1; }
// LDS bytes of one pixel of a run: 2 T values and K complex coefficients
TP_HD constexpr size_t tp_pixel_bytes(int T, bool cx, size_t real_bytes) { return 2 * (size_t)T * (cx ? 2 : 1) * real_bytes + (size_t)tp_coefs(T, cx) * 2 * real_bytes; }
// P: the largest power of two in [TP_MIN_RUN, TP_MAX_RUN] (a multiple of every VP) whose run stays within TP_LDS_BUDGET -- and a full
// wavefront of pixels (the middle passes put a pixel on a lane) where 64 of them still fit TP_LDS_WAVE: real floats at T = 53 .. 64.  The
// floor holds for complex doubles from T = 54: 48 KiB at T = 64; no run goes beyond the 64 KiB that need no opt-in
constexpr size_t TP_LDS_WAVE = 52 * 1024;
TP_HD constexpr int tp_run(int T, bool cx, size_t real_bytes) {
    int p = TP_MAX_RUN;
    while (p > TP_MIN_RUN && p * tp_pixel_bytes(T, cx, real_bytes) > TP_LDS_BUDGET) p >>= 1;
    if (p < TP_WAVE && TP_WAVE * tp_pixel_bytes(T, cx, real_bytes) <= TP_LDS_WAVE) p = TP_WAVE;
    return p;
}
TP_HD constexpr size_t tp_align16(size_t b) { return (b + 15) & ~(size_t)15; }
// LDS of one workgroup, in bytes: [u T P V][z T P V][Z K P complex R], every part on 16 bytes
TP_HD constexpr size_t tp_lds_tile_bytes(int T, int P, size_t value_bytes) { return tp_align16((size_t)T * P * value_bytes); }
TP_HD constexpr size_t tp_lds_coef_bytes(int T, int P, bool cx, size_t real_bytes) { return tp_align16((size_t)tp_coefs(T, cx) * P * 2 * real_bytes); }
TP_HD constexpr size_t tp_lds_bytes(int T, bool cx, size_t real_bytes) {
    const size_t vb = (cx ? 2 : 1) * real_bytes;
    const int P = tp_run(T, cx, real_bytes);
    return 2 * tp_lds_tile_bytes(T, P, vb) + tp_lds_coef_bytes(T, P, cx, real_bytes);
}
TP_HD constexpr size_t tp_runs(size_t N, int P) { return (N + P - 1) / P; }
// VP: pixels per access.  `align` = the alignment the three arrays share (a power of two, the low set bit of their addresses or'ed)
TP_HD constexpr int tp_group(size_t N, size_t value_bytes, size_t align) {
    int vp = (int)(16 / value_bytes);
    while (vp > 1 && (N % vp || align % (vp * value_bytes))) vp >>= 1;
    return vp;
}

// the table: tw[j] = cos(2 pi j / T), tw[T + j] = sin(2 pi j / T), in double, rounded once to R
template <typename R> inline void tp_twiddles(int T, R* tw) {
    for (int j = 0; j < T; ++j) {
        const double a = 2.0 * 3.14159265358979323846 * (double)j / (double)T;
        tw[j] = (R)cos(a);
        tw[T + j] = (R)sin(a);
    }
}
// ... and as the context holds it: e[2 (r T + c)], e[2 (r T + c) + 1] = cos, sin of table entry (r c) mod T; 2 T T values
constexpr size_t TP_MATRIX_MAX = 2 * (size_t)TP_MAX_FRAMES * TP_MAX_FRAMES;
template <typename R> inline void tp_twiddle_matrix(int T, R* e) {
    R tw[2 * TP_MAX_FRAMES];
    tp_twiddles<R>(T, tw);
    for (int r = 0; r < T; ++r)
        for (int c = 0; c < T; ++c) {
            const int j = (r * c) % T;
            e[2 * ((size_t)r * T + c)] = tw[j];
            e[2 * ((size_t)r * T + c) + 1] = tw[T + j];
        }
}

// ---- one run ------------------------------------------------------------------------------------------------------------------------
template <typename R, bool CX> using TpValue = typename std::conditional<CX, Cpx<R>, R>::type;

template <typename R, bool CX> struct TpArgs {
    using V = TpValue<R, CX>;
    const V* x;             // [S T][N]
    V *z, *w;
    const R* e;             // tp_twiddle_matrix, in memory
    ProxParamsT<R> p;
    R scale;                // T^(-1/2)
    size_t N;
    int T, S, P;
    int keep_dc;
};
template <typename R, bool CX> struct TpRun {
    size_t base;            // first value of the series: s T N
    size_t p0;              // first pixel of the run
    int np;                 // its pixels (P, or the tail's)
    TpValue<R, CX> *u, *zt; // LDS parts
    Cpx<R>* Z;
};
// run `r` of series `s` on the LDS block `lds` (16-byte aligned, tp_lds_bytes)
template <typename R, bool CX>
TP_HD inline TpRun<R, CX> tp_run_of(const TpArgs<R, CX>& a, int s, size_t r, unsigned char* lds) {
    using V = TpValue<R, CX>;
    TpRun<R, CX> t;
    t.base = (size_t)s * a.T * a.N;
    t.p0 = r * (size_t)a.P;
    t.np = (int)(a.N - t.p0 < (size_t)a.P ? a.N - t.p0 : (size_t)a.P);
    t.u = (V*)lds;
    lds += tp_lds_tile_bytes(a.T, a.P, sizeof(V));
    t.zt = (V*)lds;
    lds += tp_lds_tile_bytes(a.T, a.P, sizeof(V));
    t.Z = (Cpx<R>*)lds;
    return t;
}

// VP values moved as one access
template <typename V, int VP> struct alignas(VP * sizeof(V)) TpVec { V v[VP]; };

TP_HD inline float  tp_soft(float a, float c)   { const float m = fabsf(a) - c; const float r = m > 0.f ? m : 0.f; return a < 0.f ? -r : r; }
TP_HD inline double tp_soft(double a, double c) { const double m = fabs(a) - c; const double r = m > 0.0 ? m : 0.0; return a < 0.0 ? -r : r; }
template <typename R> TP_HD inline R tp_clip(R z, R ib) { return z < -ib ? -ib : (z > ib ? ib : z); }
// prox_cnc's combination on a real coefficient
template <typename R> TP_HD inline R tp_combine(R z, R u, const ProxParamsT<R>& p) { return cpx_fma(p.c1, z, cpx_fma(p.c2, u, p.c3 * tp_clip(z, p.ib))); }

// items of the passes
TP_HD constexpr int tp_groups(int np, int VP) { return np / VP; }                      // np is a multiple of VP (tp_group)
TP_HD constexpr int tp_load_items(int T, int np, int VP) { return T * tp_groups(np, VP); }
TP_HD constexpr int tp_store_items(int T, int np, int VP) { return T * tp_groups(np, VP); }
TP_HD constexpr int tp_pixel_slots(int np) { return (np + TP_WAVE - 1) / TP_WAVE; }
TP_HD constexpr int tp_blocks(int n, int per) { return (n + per - 1) / per; }
TP_HD constexpr int tp_coef_items(int T, bool cx, int np) { return tp_blocks(tp_coefs(T, cx), TP_KB) * tp_pixel_slots(np) * TP_WAVE; }
TP_HD constexpr int tp_synth_items(int T, int np) { return tp_blocks(T, TP_FB) * tp_pixel_slots(np) * TP_WAVE; }
// item of a middle pass -> its block (uniform over the 64 items of a slot) and its pixel (>= np: nothing to do)
struct TpSlot { int block, p; };
TP_HD inline TpSlot tp_slot(int item, int np) {
    const int slots = tp_pixel_slots(np), slot = item / TP_WAVE;
    return {TP_UNIFORM(slot / slots), (slot % slots) * TP_WAVE + item % TP_WAVE};
}

// load, item = (t, g): u = x + w (component-wise) and, CNC, z of VP pixels of frame t
template <typename R, bool CX, bool CNC, int VP>
TP_HD inline void tp_load_item(int item, const TpArgs<R, CX>& a, const TpRun<R, CX>& t) {
    using V = TpValue<R, CX>;
    using Vec = TpVec<V, VP>;
    const int G = tp_groups(t.np, VP), f = item / G, q = (item - f * G) * VP;
    const size_t o = t.base + (size_t)f * a.N + t.p0 + q;
    const Vec xv = *(const Vec*)(a.x + o), wv = *(const Vec*)(a.w + o);
    Vec uv;
    for (int e = 0; e < VP; ++e) uv.v[e] = xv.v[e] + wv.v[e];
    *(Vec*)(t.u + (size_t)f * a.P + q) = uv;
    if constexpr (CNC) *(Vec*)(t.zt + (size_t)f * a.P + q) = *(const Vec*)(a.z + o);
}

// one term of an analysis sum: acc += v e^(-i theta), (c, s) = (cos, sin) theta
template <typename R> TP_HD inline void tp_acc_fwd(R v, R c, R s, Cpx<R>& acc) {
    acc.re = cpx_fma(v, c, acc.re);
    acc.im = cpx_fma(-v, s, acc.im);
}
template <typename R> TP_HD inline void tp_acc_fwd(Cpx<R> v, R c, R s, Cpx<R>& acc) {
    acc.re = cpx_fma(v.re, c, acc.re);
    acc.re = cpx_fma(v.im, s, acc.re);
    acc.im = cpx_fma(v.im, c, acc.im);
    acc.im = cpx_fma(-v.re, s, acc.im);
}
// one term of a synthesis sum: acc += Z e^(+i theta)
template <typename R> TP_HD inline void tp_acc_inv(Cpx<R> Z, R c, R s, Cpx<R>& acc) {
    acc.re = cpx_fma(Z.re, c, acc.re);
    acc.re = cpx_fma(-Z.im, s, acc.re);
    acc.im = cpx_fma(Z.re, s, acc.im);
    acc.im = cpx_fma(Z.im, c, acc.im);
}

// the thresholded coefficient k from the finished sums of u and (CNC) z
template <typename R, bool CX, bool CNC>
TP_HD inline Cpx<R> tp_threshold(int k, Cpx<R> su, Cpx<R> sz, const TpArgs<R, CX>& a) {
    // a real image's coefficients 0 and T/2 are real: their imaginary sums are dropped
    const bool real_coef = !CX && (k == 0 || 2 * k == a.T);
    const bool penalised = !(k == 0 && a.keep_dc);
    Cpx<R> U(su.re * a.scale, su.im * a.scale), Zk = U;
    if (real_coef) {
        U.im = R(0);
        Zk = U;
        if (penalised) Zk.re = tp_soft(CNC ? tp_combine(sz.re * a.scale, U.re, a.p) : U.re, a.p.thr);
    } else if (penalised) {
        if (CNC) Zk = csoft(cnc_combine_cx(Cpx<R>(sz.re * a.scale, sz.im * a.scale), U, a.p), a.p.thr);
        else     Zk = csoft(U, a.p.thr);
    }
    return Zk;
}

// coef, item = (block of TP_KB coefficients, pixel): one walk over t for the block; the block's last coefficients beyond K - 1 repeat
// K - 1 and are not stored
template <typename R, bool CX, bool CNC>
TP_HD inline void tp_coef_item(int item, const TpArgs<R, CX>& a, const TpRun<R, CX>& t) {
    using V = TpValue<R, CX>;
    const int T = a.T, K = tp_coefs(T, CX);
    const TpSlot sl = tp_slot(item, t.np);
    if (sl.p >= t.np) return;
    const int k0 = sl.block * TP_KB;
    const R* row[TP_KB];
    Cpx<R> au[TP_KB], az[TP_KB];
    for (int i = 0; i < TP_KB; ++i) {
        const int k = k0 + i < K ? k0 + i : K - 1;
        row[i] = a.e + 2 * (size_t)k * T;
        au[i] = az[i] = Cpx<R>(R(0), R(0));
    }
    for (int f = 0; f < T; ++f) {
        const V uv = t.u[(size_t)f * a.P + sl.p];
        V zv = uv;
        if constexpr (CNC) zv = t.zt[(size_t)f * a.P + sl.p];
        for (int i = 0; i < TP_KB; ++i) {
            const R c = row[i][2 * f], s = row[i][2 * f + 1];
            tp_acc_fwd(uv, c, s, au[i]);
            if constexpr (CNC) tp_acc_fwd(zv, c, s, az[i]);
        }
    }
    for (int i = 0; i < TP_KB; ++i)
        if (k0 + i < K) t.Z[(size_t)(k0 + i) * a.P + sl.p] = tp_threshold<R, CX, CNC>(k0 + i, au[i], az[i], a);
}

// synth, item = (block of TP_FB frames, pixel): z+ of the block's frames from the Z tile by one walk over k, into the z tile; the block's
// last frames beyond T - 1 repeat T - 1 and are not stored
template <typename R, bool CX>
TP_HD inline void tp_synth_item(int item, const TpArgs<R, CX>& a, const TpRun<R, CX>& t) {
    using V = TpValue<R, CX>;
    const int T = a.T;
    const TpSlot sl = tp_slot(item, t.np);
    if (sl.p >= t.np) return;
    const int f0 = sl.block * TP_FB;
    const R* row[TP_FB];
    Cpx<R> acc[TP_FB];
    for (int i = 0; i < TP_FB; ++i) {
        const int f = f0 + i < T ? f0 + i : T - 1;
        row[i] = a.e + 2 * (size_t)f * T;
        acc[i] = Cpx<R>(R(0), R(0));
    }
    V zn[TP_FB];
    if constexpr (CX) {
        for (int k = 0; k < T; ++k) {
            const Cpx<R> Zk = t.Z[(size_t)k * a.P + sl.p];
            for (int i = 0; i < TP_FB; ++i) tp_acc_inv(Zk, row[i][2 * k], row[i][2 * k + 1], acc[i]);
        }
        for (int i = 0; i < TP_FB; ++i) zn[i] = Cpx<R>(a.scale * acc[i].re, a.scale * acc[i].im);
    } else {
        for (int k = 1; 2 * k < T; ++k) {
            const Cpx<R> Zk = t.Z[(size_t)k * a.P + sl.p];
            for (int i = 0; i < TP_FB; ++i) {
                acc[i].re = cpx_fma(Zk.re, row[i][2 * k], acc[i].re);
                acc[i].re = cpx_fma(-Zk.im, row[i][2 * k + 1], acc[i].re);
            }
        }
        const R dc = t.Z[sl.p].re, ny = T % 2 == 0 ? t.Z[(size_t)(T / 2) * a.P + sl.p].re : R(0);
        for (int i = 0; i < TP_FB; ++i) {
            R v = cpx_fma(R(2), acc[i].re, dc);
            if (T % 2 == 0) v = ((f0 + i) & 1) ? v - ny : v + ny;
            zn[i] = a.scale * v;
        }
    }
    for (int i = 0; i < TP_FB; ++i)
        if (f0 + i < T) t.zt[(size_t)(f0 + i) * a.P + sl.p] = zn[i];
}

// store, item = (t, g): z+ and w+ = u - z+ of VP pixels of frame t leave for memory
template <typename R, bool CX, int VP>
TP_HD inline void tp_store_item(int item, const TpArgs<R, CX>& a, const TpRun<R, CX>& t) {
    using V = TpValue<R, CX>;
    using Vec = TpVec<V, VP>;
    const int G = tp_groups(t.np, VP), f = item / G, q = (item - f * G) * VP;
    const Vec uv = *(const Vec*)(t.u + (size_t)f * a.P + q), zv = *(const Vec*)(t.zt + (size_t)f * a.P + q);
    Vec wv;
    for (int e = 0; e < VP; ++e) wv.v[e] = uv.v[e] - zv.v[e];
    const size_t o = t.base + (size_t)f * a.N + t.p0 + q;
    *(Vec*)(a.z + o) = zv;
    *(Vec*)(a.w + o) = wv;
}

}  // namespace pnp
