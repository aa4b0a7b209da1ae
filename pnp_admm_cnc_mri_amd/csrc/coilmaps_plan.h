// Coil sensitivity maps from the calibration region of k-space (pnp_coil_maps; kernels_coilmaps.hip): the local dominant-eigenvector
// method (Walsh's adaptive combination) in matrix-free form on low-resolution coil images.  Pure host-callable code without HIP: the
// argument rule, the window, the patch order and its wrap, one power step and the phase step as templates on the real type, the tile
// choice, and coilmaps_slice, the whole-slice restatement the kernels follow operation by operation.  The kernels run by it and
// tests/host/coilmaps_emulation.cpp checks it under g++.  Every unit is built with -ffp-contract=off: a fused multiply-add is where
// coilmix_fma is written and nowhere else.
//
// One slice, y [C][H][W] un-shifted (DC at (0, 0)), real type R:
//   window   calibration line i = 0 .. ncal - 1 of an axis has the signed frequency f = i (i < ceil(ncal / 2)) or i - ncal; its weight is
//            w(f) = cos^2(pi f / (ncal + 1)), formed in double and rounded once to R (coilmaps_window).  K_c = (w_H(i) * w_W(j)) * y_c at
//            calibration point (i, j) -- the two weights multiplied first, then re and im by that product -- and +0 elsewhere.
//   images   I_c = ifft2(K_c) by the context's own inverse transform (rows, then columns; the rows carry 1 / (H W)).
//   start    v = I(p) / ||I(p)||, ||.||^2 = coilmaps_norm2: ONE chain of fused multiply-adds over c = 0 .. C - 1, re before im;
//            v = e_0 when the norm is 0.
//   power    n times: u = 0; for the (2r + 1)^2 patch points q in row-major order (dy, dx) = (-r, -r) .. (r, r), wrapped on both axes:
//            g = sum_c conj(I_c(q)) v_c  (c in order, four fused multiply-adds per coil: coilmaps_cmac_conj), then u_c += I_c(q) g for
//            every c (coilmix_cmac).  lambda = sqrt(coilmaps_norm2(u)); v = u / lambda (a division per component) unless lambda = 0.
//   phase    g = sum_c conj(v_c) I_c(p); m = sqrt(fma(g.re, g.re, g.im * g.im)); unless m = 0: e = g / m and v_c <- v_c e
//            (re = fma(-v.im, e.im, v.re * e.re), im = fma(v.im, e.re, v.re * e.im)).  Then v^H I(p) >= 0.
//   support  lambda_max = the slice's largest lambda (of the last power step); S(p) = v(p) where lambda(p) >= tau2 * lambda_max, tau2 =
//            (R)(thresh * thresh) formed in double; elsewhere S(p) = +0 in every coil.
// No sum depends on B, on the tile, or on the pixel's position: a slice alone and the slice in a batch are bit-equal.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "coilmix_plan.h"

namespace pnp {

constexpr int COILMAPS_MAX_RADIUS = 3;        // 0 <= radius <= COILMAPS_MAX_RADIUS: patches of 1, 9, 25, 49 pixels
constexpr int COILMAPS_MAX_ITERS = 16;        // 1 <= power_iters <= COILMAPS_MAX_ITERS
constexpr int COILMAPS_WIN_THREADS = 256;     // k_calib_window: a thread owns 16 bytes of consecutive points (coilmix_points)
constexpr int COILMAPS_SPAN = 4096;           // k_maps_keymax / k_maps_support: pixels of one slice per workgroup of 256 threads
constexpr int COILMAPS_SUP_THREADS = 256;
constexpr size_t COILMAPS_LDS_SOFT = 64 * 1024;     // the tile is the largest whose staged coil images stay within this ...
constexpr size_t COILMAPS_LDS_HARD = 128 * 1024;    // ... and where none does (C = 32 in double at radius 3) the smallest, within this

enum { COILMAPS_OK = 0, COILMAPS_BAD_C = 1, COILMAPS_BAD_NCAL = 2, COILMAPS_BAD_RADIUS = 3, COILMAPS_BAD_ITERS = 4, COILMAPS_BAD_THRESH = 5,
       COILMAPS_BAD_SHAPE = 6 };
COIL_HD inline int coilmaps_check(int C, int ncal, int radius, int power_iters, double thresh, int H, int W) {
    if (C < 1 || C > COIL_MAX_C) return COILMAPS_BAD_C;
    if (H < 128 || H > 1024 || W < 128 || W > 1024) return COILMAPS_BAD_SHAPE;
    if (coilmix_check(C, 1, 1, ncal, H, W) == COILMIX_BAD_NCAL) return COILMAPS_BAD_NCAL;
    if (radius < 0 || radius > COILMAPS_MAX_RADIUS) return COILMAPS_BAD_RADIUS;
    if (power_iters < 1 || power_iters > COILMAPS_MAX_ITERS) return COILMAPS_BAD_ITERS;
    if (!(thresh >= 0.0) || !(thresh < 1.0)) return COILMAPS_BAD_THRESH;
    return COILMAPS_OK;
}

// ---- window ----------------------------------------------------------------------------------------------------------------------
COIL_HD inline int coilmaps_freq(int i, int ncal) { return i < (ncal + 1) / 2 ? i : i - ncal; }
inline double coilmaps_window(int i, int ncal) {
    const double c = cos(3.14159265358979323846 * (double)coilmaps_freq(i, ncal) / (double)(ncal + 1));
    return c * c;
}
// the weights of the ncal lines of an axis, rounded once to R: what the window kernel takes as an argument
template <typename R> struct CoilmapsWindow { R w[COILMIX_NCAL_MAX]; };
template <typename R> inline CoilmapsWindow<R> coilmaps_window_table(int ncal) {
    CoilmapsWindow<R> t;
    for (int i = 0; i < COILMIX_NCAL_MAX; ++i) t.w[i] = i < ncal ? (R)coilmaps_window(i, ncal) : R(0);
    return t;
}
// line h of an axis of length n -> its calibration line 0 .. ncal - 1, or -1 outside the region (the inverse of coilmix_cal_line)
COIL_HD inline int coilmaps_line_of(int h, int ncal, int n) {
    if (h < (ncal + 1) / 2) return h;
    if (h >= n - ncal / 2) return h - (n - ncal);
    return -1;
}
// one windowed point: the weights multiplied first
template <typename R> COIL_HD inline void coilmaps_apply_window(R wh, R ww, R yr, R yi, R& kr, R& ki) {
    const R w = wh * ww;
    kr = w * yr;
    ki = w * yi;
}

// ---- patch ------------------------------------------------------------------------------------------------------------------------
COIL_HD inline int coilmaps_patch_points(int r) { return (2 * r + 1) * (2 * r + 1); }
COIL_HD inline int coilmaps_wrap(int v, int n) { v %= n; return v < 0 ? v + n : v; }
// patch point q = 0 .. (2r + 1)^2 - 1 of pixel (y, x): row-major offsets (dy, dx) = (-r, -r) .. (r, r), wrapped
COIL_HD inline void coilmaps_patch_offset(int q, int r, int& dy, int& dx) { dy = q / (2 * r + 1) - r; dx = q % (2 * r + 1) - r; }
COIL_HD inline size_t coilmaps_patch_index(int q, int r, int y, int x, int H, int W) {
    int dy, dx;
    coilmaps_patch_offset(q, r, dy, dx);
    return (size_t)coilmaps_wrap(y + dy, H) * W + coilmaps_wrap(x + dx, W);
}

// ---- arithmetic of one pixel --------------------------------------------------------------------------------------------------------
// (re, im) += conj(a) x
template <typename R> COIL_HD inline void coilmaps_cmac_conj(R& re, R& im, R ar, R ai, R xr, R xi) {
    re = coilmix_fma(ar, xr, re);
    re = coilmix_fma(ai, xi, re);
    im = coilmix_fma(ar, xi, im);
    im = coilmix_fma(-ai, xr, im);
}
template <typename R> COIL_HD inline R coilmaps_sqrt(R v);
template <> COIL_HD inline float coilmaps_sqrt<float>(float v) { return sqrtf(v); }
template <> COIL_HD inline double coilmaps_sqrt<double>(double v) { return sqrt(v); }
// s += |a|^2, re before im
template <typename R> COIL_HD inline void coilmaps_norm2_step(R& s, R ar, R ai) {
    s = coilmix_fma(ar, ar, s);
    s = coilmix_fma(ai, ai, s);
}
// the phase factor e = g / |g| of the phase step; false when g = 0
template <typename R> COIL_HD inline bool coilmaps_phase_factor(R gr, R gi, R& er, R& ei) {
    const R m = coilmaps_sqrt<R>(coilmix_fma(gr, gr, gi * gi));
    if (!(m > R(0))) return false;
    er = gr / m;
    ei = gi / m;
    return true;
}
// v <- v e
template <typename R> COIL_HD inline void coilmaps_rotate(R& vr, R& vi, R er, R ei) {
    const R re = coilmix_fma(-vi, ei, vr * er), im = coilmix_fma(vi, er, vr * ei);
    vr = re;
    vi = im;
}

// The steps on interleaved arrays of C complex values, as the kernel runs them on its registers.  img: the coil images of ONE slice,
// [C][H][W] interleaved; at(c, o): coil c at pixel offset o.
template <typename R> inline void coilmaps_start(const R* img, int C, size_t N, size_t p, R* v) {
    R s = R(0);
    for (int c = 0; c < C; ++c) coilmaps_norm2_step(s, img[2 * (c * N + p)], img[2 * (c * N + p) + 1]);
    const R nrm = coilmaps_sqrt<R>(s);
    for (int c = 0; c < C; ++c) {
        if (nrm > R(0)) { v[2 * c] = img[2 * (c * N + p)] / nrm; v[2 * c + 1] = img[2 * (c * N + p) + 1] / nrm; }
        else            { v[2 * c] = c == 0 ? R(1) : R(0); v[2 * c + 1] = R(0); }
    }
}
// one power step at pixel (y, x): v <- R(p) v / ||R(p) v||; -> lambda = ||R(p) v||.  u: scratch of 2 C values
template <typename R> inline R coilmaps_power_step(const R* img, int C, int H, int W, int r, int y, int x, R* v, R* u) {
    const size_t N = (size_t)H * W;
    for (int c = 0; c < 2 * C; ++c) u[c] = R(0);
    for (int q = 0; q < coilmaps_patch_points(r); ++q) {
        const size_t o = coilmaps_patch_index(q, r, y, x, H, W);
        R gr = R(0), gi = R(0);
        for (int c = 0; c < C; ++c) coilmaps_cmac_conj(gr, gi, img[2 * (c * N + o)], img[2 * (c * N + o) + 1], v[2 * c], v[2 * c + 1]);
        for (int c = 0; c < C; ++c) coilmix_cmac(u[2 * c], u[2 * c + 1], img[2 * (c * N + o)], img[2 * (c * N + o) + 1], gr, gi);
    }
    R s = R(0);
    for (int c = 0; c < C; ++c) coilmaps_norm2_step(s, u[2 * c], u[2 * c + 1]);
    const R lam = coilmaps_sqrt<R>(s);
    if (lam > R(0))
        for (int c = 0; c < 2 * C; ++c) v[c] = u[c] / lam;
    return lam;
}
template <typename R> inline void coilmaps_phase_step(const R* img, int C, size_t N, size_t p, R* v) {
    R gr = R(0), gi = R(0);
    for (int c = 0; c < C; ++c) coilmaps_cmac_conj(gr, gi, v[2 * c], v[2 * c + 1], img[2 * (c * N + p)], img[2 * (c * N + p) + 1]);
    R er, ei;
    if (!coilmaps_phase_factor(gr, gi, er, ei)) return;
    for (int c = 0; c < C; ++c) coilmaps_rotate(v[2 * c], v[2 * c + 1], er, ei);
}

// ---- the windowed calibration region of one slice: k [C][H][W] interleaved, +0 outside the region.  -> -1, or the lowest offset h * W + k
// of a calibration point that the mask does not sample (the region is written all the same)
template <typename R>
inline long coilmaps_window_slice(const R* y, const uint8_t* mask, int C, int H, int W, int ncal, R* k) {
    const size_t N = (size_t)H * W;
    const CoilmapsWindow<R> win = coilmaps_window_table<R>(ncal);
    long miss = -1;
    for (int c = 0; c < C; ++c)
        for (int h = 0; h < H; ++h)
            for (int x = 0; x < W; ++x) {
                const size_t o = (size_t)h * W + x;
                const int i = coilmaps_line_of(h, ncal, H), j = coilmaps_line_of(x, ncal, W);
                R kr = R(0), ki = R(0);
                if (i >= 0 && j >= 0) {
                    coilmaps_apply_window(win.w[i], win.w[j], y[2 * (c * N + o)], y[2 * (c * N + o) + 1], kr, ki);
                    if (!mask[o] && (miss < 0 || (long)o < miss)) miss = (long)o;
                }
                k[2 * (c * N + o)] = kr;
                k[2 * (c * N + o) + 1] = ki;
            }
    return miss;
}

// ---- the eigenvector and support steps of one slice as the kernels run them: img [C][H][W] low-resolution coil images ->
// maps [C][H][W] (masked by the support), lambda [H][W]
template <typename R>
inline void coilmaps_slice(const R* img, int C, int H, int W, int r, int iters, double thresh, R* maps, R* lambda) {
    const size_t N = (size_t)H * W;
    R v[2 * COIL_MAX_C], u[2 * COIL_MAX_C];
    R lmax = R(0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            coilmaps_start(img, C, N, p, v);
            R lam = R(0);
            for (int it = 0; it < iters; ++it) lam = coilmaps_power_step(img, C, H, W, r, y, x, v, u);
            coilmaps_phase_step(img, C, N, p, v);
            for (int c = 0; c < C; ++c) { maps[2 * (c * N + p)] = v[2 * c]; maps[2 * (c * N + p) + 1] = v[2 * c + 1]; }
            lambda[p] = lam;
            if (lam > lmax) lmax = lam;
        }
    const R bar = (R)(thresh * thresh) * lmax;
    for (size_t p = 0; p < N; ++p)
        if (!(lambda[p] >= bar))
            for (int c = 0; c < C; ++c) { maps[2 * (c * N + p)] = R(0); maps[2 * (c * N + p) + 1] = R(0); }
}

// ---- tiles of k_coil_eigmaps ----------------------------------------------------------------------------------------------------------
// A workgroup owns th x tw pixels (one thread each) and stages (th + 2r) x (tw + 2r) pixels x CB coils in LDS as [pixel][coil], CB =
// coilmix_out_bucket(C).  A pixel's coils take `stride` 16-byte slots: the CB complex values rounded up to an ODD number of slots, so that
// the 16 lanes of a 16-byte LDS read, which sit at consecutive pixels, start in 16 different slots of the 256-byte bank row.
struct CoilmapsTile { int th, tw; };
constexpr int COILMAPS_TILES = 4;
COIL_HD inline CoilmapsTile coilmaps_tile_at(int k) {
    return k == 0 ? CoilmapsTile{16, 16} : k == 1 ? CoilmapsTile{8, 16} : k == 2 ? CoilmapsTile{8, 8} : CoilmapsTile{4, 8};
}
COIL_HD constexpr size_t coilmaps_cx_bytes(bool f64) { return f64 ? 16 : 8; }
// the footprint the tile rule goes by: staged pixels x CB complex values, without the padding
COIL_HD inline size_t coilmaps_footprint(CoilmapsTile t, int r, int CB, bool f64) {
    return (size_t)(t.th + 2 * r) * (t.tw + 2 * r) * CB * coilmaps_cx_bytes(f64);
}
COIL_HD inline int coilmaps_tile_choice(int C, int r, bool f64) {
    const int CB = coilmix_out_bucket(C);
    for (int k = 0; k < COILMAPS_TILES; ++k)
        if (coilmaps_footprint(coilmaps_tile_at(k), r, CB, f64) <= COILMAPS_LDS_SOFT) return k;
    return COILMAPS_TILES - 1;
}
COIL_HD constexpr int coilmaps_stride_slots(int CB, bool f64) { return (int)((size_t)CB * coilmaps_cx_bytes(f64) / 16) | 1; }
// what the launch asks for: the padded image
COIL_HD inline size_t coilmaps_lds_bytes(CoilmapsTile t, int r, int CB, bool f64) {
    return (size_t)(t.th + 2 * r) * (t.tw + 2 * r) * coilmaps_stride_slots(CB, f64) * 16;
}
COIL_HD inline int coilmaps_tiles_y(int H, CoilmapsTile t) { return (H + t.th - 1) / t.th; }
COIL_HD inline int coilmaps_tiles_x(int W, CoilmapsTile t) { return (W + t.tw - 1) / t.tw; }
// staged pixel (sy, sx) of the tile whose first pixel is (y0, x0) -> the image pixel it holds
COIL_HD inline size_t coilmaps_staged_pixel(int sy, int sx, int y0, int x0, int r, int H, int W) {
    return (size_t)coilmaps_wrap(y0 - r + sy, H) * W + coilmaps_wrap(x0 - r + sx, W);
}

// ---- support ----------------------------------------------------------------------------------------------------------------------
COIL_HD inline int coilmaps_spans(size_t N) { return (int)((N + COILMAPS_SPAN - 1) / COILMAPS_SPAN); }

// ---- scratch of pnp_coil_maps -----------------------------------------------------------------------------------------------------
// slices per pass: as many as fit min(B C, Bmax) pseudo-slices, at least one
COIL_HD inline int coilmaps_pass_slices(int B, int C, int Bmax) {
    const int nb = Bmax / C;
    return nb < 1 ? 1 : nb > B ? B : nb;
}
struct CoilmapsScratch { size_t img, lambda, part, miss, bytes; };          // byte offsets of the four arrays, and the total
COIL_HD inline size_t coilmaps_align(size_t v) { return (v + 255) / 256 * 256; }
COIL_HD inline CoilmapsScratch coilmaps_scratch(int B, int C, int Bmax, size_t N, bool f64) {
    const size_t nb = (size_t)coilmaps_pass_slices(B, C, Bmax), real = f64 ? 8 : 4;
    CoilmapsScratch s;
    s.img = 0;
    s.lambda = coilmaps_align(nb * C * N * 2 * real);
    s.part = s.lambda + coilmaps_align(nb * N * real);
    s.miss = s.part + coilmaps_align(nb * (size_t)coilmaps_spans(N) * real);
    s.bytes = s.miss + coilmaps_align((size_t)B * sizeof(int32_t));
    return s;
}

}  // namespace pnp
