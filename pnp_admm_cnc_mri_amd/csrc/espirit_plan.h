// ESPIRiT coil sensitivity maps: calibration kernels wider than one pixel (pnp_espirit_maps; kernels_espirit.hip).  Pure host-callable code
// without HIP: the argument rule, the calibration block and its index maps, the order of the patch Gram sums, the host stage (signal space
// and kernel autocorrelation, double, through coilmix_jacobi), the arithmetic of one pixel as templates on the real type, the tile and
// scratch layouts, and espirit_slice, the whole-slice restatement the kernels follow operation by operation.  The kernels run by it and
// tests/host/espirit_emulation.cpp checks it under g++.  Every unit is built with -ffp-contract=off: a fused multiply-add is where
// coilmix_fma is written and nowhere else.
//
// One slice, y [C][H][W] un-shifted (DC at (0, 0)), kernel side k, real type R:
//   block    K [C][ncal][ncal]: the calibration region of coilmix_plan.h in ASCENDING signed frequency on both axes: entry t of an axis is
//            calibration line (t + ncal - ncal / 2) % ncal (a roll by ncal / 2).  NOT windowed.
//   Gram     the (ncal - k + 1)^2 patch positions (i, j), not wrapped; row (i, j) of the calibration matrix A holds K[c][i + a][j + b] at
//            column m = (c k + a) k + b (c slowest), n = C k^2 columns.  G[m][m'] = sum_(i, j) conj(A[(i, j)][m]) A[(i, j)][m'] for m <= m':
//            ONE chain of coilmix_gram_step(re, im, A[..][m'], A[..][m]) per pair over the positions in row-major order (products and sums
//            in double for both input precisions); G[m'][m] is the conjugate of that to the bit, the diagonal's imaginary part is +0.  The
//            order depends on (ncal, k) alone.  espirit_gram_slice restates it; k_calib_patch_gram does exactly this, one thread per pair.
//   space    (host, double) eigenvalues e_j of G descending by coilmix_jacobi, s_j = sqrt(max(e_j, 0)); the rank is the number of
//            s_j >= sigma s_0; P = V V^H over those columns, upper triangle summed j ascending, the lower its conjugate, diagonal real.
//   kernels  (host, double) w_cc'(d) = (1 / k^2) sum conj(P)[(c, a), (c', a - d)] over the a = (ay, ax) in row-major order for which a - d
//            is inside the kernel, d in [-(k - 1), k - 1]^2, for c <= c'; w_c'c(-d) = conj(w_cc'(d)) for c < c'.  Stored [C][C][D][D], D =
//            2 k - 1, entry (dy + k - 1, dx + k - 1).  Rounded once to R where the per-pixel stage takes it.
//   phasors  E_n(q, d) = exp(+2 pi i ((q d) mod n) / n), the angle formed in double from the reduced integer, cos and sin rounded once to R:
//            tables E_H [H][D], E_W [W][D] (espirit_phasor), an argument of the per-pixel kernel.
//   pixel q  G_cc'(q) = sum_dy E_H(q_y, dy) [sum_dx w_cc'(dy, dx) E_W(q_x, dx)] for c <= c': the inner chain over dx ascending is
//            coilmix_cmac(inner, w, E_W), the outer over dy ascending coilmix_cmac(acc, E_H, inner) (espirit_g_entry).  G_c'c = conj(G_cc'),
//            the diagonal's imaginary part is +0.  Start v = I(q) / ||I(q)|| (coilmaps_norm2_step chain; e_0 when the norm is 0); n times:
//            u_c = sum_c' G_cc' v_c' (c' ascending, coilmix_cmac), lambda = sqrt(norm2(u)), v = u / lambda unless lambda = 0; then
//            coilmaps_phase_step: v^H I(q) >= 0.  I: the windowed low-resolution images of coilmaps_plan.h.
//   support  S(q) = v(q) where lambda(q) >= (R)crop AND ||I(q)|| >= (R)thresh * max_q ||I(q)||; elsewhere +0 in every coil.
// No sum depends on B, on the tile, or on the pixel's place in it: a slice alone and the slice in a batch are bit-equal.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "coilmaps_plan.h"

namespace pnp {

constexpr int ESPIRIT_MIN_KERNEL = 2;
constexpr int ESPIRIT_MAX_KERNEL = 8;
constexpr int ESPIRIT_MAX_N = COILMIX_MAX_IN;       // C k^2 <= 128: the documented size of the host Jacobi
constexpr int ESPIRIT_MAX_ITERS = COILMAPS_MAX_ITERS;
constexpr int ESPIRIT_TILE = COILMIX_TILE;          // k_calib_patch_gram: a workgroup owns a 16 x 16 tile of pairs (m, m'), one thread each
constexpr size_t ESPIRIT_GRAM_LDS = 48 * 1024;      // ... and stages rows of K of the coils its tile touches, complex double, within this
constexpr int ESPIRIT_HOST_THREADS = 16;            // the host stage of a pass runs on at most this many threads, whatever the machine has

enum { ESPIRIT_OK = 0, ESPIRIT_BAD_C = 1, ESPIRIT_BAD_SHAPE = 2, ESPIRIT_BAD_NCAL = 3, ESPIRIT_BAD_KERNEL = 4, ESPIRIT_KERNEL_OVER_NCAL = 5,
       ESPIRIT_BAD_SIZE = 6, ESPIRIT_BAD_ITERS = 7, ESPIRIT_BAD_SIGMA = 8, ESPIRIT_BAD_CROP = 9, ESPIRIT_BAD_THRESH = 10 };
COIL_HD inline int espirit_check(int C, int ncal, int k, int power_iters, double sigma, double crop, double thresh, int H, int W) {
    if (C < 1 || C > COIL_MAX_C) return ESPIRIT_BAD_C;
    if (H < 128 || H > 1024 || W < 128 || W > 1024) return ESPIRIT_BAD_SHAPE;
    if (coilmix_check(C, 1, 1, ncal, H, W) == COILMIX_BAD_NCAL) return ESPIRIT_BAD_NCAL;
    if (k < ESPIRIT_MIN_KERNEL || k > ESPIRIT_MAX_KERNEL) return ESPIRIT_BAD_KERNEL;
    if (k > ncal) return ESPIRIT_KERNEL_OVER_NCAL;
    if (C * k * k > ESPIRIT_MAX_N) return ESPIRIT_BAD_SIZE;
    if (power_iters < 1 || power_iters > ESPIRIT_MAX_ITERS) return ESPIRIT_BAD_ITERS;
    if (!(sigma > 0.0) || !(sigma < 1.0)) return ESPIRIT_BAD_SIGMA;
    if (!(crop >= 0.0) || !(crop <= 1.0)) return ESPIRIT_BAD_CROP;
    if (!(thresh >= 0.0) || !(thresh < 1.0)) return ESPIRIT_BAD_THRESH;
    return ESPIRIT_OK;
}

// ---- calibration block and matrix ------------------------------------------------------------------------------------------------------
COIL_HD inline int espirit_block_line(int t, int ncal) { return (t + ncal - ncal / 2) % ncal; }          // entry t -> calibration line
COIL_HD inline size_t espirit_block_index(int t, int u, int ncal, int H, int W) {
    return (size_t)coilmix_cal_line(espirit_block_line(t, ncal), ncal, H) * W + coilmix_cal_line(espirit_block_line(u, ncal), ncal, W);
}
COIL_HD inline int espirit_positions(int ncal, int k) { return ncal - k + 1; }          // patch positions per axis
COIL_HD inline int espirit_columns(int C, int k) { return C * k * k; }
COIL_HD inline void espirit_column(int m, int k, int& c, int& a, int& b) { c = m / (k * k); a = m / k % k; b = m % k; }
COIL_HD inline int espirit_side(int k) { return 2 * k - 1; }          // D: offsets per axis of the kernel autocorrelation

// tiles of pairs: coilmix_tile_of over n = C k^2.  The coils a tile's 16 consecutive columns touch: c0 .. c0 + count - 1
COIL_HD inline void espirit_tile_coils(int tile, int n, int k, int& c0, int& count) {
    const int lo = tile * ESPIRIT_TILE, hi = lo + ESPIRIT_TILE - 1 < n - 1 ? lo + ESPIRIT_TILE - 1 : n - 1;
    c0 = lo / (k * k);
    count = hi / (k * k) - c0 + 1;
}
// rows of K per staged coil that fit ESPIRIT_GRAM_LDS with `coils` coils staged (both sides of the tile); at least k for every valid size
COIL_HD inline int espirit_stage_rows(int ncal, int coils) { return (int)(ESPIRIT_GRAM_LDS / (16 * (size_t)ncal * coils)); }

// the patch Gram matrix of one slice as k_calib_patch_gram forms it: y [C][H][W] interleaved complex, gram [n][n] interleaved complex
// double.  mask [H][W] or null: a calibration point it does not sample enters as +0 (pnp_espirit_maps refuses such a mask)
template <typename R>
inline void espirit_gram_slice(const R* y, const uint8_t* mask, int C, int H, int W, int ncal, int k, double* gram) {
    const size_t N = (size_t)H * W;
    const int n = espirit_columns(C, k), P = espirit_positions(ncal, k);
    auto K = [&](int c, int t, int u, double& re, double& im) {
        const size_t at = espirit_block_index(t, u, ncal, H, W);
        const bool on = !mask || mask[at];
        re = on ? (double)y[2 * (c * N + at)] : 0.0;
        im = on ? (double)y[2 * (c * N + at) + 1] : 0.0;
    };
    for (int m = 0; m < n; ++m)
        for (int m2 = m; m2 < n; ++m2) {
            int c, a, b, c2, a2, b2;
            espirit_column(m, k, c, a, b);
            espirit_column(m2, k, c2, a2, b2);
            double re = 0.0, im = 0.0;
            for (int i = 0; i < P; ++i)
                for (int j = 0; j < P; ++j) {
                    double xr, xi, yr, yi;
                    K(c, i + a, j + b, xr, xi);
                    K(c2, i + a2, j + b2, yr, yi);
                    coilmix_gram_step(re, im, yr, yi, xr, xi);
                }
            if (m == m2) im = 0.0;
            gram[2 * ((size_t)m * n + m2)] = re;
            gram[2 * ((size_t)m * n + m2) + 1] = im;
            if (m != m2) {
                gram[2 * ((size_t)m2 * n + m)] = re;
                gram[2 * ((size_t)m2 * n + m) + 1] = -im;
            }
        }
}

// ---- host stage: signal space and kernel autocorrelation (double) -------------------------------------------------------------------------
COIL_HD inline size_t espirit_w_index(int c, int c2, int dy, int dx, int C, int k) {
    const int D = espirit_side(k);
    return (((size_t)c * C + c2) * D + (dy + k - 1)) * D + (dx + k - 1);
}
COIL_HD inline size_t espirit_w_count(int C, int k) { return (size_t)C * C * espirit_side(k) * espirit_side(k); }
COIL_HD inline size_t espirit_work_doubles(int n) { return 6 * (size_t)n * n + (size_t)n; }
// gram [n][n] -> w [C][C][D][D] complex double, sing [n] descending, rank.  work: espirit_work_doubles(n).  -> coilmix_jacobi's code
inline int espirit_kernels(const double* gram, int C, int k, double sigma, double* w, int* rank_out, double* sing, double* work) {
    const int n = espirit_columns(C, k), kk = k * k;
    double* vec = work + 2 * (size_t)n * n;          // work[0 .. 2 n n): Jacobi's own
    double* P = work + 4 * (size_t)n * n;
    double* eig = work + 6 * (size_t)n * n;
    if (int rc = coilmix_jacobi(gram, n, eig, vec, work)) return rc;
    for (int j = 0; j < n; ++j) sing[j] = sqrt(eig[j] > 0.0 ? eig[j] : 0.0);
    int rank = 0;
    while (rank < n && sing[rank] >= sigma * sing[0]) ++rank;
    *rank_out = rank;
    for (int m = 0; m < n; ++m)
        for (int m2 = m; m2 < n; ++m2) {          // P[m][m2] = sum_j V[m][j] conj(V[m2][j])
            double re = 0.0, im = 0.0;
            for (int j = 0; j < rank; ++j)
                coilmix_gram_step(re, im, vec[2 * ((size_t)m * n + j)], vec[2 * ((size_t)m * n + j) + 1], vec[2 * ((size_t)m2 * n + j)],
                                  vec[2 * ((size_t)m2 * n + j) + 1]);
            if (m == m2) im = 0.0;
            P[2 * ((size_t)m * n + m2)] = re; P[2 * ((size_t)m * n + m2) + 1] = im;
            P[2 * ((size_t)m2 * n + m)] = re; P[2 * ((size_t)m2 * n + m) + 1] = m == m2 ? 0.0 : -im;
        }
    for (int c = 0; c < C; ++c)
        for (int c2 = c; c2 < C; ++c2)
            for (int dy = -(k - 1); dy <= k - 1; ++dy)
                for (int dx = -(k - 1); dx <= k - 1; ++dx) {
                    double re = 0.0, im = 0.0;
                    for (int ay = 0; ay < k; ++ay)
                        for (int ax = 0; ax < k; ++ax) {
                            const int by = ay - dy, bx = ax - dx;
                            if (by < 0 || by >= k || bx < 0 || bx >= k) continue;
                            const size_t at = (size_t)(c * kk + ay * k + ax) * n + (c2 * kk + by * k + bx);
                            re = re + P[2 * at];
                            im = im - P[2 * at + 1];          // conj(P)
                        }
                    re = re / (double)kk;
                    im = im / (double)kk;
                    w[2 * espirit_w_index(c, c2, dy, dx, C, k)] = re;
                    w[2 * espirit_w_index(c, c2, dy, dx, C, k) + 1] = im;
                    if (c != c2) {
                        w[2 * espirit_w_index(c2, c, -dy, -dx, C, k)] = re;
                        w[2 * espirit_w_index(c2, c, -dy, -dx, C, k) + 1] = -im;
                    }
                }
    return 0;
}

// ---- phasor tables -------------------------------------------------------------------------------------------------------------------------
// E_n(q, d), d = -(k - 1) .. k - 1: table [n][D] interleaved complex in R
template <typename R> inline void espirit_phasor(int q, int d, int n, R& re, R& im) {
    long t = ((long)q * d) % n;
    if (t < 0) t += n;
    const double ang = 2.0 * 3.14159265358979323846 * (double)t / (double)n;
    re = (R)cos(ang);
    im = (R)sin(ang);
}
template <typename R> inline void espirit_phasor_table(int n, int k, R* table) {
    const int D = espirit_side(k);
    for (int q = 0; q < n; ++q)
        for (int d = 0; d < D; ++d) espirit_phasor<R>(q, d - (k - 1), n, table[2 * ((size_t)q * D + d)], table[2 * ((size_t)q * D + d) + 1]);
}

// ---- arithmetic of one pixel ---------------------------------------------------------------------------------------------------------------
// index of the pair c <= c2 in the packed upper triangle the kernel stages
COIL_HD inline int espirit_pair(int c, int c2, int C) { return c * C - c * (c - 1) / 2 + (c2 - c); }
COIL_HD inline int espirit_pairs(int C) { return C * (C + 1) / 2; }
// G_cc2 of one pixel, c <= c2: wp = w[c][c2] as [D][D] interleaved, eh / ew = the pixel's rows of the phasor tables (stride in complex values)
template <typename R>
COIL_HD inline void espirit_g_entry(const R* wp, const R* eh, size_t eh_stride, const R* ew, size_t ew_stride, int D, R& gr, R& gi) {
    gr = R(0); gi = R(0);
    for (int dy = 0; dy < D; ++dy) {
        R ir = R(0), ii = R(0);
        for (int dx = 0; dx < D; ++dx)
            coilmix_cmac(ir, ii, wp[2 * (dy * D + dx)], wp[2 * (dy * D + dx) + 1], ew[2 * dx * ew_stride], ew[2 * dx * ew_stride + 1]);
        coilmix_cmac(gr, gi, eh[2 * dy * eh_stride], eh[2 * dy * eh_stride + 1], ir, ii);
    }
}
// the entry of row c, column c2 from the upper triangle's: conjugated below the diagonal, real on it
template <typename R> COIL_HD inline void espirit_g_place(int c, int c2, R& gr, R& gi) {
    if (c2 < c) gi = -gi;
    else if (c2 == c) gi = R(0);
}

// one pixel as the kernel runs it: img [C][N] at offset p, w [C][C][D][D] in R, eh [D], ew [D] -> v [2 C]; -> lambda; inorm = ||I(p)||
template <typename R>
inline R espirit_pixel(const R* img, int C, size_t N, size_t p, const R* w, int k, int iters, const R* eh, const R* ew, R* v, R& inorm) {
    const int D = espirit_side(k);
    R u[2 * COIL_MAX_C];
    R s = R(0);
    for (int c = 0; c < C; ++c) coilmaps_norm2_step(s, img[2 * (c * N + p)], img[2 * (c * N + p) + 1]);
    inorm = coilmaps_sqrt<R>(s);
    coilmaps_start(img, C, N, p, v);
    R lam = R(0);
    for (int it = 0; it < iters; ++it) {
        for (int c = 0; c < C; ++c) {
            R ur = R(0), ui = R(0);
            for (int c2 = 0; c2 < C; ++c2) {
                const int lo = c < c2 ? c : c2, hi = c < c2 ? c2 : c;
                R gr, gi;
                espirit_g_entry(w + 2 * espirit_w_index(lo, hi, -(k - 1), -(k - 1), C, k), eh, 1, ew, 1, D, gr, gi);
                espirit_g_place(c, c2, gr, gi);
                coilmix_cmac(ur, ui, gr, gi, v[2 * c2], v[2 * c2 + 1]);
            }
            u[2 * c] = ur; u[2 * c + 1] = ui;
        }
        s = R(0);
        for (int c = 0; c < C; ++c) coilmaps_norm2_step(s, u[2 * c], u[2 * c + 1]);
        lam = coilmaps_sqrt<R>(s);
        if (lam > R(0))
            for (int c = 0; c < 2 * C; ++c) v[c] = u[c] / lam;
    }
    coilmaps_phase_step(img, C, N, p, v);
    return lam;
}

// the per-pixel and support stages of one slice: img [C][H][W], w in R -> maps [C][H][W] (masked), lambda [H][W]
template <typename R>
inline void espirit_slice(const R* img, int C, int H, int W, const R* w, int k, int iters, double crop, double thresh, R* maps, R* lambda) {
    const size_t N = (size_t)H * W;
    const int D = espirit_side(k);
    R* eh = new R[2 * (size_t)H * D];
    R* ew = new R[2 * (size_t)W * D];
    R* inorm = new R[N];
    espirit_phasor_table<R>(H, k, eh);
    espirit_phasor_table<R>(W, k, ew);
    R v[2 * COIL_MAX_C];
    R imax = R(0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            lambda[p] = espirit_pixel(img, C, N, p, w, k, iters, eh + 2 * (size_t)y * D, ew + 2 * (size_t)x * D, v, inorm[p]);
            for (int c = 0; c < C; ++c) { maps[2 * (c * N + p)] = v[2 * c]; maps[2 * (c * N + p) + 1] = v[2 * c + 1]; }
            if (inorm[p] > imax) imax = inorm[p];
        }
    const R bar = (R)thresh * imax, cr = (R)crop;
    for (size_t p = 0; p < N; ++p)
        if (!(lambda[p] >= cr && inorm[p] >= bar))
            for (int c = 0; c < C; ++c) { maps[2 * (c * N + p)] = R(0); maps[2 * (c * N + p) + 1] = R(0); }
    delete[] eh; delete[] ew; delete[] inorm;
}

// ---- tiles of k_espirit_maps ---------------------------------------------------------------------------------------------------------------
// A workgroup owns th x tw pixels (one thread each).  Its LDS image: a slab of CB complex values per thread for v at coilmaps_stride_slots
// (an ODD number of 16-byte slots: the lanes of a read sit in different slots of the bank row), then the packed upper triangle of w, the
// tile's th rows of E_H as [row][d] and its tw columns of E_W as [d][column].
struct EspiritLds { size_t slab, w, eh, ew, bytes; };          // byte offsets, and the total
COIL_HD inline EspiritLds espirit_lds(CoilmapsTile t, int C, int k, bool f64) {
    const size_t cx = coilmaps_cx_bytes(f64), D = (size_t)espirit_side(k);
    EspiritLds l;
    l.slab = 0;
    l.w = (size_t)t.th * t.tw * coilmaps_stride_slots(coilmix_out_bucket(C), f64) * 16;
    l.eh = l.w + (size_t)espirit_pairs(C) * D * D * cx;
    l.ew = l.eh + (size_t)t.th * D * cx;
    l.bytes = l.ew + (size_t)t.tw * D * cx;
    return l;
}
// the largest tile of coilmaps_tile_at within COILMAPS_LDS_SOFT, else the largest within COILMAPS_LDS_HARD (one exists for every valid size)
COIL_HD inline int espirit_tile_choice(int C, int k, bool f64) {
    for (int j = 0; j < COILMAPS_TILES; ++j)
        if (espirit_lds(coilmaps_tile_at(j), C, k, f64).bytes <= COILMAPS_LDS_SOFT) return j;
    for (int j = 0; j < COILMAPS_TILES; ++j)
        if (espirit_lds(coilmaps_tile_at(j), C, k, f64).bytes <= COILMAPS_LDS_HARD) return j;
    return COILMAPS_TILES - 1;
}

// ---- scratch of pnp_espirit_maps / pnp_espirit_eigmaps: one array on the context --------------------------------------------------------------
struct EspiritScratch { size_t img, lambda, inorm, part, miss, gram, w, eh, ew, bytes; };
// nb: slices per pass (coilmaps_pass_slices); pipeline: with the images, Gram matrices and missing points of pnp_espirit_maps
COIL_HD inline EspiritScratch espirit_scratch(int B, int nb, int C, int k, int H, int W, bool f64, bool pipeline) {
    const size_t N = (size_t)H * W, real = f64 ? 8 : 4, n = (size_t)espirit_columns(C, k), D = (size_t)espirit_side(k);
    EspiritScratch s;
    s.img = 0;
    s.lambda = pipeline ? coilmaps_align((size_t)nb * C * N * 2 * real) : 0;
    s.inorm = s.lambda + coilmaps_align((size_t)nb * N * real);
    s.part = s.inorm + coilmaps_align((size_t)nb * N * real);
    s.miss = s.part + coilmaps_align((size_t)nb * coilmaps_spans(N) * real);
    s.gram = s.miss + coilmaps_align((size_t)B * sizeof(int32_t));
    s.w = s.gram + (pipeline ? coilmaps_align((size_t)nb * n * n * 16) : 0);
    s.eh = s.w + coilmaps_align((size_t)nb * espirit_w_count(C, k) * 2 * real);
    s.ew = s.eh + coilmaps_align((size_t)H * D * 2 * real);
    s.bytes = s.ew + coilmaps_align((size_t)W * D * 2 * real);
    return s;
}

}  // namespace pnp
