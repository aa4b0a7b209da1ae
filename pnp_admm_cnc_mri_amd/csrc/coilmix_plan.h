// Coil mixing ahead of the multi-coil solve (pnp_coil_mix, pnp_coil_gram, pnp_coilmix_whiten, pnp_coilmix_compress; kernels_coilmix.hip):
// noise prewhitening and SVD coil compression are ONE operation, a C_out x C_in complex matrix applied per k-space point to the
// measurements and per pixel to the maps.  Pure host-callable code without HIP: the argument rule, the calibration region and its index
// map, the order of the Gram sums, the arithmetic of one mixing step, and the two small host solvers (inverse Cholesky factor, cyclic
// Jacobi) in double with no dependency.  The kernels run by it and tests/host/coilmix_emulation.cpp checks it under g++.
//
// Calibration region (k-space un-shifted, DC at (0, 0)): the rows 0 .. ceil(ncal / 2) - 1 and H - floor(ncal / 2) .. H - 1, the columns
// by the same rule with W; point q = 0 .. ncal^2 - 1 is (cal_line(q / ncal, ncal, H), cal_line(q % ncal, ncal, W)).
// Gram sums: R[i][j] = sum_q mask(q) y_i(q) conj(y_j(q)) for i <= j, the points in the order q = 0, 1, .. ncal^2 - 1 by ONE chain of
// coilmix_gram_step per pair (products and sums in double, every product and sum rounded once, points with mask 0 skipped); R[j][i] is
// the conjugate of that, the diagonal's imaginary part is set to 0.  The order is a function of (ncal, H, W) alone: never of B, of the
// slice's position in the batch, or of C.  coilmix_gram_slice restates it; k_coil_gram does exactly this, one thread per pair.
// Mixing: out_j = sum_c M[j][c] in_c, the coils in order c = 0 .. C_in - 1 by coilmix_cmac (four fused multiply-adds per coil).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "coil_plan.h"

namespace pnp {

constexpr int COILMIX_MAX_IN = 128;       // physical channels: 1 <= C_in <= COILMIX_MAX_IN; 1 <= C_out <= min(C_in, COIL_MAX_C)
constexpr int COILMIX_NCAL_MIN = 4;       // side of the calibration square, COILMIX_NCAL_MIN <= ncal <= min(COILMIX_NCAL_MAX, H, W)
constexpr int COILMIX_NCAL_MAX = 64;
constexpr int COILMIX_MIX_THREADS = 256;  // k_coil_mix: a thread owns coilmix_points(f64) consecutive points and all C_out sums
constexpr int COILMIX_MIX_CHUNK = 32;     // columns of M staged in LDS at a time
constexpr int COILMIX_TILE = 16;          // k_coil_gram: a workgroup owns a COILMIX_TILE x COILMIX_TILE tile of pairs (i, j), thread (ti, tj)
constexpr int COILMIX_GRAM_POINTS = 64;   // calibration points staged in LDS at a time (x 2 COILMIX_TILE coils, complex double: 32 KiB)
constexpr int COILMIX_JACOBI_SWEEPS = 60;

enum { COILMIX_OK = 0, COILMIX_BAD_IN = 1, COILMIX_BAD_OUT = 2, COILMIX_BAD_SETS = 3, COILMIX_BAD_NCAL = 4, COILMIX_BAD_SHAPE = 5 };
COIL_HD inline int coilmix_check(int C_in, int C_out, int Ks, int ncal, int H, int W) {
    if (C_in < 1 || C_in > COILMIX_MAX_IN) return COILMIX_BAD_IN;
    if (C_out < 1 || C_out > C_in || C_out > COIL_MAX_C) return COILMIX_BAD_OUT;
    if (Ks < 1) return COILMIX_BAD_SETS;
    if (H < 128 || H > 1024 || W < 128 || W > 1024) return COILMIX_BAD_SHAPE;
    if (ncal < COILMIX_NCAL_MIN || ncal > COILMIX_NCAL_MAX || ncal > H || ncal > W) return COILMIX_BAD_NCAL;
    return COILMIX_OK;
}

// ---- calibration region --------------------------------------------------------------------------------------------------------
// line i = 0 .. ncal - 1 of the region along an axis of length n
COIL_HD inline int coilmix_cal_line(int i, int ncal, int n) { return i < (ncal + 1) / 2 ? i : n - ncal + i; }
COIL_HD inline int coilmix_cal_points(int ncal) { return ncal * ncal; }
// point q of the region -> offset h * W + k inside a slice
COIL_HD inline size_t coilmix_cal_index(int q, int ncal, int H, int W) {
    return (size_t)coilmix_cal_line(q / ncal, ncal, H) * W + coilmix_cal_line(q % ncal, ncal, W);
}

// ---- Gram sums -------------------------------------------------------------------------------------------------------------------
// (re, im) += a conj(b)
COIL_HD inline void coilmix_gram_step(double& re, double& im, double ar, double ai, double br, double bi) {
    const double pr = ar * br, qr = ai * bi, pi = ai * br, qi = ar * bi;
    re = re + (pr + qr);
    im = im + (pi - qi);
}
// tiles of pairs: T = ceil(C / COILMIX_TILE) tiles per side, the T (T + 1) / 2 tile pairs (bi <= bj) in row-major order
COIL_HD inline int coilmix_tiles(int C) { return (C + COILMIX_TILE - 1) / COILMIX_TILE; }
COIL_HD inline int coilmix_tile_pairs(int C) { const int T = coilmix_tiles(C); return T * (T + 1) / 2; }
COIL_HD inline void coilmix_tile_of(int t, int C, int& bi, int& bj) {
    const int T = coilmix_tiles(C);
    bi = 0;
    while (t >= T - bi) { t -= T - bi; ++bi; }
    bj = bi + t;
}
COIL_HD inline size_t coilmix_gram_index(int b, int i, int j, int C) { return ((size_t)b * C + i) * C + j; }

// the Gram matrix of one slice as k_coil_gram forms it: y [C][H][W] interleaved complex, mask [H][W], gram [C][C] interleaved complex double
template <typename R>
inline void coilmix_gram_slice(const R* y, const uint8_t* mask, int C, int H, int W, int ncal, double* gram) {
    const size_t N = (size_t)H * W;
    for (int i = 0; i < C; ++i)
        for (int j = i; j < C; ++j) {
            double re = 0.0, im = 0.0;
            for (int q = 0; q < coilmix_cal_points(ncal); ++q) {
                const size_t at = coilmix_cal_index(q, ncal, H, W);
                if (!mask[at]) continue;
                coilmix_gram_step(re, im, (double)y[2 * (i * N + at)], (double)y[2 * (i * N + at) + 1], (double)y[2 * (j * N + at)],
                                  (double)y[2 * (j * N + at) + 1]);
            }
            if (i == j) im = 0.0;
            gram[2 * coilmix_gram_index(0, i, j, C)] = re;
            gram[2 * coilmix_gram_index(0, i, j, C) + 1] = im;
            gram[2 * coilmix_gram_index(0, j, i, C)] = re;
            gram[2 * coilmix_gram_index(0, j, i, C) + 1] = -im;
        }
}

// ---- mixing ------------------------------------------------------------------------------------------------------------------------
COIL_HD inline int coilmix_points(bool f64) { return f64 ? 1 : 2; }          // 16 bytes of consecutive points per thread
COIL_HD inline size_t coilmix_mix_blocks(size_t N, bool f64) {
    const size_t span = (size_t)COILMIX_MIX_THREADS * coilmix_points(f64);
    return (N + span - 1) / span;
}
// the accumulators a thread keeps: C_out rounded up to 4, 8, 16 or 32
COIL_HD inline int coilmix_out_bucket(int C_out) { return C_out <= 4 ? 4 : C_out <= 8 ? 8 : C_out <= 16 ? 16 : 32; }
COIL_HD inline float  coilmix_fma(float a, float b, float c) { return fmaf(a, b, c); }
COIL_HD inline double coilmix_fma(double a, double b, double c) { return fma(a, b, c); }
// (re, im) += m x
template <typename R> COIL_HD inline void coilmix_cmac(R& re, R& im, R mr, R mi, R xr, R xi) {
    re = coilmix_fma(mr, xr, re);
    re = coilmix_fma(-mi, xi, re);
    im = coilmix_fma(mr, xi, im);
    im = coilmix_fma(mi, xr, im);
}

// ---- host linear algebra (double, interleaved complex, row-major [n][n]) -----------------------------------------------------------
inline bool coilmix_all_finite(const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!(a[i] - a[i] == 0.0)) return false;
    return true;
}

// m = L^-1 with L the lower Cholesky factor of the Hermitian a (its lower triangle is read): m a m^H = I.  -> 0, or 1 + the index of
// the first pivot that is not finite and positive.  m must not alias a.
inline int coilmix_inv_chol(const double* a, int n, double* m) {
    auto RE = [n](double* p, int i, int j) -> double& { return p[2 * ((size_t)i * n + j)]; };
    auto IM = [n](double* p, int i, int j) -> double& { return p[2 * ((size_t)i * n + j) + 1]; };
    // L into m's lower triangle
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) { RE(m, i, j) = 0.0; IM(m, i, j) = 0.0; }
    for (int j = 0; j < n; ++j) {
        double d = a[2 * ((size_t)j * n + j)];
        for (int k = 0; k < j; ++k) d -= RE(m, j, k) * RE(m, j, k) + IM(m, j, k) * IM(m, j, k);
        if (!(d > 0.0) || !(d - d == 0.0)) return 1 + j;
        const double l = sqrt(d);
        RE(m, j, j) = l;
        for (int i = j + 1; i < n; ++i) {
            double sr = a[2 * ((size_t)i * n + j)], si = a[2 * ((size_t)i * n + j) + 1];
            for (int k = 0; k < j; ++k) {          // s -= L[i][k] conj(L[j][k])
                sr -= RE(m, i, k) * RE(m, j, k) + IM(m, i, k) * IM(m, j, k);
                si -= IM(m, i, k) * RE(m, j, k) - RE(m, i, k) * IM(m, j, k);
            }
            RE(m, i, j) = sr / l;
            IM(m, i, j) = si / l;
            if (!(RE(m, i, j) - RE(m, i, j) == 0.0) || !(IM(m, i, j) - IM(m, i, j) == 0.0)) return 1 + j;
        }
    }
    // X = L^-1 in place, from X L = I:  X[j][j] = 1 / L[j][j],  X[i][j] = -(sum_{k = j+1 .. i} X[i][k] L[k][j]) / L[j][j].  The columns go
    // from the last to the first (columns > j already hold X, column j still holds L) and the rows of a column from the bottom up
    // (X[i][j] overwrites L[i][j], which the rows above do not read).
    for (int j = n - 1; j >= 0; --j) {
        const double l = RE(m, j, j);
        for (int i = n - 1; i > j; --i) {
            double sr = 0.0, si = 0.0;
            for (int k = j + 1; k <= i; ++k) {
                const double ar = RE(m, i, k), ai = IM(m, i, k), br = RE(m, k, j), bi = IM(m, k, j);
                sr += ar * br - ai * bi;
                si += ar * bi + ai * br;
            }
            RE(m, i, j) = -sr / l;
            IM(m, i, j) = -si / l;
        }
        RE(m, j, j) = 1.0 / l;
        IM(m, j, j) = 0.0;
    }
    return 0;
}

// Eigen-decomposition of the Hermitian a [n][n] (symmetrised: (a + a^H) / 2) by cyclic Jacobi rotations: eig [n] descending, vec [n][n]
// with the eigenvector of eig[j] in COLUMN j, its phase fixed so that its entry of largest modulus is real and positive (on a tie the
// first such entry).  work: 2 n n doubles.  -> 0, or 1 when the sweeps did not converge (never seen; non-finite input is the caller's check).
inline int coilmix_jacobi(const double* a, int n, double* eig, double* vec, double* work) {
    auto RE = [n](double* p, int i, int j) -> double& { return p[2 * ((size_t)i * n + j)]; };
    auto IM = [n](double* p, int i, int j) -> double& { return p[2 * ((size_t)i * n + j) + 1]; };
    double* A = work;
    double norm2 = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            RE(A, i, j) = 0.5 * (a[2 * ((size_t)i * n + j)] + a[2 * ((size_t)j * n + i)]);
            IM(A, i, j) = i == j ? 0.0 : 0.5 * (a[2 * ((size_t)i * n + j) + 1] - a[2 * ((size_t)j * n + i) + 1]);
            norm2 += RE(A, i, j) * RE(A, i, j) + IM(A, i, j) * IM(A, i, j);
            RE(vec, i, j) = i == j ? 1.0 : 0.0;
            IM(vec, i, j) = 0.0;
        }
    const double tiny = 1e-18 * sqrt(norm2);          // an off-diagonal entry at or below this is left alone
    bool done = n < 2 || norm2 == 0.0;
    for (int sweep = 0; sweep < COILMIX_JACOBI_SWEEPS && !done; ++sweep) {
        done = true;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double gr = RE(A, p, q), gi = IM(A, p, q), g = hypot(gr, gi);
                if (!(g > tiny)) continue;
                done = false;
                // e = exp(i phi) = a_pq / |a_pq|; with U = diag(1, conj(e)) the 2 x 2 block becomes real, then the real rotation (c, s)
                const double er = gr / g, ei = gi / g;
                const double theta = (RE(A, q, q) - RE(A, p, p)) / (2.0 * g);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                // J = U R:  J_pp = c, J_pq = s, J_qp = -s conj(e), J_qq = c conj(e);  A <- J^H A J, vec <- vec J
                for (int pass = 0; pass < 2; ++pass) {
                    double* X = pass ? vec : A;
                    for (int k = 0; k < n; ++k) {          // columns p, q of X J
                        const double pr = RE(X, k, p), pi = IM(X, k, p), qr0 = RE(X, k, q), qi0 = IM(X, k, q);
                        const double qr = qr0 * er + qi0 * ei, qi = qi0 * er - qr0 * ei;          // X_kq conj(e)
                        RE(X, k, p) = c * pr - s * qr; IM(X, k, p) = c * pi - s * qi;
                        RE(X, k, q) = s * pr + c * qr; IM(X, k, q) = s * pi + c * qi;
                    }
                }
                for (int k = 0; k < n; ++k) {              // rows p, q of J^H (A J)
                    const double pr = RE(A, p, k), pi = IM(A, p, k), qr0 = RE(A, q, k), qi0 = IM(A, q, k);
                    const double qr = qr0 * er - qi0 * ei, qi = qi0 * er + qr0 * ei;              // e A_qk
                    RE(A, p, k) = c * pr - s * qr; IM(A, p, k) = c * pi - s * qi;
                    RE(A, q, k) = s * pr + c * qr; IM(A, q, k) = s * pi + c * qi;
                }
                RE(A, p, q) = 0.0; IM(A, p, q) = 0.0; RE(A, q, p) = 0.0; IM(A, q, p) = 0.0;
                IM(A, p, p) = 0.0; IM(A, q, q) = 0.0;
            }
    }
    if (!done) {          // the last sweep still rotated: accept it when what is left is rounding noise
        double off2 = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) if (i != j) off2 += RE(A, i, j) * RE(A, i, j) + IM(A, i, j) * IM(A, i, j);
        if (!(off2 <= 1e-26 * norm2)) return 1;
    }
    // descending order (selection sort, stable: the first of equal eigenvalues stays first), columns of vec moved along
    for (int j = 0; j < n; ++j) eig[j] = RE(A, j, j);
    for (int j = 0; j < n - 1; ++j) {
        int best = j;
        for (int k = j + 1; k < n; ++k) if (eig[k] > eig[best]) best = k;
        for (int k = best; k > j; --k) {          // rotate column `best` down to j, keeping the order of the others
            const double e = eig[k]; eig[k] = eig[k - 1]; eig[k - 1] = e;
            for (int i = 0; i < n; ++i) {
                const double r = RE(vec, i, k), m = IM(vec, i, k);
                RE(vec, i, k) = RE(vec, i, k - 1); IM(vec, i, k) = IM(vec, i, k - 1);
                RE(vec, i, k - 1) = r; IM(vec, i, k - 1) = m;
            }
        }
    }
    // phase: the entry of largest modulus (the first on a tie) real and positive
    for (int j = 0; j < n; ++j) {
        int at = 0;
        double big = -1.0;
        for (int i = 0; i < n; ++i) {
            const double m2 = RE(vec, i, j) * RE(vec, i, j) + IM(vec, i, j) * IM(vec, i, j);
            if (m2 > big) { big = m2; at = i; }
        }
        const double g = hypot(RE(vec, at, j), IM(vec, at, j));
        if (!(g > 0.0)) continue;
        const double ur = RE(vec, at, j) / g, ui = -IM(vec, at, j) / g;          // multiply the column by conj(v_at) / |v_at|
        for (int i = 0; i < n; ++i) {
            const double r = RE(vec, i, j), m = IM(vec, i, j);
            RE(vec, i, j) = r * ur - m * ui;
            IM(vec, i, j) = r * ui + m * ur;
        }
        RE(vec, at, j) = g;
        IM(vec, at, j) = 0.0;
    }
    return 0;
}

// M_c [C_out][n]: row j is the conjugate of the eigenvector of the j-th largest eigenvalue of the Gram matrix (y' = M_c y keeps the C_out
// virtual coils that carry the most calibration energy; M_c M_c^H = I).  eig [n], work: 4 n n doubles.  -> coilmix_jacobi's code
inline int coilmix_compress(const double* gram, int n, int C_out, double* m_out, double* eig, double* work) {
    double* vec = work + 2 * (size_t)n * n;
    if (int rc = coilmix_jacobi(gram, n, eig, vec, work)) return rc;
    for (int j = 0; j < C_out; ++j)
        for (int c = 0; c < n; ++c) {
            m_out[2 * ((size_t)j * n + c)] = vec[2 * ((size_t)c * n + j)];
            m_out[2 * ((size_t)j * n + c) + 1] = -vec[2 * ((size_t)c * n + j) + 1];
        }
    return 0;
}

}  // namespace pnp
