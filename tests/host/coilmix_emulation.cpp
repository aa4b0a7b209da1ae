// g++ emulation of the host-testable parts of the coil mixing (csrc/coilmix_plan.h):
//   coilmix_emulation index H W     the calibration index map for EVERY ncal in 4 .. 64: exactly ncal^2 points, each once, inside the
//                                   slice, in the documented order (rows 0 .. ceil(ncal/2) - 1 then H - floor(ncal/2) .. H - 1, columns
//                                   alike), restated here with two explicit lists; and the kernel's staging walk (chunks of
//                                   COILMIX_GRAM_POINTS points) on arrays of exactly the plan's sizes.
//   coilmix_emulation gram          the Gram sum order (coilmix_gram_slice) against a loop restated here, bit for bit, on float and double
//                                   data with holes in the mask; exact on integers; exact Hermitian symmetry; the tile walk of
//                                   k_coil_gram (every pair i <= j owned by exactly one thread of one tile) for C = 1 .. 128; the
//                                   mixing kernel's (workgroup, thread) -> point map.
//   coilmix_emulation solve C       the two host solvers on seeded Hermitian positive-definite matrices of order C: M Psi M^H = I,
//                                   A v = lambda v, V^H V = I, all to 1e-12; descending order; the phase rule; refusals.
//   coilmix_emulation check         every rule of coilmix_check
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../pnp_admm_cnc_mri_amd/csrc/coilmix_plan.h"

using namespace pnp;
typedef std::complex<double> cd;

static int index_map(int H, int W) {
    for (int ncal = COILMIX_NCAL_MIN; ncal <= COILMIX_NCAL_MAX; ++ncal) {
        if (coilmix_check(1, 1, 1, ncal, H, W) != COILMIX_OK) return 3;
        std::vector<int> rows, cols;
        for (int r = 0; r < (ncal + 1) / 2; ++r) rows.push_back(r);
        for (int r = H - ncal / 2; r < H; ++r) rows.push_back(r);
        for (int c = 0; c < (ncal + 1) / 2; ++c) cols.push_back(c);
        for (int c = W - ncal / 2; c < W; ++c) cols.push_back(c);
        if ((int)rows.size() != ncal || (int)cols.size() != ncal || coilmix_cal_points(ncal) != ncal * ncal) return 2;
        std::vector<uint8_t> seen((size_t)H * W, 0);
        int q = 0;
        for (int r : rows)
            for (int c : cols) {
                if (coilmix_cal_index(q, ncal, H, W) != (size_t)r * W + c) return 2;
                ++seen.at(coilmix_cal_index(q, ncal, H, W));
                ++q;
            }
        size_t count = 0;
        for (uint8_t v : seen) { if (v > 1) return 2; count += v; }
        if (count != (size_t)ncal * ncal) return 2;
        // the staging walk of k_coil_gram: every point lands once in a slot of the [COILMIX_GRAM_POINTS][2 COILMIX_TILE] tile
        const int npts = ncal * ncal, T = COILMIX_TILE, Q = COILMIX_GRAM_POINTS;
        std::vector<uint8_t> hit((size_t)npts, 0);
        for (int q0 = 0; q0 < npts; q0 += Q) {
            std::vector<uint8_t> sh((size_t)Q * 2 * T, 0);
            for (int tid = 0; tid < T * T; ++tid)
                for (int idx = tid; idx < Q * 2 * T; idx += T * T) {
                    const int cl = idx / Q, qq = idx % Q;
                    ++sh.at((size_t)qq * 2 * T + cl);
                    if (cl == 0 && q0 + qq < npts) ++hit.at((size_t)(q0 + qq));
                }
            for (uint8_t v : sh) if (v != 1) return 2;
        }
        for (uint8_t v : hit) if (v != 1) return 2;
    }
    printf("ok index %d %d\n", H, W);
    return 0;
}

template <typename R>
static int gram_case(int C, int H, int W, int ncal, bool integers) {
    const size_t N = (size_t)H * W;
    std::vector<R> y(2 * (size_t)C * N);
    std::vector<uint8_t> mask(N);
    std::mt19937_64 rng(1000 * C + ncal);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (auto& v : y) v = integers ? (R)(int)(8 * u(rng)) : (R)u(rng);
    for (auto& v : mask) v = u(rng) < 0.4 ? 1 : 0;
    std::vector<double> got(2 * (size_t)C * C, -7.0);
    coilmix_gram_slice<R>(y.data(), mask.data(), C, H, W, ncal, got.data());
    // restated: the region's rows then columns, skip the holes, one chain per pair, every product and sum rounded on its own
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
            volatile double re = 0.0, im = 0.0;
            long double lre = 0, lim = 0;
            for (int a = 0; a < ncal; ++a) {
                const int r = a < (ncal + 1) / 2 ? a : H - ncal + a;
                for (int b = 0; b < ncal; ++b) {
                    const int c = b < (ncal + 1) / 2 ? b : W - ncal + b;
                    const size_t at = (size_t)r * W + c;
                    if (!mask[at]) continue;
                    const int lo = i < j ? i : j, hi = i < j ? j : i;          // the pair is formed once, for lo <= hi
                    const double ar = y[2 * (lo * N + at)], ai = y[2 * (lo * N + at) + 1], br = y[2 * (hi * N + at)], bi = y[2 * (hi * N + at) + 1];
                    volatile double p1 = ar * br, p2 = ai * bi, p3 = ai * br, p4 = ar * bi;
                    volatile double s1 = p1 + p2, s2 = p3 - p4;
                    re = re + s1;
                    im = im + s2;
                    lre += (long double)ar * br + (long double)ai * bi;
                    lim += (long double)ai * br - (long double)ar * bi;
                }
            }
            double wr = re, wi = i == j ? 0.0 : (i < j ? im : -im);
            const double gr = got[2 * ((size_t)i * C + j)], gi = got[2 * ((size_t)i * C + j) + 1];
            if (gr != wr || gi != wi) return 2;
            if (got[2 * ((size_t)j * C + i)] != gr || got[2 * ((size_t)j * C + i) + 1] != -gi) return 2;          // Hermitian to the bit
            if (integers && (gr != (double)lre || (i <= j ? gi : -gi) != (double)(i == j ? 0 : lim))) return 2;
        }
    return 0;
}

static int gram() {
    for (int ncal : {4, 5, 24}) {
        if (gram_case<float>(3, 128, 128, ncal, false) || gram_case<double>(3, 131, 128, ncal, false)) return 2;
        if (gram_case<float>(2, 140, 160, ncal, true) || gram_case<double>(1, 128, 128, ncal, true)) return 2;
    }
    // tiles of pairs: every (i <= j) belongs to exactly one thread of one workgroup
    for (int C = 1; C <= COILMIX_MAX_IN; ++C) {
        std::vector<uint8_t> own((size_t)C * C, 0);
        const int T = COILMIX_TILE;
        for (int t = 0; t < coilmix_tile_pairs(C); ++t) {
            int bi, bj;
            coilmix_tile_of(t, C, bi, bj);
            if (bi < 0 || bi > bj || bj >= coilmix_tiles(C)) return 2;
            for (int tid = 0; tid < T * T; ++tid) {
                const int i = bi * T + tid / T, j = bj * T + tid % T;
                if (i < C && j < C && i <= j) ++own.at((size_t)i * C + j);
            }
        }
        for (int i = 0; i < C; ++i) for (int j = 0; j < C; ++j) if (own[(size_t)i * C + j] != (i <= j ? 1 : 0)) return 2;
    }
    // the mixing kernel: grid coilmix_mix_blocks(N) x 256 threads x coilmix_points points, guarded by p < N
    for (bool f64 : {false, true})
        for (size_t N : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1025, (size_t)128 * 130}) {
            std::vector<uint8_t> hit(N, 0);
            for (size_t blk = 0; blk < coilmix_mix_blocks(N, f64); ++blk)
                for (int t = 0; t < COILMIX_MIX_THREADS; ++t)
                    for (int k = 0; k < coilmix_points(f64); ++k) {
                        const size_t p = (blk * COILMIX_MIX_THREADS + t) * coilmix_points(f64) + k;
                        if (p < N) ++hit.at(p);
                    }
            for (uint8_t v : hit) if (v != 1) return 2;
        }
    for (int c = 1; c <= COIL_MAX_C; ++c) if (coilmix_out_bucket(c) < c || coilmix_out_bucket(c) > 32 || (c > 4 && coilmix_out_bucket(c) >= 2 * c)) return 2;
    // one mixing step is four fused multiply-adds
    double re = 1.0, im = 2.0;
    coilmix_cmac(re, im, 3.0, 4.0, 5.0, 6.0);
    if (re != 1.0 + 15.0 - 24.0 || im != 2.0 + 18.0 + 20.0) return 2;
    printf("ok gram\n");
    return 0;
}

static int solve(int n) {
    std::mt19937_64 rng(77 + n);
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<cd> B((size_t)n * n), A((size_t)n * n);
    for (auto& v : B) v = cd(g(rng), g(rng));
    double norm2 = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            cd s = i == j ? cd(0.5, 0) : cd(0, 0);
            for (int k = 0; k < n; ++k) s += B[(size_t)i * n + k] * std::conj(B[(size_t)j * n + k]) / (double)n;
            A[(size_t)i * n + j] = s;
        }
    for (int i = 0; i < n; ++i) A[(size_t)i * n + i] = cd(A[(size_t)i * n + i].real(), 0);
    for (auto& v : A) norm2 += std::norm(v);
    const double* a = reinterpret_cast<const double*>(A.data());
    // ---- inverse Cholesky factor
    std::vector<cd> M((size_t)n * n);
    if (coilmix_inv_chol(a, n, reinterpret_cast<double*>(M.data())) != 0) return 2;
    double worst = 0;
    std::vector<cd> MA((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < n; ++l) {
            cd s = 0;
            for (int k = 0; k < n; ++k) s += M[(size_t)i * n + k] * A[(size_t)k * n + l];
            MA[(size_t)i * n + l] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (j > i && M[(size_t)i * n + j] != cd(0, 0)) return 2;          // lower triangular
            cd s = 0;
            for (int l = 0; l < n; ++l) s += MA[(size_t)i * n + l] * std::conj(M[(size_t)j * n + l]);
            worst = std::fmax(worst, std::abs(s - (i == j ? cd(1, 0) : cd(0, 0))));
        }
    if (!(worst <= 1e-12)) { fprintf(stderr, "whiten %d: %.3e\n", n, worst); return 2; }
    // refusals: a negative pivot, a zero matrix, a NaN, an infinity
    {
        std::vector<cd> bad(A), out((size_t)n * n);
        bad[(size_t)(n - 1) * n + (n - 1)] = cd(-1, 0);
        if (coilmix_inv_chol(reinterpret_cast<const double*>(bad.data()), n, reinterpret_cast<double*>(out.data())) != n) return 2;
        std::vector<cd> zero((size_t)n * n, cd(0, 0));
        if (coilmix_inv_chol(reinterpret_cast<const double*>(zero.data()), n, reinterpret_cast<double*>(out.data())) != 1) return 2;
        bad = A; bad[0] = cd(NAN, 0);
        if (coilmix_inv_chol(reinterpret_cast<const double*>(bad.data()), n, reinterpret_cast<double*>(out.data())) == 0) return 2;
        if (coilmix_all_finite(reinterpret_cast<const double*>(bad.data()), 2 * (size_t)n * n)) return 2;
        bad = A; bad[(size_t)n * n - 1] = cd(INFINITY, 0);
        if (coilmix_inv_chol(reinterpret_cast<const double*>(bad.data()), n, reinterpret_cast<double*>(out.data())) == 0) return 2;
        if (coilmix_all_finite(reinterpret_cast<const double*>(bad.data()), 2 * (size_t)n * n) || !coilmix_all_finite(a, 2 * (size_t)n * n)) return 2;
    }
    // ---- Jacobi
    std::vector<cd> V((size_t)n * n);
    std::vector<double> eig((size_t)n), work(4 * (size_t)n * n);
    if (coilmix_jacobi(a, n, eig.data(), reinterpret_cast<double*>(V.data()), work.data()) != 0) return 2;
    const double an = std::sqrt(norm2);
    double r_eig = 0, r_orth = 0;
    for (int j = 0; j < n; ++j) {
        if (j && eig[j] > eig[j - 1]) return 2;
        for (int i = 0; i < n; ++i) {
            cd s = 0;
            for (int k = 0; k < n; ++k) s += A[(size_t)i * n + k] * V[(size_t)k * n + j];
            r_eig = std::fmax(r_eig, std::abs(s - eig[j] * V[(size_t)i * n + j]));
        }
        for (int l = 0; l < n; ++l) {
            cd s = 0;
            for (int k = 0; k < n; ++k) s += std::conj(V[(size_t)k * n + j]) * V[(size_t)k * n + l];
            r_orth = std::fmax(r_orth, std::abs(s - (j == l ? cd(1, 0) : cd(0, 0))));
        }
        // phase: the first entry of largest modulus is real and positive
        int at = 0;
        for (int i = 1; i < n; ++i) if (std::norm(V[(size_t)i * n + j]) > std::norm(V[(size_t)at * n + j])) at = i;
        if (V[(size_t)at * n + j].imag() != 0.0 || !(V[(size_t)at * n + j].real() > 0.0)) return 2;
    }
    if (!(r_eig <= 1e-12 * an) || !(r_orth <= 1e-12)) { fprintf(stderr, "jacobi %d: %.3e %.3e\n", n, r_eig / an, r_orth); return 2; }
    // the compression matrix: conjugated leading eigenvectors as rows
    const int co = n < 5 ? n : 5;
    std::vector<cd> Mc((size_t)co * n);
    std::vector<double> eig2((size_t)n);
    if (coilmix_compress(a, n, co, reinterpret_cast<double*>(Mc.data()), eig2.data(), work.data()) != 0) return 2;
    for (int j = 0; j < co; ++j)
        for (int c = 0; c < n; ++c) if (Mc[(size_t)j * n + c] != std::conj(V[(size_t)c * n + j]) || eig2[j] != eig[j]) return 2;
    // a diagonal matrix with a tie: eigenvalues sorted, the first of the equal ones first, unit vectors
    if (n >= 3) {
        std::vector<cd> D((size_t)n * n, cd(0, 0));
        for (int i = 0; i < n; ++i) D[(size_t)i * n + i] = cd(i == 1 ? 9.0 : i == 2 ? 9.0 : 1.0 / (1 + i), 0);
        if (coilmix_jacobi(reinterpret_cast<const double*>(D.data()), n, eig.data(), reinterpret_cast<double*>(V.data()), work.data()) != 0) return 2;
        if (eig[0] != 9.0 || eig[1] != 9.0 || V[(size_t)1 * n + 0] != cd(1, 0) || V[(size_t)2 * n + 1] != cd(1, 0)) return 2;
    }
    printf("ok solve %d\n", n);
    return 0;
}

static int check() {
    if (coilmix_check(64, 8, 1, 24, 256, 256) != COILMIX_OK || coilmix_check(128, 32, 7, 64, 1024, 128) != COILMIX_OK ||
        coilmix_check(1, 1, 1, 4, 128, 128) != COILMIX_OK) return 2;
    if (coilmix_check(0, 1, 1, 24, 128, 128) != COILMIX_BAD_IN || coilmix_check(129, 8, 1, 24, 128, 128) != COILMIX_BAD_IN) return 2;
    if (coilmix_check(8, 0, 1, 24, 128, 128) != COILMIX_BAD_OUT || coilmix_check(8, 9, 1, 24, 128, 128) != COILMIX_BAD_OUT ||
        coilmix_check(64, 33, 1, 24, 128, 128) != COILMIX_BAD_OUT) return 2;
    if (coilmix_check(8, 4, 0, 24, 128, 128) != COILMIX_BAD_SETS) return 2;
    if (coilmix_check(8, 4, 1, 3, 128, 128) != COILMIX_BAD_NCAL || coilmix_check(8, 4, 1, 65, 128, 128) != COILMIX_BAD_NCAL) return 2;
    if (coilmix_check(8, 4, 1, 24, 127, 128) != COILMIX_BAD_SHAPE || coilmix_check(8, 4, 1, 24, 128, 1025) != COILMIX_BAD_SHAPE) return 2;
    printf("ok check\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "index")) return index_map(atoi(argv[2]), atoi(argv[3]));
    if (argc == 2 && !strcmp(argv[1], "gram")) return gram();
    if (argc == 3 && !strcmp(argv[1], "solve")) return solve(atoi(argv[2]));
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    fprintf(stderr, "usage: coilmix_emulation index H W | gram | solve C | check\n");
    return 1;
}
