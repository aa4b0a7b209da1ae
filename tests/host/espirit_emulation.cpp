// g++ emulation of the host-testable parts of the ESPIRiT coil map estimation (csrc/espirit_plan.h):
//   espirit_emulation check         every rule of espirit_check, in its order
//   espirit_emulation index         the calibration block is the region rolled by ncal / 2 (ascending signed frequency); the column map;
//                                   for EVERY valid (C, k, ncal): the coils a Gram tile touches cover its columns, the staged rows are at
//                                   least k, and the staged image fits ESPIRIT_GRAM_LDS; for every valid (C, k, precision) the tile choice of
//                                   k_espirit_maps fits 128 KiB, prefers 64 KiB, keeps an odd slot stride and disjoint LDS arrays.
//   espirit_emulation gram          the staging walk of k_calib_patch_gram, emulated chunk by chunk with every LDS read checked against
//                                   what the chunk staged, equals espirit_gram_slice bit for bit (float and double); exactly Hermitian,
//                                   +0 on the diagonal's imaginary part; equals a long-hand double loop to 1e-13.
//   espirit_emulation kernels       espirit_kernels on a Gram matrix of known rank: the rank, P a Hermitian projector of that trace
//                                   (through w's zero-offset entries), w_c'c(-d) = conj(w_cc'(d)) to the bit, w equals the long-hand sums
//                                   over the known projector to 1e-10.
//   espirit_emulation slice         espirit_slice (float and double): unit norm inside the support, exact +0 outside, v^H I real and
//                                   >= 0, G Hermitian by construction: lambda equals a long-hand evaluation with a stored G bit for bit.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../pnp_admm_cnc_mri_amd/csrc/espirit_plan.h"

using namespace pnp;
typedef std::complex<double> cd;

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

template <typename R> static bool same(R a, R b) { return memcmp(&a, &b, sizeof(R)) == 0; }

static int run_check() {
    REQUIRE(espirit_check(1, 4, 2, 1, 0.5, 0.0, 0.0, 128, 128) == ESPIRIT_OK);
    REQUIRE(espirit_check(32, 64, 2, 16, 0.02, 1.0, 0.99, 1024, 1024) == ESPIRIT_OK);
    REQUIRE(espirit_check(2, 16, 8, 2, 0.02, 0.9, 0.05, 131, 128) == ESPIRIT_OK);
    REQUIRE(espirit_check(8, 24, 4, 8, 0.02, 0.9, 0.05, 128, 130) == ESPIRIT_OK);
    REQUIRE(espirit_check(0, 24, 4, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_C);
    REQUIRE(espirit_check(33, 24, 2, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_C);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, 0.9, 0.05, 127, 128) == ESPIRIT_BAD_SHAPE);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, 0.9, 0.05, 128, 1025) == ESPIRIT_BAD_SHAPE);
    REQUIRE(espirit_check(8, 3, 2, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_NCAL);
    REQUIRE(espirit_check(8, 65, 4, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_NCAL);
    REQUIRE(espirit_check(8, 24, 1, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_KERNEL);
    REQUIRE(espirit_check(1, 24, 9, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_KERNEL);
    REQUIRE(espirit_check(1, 5, 6, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_KERNEL_OVER_NCAL);
    REQUIRE(espirit_check(9, 24, 4, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_SIZE);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_OK);          // 8 * 16 = 128: the limit itself
    REQUIRE(espirit_check(3, 24, 7, 4, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_SIZE);
    REQUIRE(espirit_check(8, 24, 4, 0, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_ITERS);
    REQUIRE(espirit_check(8, 24, 4, 17, 0.02, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_ITERS);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.0, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_SIGMA);
    REQUIRE(espirit_check(8, 24, 4, 4, 1.0, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_SIGMA);
    REQUIRE(espirit_check(8, 24, 4, 4, NAN, 0.9, 0.05, 128, 128) == ESPIRIT_BAD_SIGMA);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, -0.1, 0.05, 128, 128) == ESPIRIT_BAD_CROP);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, 1.01, 0.05, 128, 128) == ESPIRIT_BAD_CROP);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, NAN, 0.05, 128, 128) == ESPIRIT_BAD_CROP);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, 0.9, -0.01, 128, 128) == ESPIRIT_BAD_THRESH);
    REQUIRE(espirit_check(8, 24, 4, 4, 0.02, 0.9, 1.0, 128, 128) == ESPIRIT_BAD_THRESH);
    REQUIRE(espirit_check(0, 3, 1, 0, 0.0, 2.0, 1.0, 127, 128) == ESPIRIT_BAD_C);           // the first broken rule is the one named
    puts("ok check");
    return 0;
}

static int run_index() {
    for (int ncal : {4, 5, 16, 24, 33, 64}) {
        const int H = 131, W = 140;
        int prev = -1000;
        for (int t = 0; t < ncal; ++t) {          // ascending signed frequency, every line once
            const int line = espirit_block_line(t, ncal), f = coilmaps_freq(line, ncal);
            REQUIRE(line >= 0 && line < ncal && f == t - ncal / 2 && f > prev);
            prev = f;
            REQUIRE(espirit_block_index(t, 0, ncal, H, W) / W == (size_t)coilmix_cal_line(line, ncal, H));
            REQUIRE(espirit_block_index(0, t, ncal, H, W) % W == (size_t)coilmix_cal_line(line, ncal, W));
        }
    }
    for (int k = 2; k <= 8; ++k)
        for (int m = 0; m < 3 * k * k; ++m) {
            int c, a, b;
            espirit_column(m, k, c, a, b);
            REQUIRE(a >= 0 && a < k && b >= 0 && b < k && (c * k + a) * k + b == m);
        }
    int cases = 0;
    for (int C = 1; C <= 32; ++C)
        for (int k = 2; k <= 8; ++k)
            for (int ncal = 4; ncal <= 64; ++ncal) {
                if (espirit_check(C, ncal, k, 1, 0.5, 0.0, 0.0, 128, 128) != ESPIRIT_OK) continue;
                ++cases;
                const int n = espirit_columns(C, k), T = coilmix_tiles(n);
                for (int t = 0; t < coilmix_tile_pairs(n); ++t) {
                    int bi, bj, ca0, na, cb0, nb;
                    coilmix_tile_of(t, n, bi, bj);
                    REQUIRE(bi >= 0 && bi <= bj && bj < T);
                    espirit_tile_coils(bi, n, k, ca0, na);
                    espirit_tile_coils(bj, n, k, cb0, nb);
                    for (int side = 0; side < 2; ++side) {
                        const int b0 = side ? bj : bi, c0 = side ? cb0 : ca0, cnt = side ? nb : na;
                        REQUIRE(cnt >= 1 && c0 >= 0 && c0 + cnt <= C);
                        for (int m = b0 * ESPIRIT_TILE; m < (b0 + 1) * ESPIRIT_TILE && m < n; ++m) REQUIRE(m / (k * k) >= c0 && m / (k * k) < c0 + cnt);
                    }
                    const int RS = espirit_stage_rows(ncal, na + nb);
                    REQUIRE(RS >= k);
                    REQUIRE((size_t)(na + nb) * RS * ncal * 16 <= ESPIRIT_GRAM_LDS);
                }
            }
    REQUIRE(cases > 1000);
    for (int f64 = 0; f64 < 2; ++f64)
        for (int C = 1; C <= 32; ++C)
            for (int k = 2; k <= 8; ++k) {
                if (C * k * k > ESPIRIT_MAX_N) continue;
                const int j = espirit_tile_choice(C, k, f64);
                const CoilmapsTile t = coilmaps_tile_at(j);
                const EspiritLds l = espirit_lds(t, C, k, f64);
                REQUIRE(l.bytes <= COILMAPS_LDS_HARD);
                if (j > 0) REQUIRE(espirit_lds(coilmaps_tile_at(j - 1), C, k, f64).bytes > COILMAPS_LDS_SOFT);
                if (l.bytes > COILMAPS_LDS_SOFT)
                    for (int i = 0; i < COILMAPS_TILES; ++i) REQUIRE(i >= j || espirit_lds(coilmaps_tile_at(i), C, k, f64).bytes > COILMAPS_LDS_HARD);
                const int slots = coilmaps_stride_slots(coilmix_out_bucket(C), f64);
                REQUIRE(slots % 2 == 1 && (size_t)slots * 16 >= (size_t)C * coilmaps_cx_bytes(f64));
                REQUIRE(l.slab == 0 && l.w == (size_t)t.th * t.tw * slots * 16 && l.w % 16 == 0 && l.eh > l.w && l.ew > l.eh && l.bytes > l.ew);
                REQUIRE(l.eh - l.w == (size_t)espirit_pairs(C) * espirit_side(k) * espirit_side(k) * coilmaps_cx_bytes(f64));
                int p = 0;
                for (int c = 0; c < C; ++c)
                    for (int c2 = c; c2 < C; ++c2) REQUIRE(espirit_pair(c, c2, C) == p++);
                REQUIRE(p == espirit_pairs(C));
            }
    puts("ok index");
    return 0;
}

// k_calib_patch_gram on the host: the same chunks, the same staged image, every read checked
template <typename R>
static void gram_kernel(const std::vector<R>& y, const uint8_t* mask, int C, int H, int W, int ncal, int k, std::vector<double>& gram) {
    const int n = espirit_columns(C, k), P = espirit_positions(ncal, k), T = ESPIRIT_TILE;
    const size_t N = (size_t)H * W;
    for (int tile = 0; tile < coilmix_tile_pairs(n); ++tile) {
        int bi, bj, ca0, na, cb0, nb;
        coilmix_tile_of(tile, n, bi, bj);
        espirit_tile_coils(bi, n, k, ca0, na);
        espirit_tile_coils(bj, n, k, cb0, nb);
        const int RS = espirit_stage_rows(ncal, na + nb), RI = RS - (k - 1);
        REQUIRE(RI >= 1);
        std::vector<double> sh(ESPIRIT_GRAM_LDS / 8), re(T * T, 0.0), im(T * T, 0.0);
        std::vector<char> staged(ESPIRIT_GRAM_LDS / 16);
        for (int i0 = 0; i0 < P; i0 += RI) {
            const int ri = P - i0 < RI ? P - i0 : RI, rows = ri + k - 1;
            std::fill(staged.begin(), staged.end(), 0);
            for (int idx = 0; idx < (na + nb) * rows * ncal; ++idx) {
                const int s = idx / (rows * ncal), r = idx / ncal % rows, u = idx % ncal;
                const int coil = s < na ? ca0 + s : cb0 + (s - na);
                REQUIRE(coil >= 0 && coil < C && i0 + r < ncal);
                const size_t at = espirit_block_index(i0 + r, u, ncal, H, W), slot = ((size_t)s * RS + r) * ncal + u;
                REQUIRE(at < N && slot < staged.size() && !staged[slot]);
                staged[slot] = 1;
                const bool on = !mask || mask[at];
                sh[2 * slot] = on ? (double)y[2 * (coil * N + at)] : 0.0;
                sh[2 * slot + 1] = on ? (double)y[2 * (coil * N + at) + 1] : 0.0;
            }
            for (int th = 0; th < T * T; ++th) {
                const int m = bi * T + th / T, m2 = bj * T + th % T;
                if (!(m < n && m2 < n && m <= m2)) continue;
                int cm, am, bm, cn, an, bn;
                espirit_column(m, k, cm, am, bm);
                espirit_column(m2, k, cn, an, bn);
                const int sm = cm - ca0, sn = na + cn - cb0;
                REQUIRE(sm >= 0 && sm < na && sn >= na && sn < na + nb);
                for (int i = 0; i < ri; ++i)
                    for (int j = 0; j < P; ++j) {
                        const size_t pa = ((size_t)sm * RS + i + am) * ncal + bm + j, pb = ((size_t)sn * RS + i + an) * ncal + bn + j;
                        REQUIRE(pa < staged.size() && pb < staged.size() && staged[pa] && staged[pb]);
                        coilmix_gram_step(re[th], im[th], sh[2 * pb], sh[2 * pb + 1], sh[2 * pa], sh[2 * pa + 1]);
                    }
            }
        }
        for (int th = 0; th < T * T; ++th) {
            const int m = bi * T + th / T, m2 = bj * T + th % T;
            if (!(m < n && m2 < n && m <= m2)) continue;
            gram[2 * ((size_t)m * n + m2)] = re[th];
            gram[2 * ((size_t)m * n + m2) + 1] = m == m2 ? 0.0 : im[th];
            if (m != m2) { gram[2 * ((size_t)m2 * n + m)] = re[th]; gram[2 * ((size_t)m2 * n + m) + 1] = -im[th]; }
        }
    }
}

template <typename R> static void gram_case(int C, int H, int W, int ncal, int k, bool holes, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> g(0.0, 1.0);
    const size_t N = (size_t)H * W;
    std::vector<R> y(2 * C * N);
    for (R& v : y) v = (R)g(rng);
    std::vector<uint8_t> mask(N, 1);
    if (holes) { mask[0] = 0; mask[(size_t)(H - 1) * W + 1] = 0; }
    const int n = espirit_columns(C, k), P = espirit_positions(ncal, k);
    std::vector<double> want(2 * (size_t)n * n, NAN), got(2 * (size_t)n * n, NAN);
    espirit_gram_slice<R>(y.data(), holes ? mask.data() : nullptr, C, H, W, ncal, k, want.data());
    gram_kernel<R>(y, holes ? mask.data() : nullptr, C, H, W, ncal, k, got);
    for (size_t i = 0; i < want.size(); ++i) REQUIRE(same(want[i], got[i]));
    // long-hand: std::complex, the block gathered first
    std::vector<cd> K((size_t)C * ncal * ncal);
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < ncal; ++t)
            for (int u = 0; u < ncal; ++u) {
                const int lt = ((t - ncal / 2) % ncal + ncal) % ncal, lu = ((u - ncal / 2) % ncal + ncal) % ncal;          // the roll, long-hand
                const int h = lt < (ncal + 1) / 2 ? lt : H - ncal + lt, x = lu < (ncal + 1) / 2 ? lu : W - ncal + lu;
                const size_t at = (size_t)h * W + x;
                K[((size_t)c * ncal + t) * ncal + u] = holes && !mask[at] ? cd(0.0) : cd((double)y[2 * (c * N + at)], (double)y[2 * (c * N + at) + 1]);
            }
    double worst = 0.0, scale = 0.0;
    for (int m = 0; m < n; ++m)
        for (int m2 = 0; m2 < n; ++m2) {
            const int c = m / (k * k), a = m / k % k, b = m % k, c2 = m2 / (k * k), a2 = m2 / k % k, b2 = m2 % k;
            cd s(0.0);
            for (int i = 0; i < P; ++i)
                for (int j = 0; j < P; ++j) s += std::conj(K[((size_t)c * ncal + i + a) * ncal + j + b]) * K[((size_t)c2 * ncal + i + a2) * ncal + j + b2];
            const cd have(got[2 * ((size_t)m * n + m2)], got[2 * ((size_t)m * n + m2) + 1]);
            worst = std::fmax(worst, std::abs(have - s));
            scale = std::fmax(scale, std::abs(s));
            REQUIRE(same(got[2 * ((size_t)m * n + m2)], got[2 * ((size_t)m2 * n + m)]));
            if (m != m2) REQUIRE(same(got[2 * ((size_t)m * n + m2) + 1], -got[2 * ((size_t)m2 * n + m) + 1]));
            else         REQUIRE(same(got[2 * ((size_t)m * n + m) + 1], 0.0));
        }
    REQUIRE(worst <= 1e-13 * scale);
}

static int run_gram() {
    gram_case<float>(1, 128, 128, 4, 2, false, 1);
    gram_case<double>(2, 131, 128, 16, 8, false, 2);
    gram_case<float>(5, 140, 160, 32, 5, true, 3);
    gram_case<double>(8, 128, 130, 24, 4, false, 4);
    gram_case<float>(8, 131, 128, 16, 3, false, 5);
    gram_case<double>(32, 128, 128, 5, 2, true, 6);
    gram_case<float>(3, 128, 128, 64, 2, false, 7);          // the most rows: several chunks
    puts("ok gram");
    return 0;
}

static int run_kernels() {
    std::mt19937 rng(11);
    std::normal_distribution<double> g(0.0, 1.0);
    for (int C : {1, 3, 8})
        for (int k : {2, 3, 4}) {
            const int n = espirit_columns(C, k), D = espirit_side(k), want_rank = n < 6 ? 2 : 5, rows = 4 * n;
            // A = L Q [rows][n] with Q [want_rank][n] of orthonormal rows (Gram-Schmidt): rank want_rank, conj(P) = sum_r q_r q_r^H
            std::vector<cd> A((size_t)rows * n), L((size_t)rows * want_rank), Rm((size_t)want_rank * n);
            for (cd& v : L) v = cd(g(rng), g(rng));
            for (cd& v : Rm) v = cd(g(rng), g(rng));
            for (int r = 0; r < want_rank; ++r) {
                for (int q = 0; q < r; ++q) {
                    cd dot(0.0);
                    for (int j = 0; j < n; ++j) dot += std::conj(Rm[(size_t)q * n + j]) * Rm[(size_t)r * n + j];
                    for (int j = 0; j < n; ++j) Rm[(size_t)r * n + j] -= dot * Rm[(size_t)q * n + j];
                }
                double nr = 0.0;
                for (int j = 0; j < n; ++j) nr += std::norm(Rm[(size_t)r * n + j]);
                for (int j = 0; j < n; ++j) Rm[(size_t)r * n + j] /= std::sqrt(nr);
            }
            for (int i = 0; i < rows; ++i)
                for (int j = 0; j < n; ++j) {
                    cd s(0.0);
                    for (int r = 0; r < want_rank; ++r) s += L[(size_t)i * want_rank + r] * Rm[(size_t)r * n + j];
                    A[(size_t)i * n + j] = s;
                }
            std::vector<double> gram(2 * (size_t)n * n), w(2 * espirit_w_count(C, k), NAN), sing(n), work(espirit_work_doubles(n));
            for (int m = 0; m < n; ++m)
                for (int m2 = 0; m2 < n; ++m2) {
                    cd s(0.0);
                    for (int i = 0; i < rows; ++i) s += std::conj(A[(size_t)i * n + m]) * A[(size_t)i * n + m2];
                    gram[2 * ((size_t)m * n + m2)] = s.real();
                    gram[2 * ((size_t)m * n + m2) + 1] = s.imag();
                }
            int rank = -1;
            REQUIRE(espirit_kernels(gram.data(), C, k, 0.02, w.data(), &rank, sing.data(), work.data()) == 0);
            REQUIRE(rank == want_rank);
            for (int j = 1; j < n; ++j) REQUIRE(sing[j] <= sing[j - 1] && sing[j] >= 0.0);
            REQUIRE(sing[want_rank] < 1e-6 * sing[0]);
            // trace(P) = rank: sum_c w_cc(0) = trace / k^2
            double tr = 0.0;
            for (int c = 0; c < C; ++c) {
                tr += w[2 * espirit_w_index(c, c, 0, 0, C, k)];
                REQUIRE(std::fabs(w[2 * espirit_w_index(c, c, 0, 0, C, k) + 1]) <= 1e-15);
            }
            REQUIRE(std::fabs(tr * k * k - want_rank) <= 1e-10);
            for (int c = 0; c < C; ++c)
                for (int c2 = c + 1; c2 < C; ++c2)
                    for (int dy = -(k - 1); dy <= k - 1; ++dy)
                        for (int dx = -(k - 1); dx <= k - 1; ++dx) {
                            REQUIRE(same(w[2 * espirit_w_index(c, c2, dy, dx, C, k)], w[2 * espirit_w_index(c2, c, -dy, -dx, C, k)]));
                            REQUIRE(same(w[2 * espirit_w_index(c, c2, dy, dx, C, k) + 1], -w[2 * espirit_w_index(c2, c, -dy, -dx, C, k) + 1]));
                        }
            // w long-hand from conj(P) = sum_r q_r q_r^H
            for (int c = 0; c < C; ++c)
                for (int c2 = 0; c2 < C; ++c2)
                    for (int dy = -(k - 1); dy <= k - 1; ++dy)
                        for (int dx = -(k - 1); dx <= k - 1; ++dx) {
                            cd sum(0.0);
                            for (int ay = 0; ay < k; ++ay)
                                for (int ax = 0; ax < k; ++ax) {
                                    const int by = ay - dy, bx = ax - dx;
                                    if (by < 0 || by >= k || bx < 0 || bx >= k) continue;
                                    for (int r = 0; r < want_rank; ++r)
                                        sum += Rm[(size_t)r * n + c * k * k + ay * k + ax] * std::conj(Rm[(size_t)r * n + c2 * k * k + by * k + bx]);
                                }
                            const cd have(w[2 * espirit_w_index(c, c2, dy, dx, C, k)], w[2 * espirit_w_index(c, c2, dy, dx, C, k) + 1]);
                            REQUIRE(std::abs(have - sum / (double)(k * k)) <= 1e-10);
                        }
            (void)D;
        }
    puts("ok kernels");
    return 0;
}

template <typename R> static void slice_case(int C, int k, int iters, double crop, double thresh, unsigned seed) {
    const int H = 12, W = 10, D = espirit_side(k);
    const size_t N = (size_t)H * W;
    std::mt19937 rng(seed);
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<R> img(2 * C * N), w(2 * espirit_w_count(C, k)), maps(2 * C * N, (R)NAN), lam(N, (R)NAN);
    for (R& v : img) v = (R)g(rng);
    for (int c = 0; c < C; ++c) { img[2 * (c * N + 7)] = R(0); img[2 * (c * N + 7) + 1] = R(0); }          // one pixel with I = 0: e_0
    // a Hermitian, roughly contractive family of kernels: w_cc'(d) small, w_cc(0) about 1 / C
    for (int c = 0; c < C; ++c)
        for (int c2 = c; c2 < C; ++c2)
            for (int dy = -(k - 1); dy <= k - 1; ++dy)
                for (int dx = -(k - 1); dx <= k - 1; ++dx) {
                    if (c == c2 && (dy < 0 || (dy == 0 && dx < 0))) continue;          // the diagonal block: filled from its other half
                    R re = (R)(0.05 * g(rng)), im = (R)(0.05 * g(rng));
                    if (c == c2 && dy == 0 && dx == 0) { re = (R)1; im = R(0); }
                    w[2 * espirit_w_index(c, c2, dy, dx, C, k)] = re;
                    w[2 * espirit_w_index(c, c2, dy, dx, C, k) + 1] = im;
                    w[2 * espirit_w_index(c2, c, -dy, -dx, C, k)] = re;
                    w[2 * espirit_w_index(c2, c, -dy, -dx, C, k) + 1] = -im;
                }
    espirit_slice<R>(img.data(), C, H, W, w.data(), k, iters, crop, thresh, maps.data(), lam.data());
    // long-hand: G stored in full, then the same chains
    std::vector<R> eh(2 * (size_t)H * D), ew(2 * (size_t)W * D);
    espirit_phasor_table<R>(H, k, eh.data());
    espirit_phasor_table<R>(W, k, ew.data());
    int inside = 0, outside = 0;
    R imax = 0;
    std::vector<R> inorm(N);
    for (size_t p = 0; p < N; ++p) {
        R s = 0;
        for (int c = 0; c < C; ++c) { s = coilmix_fma(img[2 * (c * N + p)], img[2 * (c * N + p)], s); s = coilmix_fma(img[2 * (c * N + p) + 1], img[2 * (c * N + p) + 1], s); }
        inorm[p] = std::sqrt(s);
        if (inorm[p] > imax) imax = inorm[p];
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            std::vector<R> G(2 * C * C), v(2 * C), u(2 * C);
            for (int c = 0; c < C; ++c)
                for (int c2 = c; c2 < C; ++c2) {
                    R gr = 0, gi = 0;
                    for (int dy = 0; dy < D; ++dy) {
                        R ir = 0, ii = 0;
                        for (int dx = 0; dx < D; ++dx) {
                            const R wr = w[2 * espirit_w_index(c, c2, dy - (k - 1), dx - (k - 1), C, k)], wi = w[2 * espirit_w_index(c, c2, dy - (k - 1), dx - (k - 1), C, k) + 1];
                            const R er = ew[2 * ((size_t)x * D + dx)], ei = ew[2 * ((size_t)x * D + dx) + 1];
                            ir = coilmix_fma(wr, er, ir); ir = coilmix_fma(-wi, ei, ir);
                            ii = coilmix_fma(wr, ei, ii); ii = coilmix_fma(wi, er, ii);
                        }
                        const R er = eh[2 * ((size_t)y * D + dy)], ei = eh[2 * ((size_t)y * D + dy) + 1];
                        gr = coilmix_fma(er, ir, gr); gr = coilmix_fma(-ei, ii, gr);
                        gi = coilmix_fma(er, ii, gi); gi = coilmix_fma(ei, ir, gi);
                    }
                    if (c == c2) gi = 0;
                    G[2 * (c * C + c2)] = gr; G[2 * (c * C + c2) + 1] = gi;
                    G[2 * (c2 * C + c)] = gr; G[2 * (c2 * C + c) + 1] = c == c2 ? R(0) : -gi;
                }
            for (int c = 0; c < C; ++c) {
                v[2 * c] = inorm[p] > 0 ? img[2 * (c * N + p)] / inorm[p] : (c == 0 ? R(1) : R(0));
                v[2 * c + 1] = inorm[p] > 0 ? img[2 * (c * N + p) + 1] / inorm[p] : R(0);
            }
            R l = 0;
            for (int it = 0; it < iters; ++it) {
                for (int c = 0; c < C; ++c) {
                    R ur = 0, ui = 0;
                    for (int c2 = 0; c2 < C; ++c2) {
                        const R gr = G[2 * (c * C + c2)], gi = G[2 * (c * C + c2) + 1];
                        ur = coilmix_fma(gr, v[2 * c2], ur); ur = coilmix_fma(-gi, v[2 * c2 + 1], ur);
                        ui = coilmix_fma(gr, v[2 * c2 + 1], ui); ui = coilmix_fma(gi, v[2 * c2], ui);
                    }
                    u[2 * c] = ur; u[2 * c + 1] = ui;
                }
                R s = 0;
                for (int c = 0; c < C; ++c) { s = coilmix_fma(u[2 * c], u[2 * c], s); s = coilmix_fma(u[2 * c + 1], u[2 * c + 1], s); }
                l = std::sqrt(s);
                if (l > 0) for (int c = 0; c < 2 * C; ++c) v[c] = u[c] / l;
            }
            REQUIRE(same(l, lam[p]));
            const bool keep = l >= (R)crop && inorm[p] >= (R)thresh * imax;
            double n2 = 0.0, gre = 0.0, gim = 0.0;
            for (int c = 0; c < C; ++c) {
                const double mr = maps[2 * (c * N + p)], mi = maps[2 * (c * N + p) + 1];
                if (!keep) { REQUIRE(same((R)mr, R(0)) && same((R)mi, R(0))); continue; }
                n2 += mr * mr + mi * mi;
                gre += mr * img[2 * (c * N + p)] + mi * img[2 * (c * N + p) + 1];
                gim += mr * img[2 * (c * N + p) + 1] - mi * img[2 * (c * N + p)];
            }
            if (keep) {
                const double eps = sizeof(R) == 8 ? 2.3e-16 : 1.2e-7;
                REQUIRE(std::fabs(n2 - 1.0) <= 8 * C * eps);
                REQUIRE(gre >= 0.0 && std::fabs(gim) <= 8 * C * eps * std::fabs(gre));
                ++inside;
            } else ++outside;
        }
    REQUIRE(inside > 0);
    if (crop > 0.0 || thresh > 0.0) REQUIRE(outside > 0);
}

static int run_slice() {
    for (int C : {1, 3, 5})
        for (int k : {2, 3})
            for (int it : {1, 3}) {
                slice_case<float>(C, k, it, 0.0, 0.0, 100 * C + 10 * k + it);
                slice_case<double>(C, k, it, 0.0, 0.0, 100 * C + 10 * k + it);
                slice_case<float>(C, k, it, 0.9, 0.3, 100 * C + 10 * k + it);
                slice_case<double>(C, k, it, 0.9, 0.3, 100 * C + 10 * k + it);
            }
    puts("ok slice");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "check")) return run_check();
    if (!strcmp(argv[1], "index")) return run_index();
    if (!strcmp(argv[1], "gram")) return run_gram();
    if (!strcmp(argv[1], "kernels")) return run_kernels();
    if (!strcmp(argv[1], "slice")) return run_slice();
    return 2;
}
