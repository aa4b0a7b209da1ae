// g++ emulation of the host-testable parts of the coil map estimation (csrc/coilmaps_plan.h):
//   coilmaps_emulation slice        coilmaps_slice (start, power steps, phase, support) against a third, long-hand loop written here with
//                                   std::complex-free scalar code, bit for bit, in float and double, C = 1, 3, 5, r = 0 .. 3, n = 1 .. 3 on
//                                   a small wrapped image; then the properties: unit norm inside the support, exact +0 outside, v^H I(p)
//                                   real and >= 0, r = 0 / n = 1 is I / ||I||.
//   coilmaps_emulation tiles H W    the tile choice for every (C, r, precision): the largest tile within 64 KiB, else the smallest within
//                                   128 KiB; the odd slot stride; the staging walk of k_coil_eigmaps fills every staged (pixel, coil) once;
//                                   every patch read of every thread of the four corner tiles stays inside the staged image and lands on
//                                   the pixel coilmaps_patch_index names; every image pixel is owned by exactly one thread.
//   coilmaps_emulation window       the window's symmetry w(f) = w(-f), w(0) = 1, 0 < w <= 1; coilmaps_line_of inverts coilmix_cal_line;
//                                   coilmaps_window_slice: zeros outside the region, the lowest missing point; the pass / scratch layout.
//   coilmaps_emulation check        every rule of coilmaps_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../pnp_admm_cnc_mri_amd/csrc/coilmaps_plan.h"

using namespace pnp;

static float  fm(float a, float b, float c) { return std::fmaf(a, b, c); }
static double fm(double a, double b, double c) { return std::fma(a, b, c); }
static float  sq(float a) { return std::sqrt(a); }
static double sq(double a) { return std::sqrt(a); }

template <typename R> static bool same(R a, R b) { return memcmp(&a, &b, sizeof(R)) == 0; }

// the long-hand loop: separate re / im planes, explicit wrap, no helper of the plan
template <typename R>
static void longhand(const std::vector<R>& re, const std::vector<R>& im, int C, int H, int W, int r, int iters, double thresh,
                     std::vector<R>& mre, std::vector<R>& mim, std::vector<R>& lam) {
    const int N = H * W;
    R lmax = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int p = y * W + x;
            std::vector<R> vr(C), vi(C), ur(C), ui(C);
            R s = 0;
            for (int c = 0; c < C; ++c) { s = fm(re[c * N + p], re[c * N + p], s); s = fm(im[c * N + p], im[c * N + p], s); }
            const R nrm = sq(s);
            for (int c = 0; c < C; ++c) {
                vr[c] = nrm > 0 ? re[c * N + p] / nrm : (c == 0 ? R(1) : R(0));
                vi[c] = nrm > 0 ? im[c * N + p] / nrm : R(0);
            }
            R l = 0;
            for (int it = 0; it < iters; ++it) {
                for (int c = 0; c < C; ++c) { ur[c] = 0; ui[c] = 0; }
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const int yy = ((y + dy) % H + H) % H, xx = ((x + dx) % W + W) % W, o = yy * W + xx;
                        R gr = 0, gi = 0;
                        for (int c = 0; c < C; ++c) {          // g += conj(I_c) v_c
                            gr = fm(re[c * N + o], vr[c], gr); gr = fm(im[c * N + o], vi[c], gr);
                            gi = fm(re[c * N + o], vi[c], gi); gi = fm(-im[c * N + o], vr[c], gi);
                        }
                        for (int c = 0; c < C; ++c) {          // u_c += I_c g
                            ur[c] = fm(re[c * N + o], gr, ur[c]); ur[c] = fm(-im[c * N + o], gi, ur[c]);
                            ui[c] = fm(re[c * N + o], gi, ui[c]); ui[c] = fm(im[c * N + o], gr, ui[c]);
                        }
                    }
                s = 0;
                for (int c = 0; c < C; ++c) { s = fm(ur[c], ur[c], s); s = fm(ui[c], ui[c], s); }
                l = sq(s);
                if (l > 0) for (int c = 0; c < C; ++c) { vr[c] = ur[c] / l; vi[c] = ui[c] / l; }
            }
            R gr = 0, gi = 0;
            for (int c = 0; c < C; ++c) {                      // g += conj(v_c) I_c
                gr = fm(vr[c], re[c * N + p], gr); gr = fm(vi[c], im[c * N + p], gr);
                gi = fm(vr[c], im[c * N + p], gi); gi = fm(-vi[c], re[c * N + p], gi);
            }
            const R m = sq(fm(gr, gr, gi * gi));
            if (m > 0) {
                const R er = gr / m, ei = gi / m;
                for (int c = 0; c < C; ++c) {
                    const R a = fm(-vi[c], ei, vr[c] * er), b = fm(vi[c], er, vr[c] * ei);
                    vr[c] = a; vi[c] = b;
                }
            }
            for (int c = 0; c < C; ++c) { mre[c * N + p] = vr[c]; mim[c * N + p] = vi[c]; }
            lam[p] = l;
            if (l > lmax) lmax = l;
        }
    const R bar = (R)(thresh * thresh) * lmax;
    for (int p = 0; p < N; ++p)
        if (!(lam[p] >= bar)) for (int c = 0; c < C; ++c) { mre[c * N + p] = 0; mim[c * N + p] = 0; }
}

template <typename R>
static int slice_case(int C, int H, int W, int r, int iters, double thresh, unsigned seed) {
    const int N = H * W;
    std::mt19937 gen(seed);
    std::normal_distribution<double> g(0.0, 1.0);
    std::vector<R> img(2 * (size_t)C * N), re((size_t)C * N), im((size_t)C * N);
    for (int c = 0; c < C; ++c)
        for (int p = 0; p < N; ++p) {
            const double env = (p % W < W / 2) ? 1e-3 : 1.0;              // a dim band: some pixels fall below the support bar
            re[c * N + p] = (R)(env * g(gen)); im[c * N + p] = (R)(env * g(gen));
            if (p == 5) { re[c * N + p] = 0; im[c * N + p] = 0; }         // a pixel where every coil is 0
            img[2 * ((size_t)c * N + p)] = re[c * N + p]; img[2 * ((size_t)c * N + p) + 1] = im[c * N + p];
        }
    std::vector<R> maps(2 * (size_t)C * N), lam(N), mre((size_t)C * N), mim((size_t)C * N), lam2(N);
    coilmaps_slice<R>(img.data(), C, H, W, r, iters, thresh, maps.data(), lam.data());
    longhand<R>(re, im, C, H, W, r, iters, thresh, mre, mim, lam2);
    const R eps = sizeof(R) == 8 ? (R)2.220446049250313e-16 : (R)1.1920929e-7f;
    int kept = 0;
    for (int p = 0; p < N; ++p) {
        if (!same(lam[p], lam2[p])) return 2;
        R n2 = 0, gr = 0, gi = 0;
        bool zero = true;
        for (int c = 0; c < C; ++c) {
            const R a = maps[2 * ((size_t)c * N + p)], b = maps[2 * ((size_t)c * N + p) + 1];
            if (!same(a, mre[c * N + p]) || !same(b, mim[c * N + p])) return 2;
            n2 += a * a + b * b;
            gr += a * re[c * N + p] + b * im[c * N + p];
            gi += a * im[c * N + p] - b * re[c * N + p];
            if (!same(a, R(0)) || !same(b, R(0))) zero = false;          // +0 exactly
        }
        if (zero) continue;
        ++kept;
        R scale = 0;
        for (int c = 0; c < C; ++c) scale += std::fabs(re[c * N + p]) + std::fabs(im[c * N + p]);
        if (std::fabs(n2 - 1) > 8 * C * eps) return 3;
        if (gr < 0 || std::fabs(gi) > 8 * C * eps * scale) return 4;
        if (r == 0 && iters == 1) {                                       // I / ||I||, up to the rounding of the two normalisations
            R s = 0;
            for (int c = 0; c < C; ++c) s += re[c * N + p] * re[c * N + p] + im[c * N + p] * im[c * N + p];
            for (int c = 0; c < C; ++c)
                if (std::fabs(maps[2 * ((size_t)c * N + p)] - re[c * N + p] / sq(s)) > 16 * C * eps) return 5;
        }
    }
    if (thresh > 0 && (kept == 0 || kept == N)) return 6;                // the case is built to have both kinds of pixel
    if (thresh == 0 && kept != N) return 7;                               // lambda >= 0 everywhere: nothing is dropped, e_0 at the all-zero pixel
    return 0;
}

static int slice() {
    unsigned seed = 1;
    for (int C : {1, 3, 5})
        for (int r = 0; r <= COILMAPS_MAX_RADIUS; ++r)
            for (int it = 1; it <= 3; ++it)
                for (double th : {0.0, 0.05}) {
                    if (int rc = slice_case<float>(C, 9, 16, r, it, th, seed++)) { fprintf(stderr, "float C=%d r=%d n=%d th=%g: %d\n", C, r, it, th, rc); return rc; }
                    if (int rc = slice_case<double>(C, 9, 16, r, it, th, seed++)) { fprintf(stderr, "double C=%d r=%d n=%d th=%g: %d\n", C, r, it, th, rc); return rc; }
                }
    puts("ok slice");
    return 0;
}

static int tiles(int H, int W) {
    for (int f64 = 0; f64 < 2; ++f64)
        for (int C = 1; C <= COIL_MAX_C; ++C)
            for (int r = 0; r <= COILMAPS_MAX_RADIUS; ++r) {
                const int CB = coilmix_out_bucket(C), k = coilmaps_tile_choice(C, r, f64);
                if (CB < C || k < 0 || k >= COILMAPS_TILES) return 2;
                const CoilmapsTile t = coilmaps_tile_at(k);
                const int PH = t.th + 2 * r, PW = t.tw + 2 * r, slots = coilmaps_stride_slots(CB, f64);
                const size_t cx = f64 ? 16 : 8, foot = (size_t)PH * PW * CB * cx;
                if (coilmaps_footprint(t, r, CB, f64) != foot) return 2;
                bool any_fits = false;
                for (int j = 0; j < COILMAPS_TILES; ++j) {
                    const CoilmapsTile u = coilmaps_tile_at(j);
                    const bool fits = (size_t)(u.th + 2 * r) * (u.tw + 2 * r) * CB * cx <= 64 * 1024;
                    if (fits && !any_fits && j != k) return 3;            // the first (largest) tile that fits is the choice
                    any_fits = any_fits || fits;
                    if (j > 0 && u.th * u.tw >= coilmaps_tile_at(j - 1).th * coilmaps_tile_at(j - 1).tw) return 3;
                }
                if (!any_fits && (k != COILMAPS_TILES - 1 || foot > 128 * 1024 || !(C > 16 && f64 && r == 3))) return 3;
                if (slots % 2 != 1 || (size_t)slots * 16 < CB * cx || (size_t)slots * 16 > CB * cx + 16) return 4;
                if (coilmaps_lds_bytes(t, r, CB, f64) != (size_t)PH * PW * slots * 16 || coilmaps_lds_bytes(t, r, CB, f64) > COILMAPS_LDS_HARD) return 4;
                if (t.th * t.tw > 256 || t.th * t.tw % 32) return 4;
                if (C != 1 && C != 5 && C != 32 && C != 17) continue;     // the walks below: one C per bucket is enough
                const int ty = coilmaps_tiles_y(H, t), tx = coilmaps_tiles_x(W, t), threads = t.th * t.tw;
                for (int by : {0, ty - 1})
                    for (int bx : {0, tx - 1}) {
                        const int y0 = by * t.th, x0 = bx * t.tw;
                        std::vector<long> staged((size_t)PH * PW * CB, -1);          // [pixel][coil] -> the image pixel it holds
                        for (int tid = 0; tid < threads; ++tid)
                            for (int idx = tid; idx < C * PH * PW; idx += threads) {
                                const int c = idx / (PH * PW), pix = idx % (PH * PW);
                                const size_t o = coilmaps_staged_pixel(pix / PW, pix % PW, y0, x0, r, H, W);
                                if (o >= (size_t)H * W || staged.at((size_t)pix * CB + c) != -1) return 5;
                                staged.at((size_t)pix * CB + c) = (long)o;
                            }
                        for (int pix = 0; pix < PH * PW; ++pix)
                            for (int c = 0; c < CB; ++c) if ((staged[(size_t)pix * CB + c] != -1) != (c < C)) return 5;
                        for (int tid = 0; tid < threads; ++tid) {
                            const int ly = tid / t.tw, lx = tid % t.tw, centre = (ly + r) * PW + lx + r;
                            int q = 0;
                            for (int dy = -r; dy <= r; ++dy)
                                for (int dx = -r; dx <= r; ++dx, ++q) {
                                    const int at = centre + dy * PW + dx;
                                    if (at < 0 || at >= PH * PW) return 6;
                                    int ody, odx;
                                    coilmaps_patch_offset(q, r, ody, odx);
                                    if (ody != dy || odx != dx) return 6;
                                    // threads of a remainder tile work on wrapped pixels: the same identity holds for them
                                    if ((size_t)staged[(size_t)at * CB] != coilmaps_patch_index(q, r, coilmaps_wrap(y0 + ly, H), coilmaps_wrap(x0 + lx, W), H, W)) return 6;
                                }
                            if (q != coilmaps_patch_points(r)) return 6;
                        }
                    }
                std::vector<uint8_t> owner((size_t)H * W, 0);
                for (int by = 0; by < ty; ++by)
                    for (int bx = 0; bx < tx; ++bx)
                        for (int tid = 0; tid < threads; ++tid) {
                            const int y = by * t.th + tid / t.tw, x = bx * t.tw + tid % t.tw;
                            if (y < H && x < W) ++owner.at((size_t)y * W + x);
                        }
                for (uint8_t v : owner) if (v != 1) return 7;
            }
    printf("ok tiles %d %d\n", H, W);
    return 0;
}

static int window() {
    for (int ncal = COILMIX_NCAL_MIN; ncal <= COILMIX_NCAL_MAX; ++ncal) {
        if (coilmaps_window(0, ncal) != 1.0) return 2;
        for (int i = 0; i < ncal; ++i) {
            const int f = coilmaps_freq(i, ncal);
            const double w = coilmaps_window(i, ncal);
            if (f < -(ncal / 2) || f > (ncal - 1) / 2 || !(w > 0.0) || !(w <= 1.0)) return 2;
            if (f > 0 && f <= ncal / 2 && coilmaps_window(ncal - f, ncal) != w) return 2;          // w(f) = w(-f), to the bit
            const double ref = 0.5 * (1.0 + cos(2.0 * M_PI * f / (ncal + 1)));                     // cos^2 a = (1 + cos 2a) / 2
            if (fabs(w - ref) > 1e-15) return 2;
            if (coilmaps_window_table<float>(ncal).w[i] != (float)w || coilmaps_window_table<double>(ncal).w[i] != w) return 2;
        }
        for (int n : {128, 131, 1024}) {
            if (ncal > n) continue;
            int seen = 0;
            for (int h = 0; h < n; ++h) {
                const int i = coilmaps_line_of(h, ncal, n);
                if (i >= ncal) return 3;
                if (i >= 0) { ++seen; if (coilmix_cal_line(i, ncal, n) != h) return 3; }
            }
            if (seen != ncal) return 3;
        }
    }
    // the windowed slice: zeros outside, the lowest missing point
    const int H = 128, W = 131, C = 2, ncal = 5;
    const size_t N = (size_t)H * W;
    std::vector<float> y(2 * C * N, 1.0f), k(2 * C * N, -1.0f);
    std::vector<uint8_t> mask(N, 1);
    if (coilmaps_window_slice<float>(y.data(), mask.data(), C, H, W, ncal, k.data()) != -1) return 4;
    size_t nonzero = 0;
    for (size_t i = 0; i < k.size(); i += 2) {
        if (k[i] != k[i + 1] || k[i] < 0.0f) return 4;
        nonzero += k[i] != 0.0f;
    }
    if (nonzero != (size_t)C * ncal * ncal || k[0] != 1.0f) return 4;
    mask[(size_t)(H - 1) * W + 2] = 0;
    mask[(size_t)1 * W + (W - 2)] = 0;
    mask[(size_t)64 * W + 64] = 0;                                        // outside the region: not an error
    if (coilmaps_window_slice<float>(y.data(), mask.data(), C, H, W, ncal, k.data()) != (long)(1 * W + W - 2)) return 5;
    // passes and scratch
    if (coilmaps_pass_slices(3, 5, 3) != 1 || coilmaps_pass_slices(3, 5, 10) != 2 || coilmaps_pass_slices(3, 5, 64) != 3 || coilmaps_pass_slices(1, 32, 1) != 1) return 6;
    for (int f64 = 0; f64 < 2; ++f64) {
        const CoilmapsScratch s = coilmaps_scratch(7, 5, 12, N, f64);
        const size_t real = f64 ? 8 : 4;
        if (s.img != 0 || s.lambda < 2 * 5 * N * 2 * real || s.part < s.lambda + 2 * N * real || s.miss < s.part + 2 * coilmaps_spans(N) * real ||
            s.bytes < s.miss + 7 * 4 || s.lambda % 256 || s.part % 256 || s.miss % 256) return 6;
    }
    if (coilmaps_spans(128 * 128) != 4 || coilmaps_spans(131 * 128) != 5 || coilmaps_spans(1024 * 1024) > COILMAPS_SUP_THREADS) return 6;
    puts("ok window");
    return 0;
}

static int check() {
    if (coilmaps_check(1, 4, 0, 1, 0.0, 128, 128) || coilmaps_check(32, 64, 3, 16, 0.999, 1024, 1024) || coilmaps_check(5, 24, 2, 4, 0.05, 131, 140)) return 2;
    if (coilmaps_check(0, 24, 2, 4, 0.05, 128, 128) != COILMAPS_BAD_C || coilmaps_check(33, 24, 2, 4, 0.05, 128, 128) != COILMAPS_BAD_C) return 3;
    if (coilmaps_check(8, 3, 2, 4, 0.05, 128, 128) != COILMAPS_BAD_NCAL || coilmaps_check(8, 65, 2, 4, 0.05, 128, 128) != COILMAPS_BAD_NCAL) return 3;
    if (coilmaps_check(8, 24, -1, 4, 0.05, 128, 128) != COILMAPS_BAD_RADIUS || coilmaps_check(8, 24, 4, 4, 0.05, 128, 128) != COILMAPS_BAD_RADIUS) return 3;
    if (coilmaps_check(8, 24, 2, 0, 0.05, 128, 128) != COILMAPS_BAD_ITERS || coilmaps_check(8, 24, 2, 17, 0.05, 128, 128) != COILMAPS_BAD_ITERS) return 3;
    if (coilmaps_check(8, 24, 2, 4, -0.1, 128, 128) != COILMAPS_BAD_THRESH || coilmaps_check(8, 24, 2, 4, 1.0, 128, 128) != COILMAPS_BAD_THRESH ||
        coilmaps_check(8, 24, 2, 4, NAN, 128, 128) != COILMAPS_BAD_THRESH) return 3;
    if (coilmaps_check(8, 24, 2, 4, 0.05, 127, 128) != COILMAPS_BAD_SHAPE || coilmaps_check(8, 24, 2, 4, 0.05, 128, 1025) != COILMAPS_BAD_SHAPE) return 3;
    puts("ok check");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "slice")) return slice();
    if (argc == 4 && !strcmp(argv[1], "tiles")) return tiles(atoi(argv[2]), atoi(argv[3]));
    if (argc == 2 && !strcmp(argv[1], "window")) return window();
    if (argc == 2 && !strcmp(argv[1], "check")) return check();
    fprintf(stderr, "usage: coilmaps_emulation slice | tiles H W | window | check\n");
    return 1;
}
