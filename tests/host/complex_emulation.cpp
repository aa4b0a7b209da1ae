// Host emulation of kernels_complex.hip: csoft / cclip / the two complex steps of csrc/prox_ops.h and the work-item functions of
// csrc/wavelet_plan.h instantiated on Cpx<S>, run under g++ (plain and with the sanitizers) against long-hand loops:
//   scalar cases   u = 0, |u| == c exactly, |z| == ib exactly, denormal components, +-0, and the prox identity z + c z / |z| = u; against
//                  the same formulas in long double
//   wavelet prox   tile by tile and item by item with LDS arrays of exactly the plan's sizes (poisoned with NaN), L1 and CNC: an EQUALITY
//                  OF THE TWO INSTANTIATIONS, not an independent reference -- the Cpx<S> instance of the item functions against their
//                  REAL instance run on the real and the imaginary plane, bit for bit, every pixel written exactly once.  Only the
//                  threshold between the two transforms is written out long hand.  A defect shared by both instantiations would pass
//                  here; the real instance is held against the whole-image NumPy oracle by tests/host/wavelet_emulation.cpp, and the
//                  complex kernels against tests/complex_oracle.py by tests/test_gpu_complex.py
// Prints one line per case and "ok"; a mismatch is a non-zero exit.  No input files.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pnp_admm_cnc_mri_amd/csrc/prox_ops.h"
#include "../../pnp_admm_cnc_mri_amd/csrc/wavelet_plan.h"

using namespace pnp;

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static double rnd() {                  // uniform in (-1, 1)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((g_seed >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0;
}

template <typename S> static bool same_bits(S a, S b) { return memcmp(&a, &b, sizeof(S)) == 0; }

// ---- scalar cases -------------------------------------------------------------------------------------------------------------------
template <typename S> static void scalar_cases(const char* name) {
    const S eps = std::numeric_limits<S>::epsilon(), den = std::numeric_limits<S>::denorm_min();
    // u = 0, with both signs of zero: s = 0, the result is a zero of the component's sign
    for (S zr : {S(0), -S(0)}) for (S zi : {S(0), -S(0)}) {
        const Cpx<S> r = csoft(Cpx<S>(zr, zi), S(0.25));
        EXPECT(r.re == S(0) && r.im == S(0) && std::signbit(r.re) == std::signbit(zr) && std::signbit(r.im) == std::signbit(zi), "%s csoft(+-0)", name);
        const Cpx<S> r0 = csoft(Cpx<S>(zr, zi), S(0));                    // c = 0 and m = 0: m > c is false
        EXPECT(r0.re == S(0) && r0.im == S(0), "%s csoft(0, 0)", name);
        const Cpx<S> cl = cclip(Cpx<S>(zr, zi), S(0.25));
        EXPECT(same_bits(cl.re, zr) && same_bits(cl.im, zi), "%s cclip(+-0)", name);
    }
    // |u| == c exactly (3-4-5 scaled by powers of two): zero; one ulp above: not zero
    for (S k : {S(1), S(0.125), S(1024)}) {
        const Cpx<S> r = csoft(Cpx<S>(S(3) * k, -S(4) * k), S(5) * k);
        EXPECT(r.re == S(0) && r.im == S(0), "%s csoft(|u| == c)", name);
        const Cpx<S> r1 = csoft(Cpx<S>(S(3) * k, -S(4) * k), std::nextafter(S(5) * k, S(0)));
        EXPECT(r1.re > S(0) && r1.im < S(0) && std::isfinite(r1.re) && std::isfinite(r1.im), "%s csoft(|u| just above c)", name);
        const Cpx<S> cl = cclip(Cpx<S>(S(3) * k, -S(4) * k), S(5) * k);   // |z| == ib exactly: z itself
        EXPECT(same_bits(cl.re, S(3) * k) && same_bits(cl.im, -S(4) * k), "%s cclip(|z| == ib)", name);
    }
    // denormal components: the squares underflow, m = 0, the result is 0 and finite -- never 0 / 0
    for (S c : {S(0), den, S(0.1)}) {
        const Cpx<S> r = csoft(Cpx<S>(den, -S(3) * den), c);
        EXPECT(r.re == S(0) && r.im == S(0), "%s csoft(denormal)", name);
        const Cpx<S> cl = cclip(Cpx<S>(den, -S(3) * den), c);
        EXPECT(std::isfinite(cl.re) && std::isfinite(cl.im), "%s cclip(denormal)", name);
    }
    // random values against long double, and the prox identity z + c z / |z| = u where z != 0
    double worst = 0.0, worst_id = 0.0, worst_clip = 0.0;
    for (int i = 0; i < 20000; ++i) {
        const Cpx<S> u((S)rnd(), (S)rnd());
        const S c = (S)(0.5 * std::fabs(rnd()));
        const long double m = sqrtl((long double)u.re * u.re + (long double)u.im * u.im);
        const Cpx<S> z = csoft(u, c);
        const long double s = m > c ? (m - c) / m : 0.0L;
        const S mS = cpx_abs(u);
        if (std::fabs((double)(m - (long double)c)) > 4 * (double)eps) {                 // away from the threshold: the branch is the same
            EXPECT((mS > c) == (m > c), "%s branch", name);
            const double d = std::hypot((double)(z.re - (S)(s * u.re)), (double)(z.im - (S)(s * u.im)));
            worst = std::fmax(worst, d / (double)(m > 0 ? m : 1));
        }
        if (z.re != S(0) || z.im != S(0)) {
            const long double mz = sqrtl((long double)z.re * z.re + (long double)z.im * z.im);
            const double d = std::hypot((double)(z.re + c * z.re / mz - u.re), (double)(z.im + c * z.im / mz - u.im));
            worst_id = std::fmax(worst_id, d);
        }
        const Cpx<S> cl = cclip(u, c);
        const long double mc = sqrtl((long double)cl.re * cl.re + (long double)cl.im * cl.im);
        if (mS > c) worst_clip = std::fmax(worst_clip, std::fabs((double)(mc - (long double)c)));
        else EXPECT(same_bits(cl.re, u.re) && same_bits(cl.im, u.im), "%s cclip inside", name);
        // z - csoft(z, ib) = cclip(z, ib) up to rounding
        const double d2 = std::hypot((double)(u.re - z.re - cl.re), (double)(u.im - z.im - cl.im));
        EXPECT(d2 <= 8 * (double)eps, "%s u - csoft(u) vs cclip(u): %g", name, d2);
    }
    // (m - c) / m and two products: a few ulp of |u|; |u| < 2
    EXPECT(worst <= 8 * (double)eps, "%s csoft vs long double: %g", name, worst);
    EXPECT(worst_id <= 16 * (double)eps, "%s prox identity: %g", name, worst_id);
    EXPECT(worst_clip <= 8 * (double)eps, "%s |cclip| - ib: %g", name, worst_clip);
    // zero imaginary parts: the complex steps are the real ones up to the rounding of (m - c) / m and ib / m
    const ProxParamsT<S> p{(S)0.0225, (S)0.55, (S)0.45, (S)1.44, (S)(1.0 / 64)};
    double worst_real = 0.0;
    for (int i = 0; i < 20000; ++i) {
        const S x = (S)rnd(), z0 = (S)(0.05 * rnd()), w0 = (S)(0.3 * rnd());
        Cpx<S> z(z0, S(0)), w(w0, S(0));
        prox_cnc_cx(Cpx<S>(x, S(0)), z, w, p);
        const S u = x + w0, clip = z0 < -p.ib ? -p.ib : (z0 > p.ib ? p.ib : z0);
        const S t = cpx_fma(p.c1, z0, cpx_fma(p.c2, u, p.c3 * clip));
        const S mm = std::fabs(t) - p.thr, r = mm > S(0) ? mm : S(0), zr = t < S(0) ? -r : r;
        EXPECT(z.im == S(0) && w.im == S(0), "%s imaginary part of a real step", name);
        worst_real = std::fmax(worst_real, std::fmax(std::fabs((double)(z.re - zr)), std::fabs((double)(w.re - (u - zr)))));
    }
    EXPECT(worst_real <= 8 * (double)eps, "%s real reduction: %g", name, worst_real);
    printf("%s scalar: csoft %.2e, identity %.2e, clip %.2e, real reduction %.2e\n", name, worst, worst_id, worst_clip, worst_real);
}

// ---- the wavelet prox on Cpx<S> against the real instances on the two planes ----------------------------------------------------------
template <typename V, int T, typename Emit>
static void fwd_image(const WvTile& t, const V* in0, const V* in1, V poison, Emit&& emit) {
    std::vector<V> rowbuf(wv_fwd_rowbuf_elems(T, t.L, t.tile), poison), ll(wv_fwd_ll_elems(T, t.L, t.tile), poison);
    for (int l = 0; l < t.L; ++l) {
        for (int it = 0, n = wv_fwd_row_items(T, t, l); it < n; ++it) wv_fwd_row_item<V, T>(it, l, t, in0, in1, ll.data(), rowbuf.data());
        for (int it = 0, n = wv_fwd_col_items(T, t, l); it < n; ++it) wv_fwd_col_item<V, T>(it, l, t, rowbuf.data(), ll.data(), emit);
    }
}
template <typename V, int T, typename Emit>
static void inv_image(const WvTile& t, const V* coef, V poison, Emit&& emit) {
    std::vector<V> colbuf(wv_inv_colbuf_elems(T, t.tile), poison), ll(wv_inv_ll_elems(T, t.tile), poison);
    for (int l = t.L - 1; l >= 0; --l) {
        for (int it = 0, n = wv_inv_col_items(T, t, l); it < n; ++it) wv_inv_col_item<V, T>(it, l, t, coef, ll.data(), colbuf.data());
        for (int it = 0, n = wv_inv_row_items(T, t, l); it < n; ++it) wv_inv_row_item<V, T>(it, l, t, colbuf.data(), ll.data(), emit);
    }
}
template <typename F> static void for_tiles(int H, int W, int L, int tile, F&& f) {
    for (int ty = 0; ty < wv_tiles(H, tile); ++ty)
        for (int tx = 0; tx < wv_tiles(W, tile); ++tx) f(WvTile{H, W, L, tile, ty * tile, tx * tile, 0});
}

template <typename S, int T> static void wavelet_case(const char* name, int L, int H, int W, bool cnc) {
    const size_t n = (size_t)H * W;
    const S nan = std::numeric_limits<S>::quiet_NaN();
    const Cpx<S> cnan(nan, nan);
    const int tile = wv_tile(T, L);
    EXPECT(wv_check(T == 2 ? WV_HAAR : T == 4 ? WV_DB2 : WV_DB4, L, H, W) == WV_OK, "wv_check");
    const ProxParamsT<S> p{(S)0.225, (S)0.55, (S)0.45, (S)0.9, (S)0.25};
    std::vector<Cpx<S>> x(n), z(n), w(n), coef(n, cnan), zn(n, cnan), wn(n, cnan);
    for (size_t i = 0; i < n; ++i) { x[i] = Cpx<S>((S)rnd(), (S)rnd()); z[i] = Cpx<S>((S)(0.5 * rnd()), (S)(0.5 * rnd())); w[i] = Cpx<S>((S)(0.3 * rnd()), (S)(0.3 * rnd())); }
    // the complex instance, as the kernels run it
    for_tiles(H, W, L, tile, [&](const WvTile& t) {
        if (cnc) {
            fwd_image<Cpx<S>, T>(t, z.data(), (const Cpx<S>*)nullptr, cnan, [&](size_t o, Cpx<S> v, bool) { coef[o] = v; });
            fwd_image<Cpx<S>, T>(t, x.data(), w.data(), cnan, [&](size_t o, Cpx<S> v, bool detail) {
                const Cpx<S> cz = coef[o];
                if (detail) coef[o] = csoft(cnc_combine_cx(cz, v, p), p.thr);
                else        coef[o] = Cpx<S>(cpx_fma(p.c1, cz.re, p.c2 * v.re), cpx_fma(p.c1, cz.im, p.c2 * v.im));
            });
        } else {
            fwd_image<Cpx<S>, T>(t, x.data(), w.data(), cnan, [&](size_t o, Cpx<S> v, bool detail) { coef[o] = detail ? csoft(v, p.thr) : v; });
        }
    });
    std::vector<char> seen(n, 0);
    int twice = 0;
    for_tiles(H, W, L, tile, [&](const WvTile& t) {
        inv_image<Cpx<S>, T>(t, coef.data(), cnan, [&](size_t i, Cpx<S> v) {
            twice += seen[i]++;
            const Cpx<S> u = x[i] + w[i];
            zn[i] = v;
            wn[i] = u - v;
        });
    });
    EXPECT(twice == 0, "%s: %d pixels written twice", name, twice);
    for (size_t i = 0; i < n; ++i) if (!seen[i]) { EXPECT(false, "%s: pixel %zu not written", name, i); break; }
    // long hand: the real instances on the planes, the threshold by a plain loop over the coefficients
    std::vector<S> pl[2][3], cu[2], cz[2], out[2];
    for (int k = 0; k < 2; ++k) {
        for (int a = 0; a < 3; ++a) pl[k][a].resize(n);
        for (size_t i = 0; i < n; ++i) { pl[k][0][i] = k ? x[i].im : x[i].re; pl[k][1][i] = k ? z[i].im : z[i].re; pl[k][2][i] = k ? w[i].im : w[i].re; }
        cu[k].assign(n, nan); cz[k].assign(n, nan); out[k].assign(n, nan);
        for_tiles(H, W, L, tile, [&](const WvTile& t) {
            fwd_image<S, T>(t, pl[k][0].data(), pl[k][2].data(), nan, [&](size_t o, S v, bool) { cu[k][o] = v; });
            if (cnc) fwd_image<S, T>(t, pl[k][1].data(), (const S*)nullptr, nan, [&](size_t o, S v, bool) { cz[k][o] = v; });
        });
    }
    std::vector<S> th[2] = {std::vector<S>(n), std::vector<S>(n)};
    for (int yy = 0; yy < H; ++yy)
        for (int xx = 0; xx < W; ++xx) {
            const size_t o = (size_t)yy * W + xx;
            const bool detail = wv_is_detail(yy, xx, H, W, L);
            S tr = cu[0][o], ti = cu[1][o];
            if (cnc) {
                S clr = cz[0][o], cli = cz[1][o];
                const S m = std::sqrt(clr * clr + cli * cli);
                if (detail && m > p.ib) { const S f = p.ib / m; clr = clr * f; cli = cli * f; }
                if (detail) { tr = cpx_fma(p.c1, cz[0][o], cpx_fma(p.c2, cu[0][o], p.c3 * clr)); ti = cpx_fma(p.c1, cz[1][o], cpx_fma(p.c2, cu[1][o], p.c3 * cli)); }
                else        { tr = cpx_fma(p.c1, cz[0][o], p.c2 * cu[0][o]); ti = cpx_fma(p.c1, cz[1][o], p.c2 * cu[1][o]); }
            }
            if (detail) {
                const S m = std::sqrt(tr * tr + ti * ti), s = m > p.thr ? (m - p.thr) / m : S(0);
                tr = s * tr; ti = s * ti;
            }
            th[0][o] = tr; th[1][o] = ti;
        }
    for (int k = 0; k < 2; ++k)
        for_tiles(H, W, L, tile, [&](const WvTile& t) { inv_image<S, T>(t, th[k].data(), nan, [&](size_t i, S v) { out[k][i] = v; }); });
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        const S ur = x[i].re + w[i].re, ui = x[i].im + w[i].im;
        if (!same_bits(zn[i].re, out[0][i]) || !same_bits(zn[i].im, out[1][i]) || !same_bits(wn[i].re, (S)(ur - out[0][i])) ||
            !same_bits(wn[i].im, (S)(ui - out[1][i])) || !std::isfinite(zn[i].re) || !std::isfinite(zn[i].im)) ++bad;
    }
    EXPECT(bad == 0, "%s: %zu pixels differ from the long-hand planes", name, bad);
    printf("%s T=%d L=%d %dx%d %s: tile %d, LDS %zu / %zu bytes, %zu differ\n", name, T, L, H, W, cnc ? "cnc" : "l1", tile,
           wv_fwd_lds_elems(T, L, tile) * sizeof(Cpx<S>), wv_inv_lds_elems(T, tile) * sizeof(Cpx<S>), bad);
}

template <typename S> static void wavelet_cases(const char* name) {
    for (int cnc = 0; cnc < 2; ++cnc) {
        wavelet_case<S, 2>(name, 1, 128, 128, cnc);
        wavelet_case<S, 2>(name, 3, 128, 160, cnc);
        wavelet_case<S, 4>(name, 1, 128, 130, cnc);
        wavelet_case<S, 4>(name, 3, 136, 128, cnc);
        wavelet_case<S, 8>(name, 1, 128, 128, cnc);
        wavelet_case<S, 8>(name, 3, 128, 160, cnc);
    }
}

int main() {
    static_assert(sizeof(Cpx<float>) == 8 && alignof(Cpx<float>) == 8 && sizeof(Cpx<double>) == 16 && alignof(Cpx<double>) == 16, "Cpx layout");
    scalar_cases<float>("float");
    scalar_cases<double>("double");
    wavelet_cases<float>("float");
    wavelet_cases<double>("double");
    if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
