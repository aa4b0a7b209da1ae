// Host emulation of kernels_pnp_cx.hip: the item functions of csrc/pnp_cx_ops.h -- the glue between a complex state and the real planes
// of a denoiser -- run under g++ (plain and with the sanitizers) as a stand-alone program:
//   modulus   m = 0 with both signs of zero and denormal components whose squares underflow: the result is (d, 0), never 0 / 0; negative d
//             is kept; |v| = 1 exactly returns (d re, d im); NaN and inf pass through as NaN; random values against long double
//   parts     the round trip (0.5 + g r - 0.5) / g against long double for several gains
//   dual      w+ = (w + x) - z from the unclipped values, the three projections onto the unit disc, values on the circle untouched
//   index map the kernels' thread -> element map (cx_den_vector / cx_den_threads / cx_den_span) for n = 0, 1, 2, 3 mod 4, both modes,
//             both arms: the loops of the kernels written out on arrays of exactly n (2 n) elements plus a guard, poisoned with NaN --
//             every element written exactly once, none outside, vector accesses only where they are 16-byte aligned
// Prints one line per case and "ok"; a mismatch is a non-zero exit.  No input files.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pnp_admm_cnc_mri_amd/csrc/pnp_cx_ops.h"

using namespace pnp;
typedef Cpx<float> Cf;

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static double rnd() {                  // uniform in (-1, 1)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((g_seed >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0;
}
static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

static void modulus_cases() {
    const float den = std::numeric_limits<float>::denorm_min(), nan = std::numeric_limits<float>::quiet_NaN(),
                inf = std::numeric_limits<float>::infinity();
    int n = 0;
    for (float d : {0.75f, -0.25f, 0.0f}) {
        for (float zr : {0.0f, -0.0f}) for (float zi : {0.0f, -0.0f}) {                       // m = 0, both signs of zero
            float p0 = nan, p1 = 7.0f;
            cx_den_split<CXD_MODULUS>(Cf(zr, zi), 0.5f, p0, p1);
            EXPECT(p0 == 0.0f && !std::signbit(p0) && p1 == 7.0f, "split(+-0)");
            const Cf r = cx_den_join<CXD_MODULUS>(d, nan, Cf(zr, zi), 0.5f);
            EXPECT(same_bits(r.re, d) && same_bits(r.im, 0.0f), "join(+-0) d=%g", d);
            ++n;
        }
        for (float k : {1.0f, 3.0f, 1.0e6f}) {                                               // squares underflow to 0: (d, 0)
            const Cf v(k * den, -2.0f * k * den);
            EXPECT(cpx_abs(v) == 0.0f, "denormal modulus");
            const Cf r = cx_den_join<CXD_MODULUS>(d, 0.0f, v, 0.5f);
            EXPECT(same_bits(r.re, d) && same_bits(r.im, 0.0f), "join(denormal) d=%g", d);
            ++n;
        }
        // a modulus that is itself tiny but not zero: finite, and (d / m) v is d times the phasor
        const Cf t(3.0e-20f, -4.0e-20f);
        const Cf rt = cx_den_join<CXD_MODULUS>(d, 0.0f, t, 0.5f);
        EXPECT(std::isfinite(rt.re) && std::isfinite(rt.im) && std::fabs(rt.re - 0.6f * d) <= 1e-6f && std::fabs(rt.im + 0.8f * d) <= 1e-6f, "join(tiny)");
        // |v| = 1 exactly: f = d, the products are d re, d im (0.6 / 0.8 are not exact in binary: use the axes and 2^-k pairs)
        for (Cf v : {Cf(1.0f, 0.0f), Cf(0.0f, -1.0f), Cf(-1.0f, -0.0f)}) {
            EXPECT(cpx_abs(v) == 1.0f, "|v| = 1");
            const Cf r = cx_den_join<CXD_MODULUS>(d, 0.0f, v, 0.5f);
            EXPECT(same_bits(r.re, d * v.re) && same_bits(r.im, d * v.im), "join(|v| = 1) d=%g", d);
            ++n;
        }
    }
    // negative d is not clamped: the result points the other way
    const Cf neg = cx_den_join<CXD_MODULUS>(-0.5f, 0.0f, Cf(0.0f, 2.0f), 0.5f);
    EXPECT(neg.re == 0.0f && neg.im == -0.5f, "negative d");
    // NaN / inf pass through as NaN, nothing traps
    for (Cf v : {Cf(nan, 0.25f), Cf(0.25f, nan), Cf(inf, 0.25f), Cf(0.25f, -inf)}) {
        const Cf r = cx_den_join<CXD_MODULUS>(0.5f, 0.0f, v, 0.5f);
        EXPECT(std::isnan(r.re) || std::isnan(r.im), "non-finite v");
        ++n;
    }
    const Cf rn = cx_den_join<CXD_MODULUS>(nan, 0.0f, Cf(0.3f, 0.4f), 0.5f);
    EXPECT(std::isnan(rn.re) && std::isnan(rn.im), "NaN d");
    const Cf rz = cx_den_join<CXD_MODULUS>(nan, 0.0f, Cf(0.0f, 0.0f), 0.5f);
    EXPECT(std::isnan(rz.re) && rz.im == 0.0f, "NaN d at m = 0");
    // random values against long double: |result| = |d| and the phase is v's, to a few roundings
    double worst = 0.0;
    for (int i = 0; i < 20000; ++i) {
        const Cf v((float)rnd(), (float)rnd());
        const float d = (float)rnd();
        const long double m = sqrtl((long double)v.re * v.re + (long double)v.im * v.im);
        if (m == 0.0L) continue;
        const Cf r = cx_den_join<CXD_MODULUS>(d, 0.0f, v, 0.5f);
        const long double er = fabsl(r.re - d * v.re / m), ei = fabsl(r.im - d * v.im / m);
        const double e = (double)((er > ei ? er : ei) / (fabsl(d) > 0 ? fabsl(d) : 1.0L));
        if (e > worst) worst = e;
    }
    EXPECT(worst <= 4.0 * std::numeric_limits<float>::epsilon(), "modulus join against long double: %g", worst);
    printf("modulus: %d special cases, worst random error %.2e of |d|\n", n, worst);
}

static void parts_cases() {
    double worst = 0.0;
    for (float g : {0.5f, 1.0f, 0.3f, 2.0f, 0.05f}) {
        for (int i = 0; i < 20000; ++i) {
            const Cf v((float)rnd(), (float)(2.0 * rnd()));
            float p0, p1;
            cx_den_split<CXD_PARTS>(v, g, p0, p1);
            EXPECT(std::fabs((long double)p0 - (0.5L + (long double)g * v.re)) <= 1.5L * std::numeric_limits<float>::epsilon() * (0.5L + fabsl((long double)g * v.re)), "split parts");
            const Cf r = cx_den_join<CXD_PARTS>(p0, p1, Cf(7.0f, 7.0f), g);       // the round trip of an identity network
            // one rounding of g r, one of the sum at magnitude <= 0.5 + |g r|, the subtraction is exact or nearly so: error <= ~eps (0.5 + |g r|) / g
            const long double tol = 2.0L * std::numeric_limits<float>::epsilon();
            const long double er = fabsl((long double)r.re - v.re) / ((0.5L + fabsl((long double)g * v.re)) / g);
            const long double ei = fabsl((long double)r.im - v.im) / ((0.5L + fabsl((long double)g * v.im)) / g);
            EXPECT(er <= tol && ei <= tol, "parts round trip g=%g: %Lg %Lg", g, er, ei);
            if ((double)er > worst) worst = (double)er;
            if ((double)ei > worst) worst = (double)ei;
        }
    }
    // exact cases: g = 0.5, dyadic values
    const Cf e = cx_den_join<CXD_PARTS>(0.75f, 0.25f, Cf(0.0f, 0.0f), 0.5f);
    EXPECT(e.re == 0.5f && e.im == -0.5f, "parts exact");
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const Cf n = cx_den_join<CXD_PARTS>(nan, 0.5f, Cf(0.0f, 0.0f), 0.5f);
    EXPECT(std::isnan(n.re) && n.im == 0.0f, "parts NaN plane");
    printf("parts: round trip within %.2e of (0.5 + |g r|) / g\n", worst);
}

static void dual_cases() {
    // z from an identity 'parts' network of v = x + w; then w+ = (w + x) - z = 0 where the round trip is exact
    Cf x(0.25f, -0.5f), z(9.0f, 9.0f), w(0.5f, 0.25f);
    const Cf v = x + w;
    float p0, p1;
    cx_den_split<CXD_PARTS>(v, 0.5f, p0, p1);
    cx_den_join_dual<CXD_PARTS>(p0, p1, v, 0.5f, x, z, w);
    EXPECT(x.re == 0.25f && x.im == -0.5f && z.re == 0.75f && z.im == -0.25f && w.re == 0.0f && w.im == 0.0f, "dual exact");
    // x outside the disc: w is formed from the UNCLIPPED x, x comes back on the circle
    Cf x2(3.0f, -4.0f), z2(0.0f, 0.0f), w2(0.0f, 0.0f);
    cx_den_join_dual<CXD_MODULUS>(10.0f, 0.0f, Cf(0.0f, 2.0f), 0.5f, x2, z2, w2);       // z = (0, 10) -> (0, 1); w+ = (3, -14) -> on the circle
    EXPECT(std::fabs(x2.re - 0.6f) <= 1e-7f && std::fabs(x2.im + 0.8f) <= 1e-7f, "dual clip x");
    EXPECT(z2.re == 0.0f && z2.im == 1.0f, "dual clip z");
    const float mw = sqrtf(3.0f * 3.0f + 14.0f * 14.0f);
    EXPECT(std::fabs(w2.re - 3.0f / mw) <= 1e-7f && std::fabs(w2.im + 14.0f / mw) <= 1e-7f, "dual w from unclipped x and z");
    // on the circle and inside: untouched, bit for bit
    Cf x3(1.0f, 0.0f), z3(0.0f, 0.0f), w3(-1.0f, 0.0f);
    cx_den_join_dual<CXD_MODULUS>(0.0f, 0.0f, Cf(0.0f, 0.0f), 0.5f, x3, z3, w3);
    EXPECT(same_bits(x3.re, 1.0f) && same_bits(z3.re, 0.0f) && same_bits(w3.re, 0.0f), "dual on the circle");
    printf("dual: ok\n");
}

// the loops of k_cx_den_in / k_cx_den_out[_dual] written out over the kernels' own index map; every store counts its element
template <int MODE> static void index_map(size_t n) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const int planes = MODE == CXD_PARTS ? 2 : 1;
    const bool vec = cx_den_vector(MODE, n);
    std::vector<Cf> v(n), z(n + 1, Cf(nan, nan));
    std::vector<float> p(planes * n + 1, nan);
    std::vector<int> hits_p(planes * n + 1, 0), hits_z(n + 1, 0);
    for (size_t i = 0; i < n; ++i) v[i] = Cf((float)rnd(), (float)rnd());
    const size_t threads = cx_den_threads(vec, n), launched = (threads + 255) / 256 * 256;
    int vector_groups = 0;
    for (size_t i = 0; i < launched; ++i) {                      // every thread of the grid, the idle ones of the last block too
        size_t e; int cnt;
        cx_den_span(vec, n, i, e, cnt);
        EXPECT(cnt >= 0 && cnt <= 4 && (cnt == 0 || e + cnt <= n), "span n=%zu i=%zu", n, i);
        if (i >= threads) EXPECT(cnt == 0, "idle thread with work n=%zu i=%zu", n, i);
        if (vec && cnt == 4) {
            ++vector_groups;
            EXPECT(e % 4 == 0 && (MODE != CXD_PARTS || (n + e) % 4 == 0), "vector access off 16 bytes n=%zu e=%zu", n, e);
        }
        for (int k = 0; k < cnt; ++k) {
            float p0 = nan, p1 = nan;
            cx_den_split<MODE>(v[e + k], 0.5f, p0, p1);
            p[e + k] = p0; ++hits_p[e + k];
            if (MODE == CXD_PARTS) { p[n + e + k] = p1; ++hits_p[n + e + k]; }
        }
        for (int k = 0; k < cnt; ++k) {                         // the join reads what the split wrote: an identity network
            z[e + k] = cx_den_join<MODE>(p[e + k], MODE == CXD_PARTS ? p[n + e + k] : 0.0f, v[e + k], 0.5f);
            ++hits_z[e + k];
        }
    }
    size_t bad = 0;
    for (size_t i = 0; i < planes * n; ++i) bad += hits_p[i] != 1 || std::isnan(p[i]);
    for (size_t i = 0; i < n; ++i) bad += hits_z[i] != 1 || std::isnan(z[i].re) || std::isnan(z[i].im);
    bad += hits_p[planes * n] != 0 || !std::isnan(p[planes * n]) || hits_z[n] != 0 || !std::isnan(z[n].re);
    EXPECT(bad == 0, "index map n=%zu mode=%d: %zu elements not written exactly once", n, MODE, bad);
    EXPECT(vec ? (size_t)vector_groups == n / 4 : vector_groups == 0, "vector groups n=%zu", n);
    // an identity network gives v back: modulus to a few roundings, parts within the round trip's bound
    double worst = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double e = std::fabs((double)z[i].re - v[i].re) + std::fabs((double)z[i].im - v[i].im);
        if (e > worst) worst = e;
    }
    EXPECT(worst <= 1e-6, "identity network n=%zu: %g", n, worst);
    printf("index map %s n = %zu (n mod 4 = %zu): %s arm, %zu threads, %zu bad\n", MODE == CXD_PARTS ? "parts" : "modulus", n, n % 4,
           vec ? "vector" : "scalar", threads, bad);
}

int main() {
    modulus_cases();
    parts_cases();
    dual_cases();
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)5, (size_t)1024, (size_t)1025, (size_t)1026, (size_t)1027, (size_t)16640,
                     (size_t)16899, (size_t)17030, (size_t)49920, (size_t)50697}) {
        index_map<CXD_MODULUS>(n);
        index_map<CXD_PARTS>(n);
    }
    if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
