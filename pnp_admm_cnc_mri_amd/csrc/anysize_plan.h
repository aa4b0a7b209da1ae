// Plan and butterfly arithmetic of the any-size FFT (kernels_anysize.hip): H, W in [128, 1024].
//
// Plain C++ with __host__ __device__ cores, so that the g++ emulation in tests/host/anysize_emulation.cpp runs the same
// factorisation, tables and butterflies on the CPU that the gfx950 kernels run.
//
//   7-smooth n (n = 2^a 3^b 5^c 7^d): one Stockham autosort transform of length n, radix-4 stages first, then 2, 3, 5, 7.
//   any other n (a prime factor > 7): Bluestein -- X_k = w_k sum_j (x_j w_j) conj(w_{k-j}), w_j = exp(-i pi j^2 / n) -- the
//   convolution done as a power-of-two transform of length m >= 2n - 1 (m <= 2048), the kernel's transform precomputed.
//
// Stockham stage s (radix r, Ns = product of the radices before it, L = transform length), butterfly j in [0, L/r):
//   k = j mod Ns;  v_q = in[j + q L/r] * W_{Ns r}^{q k};  V = DFT_r(v);  out[(j - k) r + k + q Ns] = V_q
// Every twiddle, the radix-r DFT's own roots included, is an entry of ONE table W_L^i = exp(-2 pi i i / L), i in [0, L),
// generated in fp64 on the host (W_{Ns r}^{q k} = W_L^{q k L / (Ns r)}, W_r^p = W_L^{p L / r}).
#pragma once
#include <math.h>
#include <vector>
#include "c2c_roles.h"

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__
#else
#define PNP_HD
#endif

namespace pnp {
namespace anysize {

constexpr int MIN_N = 128, MAX_N = 1024;
constexpr int MAX_M = 2048;         // longest transform: the Bluestein length of n = 1024 - k
constexpr int MAX_STAGES = 12;      // 2048 = 4^5 * 2: 6 stages; 7-smooth n <= 1024: at most 10 (2^10)

struct Plan {
    int n;                          // length of the line transform
    int bluestein;                  // 0: Stockham of length n; 1: Bluestein, Stockham of length m
    int m;                          // the Stockham length (n, or the power of two >= 2n - 1)
    int nstages;
    int radix[MAX_STAGES];
};

inline bool smooth7(int n) {
    if (n < 1) return false;
    for (int p : {2, 3, 5, 7}) while (n % p == 0) n /= p;
    return n == 1;
}

inline int bluestein_length(int n) {
    int m = 1;
    while (m < 2 * n - 1) m <<= 1;
    return m;
}

// radices of a 7-smooth L: 4s, then at most one 2, then 3s, 5s, 7s
inline int factor(int L, int* radix) {
    int s = 0;
    while (L % 4 == 0) { radix[s++] = 4; L /= 4; }
    if (L % 2 == 0) { radix[s++] = 2; L /= 2; }
    for (int p : {3, 5, 7}) while (L % p == 0) { radix[s++] = p; L /= p; }
    return L == 1 ? s : -1;
}

inline Plan make_plan(int n) {
    Plan p{};
    p.n = n;
    p.bluestein = smooth7(n) ? 0 : 1;
    p.m = p.bluestein ? bluestein_length(n) : n;
    p.nstages = factor(p.m, p.radix);
    return p;
}

// ---- host tables, in fp64 (rounded once to float for a float context) ----

// exp(-2 pi i k / L), k in [0, L], to an ulp or two.  The angle is reduced to phi in [0, pi / 4] in integers first (8k = o L + rem:
// octant o, and phi = pi rem / 4L from the nearer axis), so cos and sin see an argument that carries a relative error of a few
// 1e-16 of at most pi / 4, and the roots on the axes are exact; cos(2 pi k / L) of the unreduced angle is off by up to 1.3e-15.
inline void unit_root(long long k, long long L, double& re, double& im) {
    const long long o = 8 * k / L, rem = 8 * k % L;
    const bool up = o % 2 == 0;                            // theta = q pi / 2 + phi (up) or q pi / 2 - phi
    const double phi = M_PI * (double)(up ? rem : L - rem) / (4.0 * (double)L);
    const double c = cos(phi), s = up ? sin(phi) : -sin(phi);
    double ct, st;                                         // cos(theta), sin(theta), theta = 2 pi k / L
    switch (((o + 1) / 2) % 4) {
    case 0:  ct = c;  st = s;  break;
    case 1:  ct = -s; st = c;  break;
    case 2:  ct = -c; st = -s; break;
    default: ct = s;  st = -c; break;
    }
    re = ct; im = -st;
}

// W_L^i = exp(-2 pi i i / L), i in [0, L)
inline void twiddles(int L, std::vector<double>& re, std::vector<double>& im) {
    re.resize(L); im.resize(L);
    for (int i = 0; i < L; ++i) unit_root(i, L, re[i], im[i]);
}

// w_j = exp(-i pi j^2 / n), j in [0, n); j^2 is reduced mod 2n first (exact in integers) so the angle stays in [0, 2 pi)
inline void chirp(int n, std::vector<double>& re, std::vector<double>& im) {
    re.resize(n); im.resize(n);
    for (int j = 0; j < n; ++j) unit_root(((long long)j * j) % (2LL * n), 2LL * n, re[j], im[j]);
}

// ---- butterflies, shared by the host emulation and the kernels (C: float2 / double2 or any struct with x, y).  The complex
// helpers are those of c2c_roles.h, named here too for callers that open this namespace alone ----
using pnp::mkc; using pnp::cmul; using pnp::cmulc; using pnp::cadd; using pnp::csub; using pnp::cconj;

// in-register DFT of length RAD; roots W_RAD^p = tw[p * (L / RAD)] (conjugated for the inverse)
template <int RAD, bool INV, typename C>
PNP_HD inline void dft_small(C (&v)[RAD], const C* tw, int L) {
    if constexpr (RAD == 2) {
        const C a = v[0], b = v[1];
        v[0] = cadd(a, b); v[1] = csub(a, b);
    } else if constexpr (RAD == 4) {
        const C t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), d = csub(v[1], v[3]);
        const C t3 = INV ? mkc<C>(-d.y, d.x) : mkc<C>(d.y, -d.x);          // (+/-) i d
        v[0] = cadd(t0, t2); v[1] = cadd(t1, t3); v[2] = csub(t0, t2); v[3] = csub(t1, t3);
    } else {                                                               // 3, 5, 7: direct sums over the table's roots
        const int step = L / RAD;
        C o[RAD];
        for (int p = 0; p < RAD; ++p) {
            C acc = v[0];
            for (int q = 1; q < RAD; ++q) {
                const C w = tw[((p * q) % RAD) * step];
                acc = cadd(acc, INV ? cmulc(v[q], w) : cmul(v[q], w));
            }
            o[p] = acc;
        }
        for (int p = 0; p < RAD; ++p) v[p] = o[p];
    }
}

// butterfly j of a Stockham stage of radix RAD (header comment); a -> b, both of length L
template <int RAD, bool INV, typename C>
PNP_HD inline void stockham_bfly(const C* a, C* b, const C* tw, int L, int Ns, int j) {
    const int k = j % Ns, stride = L / RAD, tstep = L / (Ns * RAD);
    C v[RAD];
    for (int q = 0; q < RAD; ++q) v[q] = a[j + q * stride];
    if (Ns > 1)
        for (int q = 1; q < RAD; ++q) {
            const C w = tw[q * k * tstep];
            v[q] = INV ? cmulc(v[q], w) : cmul(v[q], w);
        }
    dft_small<RAD, INV>(v, tw, L);
    const int j0 = (j - k) * RAD + k;
    for (int q = 0; q < RAD; ++q) b[j0 + q * Ns] = v[q];
}

template <bool INV, typename C>
PNP_HD inline void stockham_bfly_r(int r, const C* a, C* b, const C* tw, int L, int Ns, int j) {
    switch (r) {
    case 2: stockham_bfly<2, INV>(a, b, tw, L, Ns, j); break;
    case 3: stockham_bfly<3, INV>(a, b, tw, L, Ns, j); break;
    case 4: stockham_bfly<4, INV>(a, b, tw, L, Ns, j); break;
    case 5: stockham_bfly<5, INV>(a, b, tw, L, Ns, j); break;
    case 7: stockham_bfly<7, INV>(a, b, tw, L, Ns, j); break;
    default: break;
    }
}

// Serial reference of the same transform (host: the emulation and the Bluestein kernel's table).  Unnormalised; returns the
// buffer holding the result.
template <bool INV, typename C>
inline C* stockham_host(C* a, C* b, const C* tw, const int* radix, int nstages, int L) {
    int Ns = 1;
    for (int s = 0; s < nstages; ++s) {
        const int r = radix[s];
        for (int j = 0; j < L / r; ++j) stockham_bfly_r<INV>(r, a, b, tw, L, Ns, j);
        C* t = a; a = b; b = t;
        Ns *= r;
    }
    return a;
}

// Bluestein kernel spectrum in fp64: FFT_m(b) / m, b_j = conj(w_j) for |j| < n (indices mod m), 0 elsewhere.  The 1/m of the
// inverse convolution transform is folded in (exact: m is a power of two).
template <typename C>
inline void bluestein_kernel(const Plan& p, const std::vector<double>& cre, const std::vector<double>& cim, std::vector<C>& out) {
    std::vector<double> tre, tim;
    twiddles(p.m, tre, tim);
    std::vector<C> tw(p.m), a(p.m), b(p.m);
    for (int i = 0; i < p.m; ++i) { tw[i] = mkc<C>(tre[i], tim[i]); a[i] = mkc<C>(0.0, 0.0); }
    for (int j = 0; j < p.n; ++j) {
        a[j] = mkc<C>(cre[j], -cim[j]);
        if (j) a[p.m - j] = a[j];
    }
    C* r = stockham_host<false>(a.data(), b.data(), tw.data(), p.radix, p.nstages, p.m);
    out.resize(p.m);
    for (int i = 0; i < p.m; ++i) out[i] = mkc<C>(r[i].x / p.m, r[i].y / p.m);
}

}  // namespace anysize
}  // namespace pnp
