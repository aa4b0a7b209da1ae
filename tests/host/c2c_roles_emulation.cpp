// CPU run of the row / column roles of the c2c kernels from the header the kernels include (csrc/c2c_roles.h): every RowIn, RowEpi and
// ColMid element form in double and in float, and the two lists of legal triples.
//   c2c_roles_emulation <in.bin> <out.bin>
//   in : int32 n; double scale, c, thr, c1, c2, c3, ib; double cin[2n], rin0[n], rin1[n], v[2n], z[n], w[n], X[2n], y[2n]; uint8 mask[n]
//        (the float run takes every value rounded to float)
//   out: for double, then float, as doubles: row_load of IN_COMPLEX, IN_REAL, IN_REAL_DIFF [2n each]; row_store of v: EPI_COMPLEX cout [2n],
//        EPI_ABS_REAL x [n], EPI_ABS_COMPLEX x [n], EPI_L1 z, w, x [n each], EPI_CNC z, w, x [n each]; col_mid of X: MID_NONE, MID_BLEND,
//        MID_MASK, MID_RESID, MID_MASK_ADD [2n each]
// y is handed to col_mid as a pointer, null wherever the role must not read it (MASK everywhere; BLEND, RESID where the mask byte is 0):
// a read there is a null dereference.  The by-value operand form must give the same bits; x_out = null must not change z, w.
//   c2c_roles_emulation triples
//   prints one line per (RowIn, inverse, RowEpi) and per (pre, ColMid, post): "row 1 0 0 -> 1 0 0" or "col 1 2 1 -> invalid"
#include "../../pnp_admm_cnc_mri_amd/csrc/c2c_roles.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct cd { double x, y; };
struct cf { float x, y; };
namespace pnp {
template <> struct CxOf<double> { using type = cd; };
template <> struct CxOf<float>  { using type = cf; };
}
using namespace pnp;

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(2); } } while (0)

struct Input {
    int n;
    double scale, c, prox[5];
    std::vector<double> cin, rin0, rin1, v, z, w, X, y;
    std::vector<uint8_t> mask;
};

template <typename T> static void put(std::vector<double>& out, const std::vector<T>& a) { for (T v : a) out.push_back((double)v); }
template <typename C> static void putc(std::vector<double>& out, const std::vector<C>& a) { for (C v : a) { out.push_back((double)v.x); out.push_back((double)v.y); } }
template <typename C, typename R> static std::vector<C> cx(const std::vector<double>& a) {
    std::vector<C> r(a.size() / 2);
    for (size_t i = 0; i < r.size(); ++i) r[i] = mkc<C>((R)a[2 * i], (R)a[2 * i + 1]);
    return r;
}
template <typename R> static std::vector<R> re(const std::vector<double>& a) { return std::vector<R>(a.begin(), a.end()); }
template <typename C> static bool same_bits(const std::vector<C>& a, const std::vector<C>& b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(C)) == 0;
}

template <int IN, typename R> static void run_load(const RowArgsT<R>& p, int n, std::vector<double>& out) {
    std::vector<typename CxOf<R>::type> r(n);
    for (int e = 0; e < n; ++e) r[e] = row_load<IN>(p, (size_t)e);
    putc(out, r);
}

// z, w, x of a prox epilogue; x_out = null must leave z and w as they come out with it
template <int EPI, typename R> static void run_prox(RowArgsT<R> p, const Input& in, const std::vector<typename CxOf<R>::type>& v, std::vector<double>& out) {
    const int n = in.n;
    std::vector<R> z = re<R>(in.z), w = re<R>(in.w), x(n), z2 = z, w2 = w;
    p.z = z.data(); p.w = w.data(); p.x_out = x.data();
    for (int e = 0; e < n; ++e) row_store<EPI>(p, (size_t)e, v[e]);
    p.z = z2.data(); p.w = w2.data(); p.x_out = nullptr;
    for (int e = 0; e < n; ++e) row_store<EPI>(p, (size_t)e, v[e]);
    REQUIRE(same_bits(z, z2) && same_bits(w, w2), "EPI %d: z, w depend on x_out", EPI);
    put(out, z); put(out, w); put(out, x);
}

template <int MID, typename R> static void run_mid(const Input& in, std::vector<double>& out) {
    using C = typename CxOf<R>::type;
    const int n = in.n;
    const std::vector<C> X = cx<C, R>(in.X), y = cx<C, R>(in.y);
    std::vector<C> byptr(n), byval(n);
    for (int e = 0; e < n; ++e) {
        const bool m = in.mask[e] != 0;
        const bool reads = MID == MID_MASK_ADD || ((MID == MID_BLEND || MID == MID_RESID) && m);
        byptr[e] = col_mid<MID>(X[e], m, reads ? &y[e] : (const C*)nullptr, (R)in.c);
        byval[e] = col_mid<MID>(X[e], m, y[e], (R)in.c);
    }
    REQUIRE(same_bits(byptr, byval), "MID %d: the pointer and the value operand differ", MID);
    putc(out, byptr);
}

template <typename R> static void run(const Input& in, std::vector<double>& out) {
    using C = typename CxOf<R>::type;
    const int n = in.n;
    const std::vector<C> cin = cx<C, R>(in.cin), v = cx<C, R>(in.v);
    const std::vector<R> rin0 = re<R>(in.rin0), rin1 = re<R>(in.rin1);
    RowArgsT<R> p{};
    p.cin = cin.data(); p.rin0 = rin0.data(); p.rin1 = rin1.data();
    p.scale = (R)in.scale;
    p.prox = ProxParamsT<R>{(R)in.prox[0], (R)in.prox[1], (R)in.prox[2], (R)in.prox[3], (R)in.prox[4]};
    p.nrows = 1;
    run_load<IN_COMPLEX>(p, n, out);
    run_load<IN_REAL>(p, n, out);
    run_load<IN_REAL_DIFF>(p, n, out);
    std::vector<C> co(n);
    std::vector<R> x(n);
    p.cout = co.data();
    for (int e = 0; e < n; ++e) row_store<EPI_COMPLEX>(p, (size_t)e, v[e]);
    putc(out, co);
    p.x_out = x.data();
    for (int e = 0; e < n; ++e) row_store<EPI_ABS_REAL>(p, (size_t)e, v[e]);
    put(out, x);
    for (int e = 0; e < n; ++e) row_store<EPI_ABS_COMPLEX>(p, (size_t)e, v[e]);
    put(out, x);
    run_prox<EPI_L1>(p, in, v, out);
    run_prox<EPI_CNC>(p, in, v, out);
    run_mid<MID_NONE, R>(in, out);
    run_mid<MID_BLEND, R>(in, out);
    run_mid<MID_MASK, R>(in, out);
    run_mid<MID_RESID, R>(in, out);
    run_mid<MID_MASK_ADD, R>(in, out);
}

static int triples() {
    for (int in = 0; in < 3; ++in)
        for (int inv = 0; inv < 2; ++inv)
            for (int epi = 0; epi < 5; ++epi) {
                const int r = row_roles((RowIn)in, inv != 0, (RowEpi)epi, -1, [](auto IN, auto INV, auto EPI) { return 100 * IN() + 10 * (int)INV() + EPI(); });
                if (r < 0) printf("row %d %d %d -> invalid\n", in, inv, epi);
                else printf("row %d %d %d -> %d %d %d\n", in, inv, epi, r / 100, r / 10 % 10, r % 10);
            }
    for (int pre = 0; pre < 2; ++pre)
        for (int mid = 0; mid < 5; ++mid)
            for (int post = 0; post < 2; ++post) {
                const int r = col_roles(pre != 0, (ColMid)mid, post != 0, -1, [](auto PRE, auto MID, auto POST) { return 100 * (int)PRE() + 10 * MID() + (int)POST(); });
                if (r < 0) printf("col %d %d %d -> invalid\n", pre, mid, post);
                else printf("col %d %d %d -> %d %d %d\n", pre, mid, post, r / 100, r / 10 % 10, r % 10);
            }
    return 0;
}

static void rd(FILE* f, void* p, size_t bytes) { REQUIRE(fread(p, 1, bytes, f) == bytes, "short input"); }

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "triples")) return triples();
    REQUIRE(argc == 3, "usage: c2c_roles_emulation <in.bin> <out.bin> | triples");
    FILE* f = fopen(argv[1], "rb");
    REQUIRE(f, "cannot open %s", argv[1]);
    Input in;
    int32_t n;
    rd(f, &n, 4);
    REQUIRE(n > 0 && n <= (1 << 20), "n");
    in.n = n;
    double sc[7];
    rd(f, sc, sizeof(sc));
    in.scale = sc[0]; in.c = sc[1];
    for (int i = 0; i < 5; ++i) in.prox[i] = sc[2 + i];
    for (auto* a : {&in.cin, &in.rin0, &in.rin1, &in.v, &in.z, &in.w, &in.X, &in.y}) {
        const bool complex = a == &in.cin || a == &in.v || a == &in.X || a == &in.y;
        a->resize((size_t)n * (complex ? 2 : 1));
        rd(f, a->data(), a->size() * sizeof(double));
    }
    in.mask.resize(n);
    rd(f, in.mask.data(), n);
    fclose(f);
    std::vector<double> out;
    run<double>(in, out);
    run<float>(in, out);
    REQUIRE(out.size() == (size_t)52 * n, "output size");
    f = fopen(argv[2], "wb");
    REQUIRE(f && fwrite(out.data(), sizeof(double), out.size(), f) == out.size(), "cannot write %s", argv[2]);
    fclose(f);
    return 0;
}
