// CPU emulation of the any-size FFT (csrc/kernels_anysize.hip) from the header the kernels include (csrc/anysize_plan.h):
// the plan, the fp64 tables and one line transform, forward and inverse, in the order line_fft runs them.
//   anysize_emulation <n> <in.bin> <out.bin>
//   in : n complex128 (x)
//   out: int32 n, bluestein, m, nstages, radix[12]; complex128 tw[m], chirp[n], kern[m] (zeros unless Bluestein);
//        complex128 fwd[n], inv[n] (unnormalised)
//
// Every length in one process, in double and in float (the same template over a {float x, y} struct; the float tables are the
// fp64 ones rounded once and the Bluestein kernel spectrum is computed in double and rounded, as upload_axis<float2> does):
//   anysize_emulation sweep <in.bin> <out.bin>
//   in : for n = 128 .. 1024: n complex128, concatenated (the float run takes them rounded to float)
//   out: for n = 128 .. 1024: int32 n, bluestein, m, nstages, radix[12]; complex128 fwd[n], inv[n]; complex64 fwd[n], inv[n]
//
// One H x W array, the line transform along the rows (length W), then along the columns (length H), as fft2 of the kernels:
//   anysize_emulation grid <H> <W> <in.bin> <out.bin>
//   in : H * W complex128, row-major
//   out: complex128 fwd[H * W], inv[H * W]; complex64 fwd[H * W], inv[H * W] (unnormalised)
#include "../../pnp_admm_cnc_mri_amd/csrc/anysize_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace pnp::anysize;

struct cd { double x, y; };
struct cf { float x, y; };

// one axis as a context holds it: the plan and its tables in the precision of C
template <typename C> struct Axis {
    Plan p;
    std::vector<C> tw, ch, kern;
};

template <typename C>
static Axis<C> make_axis(int n) {
    Axis<C> t;
    t.p = make_plan(n);
    std::vector<double> tre, tim, cre, cim;
    twiddles(t.p.m, tre, tim);
    t.tw.resize(t.p.m);
    t.ch.assign(n, mkc<C>(0.0, 0.0));
    t.kern.assign(t.p.m, mkc<C>(0.0, 0.0));
    for (int i = 0; i < t.p.m; ++i) t.tw[i] = mkc<C>(tre[i], tim[i]);
    if (t.p.bluestein) {
        chirp(n, cre, cim);
        std::vector<cd> kd;
        bluestein_kernel<cd>(t.p, cre, cim, kd);
        for (int j = 0; j < n; ++j) t.ch[j] = mkc<C>(cre[j], cim[j]);
        for (int i = 0; i < t.p.m; ++i) t.kern[i] = mkc<C>(kd[i].x, kd[i].y);
    }
    return t;
}

// line_fft of the kernels, one line, serial: x[0], x[stride], ... -> out[0], out[stride], ...
template <bool INV, typename C>
static void line(const Axis<C>& t, const C* x, C* out, size_t stride, std::vector<C>& a, std::vector<C>& b) {
    const Plan& p = t.p;
    a.resize(p.m + 1); b.resize(p.m + 1);
    for (int j = 0; j < p.n; ++j) a[j] = x[j * stride];
    if (!p.bluestein) {
        const C* r = stockham_host<INV>(a.data(), b.data(), t.tw.data(), p.radix, p.nstages, p.m);
        for (int j = 0; j < p.n; ++j) out[j * stride] = r[j];
        return;
    }
    for (int j = 0; j < p.m; ++j) {
        C v = mkc<C>(0.0, 0.0);
        if (j < p.n) { v = a[j]; if (INV) v = cconj(v); v = cmul(v, t.ch[j]); }
        a[j] = v;
    }
    C* r = stockham_host<false>(a.data(), b.data(), t.tw.data(), p.radix, p.nstages, p.m);
    C* o = (r == a.data()) ? b.data() : a.data();
    for (int j = 0; j < p.m; ++j) r[j] = cmul(r[j], t.kern[j]);
    r = stockham_host<true>(r, o, t.tw.data(), p.radix, p.nstages, p.m);
    for (int j = 0; j < p.n; ++j) { C v = cmul(r[j], t.ch[j]); out[j * stride] = INV ? cconj(v) : v; }
}

template <bool INV, typename C>
static std::vector<C> line(const Axis<C>& t, const std::vector<C>& x) {
    std::vector<C> out(t.p.n), a, b;
    line<INV>(t, x.data(), out.data(), 1, a, b);
    return out;
}

static bool read_all(const char* path, void* dst, size_t bytes) {
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(dst, 1, bytes, f) == bytes;
    if (f) fclose(f);
    return ok;
}

static void write_plan(FILE* f, const Plan& p) {
    const int hdr[4] = {p.n, p.bluestein, p.m, p.nstages};
    fwrite(hdr, sizeof(int), 4, f);
    fwrite(p.radix, sizeof(int), MAX_STAGES, f);
}

template <typename C>
static std::vector<C> rounded(const std::vector<cd>& x) {
    std::vector<C> r(x.size());
    for (size_t i = 0; i < x.size(); ++i) r[i] = mkc<C>(x[i].x, x[i].y);
    return r;
}

template <typename C>
static void sweep_one(FILE* f, int n, const std::vector<cd>& x) {
    const Axis<C> t = make_axis<C>(n);
    const std::vector<C> xc = rounded<C>(x), fwd = line<false>(t, xc), inv = line<true>(t, xc);
    fwrite(fwd.data(), sizeof(C), n, f);
    fwrite(inv.data(), sizeof(C), n, f);
}

static int sweep(const char* in, const char* out) {
    size_t total = 0;
    for (int n = MIN_N; n <= MAX_N; ++n) total += n;
    std::vector<cd> all(total);
    if (!read_all(in, all.data(), total * sizeof(cd))) return 4;
    FILE* f = fopen(out, "wb");
    if (!f) return 5;
    size_t o = 0;
    for (int n = MIN_N; n <= MAX_N; ++n) {
        const Plan p = make_plan(n);
        if (p.nstages < 1) return 3;
        const std::vector<cd> x(all.begin() + o, all.begin() + o + n);
        o += n;
        write_plan(f, p);
        sweep_one<cd>(f, n, x);
        sweep_one<cf>(f, n, x);
    }
    fclose(f);
    return 0;
}

// one pass of the line transform over `lines` lines of an array, in place
template <bool INV, typename C>
static void grid_pass(const Axis<C>& t, C* x, int lines, size_t between, size_t stride) {
    std::vector<C> a, b;
    for (int i = 0; i < lines; ++i) line<INV>(t, x + i * between, x + i * between, stride, a, b);
}

template <typename C>
static void grid_one(FILE* f, int H, int W, const std::vector<cd>& x) {
    const Axis<C> row = make_axis<C>(W), col = make_axis<C>(H);
    std::vector<C> fwd = rounded<C>(x), inv = fwd;
    grid_pass<false>(row, fwd.data(), H, W, 1);
    grid_pass<false>(col, fwd.data(), W, 1, W);
    grid_pass<true>(row, inv.data(), H, W, 1);
    grid_pass<true>(col, inv.data(), W, 1, W);
    fwrite(fwd.data(), sizeof(C), fwd.size(), f);
    fwrite(inv.data(), sizeof(C), inv.size(), f);
}

static int grid(int H, int W, const char* in, const char* out) {
    if (H < MIN_N || H > MAX_N || W < MIN_N || W > MAX_N) return 3;
    std::vector<cd> x((size_t)H * W);
    if (!read_all(in, x.data(), x.size() * sizeof(cd))) return 4;
    FILE* f = fopen(out, "wb");
    if (!f) return 5;
    grid_one<cd>(f, H, W, x);
    grid_one<cf>(f, H, W, x);
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "sweep")) return sweep(argv[2], argv[3]);
    if (argc == 6 && !strcmp(argv[1], "grid")) return grid(atoi(argv[2]), atoi(argv[3]), argv[4], argv[5]);
    if (argc != 4) return 2;
    const int n = atoi(argv[1]);
    const Plan p = make_plan(n);
    if (p.nstages < 1) return 3;
    std::vector<cd> x(n);
    if (!read_all(argv[2], x.data(), n * sizeof(cd))) return 4;
    const Axis<cd> t = make_axis<cd>(n);
    const std::vector<cd> fwd = line<false>(t, x), inv = line<true>(t, x);
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 5;
    write_plan(f, p);
    const std::vector<cd>* parts[] = {&t.tw, &t.ch, &t.kern, &fwd, &inv};
    for (const std::vector<cd>* v : parts) fwrite(v->data(), sizeof(cd), v->size(), f);
    fclose(f);
    return 0;
}
