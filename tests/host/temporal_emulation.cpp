// Host emulation of the temporal prox (pnp_admm_cnc_mri_amd/csrc/temporal_plan.h): a stand-alone program that runs the plan's item
// functions run by run, one item after another, exactly as the kernel does one item per thread -- under g++, plain and with
// -fsanitize=address,undefined (tests/test_temporal_host.py builds both and runs them with nothing preloaded).
//
//   temporal_emulation CASE...      every CASE a file of doubles written by the test from tests/temporal_oracle.py:
//       T, S, N, cx, cnc, keep_dc, thr, c1, c2, c3, ib,  then x, z, w, z+, w+ (oracle), each S T N values (2 S T N with cx, interleaved)
//
// Per case, in double and in float: the arrays have exactly the plan's sizes (heap blocks, so the sanitizer sees the first byte beyond
// them), the LDS block is tp_lds_bytes long and filled with NaN before every run, VP is tp_group's for the block's real alignment (also
// forced down to the narrower ones), the twiddle matrix has exactly 2 T T values, and the store pass runs on output arrays filled with
// NaN: after it as many values of z and of w are set as its items stored, all of them inside the run -- every pixel-frame is written
// exactly once, and nowhere else.  Double results must equal the oracle to 1e-12, float to 2e-5 (relative to the largest value).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../pnp_admm_cnc_mri_amd/csrc/temporal_plan.h"

using namespace pnp;

struct Case {
    int T, S, cx, cnc, keep_dc;
    size_t N;
    double thr, c1, c2, c3, ib;
    std::vector<double> x, z, w, zr, wr;
};

static bool read_case(const char* path, Case* c) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    double h[11];
    bool ok = fread(h, sizeof(double), 11, f) == 11;
    if (ok) {
        c->T = (int)h[0]; c->S = (int)h[1]; c->N = (size_t)h[2]; c->cx = (int)h[3]; c->cnc = (int)h[4]; c->keep_dc = (int)h[5];
        c->thr = h[6]; c->c1 = h[7]; c->c2 = h[8]; c->c3 = h[9]; c->ib = h[10];
        const size_t n = (size_t)c->S * c->T * c->N * (c->cx ? 2 : 1);
        for (std::vector<double>* v : {&c->x, &c->z, &c->w, &c->zr, &c->wr}) {
            v->resize(n);
            ok = ok && fread(v->data(), sizeof(double), n, f) == n;
        }
    }
    fclose(f);
    if (!ok) fprintf(stderr, "%s: short file\n", path);
    return ok;
}

template <typename R> static size_t count_set(const R* a, size_t n) {
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) k += a[i] == a[i];
    return k;
}

// one case in precision R with VP pixels per access; -> largest |difference| / largest |reference|, or -1 on a coverage failure
template <typename R, bool CX, bool CNC, int VP>
static double run_case(const Case& c) {
    using V = TpValue<R, CX>;
    constexpr int comps = CX ? 2 : 1;
    const size_t vals = (size_t)c.S * c.T * c.N, n = vals * comps;
    // exactly the plan's sizes, aligned as hipMalloc aligns (at least 16 bytes)
    R *x = nullptr, *zin = nullptr, *win = nullptr;
    unsigned char* lds = nullptr;
    const size_t lds_bytes = tp_lds_bytes(c.T, CX, sizeof(R));
    bool have = posix_memalign((void**)&lds, 16, lds_bytes) == 0;
    for (R** p : {&x, &zin, &win}) have = posix_memalign((void**)p, 16, n * sizeof(R)) == 0 && have;
    if (!have) { free(x); free(zin); free(win); free(lds); return -3.0; }
    std::vector<R> zwork(n), wwork(n), zout(n), wout(n), e(2 * (size_t)c.T * c.T);
    for (size_t i = 0; i < n; ++i) { x[i] = (R)c.x[i]; zin[i] = (R)c.z[i]; win[i] = (R)c.w[i]; }
    tp_twiddle_matrix<R>(c.T, e.data());
    TpArgs<R, CX> a;
    a.x = (const V*)x; a.e = e.data();
    a.p.thr = (R)c.thr; a.p.c1 = (R)c.c1; a.p.c2 = (R)c.c2; a.p.c3 = (R)c.c3; a.p.ib = (R)c.ib;
    a.scale = (R)(1.0 / sqrt((double)c.T));
    a.N = c.N; a.T = c.T; a.S = c.S; a.P = tp_run(c.T, CX, sizeof(R)); a.keep_dc = c.keep_dc;
    bool covered = true;
    const size_t runs = tp_runs(c.N, a.P);
    for (int s = 0; s < c.S; ++s) for (size_t r = 0; r < runs; ++r) {
        R* l = (R*)lds;
        for (size_t i = 0; i < lds_bytes / sizeof(R); ++i) l[i] = (R)NAN;
        // the first three passes read the inputs and work in LDS ...
        a.z = (V*)zin; a.w = (V*)win;
        const TpRun<R, CX> t = tp_run_of<R, CX>(a, s, r, lds);
        for (int i = 0, m = tp_load_items(c.T, t.np, VP); i < m; ++i) tp_load_item<R, CX, CNC, VP>(i, a, t);
        for (int i = 0, m = tp_coef_items(c.T, CX, t.np); i < m; ++i) tp_coef_item<R, CX, CNC>(i, a, t);
        for (int i = 0, m = tp_synth_items(c.T, t.np); i < m; ++i) tp_synth_item<R, CX>(i, a, t);
        // ... the fourth writes: onto NaN
        for (size_t i = 0; i < n; ++i) zwork[i] = wwork[i] = (R)NAN;
        a.z = (V*)zwork.data(); a.w = (V*)wwork.data();
        const int items = tp_store_items(c.T, t.np, VP);
        for (int i = 0; i < items; ++i) tp_store_item<R, CX, VP>(i, a, t);
        // an item stores VP values per array: as many set values as the items stored means no two items met, and that many is the run
        const size_t set = (size_t)items * VP * comps;
        if (count_set(zwork.data(), n) != set || count_set(wwork.data(), n) != set || set != (size_t)c.T * t.np * comps) covered = false;
        for (int f = 0; f < c.T; ++f) for (int p = 0; p < t.np * comps; ++p) {         // all of them inside the run
            const size_t o = (t.base + (size_t)f * c.N + t.p0) * comps + p;
            if (!(zwork[o] == zwork[o]) || !(wwork[o] == wwork[o])) covered = false;
            zout[o] = zwork[o]; wout[o] = wwork[o];
        }
    }
    double err = 0, top = 0;
    bool finite = true;
    for (size_t i = 0; i < n; ++i) {
        const double dz = fabs((double)zout[i] - c.zr[i]), dw = fabs((double)wout[i] - c.wr[i]);
        finite = finite && dz == dz && dw == dw;
        err = fmax(err, fmax(dz, dw));
        top = fmax(top, fmax(fabs(c.zr[i]), fabs(c.wr[i])));
    }
    if (!finite) err = INFINITY;
    free(x); free(zin); free(win); free(lds);
    return covered ? err / top : -1.0;
}

template <typename R, bool CX, bool CNC> static int run_widths(const Case& c, const char* path, const char* prec, double bar) {
    using V = TpValue<R, CX>;
    const int widest = tp_group(c.N, sizeof(V), 16);
    int bad = 0;
    for (int vp = widest; vp >= 1; vp >>= 1) {
        double e = -2.0;
        if (vp == 4) { if constexpr (sizeof(V) <= 4) e = run_case<R, CX, CNC, 4>(c); }
        else if (vp == 2) { if constexpr (sizeof(V) <= 8) e = run_case<R, CX, CNC, 2>(c); }
        else e = run_case<R, CX, CNC, 1>(c);
        const bool ok = e >= 0.0 && e <= bar;
        printf("%s %s T=%d S=%d N=%zu %s %s keep_dc=%d P=%d VP=%d lds=%zu err=%.3e %s\n", path, prec, c.T, c.S, c.N, CX ? "complex" : "real",
               CNC ? "cnc" : "l1", c.keep_dc, tp_run(c.T, CX, sizeof(R)), vp, tp_lds_bytes(c.T, CX, sizeof(R)), e,
               ok ? "ok" : e == -1.0 ? "COVERAGE" : "DIFFER");
        bad += !ok;
    }
    return bad;
}

template <typename R> static int run_prec(const Case& c, const char* path, const char* prec, double bar) {
    if (c.cx) return c.cnc ? run_widths<R, true, true>(c, path, prec, bar) : run_widths<R, true, false>(c, path, prec, bar);
    return c.cnc ? run_widths<R, false, true>(c, path, prec, bar) : run_widths<R, false, false>(c, path, prec, bar);
}

int main(int argc, char** argv) {
    // the plan's own promises
    for (int T = TP_MIN_FRAMES; T <= TP_MAX_FRAMES; ++T)
        for (int cx = 0; cx < 2; ++cx) for (int cnc = 0; cnc < 2; ++cnc) for (size_t rb : {sizeof(float), sizeof(double)}) {
            const size_t vb = (cx ? 2 : 1) * rb;
            const int P = tp_run(T, cx, rb);
            if (tp_lds_bytes(T, cx, rb) > 64 * 1024 || P % (int)(16 / vb) || P < TP_MIN_RUN || P > TP_MAX_RUN || tp_layout(T, vb) != TP_LDS) {
                printf("plan: T=%d cx=%d cnc=%d real=%zu: P=%d lds=%zu\n", T, cx, cnc, rb, P, tp_lds_bytes(T, cx, rb));
                return 1;
            }
        }
    if (tp_check(1, 4) != TP_BAD_FRAMES || tp_check(65, 65) != TP_BAD_FRAMES || tp_check(4, 6) != TP_BAD_BATCH || tp_check(4, 0) != TP_BAD_BATCH ||
        tp_check(3, 9) != TP_OK || tp_group(130 * 129, 4, 16) != 2 || tp_group(129 * 131, 4, 16) != 1 || tp_group(128 * 128, 4, 16) != 4 ||
        tp_group(128 * 128, 4, 8) != 2 || tp_group(129 * 131, 16, 16) != 1 || tp_group(129 * 131, 8, 16) != 1 || tp_group(130 * 129, 8, 16) != 2) {
        printf("plan: tp_check / tp_group\n");
        return 1;
    }
    int bad = 0;
    for (int i = 1; i < argc; ++i) {
        Case c;
        if (!read_case(argv[i], &c)) return 2;
        bad += run_prec<double>(c, argv[i], "double", 1e-12);
        bad += run_prec<float>(c, argv[i], "float", 2e-5);
    }
    printf("%d cases, %d bad\n%s\n", argc - 1, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
