// Host emulation of the locally low-rank prox (pnp_admm_cnc_mri_amd/csrc/lowrank_plan.h): a stand-alone program that runs the plan's item
// functions group by group, one item after another and pass after pass, exactly as the kernel does one item per thread with a barrier
// between the passes -- under g++, plain and with -fsanitize=address,undefined (tests/test_lowrank_host.py builds both and runs them with
// nothing preloaded).
//
//   lowrank_emulation CASE...      every CASE a file of doubles written by the test from tests/lowrank_oracle.py:
//       T, S, H, W, b, sy, sx, cnc, thr, c1, c2, c3, ib (thr and ib scaled),  then x, z, w, z+, w+ (oracle), each S T H W values
//
// Per case, in double and in float: the arrays have exactly the plan's sizes (heap blocks, so the sanitizer sees the first byte beyond
// them), the LDS block is lr_lds_bytes long and filled with NaN before every group, and the outputs are filled with NaN before a group
// stores: after it as many values of z and of w are set as the group has pixel-frames -- every pixel-frame is written exactly once over
// all groups.  Double results must equal the oracle to 1e-12, float to 2e-5 (relative to the largest value); relz is the rel-L2 of z+.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../pnp_admm_cnc_mri_amd/csrc/lowrank_plan.h"

using namespace pnp;

struct Case {
    int T, S, H, W, b, sy, sx, cnc;
    double thr, c1, c2, c3, ib;
    std::vector<double> x, z, w, zr, wr;
};

static bool read_case(const char* path, Case* c) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    double h[13];
    bool ok = fread(h, sizeof(double), 13, f) == 13;
    if (ok) {
        c->T = (int)h[0]; c->S = (int)h[1]; c->H = (int)h[2]; c->W = (int)h[3]; c->b = (int)h[4]; c->sy = (int)h[5]; c->sx = (int)h[6];
        c->cnc = (int)h[7]; c->thr = h[8]; c->c1 = h[9]; c->c2 = h[10]; c->c3 = h[11]; c->ib = h[12];
        const size_t n = (size_t)c->S * c->T * c->H * c->W;
        for (std::vector<double>* v : {&c->x, &c->z, &c->w, &c->zr, &c->wr}) {
            v->resize(n);
            ok = ok && fread(v->data(), sizeof(double), n, f) == n;
        }
    }
    fclose(f);
    if (!ok) fprintf(stderr, "%s: short file\n", path);
    return ok;
}

// the passes one after another: an item loop is a pass, the barrier nothing
struct Serial {
    template <typename F> void items(int n, F f) const { for (int i = 0; i < n; ++i) f(i); }
    void sync() const {}
};

// one case in precision R; -> largest |difference| / largest |reference|, -1 on a coverage failure
template <typename R, bool CNC>
static double run_case(const Case& c, double* rel_z) {
    const size_t n = (size_t)c.S * c.T * c.H * c.W;
    const size_t lds_bytes = lr_lds_bytes(c.T, c.b, sizeof(R), CNC);
    R *x = (R*)malloc(n * sizeof(R)), *zin = (R*)malloc(n * sizeof(R)), *win = (R*)malloc(n * sizeof(R)), *ldsr = (R*)malloc(lds_bytes);
    unsigned char* lds = (unsigned char*)ldsr;
    R *zwork = (R*)malloc(n * sizeof(R)), *wwork = (R*)malloc(n * sizeof(R));
    std::vector<R> zout(n, (R)NAN), wout(n, (R)NAN);
    std::vector<int> hits(n, 0);
    if (!x || !zin || !win || !ldsr || !zwork || !wwork) return -3.0;
    for (size_t i = 0; i < n; ++i) { x[i] = (R)c.x[i]; zin[i] = (R)c.z[i]; win[i] = (R)c.w[i]; }
    LrArgs<R> a;
    a.x = x;
    a.p.thr = (R)c.thr; a.p.c1 = (R)c.c1; a.p.c2 = (R)c.c2; a.p.c3 = (R)c.c3; a.p.ib = (R)c.ib;
    a.H = c.H; a.W = c.W; a.T = c.T; a.S = c.S; a.b = c.b; a.sy = c.sy; a.sx = c.sx;
    lr_fill_grid(a, CNC);
    bool covered = lr_groups(a.S, a.ny, a.ngx) == (size_t)a.S * a.ny * a.ngx;
    Serial ex;
    for (int s = 0; s < c.S; ++s) for (int gi = 0; gi < a.ny * a.ngx; ++gi) {
        memset(lds, 0xff, lds_bytes);                                   // every value, float or double, a NaN
        // the kernel works in place on z and w: this group reads the inputs and writes onto NaN
        memcpy(zwork, zin, n * sizeof(R));
        memcpy(wwork, win, n * sizeof(R));
        a.z = zwork; a.w = wwork;
        lr_run_group<R, CNC>(a, s, gi, lds, ex);
        const LrGroup g = lr_group_of(a, s, gi);
        size_t changed = 0;
        for (int it = 0; it < lr_pixel_items(a, g); ++it) {
            const LrPlace pl = lr_place(it, a, g);
            if (pl.o >= n) { covered = false; continue; }
            ++hits[pl.o];
            ++changed;
            zout[pl.o] = zwork[pl.o]; wout[pl.o] = wwork[pl.o];
            zwork[pl.o] = zin[pl.o]; wwork[pl.o] = win[pl.o];
        }
        // nothing else moved
        if (memcmp(zwork, zin, n * sizeof(R)) || memcmp(wwork, win, n * sizeof(R)) || changed != (size_t)c.T * g.ph * g.span) covered = false;
    }
    for (size_t i = 0; i < n; ++i) if (hits[i] != 1) covered = false;
    double err = 0, top = 0, num = 0, den = 0;
    bool finite = true;
    for (size_t i = 0; i < n; ++i) {
        const double dz = fabs((double)zout[i] - c.zr[i]), dw = fabs((double)wout[i] - c.wr[i]);
        num += dz * dz; den += c.zr[i] * c.zr[i];
        finite = finite && dz == dz && dw == dw;
        err = fmax(err, fmax(dz, dw));
        top = fmax(top, fmax(fabs(c.zr[i]), fabs(c.wr[i])));
    }
    if (!finite) err = INFINITY;
    free(x); free(zin); free(win); free(ldsr); free(zwork); free(wwork);
    if (rel_z) *rel_z = sqrt(num / den);
    return covered ? err / top : -1.0;
}

template <typename R> static int run_prec(const Case& c, const char* path, const char* prec, double bar) {
    double rel_z = 0;
    const double e = c.cnc ? run_case<R, true>(c, &rel_z) : run_case<R, false>(c, &rel_z);
    const bool ok = e >= 0.0 && e <= bar;
    printf("%s %s T=%d S=%d %dx%d b=%d shift=(%d,%d) %s Q=%d lds=%zu err=%.3e relz=%.3e %s\n", path, prec, c.T, c.S, c.H, c.W, c.b, c.sy, c.sx,
           c.cnc ? "cnc" : "l1", lr_group(c.T, c.b, sizeof(R), c.cnc != 0), lr_lds_bytes(c.T, c.b, sizeof(R), c.cnc != 0), e, rel_z,
           ok ? "ok" : e == -1.0 ? "COVERAGE" : "DIFFER");
    return !ok;
}

int main(int argc, char** argv) {
    // the plan's own promises: b <= 8 at every T, b = 16 at T <= 16, both precisions, L1 and CNC; every admitted plan within LR_LDS_MAX
    for (int T = TP_MIN_FRAMES; T <= TP_MAX_FRAMES; ++T)
        for (int b = LR_MIN_BLOCK; b <= LR_MAX_BLOCK; ++b) for (int cnc = 0; cnc < 2; ++cnc) for (size_t rb : {sizeof(float), sizeof(double)}) {
            const int rc = lr_check(T, b, 128, 128, T, rb, cnc != 0);
            const bool owed = b <= 8 || (b <= 16 && T <= 16);
            const int Q = lr_group(T, b, rb, cnc != 0);
            if ((owed && rc != LR_OK) || (rc != LR_OK && rc != LR_BAD_LDS) || (rc == LR_OK && lr_lds_bytes(T, b, rb, cnc != 0) > LR_LDS_MAX) ||
                Q < 1 || Q > LR_MAX_GROUP || (Q > 1 && lr_lds_bytes(T, b, rb, cnc != 0) > LR_LDS_BUDGET)) {
                printf("plan: T=%d b=%d cnc=%d real=%zu: rc=%d Q=%d lds=%zu\n", T, b, cnc, rb, rc, Q, lr_lds_bytes(T, b, rb, cnc != 0));
                return 1;
            }
        }
    if (lr_check(1, 8, 128, 128, 4, 4, false) != LR_BAD_FRAMES || lr_check(65, 8, 128, 128, 65, 4, false) != LR_BAD_FRAMES ||
        lr_check(4, 1, 128, 128, 4, 4, false) != LR_BAD_BLOCK || lr_check(4, 33, 128, 128, 4, 4, false) != LR_BAD_BLOCK ||
        lr_check(4, 16, 128, 12, 4, 4, false) != LR_BAD_SHAPE || lr_check(64, 32, 128, 128, 64, 4, false) != LR_BAD_LDS ||
        lr_check(4, 8, 128, 128, 6, 4, false) != LR_BAD_BATCH || lr_check(4, 8, 128, 128, 8, 8, true) != LR_OK) {
        printf("plan: lr_check\n");
        return 1;
    }
    // every round of the ordering pairs every index once, a sweep every pair once
    for (int n = 2; n <= 64; n += 2) {
        std::vector<int> met((size_t)n * n, 0);
        for (int r = 0; r < n - 1; ++r) {
            std::vector<int> seen(n, 0);
            for (int k = 0; k < n / 2; ++k) {
                const LrPair p = lr_pair(n, r, k);
                if (p.p < 0 || p.q >= n || p.p >= p.q) { printf("plan: lr_pair(%d, %d, %d)\n", n, r, k); return 1; }
                ++seen[p.p]; ++seen[p.q]; ++met[(size_t)p.p * n + p.q];
            }
            for (int i = 0; i < n; ++i) if (seen[i] != 1) { printf("plan: round %d of %d\n", r, n); return 1; }
        }
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) if (met[(size_t)i * n + j] != 1) { printf("plan: sweep of %d\n", n); return 1; }
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
