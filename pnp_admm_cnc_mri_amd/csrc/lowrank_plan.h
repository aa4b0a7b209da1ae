// Locally low-rank prox (pnp_set_lowrank; kernels_lowrank.hip; include/pnp_mri.h, "low-rank"): the argument check, the patches a workgroup
// owns, its LDS layout and -- as work-item functions -- every load, sum, rotation and store of the prox.  Host- and device-callable code
// without HIP: the kernel runs these functions one item per thread with a barrier between the passes, tests/host/lowrank_emulation.cpp
// runs them one item after another under g++ and the sanitizers.
//
// The batch is S series of T frames of H x W real values.  The grid of b x b patches is anchored at the shift (sy, sx), 0 <= sy, sx < b:
// patch (i, j) holds the rows (sy + i b + r) mod H and the columns (sx + j b + c) mod W, r, c < b; the last patch row has H mod b rows and the
// last patch column W mod b columns where b does not divide them (it does not wrap onto the first patch), so the patches partition the
// image.  X is the P x T matrix of one patch (P <= b^2 pixels, pixel p = r pw + c with pw the patch's width), X = U diag(sigma) V^T, and
// S_g(X) = X V diag(g(sigma)) V^T:
//     L1    z+ = S_shrink(u),  u = x + w,  shrink(s) = (s - thr) / s where s > thr, 0 elsewhere
//     CNC   t = c1 z + c2 u + c3 S_clip(z)  [fma(c1, z, fma(c2, u, c3 * S_clip(z)))],  clip(s) = ib / s where s > ib, 1 elsewhere;  z+ = S_shrink(t)
//     both  w+ = u - z+
// thr and ib arrive scaled by the host (pnp_set_lowrank's scale).
//
// Route: G = X^T X (T x T, every entry one chain of fma over p ascending, so G is exactly symmetric), diagonalised by cyclic Jacobi in the
// round-robin ordering -- n = T rounded up to even, n - 1 rounds a sweep, round r pairs (n - 1, r) and ((r + k) mod (n - 1),
// (r - k) mod (n - 1)), 0 < k < n / 2; a pair that holds the padding index T of an odd T is skipped.  A round is three passes: the
// rotations (c, s) of its pairs from G, the columns of G and V, the rows of G (and the rotated entry set to 0).  Before every sweep
// off^2 = sum_{i != j} G_ij^2 (row sums over j ascending, summed over i ascending) is tested against (eps_R ||G||_F)^2, ||G||_F of the
// untouched Gram matrix and eps_R = LrEps (the machine epsilon / 64); a patch that passes rotates no more, and the loop ends when every
// patch of the workgroup has passed or after LR_MAX_SWEEPS sweeps: what a patch receives depends on that patch alone.
// V and the rotations (c, s) are DOUBLE in both precisions; G is R and turns by (c, s) rounded to R.  A V kept in float leaves orthogonality
// by an ulp per rotation -- the float kernel then stood 1.5 .. 4 x the float32 restatement from the oracle, growing with T -- whereas an
// orthogonal V makes M an exact spectral function of a matrix within float round-off of G, which is all an eigen-solver in float offers.
// Then lambda_j = max(G_jj, 0), sigma_j = sqrt(lambda_j), M = V diag(g(sigma)) V^T (j ascending, fma((V_aj g_j), V_bj, acc) in double,
// rounded once to R), and S_g(X) = X M row by row (t' ascending).
// CNC runs this twice: on z, then on t, which takes z's place in a second tile; u is re-read from x and w.
//
// A workgroup owns LR_GROUP consecutive patches of one patch row of one series (lr_group: as many as fit LR_LDS_BUDGET, the row's last
// group fewer), so that a frame's row segment is one run of consecutive columns.  Every global access is one value: the shift leaves no
// alignment to use.  LDS of one patch: in doubles V [T][TS] and the rotations [n]; in values of R the tile [b^2][TS] (CNC: two), G [T][TS]
// (TS = T | 1: an odd stride, since lanes walk p resp. rows), a vector [T] (row sums, then g(sigma)) and two scalars (the bar of off^2,
// the flag); rounded up to 8 bytes.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "prox_ops.h"
#include "temporal_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LR_HD __host__ __device__
#else
#define LR_HD
#endif

namespace pnp {

constexpr int LR_MIN_BLOCK = 2, LR_MAX_BLOCK = 32;
constexpr int LR_THREADS = 256;
constexpr int LR_MAX_SWEEPS = 20;
constexpr int LR_MAX_GROUP = 16;                                   // patches of one workgroup, at most
constexpr size_t LR_LDS_BUDGET = 40 * 1024;                        // aim of one workgroup's LDS: four workgroups share a compute unit's 160 KiB
constexpr size_t LR_LDS_MAX = 160 * 1024;                          // what one workgroup may declare (beyond 64 KiB by opt-in)
constexpr int LR_MAX_SHIFTS = 1 << 16;                             // entries of a shift table

// Argument check of pnp_set_lowrank / pnp_lowrank_check: 0 = valid, else which rule fails (the first in this order)
enum { LR_OK = 0, LR_BAD_FRAMES = 1, LR_BAD_BLOCK = 2, LR_BAD_SHAPE = 3, LR_BAD_LDS = 4, LR_BAD_BATCH = 5 };

LR_HD constexpr int lr_even(int T) { return T + (T & 1); }
LR_HD constexpr int lr_stride(int T) { return T | 1; }
// values of R one patch holds in LDS
LR_HD constexpr size_t lr_tile_vals(int T, int b) { return (size_t)b * b * lr_stride(T); }
LR_HD constexpr size_t lr_square_vals(int T) { return (size_t)T * lr_stride(T); }
LR_HD constexpr size_t lr_patch_doubles(int T) { return lr_square_vals(T) + lr_even(T); }
LR_HD constexpr size_t lr_patch_vals(int T, int b, bool cnc) { return (cnc ? 2 : 1) * lr_tile_vals(T, b) + lr_square_vals(T) + T + 2; }
LR_HD constexpr size_t lr_patch_bytes(int T, int b, size_t real_bytes, bool cnc) {
    return (lr_patch_doubles(T) * sizeof(double) + lr_patch_vals(T, b, cnc) * real_bytes + 7) & ~(size_t)7;
}
// patches of a workgroup
LR_HD constexpr int lr_group(int T, int b, size_t real_bytes, bool cnc) {
    const size_t q = LR_LDS_BUDGET / lr_patch_bytes(T, b, real_bytes, cnc);
    return q < 1 ? 1 : (q > (size_t)LR_MAX_GROUP ? LR_MAX_GROUP : (int)q);
}
LR_HD constexpr size_t lr_lds_bytes(int T, int b, size_t real_bytes, bool cnc) { return lr_group(T, b, real_bytes, cnc) * lr_patch_bytes(T, b, real_bytes, cnc); }

LR_HD constexpr int lr_check(int frames, int block, int H, int W, int B, size_t real_bytes, bool cnc) {
    if (frames < TP_MIN_FRAMES || frames > TP_MAX_FRAMES) return LR_BAD_FRAMES;
    if (block < LR_MIN_BLOCK || block > LR_MAX_BLOCK) return LR_BAD_BLOCK;
    if (H < 1 || W < 1 || block > H || block > W) return LR_BAD_SHAPE;
    if (lr_patch_bytes(frames, block, real_bytes, cnc) > LR_LDS_MAX) return LR_BAD_LDS;
    if (B < 1 || B % frames) return LR_BAD_BATCH;
    return LR_OK;
}
LR_HD constexpr bool lr_shift_ok(int block, int sy, int sx) { return sy >= 0 && sx >= 0 && sy < block && sx < block; }
// entry of the shift table that prox step `cursor` uses
LR_HD constexpr int lr_shift_entry(int cursor, int n) { return cursor % n; }

LR_HD constexpr int lr_ceil_div(int a, int b) { return (a + b - 1) / b; }

// eps_R of the off-diagonal test: a sixty-fourth of the machine epsilon, 2^-29 resp. 2^-58.  Jacobi converges quadratically and a rotated
// entry is set to 0, so the sweep after the one that reaches the machine epsilon reaches this too; the vectors then carry the rotations'
// rounding alone (at the machine epsilon itself the float kernel stood 1.5 .. 4 x the float32 restatement from the oracle, growing with T)
template <typename R> struct LrEps;
template <> struct LrEps<float>  { static constexpr float  value = 1.862645149230957e-09f; };
template <> struct LrEps<double> { static constexpr double value = 3.469446951953614e-18; };

template <typename R> struct LrArgs {
    const R* x;             // [S T][H][W]
    R *z, *w;
    ProxParamsT<R> p;       // thr and ib scaled
    int H, W, T, S, b;
    int sy, sx;
    int Q, ny, nx, ngx;     // patches of a group; patch rows and columns of the grid; groups of a patch row
};
template <typename R> LR_HD inline void lr_fill_grid(LrArgs<R>& a, bool cnc) {
    a.Q = lr_group(a.T, a.b, sizeof(R), cnc);
    a.ny = lr_ceil_div(a.H, a.b);
    a.nx = lr_ceil_div(a.W, a.b);
    a.ngx = lr_ceil_div(a.nx, a.Q);
}
LR_HD constexpr size_t lr_groups(int S, int ny, int ngx) { return (size_t)S * ny * ngx; }

// group `gi` (patch row gi / ngx, group gi % ngx of it) of series s
struct LrGroup {
    size_t base;            // first value of the series
    int y0, ph;             // first row (before the shift) and rows of its patches
    int j0, nq;             // first patch column and patches
    int x0, span;           // first column (before the shift) and columns
};
template <typename R> LR_HD inline LrGroup lr_group_of(const LrArgs<R>& a, int s, int gi) {
    LrGroup g;
    const int i = gi / a.ngx, k = gi - i * a.ngx;
    g.base = (size_t)s * a.T * a.H * a.W;
    g.y0 = i * a.b;
    g.ph = a.H - g.y0 < a.b ? a.H - g.y0 : a.b;
    g.j0 = k * a.Q;
    g.nq = a.nx - g.j0 < a.Q ? a.nx - g.j0 : a.Q;
    g.x0 = g.j0 * a.b;
    g.span = a.W - g.x0 < g.nq * a.b ? a.W - g.x0 : g.nq * a.b;
    return g;
}
// columns and pixels of patch q of a group
template <typename R> LR_HD inline int lr_patch_width(const LrArgs<R>& a, const LrGroup& g, int q) {
    const int left = a.W - (g.j0 + q) * a.b;
    return left < a.b ? left : a.b;
}

// LDS parts of patch q
template <typename R> struct LrPatch { double *V, *rot; R *tile, *tile2, *G, *vec, *sc; };
template <typename R> LR_HD inline LrPatch<R> lr_patch_of(const LrArgs<R>& a, bool cnc, unsigned char* lds, int q) {
    LrPatch<R> t;
    unsigned char* base = lds + (size_t)q * lr_patch_bytes(a.T, a.b, sizeof(R), cnc);
    t.V = (double*)base;
    t.rot = t.V + lr_square_vals(a.T);
    R* p = (R*)(t.rot + lr_even(a.T));
    t.tile = p;  p += lr_tile_vals(a.T, a.b);
    t.tile2 = p; if (cnc) p += lr_tile_vals(a.T, a.b);
    t.G = p;     p += lr_square_vals(a.T);
    t.vec = p;   p += a.T;
    t.sc = p;
    return t;
}

// a pixel-frame of a group: item = (t, r, column of the span) -> its place in memory and in LDS
struct LrPlace { size_t o; int q, at, t; };                       // at: p TS + t in the tile of patch q
template <typename R> LR_HD inline LrPlace lr_place(int item, const LrArgs<R>& a, const LrGroup& g) {
    const int per = g.ph * g.span, t = item / per, rem = item - t * per, r = rem / g.span, cx = rem - r * g.span;
    const int q = cx / a.b, c = cx - q * a.b;
    int row = a.sy + g.y0 + r, col = a.sx + g.x0 + cx;
    if (row >= a.H) row -= a.H;
    if (col >= a.W) col -= a.W;
    LrPlace pl;
    pl.o = g.base + ((size_t)t * a.H + row) * a.W + col;
    pl.q = q;
    pl.at = (r * lr_patch_width(a, g, q) + c) * lr_stride(a.T) + t;
    pl.t = t;
    return pl;
}
template <typename R> LR_HD inline int lr_pixel_items(const LrArgs<R>& a, const LrGroup& g) { return a.T * g.ph * g.span; }

// load: L1 u = x + w, CNC z -> the first tile
template <typename R, bool CNC> LR_HD inline void lr_load_item(int item, const LrArgs<R>& a, const LrGroup& g, unsigned char* lds) {
    const LrPlace pl = lr_place(item, a, g);
    lr_patch_of(a, CNC, lds, pl.q).tile[pl.at] = CNC ? a.z[pl.o] : a.x[pl.o] + a.w[pl.o];
}

// Gram, item = (q, a, b): G_ab = sum_p X_pa X_pb, V = I
template <typename R> LR_HD inline void lr_gram_item(int item, const LrArgs<R>& a, const LrGroup& g, bool cnc, unsigned char* lds, int which) {
    const int T = a.T, TS = lr_stride(T), q = item / (T * T), rem = item - q * T * T, i = rem / T, j = rem - i * T;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    const R* X = which ? t.tile2 : t.tile;
    const int P = g.ph * lr_patch_width(a, g, q);
    R acc = R(0);
    for (int p = 0; p < P; ++p) acc = cpx_fma(X[p * TS + i], X[p * TS + j], acc);
    t.G[i * TS + j] = acc;
    t.V[i * TS + j] = i == j ? 1.0 : 0.0;
}
// row sums of squares, item = (q, i): vec_i = sum_j G_ij^2, the diagonal left out or not
template <typename R> LR_HD inline void lr_rowsum_item(int item, const LrArgs<R>& a, bool cnc, unsigned char* lds, bool diagonal) {
    const int T = a.T, TS = lr_stride(T), q = item / T, i = item - q * T;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    R acc = R(0);
    for (int j = 0; j < T; ++j) if (diagonal || j != i) acc = cpx_fma(t.G[i * TS + j], t.G[i * TS + j], acc);
    t.vec[i] = acc;
}
// item = q: the bar (eps ||G||_F)^2 of a fresh Gram matrix and the flag down, or the test of off^2 against the bar
template <typename R> LR_HD inline void lr_norm_item(int q, const LrArgs<R>& a, bool cnc, unsigned char* lds, bool first) {
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    R acc = R(0);
    for (int i = 0; i < a.T; ++i) acc = acc + t.vec[i];
    if (first) { t.sc[0] = (LrEps<R>::value * LrEps<R>::value) * acc; t.sc[1] = R(0); }
    else if (acc <= t.sc[0]) t.sc[1] = R(1);
}
template <typename R> LR_HD inline bool lr_all_passed(const LrArgs<R>& a, const LrGroup& g, bool cnc, unsigned char* lds) {
    bool all = true;
    for (int q = 0; q < g.nq; ++q) all = all && lr_patch_of(a, cnc, lds, q).sc[1] != R(0);
    return all;
}
// pair k of round r of the round-robin ordering on n (even) indices
struct LrPair { int p, q; };
LR_HD inline LrPair lr_pair(int n, int r, int k) {
    int i, j;
    if (k == 0) { i = n - 1; j = r; }
    else { i = (r + k) % (n - 1); j = (r + (n - 1) - k) % (n - 1); }
    return i < j ? LrPair{i, j} : LrPair{j, i};
}
LR_HD inline float  lr_sqrt(float a)  { return sqrtf(a); }
LR_HD inline double lr_sqrt(double a) { return sqrt(a); }
LR_HD inline float  lr_abs(float a)  { return fabsf(a); }
LR_HD inline double lr_abs(double a) { return fabs(a); }
// rotations, item = (q, k): (c, s) of pair k that annihilates G_pq; the identity for a padded pair, a patch that passed, G_pq = 0
template <typename R> LR_HD inline void lr_rot_item(int item, const LrArgs<R>& a, bool cnc, unsigned char* lds, int round) {
    const int T = a.T, TS = lr_stride(T), n = lr_even(T), half = n / 2, q = item / half, k = item - q * half;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    const LrPair pr = lr_pair(n, round, k);
    double c = 1.0, s = 0.0;
    if (pr.q < T && t.sc[1] == R(0)) {
        const double apq = (double)t.G[pr.p * TS + pr.q];
        if (apq != 0.0) {
            const double theta = ((double)t.G[pr.q * TS + pr.q] - (double)t.G[pr.p * TS + pr.p]) / (2.0 * apq);
            const double tn = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
            c = 1.0 / sqrt(fma(tn, tn, 1.0));
            s = tn * c;
            if (!(s == s) || !(c == c) || (R)s == R(0)) { c = 1.0; s = 0.0; }   // an overflowed theta, or a turn G would not feel: negligible
        }
    }
    t.rot[2 * k] = c;
    t.rot[2 * k + 1] = s;
}
// columns, item = (q, i, k): columns p, q of row i of G and of V
template <typename R> LR_HD inline void lr_col_item(int item, const LrArgs<R>& a, bool cnc, unsigned char* lds, int round) {
    const int T = a.T, TS = lr_stride(T), n = lr_even(T), half = n / 2, q = item / (T * half), rem = item - q * T * half, i = rem / half, k = rem - i * half;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    const double cd = t.rot[2 * k], sd = t.rot[2 * k + 1];
    if (sd == 0.0) return;
    const LrPair pr = lr_pair(n, round, k);
    const R c = (R)cd, s = (R)sd;
    R* g = t.G + i * TS;
    const R gp = g[pr.p], gq = g[pr.q];
    g[pr.p] = cpx_fma(c, gp, -(s * gq));
    g[pr.q] = cpx_fma(s, gp, c * gq);
    double* v = t.V + i * TS;
    const double vp = v[pr.p], vq = v[pr.q];
    v[pr.p] = fma(cd, vp, -(sd * vq));
    v[pr.q] = fma(sd, vp, cd * vq);
}
// rows, item = (q, k, j): rows p, q of column j of G; the rotated entry itself becomes 0
template <typename R> LR_HD inline void lr_row_item(int item, const LrArgs<R>& a, bool cnc, unsigned char* lds, int round) {
    const int T = a.T, TS = lr_stride(T), n = lr_even(T), half = n / 2, q = item / (T * half), rem = item - q * T * half, k = rem / T, j = rem - k * T;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    const R c = (R)t.rot[2 * k], s = (R)t.rot[2 * k + 1];
    if (s == R(0)) return;
    const LrPair pr = lr_pair(n, round, k);
    const R vp = t.G[pr.p * TS + j], vq = t.G[pr.q * TS + j];
    t.G[pr.p * TS + j] = j == pr.q ? R(0) : cpx_fma(c, vp, -(s * vq));
    t.G[pr.q * TS + j] = j == pr.p ? R(0) : cpx_fma(s, vp, c * vq);
}
// g(sigma), item = (q, j)
template <typename R> LR_HD inline void lr_gain_item(int item, const LrArgs<R>& a, bool cnc, unsigned char* lds, bool clip) {
    const int T = a.T, TS = lr_stride(T), q = item / T, j = item - q * T;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    const R lam = t.G[j * TS + j], sg = lr_sqrt(lam > R(0) ? lam : R(0));
    if (clip) t.vec[j] = sg > a.p.ib ? a.p.ib / sg : R(1);
    else      t.vec[j] = sg > a.p.thr ? (sg - a.p.thr) / sg : R(0);
}
// M = V diag(g) V^T into G's place, item = (q, a, b)
template <typename R> LR_HD inline void lr_map_item(int item, const LrArgs<R>& a, bool cnc, unsigned char* lds) {
    const int T = a.T, TS = lr_stride(T), q = item / (T * T), rem = item - q * T * T, i = rem / T, j = rem - i * T;
    const LrPatch<R> t = lr_patch_of(a, cnc, lds, q);
    double acc = 0.0;
    for (int e = 0; e < T; ++e) acc = fma(t.V[i * TS + e] * (double)t.vec[e], t.V[j * TS + e], acc);
    t.G[i * TS + j] = (R)acc;
}
// (X M)_pt of the pixel-frame at `pl`
template <typename R> LR_HD inline R lr_apply(const LrArgs<R>& a, const LrPatch<R>& t, const R* X, const LrPlace& pl) {
    const int T = a.T, TS = lr_stride(T);
    const R* row = X + (pl.at - pl.t);
    R acc = R(0);
    for (int e = 0; e < T; ++e) acc = cpx_fma(row[e], t.G[e * TS + pl.t], acc);
    return acc;
}
// CNC: t = c1 z + c2 u + c3 S_clip(z) -> the second tile
template <typename R> LR_HD inline void lr_combine_item(int item, const LrArgs<R>& a, const LrGroup& g, unsigned char* lds) {
    const LrPlace pl = lr_place(item, a, g);
    const LrPatch<R> t = lr_patch_of(a, true, lds, pl.q);
    const R u = a.x[pl.o] + a.w[pl.o];
    t.tile2[pl.at] = cpx_fma(a.p.c1, t.tile[pl.at], cpx_fma(a.p.c2, u, a.p.c3 * lr_apply(a, t, t.tile, pl)));
}
// store: z+ = (X M)_pt and w+ = u - z+ leave for memory
template <typename R, bool CNC> LR_HD inline void lr_store_item(int item, const LrArgs<R>& a, const LrGroup& g, unsigned char* lds) {
    const LrPlace pl = lr_place(item, a, g);
    const LrPatch<R> t = lr_patch_of(a, CNC, lds, pl.q);
    const R u = CNC ? a.x[pl.o] + a.w[pl.o] : t.tile[pl.at];
    const R zn = lr_apply(a, t, CNC ? t.tile2 : t.tile, pl);
    a.z[pl.o] = zn;
    a.w[pl.o] = u - zn;
}

// ---- the passes of one group -----------------------------------------------------------------------------------------------------------
// Exec: items(n, f) runs f(item) for every item < n, sync() is the barrier between two passes.  No item of a pass reads what another item
// of the same pass writes, so the passes may run their items in any order or side by side.

// eigen-decomposition of the Gram matrices of tile `which` of every patch of the group: G ends diagonal (to the bar), V holds the vectors
template <typename R, typename Exec>
LR_HD inline void lr_solve(const LrArgs<R>& a, const LrGroup& g, bool cnc, unsigned char* lds, int which, Exec& ex) {
    const int T = a.T, n = lr_even(T), half = n / 2, nq = g.nq;
    ex.items(nq * T * T, [&](int it) { lr_gram_item(it, a, g, cnc, lds, which); });
    ex.sync();
    ex.items(nq * T, [&](int it) { lr_rowsum_item(it, a, cnc, lds, true); });
    ex.sync();
    ex.items(nq, [&](int it) { lr_norm_item(it, a, cnc, lds, true); });
    ex.sync();
    for (int sweep = 0; sweep < LR_MAX_SWEEPS; ++sweep) {
        ex.items(nq * T, [&](int it) { lr_rowsum_item(it, a, cnc, lds, false); });
        ex.sync();
        ex.items(nq, [&](int it) { lr_norm_item(it, a, cnc, lds, false); });
        ex.sync();
        if (lr_all_passed(a, g, cnc, lds)) break;                  // the same on every thread: the flags change in the pass above alone
        for (int r = 0; r < n - 1; ++r) {
            ex.items(nq * half, [&](int it) { lr_rot_item(it, a, cnc, lds, r); });
            ex.sync();
            ex.items(nq * T * half, [&](int it) { lr_col_item(it, a, cnc, lds, r); });
            ex.sync();
            ex.items(nq * T * half, [&](int it) { lr_row_item(it, a, cnc, lds, r); });
            ex.sync();
        }
    }
}
// M = V g(sigma) V^T of every patch, into G's place
template <typename R, typename Exec>
LR_HD inline void lr_map(const LrArgs<R>& a, const LrGroup& g, bool cnc, unsigned char* lds, bool clip, Exec& ex) {
    ex.items(g.nq * a.T, [&](int it) { lr_gain_item(it, a, cnc, lds, clip); });
    ex.sync();
    ex.items(g.nq * a.T * a.T, [&](int it) { lr_map_item(it, a, cnc, lds); });
    ex.sync();
}
// group `gi` of series s on the LDS block `lds` (lr_lds_bytes)
template <typename R, bool CNC, typename Exec>
LR_HD inline void lr_run_group(const LrArgs<R>& a, int s, int gi, unsigned char* lds, Exec& ex) {
    const LrGroup g = lr_group_of(a, s, gi);
    const int pixels = lr_pixel_items(a, g);
    ex.items(pixels, [&](int it) { lr_load_item<R, CNC>(it, a, g, lds); });
    ex.sync();
    if (CNC) {
        lr_solve(a, g, true, lds, 0, ex);
        lr_map(a, g, true, lds, true, ex);
        ex.items(pixels, [&](int it) { lr_combine_item(it, a, g, lds); });
        ex.sync();
    }
    lr_solve(a, g, CNC, lds, CNC ? 1 : 0, ex);
    lr_map(a, g, CNC, lds, false, ex);
    ex.items(pixels, [&](int it) { lr_store_item<R, CNC>(it, a, g, lds); });
}

}  // namespace pnp
