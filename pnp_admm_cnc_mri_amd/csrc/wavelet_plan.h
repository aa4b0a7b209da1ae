// Wavelet-domain sparsity (pnp_set_sparsity, pnp_dwt2_*; kernels_wavelet.hip): the filters, the argument checks, the tiling of the two
// kernels and -- as work-item functions -- the index maps of every pass.  Host- and device-callable code without HIP: the kernels run
// these functions one item per thread, tests/host/wavelet_emulation.cpp runs them one item after another under g++ and the sanitizers.
//
// Psi is the orthonormal periodic 2-D DWT with filter h of length T (g[n] = (-1)^n h[T-1-n]); one level along an axis of length M:
//     a[k] = sum_n h[n] s[(2k + n) mod M],   d[k] = sum_n g[n] s[(2k + n) mod M],   k < M / 2;   synthesis = the transpose.
// 2-D, L levels, Mallat layout: level l = 0 .. L-1 works on the top-left (H >> l) x (W >> l) block, rows first ([a | d]), then
// columns ([a ; d]); the inverse undoes the levels in reverse order, columns first.  "Detail" = everything outside the final LL band,
// the top-left (H >> L) x (W >> L).  This regulariser has no counterpart in the reference scripts.
//
// Analysis (wv_fwd_*): a workgroup owns a tile x tile block of pixels, tile a multiple of 2^L, and with it the coefficients of every
// band at the same relative place.  In LOCAL coordinates -- index i stands for global index (origin >> l) + i, taken modulo the
// level's length only when the image is read -- a level needs of the level below 2 n + T - 2 samples for n outputs, so level l is
// computed on wv_fwd_ext(l) = (tile >> l) + (T - 2)(2^(L-l) - 1) samples per axis: the tile plus a right / bottom halo of
// (T - 2)(2^L - 1) pixels at level 0 (at 128 x 128, db4, L = 4 it wraps past the tile itself).  Level 0's row pass reads the image;
// two LDS arrays carry the rest: rowbuf [ext(l)][2 ext(l+1)] (a row pass' [a | d]) and ll [ext(l+1)]^2 (a column pass' LL band).
// Detail bands leave for memory from the column pass of their level, the LL band from the last one.
//
// Synthesis (wv_inv_*): the same tile of pixels; output m of a level needs the coefficients k = (m - n) / 2, n = m mod 2, .. < T, so a
// left / top halo: level l is rebuilt on wv_inv_ext(l) = (tile >> l) + e_l samples per axis, e_0 = 0, e_(l+1) = ceil((e_l + T - 2) / 2)
// (< T - 2).  colbuf [ext(l)][2 ext(l+1)] holds a column pass' result, ll [ext(l)]^2 the rebuilt LL band of level l >= 1.
//
// Cycle spinning (WvTile::sy, sx; wv_spin_check): the transform of the circularly shifted frame, Psi_s = Psi R_s with
// (R_s v)[i, j] = v[(i + sy) mod H, (j + sx) mod W], 0 <= sy, sx < 2^L.  Only the two places that touch the image know of it -- level 0 of
// the analysis row pass reads pixel (i + sy, j + sx), level 0 of the synthesis row pass emits to it; the coefficients stay in the Mallat
// layout of the shifted frame, and tiles, items, LDS sizes and arithmetic are those of s = (0, 0).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WV_HD __host__ __device__
#else
#define WV_HD
#endif

namespace pnp {

enum { WV_NONE = 0, WV_HAAR = 1, WV_DB2 = 2, WV_DB4 = 3 };       // PNP_WAVELET_* of include/pnp_mri.h
constexpr int WV_MAX_LEVELS = 4;
constexpr int WV_THREADS = 256;
constexpr size_t WV_LDS_MAX = 160 * 1024;                          // LDS of one compute unit

// filter length by name (0: not a wavelet)
WV_HD constexpr int wv_taps(int wavelet) { return wavelet == WV_HAAR ? 2 : wavelet == WV_DB2 ? 4 : wavelet == WV_DB4 ? 8 : 0; }

// Low-pass filters in double.  haar: [1, 1] / sqrt 2; db2: [1 + r, 3 + r, 3 - r, 1 - r] / (4 sqrt 2), r = sqrt 3; db4: minimum-phase
// Daubechies with four vanishing moments, (1 + z)^4 prod (1 - z_k z) over the roots z_k inside the unit circle from
// P(y) = sum_{k<4} C(3 + k, k) y^k, y = (2 - z - 1/z) / 4, normalised to sum h = sqrt 2 -- derived in extended precision
// (tests/wavelet_oracle.py, _daubechies) and rounded once; tests/test_wavelet_host.py checks them against that derivation.
template <int T> WV_HD constexpr double wv_h(int n);
template <> WV_HD constexpr double wv_h<2>(int) { return 0.70710678118654757; }
template <> WV_HD constexpr double wv_h<4>(int n) {
    return n == 0 ? 0.4829629131445341 : n == 1 ? 0.83651630373780772 : n == 2 ? 0.22414386804201339 : -0.12940952255126034;
}
template <> WV_HD constexpr double wv_h<8>(int n) {
    return n == 0 ? 0.23037781330889651 : n == 1 ? 0.71484657055291567 : n == 2 ? 0.63088076792985892 : n == 3 ? -0.027983769416859854
         : n == 4 ? -0.18703481171909309 : n == 5 ? 0.030841381835560764 : n == 6 ? 0.032883011666885197 : -0.010597401785069032;
}
template <int T> WV_HD constexpr double wv_g(int n) { return (n & 1) ? -wv_h<T>(T - 1 - n) : wv_h<T>(T - 1 - n); }

// Argument check of pnp_set_sparsity: 0 = valid, else which rule fails
enum { WV_OK = 0, WV_BAD_NAME = 1, WV_BAD_LEVELS = 2, WV_BAD_DIVISOR = 3, WV_TOO_SHORT = 4 };
WV_HD constexpr int wv_check(int wavelet, int levels, int H, int W) {
    if (wv_taps(wavelet) == 0) return WV_BAD_NAME;
    if (levels < 1 || levels > WV_MAX_LEVELS) return WV_BAD_LEVELS;
    if (H < 1 || W < 1 || H % (1 << levels) || W % (1 << levels)) return WV_BAD_DIVISOR;
    if (((H < W ? H : W) >> (levels - 1)) < wv_taps(wavelet)) return WV_TOO_SHORT;       // the input of the last level
    return WV_OK;
}

// ---- tiling -------------------------------------------------------------------------------------------------------------------
WV_HD constexpr int wv_fwd_halo(int T, int L) { return (T - 2) * ((1 << L) - 1); }
// Tile edge (pixels): 64 while the analysis halo is at most 16 pixels (haar; db2 to L = 3; db4 at L = 1), else 32.  Both are
// multiples of 2^L for every L <= 4; the image need not be a multiple of the tile (partial tiles compute wrapped data and drop it).
WV_HD constexpr int wv_tile(int T, int L) { return wv_fwd_halo(T, L) <= 16 ? 64 : 32; }
WV_HD constexpr int wv_fwd_ext(int T, int L, int tile, int l) { return (tile >> l) + (T - 2) * ((1 << (L - l)) - 1); }
WV_HD constexpr int wv_inv_halo(int T, int l) {                    // e_l
    int e = 0;
    for (int i = 0; i < l; ++i) e = (e + T - 2 + 1) / 2;
    return e;
}
WV_HD constexpr int wv_inv_ext(int T, int tile, int l) { return (tile >> l) + wv_inv_halo(T, l); }
// LDS elements of one workgroup: rowbuf + ll (analysis), colbuf + ll (synthesis)
WV_HD constexpr size_t wv_fwd_rowbuf_elems(int T, int L, int tile) { return (size_t)wv_fwd_ext(T, L, tile, 0) * 2 * wv_fwd_ext(T, L, tile, 1); }
WV_HD constexpr size_t wv_fwd_ll_elems(int T, int L, int tile) { return (size_t)wv_fwd_ext(T, L, tile, 1) * wv_fwd_ext(T, L, tile, 1); }
WV_HD constexpr size_t wv_fwd_lds_elems(int T, int L, int tile) { return wv_fwd_rowbuf_elems(T, L, tile) + wv_fwd_ll_elems(T, L, tile); }
WV_HD constexpr size_t wv_inv_colbuf_elems(int T, int tile) { return (size_t)tile * 2 * wv_inv_ext(T, tile, 1); }
WV_HD constexpr size_t wv_inv_ll_elems(int T, int tile) { return (size_t)wv_inv_ext(T, tile, 1) * wv_inv_ext(T, tile, 1); }
WV_HD constexpr size_t wv_inv_lds_elems(int T, int tile) { return wv_inv_colbuf_elems(T, tile) + wv_inv_ll_elems(T, tile); }
WV_HD constexpr int wv_tiles(int n, int tile) { return (n + tile - 1) / tile; }

// i modulo M for the few periods a halo can leave the image by (either side)
WV_HD inline int wv_wrap(int i, int M) {
    while (i >= M) i -= M;
    while (i < 0) i += M;
    return i;
}
// i modulo M for 0 <= i < 2 M: a pixel of the image moved by a shift (< 2^L <= M)
WV_HD inline int wv_wrap_once(int i, int M) { return i >= M ? i - M : i; }
// band test: is (y, x) of the Mallat layout a detail coefficient, i.e. outside the final LL band
WV_HD constexpr bool wv_is_detail(int y, int x, int H, int W, int L) { return !(y < (H >> L) && x < (W >> L)); }

WV_HD inline float  wv_fma(float a, float b, float c)    { return fmaf(a, b, c); }
WV_HD inline double wv_fma(double a, double b, double c) { return fma(a, b, c); }

// One tile of one slice
struct WvTile {
    int H, W, L, tile;
    int ty0, tx0;           // origin of the tile in pixels (multiples of tile)
    size_t base;            // offset of the slice: b * H * W
    int sy = 0, sx = 0;     // cycle spinning: the frame's shift, pixel (i, j) of the frame is pixel (i + sy, j + sx) of the image (periodic)
};

// Argument check of pnp_set_spin / pnp_spin_check: a table shifts[n][2] used per_prox entries per prox step; 0 = valid, else which rule fails
constexpr int WV_SPIN_MAX_N = 4096, WV_SPIN_MAX_K = 16;
enum { WV_SPIN_OK = 0, WV_SPIN_BAD_LEVELS = 1, WV_SPIN_BAD_N = 2, WV_SPIN_BAD_K = 3, WV_SPIN_BAD_MULTIPLE = 4, WV_SPIN_BAD_RANGE = 5 };
WV_HD constexpr bool wv_shift_ok(int levels, int sy, int sx) { return sy >= 0 && sx >= 0 && sy < (1 << levels) && sx < (1 << levels); }
WV_HD inline int wv_spin_check(int levels, const int* shifts, int n, int per_prox) {
    if (levels < 1 || levels > WV_MAX_LEVELS) return WV_SPIN_BAD_LEVELS;
    if (n < 1 || n > WV_SPIN_MAX_N || !shifts) return WV_SPIN_BAD_N;
    if (per_prox < 1 || per_prox > WV_SPIN_MAX_K) return WV_SPIN_BAD_K;
    if (n % per_prox) return WV_SPIN_BAD_MULTIPLE;
    for (int i = 0; i < n; ++i) if (!wv_shift_ok(levels, shifts[2 * i], shifts[2 * i + 1])) return WV_SPIN_BAD_RANGE;
    return WV_SPIN_OK;
}
// the table entries of prox step `cursor`: first index of its group of per_prox entries
WV_HD constexpr int wv_spin_first(int cursor, int n, int per_prox) { return (cursor % (n / per_prox)) * per_prox; }

// ---- analysis: work items -------------------------------------------------------------------------------------------------------
// Items of the row pass / the column pass of level l
WV_HD constexpr int wv_fwd_row_items(int T, const WvTile& t, int l) { return wv_fwd_ext(T, t.L, t.tile, l) * wv_fwd_ext(T, t.L, t.tile, l + 1); }
WV_HD constexpr int wv_fwd_col_items(int T, const WvTile& t, int l) { return 2 * wv_fwd_ext(T, t.L, t.tile, l + 1) * wv_fwd_ext(T, t.L, t.tile, l + 1); }

// Row pass of level l, item = (row r of the level's input, output column kx): a and d of that row into rowbuf [r][kx], [r][n_out + kx].
// Level 0 reads the image: in0 (+ in1 when non-null: the sum is formed on the way in) at the frame's shift with periodic wrap; level >= 1 reads ll.
// Only what the column pass will read is computed: of the last level, and of every d, the part that lands inside the tile.
template <typename R, int T>
WV_HD inline void wv_fwd_row_item(int item, int l, const WvTile& t, const R* in0, const R* in1, const R* ll, R* rowbuf) {
    const int n_in = wv_fwd_ext(T, t.L, t.tile, l), n_out = wv_fwd_ext(T, t.L, t.tile, l + 1), tl = t.tile >> (l + 1);
    const int r = item / n_out, kx = item - r * n_out;
    const bool inside = kx < tl && r < 2 * tl + T - 2;
    const bool need_a = (l + 1 < t.L) || inside, need_d = inside;
    if (!need_a) return;
    R s[T];
    if (l == 0) {
        const size_t row = t.base + (size_t)wv_wrap(t.ty0 + r + t.sy, t.H) * t.W;
        for (int n = 0; n < T; ++n) {
            const size_t p = row + wv_wrap(t.tx0 + 2 * kx + n + t.sx, t.W);
            s[n] = in1 ? in0[p] + in1[p] : in0[p];
        }
    } else {
        for (int n = 0; n < T; ++n) s[n] = ll[r * n_in + 2 * kx + n];
    }
    R a = (R)wv_h<T>(0) * s[0];
    for (int n = 1; n < T; ++n) a = wv_fma((R)wv_h<T>(n), s[n], a);
    rowbuf[r * 2 * n_out + kx] = a;
    if (need_d) {
        R d = (R)wv_g<T>(0) * s[0];
        for (int n = 1; n < T; ++n) d = wv_fma((R)wv_g<T>(n), s[n], d);
        rowbuf[r * 2 * n_out + n_out + kx] = d;
    }
}

// Column pass of level l, item = (output row ky, column c of rowbuf): the a of a row-a column goes on to ll (or, at the last level, out as
// the final LL band), every other result is a detail coefficient of level l + 1 and leaves through emit(offset, value, detail) when it
// lies inside the tile and the image.  Offsets are those of the Mallat layout of the whole slice.
template <typename R, int T, typename Emit>
WV_HD inline void wv_fwd_col_item(int item, int l, const WvTile& t, const R* rowbuf, R* ll, Emit&& emit) {
    const int n_out = wv_fwd_ext(T, t.L, t.tile, l + 1), tl = t.tile >> (l + 1);
    const int Hl = t.H >> (l + 1), Wl = t.W >> (l + 1);
    const int ky = item / (2 * n_out), c = item - ky * 2 * n_out;
    const bool row_d = c >= n_out, last = l + 1 == t.L;
    const int cx = row_d ? c - n_out : c;
    const int gy = (t.ty0 >> (l + 1)) + ky, gx = (t.tx0 >> (l + 1)) + cx;
    const bool out = ky < tl && cx < tl && gy < Hl && gx < Wl;
    const bool need_a = out || (!row_d && !last);
    if (!need_a) return;
    R s[T];
    for (int n = 0; n < T; ++n) s[n] = rowbuf[(2 * ky + n) * 2 * n_out + c];
    R a = (R)wv_h<T>(0) * s[0];
    for (int n = 1; n < T; ++n) a = wv_fma((R)wv_h<T>(n), s[n], a);
    if (!row_d && !last) ll[ky * n_out + cx] = a;
    if (!out) return;
    R d = (R)wv_g<T>(0) * s[0];
    for (int n = 1; n < T; ++n) d = wv_fma((R)wv_g<T>(n), s[n], d);
    const size_t top = t.base + (size_t)gy * t.W + gx + (row_d ? Wl : 0), bottom = top + (size_t)Hl * t.W;
    if (row_d) emit(top, a, true);
    else if (last) emit(top, a, false);
    emit(bottom, d, true);
}

// ---- synthesis: work items ------------------------------------------------------------------------------------------------------
WV_HD constexpr int wv_inv_col_items(int T, const WvTile& t, int l) { return wv_inv_ext(T, t.tile, l) * 2 * wv_inv_ext(T, t.tile, l + 1); }
WV_HD constexpr int wv_inv_row_items(int T, const WvTile& t, int l) { return wv_inv_ext(T, t.tile, l) * wv_inv_ext(T, t.tile, l); }

// the taps of one output: local output index v = i - e_l (may be negative) takes n = (v mod 2), + 2, .. from the coefficient at local
// index (v - n) / 2 + e_(l+1); T / 2 terms each of h and g
template <typename R, int T, typename A, typename D>
WV_HD inline R wv_inv_taps(int v, int e1, A&& a, D&& d) {
    const int par = v & 1;
    R acc = R(0);
    for (int nn = 0; nn < T / 2; ++nn) {
        const int n = 2 * nn + par, j = (v - n) / 2 + e1;            // v - n is even: exact
        const R hn = (R)(par ? wv_h<T>(2 * nn + 1) : wv_h<T>(2 * nn)), gn = (R)(par ? wv_g<T>(2 * nn + 1) : wv_g<T>(2 * nn));
        acc = wv_fma(hn, a(j), acc);
        acc = wv_fma(gn, d(j), acc);
    }
    return acc;
}

// Column pass that undoes the columns of level l + 1, item = (row i of level l's local block, column c of [a-columns | d-columns]):
// the detail bands come from the coefficient array c (Mallat layout, periodic wrap), the LL band from ll -- at the last level from c too.
template <typename R, int T>
WV_HD inline void wv_inv_col_item(int item, int l, const WvTile& t, const R* coef, const R* ll, R* colbuf) {
    const int m_in = wv_inv_ext(T, t.tile, l + 1), e0 = wv_inv_halo(T, l), e1 = wv_inv_halo(T, l + 1);
    const int Hl = t.H >> (l + 1), Wl = t.W >> (l + 1);
    const int i = item / (2 * m_in), c = item - i * 2 * m_in;
    const bool row_d = c >= m_in, last = l + 1 == t.L;
    const int cx = row_d ? c - m_in : c;
    const int gx = wv_wrap((t.tx0 >> (l + 1)) - e1 + cx, Wl) + (row_d ? Wl : 0);
    const int gy0 = (t.ty0 >> (l + 1)) - e1;
    auto band = [&](int j, bool col_d) { return coef[t.base + (size_t)(wv_wrap(gy0 + j, Hl) + (col_d ? Hl : 0)) * t.W + gx]; };
    colbuf[i * 2 * m_in + c] = wv_inv_taps<R, T>(
        i - e0, e1, [&](int j) { return (row_d || last) ? band(j, false) : ll[j * m_in + cx]; }, [&](int j) { return band(j, true); });
}

// Row pass that undoes the rows of level l + 1, item = (row iy, column ix of level l's local block): into ll for l >= 1; at l = 0 the
// pixel leaves through emit(offset, value) when it lies inside the image -- for its place in the image, the frame's shift away.
template <typename R, int T, typename Emit>
WV_HD inline void wv_inv_row_item(int item, int l, const WvTile& t, const R* colbuf, R* ll, Emit&& emit) {
    const int m_out = wv_inv_ext(T, t.tile, l), m_in = wv_inv_ext(T, t.tile, l + 1), e0 = wv_inv_halo(T, l), e1 = wv_inv_halo(T, l + 1);
    const int iy = item / m_out, ix = item - iy * m_out;
    const R* row = colbuf + iy * 2 * m_in;
    const R v = wv_inv_taps<R, T>(ix - e0, e1, [&](int j) { return row[j]; }, [&](int j) { return row[m_in + j]; });
    if (l > 0) { ll[iy * m_out + ix] = v; return; }
    const int gy = t.ty0 + iy, gx = t.tx0 + ix;
    if (gy < t.H && gx < t.W) emit(t.base + (size_t)wv_wrap_once(gy + t.sy, t.H) * t.W + wv_wrap_once(gx + t.sx, t.W), v);
}

}  // namespace pnp
