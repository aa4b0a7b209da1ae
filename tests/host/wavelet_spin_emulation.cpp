// Host emulation of kernels_wavelet.hip with cycle spinning: the work-item functions of csrc/wavelet_plan.h, run tile by tile and item by item
// in SHIFTED frames (WvTile::sy, sx), with LDS arrays of exactly the plan's sizes (poisoned with NaN before every image), on whole-slice
// arrays of exactly B H W values -- under AddressSanitizer every index the kernels form is checked -- and the averaging of K shifts in the
// order the library's synthesis launches apply it.  Structure and flags of wavelet_emulation.cpp.
//   wavelet_spin_emulation run in.bin out.bin   header: int32 wavelet, L, H, W, B, mode (0 Psi_s, 1 Psi_s^T, 2 L1 prox, 3 CNC prox), f64, K;
//                                               K pairs int32 (sy, sx) (mode 0 / 1: K = 1); 5 doubles thr, c1, c2, c3, ib; then the arrays
//                                               (mode 0 / 1: in; 2 / 3: x, z, w) in float or double
//                                               out: mode 0 / 1: out; 2 / 3: z+, w+
//   wavelet_spin_emulation check L K n sy sx    prints wv_spin_check's code for a table of n entries, all (sy, sx)
//   wavelet_spin_emulation first cursor n K     prints wv_spin_first
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../pnp_admm_cnc_mri_amd/csrc/prox_params.h"
#include "../../pnp_admm_cnc_mri_amd/csrc/wavelet_plan.h"

using namespace pnp;

template <typename R> static R soft(R a, R c) {
    const R m = std::fabs(a) - c;
    const R r = m > R(0) ? m : R(0);
    return a < R(0) ? -r : r;
}

static int g_bad_detail = 0;      // emit's detail flag must agree with the band test

template <typename R, int T>
static void fwd_image(const WvTile& t, const R* in0, const R* in1, R* c, int mode /* 0 store, 1 L1, 2 CNC combine */, const ProxParamsT<R>& p) {
    const R nan = std::numeric_limits<R>::quiet_NaN();
    std::vector<R> rowbuf(wv_fwd_rowbuf_elems(T, t.L, t.tile), nan), ll(wv_fwd_ll_elems(T, t.L, t.tile), nan);
    const size_t N = (size_t)t.H * t.W;
    auto emit = [&](size_t o, R v, bool detail) {
        const size_t q = o - t.base;
        if (o < t.base || q >= N || detail != wv_is_detail((int)(q / t.W), (int)(q % t.W), t.H, t.W, t.L)) { ++g_bad_detail; return; }
        if (mode == 0) c[o] = v;
        else if (mode == 1) c[o] = detail ? soft(v, p.thr) : v;
        else {
            const R cz = c[o];
            if (detail) {
                const R clipz = cz < -p.ib ? -p.ib : (cz > p.ib ? p.ib : cz);
                c[o] = soft(wv_fma(p.c1, cz, wv_fma(p.c2, v, p.c3 * clipz)), p.thr);
            } else c[o] = wv_fma(p.c1, cz, p.c2 * v);
        }
    };
    for (int l = 0; l < t.L; ++l) {
        for (int it = 0, n = wv_fwd_row_items(T, t, l); it < n; ++it) wv_fwd_row_item<R, T>(it, l, t, in0, in1, ll.data(), rowbuf.data());
        for (int it = 0, n = wv_fwd_col_items(T, t, l); it < n; ++it) wv_fwd_col_item<R, T>(it, l, t, rowbuf.data(), ll.data(), emit);
    }
}

template <typename R, int T, typename Emit>
static void inv_image(const WvTile& t, const R* coef, Emit&& emit) {
    const R nan = std::numeric_limits<R>::quiet_NaN();
    std::vector<R> colbuf(wv_inv_colbuf_elems(T, t.tile), nan), ll(wv_inv_ll_elems(T, t.tile), nan);
    for (int l = t.L - 1; l >= 0; --l) {
        for (int it = 0, n = wv_inv_col_items(T, t, l); it < n; ++it) wv_inv_col_item<R, T>(it, l, t, coef, ll.data(), colbuf.data());
        for (int it = 0, n = wv_inv_row_items(T, t, l); it < n; ++it) wv_inv_row_item<R, T>(it, l, t, colbuf.data(), ll.data(), emit);
    }
}

template <typename F> static void for_tiles(int B, int H, int W, int L, int tile, int sy, int sx, F&& f) {
    for (int b = 0; b < B; ++b)
        for (int ty = 0; ty < wv_tiles(H, tile); ++ty)
            for (int tx = 0; tx < wv_tiles(W, tile); ++tx) {
                WvTile t{H, W, L, tile, ty * tile, tx * tile, (size_t)b * H * W};
                t.sy = sy; t.sx = sx;
                f(t);
            }
}

template <typename R, int T>
static int run_t(FILE* fi, FILE* fo, int L, int H, int W, int B, int mode, const double* pd, const std::vector<int32_t>& sh) {
    const size_t n = (size_t)B * H * W;
    const int K = (int)(sh.size() / 2);
    const R nan = std::numeric_limits<R>::quiet_NaN();
    const ProxParamsT<R> p{(R)pd[0], (R)pd[1], (R)pd[2], (R)pd[3], (R)pd[4]};
    std::vector<R> a0(n), a1, a2, coef(n, nan), out0(n, nan), out1, acc;
    if (fread(a0.data(), sizeof(R), n, fi) != n) return 2;
    if (mode >= 2) {
        a1.resize(n); a2.resize(n); out1.assign(n, nan); acc.assign(n, nan);
        if (fread(a1.data(), sizeof(R), n, fi) != n || fread(a2.data(), sizeof(R), n, fi) != n) return 2;
    } else if (K != 1) return 7;
    const int tile = wv_tile(T, L);
    if (wv_fwd_lds_elems(T, L, tile) * sizeof(R) > WV_LDS_MAX || wv_inv_lds_elems(T, tile) * sizeof(R) > WV_LDS_MAX) return 3;
    int twice = 0;
    const R rk = (R)(1.0 / K);
    // z+ and w+ go to out0 / out1, never into z (a1) or w (a2): every shift's analysis sees the old state, as on the card, where the last
    // synthesis alone writes them
    for (int j = 0; j < K; ++j) {
        const int sy = sh[2 * j], sx = sh[2 * j + 1];
        std::vector<char> seen(n, 0);
        if (mode != 1) for_tiles(B, H, W, L, tile, sy, sx, [&](const WvTile& t) {
            if (mode == 0) fwd_image<R, T>(t, a0.data(), (const R*)nullptr, out0.data(), 0, p);
            if (mode == 2) fwd_image<R, T>(t, a0.data(), a2.data(), coef.data(), 1, p);                  // x, w
            if (mode == 3) {
                fwd_image<R, T>(t, a1.data(), (const R*)nullptr, coef.data(), 0, p);                      // z
                fwd_image<R, T>(t, a0.data(), a2.data(), coef.data(), 2, p);
            }
        });
        if (mode != 0) for_tiles(B, H, W, L, tile, sy, sx, [&](const WvTile& t) {
            if (mode == 1) inv_image<R, T>(t, a0.data(), [&](size_t i, R v) { twice += seen[i]++; out0[i] = v; });
            else inv_image<R, T>(t, coef.data(), [&](size_t i, R v) {
                twice += seen[i]++;
                if (K > 1 && j == 0) { acc[i] = v; return; }
                if (K > 1 && j < K - 1) { acc[i] = acc[i] + v; return; }
                const R u = a0[i] + a2[i];
                const R zn = K > 1 ? (acc[i] + v) * rk : v;
                out0[i] = zn;
                out1[i] = u - zn;
            });
        });
        if (mode != 0) for (size_t i = 0; i < n; ++i) if (!seen[i]) { fprintf(stderr, "pixel %zu not written by shift %d\n", i, j); return 4; }
    }
    if (twice || g_bad_detail) { fprintf(stderr, "written twice: %d, bad band flags: %d\n", twice, g_bad_detail); return 4; }
    fwrite(out0.data(), sizeof(R), n, fo);
    if (mode >= 2) fwrite(out1.data(), sizeof(R), n, fo);
    return 0;
}

template <typename R>
static int run_r(FILE* fi, FILE* fo, int wavelet, int L, int H, int W, int B, int mode, const double* pd, const std::vector<int32_t>& sh) {
    switch (wv_taps(wavelet)) {
    case 2: return run_t<R, 2>(fi, fo, L, H, W, B, mode, pd, sh);
    case 4: return run_t<R, 4>(fi, fo, L, H, W, B, mode, pd, sh);
    case 8: return run_t<R, 8>(fi, fo, L, H, W, B, mode, pd, sh);
    }
    return 5;
}

int main(int argc, char** argv) {
    if (argc == 7 && !strcmp(argv[1], "check")) {
        const int n = atoi(argv[4]);
        std::vector<int> table;
        for (int i = 0; i < (n > 0 ? n : 0); ++i) { table.push_back(atoi(argv[5])); table.push_back(atoi(argv[6])); }
        printf("%d\n", wv_spin_check(atoi(argv[2]), table.empty() ? nullptr : table.data(), n, atoi(argv[3])));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "first")) {
        printf("%d\n", wv_spin_first(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])));
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "run")) return 1;
    FILE* fi = fopen(argv[2], "rb");
    FILE* fo = fopen(argv[3], "wb");
    if (!fi || !fo) return 1;
    int32_t h[8];
    double pd[5];
    if (fread(h, sizeof(int32_t), 8, fi) != 8 || h[7] < 1 || h[7] > WV_SPIN_MAX_K) return 2;
    std::vector<int32_t> sh(2 * (size_t)h[7]);
    if (fread(sh.data(), sizeof(int32_t), sh.size(), fi) != sh.size() || fread(pd, sizeof(double), 5, fi) != 5) return 2;
    if (wv_check(h[0], h[1], h[2], h[3]) != WV_OK) return 6;
    if (wv_spin_check(h[1], sh.data(), h[7], h[7]) != WV_SPIN_OK) return 8;
    const int rc = h[6] ? run_r<double>(fi, fo, h[0], h[1], h[2], h[3], h[4], h[5], pd, sh) : run_r<float>(fi, fo, h[0], h[1], h[2], h[3], h[4], h[5], pd, sh);
    fclose(fi);
    fclose(fo);
    return rc;
}
