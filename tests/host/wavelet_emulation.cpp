// Host emulation of kernels_wavelet.hip: the work-item functions of csrc/wavelet_plan.h, run tile by tile and item by item with LDS arrays
// of exactly the plan's sizes (poisoned with NaN before every image), on whole-slice arrays of exactly B H W values -- under
// AddressSanitizer every index the kernels form is checked, and the result goes back to the test for comparison with the whole-image oracle.
//   wavelet_emulation run  in.bin out.bin    header: int32 wavelet, L, H, W, B, mode (0 Psi, 1 Psi^T, 2 L1 prox, 3 CNC prox), f64;
//                                            5 doubles thr, c1, c2, c3, ib; then the arrays (mode 0 / 1: in; 2 / 3: x, z, w) in float or double
//                                            out: mode 0 / 1: out; 2 / 3: z+, w+
//   wavelet_emulation plan                   one line per (wavelet, L, precision): tile, halo, LDS bytes of the two kernels
//   wavelet_emulation check wavelet L H W    prints wv_check's code
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

template <typename R, int T>
static int run_t(FILE* fi, FILE* fo, int L, int H, int W, int B, int mode, const double* pd) {
    const size_t n = (size_t)B * H * W;
    const R nan = std::numeric_limits<R>::quiet_NaN();
    const ProxParamsT<R> p{(R)pd[0], (R)pd[1], (R)pd[2], (R)pd[3], (R)pd[4]};
    std::vector<R> a0(n), a1, a2, coef(n, nan), out0(n, nan), out1;
    if (fread(a0.data(), sizeof(R), n, fi) != n) return 2;
    if (mode >= 2) {
        a1.resize(n); a2.resize(n); out1.assign(n, nan);
        if (fread(a1.data(), sizeof(R), n, fi) != n || fread(a2.data(), sizeof(R), n, fi) != n) return 2;
    }
    const int tile = wv_tile(T, L);
    if (wv_fwd_lds_elems(T, L, tile) * sizeof(R) > WV_LDS_MAX || wv_inv_lds_elems(T, tile) * sizeof(R) > WV_LDS_MAX) return 3;
    std::vector<char> seen(n, 0);
    int twice = 0;
    for (int b = 0; b < B; ++b)
        for (int ty = 0; ty < wv_tiles(H, tile); ++ty)
            for (int tx = 0; tx < wv_tiles(W, tile); ++tx) {
                const WvTile t{H, W, L, tile, ty * tile, tx * tile, (size_t)b * H * W};
                if (mode == 0) fwd_image<R, T>(t, a0.data(), (const R*)nullptr, out0.data(), 0, p);
                if (mode == 2) fwd_image<R, T>(t, a0.data(), a2.data(), coef.data(), 1, p);                  // x, w
                if (mode == 3) {
                    fwd_image<R, T>(t, a1.data(), (const R*)nullptr, coef.data(), 0, p);                      // z
                    fwd_image<R, T>(t, a0.data(), a2.data(), coef.data(), 2, p);
                }
            }
    for (int b = 0; b < B && mode != 0; ++b)
        for (int ty = 0; ty < wv_tiles(H, tile); ++ty)
            for (int tx = 0; tx < wv_tiles(W, tile); ++tx) {
                const WvTile t{H, W, L, tile, ty * tile, tx * tile, (size_t)b * H * W};
                if (mode == 1) inv_image<R, T>(t, a0.data(), [&](size_t i, R v) { twice += seen[i]++; out0[i] = v; });
                else inv_image<R, T>(t, coef.data(), [&](size_t i, R v) {
                    twice += seen[i]++;
                    const R u = a0[i] + a2[i];
                    out0[i] = v;
                    out1[i] = u - v;
                });
            }
    if (twice || g_bad_detail) { fprintf(stderr, "written twice: %d, bad band flags: %d\n", twice, g_bad_detail); return 4; }
    fwrite(out0.data(), sizeof(R), n, fo);
    if (mode >= 2) fwrite(out1.data(), sizeof(R), n, fo);
    return 0;
}

template <typename R>
static int run_r(FILE* fi, FILE* fo, int wavelet, int L, int H, int W, int B, int mode, const double* pd) {
    switch (wv_taps(wavelet)) {
    case 2: return run_t<R, 2>(fi, fo, L, H, W, B, mode, pd);
    case 4: return run_t<R, 4>(fi, fo, L, H, W, B, mode, pd);
    case 8: return run_t<R, 8>(fi, fo, L, H, W, B, mode, pd);
    }
    return 5;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "plan")) {
        for (int wv = WV_HAAR; wv <= WV_DB4; ++wv)
            for (int L = 1; L <= WV_MAX_LEVELS; ++L)
                for (int bytes = 4; bytes <= 8; bytes += 4) {
                    const int T = wv_taps(wv), tile = wv_tile(T, L);
                    printf("%d %d %d %d %d %zu %zu\n", wv, L, bytes, tile, wv_fwd_halo(T, L), wv_fwd_lds_elems(T, L, tile) * bytes,
                           wv_inv_lds_elems(T, tile) * bytes);
                }
        printf("filters");
        for (int n = 0; n < 2; ++n) printf(" %.17g", wv_h<2>(n));
        for (int n = 0; n < 4; ++n) printf(" %.17g", wv_h<4>(n));
        for (int n = 0; n < 8; ++n) printf(" %.17g", wv_h<8>(n));
        printf("\n");
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "check")) {
        printf("%d\n", wv_check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "run")) return 1;
    FILE* fi = fopen(argv[2], "rb");
    FILE* fo = fopen(argv[3], "wb");
    if (!fi || !fo) return 1;
    int32_t h[7];
    double pd[5];
    if (fread(h, sizeof(int32_t), 7, fi) != 7 || fread(pd, sizeof(double), 5, fi) != 5) return 2;
    if (wv_check(h[0], h[1], h[2], h[3]) != WV_OK) return 6;
    const int rc = h[6] ? run_r<double>(fi, fo, h[0], h[1], h[2], h[3], h[4], h[5], pd) : run_r<float>(fi, fo, h[0], h[1], h[2], h[3], h[4], h[5], pd);
    fclose(fi);
    fclose(fo);
    return rc;
}
