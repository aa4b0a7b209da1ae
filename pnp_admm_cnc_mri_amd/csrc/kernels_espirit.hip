// ESPIRiT coil sensitivity maps for gfx950, float and double (espirit_plan.h).  Between the two kernels the caller runs the host stage
// (espirit_kernels) on the Gram matrices; the low-resolution images come from k_calib_window and the context's inverse transform.
//   k_calib_patch_gram  one workgroup per (slice, 16 x 16 tile of the upper triangle of the n x n Gram matrix, n = C k^2), one thread per
//                       pair (m, m').  The rows of the calibration block K that a chunk of patch-position rows reads are staged in LDS as
//                       complex double for the coils the tile's 16 rows and 16 columns touch (espirit_tile_coils, espirit_stage_rows);
//                       every thread runs ONE chain of coilmix_gram_step over all positions in row-major order, so the chunking is
//                       invisible in the result.  Both triangles are written.
//   k_espirit_maps      a workgroup owns a th x tw tile of one slice, one thread per pixel.  LDS (espirit_lds): the packed upper triangle of
//                       the slice's w, read at one address by the whole wave (a broadcast); the tile's rows of E_H and columns of E_W; a
//                       slab of CB complex values per thread for v at an odd slot stride.  G(q) is applied entry by entry and never
//                       stored: row c of u = G v sits in a register pair while c' runs over the slab, the rows are unrolled (u [CB] in
//                       registers, static indices: no scratch in any instance).  The phase rule is fused; writes the unit vectors
//                       [B][C][H][W], lambda [B][H][W] and ||I|| [B][H][W].
// The support (lambda < crop or ||I|| < tau * max zeroed) is kernels_coilmaps.hip's k_maps_keymax / k_maps_support, gated on lambda.
// Vector stores only, no atomics; no sum depends on the batch, on the tile or on a pixel's place in it.
#include <atomic>
#include "internal.h"
#include "espirit_plan.h"

namespace pnp {

template <typename R>
__global__ __launch_bounds__(ESPIRIT_TILE * ESPIRIT_TILE) void k_calib_patch_gram(const typename CxOf<R>::type* __restrict__ y,
                                                                                  const uint8_t* __restrict__ mask_bank,
                                                                                  const int32_t* __restrict__ mask_id,
                                                                                  double2* __restrict__ gram, int Cn, int H, int W, int ncal, int k) {
    using C = typename CxOf<R>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_raw[];
    double2* sh = reinterpret_cast<double2*>(sh_raw);
    constexpr int T = ESPIRIT_TILE, THREADS = T * T;
    const int b = blockIdx.y, n = espirit_columns(Cn, k), P = espirit_positions(ncal, k);
    int bi, bj;
    coilmix_tile_of((int)blockIdx.x, n, bi, bj);
    int ca0, na, cb0, nb;
    espirit_tile_coils(bi, n, k, ca0, na);
    espirit_tile_coils(bj, n, k, cb0, nb);
    const int RS = espirit_stage_rows(ncal, na + nb);          // staged rows per coil; >= k
    const int RI = RS - (k - 1);                                // position rows per chunk; >= 1
    const size_t N = (size_t)H * W;
    const C* src = y + (size_t)b * Cn * N;
    const uint8_t* mask = mask_bank ? mask_bank + (size_t)(mask_id ? mask_id[b] : 0) * N : nullptr;

    const int m = bi * T + (int)threadIdx.x / T, m2 = bj * T + (int)threadIdx.x % T;
    const bool active = m < n && m2 < n && m <= m2;
    int cm = 0, am = 0, bm = 0, cn = 0, an = 0, bn = 0;
    if (active) {
        espirit_column(m, k, cm, am, bm);
        espirit_column(m2, k, cn, an, bn);
    }
    const int sm = cm - ca0, sn = na + cn - cb0;               // the staged slots of the two coils
    double re = 0.0, im = 0.0;
    for (int i0 = 0; i0 < P; i0 += RI) {
        const int ri = P - i0 < RI ? P - i0 : RI, rows = ri + k - 1;
        __syncthreads();                                        // the previous chunk has been read
        for (int idx = threadIdx.x; idx < (na + nb) * rows * ncal; idx += THREADS) {
            const int s = idx / (rows * ncal), r = idx / ncal % rows, u = idx % ncal;
            const int coil = s < na ? ca0 + s : cb0 + (s - na);
            const size_t at = espirit_block_index(i0 + r, u, ncal, H, W);
            double2 v;
            v.x = 0.0; v.y = 0.0;
            if (!mask || mask[at]) { const C t = src[(size_t)coil * N + at]; v.x = (double)t.x; v.y = (double)t.y; }
            sh[((size_t)s * RS + r) * ncal + u] = v;
        }
        __syncthreads();
        if (active)
            for (int i = 0; i < ri; ++i) {
                const double2* pa = sh + ((size_t)sm * RS + i + am) * ncal + bm;
                const double2* pb = sh + ((size_t)sn * RS + i + an) * ncal + bn;
                for (int j = 0; j < P; ++j) coilmix_gram_step(re, im, pb[j].x, pb[j].y, pa[j].x, pa[j].y);
            }
    }
    if (!active) return;
    double2* g = gram + (size_t)b * n * n;
    double2 o;
    o.x = re; o.y = m == m2 ? 0.0 : im;
    g[(size_t)m * n + m2] = o;
    if (m != m2) { o.y = -im; g[(size_t)m2 * n + m] = o; }
}

template <typename R, int CB>
__global__ __launch_bounds__(256) void k_espirit_maps(const typename CxOf<R>::type* __restrict__ img, const typename CxOf<R>::type* __restrict__ w,
                                                      const typename CxOf<R>::type* __restrict__ eh_tab,
                                                      const typename CxOf<R>::type* __restrict__ ew_tab,
                                                      typename CxOf<R>::type* __restrict__ maps, R* __restrict__ lambda, R* __restrict__ inorm,
                                                      int Cn, int H, int W, int k, int iters, int th, int tw) {
    using C = typename CxOf<R>::type;
    constexpr bool F64 = sizeof(R) == 8;
    constexpr int STRIDE = coilmaps_stride_slots(CB, F64) * 16;          // bytes per thread's slab
    extern __shared__ __attribute__((aligned(16))) unsigned char sh[];
    const EspiritLds lay = espirit_lds(CoilmapsTile{th, tw}, Cn, k, F64);
    C* wl = reinterpret_cast<C*>(sh + lay.w);
    C* ehl = reinterpret_cast<C*>(sh + lay.eh);
    C* ewl = reinterpret_cast<C*>(sh + lay.ew);
    const int b = blockIdx.y, D = espirit_side(k), DD = D * D, threads = th * tw;
    const int tiles_x = coilmaps_tiles_x(W, CoilmapsTile{th, tw});
    const int y0 = (int)(blockIdx.x / tiles_x) * th, x0 = (int)(blockIdx.x % tiles_x) * tw;
    const size_t N = (size_t)H * W;

    const C* wsrc = w + (size_t)b * Cn * Cn * DD;
    for (int idx = threadIdx.x; idx < Cn * Cn * DD; idx += threads) {
        const int c = idx / (Cn * DD), c2 = idx / DD % Cn;
        if (c <= c2) wl[espirit_pair(c, c2, Cn) * DD + idx % DD] = wsrc[idx];
    }
    for (int idx = threadIdx.x; idx < th * D; idx += threads) {          // a remainder tile repeats the last row / column: never stored
        const int yy = y0 + idx / D < H ? y0 + idx / D : H - 1;
        ehl[idx] = eh_tab[(size_t)yy * D + idx % D];
    }
    for (int idx = threadIdx.x; idx < D * tw; idx += threads) {
        const int xx = x0 + idx % tw < W ? x0 + idx % tw : W - 1;
        ewl[idx] = ew_tab[(size_t)xx * D + idx / tw];
    }
    __syncthreads();

    const int ly = threadIdx.x / tw, lx = threadIdx.x % tw;
    const int y = y0 + ly < H ? y0 + ly : H - 1, x = x0 + lx < W ? x0 + lx : W - 1;
    const size_t p = (size_t)y * W + x;
    const C* src = img + (size_t)b * Cn * N + p;
    C* vs = reinterpret_cast<C*>(sh + lay.slab + (size_t)threadIdx.x * STRIDE);          // this thread's v
    const C* eh = ehl + ly * D;
    const C* ew = ewl + lx;

    // start: v = I(q) / ||I(q)||, or e_0
    R s = R(0);
    for (int c = 0; c < Cn; ++c) { const C t = src[(size_t)c * N]; coilmaps_norm2_step(s, t.x, t.y); }
    const R nrm = coilmaps_sqrt<R>(s);
    for (int c = 0; c < Cn; ++c) {
        C t;
        if (nrm > R(0)) { const C a = src[(size_t)c * N]; t.x = a.x / nrm; t.y = a.y / nrm; }
        else            { t.x = c == 0 ? R(1) : R(0); t.y = R(0); }
        vs[c] = t;
    }

    R lam = R(0);
    R ur[CB], ui[CB];
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            ur[c] = R(0); ui[c] = R(0);
            if (c < Cn) {
                R ar = R(0), ai = R(0);
                for (int c2 = 0; c2 < Cn; ++c2) {
                    const C* wp = wl + espirit_pair(c < c2 ? c : c2, c < c2 ? c2 : c, Cn) * DD;
                    R gr = R(0), gi = R(0);
                    for (int dy = 0; dy < D; ++dy) {
                        R ir = R(0), ii = R(0);
                        for (int dx = 0; dx < D; ++dx) {
                            const C wv = wp[dy * D + dx], e = ew[dx * tw];
                            coilmix_cmac(ir, ii, wv.x, wv.y, e.x, e.y);
                        }
                        const C e = eh[dy];
                        coilmix_cmac(gr, gi, e.x, e.y, ir, ii);
                    }
                    espirit_g_place(c, c2, gr, gi);
                    const C v = vs[c2];
                    coilmix_cmac(ar, ai, gr, gi, v.x, v.y);
                }
                ur[c] = ar; ui[c] = ai;
            }
        }
        s = R(0);
#pragma unroll
        for (int c = 0; c < CB; ++c) if (c < Cn) coilmaps_norm2_step(s, ur[c], ui[c]);
        lam = coilmaps_sqrt<R>(s);
        if (lam > R(0)) {
#pragma unroll
            for (int c = 0; c < CB; ++c) if (c < Cn) { C t; t.x = ur[c] / lam; t.y = ui[c] / lam; vs[c] = t; }
        }
    }

    // phase: v^H I(q) real and >= 0
    R gr = R(0), gi = R(0), er = R(1), ei = R(0);
    for (int c = 0; c < Cn; ++c) { const C v = vs[c], a = src[(size_t)c * N]; coilmaps_cmac_conj(gr, gi, v.x, v.y, a.x, a.y); }
    const bool turn = coilmaps_phase_factor(gr, gi, er, ei);

    if (y0 + ly >= H || x0 + lx >= W) return;            // a remainder tile: the thread worked on a repeated pixel, it stores nothing
    C* dst = maps + (size_t)b * Cn * N + p;
    for (int c = 0; c < Cn; ++c) {
        C v = vs[c];
        if (turn) coilmaps_rotate(v.x, v.y, er, ei);
        dst[(size_t)c * N] = v;
    }
    lambda[(size_t)b * N + p] = lam;
    inorm[(size_t)b * N + p] = nrm;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the caller has checked espirit_check and that B fits a grid dimension
template <typename R>
hipError_t launch_calib_patch_gram(hipStream_t s, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int Cn,
                                   int H, int W, int ncal, int k) {
    using C = typename CxOf<R>::type;
    const dim3 grid((unsigned)coilmix_tile_pairs(espirit_columns(Cn, k)), (unsigned)B), blk(ESPIRIT_TILE * ESPIRIT_TILE);
    hipLaunchKernelGGL(k_calib_patch_gram<R>, grid, blk, ESPIRIT_GRAM_LDS, s, (const C*)y, mask_bank, mask_id, (double2*)gram, Cn, H, W, ncal, k);
    return hipGetLastError();
}

template <typename R, int CB>
static hipError_t espirit_bucket(hipStream_t s, dim3 grid, CoilmapsTile t, size_t lds, const typename CxOf<R>::type* img,
                                 const typename CxOf<R>::type* w, const typename CxOf<R>::type* eh, const typename CxOf<R>::type* ew,
                                 typename CxOf<R>::type* maps, R* lambda, R* inorm, int Cn, int H, int W, int k, int iters) {
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_espirit_maps<R, CB>, done, lds, COILMAPS_LDS_HARD)) return e;
    hipLaunchKernelGGL((k_espirit_maps<R, CB>), grid, dim3((unsigned)(t.th * t.tw)), lds, s, img, w, eh, ew, maps, lambda, inorm, Cn, H, W, k, iters,
                       t.th, t.tw);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_espirit_maps(hipStream_t s, const R* img, const R* w, const R* eh, const R* ew, R* maps, R* lambda, R* inorm, int B, int Cn,
                               int H, int W, int k, int iters) {
    using C = typename CxOf<R>::type;
    const bool f64 = sizeof(R) == 8;
    const CoilmapsTile t = coilmaps_tile_at(espirit_tile_choice(Cn, k, f64));
    const size_t lds = espirit_lds(t, Cn, k, f64).bytes;
    if (lds > COILMAPS_LDS_HARD) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(coilmaps_tiles_y(H, t) * coilmaps_tiles_x(W, t)), (unsigned)B);
#define ESPIRIT_CASE(CB) return espirit_bucket<R, CB>(s, grid, t, lds, (const C*)img, (const C*)w, (const C*)eh, (const C*)ew, (C*)maps, lambda, \
                                                      inorm, Cn, H, W, k, iters)
    switch (coilmix_out_bucket(Cn)) {
    case 4:  ESPIRIT_CASE(4);
    case 8:  ESPIRIT_CASE(8);
    case 16: ESPIRIT_CASE(16);
    default: ESPIRIT_CASE(32);
    }
#undef ESPIRIT_CASE
}

#define ESPIRIT_INST(R)                                                                                                                     \
    template hipError_t launch_calib_patch_gram<R>(hipStream_t, const R*, const uint8_t*, const int32_t*, double*, int, int, int, int, int, int); \
    template hipError_t launch_espirit_maps<R>(hipStream_t, const R*, const R*, const R*, const R*, R*, R*, R*, int, int, int, int, int, int);
ESPIRIT_INST(float)
ESPIRIT_INST(double)
#undef ESPIRIT_INST

}  // namespace pnp
