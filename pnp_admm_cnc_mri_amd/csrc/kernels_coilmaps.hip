// Coil sensitivity maps from the calibration region of k-space for gfx950, float and double (coilmaps_plan.h): the local
// dominant-eigenvector method in matrix-free form.  Between k_calib_window and k_coil_eigmaps the caller runs the context's own inverse
// transform over the B C pseudo-slices.
//   k_calib_window      out[s][p] = w_H w_W y[s][p] on the ncal x ncal calibration region, +0 elsewhere: a thread owns 16 bytes of consecutive
//                       points (2 float, 1 double); points outside the region are never loaded, so the rows outside it are pure zero stores.
//                       The first workgroup of a slice's coil 0 also walks the region of the slice's mask and leaves the lowest offset of a
//                       point that is not sampled in miss[b] (-1: none): a minimum over the workgroup's threads, written by one of them.
//   k_coil_eigmaps      a workgroup owns a th x tw tile of one slice (one thread per pixel) and stages the tile plus its halo of r, wrapped,
//                       for all C coils in LDS as [pixel][coil] at a stride of an odd number of 16-byte slots; a thread keeps v and u (2 x CB
//                       complex, CB = 4, 8, 16, 32) in registers for all iterations and reads a patch point's coils as consecutive 16-byte
//                       slots.  16 (2r + 1)^2 C n flops per pixel; writes the unit vectors [B][C][H][W] and lambda [B][H][W].
//   k_maps_keymax       the maximum of the key (here lambda; ESPIRiT: inorm) per span of COILMAPS_SPAN pixels, by a tree over the workgroup
//   k_maps_support      the support stage of both estimators: every workgroup of a slice recomputes the slice's maximum from the spans'
//                       partials and zeroes the vectors of its span where key < frac * key_max or, with a gate array, gate < floor
// Vector stores only, no atomics; no sum depends on the batch, on the tile or on a pixel's place in it.
#include <atomic>
#include "internal.h"
#include "coilmaps_plan.h"

namespace pnp {

template <typename R, bool VEC>
__global__ __launch_bounds__(COILMAPS_WIN_THREADS) void k_calib_window(const typename CxOf<R>::type* __restrict__ y,
                                                                       const uint8_t* __restrict__ mask_bank,
                                                                       const int32_t* __restrict__ mask_id,
                                                                       typename CxOf<R>::type* __restrict__ out, int32_t* __restrict__ miss,
                                                                       int Cn, int H, int W, int ncal, CoilmapsWindow<R> win) {
    using C = typename CxOf<R>::type;
    constexpr int P = sizeof(R) == 8 ? 1 : 2;
    __shared__ int shmin[COILMAPS_WIN_THREADS];
    const int s = blockIdx.y;                            // pseudo-slice: coil s % Cn of slice s / Cn
    const size_t N = (size_t)H * W;
    const C* src = y + (size_t)s * N;
    C* dst = out + (size_t)s * N;
    const size_t p0 = ((size_t)blockIdx.x * COILMAPS_WIN_THREADS + threadIdx.x) * P;
    C k[P];
#pragma unroll
    for (int e = 0; e < P; ++e) {
        k[e].x = R(0); k[e].y = R(0);
        const size_t p = p0 + e;
        if (p >= N) continue;
        const int i = coilmaps_line_of((int)(p / W), ncal, H), j = coilmaps_line_of((int)(p % W), ncal, W);
        if (i < 0 || j < 0) continue;
        const C v = src[p];
        coilmaps_apply_window(win.w[i], win.w[j], v.x, v.y, k[e].x, k[e].y);
    }
    if constexpr (P == 2 && VEC) {                       // N even, 16-byte aligned: one store of two points
        if (p0 < N) {
            float4 t;
            t.x = k[0].x; t.y = k[0].y; t.z = k[1].x; t.w = k[1].y;
            *reinterpret_cast<float4*>(dst + p0) = t;
        }
    } else {
#pragma unroll
        for (int e = 0; e < P; ++e) if (p0 + e < N) dst[p0 + e] = k[e];
    }

    if (blockIdx.x != 0 || s % Cn != 0) return;          // the same for every thread of the workgroup
    const int b = s / Cn;
    const uint8_t* mask = mask_bank + (size_t)(mask_id ? mask_id[b] : 0) * N;
    int m = INT32_MAX;
    for (int q = threadIdx.x; q < coilmix_cal_points(ncal); q += COILMAPS_WIN_THREADS) {
        const int at = (int)coilmix_cal_index(q, ncal, H, W);
        if (!mask[at] && at < m) m = at;
    }
    shmin[threadIdx.x] = m;
    __syncthreads();
    for (int d = COILMAPS_WIN_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d && shmin[threadIdx.x + d] < shmin[threadIdx.x]) shmin[threadIdx.x] = shmin[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) miss[b] = shmin[0] == INT32_MAX ? -1 : shmin[0];
}

// the coils of one staged pixel, 16 bytes at a time
template <typename R> struct SlotOf;
template <> struct SlotOf<float>  { using type = float4; };
template <> struct SlotOf<double> { using type = double2; };

// f(c, re, im) for the coils c = 0 .. Cn - 1 of the staged pixel at `at`
template <typename R, int CB, typename F>
__device__ __forceinline__ void for_coils(const unsigned char* at, int Cn, F&& f) {
    using S = typename SlotOf<R>::type;
    const S* slot = reinterpret_cast<const S*>(at);
    if constexpr (sizeof(R) == 8) {
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            if (c < Cn) { const S t = slot[c]; f(c, t.x, t.y); }
        }
    } else {
#pragma unroll
        for (int c = 0; c < CB; c += 2) {
            if (c < Cn) {
                const S t = slot[c / 2];
                f(c, t.x, t.y);
                if (c + 1 < Cn) f(c + 1, t.z, t.w);
            }
        }
    }
}

template <typename R, int CB>
__global__ __launch_bounds__(256) void k_coil_eigmaps(const typename CxOf<R>::type* __restrict__ img,
                                                      typename CxOf<R>::type* __restrict__ maps, R* __restrict__ lambda, int Cn, int H, int W,
                                                      int r, int iters, int th, int tw) {
    using C = typename CxOf<R>::type;
    constexpr bool F64 = sizeof(R) == 8;
    constexpr int STRIDE = coilmaps_stride_slots(CB, F64) * 16;          // bytes per staged pixel
    extern __shared__ __attribute__((aligned(16))) unsigned char sh[];
    const int b = blockIdx.y;
    const int tiles_x = coilmaps_tiles_x(W, CoilmapsTile{th, tw});
    const int y0 = (int)(blockIdx.x / tiles_x) * th, x0 = (int)(blockIdx.x % tiles_x) * tw;
    const int PH = th + 2 * r, PW = tw + 2 * r, threads = th * tw;
    const size_t N = (size_t)H * W;
    const C* src = img + (size_t)b * Cn * N;
    for (int idx = threadIdx.x; idx < Cn * PH * PW; idx += threads) {
        const int c = idx / (PH * PW), pix = idx % (PH * PW);
        reinterpret_cast<C*>(sh + (size_t)pix * STRIDE)[c] = src[(size_t)c * N + coilmaps_staged_pixel(pix / PW, pix % PW, y0, x0, r, H, W)];
    }
    __syncthreads();

    const int ly = threadIdx.x / tw, lx = threadIdx.x % tw;
    const unsigned char* centre = sh + (size_t)((ly + r) * PW + lx + r) * STRIDE;
    R vr[CB], vi[CB], ur[CB], ui[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) { vr[c] = R(0); vi[c] = R(0); ur[c] = R(0); ui[c] = R(0); }

    // start: v = I(p) / ||I(p)||, or e_0
    R s = R(0);
    for_coils<R, CB>(centre, Cn, [&](int c, R ar, R ai) { coilmaps_norm2_step(s, ar, ai); });
    const R nrm = coilmaps_sqrt<R>(s);
    if (nrm > R(0)) for_coils<R, CB>(centre, Cn, [&](int c, R ar, R ai) { vr[c] = ar / nrm; vi[c] = ai / nrm; });
    else            vr[0] = R(1);

    R lam = R(0);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < CB; ++c) { ur[c] = R(0); ui[c] = R(0); }
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) {
                const unsigned char* at = centre + (dy * PW + dx) * STRIDE;
                R gr = R(0), gi = R(0);
                for_coils<R, CB>(at, Cn, [&](int c, R ar, R ai) { coilmaps_cmac_conj(gr, gi, ar, ai, vr[c], vi[c]); });
                for_coils<R, CB>(at, Cn, [&](int c, R ar, R ai) { coilmix_cmac(ur[c], ui[c], ar, ai, gr, gi); });
            }
        s = R(0);
#pragma unroll
        for (int c = 0; c < CB; ++c) if (c < Cn) coilmaps_norm2_step(s, ur[c], ui[c]);
        lam = coilmaps_sqrt<R>(s);
        if (lam > R(0)) {
#pragma unroll
            for (int c = 0; c < CB; ++c) if (c < Cn) { vr[c] = ur[c] / lam; vi[c] = ui[c] / lam; }
        }
    }

    // phase: v^H I(p) real and >= 0
    R gr = R(0), gi = R(0), er, ei;
    for_coils<R, CB>(centre, Cn, [&](int c, R ar, R ai) { coilmaps_cmac_conj(gr, gi, vr[c], vi[c], ar, ai); });
    if (coilmaps_phase_factor(gr, gi, er, ei)) {
#pragma unroll
        for (int c = 0; c < CB; ++c) if (c < Cn) coilmaps_rotate(vr[c], vi[c], er, ei);
    }

    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) return;                        // a remainder tile: the thread worked on wrapped pixels, it stores nothing
    const size_t p = (size_t)y * W + x;
    C* dst = maps + (size_t)b * Cn * N + p;
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < Cn) { C o; o.x = vr[c]; o.y = vi[c]; dst[(size_t)c * N] = o; }
    lambda[(size_t)b * N + p] = lam;
}

// the maximum of the workgroup's values by a tree over its COILMAPS_SUP_THREADS threads; every thread gets it
template <typename R> __device__ __forceinline__ R tree_max(R v, R* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = COILMAPS_SUP_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d && sh[threadIdx.x + d] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + d];
        __syncthreads();
    }
    return sh[0];
}

template <typename R>
__global__ __launch_bounds__(COILMAPS_SUP_THREADS) void k_maps_keymax(const R* __restrict__ key, R* __restrict__ part, size_t N) {
    __shared__ R sh[COILMAPS_SUP_THREADS];
    const size_t lo = (size_t)blockIdx.x * COILMAPS_SPAN;
    const size_t hi = lo + COILMAPS_SPAN < N ? lo + COILMAPS_SPAN : N;
    const R* l = key + (size_t)blockIdx.y * N;
    R m = R(0);                                           // the key is a norm: >= 0
    for (size_t p = lo + threadIdx.x; p < hi; p += COILMAPS_SUP_THREADS) if (l[p] > m) m = l[p];
    m = tree_max(m, sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
}

template <typename R>
__global__ __launch_bounds__(COILMAPS_SUP_THREADS) void k_maps_support(const R* __restrict__ gate, R floor, const R* __restrict__ key, R frac,
                                                                       const R* __restrict__ part, typename CxOf<R>::type* __restrict__ maps,
                                                                       int Cn, size_t N) {
    using C = typename CxOf<R>::type;
    __shared__ R sh[COILMAPS_SUP_THREADS];
    const int b = blockIdx.y, spans = gridDim.x;
    R m = R(0);
    for (int j = threadIdx.x; j < spans; j += COILMAPS_SUP_THREADS) if (part[(size_t)b * spans + j] > m) m = part[(size_t)b * spans + j];
    const R bar = frac * tree_max(m, sh);
    const size_t lo = (size_t)blockIdx.x * COILMAPS_SPAN;
    const size_t hi = lo + COILMAPS_SPAN < N ? lo + COILMAPS_SPAN : N;
    const R* l = key + (size_t)b * N;
    C zero;
    zero.x = R(0); zero.y = R(0);
    for (size_t p = lo + threadIdx.x; p < hi; p += COILMAPS_SUP_THREADS) {
        if ((!gate || gate[(size_t)b * N + p] >= floor) && l[p] >= bar) continue;
        for (int c = 0; c < Cn; ++c) maps[((size_t)b * Cn + c) * N + p] = zero;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the caller has checked coilmaps_check and that B C and B fit a grid dimension
template <typename R>
hipError_t launch_calib_window(hipStream_t s, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, R* out, int32_t* miss, int B,
                               int Cn, int H, int W, int ncal) {
    using C = typename CxOf<R>::type;
    const bool f64 = sizeof(R) == 8;
    const size_t N = (size_t)H * W;
    const dim3 grid((unsigned)coilmix_mix_blocks(N, f64), (unsigned)(B * Cn)), blk(COILMAPS_WIN_THREADS);
    const CoilmapsWindow<R> win = coilmaps_window_table<R>(ncal);
    // two points per 16-byte store need every pseudo-slice to start on a 16-byte boundary: N even and the array aligned
    const bool vec = !f64 && N % 2 == 0 && (uintptr_t)out % 16 == 0;
    if (vec) hipLaunchKernelGGL((k_calib_window<R, true>), grid, blk, 0, s, (const C*)y, mask_bank, mask_id, (C*)out, miss, Cn, H, W, ncal, win);
    else     hipLaunchKernelGGL((k_calib_window<R, false>), grid, blk, 0, s, (const C*)y, mask_bank, mask_id, (C*)out, miss, Cn, H, W, ncal, win);
    return hipGetLastError();
}

template <typename R, int CB>
static hipError_t eig_bucket(hipStream_t s, dim3 grid, CoilmapsTile t, size_t lds, const typename CxOf<R>::type* img,
                             typename CxOf<R>::type* maps, R* lambda, int Cn, int H, int W, int r, int iters) {
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_coil_eigmaps<R, CB>, done, lds, COILMAPS_LDS_HARD)) return e;
    hipLaunchKernelGGL((k_coil_eigmaps<R, CB>), grid, dim3((unsigned)(t.th * t.tw)), lds, s, img, maps, lambda, Cn, H, W, r, iters, t.th, t.tw);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_coil_eigmaps(hipStream_t s, const R* img, R* maps, R* lambda, int B, int Cn, int H, int W, int r, int iters) {
    using C = typename CxOf<R>::type;
    const bool f64 = sizeof(R) == 8;
    const int CB = coilmix_out_bucket(Cn);
    const CoilmapsTile t = coilmaps_tile_at(coilmaps_tile_choice(Cn, r, f64));
    const size_t lds = coilmaps_lds_bytes(t, r, CB, f64);
    if (lds > COILMAPS_LDS_HARD) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(coilmaps_tiles_y(H, t) * coilmaps_tiles_x(W, t)), (unsigned)B);
    switch (CB) {
    case 4:  return eig_bucket<R, 4>(s, grid, t, lds, (const C*)img, (C*)maps, lambda, Cn, H, W, r, iters);
    case 8:  return eig_bucket<R, 8>(s, grid, t, lds, (const C*)img, (C*)maps, lambda, Cn, H, W, r, iters);
    case 16: return eig_bucket<R, 16>(s, grid, t, lds, (const C*)img, (C*)maps, lambda, Cn, H, W, r, iters);
    default: return eig_bucket<R, 32>(s, grid, t, lds, (const C*)img, (C*)maps, lambda, Cn, H, W, r, iters);
    }
}

template <typename R>
hipError_t launch_maps_support(hipStream_t s, const R* gate, R floor, const R* key, R frac, R* part, R* maps, int B, int Cn, size_t N) {
    using C = typename CxOf<R>::type;
    const dim3 grid((unsigned)coilmaps_spans(N), (unsigned)B), blk(COILMAPS_SUP_THREADS);
    hipLaunchKernelGGL(k_maps_keymax<R>, grid, blk, 0, s, key, part, N);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_maps_support<R>, grid, blk, 0, s, gate, floor, key, frac, (const R*)part, (C*)maps, Cn, N);
    return hipGetLastError();
}

#define COILMAPS_INST(R)                                                                                                                  \
    template hipError_t launch_calib_window<R>(hipStream_t, const R*, const uint8_t*, const int32_t*, R*, int32_t*, int, int, int, int, int); \
    template hipError_t launch_coil_eigmaps<R>(hipStream_t, const R*, R*, R*, int, int, int, int, int, int);                             \
    template hipError_t launch_maps_support<R>(hipStream_t, const R*, R, const R*, R, R*, R*, int, int, size_t);
COILMAPS_INST(float)
COILMAPS_INST(double)
#undef COILMAPS_INST

}  // namespace pnp
