// Wavelet-domain sparsity: Psi = orthonormal periodic 2-D DWT (wavelet_plan.h), prox of thr ||Psi z||_1 = Psi^T soft(Psi v, thr) in closed
// form, and the CNC pair of thresholds coefficient-wise.  Two launches per prox, both tiled through LDS:
//   k_wv_fwd  analysis + threshold: a workgroup stages nothing but what a level hands to the next -- level 0's row pass reads the image
//             (x + w formed on the way in) with periodic wrap, all L levels run in LDS, the coefficients leave thresholded, in Mallat
//             layout, for the context's scratch.  CNC: z goes through first and its raw coefficients wait in the scratch; x + w follows
//             through the same LDS, and the thread that wrote a coefficient of z combines it with that of x + w (same item -> same thread).
//   k_wv_inv  synthesis + dual: reads the coefficient tile with its left / top halo, undoes all levels in LDS, writes z+ and
//             w+ = (x + w) - z+ in place.
// Cycle spinning (wavelet_plan.h): both kernels take the frame's shift (sy, sx) and apply it where they touch the image, nowhere else.  A
// prox that averages K > 1 shifts is the two launches per shift; the synthesis of shift 0 stores its z+ into an accumulator, those of
// shifts 1 .. K - 2 add theirs, the last one forms z+ = (acc + z_(K-1)) (1 / K) and w+ -- so z and w keep the old state for every analysis.
// The work of every pass is wavelet_plan.h's item functions, one item per thread and step; tests/host/wavelet_emulation.cpp runs the
// same functions on the host.  -ffp-contract=off (Makefile); products are chained by explicit fma.
#include "internal.h"
#include "prox_ops.h"
#include "wavelet_plan.h"
#include "wavelet_kernels.h"

namespace pnp {

namespace {

// what happens to a coefficient on its way out
template <typename R> struct EmitStore {            // Psi alone; CNC: the raw coefficients of z
    R* c;
    __device__ void operator()(size_t o, R v, bool) const { c[o] = v; }
};
template <typename R> struct EmitL1 {
    R* c; R thr;
    __device__ void operator()(size_t o, R v, bool detail) const { c[o] = detail ? soft(v, thr) : v; }
};
template <typename R> struct EmitCnc {              // v = coefficient of x + w; c[o] = that of z, written by this thread
    R* c; ProxParamsT<R> p;
    __device__ void operator()(size_t o, R v, bool detail) const {
        const R cz = c[o];
        if (detail) {
            const R clipz = cz < -p.ib ? -p.ib : (cz > p.ib ? p.ib : cz);
            c[o] = soft(fma_r(p.c1, cz, fma_r(p.c2, v, p.c3 * clipz)), p.thr);
        } else {
            c[o] = fma_r(p.c1, cz, p.c2 * v);
        }
    }
};

// PROX: 0 none, 1 L1, 2 CNC
template <typename R, int PROX, int T>
__global__ __launch_bounds__(WV_THREADS) void k_wv_fwd(const WvArgs<R> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wv_smem[];
    const WvTile t = wv_tile_of_block(a);
    R* rowbuf = (R*)wv_smem;
    R* ll = rowbuf + wv_fwd_rowbuf_elems(T, a.L, a.tile);
    if constexpr (PROX == 0) wv_fwd_image<R, T>(t, a.in0, a.in1, rowbuf, ll, EmitStore<R>{a.out});
    if constexpr (PROX == 1) wv_fwd_image<R, T>(t, a.in0, a.in1, rowbuf, ll, EmitL1<R>{a.out, a.p.thr});
    if constexpr (PROX == 2) {
        wv_fwd_image<R, T>(t, a.zin, (const R*)nullptr, rowbuf, ll, EmitStore<R>{a.out});
        wv_fwd_image<R, T>(t, a.in0, a.in1, rowbuf, ll, EmitCnc<R>{a.out, a.p});
    }
}

template <typename R> struct EmitImage {
    R* o;
    __device__ void operator()(size_t i, R v) const { o[i] = v; }
};
template <typename R> struct EmitDual {             // z+ = v, w+ = (x + w) - z+
    const R* x; R *z, *w;
    __device__ void operator()(size_t i, R v) const {
        const R u = x[i] + w[i];
        z[i] = v;
        w[i] = u - v;
    }
};

// averaging K > 1 shifts: the first, the middle ones, the last
template <typename R> struct EmitAccStore {
    R* acc;
    __device__ void operator()(size_t i, R v) const { acc[i] = v; }
};
template <typename R> struct EmitAccAdd {
    R* acc;
    __device__ void operator()(size_t i, R v) const { acc[i] = acc[i] + v; }
};
template <typename R> struct EmitAvgDual {          // z+ = (acc + v) (1 / K), w+ = (x + w) - z+
    const R* x; const R* acc; R *z, *w; R rk;
    __device__ void operator()(size_t i, R v) const {
        const R u = x[i] + w[i];
        const R zn = (acc[i] + v) * rk;
        z[i] = zn;
        w[i] = u - zn;
    }
};

// what the synthesis does with a pixel
enum { WV_OUT_IMAGE = 0, WV_OUT_DUAL = 1, WV_OUT_ACC_STORE = 2, WV_OUT_ACC_ADD = 3, WV_OUT_AVG_DUAL = 4 };

template <typename R, int OUT, int T>
__global__ __launch_bounds__(WV_THREADS) void k_wv_inv(const WvArgs<R> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wv_smem[];
    const WvTile t = wv_tile_of_block(a);
    R* colbuf = (R*)wv_smem;
    R* ll = colbuf + wv_inv_colbuf_elems(T, a.tile);
    if constexpr (OUT == WV_OUT_IMAGE) wv_inv_image<R, T>(t, a.L, a.in0, colbuf, ll, [&] { return EmitImage<R>{a.out}; });
    if constexpr (OUT == WV_OUT_DUAL) wv_inv_image<R, T>(t, a.L, a.in0, colbuf, ll, [&] { return EmitDual<R>{a.x, a.z, a.w}; });
    if constexpr (OUT == WV_OUT_ACC_STORE) wv_inv_image<R, T>(t, a.L, a.in0, colbuf, ll, [&] { return EmitAccStore<R>{a.acc}; });
    if constexpr (OUT == WV_OUT_ACC_ADD) wv_inv_image<R, T>(t, a.L, a.in0, colbuf, ll, [&] { return EmitAccAdd<R>{a.acc}; });
    if constexpr (OUT == WV_OUT_AVG_DUAL) wv_inv_image<R, T>(t, a.L, a.in0, colbuf, ll, [&] { return EmitAvgDual<R>{a.x, a.acc, a.z, a.w, a.rk}; });
}

template <typename R, int PROX, int T> hipError_t wv_fwd_t(hipStream_t s, const WvArgs<R>& a, int B) {
    static std::atomic<bool> done[64] = {};
    return wv_launch(k_wv_fwd<R, PROX, T>, s, B * a.tiles_x * a.tiles_y, wv_fwd_lds_elems(T, a.L, a.tile) * sizeof(R), done, a);
}
template <typename R, int OUT, int T> hipError_t wv_inv_t(hipStream_t s, const WvArgs<R>& a, int B) {
    static std::atomic<bool> done[64] = {};
    return wv_launch(k_wv_inv<R, OUT, T>, s, B * a.tiles_x * a.tiles_y, wv_inv_lds_elems(T, a.tile) * sizeof(R), done, a);
}

template <typename R, int PROX> hipError_t wv_fwd_p(hipStream_t s, int wavelet, const WvArgs<R>& a, int B) {
    switch (wavelet) {
    case WV_HAAR: return wv_fwd_t<R, PROX, 2>(s, a, B);
    case WV_DB2:  return wv_fwd_t<R, PROX, 4>(s, a, B);
    case WV_DB4:  return wv_fwd_t<R, PROX, 8>(s, a, B);
    }
    return hipErrorInvalidValue;
}
template <typename R, int OUT> hipError_t wv_inv_p(hipStream_t s, int wavelet, const WvArgs<R>& a, int B) {
    switch (wavelet) {
    case WV_HAAR: return wv_inv_t<R, OUT, 2>(s, a, B);
    case WV_DB2:  return wv_inv_t<R, OUT, 4>(s, a, B);
    case WV_DB4:  return wv_inv_t<R, OUT, 8>(s, a, B);
    }
    return hipErrorInvalidValue;
}

}  // namespace

template <typename R>
hipError_t launch_dwt2(hipStream_t s, int wavelet, int levels, bool inv, const R* in, R* out, int B, int H, int W, int sy, int sx) {
    if (wv_check(wavelet, levels, H, W) != WV_OK || B < 1 || !wv_shift_ok(levels, sy, sx)) return hipErrorInvalidValue;
    WvArgs<R> a = wv_args<R>(wavelet, levels, H, W);
    a.in0 = in; a.out = out; a.sy = sy; a.sx = sx;
    return inv ? wv_inv_p<R, WV_OUT_IMAGE>(s, wavelet, a, B) : wv_fwd_p<R, 0>(s, wavelet, a, B);
}

template <typename R>
hipError_t launch_wavelet_prox(hipStream_t s, int wavelet, int levels, bool cnc, const R* x, R* z, R* w, R* coef, const ProxParamsT<R>& p,
                               int B, int H, int W, const int* shifts, int K, R* acc) {
    if (wv_check(wavelet, levels, H, W) != WV_OK || B < 1 || K < 1 || K > WV_SPIN_MAX_K || (K > 1 && (!shifts || !acc))) return hipErrorInvalidValue;
    for (int j = 0; shifts && j < K; ++j) if (!wv_shift_ok(levels, shifts[2 * j], shifts[2 * j + 1])) return hipErrorInvalidValue;
    for (int j = 0; j < K; ++j) {
        WvArgs<R> a = wv_args<R>(wavelet, levels, H, W);
        if (shifts) { a.sy = shifts[2 * j]; a.sx = shifts[2 * j + 1]; }
        a.in0 = x; a.in1 = w; a.zin = z; a.out = coef; a.p = p;
        hipError_t e = cnc ? wv_fwd_p<R, 2>(s, wavelet, a, B) : wv_fwd_p<R, 1>(s, wavelet, a, B);
        if (e != hipSuccess) return e;
        a.in0 = coef; a.in1 = nullptr; a.zin = nullptr; a.out = nullptr; a.x = x; a.z = z; a.w = w; a.acc = acc; a.rk = (R)(1.0 / K);
        if (K == 1) e = wv_inv_p<R, WV_OUT_DUAL>(s, wavelet, a, B);
        else if (j == K - 1) e = wv_inv_p<R, WV_OUT_AVG_DUAL>(s, wavelet, a, B);
        else e = j == 0 ? wv_inv_p<R, WV_OUT_ACC_STORE>(s, wavelet, a, B) : wv_inv_p<R, WV_OUT_ACC_ADD>(s, wavelet, a, B);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template hipError_t launch_dwt2<float>(hipStream_t, int, int, bool, const float*, float*, int, int, int, int, int);
template hipError_t launch_dwt2<double>(hipStream_t, int, int, bool, const double*, double*, int, int, int, int, int);
template hipError_t launch_wavelet_prox<float>(hipStream_t, int, int, bool, const float*, float*, float*, float*, const ProxParamsT<float>&, int, int, int,
                                               const int*, int, float*);
template hipError_t launch_wavelet_prox<double>(hipStream_t, int, int, bool, const double*, double*, double*, double*, const ProxParamsT<double>&, int, int,
                                                int, const int*, int, double*);

}  // namespace pnp
