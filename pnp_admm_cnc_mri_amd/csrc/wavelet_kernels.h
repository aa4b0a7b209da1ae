// What the wavelet kernels of kernels_wavelet.hip (real values) and kernels_complex.hip (Cpx<S>, prox_ops.h) share, written once on the
// value type V: the launch arguments, the tile of a workgroup, the level loops with their barriers around wavelet_plan.h's item functions,
// and the launch with its LDS opt-in.  A unit adds its emitters (what happens to a coefficient or a pixel on its way out) and its kernels.
#pragma once
#include "internal.h"
#include "wavelet_plan.h"

namespace pnp {

// V: the value type of the images and coefficients; S: the scalar type of the thresholds (V itself for real values)
template <typename V, typename S = V>
struct WvArgs {
    const V* in0;      // fwd: image (NONE), x (L1, CNC);   inv: coefficients
    const V* in1;      // fwd: null (NONE), w
    const V* zin;      // fwd CNC: z
    V* out;            // fwd: coefficients;   inv NONE: image
    const V* x;        // inv with dual: x, w (read), z, w (written)
    V *z, *w;
    ProxParamsT<S> p;
    int H, W, L, tile, tiles_x, tiles_y;
    int sy, sx;        // the frame's shift
    V* acc;            // inv, averaging: the sum of the shifts' z+
    S rk;              // inv, last of K > 1 shifts: 1 / K
};

template <typename V, typename S> __device__ __forceinline__ WvTile wv_tile_of_block(const WvArgs<V, S>& a) {
    const int per = a.tiles_x * a.tiles_y, b = blockIdx.x / per, rem = blockIdx.x - b * per, ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
    return WvTile{a.H, a.W, a.L, a.tile, ty * a.tile, tx * a.tile, (size_t)b * a.H * a.W, a.sy, a.sx};
}

// analysis of one tile, all levels in LDS: emit(offset, value, detail) takes every coefficient that leaves
template <typename V, int T, typename Emit>
__device__ __forceinline__ void wv_fwd_image(const WvTile& t, const V* in0, const V* in1, V* rowbuf, V* ll, Emit emit) {
    for (int l = 0; l < t.L; ++l) {
        for (int it = threadIdx.x, n = wv_fwd_row_items(T, t, l); it < n; it += WV_THREADS) wv_fwd_row_item<V, T>(it, l, t, in0, in1, ll, rowbuf);
        __syncthreads();
        for (int it = threadIdx.x, n = wv_fwd_col_items(T, t, l); it < n; it += WV_THREADS) wv_fwd_col_item<V, T>(it, l, t, rowbuf, ll, emit);
        __syncthreads();
    }
}

// synthesis of one tile: make() gives the emitter, and emit(offset, value) takes every pixel.  The emitter is made per item, from the
// kernel's arguments, as the real kernels always did: hoisting it out of the loops changes their register allocation
template <typename V, int T, typename Make>
__device__ __forceinline__ void wv_inv_image(const WvTile& t, int L, const V* coef, V* colbuf, V* ll, Make make) {
    for (int l = L - 1; l >= 0; --l) {
        for (int it = threadIdx.x, n = wv_inv_col_items(T, t, l); it < n; it += WV_THREADS) wv_inv_col_item<V, T>(it, l, t, coef, ll, colbuf);
        __syncthreads();
        for (int it = threadIdx.x, n = wv_inv_row_items(T, t, l); it < n; it += WV_THREADS) wv_inv_row_item<V, T>(it, l, t, colbuf, ll, make());
        __syncthreads();
    }
}

template <typename K, typename A> hipError_t wv_launch(K kernel, hipStream_t s, int blocks, size_t lds, std::atomic<bool>* done, const A& a) {
    if (lds > WV_LDS_MAX) return hipErrorInvalidValue;
    if (hipError_t e = lds_opt_in((const void*)kernel, done, lds, WV_LDS_MAX)) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(WV_THREADS), lds, s, a);
    return hipGetLastError();
}

template <typename V, typename S = V> WvArgs<V, S> wv_args(int wavelet, int levels, int H, int W) {
    WvArgs<V, S> a{};
    const int T = wv_taps(wavelet);
    a.H = H; a.W = W; a.L = levels; a.tile = wv_tile(T, levels);
    a.tiles_x = wv_tiles(W, a.tile); a.tiles_y = wv_tiles(H, a.tile);
    return a;
}

}  // namespace pnp
