// Complex-valued images on a coil context (pnp_set_image; include/pnp_mri.h, "complex-valued images"): the z / w step on a complex
// state, float and double.  The x-step's complex ends are the CX roles of kernels_coils.hip; here are
//   k_prox_cx   the pixel prox: z+ = csoft(u, thr) (L1) or csoft(c1 z + c2 u + c3 cclip(z, ib), thr) (CNC), w+ = u - z+, u = x + w.
//               A thread moves 16 bytes per access -- two complex floats or one complex double -- and the thread behind the last pair
//               takes the odd element of a float array
//   k_wvc_fwd / k_wvc_inv   the fused wavelet prox of kernels_wavelet.hip on a complex value type (the level loops and the launch are
//               wavelet_kernels.h's, shared with that unit; only the emitters differ): Psi is real-linear, so wavelet_plan.h's
//               item functions are instantiated on Cpx<S> (prox_ops.h), a tap is one fma per component, and the thread that emits a
//               coefficient holds both components: the modulus of csoft needs no second pass.  Two launches per prox, all levels in LDS,
//               twice the bytes of the real kernels per tile; the tile is wv_tile's, and a setting whose tile does not fit WV_LDS_MAX
//               (db4 with 4 levels in double: 274 KiB) is refused by wavelet_cx_fits before anything is launched.  No spin.
// -ffp-contract=off (Makefile); products are chained by explicit fma.  Vector stores only, no atomics.
#include "internal.h"
#include "prox_ops.h"
#include "wavelet_plan.h"
#include "wavelet_kernels.h"

namespace pnp {

namespace {

template <typename S, bool CNC> __device__ __forceinline__ void prox_step_cx(Cpx<S> x, Cpx<S>& z, Cpx<S>& w, const ProxParamsT<S>& p) {
    if constexpr (CNC) prox_cnc_cx(x, z, w, p); else prox_l1_cx(x, z, w, p);
}

template <typename S> struct alignas(16) CpxVec {
    static constexpr int V = 16 / (int)sizeof(Cpx<S>);       // 2 (float) | 1 (double)
    Cpx<S> v[V];
};

// n complex elements; nv = n / V full 16-byte accesses.  Grid: one thread per access and one more for the tail.
template <typename S, bool CNC>
__global__ __launch_bounds__(256) void k_prox_cx(const Cpx<S>* x, Cpx<S>* z, Cpx<S>* w, ProxParamsT<S> p, size_t n) {
    using Vec = CpxVec<S>;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, nv = n / Vec::V;
    if (i < nv) {
        const Vec xv = ((const Vec*)x)[i];
        Vec zv, wv = ((const Vec*)w)[i];
        if constexpr (CNC) zv = ((const Vec*)z)[i];          // L1 does not read z
#pragma unroll
        for (int k = 0; k < Vec::V; ++k) prox_step_cx<S, CNC>(xv.v[k], zv.v[k], wv.v[k], p);
        ((Vec*)z)[i] = zv;
        ((Vec*)w)[i] = wv;
    } else if (i == nv && nv * Vec::V < n) {                  // the odd element of a float array
        const size_t e = nv * Vec::V;
        Cpx<S> zv = z[e], wv = w[e];
        prox_step_cx<S, CNC>(x[e], zv, wv, p);
        z[e] = zv;
        w[e] = wv;
    }
}

// ---- the fused wavelet prox on Cpx<S>: wavelet_kernels.h's arguments, level loops and launch; here the emitters and the kernels ------
template <typename S> using WvcArgs = WvArgs<Cpx<S>, S>;

template <typename S> struct EmitStoreC {           // CNC: the raw coefficients of z
    Cpx<S>* c;
    __device__ void operator()(size_t o, Cpx<S> v, bool) const { c[o] = v; }
};
template <typename S> struct EmitL1C {
    Cpx<S>* c; S thr;
    __device__ void operator()(size_t o, Cpx<S> v, bool detail) const { c[o] = detail ? csoft(v, thr) : v; }
};
template <typename S> struct EmitCncC {             // v = coefficient of x + w; c[o] = that of z, written by this thread
    Cpx<S>* c; ProxParamsT<S> p;
    __device__ void operator()(size_t o, Cpx<S> v, bool detail) const {
        const Cpx<S> cz = c[o];
        if (detail) c[o] = csoft(cnc_combine_cx(cz, v, p), p.thr);
        else        c[o] = Cpx<S>(cpx_fma(p.c1, cz.re, p.c2 * v.re), cpx_fma(p.c1, cz.im, p.c2 * v.im));
    }
};
template <typename S> struct EmitDualC {            // z+ = v, w+ = (x + w) - z+
    const Cpx<S>* x; Cpx<S> *z, *w;
    __device__ void operator()(size_t i, Cpx<S> v) const {
        const Cpx<S> u = x[i] + w[i];
        z[i] = v;
        w[i] = u - v;
    }
};

template <typename S, bool CNC, int T>
__global__ __launch_bounds__(WV_THREADS) void k_wvc_fwd(const WvcArgs<S> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wvc_smem[];
    const WvTile t = wv_tile_of_block(a);
    Cpx<S>* rowbuf = (Cpx<S>*)wvc_smem;
    Cpx<S>* ll = rowbuf + wv_fwd_rowbuf_elems(T, a.L, a.tile);
    if constexpr (CNC) {
        wv_fwd_image<Cpx<S>, T>(t, a.zin, (const Cpx<S>*)nullptr, rowbuf, ll, EmitStoreC<S>{a.out});
        wv_fwd_image<Cpx<S>, T>(t, a.in0, a.in1, rowbuf, ll, EmitCncC<S>{a.out, a.p});
    } else {
        wv_fwd_image<Cpx<S>, T>(t, a.in0, a.in1, rowbuf, ll, EmitL1C<S>{a.out, a.p.thr});
    }
}

template <typename S, int T>
__global__ __launch_bounds__(WV_THREADS) void k_wvc_inv(const WvcArgs<S> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wvc_smem[];
    const WvTile t = wv_tile_of_block(a);
    Cpx<S>* colbuf = (Cpx<S>*)wvc_smem;
    Cpx<S>* ll = colbuf + wv_inv_colbuf_elems(T, a.tile);
    wv_inv_image<Cpx<S>, T>(t, a.L, a.in0, colbuf, ll, [&] { return EmitDualC<S>{a.x, a.z, a.w}; });
}

template <typename S, bool CNC, int T> hipError_t wvc_fwd_t(hipStream_t s, const WvcArgs<S>& a, int B) {
    static std::atomic<bool> done[64] = {};
    return wv_launch(k_wvc_fwd<S, CNC, T>, s, B * a.tiles_x * a.tiles_y, wv_fwd_lds_elems(T, a.L, a.tile) * sizeof(Cpx<S>), done, a);
}
template <typename S, int T> hipError_t wvc_inv_t(hipStream_t s, const WvcArgs<S>& a, int B) {
    static std::atomic<bool> done[64] = {};
    return wv_launch(k_wvc_inv<S, T>, s, B * a.tiles_x * a.tiles_y, wv_inv_lds_elems(T, a.tile) * sizeof(Cpx<S>), done, a);
}

template <typename S, int T> hipError_t wvc_prox_t(hipStream_t s, bool cnc, WvcArgs<S> a, int B) {
    hipError_t e = cnc ? wvc_fwd_t<S, true, T>(s, a, B) : wvc_fwd_t<S, false, T>(s, a, B);
    if (e != hipSuccess) return e;
    a.in0 = a.out; a.in1 = nullptr; a.zin = nullptr; a.out = nullptr;
    return wvc_inv_t<S, T>(s, a, B);
}

unsigned cx_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// LDS bytes of the two complex wavelet kernels at wv_tile's tile: the larger must fit WV_LDS_MAX
bool wavelet_cx_fits(int wavelet, int levels, bool f64) {
    const int T = wv_taps(wavelet), tile = wv_tile(T, levels);
    const size_t elem = f64 ? sizeof(Cpx<double>) : sizeof(Cpx<float>);
    const size_t fwd = wv_fwd_lds_elems(T, levels, tile) * elem, inv = wv_inv_lds_elems(T, tile) * elem;
    return (fwd > inv ? fwd : inv) <= WV_LDS_MAX;
}

template <typename R>
hipError_t launch_prox_cx(hipStream_t s, bool cnc, const typename CxOf<R>::type* x, typename CxOf<R>::type* z, typename CxOf<R>::type* w,
                          const ProxParamsT<R>& p, size_t n) {
    if (n < 1 || (((uintptr_t)x | (uintptr_t)z | (uintptr_t)w) & 15)) return hipErrorInvalidValue;      // 16-byte accesses
    const size_t nv = n / CpxVec<R>::V;
    const dim3 grid(cx_blocks(nv + 1));
    if (cnc) hipLaunchKernelGGL((k_prox_cx<R, true>), grid, dim3(256), 0, s, (const Cpx<R>*)x, (Cpx<R>*)z, (Cpx<R>*)w, p, n);
    else     hipLaunchKernelGGL((k_prox_cx<R, false>), grid, dim3(256), 0, s, (const Cpx<R>*)x, (Cpx<R>*)z, (Cpx<R>*)w, p, n);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_wavelet_prox_cx(hipStream_t s, int wavelet, int levels, bool cnc, const typename CxOf<R>::type* x, typename CxOf<R>::type* z,
                                  typename CxOf<R>::type* w, typename CxOf<R>::type* coef, const ProxParamsT<R>& p, int B, int H, int W) {
    if (wv_check(wavelet, levels, H, W) != WV_OK || B < 1 || !wavelet_cx_fits(wavelet, levels, sizeof(R) == 8)) return hipErrorInvalidValue;
    WvcArgs<R> a = wv_args<Cpx<R>, R>(wavelet, levels, H, W);
    a.in0 = (const Cpx<R>*)x; a.in1 = (const Cpx<R>*)w; a.zin = (const Cpx<R>*)z; a.out = (Cpx<R>*)coef; a.p = p;
    a.x = (const Cpx<R>*)x; a.z = (Cpx<R>*)z; a.w = (Cpx<R>*)w;
    switch (wavelet) {
    case WV_HAAR: return wvc_prox_t<R, 2>(s, cnc, a, B);
    case WV_DB2:  return wvc_prox_t<R, 4>(s, cnc, a, B);
    case WV_DB4:  return wvc_prox_t<R, 8>(s, cnc, a, B);
    }
    return hipErrorInvalidValue;
}

#define CX_INST(R)                                                                                                                          \
    template hipError_t launch_prox_cx<R>(hipStream_t, bool, const CxOf<R>::type*, CxOf<R>::type*, CxOf<R>::type*, const ProxParamsT<R>&,   \
                                          size_t);                                                                                          \
    template hipError_t launch_wavelet_prox_cx<R>(hipStream_t, int, int, bool, const CxOf<R>::type*, CxOf<R>::type*, CxOf<R>::type*,        \
                                                  CxOf<R>::type*, const ProxParamsT<R>&, int, int, int);
CX_INST(float)
CX_INST(double)
#undef CX_INST

}  // namespace pnp
