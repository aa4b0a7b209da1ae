// Internal declarations shared by the translation units of libpnpmri.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <type_traits>
#include <stdint.h>
#include <stdlib.h>
#include "loop_schedule.h"
#include "prox_params.h"
#include "c2c_roles.h"
#include "trace_plan.h"

namespace pnp {

// Error reporting of the ABI layer (api.hip, api_conv.hip): formats the calling thread's message -- ONE thread_local buffer, owned by api.hip
// and read by pnp_last_error -- and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(PNP_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// complex / real types per precision: float2 for the production path, double2 for the fp64
// validation context (pnp_ctx_create_f64)
template <> struct CxOf<float>  { using type = float2; };
template <> struct CxOf<double> { using type = double2; };

// More than 64 KiB of dynamic LDS needs an opt-in per kernel and device: `done` is the launcher's own static std::atomic<bool>[64] of
// that kernel instantiation.  Only a launch that needs it makes it, and it asks for `cap`, the bound of every configuration of the
// kernel: the attribute is a cap, not an allocation, so one value serves every context on the device and a racing second opt-in writes
// the same value.
inline hipError_t lds_opt_in(const void* fn, std::atomic<bool>* done, size_t lds, size_t cap) {
    if (lds <= 64 * 1024) return hipSuccess;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
    if (e == hipSuccess) done[dev].store(true, std::memory_order_release);
    return e;
}

// the roles of a row / column launch, their argument structs and element forms: c2c_roles.h
using RowArgs = RowArgsT<float>;
using ColArgs = ColArgsT<float>;

// generic path (kernels_generic.hip); H, W in {256, 512}; R = float | double
template <typename R> hipError_t launch_rows(hipStream_t s, int W, RowIn in, bool inv, RowEpi epi, const RowArgsT<R>& a);
template <typename R> hipError_t launch_cols(hipStream_t s, int H, int W, bool pre_fwd, ColMid mid, bool post_inv, const ColArgsT<R>& a);
hipError_t upload_twiddles();       // fills the __device__ tables of the current device

// any-size path (kernels_anysize.hip): H, W in [128, 1024], the same roles and epilogues as launch_rows / launch_cols; plan and
// twiddle / chirp tables owned by the context (anysize_plan.h), in the context's precision
struct AnySize;
bool       anysize_supported(int n);
AnySize*   anysize_create(int H, int W, bool f64, hipError_t* err);
void       anysize_destroy(AnySize*);
int        anysize_describe(const AnySize*, int axis /* 0 rows (W), 1 columns (H) */, char* buf, int len);
template <typename R> hipError_t anysize_rows(const AnySize*, hipStream_t s, RowIn in, bool inv, RowEpi epi, const RowArgsT<R>& a);
template <typename R> hipError_t anysize_cols(const AnySize*, hipStream_t s, bool pre_fwd, ColMid mid, bool post_inv, const ColArgsT<R>& a);

// multi-coil (SENSE) row roles of the any-size kernels (coil_plan.h): the coil-expanding forward rows and the coil-combining inverse rows
template <typename R>
struct CoilRowArgsT {
    using C = typename CxOf<R>::type;
    const C*       maps;      // [Ks][C][H][W]
    const int32_t* coil_id;   // [B] or null (set 0)
    int            ncoils, H;
    C*             work;      // [B][C][H][W]: written by the expanding rows, read by the combining rows
    const C*       cin;       // expanding rows: the image, complex [B][H][W] ...
    const R*       rin;       // ... or real (cin null)
    C*             cout;      // combining rows: sum_c conj(S_c) * scale * inverse rows [+ la2 * p]
    const C*       p;         // combining rows: null (plain A^H), or the operand of G: la2 * p is added and Re<p, Gp> summed per row ...
    double*        partial;   // ... into [B * H]
    R              la2, scale;
    int            nrows;     // B * H
};
template <typename R> hipError_t anysize_coil_rows_in(const AnySize*, hipStream_t s, const CoilRowArgsT<R>& a);
template <typename R> hipError_t anysize_coil_rows_epi(const AnySize*, hipStream_t s, const CoilRowArgsT<R>& a);

// multi-coil pointwise kernels and the batched conjugate-gradient updates (kernels_coils.hip; sums by coil_plan.h).  Complex arrays
// [B][N] in the context's precision, partials and scalars in double; grid (cg_blocks(N), B).
hipError_t launch_expand_ids(hipStream_t s, const int32_t* mask_id, int32_t* out, int B, int C);          // out[b * C + c] = mask_id[b]
// the state arrays z, w, x of a coil context: real, or complex with pnp_set_image(PNP_IMAGE_COMPLEX) (the CX roles)
template <typename R, bool CX> using CoilState = typename std::conditional<CX, typename CxOf<R>::type, R>::type;
template <typename R, bool CX = false>
hipError_t launch_cg_begin(hipStream_t s, const CoilState<R, CX>* z, const CoilState<R, CX>* w, typename CxOf<R>::type* xh, int B, size_t N);
template <typename R> hipError_t launch_cg_init(hipStream_t s, const typename CxOf<R>::type* aty, const typename CxOf<R>::type* xh,
                                                const typename CxOf<R>::type* gp, typename CxOf<R>::type* r, typename CxOf<R>::type* p,
                                                R la2, double* part_rr, double* part_bb, int B, size_t N);
// alpha = <r,r> / Re<p,Gp> from the partials; x^ += alpha p, r -= alpha Gp, partials of the new <r,r>; x_out (last iteration): |Re x^|, CX: x^
template <typename R, bool CX = false> hipError_t launch_cg_xr(hipStream_t s, typename CxOf<R>::type* xh, typename CxOf<R>::type* r,
                                              const typename CxOf<R>::type* p, const typename CxOf<R>::type* gp, const double* part_rr,
                                              const double* part_pgp, double* part_rr_next, double* scal /*[B][4]: alpha, beta, rr, -*/,
                                              CoilState<R, CX>* x_out, int B, size_t N, int H);
template <typename R> hipError_t launch_cg_p(hipStream_t s, const typename CxOf<R>::type* r, typename CxOf<R>::type* p, const double* part_rr,
                                             const double* part_rr_next, double* scal, int B, size_t N);
hipError_t launch_cg_residual(hipStream_t s, const double* part_rr, const double* part_bb, double* rel /*[B]*/, int B, size_t N);
template <typename R> hipError_t launch_cabs(hipStream_t s, const typename CxOf<R>::type* in, R* out, size_t n);
hipError_t launch_prox_f64(hipStream_t s, bool cnc, const double* x, double* z, double* w, ProxParamsT<double> p, size_t n);

// complex-valued images on a coil context (kernels_complex.hip): the z / w step on complex arrays [n] resp. [B][H][W], interleaved, in the
// context's precision.  launch_prox_cx: 16-byte accesses, so x, z, w must be 16-byte aligned (hipErrorInvalidValue otherwise).
// launch_wavelet_prox_cx: two launches, coef [B][H][W] complex scratch; wavelet_cx_fits: whether the setting's tile fits the LDS
template <typename R>
hipError_t launch_prox_cx(hipStream_t s, bool cnc, const typename CxOf<R>::type* x, typename CxOf<R>::type* z, typename CxOf<R>::type* w,
                          const ProxParamsT<R>& p, size_t n);
template <typename R>
hipError_t launch_wavelet_prox_cx(hipStream_t s, int wavelet, int levels, bool cnc, const typename CxOf<R>::type* x, typename CxOf<R>::type* z,
                                  typename CxOf<R>::type* w, typename CxOf<R>::type* coef, const ProxParamsT<R>& p, int B, int H, int W);
bool wavelet_cx_fits(int wavelet, int levels, bool f64);

// PnP denoisers on complex images (kernels_pnp_cx.hip, pnp_cx_ops.h): n complex floats, interleaved, and the real planes of a CNN -- one
// plane of n floats (mode CXD_MODULUS) or two, the second n floats behind the first (CXD_PARTS).  a (+ b, or null) is the value the network
// is asked about; every complex array and the plane base on 16 bytes (hipErrorInvalidValue otherwise)
hipError_t launch_cx_den_in(hipStream_t s, int mode, const float2* a, const float2* b, float* planes, float g, size_t n);
hipError_t launch_cx_den_out(hipStream_t s, int mode, const float* q, const float2* a, const float2* b, float2* z, float g, size_t n);
hipError_t launch_cx_den_out_dual(hipStream_t s, int mode, const float* q, const float2* a, const float2* b, float2* x, float2* z, float2* w,
                                  float g, size_t n);

// coil mixing ahead of the multi-coil solve (kernels_coilmix.hip, coilmix_plan.h): interleaved complex arrays in R, no context.
// out[b][j][p] = sum_c m[set_id[b]][j][c] in[b][c][p] (in [B][C_in][N], m [Ks][C_out][C_in], out [B][C_out][N]; set_id null: set 0), and
// the per-slice Gram matrices of the calibration region, gram [B][C][C] complex double
template <typename R> hipError_t launch_coil_mix(hipStream_t s, const R* in, const R* m, const int32_t* set_id, R* out, int B, int C_in,
                                                 int C_out, size_t N);
template <typename R> hipError_t launch_coil_gram(hipStream_t s, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram,
                                                  int B, int C, int H, int W, int ncal);

// coil sensitivity maps from the calibration region (kernels_coilmaps.hip, coilmaps_plan.h): interleaved complex arrays in R.  The windowed
// calibration region of B C pseudo-slices (+0 elsewhere) and the lowest offset of an unsampled calibration point per slice, miss [B] (-1:
// none); the local dominant eigenvectors of the low-resolution coil images img [B][C][H][W] -> maps [B][C][H][W], lambda [B][H][W]; the
// support stage of both estimators: maps zeroed where gate < floor (gate null: no such rule) or key < frac * the slice's largest key (part:
// scratch of B * coilmaps_spans(N) values).  Here key = lambda, frac = tau2 and no gate
template <typename R> hipError_t launch_calib_window(hipStream_t s, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, R* out,
                                                     int32_t* miss, int B, int C, int H, int W, int ncal);
template <typename R> hipError_t launch_coil_eigmaps(hipStream_t s, const R* img, R* maps, R* lambda, int B, int C, int H, int W, int r, int iters);
template <typename R> hipError_t launch_maps_support(hipStream_t s, const R* gate, R floor, const R* key, R frac, R* part, R* maps, int B, int C,
                                                     size_t N);

// ESPIRiT coil maps (kernels_espirit.hip, espirit_plan.h).  The patch Gram matrices of the calibration block, gram [B][n][n] complex double,
// n = C k^2; the per-pixel stage: img [B][C][H][W], w [B][C][C][D][D] (D = 2 k - 1), the phasor tables eh [H][D] and ew [W][D] -> the unit
// vectors maps [B][C][H][W], lambda [B][H][W] and inorm [B][H][W] = ||I||; the support is launch_maps_support with gate = lambda, floor =
// crop, key = inorm, frac = tau
template <typename R> hipError_t launch_calib_patch_gram(hipStream_t s, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram,
                                                         int B, int C, int H, int W, int ncal, int k);
template <typename R> hipError_t launch_espirit_maps(hipStream_t s, const R* img, const R* w, const R* eh, const R* ew, R* maps, R* lambda,
                                                     R* inorm, int B, int C, int H, int W, int k, int iters);

// pointwise
hipError_t launch_prox(hipStream_t s, bool cnc, const float* x, float* z, float* w, ProxParams p, size_t n);
hipError_t launch_combine(hipStream_t s, const float* z, const float* x, const float* w, const float* sden,
                          float* t, float c1, float c2, float c3, size_t n);
hipError_t launch_add(hipStream_t s, const float* a, const float* b, float* o, size_t n);
hipError_t launch_dual_clamp(hipStream_t s, float* x, float* z, float* w, size_t n);
template <typename X> hipError_t launch_metrics(hipStream_t s, const X* x, const uint8_t* gt, double* acc /*[B][2]*/, int B, int N);
hipError_t upload_gauss();
template <typename X> hipError_t launch_ssim(hipStream_t s, const X* x, const uint8_t* gt, double* partial /*[B][tiles]*/, int B, int H, int W);
hipError_t launch_widen(hipStream_t s, const float* in, double* out, size_t n);      // float -> double

// convergence trace (kernels_trace.hip): the TRACE_Q sums of squares of trace_plan.h for B slices of N elements into out [TRACE_Q][B], one
// launch.  x (and gt, or null) in natural order at stride N; z, zp, w at stride `state_stride`, in natural order or -- slice_order, 256 x 256
// float -- by sl_state_index.  partial / counter: scratch of trace_scratch_bytes(Bmax) bytes resp. Bmax zeroed unsigneds, one stream at a time.
size_t trace_scratch_bytes(int Bmax);
template <typename R>
hipError_t launch_residuals(hipStream_t s, const R* x, const R* z, const R* zp, const R* w, const uint8_t* gt, int quantise, int B, size_t N,
                            size_t state_stride, bool slice_order, double* partial, unsigned* counter, double* out);

// wavelet-domain sparsity (kernels_wavelet.hip, wavelet_plan.h): Psi / Psi^T of B slices [H][W] (in != out: tiles read their neighbours'
// halo), and the prox step z+ = Psi^T thresholded(Psi ...), w+ = (x + w) - z+ in place, through `coef`, scratch of B H W values
// Cycle spinning: (sy, sx) in [0, 2^levels) is the frame's shift, by addressing alone.  The prox takes K >= 1 shifts [K][2] (host; null:
// one unshifted step): K = 1 is the two launches in that frame; K > 1 runs them per shift, the syntheses summing z+ in `acc` (B H W values)
// in the order of the table, and the last one writes z+ = (acc + z_(K-1)) (1 / K), w+ = (x + w) - z+ -- nothing else writes z or w.
template <typename R> hipError_t launch_dwt2(hipStream_t s, int wavelet, int levels, bool inv, const R* in, R* out, int B, int H, int W,
                                             int sy = 0, int sx = 0);
template <typename R> hipError_t launch_wavelet_prox(hipStream_t s, int wavelet, int levels, bool cnc, const R* x, R* z, R* w, R* coef,
                                                     const ProxParamsT<R>& p, int B, int H, int W, const int* shifts = nullptr, int K = 1,
                                                     R* acc = nullptr);

// temporal sparsity (kernels_temporal.hip, temporal_plan.h): the prox on the DFT along the frames of B / frames series of `frames` slices
// of N values, real or (CX) complex, in place on z and w; one launch.  e: the context's twiddle matrix in R (tp_twiddle_matrix).
// The accesses are as wide as N and the arrays' alignment allow (tp_group); an array not aligned to one value is hipErrorInvalidValue.
template <typename R, bool CX>
hipError_t launch_temporal_prox(hipStream_t s, bool cnc, const CoilState<R, CX>* x, CoilState<R, CX>* z, CoilState<R, CX>* w, const R* e,
                                const ProxParamsT<R>& p, int frames, bool keep_dc, int B, size_t N);

// locally low-rank prox (kernels_lowrank.hip, lowrank_plan.h): singular-value thresholding of the block x block patches, anchored at the
// shift (sy, sx), of B / frames series of `frames` real slices of H x W, in place on z and w; one launch.  p: thr and ib already scaled.
// A setting lr_check refuses, a shift outside [0, block) or an array not aligned to one value is hipErrorInvalidValue.
template <typename R>
hipError_t launch_lowrank_prox(hipStream_t s, bool cnc, const R* x, R* z, R* w, const ProxParamsT<R>& p, int frames, int block, int sy, int sx,
                               int B, int H, int W);

// calibration (pnp_calibrate_stream): the slice-resident loop's access shape without its arithmetic, `passes` passes over `slices` slices of 256 KiB
hipError_t launch_calibrate_stream(hipStream_t s, float* z, float* w, const float* y, int slices, int passes);
// The denoisers' conv layers.  Shape rules, tiles / items and the persistent grids of every launcher below: conv_plan.h -- a launcher
// returns hipErrorInvalidValue for what the plan's check of its layer kind refuses (api_conv.hip turns the same check into a message first).
// optional HIP backend of the denoisers' 64-channel conv3x3 body layers (kernels_conv.hip); activations NHWC float32
hipError_t launch_conv_pack_w(hipStream_t s, const float* w_oihw /*[64][64][3][3]*/, float* wfrag /*36 864 floats*/);
hipError_t launch_conv3x3_c64(hipStream_t s, const float* x, const float* wfrag, const float* bias, const float* skip,
                              float* y, int n, int H, int W, int relu, int dilation /* 1..4 */);
// the same layer in split-half arithmetic on the f16 matrix cores (kernels_conv_f16x3.hip): own packing, same buffer size
hipError_t launch_conv_pack_w_f16x3(hipStream_t s, const float* w_oihw /*[C][C][3][3]*/, float* wfrag /*9 C C floats*/, int C);
hipError_t launch_conv3x3_f16x3(hipStream_t s, const float* x, const float* wfrag, const float* bias, const float* skip,
                                float* y, int n, int C /* 64 k <= 1024 */, int H, int W, int relu, int dilation /* 1..4; 1 if C > 64 */,
                                int fmt = 0 /* bit 0: x, bit 1: skip, bit 2: y in the split activation format (f16x3_common.h) */);
// the same layer at dilation 1 with 64 x 64 wave tiles, compute + helper waves (kernels_conv_f16x3_wide.hip): same arguments, same packed
// weights, bit-equal results; launch_conv3x3_f16x3 dispatches to it (conv_wide_mode below) -- callers never name it
hipError_t launch_conv3x3_f16x3_wide(hipStream_t s, const float* x, const float* wfrag, const float* bias, const float* skip,
                                     float* y, int n, int C, int H, int W, int relu, int fmt);
int conv_wide_mode();            // -1 = by size (conv_plan.h: cp_use_wide), 0 = never, 1 = always (dilation 1); initial value: PNP_CONV_WIDE
int conv_set_wide_mode(int m);   // pnp_conv3x3_f16x3_set_variant; returns the previous setting.  One atomic int: any thread may set it while others launch
hipError_t launch_conv3x3_tail_f16x3(hipStream_t s, const float* x_nhwc, const float* x2_nhwc /* null or added to x */, const float* w_oihw,
                                     const float* bias, float* y_nchw, int n, int cout, int H, int W,
                                     int shuffle_h = 0, int shuffle_w = 0 /* FFDNet: cout = 4 written as one pixel-shuffled [shuffle_h][shuffle_w] channel */);
hipError_t launch_ffdnet_head(hipStream_t s, const float* x_full /* [n][1][h][w] */, const float* sigma, int sigma_per_image, const float* w_oihw /* [64][5][3][3] */,
                              const float* bias, float* y_nhwc /* [n][ceil(h/2)][ceil(w/2)][64] */, int n, int h, int w, int relu);
// DRUNet's 2 x 2 stride-2 convolution (C -> 2C, up = 0) and 2 x 2 transposed convolution (C -> C/2, up = 1) in the same arithmetic
// (kernels_pix2x2_f16x3.hip); x2: null or a tensor of x's shape added to it
hipError_t launch_pix2_pack_w_f16x3(hipStream_t s, const float* w, float* wfrag /* 8 C C floats (down), 2 C C (up) */, int C, int up);
hipError_t launch_pix2x2_f16x3(hipStream_t s, const float* x, const float* x2, const float* wfrag, float* y, int n, int C, int H, int W, int up);
hipError_t launch_relayout64(hipStream_t s, const float* in, float* out, int n, int HW, bool to_nhwc);
hipError_t launch_conv3x3_head(hipStream_t s, const float* x_nchw, const float* w_oihw, const float* bias, float* y_nhwc,
                               int n, int cin, int H, int W, int relu);
hipError_t launch_conv3x3_tail(hipStream_t s, const float* x_nhwc, const float* w_oihw, const float* bias, float* y_nchw,
                               int n, int cout, int H, int W);

// the denoisers' layers in HALF precision (kernels_conv_f16.hip, kernels_pix2x2_f16.hip): activations NHWC halves, weights
// rounded to half at pack time, float32 accumulation, one rounding on store.  fmt: HF_FMT_X32 | HF_FMT_SKIP32 | HF_FMT_Y32 (f16_common.h)
hipError_t launch_conv_pack_w_f16(hipStream_t s, const float* w_oihw /*[C][C][3][3]*/, void* wfrag /*9 C C halves*/, int C);
hipError_t launch_conv3x3_f16(hipStream_t s, const void* x, const void* wfrag, const float* bias, const void* skip, void* y,
                              int n, int C /* 64 k <= 1024 */, int H, int W, int relu, int dilation /* 1..4; 1 if C > 64 */, int fmt);
hipError_t launch_conv3x3_head_f16(hipStream_t s, const float* x, const float* sigma, int sigma_per_image, const float* w_oihw, const float* bias,
                                   void* y_nhwc, int n, int cin, int H, int W, int relu, int ffdnet /* x = the full-resolution [n][1][H][W] image */);
hipError_t launch_conv3x3_tail_f16(hipStream_t s, const void* x_nhwc, const void* x2_nhwc /* null or added to x */, const float* w_oihw,
                                   const float* bias, float* y, int n, int cout, int H, int W, int shuffle_h = 0, int shuffle_w = 0);
hipError_t launch_pix2_pack_w_f16(hipStream_t s, const float* w, void* wfrag /* 8 C C halves (down), 2 C C (up) */, int C, int up);
hipError_t launch_pix2x2_f16(hipStream_t s, const void* x, const void* x2, const void* wfrag, void* y, int n, int C, int H, int W, int up, int y_f32);

// steps of a run driven launch by launch (engine_host.h, chain_step; the *_step functions of the two-launch engines below)
enum class ChainStep { open, cols, mid, last };

// fused 256x256 path (kernels_fused256.hip): state resident in the ctx, two slices packed into
// one complex transform.  See DESIGN.md.
struct Fused256;
Fused256*  fused256_create(int Bmax, hipError_t* err);
void       fused256_destroy(Fused256*);
// builds the Hermitian-symmetrised measurement / mask tables from y and the masks
hipError_t fused256_prepare(Fused256*, hipStream_t s, const float2* y, const uint8_t* mask_bank,
                            const int32_t* mask_id, int B);
// iters iterations of x=dc(z,w); (z,w)=prox(x,z,w) on z,w [B][256][256]; x written on the last
hipError_t fused256_run(Fused256*, hipStream_t s, float* z, float* w, float* x, int B, int iters,
                        bool cnc, float dc_c, ProxParams p, const FusedSchedule& sch);
// one data-consistency step on caller pointers
hipError_t fused256_dc(Fused256*, hipStream_t s, const float* z, const float* w, float* x, int B, float dc_c);
// one launch of a run's chain on the whole batch (chain_step): rows read z, w and write zo, wo, x (last) or zo, wo (mid)
hipError_t fused256_step(Fused256*, hipStream_t s, ChainStep st, const float* z, const float* w, float* zo, float* wo, float* x, int B,
                         bool cnc, float dc_c, ProxParams p, const FusedSchedule& sch, bool u_first);

// "split chain" engine for 256x256 (kernels_fused256.hip, k_fcols2): one column chain per thread and
// slice; R = float | double.  y is [B][256][256] complex in R (float2 / double2 layout).
template <typename R> struct Fused256S;
template <typename R> Fused256S<R>* fused256s_create(int Bmax, hipError_t* err);
template <typename R> void          fused256s_destroy(Fused256S<R>*);
template <typename R> hipError_t    fused256s_prepare(Fused256S<R>*, hipStream_t s, const void* y, const uint8_t* mask_bank,
                                                      const int32_t* mask_id, int B);
template <typename R> hipError_t    fused256s_run(Fused256S<R>*, hipStream_t s, R* z, R* w, R* x, int B, int iters, bool cnc,
                                                  R dc_c, ProxParamsT<R> p, const FusedSchedule& sch);
template <typename R> hipError_t    fused256s_dc(Fused256S<R>*, hipStream_t s, const R* z, const R* w, R* x, int B, R dc_c);
template <typename R> hipError_t    fused256s_step(Fused256S<R>*, hipStream_t s, ChainStep st, const R* z, const R* w, R* zo, R* wo, R* x, int B,
                                                   bool cnc, R dc_c, ProxParamsT<R> p, const FusedSchedule& sch, bool u_first);

// slice-resident 256x256 path (kernels_slice256.hip): one workgroup keeps one slice in registers for a whole run
struct Slice256;
Slice256*  slice256_create(int Bmax, int pad_kb /* state */, int yh_pad_kb /* table */, hipError_t* err);
void       slice256_destroy(Slice256*);
int        slice256_cus(const Slice256*);     // compute units of the device (= slices in flight)
hipError_t slice256_prepare(Slice256*, hipStream_t s, const float2* y, const uint8_t* mask_bank, const int32_t* mask_id, int B);
// z, w in SLICE ORDER (slice_layout.h, sl_state_index); x comes out in natural order
hipError_t slice256_run(Slice256*, hipStream_t s, float* z, float* w, float* x, int B, int iters, bool cnc, float dc_c,
                        ProxParams p, const FusedSchedule& sch);
// in-place conversion of both state arrays [B][256][256] between natural order and slice order
hipError_t slice256_state_order(Slice256*, hipStream_t s, float* z, float* w, int B, bool to_slice);
// Convergence trace of a slice-order state (z, w as slice256_run leaves them; the caller's arrays when the engine keeps no padded ones):
// keep z as it lies now as the z_prev of the next check (the copy is the engine's), and the reduction of launch_residuals on x (natural),
// z, that z_prev and w where they lie.
hipError_t slice256_trace_snapshot(Slice256*, hipStream_t s, const float* z, int B);
hipError_t slice256_residuals(Slice256*, hipStream_t s, const float* x, const float* z, const float* w, const uint8_t* gt, int B,
                              double* partial, unsigned* counter, double* out);

// fused 512x512 path (kernels_fused512.hip): same scheme with 32-lane transforms
struct Fused512;
Fused512*  fused512_create(int Bmax, hipError_t* err);
void       fused512_destroy(Fused512*);
hipError_t fused512_prepare(Fused512*, hipStream_t s, const float2* y, const uint8_t* mask_bank,
                            const int32_t* mask_id, int B);
hipError_t fused512_run(Fused512*, hipStream_t s, float* z, float* w, float* x, int B, int iters,
                        bool cnc, float dc_c, ProxParams p, const FusedSchedule& sch);
hipError_t fused512_dc(Fused512*, hipStream_t s, const float* z, const float* w, float* x, int B, float dc_c);
hipError_t fused512_step(Fused512*, hipStream_t s, ChainStep st, const float* z, const float* w, float* zo, float* wo, float* x, int B,
                         bool cnc, float dc_c, ProxParams p, const FusedSchedule& sch, bool u_first);

}  // namespace pnp
