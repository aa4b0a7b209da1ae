// Temporal sparsity (pnp_set_temporal; include/pnp_mri.h, "temporal sparsity"): the prox on the coefficients of a unitary DFT along the
// frames of every pixel's series, one launch, float and double, real and complex values, L1 and CNC.
//   k_temporal_prox   a workgroup owns a run of P consecutive pixels of one series across its T frames (temporal_plan.h): the run is
//                     staged in LDS as [T][P], the coefficients formed by direct sums, thresholded, summed back; z+ and w+ = (x + w) - z+
//                     are the only values written, every pixel-frame by one thread.  Every load, sum and store is an item function of
//                     temporal_plan.h, run here one item per thread in four passes (load, coef, synth, store); VP (pixels per 16-, 8-
//                     or 4-byte global access) is chosen by tp_group from N and the arrays' alignment, so no access is wider than the
//                     addresses allow.  The two middle passes give a wavefront one block of coefficients resp. frames: their twiddle
//                     rows are read through scalar loads.
// -ffp-contract=off (Makefile); products are chained by explicit fma.  Vector stores only, no atomics.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 16 instantiations): 31 .. 61 VGPRs, no scratch, no VGPR spill; the
// unrolled walks keep their twiddles in scalar registers and the compiler parks 2 .. 54 of them in VGPR lanes (SGPR spills, no memory;
// most in double, whose twiddles take two registers each); occupancy 7 waves per SIMD.  Unrolled twice (`#pragma unroll 2` on the three walks) it is 0 .. 14, and
// measured slower from T = 8 up (T = 64, L1, float: 0.378 against 0.331 ms; double iteration: 0.368 against 0.349 ms), so it is not the build.  LDS is dynamic, tp_lds_bytes: 16 .. 32 KiB up to
// T = 32, 49.7 KiB (real float) resp. 48 KiB (complex double) at T = 64 -- never beyond the 64 KiB that need no opt-in.
#include "internal.h"
#include "prox_ops.h"
#include "temporal_plan.h"

namespace pnp {

namespace {

template <typename R, bool CX, bool CNC, int VP>
__global__ __launch_bounds__(TP_THREADS) void k_temporal_prox(const TpArgs<R, CX> a, unsigned runs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
    const unsigned s = blockIdx.x / runs, r = blockIdx.x - s * runs;
    const TpRun<R, CX> t = tp_run_of<R, CX>(a, (int)s, r, tp_smem);
    const int tid = threadIdx.x;
    for (int i = tid, n = tp_load_items(a.T, t.np, VP); i < n; i += TP_THREADS) tp_load_item<R, CX, CNC, VP>(i, a, t);
    __syncthreads();
    for (int i = tid, n = tp_coef_items(a.T, CX, t.np); i < n; i += TP_THREADS) tp_coef_item<R, CX, CNC>(i, a, t);
    __syncthreads();
    for (int i = tid, n = tp_synth_items(a.T, t.np); i < n; i += TP_THREADS) tp_synth_item<R, CX>(i, a, t);
    __syncthreads();
    for (int i = tid, n = tp_store_items(a.T, t.np, VP); i < n; i += TP_THREADS) tp_store_item<R, CX, VP>(i, a, t);
}

template <typename R, bool CX, bool CNC, int VP>
hipError_t temporal_launch(hipStream_t s, const TpArgs<R, CX>& a) {
    const size_t runs = tp_runs(a.N, a.P), blocks = runs * (size_t)a.S;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t lds = tp_lds_bytes(a.T, CX, sizeof(R));
    if (lds > 64 * 1024) return hipErrorInvalidValue;                 // the plan never asks for more
    hipLaunchKernelGGL((k_temporal_prox<R, CX, CNC, VP>), dim3((unsigned)blocks), dim3(TP_THREADS), lds, s, a, (unsigned)runs);
    return hipGetLastError();
}

template <typename R, bool CX, int VP>
hipError_t temporal_launch_vp(hipStream_t s, bool cnc, const TpArgs<R, CX>& a) {
    return cnc ? temporal_launch<R, CX, true, VP>(s, a) : temporal_launch<R, CX, false, VP>(s, a);
}

}  // namespace

template <typename R, bool CX>
hipError_t launch_temporal_prox(hipStream_t s, bool cnc, const CoilState<R, CX>* x, CoilState<R, CX>* z, CoilState<R, CX>* w, const R* e,
                                const ProxParamsT<R>& p, int frames, bool keep_dc, int B, size_t N) {
    using V = TpValue<R, CX>;
    static_assert(sizeof(V) == sizeof(CoilState<R, CX>), "the state's element is the plan's value");
    if (tp_check(frames, B) != TP_OK || N < 1 || !x || !z || !w || !e) return hipErrorInvalidValue;
    const uintptr_t addr = (uintptr_t)x | (uintptr_t)z | (uintptr_t)w;
    if (addr % sizeof(V)) return hipErrorInvalidValue;
    TpArgs<R, CX> a;
    a.x = (const V*)x; a.z = (V*)z; a.w = (V*)w; a.e = e; a.p = p;
    a.scale = (R)(1.0 / sqrt((double)frames));
    a.N = N; a.T = frames; a.S = B / frames; a.P = tp_run(frames, CX, sizeof(R)); a.keep_dc = keep_dc ? 1 : 0;
    size_t align = 16;                                               // what the three arrays share, 16 bytes at most
    while (addr % align) align >>= 1;
    const int vp = tp_group(N, sizeof(V), align);
    constexpr int VMAX = 16 / (int)sizeof(V);
    if constexpr (VMAX >= 4) if (vp == 4) return temporal_launch_vp<R, CX, 4>(s, cnc, a);
    if constexpr (VMAX >= 2) if (vp == 2) return temporal_launch_vp<R, CX, 2>(s, cnc, a);
    return temporal_launch_vp<R, CX, 1>(s, cnc, a);
}

#define TP_INST(R, CX)                                                                                                                   \
    template hipError_t launch_temporal_prox<R, CX>(hipStream_t, bool, const CoilState<R, CX>*, CoilState<R, CX>*, CoilState<R, CX>*,     \
                                                    const R*, const ProxParamsT<R>&, int, bool, int, size_t);
TP_INST(float, false)
TP_INST(float, true)
TP_INST(double, false)
TP_INST(double, true)
#undef TP_INST

}  // namespace pnp
