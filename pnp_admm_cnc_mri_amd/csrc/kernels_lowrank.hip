// Locally low-rank prox (pnp_set_lowrank; include/pnp_mri.h, "low-rank"): singular-value thresholding of the b x b patches of a series
// across its T frames, one launch, float and double, real images, L1 and CNC.
//   k_lowrank_prox    a workgroup owns up to LR_MAX_GROUP horizontally adjacent patches of one series (lowrank_plan.h): their P x T matrices
//                     are staged in LDS, the T x T Gram matrices formed and diagonalised there by cyclic Jacobi in the round-robin ordering
//                     (T / 2 disjoint rotations a round, all patches of the group side by side; V in double), M = V g(sigma) V^T takes the Gram matrix's
//                     place and z+ = X M, w+ = u - z+ are the only values written, every pixel-frame by one thread.  Every load, sum,
//                     rotation and store is an item function of lowrank_plan.h, run here one item per thread with a barrier between the
//                     passes (lr_run_group); the sweep loop ends on a test every thread reads from LDS after a barrier, so it is uniform
//                     over the workgroup, and under LR_MAX_SWEEPS.
// -ffp-contract=off (Makefile); products are chained by explicit fma.  Vector stores only, no atomics.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 80 (float L1), 116 (float CNC), 90 (double L1), 124 (double CNC) VGPRs,
// no scratch, no SGPR or VGPR spill; occupancy 6 / 4 / 5 / 4 waves per SIMD.  LDS is dynamic, lr_lds_bytes: within LR_LDS_BUDGET where one
// patch fits it, else one patch, up to LR_LDS_MAX (by opt-in beyond 64 KiB): 131 KiB for b = 8, T = 64 in double CNC, the most admitted
// among the settings the plan owes.
#include "internal.h"
#include "prox_ops.h"
#include "lowrank_plan.h"

namespace pnp {

namespace {

struct LrThreads {
    template <typename F> __device__ void items(int n, F f) const {
        for (int i = threadIdx.x; i < n; i += LR_THREADS) f(i);
    }
    __device__ void sync() const { __syncthreads(); }
};

template <typename R, bool CNC>
__global__ __launch_bounds__(LR_THREADS) void k_lowrank_prox(const LrArgs<R> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lr_smem[];
    const unsigned per = (unsigned)(a.ny * a.ngx), s = blockIdx.x / per, gi = blockIdx.x - s * per;
    LrThreads ex;
    lr_run_group<R, CNC>(a, (int)s, (int)gi, lr_smem, ex);
}

template <typename R, bool CNC>
hipError_t lowrank_launch(hipStream_t s, const LrArgs<R>& a) {
    const size_t blocks = lr_groups(a.S, a.ny, a.ngx);
    if (blocks < 1 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t lds = lr_lds_bytes(a.T, a.b, sizeof(R), CNC);
    if (lds > LR_LDS_MAX) return hipErrorInvalidValue;                // lr_check refuses such a setting
    static std::atomic<bool> done[64] = {};
    if (hipError_t e = lds_opt_in((const void*)k_lowrank_prox<R, CNC>, done, lds, LR_LDS_MAX)) return e;
    hipLaunchKernelGGL((k_lowrank_prox<R, CNC>), dim3((unsigned)blocks), dim3(LR_THREADS), lds, s, a);
    return hipGetLastError();
}

}  // namespace

template <typename R>
hipError_t launch_lowrank_prox(hipStream_t s, bool cnc, const R* x, R* z, R* w, const ProxParamsT<R>& p, int frames, int block, int sy, int sx,
                               int B, int H, int W) {
    if (lr_check(frames, block, H, W, B, sizeof(R), cnc) != LR_OK || !lr_shift_ok(block, sy, sx) || !x || !z || !w) return hipErrorInvalidValue;
    if (((uintptr_t)x | (uintptr_t)z | (uintptr_t)w) % sizeof(R)) return hipErrorInvalidValue;
    LrArgs<R> a;
    a.x = x; a.z = z; a.w = w; a.p = p;
    a.H = H; a.W = W; a.T = frames; a.S = B / frames; a.b = block; a.sy = sy; a.sx = sx;
    lr_fill_grid(a, cnc);
    return cnc ? lowrank_launch<R, true>(s, a) : lowrank_launch<R, false>(s, a);
}

template hipError_t launch_lowrank_prox<float>(hipStream_t, bool, const float*, float*, float*, const ProxParamsT<float>&, int, int, int, int, int, int, int);
template hipError_t launch_lowrank_prox<double>(hipStream_t, bool, const double*, double*, double*, const ProxParamsT<double>&, int, int, int, int, int, int, int);

}  // namespace pnp
