// Convergence trace: the per-slice sums of squares behind r_pri = ||x - z||, r_dual = ||z - z_prev||, ||x||, ||z||, ||w|| and, with a
// ground truth, PSNR / RE (pnp_admm_*_run_traced, pnp_residuals; trace_plan.h has the order of the sums and the shape of the launch).
//
// ONE launch per check for all B slices: grid (groups, B), 256 threads.  A workgroup reduces `span` consecutive elements of its
// slice -- 16-byte loads of the four arrays where N and the pointers allow, element loads otherwise (N not a multiple of the vector
// width moves every slice but the first off 16-byte alignment) -- accumulates in double and writes its TRACE_Q partial sums; the last
// workgroup of a slice to finish (an integer ticket counter, reset by its taker) adds the slice's partials in workgroup order and
// writes the row.  The tree is fixed by (B, N): the same inputs give the same bits on every run; no floating-point atomics.
//
// Slice-order flavour (the slice-resident path at 256 x 256, float): z, z_prev and w lie in the row transform's order with a padded
// slice stride (slice_layout.h, sl_state_index) while x and the ground truth are in natural order.  Sums of squares of z, w and
// z - z_prev do not care about the order; for x - z a workgroup walks its span in tiles of four row pairs, sends the tile of x
// through LDS by the index map and pairs it there with z -- every global access is still a 16-byte lane access, no k_state_order
// pass, and addresses beyond 65536 floats of a slice (the padding) are never formed.
#include "internal.h"
#include "slice_layout.h"
#include "trace_plan.h"
#include <type_traits>

namespace pnp {

namespace {

template <typename R> struct VecOf;
template <> struct VecOf<float>  { using type = float4;  static constexpr int n = 4; };
template <> struct VecOf<double> { using type = double2; static constexpr int n = 2; };

__device__ __forceinline__ void unpack(const float4& v, float (&a)[4]) { a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
__device__ __forceinline__ void unpack(const double2& v, double (&a)[2]) { a[0] = v.x; a[1] = v.y; }

// img_E of the PnP solvers, S6:314, as solvers_pnp._finish_pnp forms it on the device: torch.round(x * 255.0) / 255.0 in the arithmetic of the
// state -- round half to even, and the division by a scalar is torch's multiplication by the scalar's reciprocal
__device__ __forceinline__ float quantised(float x) { return rintf(x * 255.0f) * (1.0f / 255.0f); }
__device__ __forceinline__ double quantised(double x) { return rint(x * 255.0) * (1.0 / 255.0); }

struct Sums {
    double s[TRACE_Q];
    __device__ __forceinline__ void state(double x, double z, double zp, double w) {
        const double d = x - z, e = z - zp;
        s[TR_XZ] += d * d; s[TR_ZZP] += e * e; s[TR_Z] += z * z; s[TR_W] += w * w;
    }
    __device__ __forceinline__ void x2(double x) { s[TR_X] += x * x; }
    template <typename R> __device__ __forceinline__ void truth(R x, uint8_t gt, bool quantise) {
        const double g = (double)gt, d = (double)(quantise ? quantised(x) : x) * 255.0 - g;      // k_metrics' own expression
        s[TR_E] += d * d; s[TR_G] += g * g;
    }
};

// workgroup sum in a fixed order (lanes by halving strides, then waves 0..3), partial to memory, and the slice's last workgroup adds
// the partials of all of them in workgroup order
__device__ __forceinline__ void finish(Sums& a, double* partial, unsigned* counter, double* out, int B) {
    __shared__ double wave_sum[TRACE_THREADS / 64][TRACE_Q];
    __shared__ unsigned ticket;
    const int tid = threadIdx.x, b = blockIdx.y, groups = gridDim.x;
#pragma unroll
    for (int q = 0; q < TRACE_Q; ++q) {
        double v = a.s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((tid & 63) == 0) wave_sum[tid >> 6][q] = v;
    }
    __syncthreads();
    double* mine = partial + ((size_t)b * groups + blockIdx.x) * TRACE_Q;
    if (tid == 0) {
        for (int q = 0; q < TRACE_Q; ++q) {
            double v = wave_sum[0][q];
            for (int wv = 1; wv < TRACE_THREADS / 64; ++wv) v += wave_sum[wv][q];
            __hip_atomic_store(mine + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // the partials (write-through stores) are out before the ticket is drawn: release, drain, then the counter -- in this order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(counter + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (ticket != (unsigned)(groups - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid < TRACE_Q) {
        const double* p = partial + (size_t)b * groups * TRACE_Q + tid;
        double v = 0.0;
        for (int g = 0; g < groups; ++g) v += __hip_atomic_load(p + (size_t)g * TRACE_Q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[(size_t)tid * B + b] = v;
    }
    if (tid == 0) __hip_atomic_store(counter + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // ready for the next launch on this stream
}

template <typename R>
struct TraceArgs {
    const R *x, *z, *zp, *w;       // [B] slices: x at stride N, the three state arrays at stride `state_stride`
    const uint8_t* gt;             // [B][N] or null
    size_t N, state_stride, span;
    int quantise, B;
    double* partial;
    unsigned* counter;
    double* out;                   // [TRACE_Q][B]
};

// natural order; VEC: 16-byte loads (N a multiple of the vector width, all pointers aligned)
template <typename R, bool VEC>
__global__ __launch_bounds__(TRACE_THREADS) void k_residuals(TraceArgs<R> p) {
    using V = typename VecOf<R>::type;
    constexpr int VW = VecOf<R>::n;
    const int tid = threadIdx.x, b = blockIdx.y;
    const size_t lo = (size_t)blockIdx.x * p.span, hi = lo + p.span < p.N ? lo + p.span : p.N;
    const R* x = p.x + (size_t)b * p.N;
    const R* z = p.z + (size_t)b * p.state_stride;
    const R* zp = p.zp + (size_t)b * p.state_stride;
    const R* w = p.w + (size_t)b * p.state_stride;
    const uint8_t* gt = p.gt ? p.gt + (size_t)b * p.N : nullptr;
    const bool quantise = p.quantise != 0;
    Sums a = {};
    if constexpr (VEC) {
#pragma unroll 2
        for (size_t i = lo + (size_t)tid * VW; i < hi; i += (size_t)TRACE_THREADS * VW) {
            R xv[VW], zv[VW], pv[VW], wv[VW];
            unpack(*reinterpret_cast<const V*>(x + i), xv);
            unpack(*reinterpret_cast<const V*>(z + i), zv);
            unpack(*reinterpret_cast<const V*>(zp + i), pv);
            unpack(*reinterpret_cast<const V*>(w + i), wv);
#pragma unroll
            for (int k = 0; k < VW; ++k) { a.state(xv[k], zv[k], pv[k], wv[k]); a.x2(xv[k]); }
            if (gt) {
                uint8_t g[VW];
                __builtin_memcpy(g, __builtin_assume_aligned(gt + i, VW), VW);               // one 4- / 2-byte load
#pragma unroll
                for (int k = 0; k < VW; ++k) a.truth(xv[k], g[k], quantise);
            }
        }
    } else {
        for (size_t i = lo + tid; i < hi; i += TRACE_THREADS) {
            const R xv = x[i];
            a.state(xv, z[i], zp[i], w[i]); a.x2(xv);
            if (gt) a.truth(xv, gt[i], quantise);
        }
    }
    finish(a, p.partial, p.counter, p.out, p.B);
}

// slice order (256 x 256 float): z, zp, w by sl_state_index at stride state_stride, x and gt natural
__global__ __launch_bounds__(TRACE_THREADS) void k_residuals_slice(TraceArgs<float> p) {
    __shared__ float xt[TRACE_TILE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const size_t lo = (size_t)blockIdx.x * p.span, hi = lo + p.span < p.N ? lo + p.span : p.N;       // multiples of TRACE_TILE (N = 65536)
    const float* x = p.x + (size_t)b * p.N;
    const float* z = p.z + (size_t)b * p.state_stride;
    const float* zp = p.zp + (size_t)b * p.state_stride;
    const float* w = p.w + (size_t)b * p.state_stride;
    const uint8_t* gt = p.gt ? p.gt + (size_t)b * p.N : nullptr;
    const bool quantise = p.quantise != 0;
    Sums a = {};
    for (size_t base = lo; base < hi; base += TRACE_TILE) {
        float zv[2][4], pv[2][4], wv[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + TRACE_THREADS * u;                      // 16-byte access f of the tile, in either order
            float xv[4];
            unpack(*reinterpret_cast<const float4*>(x + base + 4 * f), xv);
            unpack(*reinterpret_cast<const float4*>(z + base + 4 * f), zv[u]);
            unpack(*reinterpret_cast<const float4*>(zp + base + 4 * f), pv[u]);
            unpack(*reinterpret_cast<const float4*>(w + base + 4 * f), wv[u]);
            const int row = f >> 6, n0 = 4 * (f & 63);                  // natural: image row (of the tile's 8) x pixels n0 .. n0 + 3
#pragma unroll
            for (int k = 0; k < 4; ++k) { a.x2(xv[k]); xt[sl_state_index(row, n0 + k)] = xv[k]; }
            if (gt) {
                uint8_t g[4];
                __builtin_memcpy(g, __builtin_assume_aligned(gt + base + 4 * f, 4), 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) a.truth(xv[k], g[k], quantise);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + TRACE_THREADS * u;
            float xs[4];
            unpack(*reinterpret_cast<const float4*>(xt + 4 * f), xs);   // x of the pixels that z's access f holds
#pragma unroll
            for (int k = 0; k < 4; ++k) a.state(xs[k], zv[u][k], pv[u][k], wv[u][k]);
        }
        __syncthreads();
    }
    finish(a, p.partial, p.counter, p.out, p.B);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

size_t trace_scratch_bytes(int Bmax) { return (size_t)(TRACE_TARGET_GROUPS + Bmax) * TRACE_Q * sizeof(double); }      // B * trace_groups(B, N) < target + B

template <typename R>
hipError_t launch_residuals(hipStream_t s, const R* x, const R* z, const R* zp, const R* w, const uint8_t* gt, int quantise, int B, size_t N,
                            size_t state_stride, bool slice_order, double* partial, unsigned* counter, double* out) {
    if (B <= 0) return hipSuccess;
    TraceArgs<R> a;
    a.x = x; a.z = z; a.zp = zp; a.w = w; a.gt = gt; a.N = N; a.state_stride = state_stride; a.span = trace_span(B, N);
    a.quantise = quantise; a.B = B; a.partial = partial; a.counter = counter; a.out = out;
    const dim3 grid(trace_groups(B, N), B), block(TRACE_THREADS);
    constexpr int VW = VecOf<R>::n;
    const bool vec = N % VW == 0 && state_stride % VW == 0 && aligned16(x) && aligned16(z) && aligned16(zp) && aligned16(w) &&
                     (!gt || ((uintptr_t)gt % VW) == 0);
    if (slice_order) {
        if constexpr (std::is_same_v<R, float>) {
            if (N != 65536 || !vec) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_residuals_slice, grid, block, 0, s, a);
        } else {
            return hipErrorInvalidValue;
        }
    } else if (vec) {
        hipLaunchKernelGGL((k_residuals<R, true>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((k_residuals<R, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}
template hipError_t launch_residuals<float>(hipStream_t, const float*, const float*, const float*, const float*, const uint8_t*, int, int, size_t,
                                            size_t, bool, double*, unsigned*, double*);
template hipError_t launch_residuals<double>(hipStream_t, const double*, const double*, const double*, const double*, const uint8_t*, int, int,
                                             size_t, size_t, bool, double*, unsigned*, double*);

}  // namespace pnp
