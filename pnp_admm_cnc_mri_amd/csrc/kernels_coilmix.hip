// Coil mixing ahead of the multi-coil solve for gfx950, float and double (coilmix_plan.h): noise prewhitening and coil compression are one
// C_out x C_in complex matrix per coil set, applied to every k-space point of the measurements and to every pixel of the maps.
//   k_coil_mix   out[b][j][p] = sum_c M[set(b)][j][c] in[b][c][p]: a thread owns 16 bytes of consecutive points (2 float, 1 double) and
//                all C_out sums in registers (C_out rounded up to 4, 8, 16 or 32: 32 complex sums are 128 registers in either precision);
//                per input coil, in order, the workgroup reads one coalesced run of in[b][c][.] and every lane the same row of M^T from LDS
//                (a broadcast; M goes through LDS COILMIX_MIX_CHUNK columns at a time).  A stream of (C_in + C_out) 8 B N bytes per
//                slice; 8 C_in C_out flops per point, which at 128 -> 32 (32 k) is bound by the f32 vector unit and not by HBM.
//   k_coil_gram  R_b[i][j] = sum_{q in calibration} mask_b(q) y_b[i](q) conj(y_b[j](q)) in double: a workgroup owns one slice and one
//                COILMIX_TILE^2 tile of pairs (i <= j by tiles), stages COILMIX_GRAM_POINTS points x 2 COILMIX_TILE coils in LDS (32 KiB;
//                64 coils of a 24^2 region would be 295 KB, more than a compute unit has) and every thread runs ONE chain over the points
//                in the plan's order; it stores R[i][j] and its conjugate R[j][i], so the matrix is Hermitian to the bit.
// Vector stores only, no atomics; no sum depends on the batch or on a slice's place in it.
#include "internal.h"
#include "coilmix_plan.h"

namespace pnp {

template <typename R, int NOUT, bool VEC>
__global__ __launch_bounds__(COILMIX_MIX_THREADS) void k_coil_mix(const typename CxOf<R>::type* __restrict__ in,
                                                                  const typename CxOf<R>::type* __restrict__ m,
                                                                  const int32_t* __restrict__ set_id, typename CxOf<R>::type* __restrict__ out,
                                                                  int C_in, int C_out, size_t N) {
    using C = typename CxOf<R>::type;
    constexpr int P = sizeof(R) == 8 ? 1 : 2;
    __shared__ C shM[COILMIX_MIX_CHUNK][NOUT];          // M^T: row cc holds M[0 .. NOUT)[c0 + cc], zero past C_out
    const int b = blockIdx.y;
    const int set = set_id ? set_id[b] : 0;
    const C* M = m + (size_t)set * C_out * C_in;
    const C* src = in + (size_t)b * C_in * N;
    const size_t p0 = ((size_t)blockIdx.x * COILMIX_MIX_THREADS + threadIdx.x) * P;
    R ar[NOUT][P], ai[NOUT][P];
#pragma unroll
    for (int j = 0; j < NOUT; ++j)
#pragma unroll
        for (int k = 0; k < P; ++k) { ar[j][k] = R(0); ai[j][k] = R(0); }

    for (int c0 = 0; c0 < C_in; c0 += COILMIX_MIX_CHUNK) {
        __syncthreads();                                 // the previous chunk has been read
        for (int idx = threadIdx.x; idx < COILMIX_MIX_CHUNK * NOUT; idx += COILMIX_MIX_THREADS) {
            const int j = idx / COILMIX_MIX_CHUNK, cc = idx % COILMIX_MIX_CHUNK;
            C v;
            v.x = R(0); v.y = R(0);
            if (j < C_out && c0 + cc < C_in) v = M[(size_t)j * C_in + c0 + cc];
            shM[cc][j] = v;
        }
        __syncthreads();
        const int nc = C_in - c0 < COILMIX_MIX_CHUNK ? C_in - c0 : COILMIX_MIX_CHUNK;
#pragma unroll 2
        for (int cc = 0; cc < nc; ++cc) {
            const C* row = src + (size_t)(c0 + cc) * N;
            C x[P];
#pragma unroll
            for (int k = 0; k < P; ++k) { x[k].x = R(0); x[k].y = R(0); }
            if constexpr (P == 2 && VEC) {               // N even, 16-byte aligned: one load of two points
                if (p0 < N) {
                    const float4 t = *reinterpret_cast<const float4*>(row + p0);
                    x[0].x = t.x; x[0].y = t.y; x[1].x = t.z; x[1].y = t.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < P; ++k) if (p0 + k < N) x[k] = row[p0 + k];
            }
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                const C mv = shM[cc][j];
#pragma unroll
                for (int k = 0; k < P; ++k) coilmix_cmac(ar[j][k], ai[j][k], mv.x, mv.y, x[k].x, x[k].y);
            }
        }
    }
    C* dst = out + (size_t)b * C_out * N;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        if (j >= C_out) break;
        C* row = dst + (size_t)j * N;
        if constexpr (P == 2 && VEC) {
            if (p0 < N) {
                float4 t;
                t.x = ar[j][0]; t.y = ai[j][0]; t.z = ar[j][1]; t.w = ai[j][1];
                *reinterpret_cast<float4*>(row + p0) = t;
            }
        } else {
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (p0 + k < N) { C v; v.x = ar[j][k]; v.y = ai[j][k]; row[p0 + k] = v; }
        }
    }
}

template <typename R>
__global__ __launch_bounds__(COILMIX_TILE * COILMIX_TILE) void k_coil_gram(const typename CxOf<R>::type* __restrict__ y,
                                                                           const uint8_t* __restrict__ mask_bank,
                                                                           const int32_t* __restrict__ mask_id, double2* __restrict__ gram,
                                                                           int Cn, int H, int W, int ncal) {
    using C = typename CxOf<R>::type;
    constexpr int T = COILMIX_TILE, Q = COILMIX_GRAM_POINTS, THREADS = T * T;
    __shared__ double2 sh[Q][2 * T];                     // point qq: the tile's T row coils, then its T column coils
    __shared__ uint8_t shm[Q];
    const int b = blockIdx.y;
    int bi, bj;
    coilmix_tile_of(blockIdx.x, Cn, bi, bj);
    const int ti = threadIdx.x / T, tj = threadIdx.x % T;
    const int i = bi * T + ti, j = bj * T + tj;
    const size_t N = (size_t)H * W;
    const uint8_t* mask = mask_bank + (size_t)(mask_id ? mask_id[b] : 0) * N;
    const C* ys = y + (size_t)b * Cn * N;
    const int npts = coilmix_cal_points(ncal);
    double re = 0.0, im = 0.0;
    for (int q0 = 0; q0 < npts; q0 += Q) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < Q * 2 * T; idx += THREADS) {
            const int cl = idx / Q, qq = idx % Q, q = q0 + qq;
            const int coil = cl < T ? bi * T + cl : bj * T + cl - T;
            double2 v;
            v.x = 0.0; v.y = 0.0;
            if (q < npts && coil < Cn) {
                const C t = ys[(size_t)coil * N + coilmix_cal_index(q, ncal, H, W)];
                v.x = (double)t.x; v.y = (double)t.y;
            }
            sh[qq][cl] = v;
        }
        if ((int)threadIdx.x < Q) shm[threadIdx.x] = q0 + (int)threadIdx.x < npts ? mask[coilmix_cal_index(q0 + threadIdx.x, ncal, H, W)] : 0;
        __syncthreads();
        const int nq = npts - q0 < Q ? npts - q0 : Q;
        for (int qq = 0; qq < nq; ++qq) {
            if (!shm[qq]) continue;                      // the same for every thread of the workgroup
            const double2 a = sh[qq][ti], c = sh[qq][T + tj];
            coilmix_gram_step(re, im, a.x, a.y, c.x, c.y);
        }
    }
    if (i < Cn && j < Cn && i <= j) {
        if (i == j) im = 0.0;
        double2 v, vc;
        v.x = re; v.y = im; vc.x = re; vc.y = -im;
        gram[coilmix_gram_index(b, i, j, Cn)] = v;
        gram[coilmix_gram_index(b, j, i, Cn)] = vc;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
template <typename R, bool VEC>
static void mix_bucket(hipStream_t s, dim3 grid, const typename CxOf<R>::type* in, const typename CxOf<R>::type* m, const int32_t* set_id,
                       typename CxOf<R>::type* out, int C_in, int C_out, size_t N) {
    const dim3 blk(COILMIX_MIX_THREADS);
    switch (coilmix_out_bucket(C_out)) {
    case 4:  hipLaunchKernelGGL((k_coil_mix<R, 4, VEC>), grid, blk, 0, s, in, m, set_id, out, C_in, C_out, N); break;
    case 8:  hipLaunchKernelGGL((k_coil_mix<R, 8, VEC>), grid, blk, 0, s, in, m, set_id, out, C_in, C_out, N); break;
    case 16: hipLaunchKernelGGL((k_coil_mix<R, 16, VEC>), grid, blk, 0, s, in, m, set_id, out, C_in, C_out, N); break;
    default: hipLaunchKernelGGL((k_coil_mix<R, 32, VEC>), grid, blk, 0, s, in, m, set_id, out, C_in, C_out, N); break;
    }
}

// the caller has checked coilmix's argument rule, the grid limits and that in / out do not overlap
template <typename R>
hipError_t launch_coil_mix(hipStream_t s, const R* in, const R* m, const int32_t* set_id, R* out, int B, int C_in, int C_out, size_t N) {
    using C = typename CxOf<R>::type;
    const bool f64 = sizeof(R) == 8;
    const dim3 grid((unsigned)coilmix_mix_blocks(N, f64), (unsigned)B);
    // two points per 16-byte access need every row to start on a 16-byte boundary: N even and both arrays aligned
    const bool vec = !f64 && N % 2 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (vec) mix_bucket<R, true>(s, grid, (const C*)in, (const C*)m, set_id, (C*)out, C_in, C_out, N);
    else     mix_bucket<R, false>(s, grid, (const C*)in, (const C*)m, set_id, (C*)out, C_in, C_out, N);
    return hipGetLastError();
}

template <typename R>
hipError_t launch_coil_gram(hipStream_t s, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int Cn,
                            int H, int W, int ncal) {
    using C = typename CxOf<R>::type;
    hipLaunchKernelGGL(k_coil_gram<R>, dim3((unsigned)coilmix_tile_pairs(Cn), (unsigned)B), dim3(COILMIX_TILE * COILMIX_TILE), 0, s,
                       (const C*)y, mask_bank, mask_id, (double2*)gram, Cn, H, W, ncal);
    return hipGetLastError();
}

#define COILMIX_INST(R)                                                                                                          \
    template hipError_t launch_coil_mix<R>(hipStream_t, const R*, const R*, const int32_t*, R*, int, int, int, size_t);         \
    template hipError_t launch_coil_gram<R>(hipStream_t, const R*, const uint8_t*, const int32_t*, double*, int, int, int, int, int);
COILMIX_INST(float)
COILMIX_INST(double)
#undef COILMIX_INST

}  // namespace pnp
