// Multi-coil (SENSE) data consistency (pnp_set_coils; kernels_coils.hip, the coil row roles of kernels_anysize.hip): the index maps of the
// coil arrays and the order of every sum of the batched conjugate-gradient x-step.  Pure host-callable code without HIP: the kernels and
// the driver in api.hip run by it and tests/host/coil_emulation.cpp checks it under g++.
//
// Arrays (complex in the context's precision unless said otherwise):
//   maps   [Ks][C][H][W]   a bank of Ks coil sets; slice b uses set coil_id[b] (null: set 0)
//   work   [B][C][H][W]    coil images / coil k-space of the batch: B * C pseudo-slices for the column kernels, whose mask index
//                          is that of slice s / C (the expanded mask_id, written once per upload)
//   x^, r, p, Gp, aty      [B][H][W]
// Sums (all in double): one application of G leaves one partial of Re<p, Gp> per image ROW (the row kernel sums a row of W products:
// lane l of a 64-lane wave takes k = l, l + 64, ... in order, then a butterfly of xor distances 32 .. 1); the pointwise CG kernels leave
// one partial of <r, r> per workgroup of CG_SPAN elements (thread t takes t, t + 256, ... in order, then cg_tree_sum's tree over the 256
// threads).  A slice's H resp. cg_blocks(N) partials are then summed by cg_tree_sum again.  Every order is a function of (H, W) alone:
// never of B, of the slice's position in the batch, or of the coil count (the coils are accumulated in order c = 0 .. C - 1 per pixel).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define COIL_HD __host__ __device__
#else
#define COIL_HD
#endif

namespace pnp {

constexpr int COIL_MAX_C = 32;            // pnp_coils_check: 1 <= C <= COIL_MAX_C
constexpr int CG_MAX_ITERS = 64;          // pnp_set_cg: 1 <= iters <= CG_MAX_ITERS
constexpr int CG_THREADS = 256;
constexpr int CG_SPAN = 1024;             // elements of one slice per workgroup of the pointwise CG kernels (4 per thread)

enum { COIL_OK = 0, COIL_BAD_C = 1, COIL_BAD_SETS = 2, COIL_BAD_SHAPE = 3 };
COIL_HD inline int coil_check(int C, int Ks, int H, int W) {
    if (C < 1 || C > COIL_MAX_C) return COIL_BAD_C;
    if (Ks < 1) return COIL_BAD_SETS;
    if (H < 128 || H > 1024 || W < 128 || W > 1024) return COIL_BAD_SHAPE;
    return COIL_OK;
}

// ---- index maps ----------------------------------------------------------------------------------------------------------------
// element (h, k) of coil c of slice b in the work array, and of coil c of set `set` in the maps
COIL_HD inline size_t coil_work_index(int b, int c, int C, int h, int k, int H, int W) {
    return (((size_t)b * C + c) * H + h) * W + k;
}
COIL_HD inline size_t coil_map_index(int set, int c, int C, int h, int k, int H, int W) {
    return (((size_t)set * C + c) * H + h) * W + k;
}
COIL_HD inline int coil_set_of(const int32_t* coil_id, int b) { return coil_id ? coil_id[b] : 0; }
// row `row` of the [B][H] rows of the batch -> slice and row inside it
COIL_HD inline int coil_row_slice(int row, int H) { return row / H; }
COIL_HD inline int coil_row_line(int row, int H) { return row % H; }
// the mask index of pseudo-slice s of the B * C the column kernels see: that of slice s / C
COIL_HD inline int coil_pseudo_slice(int s, int C) { return s / C; }

// elements of the work array / the maps; 0 when the count does not fit a size_t (never on a 64-bit host; kept for the emulation)
COIL_HD inline size_t coil_work_elems(int B, int C, int H, int W) { return (size_t)B * C * H * W; }
COIL_HD inline size_t coil_map_elems(int Ks, int C, int H, int W) { return (size_t)Ks * C * H * W; }

// ---- sums ----------------------------------------------------------------------------------------------------------------------
// partials per slice: of Re<p, Gp> (one per row) and of <r, r> (one per pointwise workgroup)
COIL_HD inline int cg_row_partials(int H) { return H; }
COIL_HD inline int cg_blocks(size_t N) { return (int)((N + CG_SPAN - 1) / CG_SPAN); }
// partials array of the batch: [B][cg_row_partials] resp. [B][cg_blocks]
COIL_HD inline size_t cg_partial_index(int b, int i, int per_slice) { return (size_t)b * per_slice + i; }

// The sum of v[0 .. n) as 256 threads form it: thread t adds v[t], v[t + 256], ... in order, then a tree over the threads with
// strides 128, 64, .. 1 (a[t] += a[t + s] for t < s).  The device code (kernels_coils.hip, block_sum) does exactly this in parallel.
COIL_HD inline double cg_tree_sum(const double* v, int n) {
    double a[CG_THREADS];
    for (int t = 0; t < CG_THREADS; ++t) {
        double s = 0.0;
        for (int i = t; i < n; i += CG_THREADS) s += v[i];
        a[t] = s;
    }
    for (int s = CG_THREADS / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; ++t) a[t] += a[t + s];
    return a[0];
}
// the sum of one row's W products as one 64-lane wave forms it (the coil row epilogue)
COIL_HD inline double cg_wave_sum(const double* v, int n) {
    double a[64];
    for (int l = 0; l < 64; ++l) {
        double s = 0.0;
        for (int i = l; i < n; i += 64) s += v[i];
        a[l] = s;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        double b[64];
        for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ d];
        for (int l = 0; l < 64; ++l) a[l] = b[l];
    }
    return a[0];
}
// alpha = rr / pGp and beta = rr_new / rr: a zero (or non-finite-making) denominator gives 0, never a NaN -- with one coil of uniform
// sensitivity the first iteration already converges and the second divides 0 by 0
COIL_HD inline double cg_ratio(double num, double den) {
    if (den == 0.0) return 0.0;
    const double q = num / den;
    return q - q == 0.0 ? q : 0.0;          // q - q is 0 exactly for a finite q, NaN for an infinite or NaN one
}

// launches of one x-step with `iters` CG iterations: v -> x^ (1), G v (3), r0 / p0 (1), per iteration G p (3) and the x^ / r update (1),
// between iterations the p update (iters - 1), the residual (1); and of a whole coil iteration with the pixel (1) or wavelet (2) prox
COIL_HD inline int cg_launches(int iters) { return 5 + 5 * iters; }
COIL_HD inline int coil_iteration_launches(int iters, bool wavelet) { return cg_launches(iters) + (wavelet ? 2 : 1); }

}  // namespace pnp
