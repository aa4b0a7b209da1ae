// Convergence trace of the ADMM loops (pnp_admm_*_run_traced, pnp_residuals): which iterations are checked, how a traced run
// is cut into launches, and the shape of the reduction kernel (kernels_trace.hip).  Pure host-callable code without HIP: the
// driver in api.hip runs by it and tests/host/trace_emulation.cpp checks it under g++.
//
// A check at iteration k (1-based, k completed iterations) needs the state of TWO launch boundaries: z of k - 1 (for
// r_dual = ||z_k - z_{k-1}||) and x, z, w of k.  The loops leave the complete (z, w) in memory only at the end of a launch,
// and a run split into launches is bit-identical to one launch, so check c becomes a LEG:
//     [launch of `pre` iterations]  ->  snapshot of z  ->  launch of ONE iteration  ->  reduction into trace row c
// with `pre` = the iterations between the previous check and k - 1 (0: no such launch; the snapshot is then taken right
// behind the previous check, or of the initial state).  The snapshot and the reduction are enqueued on the context's stream
// behind the join that ends a launch (engine_host.h, run_parts), never inside a run's chain.
// That is the slice-resident and the generic path.  The two-launch engines are not cut into legs: their run is a chain of launches whose
// transform buffer carries rounding state from iteration to iteration, so the chain runs on unbroken and the state of iterations k - 1
// and k is materialised beside it by a last-stage row launch (engine_host.h, chain_step; api.hip, run_traced_chain) -- at the same
// checked iterations (trace_checks / trace_check_iter).
#pragma once
#include <stddef.h>

namespace pnp {

// Checked iterations: every multiple of `every` that is <= iters, plus iters itself when it is not one.
constexpr int trace_checks(int iters, int every) {
    return (iters <= 0 || every < 1) ? 0 : iters / every + (iters % every != 0 ? 1 : 0);
}
// the iteration of check c = 0 .. trace_checks - 1
constexpr int trace_check_iter(int iters, int every, int c) {
    return (c + 1) * every <= iters ? (c + 1) * every : iters;
}

struct TraceLeg {
    int pre;    // iterations of the launch in front of the snapshot (0: none)
    int iter;   // the checked iteration: snapshot at iter - 1, one iteration, reduction
};
constexpr TraceLeg trace_leg(int iters, int every, int c) {
    const int k = trace_check_iter(iters, every, c), prev = c > 0 ? trace_check_iter(iters, every, c - 1) : 0;
    return {k - 1 - prev, k};
}

// ---- shape of the reduction ---------------------------------------------------------------------------------------------
// Sums of squares per slice, in this order, in the device trace buffer [check][TRACE_Q][B] (doubles):
enum { TR_XZ = 0, TR_ZZP = 1, TR_X = 2, TR_Z = 3, TR_W = 4, TR_E = 5, TR_G = 6, TRACE_Q = 7 };
//   sum (x - z)^2, sum (z - z_prev)^2, sum x^2, sum z^2, sum w^2, sum (255 x - gt)^2, sum gt^2   (the last two 0 without gt)

constexpr int TRACE_THREADS = 256;
constexpr int TRACE_TILE = 2048;          // elements of one block-wide step of the slice-order flavour: four row pairs (slice_layout.h)

// Workgroups per slice: about 1024 / B (at most 64), so that B = 1 .. 8 is spread over the card and B = 512 fills it with two
// workgroups per slice (measured at 512 slices: 3.7 TB/s; with four per slice 2.7 TB/s -- DESIGN.md section 11).  Functions of (B, N) alone -- the reduction tree, hence every bit of a row, is fixed by the shape of the batch.
constexpr int TRACE_MAX_GROUPS = 64, TRACE_TARGET_GROUPS = 1024;
// elements per workgroup: a multiple of TRACE_TILE (so of every vector width and of the slice-order tile)
constexpr size_t trace_span(int B, size_t N) {
    size_t g = (size_t)((TRACE_TARGET_GROUPS + B - 1) / B);
    if (g > (size_t)TRACE_MAX_GROUPS) g = TRACE_MAX_GROUPS;
    if (g < 1) g = 1;
    return ((N + g - 1) / g + TRACE_TILE - 1) / TRACE_TILE * TRACE_TILE;
}
constexpr int trace_groups(int B, size_t N) { return (int)((N + trace_span(B, N) - 1) / trace_span(B, N)); }

}  // namespace pnp
