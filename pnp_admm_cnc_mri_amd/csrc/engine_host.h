// Host machinery of the fast engines (kernels_fused256.hip, kernels_fused512.hip, kernels_slice256.hip): the side queues, the
// walk over a plan's parts (loop_schedule.h), the two-launch iteration chain and the twiddle-table upload.
#pragma once
#include "internal.h"
#include "fused_pointwise.h"
#include <math.h>
#include <vector>

namespace pnp {

// The side queues of an engine: created on its first run that needs them, destroyed with the engine.
struct SideQueues {
    hipStream_t side[kMaxQueues - 1] = {};
    hipEvent_t fork = nullptr, join[kMaxQueues - 1] = {};
    SideQueues() = default;
    SideQueues(const SideQueues&) = delete;
    SideQueues& operator=(const SideQueues&) = delete;
    ~SideQueues() {
        for (int q = 0; q < kMaxQueues - 1; ++q) {
            if (side[q]) (void)hipStreamDestroy(side[q]);
            if (join[q]) (void)hipEventDestroy(join[q]);
        }
        if (fork) (void)hipEventDestroy(fork);
    }
};

// Enqueues the parts of a plan: run_part(stream, part) for each, queue 0 being the caller's stream s.  With side queues they
// start after what s holds so far (fork), and s goes on after all of them (join).
template <typename F>
hipError_t run_parts(SideQueues& sq, hipStream_t s, const LoopPlan& plan, int B, F&& run_part) {
    const int nside = plan.queues - 1;
    hipError_t e = hipSuccess;
    if (nside > 0) {
        if (!sq.fork) e = hipEventCreateWithFlags(&sq.fork, hipEventDisableTiming);
        for (int q = 0; q < nside && e == hipSuccess; ++q) {
            if (!sq.side[q]) e = hipStreamCreateWithFlags(&sq.side[q], hipStreamNonBlocking);
            if (e == hipSuccess && !sq.join[q]) e = hipEventCreateWithFlags(&sq.join[q], hipEventDisableTiming);
        }
        if (e == hipSuccess) e = hipEventRecord(sq.fork, s);
        for (int q = 0; q < nside && e == hipSuccess; ++q) e = hipStreamWaitEvent(sq.side[q], sq.fork, 0);
    }
    for (int i = 0; i < plan.parts && e == hipSuccess; ++i) {
        const Part p = plan_part(plan, B, i);
        if (p.count > 0) e = run_part(p.queue ? sq.side[p.queue - 1] : s, p);
    }
    for (int q = 0; q < nside && e == hipSuccess; ++q) {
        e = hipEventRecord(sq.join[q], sq.side[q]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, sq.join[q], 0);
    }
    return e;
}

// The template arguments <HAS_INV, PROX, HAS_FWD, WRITE_X> of the row kernels (k_frows, k5_rows, k_fmixed) as a tag type.
template <bool INV, int PROX, bool FWD, bool X>
struct RowKind {
    static constexpr bool inv = INV, fwd = FWD, write_x = X;
    static constexpr int prox = PROX;
};

// Stages of the row launches: first (forward transform only), mid (inverse, z / w update, forward), last (inverse, update, x).
enum class Stage { first, mid, last };

// Calls f(RowKind<...>{}) for a run-time (stage, prox).  prox 0 (no update) exists in the last stage only, and only WITH_DC:
// k_fmixed has no such variant.  These are all the instantiations there are.
template <bool WITH_DC = true, typename F>
hipError_t with_row_kind(Stage st, int prox, F&& f) {
    if (st == Stage::first) return f(RowKind<false, 0, true, false>{});
    const bool last = st == Stage::last;
    if (prox == 2) return last ? f(RowKind<true, 2, false, true>{}) : f(RowKind<true, 2, true, false>{});
    if (prox == 1) return last ? f(RowKind<true, 1, false, true>{}) : f(RowKind<true, 1, true, false>{});
    if (prox == 3) return last ? f(RowKind<true, 3, false, true>{}) : f(RowKind<true, 3, true, false>{});
    if constexpr (WITH_DC) if (prox == 0 && last) return f(RowKind<true, 0, false, true>{});
    return hipErrorInvalidValue;
}

// Row arguments of the slices [c0, c0 + Bc) of a two-launch engine E (field E::T, E::N = H W complex values per slice pair).
// zo / wo null: z and w are only read (a data-consistency step).
template <typename E, typename R>
FRowArgsT<R> chain_row_args(const E* f, const R* z, const R* w, R* zo, R* wo, R* x, int c0, int Bc, const ProxParamsT<R>& pp) {
    const size_t so = (size_t)c0 * E::N;
    FRowArgsT<R> a;
    a.T = f->T + (size_t)(c0 / 2) * E::N;
    a.z_in = z + so; a.w_in = w + so;
    a.z_out = zo ? zo + so : nullptr; a.w_out = wo ? wo + so : nullptr;
    a.x_out = x + so; a.B = Bc;
    a.scale = (R)(1.0 / (double)E::N); a.prox = pp; a.u_first = 1;
    return a;
}

// The iteration chain of a two-launch engine on one part of the batch: forward rows, then per iteration the columns and the
// rows of the mid stage, or of the last stage on the final iteration.  E supplies rows(RowKind, s, pairs, args) and
// cols(s, pair0, pairs, c) for `pairs` slice pairs.  One iteration at prox 0 is one data-consistency step.
template <typename E, typename R>
hipError_t chain_part(const E* f, hipStream_t s, FRowArgsT<R> a, int c0, int Bc, int iters, int prox, R c) {
    const int np = (Bc + 1) / 2, pair0 = c0 / 2;
    auto rows = [&](auto k) { return f->rows(k, s, np, a); };
    hipError_t e = with_row_kind(Stage::first, prox, rows);
    for (int i = 0; i < iters && e == hipSuccess; ++i) {
        e = f->cols(s, pair0, np, c);
        a.u_first = (i == 0);
        if (e == hipSuccess) e = with_row_kind(i == iters - 1 ? Stage::last : Stage::mid, prox, rows);
    }
    return e;
}

// A whole run of a two-launch engine by a plan of loop_schedule.h, and one data-consistency step on caller pointers.
template <typename E, typename R>
hipError_t chain_run(E* f, hipStream_t s, R* z, R* w, R* x, int B, int iters, int prox, R c, const ProxParamsT<R>& pp,
                     const LoopPlan& plan) {
    if (iters <= 0) return hipSuccess;
    return run_parts(f->queues, s, plan, B, [&](hipStream_t sq, const Part& p) {
        return chain_part(f, sq, chain_row_args(f, z, w, z, w, x, p.first, p.count, pp), p.first, p.count, iters, prox, c);
    });
}
template <typename E, typename R>
hipError_t chain_dc(const E* f, hipStream_t s, const R* z, const R* w, R* x, int B, R c) {
    return chain_part(f, s, chain_row_args<E, R>(f, z, w, nullptr, nullptr, x, 0, B, ProxParamsT<R>{}), 0, B, 1, 0, c);
}

// One step of a run whose chain the caller drives itself (the convergence trace, api.hip): the whole batch on one stream, the launches
// of chain_part one by one -- open = the forward rows that start a run, cols = the column launch of an iteration, mid / last = its row
// launch in the mid or the last stage -- plus what a trace needs: a LAST-stage row launch writes z, w, x wherever zo, wo, x point and
// leaves the transform buffer and its inputs alone, so between the columns and the mid-stage rows of an iteration it materialises
// the state of that iteration beside a chain that goes on unbroken.  The launches on the data are those of the uncut run.
template <typename E, typename R>
hipError_t chain_step(const E* f, hipStream_t s, ChainStep st, const R* z, const R* w, R* zo, R* wo, R* x, int B, int prox, R c,
                      const ProxParamsT<R>& pp, bool u_first) {
    const int np = (B + 1) / 2;
    if (st == ChainStep::cols) return f->cols(s, 0, np, c);
    FRowArgsT<R> a = chain_row_args(f, z, w, zo, wo, x, 0, B, pp);
    a.u_first = u_first;
    return with_row_kind(st == ChainStep::open ? Stage::first : st == ChainStep::mid ? Stage::mid : Stage::last, prox,
                         [&](auto k) { return f->rows(k, s, np, a); });
}

// W_n^m = exp(-2 pi i m / n), m in [0, n): computed in double, rounded once to R, copied to the __device__ table `symbol`
template <typename R>
hipError_t upload_twiddle_table(const void* symbol, int n) {
    std::vector<cxT<R>> h(n);
    for (int m = 0; m < n; ++m) {
        const double a = -2.0 * M_PI * (double)m / (double)n;
        h[m] = mk<R>((R)cos(a), (R)sin(a));
    }
    return hipMemcpyToSymbol(symbol, h.data(), (size_t)n * sizeof(cxT<R>));
}

}  // namespace pnp
