// How the fast ADMM loops spread a batch of B slices over HIP queues and launches: one plan per engine kind, and the parts of
// the batch a plan runs.  Pure host code without HIP: the engines run by these plans, pnp_get_plan (api.hip) reports them, and
// tests/host/loop_schedule_emulation.cpp checks them under g++.  Scheduling only: results are bit-identical for every setting.
#pragma once

namespace pnp {

constexpr int kMaxQueues = 4;       // HIP queues of one run: the caller's and at most 3 side queues

// How the fused loops are scheduled (defaults overridable by PNP_FUSED_* at pnp_ctx_create / pnp_set_schedule).
struct FusedSchedule {
    int queues = 2;         // HIP queues the batch is split over (1..4); kernel heads/tails overlap
    int mixed = 0;          // 256x256: row workgroups of one half + column workgroups of the other per launch (k_fmixed)
    int chunk = 0;          // >0: a queue finishes all iterations on `chunk` slices before its next chunk; 0: the path's default
                            // (plan_chunked below); <0: off (whole batch / two halves)
    int l1_two_state = 0;   // test hook: ADMM_L1 keeps z and w every iteration instead of u only
    // Experiment knobs.  They stay at these defaults unless the library is built with -DPNP_EXPERIMENT_KNOBS (profiles/variants.sh
    // does); such a build reads them from the environment ONCE, at pnp_ctx_create (api.hip, read_knobs), range-checked.
    int chunk_queues = 0;   // >0: queues of the chunked schedules           (PNP_F512_QUEUES / PNP_F256S_QUEUES)
    int slice_xor = 0;      // slice <-> workgroup permutation b ^ xor          (PNP_SLICE_XOR)
    int slice_queues = 1;   // slice-resident run cut over HIP queues ...       (PNP_SLICE_QUEUES)
    int slice_segment = 0;  // ... and into launches of this many iterations    (PNP_SLICE_SEGMENT)
    int slice_flip = 1;     // every other multi-round call walks the batch backwards (PNP_SLICE_FLIP)
};

// The z / w update a run applies: 1 ADMM_L1 in two-state form, 2 ADMM_CNC, 3 ADMM_L1 in single-state form (fused_pointwise.h);
// 0, no update, is the data-consistency step alone (the *_dc functions).
inline int prox_kind(bool cnc, const FusedSchedule& sch) { return cnc ? 2 : (sch.l1_two_state ? 1 : 3); }

// The schedule of one run: the batch runs as `parts` parts of `part` slices (the last part takes the rest), part i on queue
// i % queues; a queue runs all iterations of a part before its next part.
struct LoopPlan {
    int queues;     // HIP queues (1: the caller's queue alone)
    int chunk;      // slices per sequential chunk, as pnp_get_plan reports it (B: one chunk)
    int launches;   // kernel launches per iteration (0: the iterations loop inside one launch)
    bool mixed;     // parts of at least 64 slices take the staggered mixed launches (fused256: k_fmixed)
    int parts, part;
};

struct Part { int first, count, queue; };
inline Part plan_part(const LoopPlan& p, int B, int i) {
    const int first = i * p.part;
    return {first, i == p.parts - 1 ? B - first : p.part, i % p.queues};
}
inline bool takes_mixed(const LoopPlan& p, const Part& q) { return p.mixed && q.count >= 64; }

// 256x256, two launches per iteration (fused256_run).  Slices are independent, so the K-iteration chains of different parts of
// the batch may run on different queues, share launches (run_mixed) or run one chunk after another (chunk*(z,w,T,Yh) <= the
// 256 MiB Infinity Cache keeps a chunk's working set on die; measured +-2 %).  Parts over queues are even-sized.
inline LoopPlan plan_fused256(int B, const FusedSchedule& sch) {
    const int queues = sch.queues < 1 ? 1 : (sch.queues > kMaxQueues ? kMaxQueues : sch.queues);
    if (sch.chunk > 0) {                                                  // one queue, one chunk after another
        const int chunk = (sch.chunk & ~1) < 2 ? 2 : (sch.chunk & ~1);
        if (chunk < B) {
            const int n = (B + chunk - 1) / chunk;
            return {1, chunk, 2 * n, false, n, chunk};
        }
        return {1, B, 2, false, 1, B};
    }
    if (queues >= 2 && B >= 32 * queues) return {queues, B, 2 * queues, sch.mixed != 0, queues, ((B / queues) + 1) & ~1};
    return {1, B, 2, queues == 1 && sch.mixed != 0, 1, B};
}

// Chunked schedules of the 512x512 loops and of the split-chain 256x256 loops: a queue runs ALL iterations of a run on
// `chunk` slices before its next chunk, and the chunks go round-robin to Q queues -- Q chunks in flight, whose working set
// (Q * chunk * 4 MiB at 512x512, * 2.5 MiB in double) stays around the 256 MiB Infinity Cache and whose kernel tails overlap
// each other's heads.  Measured on one box each (it/s; profiles/bench_r02):
//   512x512, 256 slices: whole batch 1057-1171 (a slow mode on some boxes), 1 x 48: 1161-1172, 2 x 32: 1338, 3 x 24: 1360,
//                        4 x 16: 1358, 4 x 24: 1361, 4 x 8: 1244
//   double, 512 slices:  two halves on two queues 2186-2400, 1 x 96: 2423, 2 x 48: 2563, 3 x 32: 2570, 4 x 24: 2573, 4 x 64: 2436
// sch.chunk < 0 (PNP_FUSED_CHUNK=-1): the whole batch, or at 256x256 two halves on two queues (the round-1 schedule);
// sch.chunk_queues overrides the number of queues (experiment builds).  The split chain in float has no default chunk.
enum class Chunked { split_f32, split_f64, fused512 };
inline LoopPlan plan_chunked(int B, const FusedSchedule& sch, Chunked kind) {
    const bool is512 = kind == Chunked::fused512;
    int queues = sch.chunk_queues > 0 ? sch.chunk_queues : (sch.queues >= 2 ? 4 : 1);
    if (queues > kMaxQueues) queues = kMaxQueues;
    const int dflt = is512 ? (queues >= 2 ? 16 : 48) : (kind == Chunked::split_f64 ? (queues >= 2 ? 24 : 96) : 0);
    int chunk = sch.chunk != 0 ? sch.chunk : dflt;
    if (chunk <= 0) {                                                     // off
        if (!is512 && sch.queues >= 2 && B >= 64) { queues = 2; chunk = ((B / 2) + 1) & ~1; }     // two halves (round 1)
        else { queues = 1; chunk = B; }
    }
    chunk &= ~1;
    if (chunk < 2) chunk = 2;
    if (chunk >= B) { chunk = B > 2 ? ((B + 1) & ~1) : 2; queues = 1; }
    const int n = (B + chunk - 1) / chunk;
    const int part = chunk < B ? chunk : B;
    return {queues, part, 2 * n, false, n, part};
}

// Slice-resident 256x256 loops (slice256_run): one launch per run, or -- experiment knob slice_queues -- parts of B / q slices
// on q queues when every part has at least 64 slices.
inline LoopPlan plan_slice(int B, const FusedSchedule& sch) {
    int queues = sch.slice_queues < 1 ? 1 : (sch.slice_queues > kMaxQueues ? kMaxQueues : sch.slice_queues);
    if (B < 64 * queues) queues = 1;
    return {queues, B, 0, false, queues, B / queues};
}

}  // namespace pnp
