// C ABI of libpnpmri.so (include/pnp_mri.h): context, problem upload, whole ADMM loops, step-wise
// operators.  (The denoisers' conv layers: api_conv.hip.)  Host-side only; the kernels live in the kernels_*.hip files.
#include "../../include/pnp_mri.h"
#include "internal.h"
#include "wavelet_plan.h"
#include "temporal_plan.h"
#include "lowrank_plan.h"
#include "coil_plan.h"
#include "coilmix_plan.h"
#include "coilmaps_plan.h"
#include "espirit_plan.h"

#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dlfcn.h>
#include <chrono>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

using namespace pnp;

static thread_local char g_err[512] = "";

int pnp::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// roctx ranges around the loops so that rocprofv3 --marker-trace output is self-describing.  The
// marker library is looked up at run time (it is part of the ROCm image, not a link dependency);
// without it the ranges are no-ops.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            void* h = dlopen(name, RTLD_LAZY | RTLD_LOCAL);
            if (!h) continue;
            push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
struct Range {
    static Roctx& api() { static Roctx r; return r; }
    explicit Range(const char* name) { if (api().push) api().push(name); }
    ~Range() { if (api().pop) api().pop(); }
};
}  // namespace

// The context's fast path, chosen at creation by shape, precision and PNP_FUSED_COLS, and beside it the slice-resident add-on of the
// 256x256 float engine.  No engine (512x512 double, H != W, any other size): the generic kernels only.
struct Engine {
    enum Kind { none, fused256, split_f32, split_f64, fused512 } kind = none;
    union {
        Fused256* f256 = nullptr;     // 256 x 256 float: two launches per iteration
        Fused256S<float>* s32;        // 256 x 256 "split chain" in float (PNP_FUSED_COLS=2) ...
        Fused256S<double>* s64;       // ... and in double: the fast path of an fp64 context
        Fused512* f512;               // 512 x 512 float
    };
    Slice256* slice = nullptr;        // fused256 only: whole loops slice-resident (pnp_dc_step stays on f256) ...
    int slice_min_b = 0;              // ... for batches at least this large
};

// Which kernels run the loops (pnp_admm_*_run) of the uploaded problem.
enum class Path { generic, slice, fused };

// What the uploaded problem has of its tables: reset by every upload / synthesize (begin_problem, finish_problem).
struct Problem {
    Path path = Path::generic;        // the loops' path with the fast path on (loop_path)
    bool fused_built = false;         // the engine's own tables (ensure_tables)
    bool slice_built = false;         // the slice-resident tables
};

// Convergence trace (trace_plan.h, kernels_trace.hip): the device buffers of the reduction and the host copy of the last traced run.
struct Trace {
    double* partial = nullptr;        // scratch of the reduction (trace_scratch_bytes)
    unsigned* counter = nullptr;      // [Bmax] ticket counters, zero between launches
    double* rows = nullptr;           // [rows_cap][TRACE_Q][Bmax] sums of squares, row c = check c
    int rows_cap = 0;
    void* zprev = nullptr;            // [Bmax][H][W] z of the iteration before a check (natural order; on first use)
    void *zc = nullptr, *wc = nullptr;  // two-launch engines: z, w of a checked iteration, materialised beside the running chain
    // what pnp_trace_read returns: the last traced run
    int B = 0;
    std::vector<int32_t> iters, converged_at;
    std::vector<double> values;       // [checks][TRACE_Q][B]: r_pri, r_dual, x_norm, z_norm, w_norm, psnr, re
};

// Multi-coil (SENSE) data consistency (pnp_set_coils; coil_plan.h): the maps, the coil arrays and the state of the batched CG x-step.
// C = 0: no coils -- the context is what it was.
struct Coils {
    int C = 0, Ks = 0, cg_iters = 3;
    void* maps = nullptr;             // [Ks][C][H][W] complex
    int32_t* coil_id = nullptr;       // [Bmax]
    int32_t* mask_idx = nullptr;      // [Bmax * C]: mask_id expanded to the pseudo-slices of the column kernels
    void* work = nullptr;             // [Bmax][C][H][W] complex: the coil transform intermediate
    void* ymc = nullptr;              // [Bmax][C][H][W] complex: the measurements (pnp_download_y)
    void *aty = nullptr, *xh = nullptr, *r = nullptr, *p = nullptr, *gp = nullptr;      // [Bmax][H][W] complex
    double *part_row = nullptr, *part_rr[2] = {nullptr, nullptr}, *part_bb = nullptr;   // [Bmax][H] resp. [Bmax][cg_blocks(N)]
    double *scal = nullptr, *rel = nullptr;                                             // [Bmax][4]: alpha, beta, <r,r>; [Bmax]
    bool have_rel = false;            // an x-step has run on the current problem
    AnySize* any = nullptr;           // the transforms of a coil context: the any-size kernels at every shape (the context's own, or made here)
    bool own_any = false;
};

// The three stage times of a coil-map estimator (pnp_*_stage_times): ms accumulates since the last read, the events exist once enabled.
struct StageTimer {
    bool on = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0.f, 0.f, 0.f};
};

struct pnp_ctx {
    int device = 0, H = 0, W = 0, Bmax = 0;
    int B = 0, K = 0;                 // current problem (0 = none uploaded)
    size_t N = 0;                     // H*W
    hipStream_t stream = nullptr;
    bool f64 = false;                 // fp64 validation context (pnp_ctx_create_f64): y, work, z, w, x hold doubles
    bool fast = true;
    bool have_x = false;
    bool have_state = false;         // z / w hold a defined state for the CURRENT problem: cleared by upload / synthesize, set by pnp_init_state or pnp_set_state(z, w)
    bool state_sliced = false;       // z / w are in the slice-resident kernel's order (slice_layout.h, sl_state_index)
    void* y = nullptr;                // [Bmax][H][W] complex, in the context's precision (bufs<R>)
    void* work = nullptr;             // [Bmax][H][W] complex transform intermediate
    // the state of the loops (state<R, CX>): real, and beside it the complex one of a coil context with complex-valued images
    void *z = nullptr, *w = nullptr, *x = nullptr;     // [Bmax][H][W] real
    int image = PNP_IMAGE_REAL;       // pnp_set_image; back to real, and the complex arrays freed, with the coils (coils_free)
    void *zc = nullptr, *wc = nullptr, *xc = nullptr;  // [Bmax][H][W] complex, allocated by pnp_set_image(PNP_IMAGE_COMPLEX)
    uint8_t* mask_bank = nullptr;     // [Kcap][H][W]
    int Kcap = 0;
    int32_t* mask_id = nullptr;       // [Bmax]
    uint8_t* gt = nullptr;            // [Bmax][H][W] (metrics, lazily)
    double* acc = nullptr;            // [Bmax][2]
    double* ssim_part = nullptr;      // [Bmax][tiles] (lazily)
    void* stage = nullptr;            // staging for host inputs of synthesize
    size_t stage_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Engine eng;
    AnySize* any = nullptr;           // H, W not both in {256, 512}: the row / column transforms run on the any-size kernels
    Problem prob;
    FusedSchedule sched;              // defaults overridable by PNP_FUSED_* (read at creation) / pnp_set_schedule
    Trace trace;
    int wavelet = WV_NONE, wv_levels = 0;   // pnp_set_sparsity: the prox of the loops acts on the coefficients of this transform
    void* wv_coef = nullptr;          // [Bmax][H][W] real: the coefficients between the two prox launches (on first use)
    void* wv_coef_cx = nullptr;       // [Bmax][H][W] complex: the same of the complex prox (by pnp_set_image / pnp_set_sparsity, whichever comes second)
    std::vector<int32_t> spin;        // pnp_set_spin: shifts[n][2] of the wavelet prox (empty: none) ...
    int spin_k = 1, spin_p = 0;       // ... per_prox of them a step, and the cursor: prox steps since it was last set
    void* wv_acc = nullptr;           // [Bmax][H][W] real: the sum of the shifts' z+ (by the first per_prox > 1)
    int tp_frames = 0;                // pnp_set_temporal: the prox acts on the temporal DFT of series of this many slices (0: none) ...
    bool tp_keep_dc = true;           // ... with coefficient 0 unpenalised
    void* tp_tw = nullptr;            // the twiddle matrix of tp_frames in the context's precision (tp_twiddle_matrix), room for TP_MAX_FRAMES
    int lr_block = 0;                 // pnp_set_lowrank: with tp_frames set, the prox thresholds the singular values of patches of this side (0: none) ...
    double lr_scale = 1.0;            // ... with thr and ib times this ...
    std::vector<int32_t> lr_shifts;   // ... on the grid anchored at shifts[n][2], one entry per prox step ...
    int lr_p = 0;                     // ... by the cursor: prox steps since it was last set
    Coils coils;
    void* maps_scratch = nullptr;     // the coil-map estimators' array, laid out by the call that runs (coilmaps_scratch, espirit_scratch); on first use
    size_t maps_bytes = 0;
    StageTimer cm_t;                  // pnp_coil_maps_stage_times: window, transform, eigenvectors + support; every pass is synchronised
    StageTimer es_t;                  // pnp_espirit_stage_times: patch Gram (with its read-back), host stage, per-pixel kernel with support
    std::vector<int32_t> es_rank;     // the signal-space rank of every slice of the most recent pnp_espirit_maps (pnp_espirit_ranks)
};

// The context's buffers as the element type of its precision (R = float | double).
template <typename R> struct Bufs {
    using C = typename CxOf<R>::type;
    C *y, *work;
    R *z, *w, *x;
};
template <typename R> static Bufs<R> bufs(const pnp_ctx* c) {
    using C = typename CxOf<R>::type;
    return {(C*)c->y, (C*)c->work, (R*)c->z, (R*)c->w, (R*)c->x};
}
// The state of the loops and the wavelet prox's coefficient array as their element type: R, or with CX (complex-valued images) the complex of R.
template <typename R, bool CX> struct State {
    CoilState<R, CX> *z, *w, *x, *wv_coef;
};
template <typename R, bool CX> static State<R, CX> state(const pnp_ctx* c) {
    using T = CoilState<R, CX>;
    if constexpr (CX) return {(T*)c->zc, (T*)c->wc, (T*)c->xc, (T*)c->wv_coef_cx};
    else return {(T*)c->z, (T*)c->w, (T*)c->x, (T*)c->wv_coef};
}
static bool cx_mode(const pnp_ctx* c) { return c->image == PNP_IMAGE_COMPLEX; }

static bool supported(int n) { return n == 256 || n == 512; }

// The row and column roles of the generic path: the fixed-size kernels for H, W in {256, 512}, the any-size kernels otherwise.
template <typename R> static hipError_t rows(const pnp_ctx* c, RowIn in, bool inv, RowEpi epi, const RowArgsT<R>& a) {
    return c->any ? anysize_rows<R>(c->any, c->stream, in, inv, epi, a) : launch_rows<R>(c->stream, c->W, in, inv, epi, a);
}
template <typename R> static hipError_t cols(const pnp_ctx* c, bool pre_fwd, ColMid mid, bool post_inv, const ColArgsT<R>& a) {
    return c->any ? anysize_cols<R>(c->any, c->stream, pre_fwd, mid, post_inv, a) : launch_cols<R>(c->stream, c->H, c->W, pre_fwd, mid, post_inv, a);
}

// Environment knobs: read ONCE per context (pnp_ctx_create), whole-string integers, range-checked -- a stray or mistyped
// variable fails the creation with PNP_E_ARG instead of silently changing which kernel a caller gets.
struct Knobs {
    int slice = -1;            // PNP_SLICE: 0 never, 1 always, unset: batches of at least slice_min_b slices
    int slice_min_b = 64;      // PNP_SLICE_MIN_B
    int slice_pad_kb = 4;      // PNP_SLICE_PAD_KB / PNP_SLICE_YH_PAD_KB: padding per slice of the slice path's own arrays
    int slice_yh_pad_kb = 4;
    int fused_cols = 1;        // PNP_FUSED_COLS: 2 = the split-chain column kernel in float
};
static int knob(const char* name, int lo, int hi, int* out) {
    const char* e = getenv(name);
    if (!e) return PNP_OK;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end != '\0' || v < lo || v > hi)
        return fail(PNP_E_ARG, "pnp_ctx_create: environment variable %s=\"%s\" is not an integer in [%d, %d]", name, e, lo, hi);
    *out = (int)v;
    return PNP_OK;
}
static int read_knobs(Knobs* k, FusedSchedule* sch) {
    int rc;
    if ((rc = knob("PNP_SLICE", 0, 1, &k->slice))) return rc;
    if ((rc = knob("PNP_SLICE_MIN_B", 1, 1 << 20, &k->slice_min_b))) return rc;
    if ((rc = knob("PNP_SLICE_PAD_KB", 0, 64, &k->slice_pad_kb))) return rc;
    if ((rc = knob("PNP_SLICE_YH_PAD_KB", 0, 64, &k->slice_yh_pad_kb))) return rc;
    if ((rc = knob("PNP_FUSED_COLS", 1, 2, &k->fused_cols))) return rc;
    if ((rc = knob("PNP_FUSED_STREAMS", 1, 4, &sch->queues))) return rc;
    if ((rc = knob("PNP_FUSED_SCHED", 0, 1, &sch->mixed))) return rc;
    if ((rc = knob("PNP_FUSED_CHUNK", -1, 1 << 20, &sch->chunk))) return rc;
    if ((rc = knob("PNP_FUSED_L1_TWO_STATE", 0, 1, &sch->l1_two_state))) return rc;     // test hook
#ifdef PNP_EXPERIMENT_KNOBS
    // A/B builds only (profiles/variants.sh): the product library does not look at these variables
    if ((rc = knob("PNP_F512_QUEUES", 1, 4, &sch->chunk_queues))) return rc;
    if ((rc = knob("PNP_F256S_QUEUES", 1, 4, &sch->chunk_queues))) return rc;
    if ((rc = knob("PNP_SLICE_XOR", 0, 1 << 20, &sch->slice_xor))) return rc;
    if ((rc = knob("PNP_SLICE_QUEUES", 1, 4, &sch->slice_queues))) return rc;
    if ((rc = knob("PNP_SLICE_SEGMENT", 0, 1 << 20, &sch->slice_segment))) return rc;
    if ((rc = knob("PNP_SLICE_FLIP", 0, 1, &sch->slice_flip))) return rc;
#endif
    return PNP_OK;
}

// the z / w update's scalars (internal.h, ProxParamsT): combined in double, rounded once to R
template <typename R> static ProxParamsT<R> prox_l1(double lambda1, double reo) { return {(R)(reo * lambda1)}; }
template <typename R> static ProxParamsT<R> prox_cnc(double alpha, double lambda1, double reo, double b) {
    return {(R)(alpha * reo * lambda1), (R)(1.0 - alpha), (R)alpha, (R)(alpha * reo * lambda1 * b), (R)(1.0 / b)};
}
template <typename R> static R dc_coeff(double reo) { return (R)(1.0 / (1.0 + 1.0 / 2.0 / reo)); }

#define CTX(c) do { if (!(c)) return fail(PNP_E_ARG, "%s: ctx is null", __func__); HIPCHK(hipSetDevice((c)->device)); } while (0)
#define NEED_PROBLEM(c) do { if ((c)->B <= 0) return fail(PNP_E_STATE, "%s: no problem uploaded", __func__); } while (0)
#define NEED_STATE(c) do { if (!(c)->have_state) return undefined_state(__func__); } while (0)
#define F32_ONLY(c) do { if ((c)->f64) return fail(PNP_E_STATE, "%s: not available on an fp64 validation context", __func__); } while (0)
#define F64_ONLY(c) do { if (!(c)->f64) return fail(PNP_E_STATE, "%s: needs a context made by pnp_ctx_create_f64", __func__); } while (0)

static int undefined_state(const char* who) {
    return fail(PNP_E_STATE, "%s: z / w are undefined since the last upload / synthesize (call pnp_init_state or pnp_set_state with both z and w)", who);
}

static int copy_in(pnp_ctx* c, void* dst, const void* src, size_t bytes, int on_device) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (!on_device) HIPCHK(hipStreamSynchronize(c->stream));   // caller may reuse its host buffer
    return PNP_OK;
}
static int copy_out(pnp_ctx* c, void* dst, const void* src, size_t bytes, int on_device) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!on_device) HIPCHK(hipStreamSynchronize(c->stream));
    return PNP_OK;
}

// hipMalloc with a report: on failure the HIP error is cleared, *p is null and the message names the array, the bytes asked for and the
// caller's sizes (`sizes`: printf-style, as in "Bmax=%d, %dx%d")
__attribute__((format(printf, 5, 6)))
static int alloc_or_fail(void** p, size_t bytes, const char* who, const char* what, const char* sizes, ...) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return PNP_OK;
    (void)hipGetLastError();
    *p = nullptr;
    char tail[128];
    va_list ap;
    va_start(ap, sizes);
    vsnprintf(tail, sizeof(tail), sizes, ap);
    va_end(ap);
    return fail(e == hipErrorOutOfMemory ? PNP_E_NOMEM : PNP_E_HIP, "%s: cannot allocate the %s: %zu bytes asked for (%s): %s", who, what, bytes, tail,
                hipGetErrorString(e));
}

// ---- the problem lifecycle: begin_problem, y written, finish_problem ----

// Drops the current problem and loads the masks of the next one.  A new problem invalidates the state (include/pnp_mri.h): z / w are
// UNDEFINED until pnp_init_state or pnp_set_state(z, w).  The order flag goes with it -- a conversion under the new B would read the
// slice path's padded arrays beyond the old batch.
static int begin_problem(pnp_ctx* c, const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device) {
    c->B = 0;
    c->prob = Problem{};
    c->state_sliced = c->have_x = c->have_state = false;
    if (!mask_bank) return fail(PNP_E_ARG, "mask_bank is null");
    if (B < 1 || B > c->Bmax) return fail(PNP_E_ARG, "B=%d out of range [1,%d]", B, c->Bmax);
    if (K < 1) return fail(PNP_E_ARG, "K must be >= 1");
    if (K > c->Kcap) {
        if (c->mask_bank) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->mask_bank)); c->mask_bank = nullptr; c->Kcap = 0; }
        HIPCHK(hipMalloc((void**)&c->mask_bank, (size_t)K * c->N));
        c->Kcap = K;
    }
    int rc = copy_in(c, c->mask_bank, mask_bank, (size_t)K * c->N, on_device);
    if (rc) return rc;
    if (mask_id) {
        // ids index the mask bank inside the kernels: validate them for host AND device inputs
        // (B int32 values; a device array is read back once -- problem upload is not the hot path)
        std::vector<int32_t> tmp;
        const int32_t* ids = mask_id;
        if (on_device) {
            tmp.resize((size_t)B);
            HIPCHK(hipMemcpyAsync(tmp.data(), mask_id, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            ids = tmp.data();
        }
        for (int i = 0; i < B; ++i) if (ids[i] < 0 || ids[i] >= K) return fail(PNP_E_ARG, "mask_id[%d]=%d out of range [0,%d)", i, ids[i], K);
        rc = copy_in(c, c->mask_id, mask_id, (size_t)B * sizeof(int32_t), on_device);
        if (rc) return rc;
    } else {
        HIPCHK(hipMemsetAsync(c->mask_id, 0, (size_t)B * sizeof(int32_t), c->stream));
    }
    c->B = B; c->K = K;
    return PNP_OK;
}

// One workgroup per slice, one workgroup per compute unit at a time: the batch runs in rounds of `cus` slices.
// Measured on MI355X, ms per iteration, two-launch vs slice-resident (profiles/run_slice_sizes.sh, one box each):
//   round 3 (profiles/slice_sizes_r03.txt):  B = 16: 0.0218 / 0.0289   32: 0.0253 / 0.0291   48: 0.0269 / 0.0302   56: 0.0290 / 0.0310
//                                            64: 0.0340 / 0.0309   96: 0.0437 / 0.0319
//   round 2:  B = 128: 0.0544 / 0.0405   256: 0.0954 / 0.0565   272: 0.1063 / 0.0904   320: 0.1224 / 0.0936   512: 0.1919 / 0.1075
// A round costs the same full or not, and even a nearly empty second round (B = 272) beats the two-launch path:
// the rule is simply "at least PNP_SLICE_MIN_B (64) slices" -- the crossover still sits between 56 and 64 with round 3's kernel.
static bool slice_pays(const pnp_ctx* c) { return c->B >= c->eng.slice_min_b; }

// The only place that builds per-problem tables, each set once per problem.  Path::fused: the engine's own tables -- built at upload,
// unless the slice path serves the loops of a 256x256 float problem: then on first use (pnp_dc_step always runs on them).
// Path::slice: the slice-resident tables (256 KiB per slice), built by the first slice loop or pnp_prepare_loops, so that the step-wise
// PnP solvers -- which only ever call pnp_dc_step on such a context -- never pay for them.
static int ensure_tables(pnp_ctx* c, Path path) {
    const float2* y = (const float2*)c->y;
    switch (path) {
    case Path::generic:
        return PNP_OK;
    case Path::slice:
        if (!c->prob.slice_built) HIPCHK(slice256_prepare(c->eng.slice, c->stream, y, c->mask_bank, c->mask_id, c->B));
        c->prob.slice_built = true;
        return PNP_OK;
    case Path::fused:
        if (c->prob.fused_built) return PNP_OK;
        switch (c->eng.kind) {
        case Engine::none:      return PNP_OK;
        case Engine::fused256:  HIPCHK(fused256_prepare(c->eng.f256, c->stream, y, c->mask_bank, c->mask_id, c->B)); break;
        case Engine::split_f32: HIPCHK(fused256s_prepare<float>(c->eng.s32, c->stream, c->y, c->mask_bank, c->mask_id, c->B)); break;
        case Engine::split_f64: HIPCHK(fused256s_prepare<double>(c->eng.s64, c->stream, c->y, c->mask_bank, c->mask_id, c->B)); break;
        case Engine::fused512:  HIPCHK(fused512_prepare(c->eng.f512, c->stream, y, c->mask_bank, c->mask_id, c->B)); break;
        }
        c->prob.fused_built = true;
        return PNP_OK;
    }
    return PNP_OK;
}

// Ends every upload / synthesize: decides the loops' path of the new problem and builds the tables that must exist now.  Any failure --
// rc from writing the problem, or a failed build -- leaves no problem behind: B = 0.
static int finish_problem(pnp_ctx* c, int rc) {
    if (rc == PNP_OK && c->eng.kind != Engine::none && c->coils.C == 0) {          // a coil context never enters the fast engines
        c->prob.path = (c->eng.slice && slice_pays(c)) ? Path::slice : Path::fused;
        if (c->prob.path == Path::fused) rc = ensure_tables(c, Path::fused);
    }
    if (rc != PNP_OK) { c->B = 0; c->prob = Problem{}; }
    return rc;
}

// The loops' path now: pnp_set_fast_path may change it after the upload.
static Path loop_path(const pnp_ctx* c) { return (c->fast && c->coils.C == 0) ? c->prob.path : Path::generic; }
// ... and where the data-consistency step alone runs (pnp_dc_step; the loops with a wavelet set): it has no slice-resident form
static Path dc_path(const pnp_ctx* c) { return loop_path(c) == Path::generic ? Path::generic : Path::fused; }

// The slice-resident loops keep z / w in their own order; everything else (the other kernel families, pnp_get_state /
// pnp_set_state, pnp_init_state) sees natural [H][W].  One kernel converts when the need changes (into the slice path's own
// padded arrays; in place with PNP_SLICE_PAD_KB=0).  The slice path is float only: a double state is always in natural order.
template <typename R> static int state_order(pnp_ctx* c, bool sliced) {
    if constexpr (std::is_same_v<R, double>) {
        return PNP_OK;
    } else {
        if (c->state_sliced == sliced) return PNP_OK;
        if (c->B > 0) {
            hipError_t e = slice256_state_order(c->eng.slice, c->stream, (float*)c->z, (float*)c->w, c->B, sliced);
            if (e != hipSuccess) return fail(PNP_E_HIP, "state order: %s", hipGetErrorString(e));
        }
        c->state_sliced = sliced;
        return PNP_OK;
    }
}

// ---- problem, state and loops: one body per precision, R = float | double ----

template <typename R>
static int upload_problem(pnp_ctx* c, const char* who, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, int B, int K,
                          int on_device) {
    if (!y) return fail(PNP_E_ARG, "%s: y is null", who);
    int rc = begin_problem(c, mask_bank, mask_id, B, K, on_device);
    if (rc == PNP_OK) rc = copy_in(c, c->y, y, (size_t)B * c->N * 2 * sizeof(R), on_device);
    return finish_problem(c, rc);
}

// y = fft2(img) * mask + noise (S4:102).  In double the reference's first fft2 runs on the float32 image in complex64 (NumPy >= 2) and
// is promoted by the float64 mask; here the float32 image is widened (exactly) and transformed in double, which is the nearer of the
// two to the exact transform -- the two y differ by NumPy's own complex64 round-off, ~1e-7.
template <typename R>
static int synthesize_y(pnp_ctx* c, const float* img, const R* noise, int noise_per_slice, int B, int on_device) {
    using C = typename CxOf<R>::type;
    const Bufs<R> b = bufs<R>(c);
    const size_t img_bytes = (size_t)B * c->N * sizeof(float);
    const size_t noise_bytes = (noise_per_slice ? (size_t)B : 1) * c->N * sizeof(C);
    const float* d_img = img;
    const C* d_noise = (const C*)noise;
    if (!on_device) {
        if (noise_bytes + img_bytes > c->stage_bytes) {
            if (c->stage) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->stage)); c->stage = nullptr; c->stage_bytes = 0; }
            HIPCHK(hipMalloc(&c->stage, noise_bytes + img_bytes));
            c->stage_bytes = noise_bytes + img_bytes;
        }
        d_noise = (const C*)c->stage;                                   // the complex noise first: alignment
        d_img = (const float*)((const char*)c->stage + noise_bytes);
        int rc = copy_in(c, (void*)d_noise, noise, noise_bytes, 0);
        if (rc == PNP_OK) rc = copy_in(c, (void*)d_img, img, img_bytes, 0);
        if (rc) return rc;
    }
    RowArgsT<R> ra{};
    if constexpr (std::is_same_v<R, double>) {
        HIPCHK(launch_widen(c->stream, d_img, b.x, (size_t)B * c->N));     // x is invalid until the next run anyway (have_x = false)
        ra.rin0 = b.x;
    } else {
        ra.rin0 = d_img;
    }
    ra.cout = b.y; ra.scale = 1; ra.nrows = B * c->H;
    HIPCHK(rows<R>(c, IN_REAL, false, EPI_COMPLEX, ra));
    ColArgsT<R> ca{};
    ca.in = b.y; ca.out = b.y; ca.y = d_noise; ca.mask_bank = c->mask_bank; ca.mask_id = c->mask_id;
    ca.y_per_slice = noise_per_slice; ca.B = B;
    HIPCHK(cols<R>(c, true, MID_MASK_ADD, false, ca));
    return PNP_OK;
}

template <typename R>
static int synthesize_problem(pnp_ctx* c, const char* who, const float* img, const R* noise, int noise_per_slice,
                              const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device) {
    if (!img || !noise) return fail(PNP_E_ARG, "%s: img/noise is null", who);
    int rc = begin_problem(c, mask_bank, mask_id, B, K, on_device);
    if (rc == PNP_OK) rc = synthesize_y<R>(c, img, noise, noise_per_slice, B, on_device);
    return finish_problem(c, rc);
}

template <typename R> static int download_y(pnp_ctx* c, const char* who, R* y, int on_device) {
    if (!y) return fail(PNP_E_ARG, "%s: null", who);
    if (c->coils.C > 0) return copy_out(c, y, c->coils.ymc, (size_t)c->B * c->coils.C * c->N * 2 * sizeof(R), on_device);      // [B][C][H][W]
    return copy_out(c, y, c->y, (size_t)c->B * c->N * 2 * sizeof(R), on_device);
}

// The state surface (pnp_set_state / pnp_get_state / pnp_download_x and their _cx forms) on the arrays of state<R, CX>; the caller's arrays
// are R (CX: interleaved).  A coil context never holds a sliced state, so state_order does nothing there.
template <typename R, bool CX = false> static int download_x(pnp_ctx* c, const char* who, R* x, int on_device) {
    const State<R, CX> s = state<R, CX>(c);
    if (!x) return fail(PNP_E_ARG, "%s: null", who);
    if (!c->have_x) return fail(PNP_E_STATE, "%s: no iteration has been run since the state was set", who);
    return copy_out(c, x, s.x, (size_t)c->B * c->N * sizeof(*s.x), on_device);
}

// the initial state of a coil context: z = |A^H y| (CX: A^H y itself, no modulus), w = 0
template <typename R, bool CX> static int coil_init_state(pnp_ctx* c) {
    using C = typename CxOf<R>::type;
    const State<R, CX> s = state<R, CX>(c);
    const size_t n = (size_t)c->B * c->N;
    if constexpr (CX) HIPCHK(hipMemcpyAsync(s.z, c->coils.aty, n * sizeof(C), hipMemcpyDeviceToDevice, c->stream));
    else HIPCHK(launch_cabs<R>(c->stream, (const C*)c->coils.aty, s.z, n));
    HIPCHK(hipMemsetAsync(s.w, 0, n * sizeof(*s.w), c->stream));
    return PNP_OK;
}

// z = |ifft2(y)|, w = 0
template <typename R> static int init_state(pnp_ctx* c) {
    const Bufs<R> b = bufs<R>(c);
    c->state_sliced = false;                           // both arrays are rewritten below, in natural order
    if (c->coils.C > 0) {
        if (int rc = cx_mode(c) ? coil_init_state<R, true>(c) : coil_init_state<R, false>(c)) return rc;
        c->have_x = false;
        c->have_state = true;
        return PNP_OK;
    }
    ColArgsT<R> ca{};
    ca.in = b.y; ca.out = b.work; ca.B = c->B;
    HIPCHK(cols<R>(c, false, MID_NONE, true, ca));
    RowArgsT<R> ra{};
    ra.cin = b.work; ra.x_out = b.z; ra.scale = (R)1 / (R)c->N; ra.nrows = c->B * c->H;
    HIPCHK(rows<R>(c, IN_COMPLEX, true, EPI_ABS_COMPLEX, ra));
    HIPCHK(hipMemsetAsync(b.w, 0, (size_t)c->B * c->N * sizeof(R), c->stream));
    c->have_x = false;
    c->have_state = true;
    return PNP_OK;
}

template <typename R, bool CX = false> static int set_state(pnp_ctx* c, const char* who, const R* z, const R* w, int on_device) {
    const State<R, CX> s = state<R, CX>(c);
    const size_t bytes = (size_t)c->B * c->N * sizeof(*s.z);
    int rc;
    if (z && w) c->state_sliced = false;               // both replaced: nothing to convert
    else if (!c->have_state) return undefined_state(who);                         // one of the two kept: it must be defined
    else if ((rc = state_order<R>(c, false))) return rc;
    if (z) { rc = copy_in(c, s.z, z, bytes, on_device); if (rc) return rc; }
    if (w) { rc = copy_in(c, s.w, w, bytes, on_device); if (rc) return rc; }
    c->have_x = false;
    if (z && w) c->have_state = true;
    return PNP_OK;
}

template <typename R, bool CX = false> static int get_state(pnp_ctx* c, R* z, R* w, int on_device) {
    const State<R, CX> s = state<R, CX>(c);
    const size_t bytes = (size_t)c->B * c->N * sizeof(*s.z);
    int rc;
    if ((rc = state_order<R>(c, false))) return rc;
    if (z) { rc = copy_out(c, z, s.z, bytes, on_device); if (rc) return rc; }
    if (w) { rc = copy_out(c, w, s.w, bytes, on_device); if (rc) return rc; }
    return PNP_OK;
}


// ---- multi-coil (SENSE) data consistency: coil_plan.h, kernels_coils.hip, the coil row roles of kernels_anysize.hip ----

#define NO_COILS(c, mc) do { if ((c)->coils.C > 0) return fail(PNP_E_STATE, "%s: the context has coils (pnp_set_coils): use %s", __func__, mc); } while (0)
#define NEED_COILS(c) do { if ((c)->coils.C == 0) return fail(PNP_E_STATE, "%s: the context has no coils (pnp_set_coils); without coils use the call without _mc", __func__); } while (0)

static void coils_free(pnp_ctx* c) {
    Coils& k = c->coils;
    void* ptrs[] = {k.maps, k.coil_id, k.mask_idx, k.work, k.ymc, k.aty, k.xh, k.r, k.p, k.gp, k.part_row, k.part_rr[0], k.part_rr[1],
                    k.part_bb, k.scal, k.rel, c->zc, c->wc, c->xc, c->wv_coef_cx};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (k.own_any) anysize_destroy(k.any);
    const int iters = k.cg_iters;
    k = Coils{};
    k.cg_iters = iters;
    c->zc = c->wc = c->xc = c->wv_coef_cx = nullptr;     // complex-valued images go with the coils
    c->image = PNP_IMAGE_REAL;
}

template <typename R> static CoilRowArgsT<R> coil_rows(const pnp_ctx* c, int B) {
    using C = typename CxOf<R>::type;
    CoilRowArgsT<R> a{};
    a.maps = (const C*)c->coils.maps; a.coil_id = c->coils.coil_id; a.ncoils = c->coils.C; a.H = c->H;
    a.work = (C*)c->coils.work; a.scale = 1; a.nrows = B * c->H;
    return a;
}
template <typename R> static ColArgsT<R> coil_cols(const pnp_ctx* c, const void* in, void* out) {
    using C = typename CxOf<R>::type;
    ColArgsT<R> a{};
    a.in = (const C*)in; a.out = (C*)out; a.mask_bank = c->mask_bank; a.mask_id = c->coils.mask_idx; a.B = c->B * c->coils.C;
    return a;
}

// out = A^H k = sum_c conj(S_c) ifft2(m k_c): columns out of place into the work array, combining rows.  k: [B][C][H][W], out: [B][H][W] complex
template <typename R> static int coil_AH(pnp_ctx* c, const void* k, void* out) {
    using C = typename CxOf<R>::type;
    HIPCHK(anysize_cols<R>(c->coils.any, c->stream, false, MID_MASK, true, coil_cols<R>(c, k, c->coils.work)));
    CoilRowArgsT<R> ra = coil_rows<R>(c, c->B);
    ra.cout = (C*)out; ra.scale = (R)1 / (R)c->N;
    HIPCHK(anysize_coil_rows_epi<R>(c->coils.any, c->stream, ra));
    return PNP_OK;
}

// gp = G p: three launches.  Leaves the row partials of Re<p, Gp> in part_row.
template <typename R> static int coil_G(pnp_ctx* c, const void* p, void* gp, R la2) {
    using C = typename CxOf<R>::type;
    CoilRowArgsT<R> ra = coil_rows<R>(c, c->B);
    ra.cin = (const C*)p;
    HIPCHK(anysize_coil_rows_in<R>(c->coils.any, c->stream, ra));
    HIPCHK(anysize_cols<R>(c->coils.any, c->stream, true, MID_MASK, true, coil_cols<R>(c, c->coils.work, c->coils.work)));
    CoilRowArgsT<R> rb = coil_rows<R>(c, c->B);
    rb.cout = (C*)gp; rb.p = (const C*)p; rb.partial = c->coils.part_row; rb.la2 = la2; rb.scale = (R)1 / (R)c->N;
    HIPCHK(anysize_coil_rows_epi<R>(c->coils.any, c->stream, rb));
    return PNP_OK;
}

// The x-step: cg_iters iterations of CG on G x^ = aty + La2 (z - w), warm-started at z - w; x = |Re x^|.  cg_launches(cg_iters) launches,
// no host synchronisation: every scalar stays on the device (kernels_coils.hip).
// CX (complex images, pnp_set_image): z, w, x are complex and x = x^; the launches between the two ends are the same.
template <typename R, bool CX = false>
static int coil_xstep(pnp_ctx* c, const CoilState<R, CX>* z, const CoilState<R, CX>* w, CoilState<R, CX>* x, double reo) {
    using C = typename CxOf<R>::type;
    Coils& k = c->coils;
    const R la2 = (R)(1.0 / 2.0 / reo);
    const int B = c->B, iters = k.cg_iters;
    C *xh = (C*)k.xh, *r = (C*)k.r, *p = (C*)k.p, *gp = (C*)k.gp;
    HIPCHK((launch_cg_begin<R, CX>(c->stream, z, w, xh, B, c->N)));
    if (int rc = coil_G<R>(c, xh, gp, la2)) return rc;
    HIPCHK(launch_cg_init<R>(c->stream, (const C*)k.aty, xh, gp, r, p, la2, k.part_rr[0], k.part_bb, B, c->N));
    int cur = 0;
    for (int i = 0; i < iters; ++i) {
        const bool last = i == iters - 1;
        if (int rc = coil_G<R>(c, p, gp, la2)) return rc;
        HIPCHK((launch_cg_xr<R, CX>(c->stream, xh, r, p, gp, k.part_rr[cur], k.part_row, k.part_rr[cur ^ 1], k.scal,
                                    last ? x : (CoilState<R, CX>*)nullptr, B, c->N, c->H)));
        if (!last) HIPCHK(launch_cg_p<R>(c->stream, r, p, k.part_rr[cur], k.part_rr[cur ^ 1], k.scal, B, c->N));
        cur ^= 1;
    }
    HIPCHK(launch_cg_residual(c->stream, k.part_rr[cur], k.part_bb, k.rel, B, c->N));
    k.have_rel = true;
    return PNP_OK;
}

// ---- complex-valued images (pnp_set_image; kernels_complex.hip): the guards of the entry points ----

#define REAL_IMAGE(c, cx) do { if (cx_mode(c)) return fail(PNP_E_STATE, "%s: the context is in complex image mode (pnp_set_image): use %s", __func__, cx); } while (0)
#define NOT_IN_COMPLEX(c) do { if (cx_mode(c)) return fail(PNP_E_STATE, "%s: not available in complex image mode (pnp_set_image)", __func__); } while (0)
#define NEED_COMPLEX(c) do { if (!cx_mode(c)) return fail(PNP_E_STATE, "%s: needs complex image mode (pnp_set_image); in real mode use the call without _cx", __func__); } while (0)

// every complex array a caller hands in is read and written as 2 sizeof(R)-byte values (float2 / double2; the pixel prox: 16 bytes)
template <typename R> static int cx_aligned(const char* who, const void* a, const void* b = nullptr, const void* c = nullptr, size_t to = 2 * sizeof(R)) {
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & (to - 1)) == 0) return PNP_OK;
    return fail(PNP_E_ARG, "%s: complex arrays must be %zu-byte aligned", who, to);
}

// after begin_problem on a coil context: the coil set of every slice, the expanded mask index
static int coil_begin(pnp_ctx* c, const int32_t* coil_id, int B, int on_device) {
    Coils& k = c->coils;
    k.have_rel = false;
    if (coil_id) {
        std::vector<int32_t> tmp;
        const int32_t* ids = coil_id;
        if (on_device) {
            tmp.resize((size_t)B);
            HIPCHK(hipMemcpyAsync(tmp.data(), coil_id, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            ids = tmp.data();
        }
        for (int i = 0; i < B; ++i) if (ids[i] < 0 || ids[i] >= k.Ks) return fail(PNP_E_ARG, "coil_id[%d]=%d out of range [0,%d)", i, ids[i], k.Ks);
        if (int rc = copy_in(c, k.coil_id, coil_id, (size_t)B * sizeof(int32_t), on_device)) return rc;
    } else {
        HIPCHK(hipMemsetAsync(k.coil_id, 0, (size_t)B * sizeof(int32_t), c->stream));
    }
    HIPCHK(launch_expand_ids(c->stream, c->mask_id, k.mask_idx, B, k.C));
    return PNP_OK;
}
// ends a coil upload / synthesis: aty = A^H y, once per problem; a failure leaves no problem behind
template <typename R> static int coil_finish(pnp_ctx* c, int rc) {
    if (rc == PNP_OK) rc = coil_AH<R>(c, c->coils.ymc, c->coils.aty);
    if (rc != PNP_OK) { c->B = 0; c->prob = Problem{}; }
    return rc;
}

template <typename R>
static int upload_problem_mc(pnp_ctx* c, const char* who, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, const int32_t* coil_id,
                             int B, int K, int on_device) {
    if (!y) { c->B = 0; return fail(PNP_E_ARG, "%s: y is null", who); }
    int rc = begin_problem(c, mask_bank, mask_id, B, K, on_device);
    if (rc == PNP_OK) rc = coil_begin(c, coil_id, B, on_device);
    if (rc == PNP_OK) rc = copy_in(c, c->coils.ymc, y, (size_t)B * c->coils.C * c->N * 2 * sizeof(R), on_device);
    return coil_finish<R>(c, rc);
}

// y_c = m fft2(S_c img) + noise; noise_mode 0: one [H][W] array for every coil and slice, 1: [C][H][W] for every slice, 2: [B][C][H][W]
template <typename R>
static int synthesize_y_mc(pnp_ctx* c, const float* img, const R* noise, int noise_mode, int B, int on_device) {
    using C = typename CxOf<R>::type;
    const Bufs<R> b = bufs<R>(c);
    const int nc = c->coils.C;
    const size_t img_bytes = (size_t)B * c->N * sizeof(float), coil_bytes = (size_t)nc * c->N * sizeof(C);
    const size_t noise_bytes = noise_mode == 0 ? c->N * sizeof(C) : (size_t)B * coil_bytes;
    const float* d_img = img;
    const C* d_noise = (const C*)noise;
    if (!on_device || noise_mode == 1) {
        if (noise_bytes + img_bytes > c->stage_bytes) {
            if (c->stage) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->stage)); c->stage = nullptr; c->stage_bytes = 0; }
            HIPCHK(hipMalloc(&c->stage, noise_bytes + img_bytes));
            c->stage_bytes = noise_bytes + img_bytes;
        }
        char* st = (char*)c->stage;
        if (noise_mode == 1) {
            for (int s = 0; s < B; ++s) if (int rc = copy_in(c, st + (size_t)s * coil_bytes, noise, coil_bytes, on_device)) return rc;
            d_noise = (const C*)st;
        } else if (!on_device) {
            if (int rc = copy_in(c, st, noise, noise_bytes, 0)) return rc;
            d_noise = (const C*)st;
        }
        if (!on_device) {
            if (int rc = copy_in(c, st + noise_bytes, img, img_bytes, 0)) return rc;
            d_img = (const float*)(st + noise_bytes);
        }
    }
    CoilRowArgsT<R> ra = coil_rows<R>(c, B);
    if constexpr (std::is_same_v<R, double>) {
        HIPCHK(launch_widen(c->stream, d_img, b.x, (size_t)B * c->N));
        ra.rin = b.x;
    } else {
        ra.rin = d_img;
    }
    ra.work = (C*)c->coils.ymc;
    HIPCHK(anysize_coil_rows_in<R>(c->coils.any, c->stream, ra));
    ColArgsT<R> ca = coil_cols<R>(c, c->coils.ymc, c->coils.ymc);
    ca.y = d_noise; ca.y_per_slice = noise_mode != 0;
    HIPCHK(anysize_cols<R>(c->coils.any, c->stream, true, MID_MASK_ADD, false, ca));
    return PNP_OK;
}

template <typename R>
static int synthesize_problem_mc(pnp_ctx* c, const char* who, const float* img, const R* noise, int noise_mode, const uint8_t* mask_bank,
                                 const int32_t* mask_id, const int32_t* coil_id, int B, int K, int on_device) {
    if (!img || !noise) { c->B = 0; return fail(PNP_E_ARG, "%s: img/noise is null", who); }
    if (noise_mode < 0 || noise_mode > 2) { c->B = 0; return fail(PNP_E_ARG, "%s: noise_mode must be 0 ([H][W]), 1 ([C][H][W]) or 2 ([B][C][H][W]) (got %d)", who, noise_mode); }
    int rc = begin_problem(c, mask_bank, mask_id, B, K, on_device);
    if (rc == PNP_OK) rc = coil_begin(c, coil_id, B, on_device);
    if (rc == PNP_OK) rc = synthesize_y_mc<R>(c, img, noise, noise_mode, B, on_device);
    return coil_finish<R>(c, rc);
}

// pnp_set_coils: C = 0 clears.  Either way the uploaded problem is dropped.
template <typename R>
static int set_coils(pnp_ctx* c, const char* who, const R* sens, int C, int Ks, int on_device) {
    using Cx = typename CxOf<R>::type;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->B = 0; c->prob = Problem{};
    c->state_sliced = c->have_x = c->have_state = false;
    coils_free(c);
    if (C == 0) return PNP_OK;
    if (!sens) return fail(PNP_E_ARG, "%s: sens is null", who);
    Coils& k = c->coils;
    const size_t BN = (size_t)c->Bmax * c->N, nblk = (size_t)cg_blocks(c->N);
    const size_t work_bytes = coil_work_elems(c->Bmax, C, c->H, c->W) * sizeof(Cx), map_bytes = coil_map_elems(Ks, C, c->H, c->W) * sizeof(Cx);
    struct Want { void** p; size_t bytes; const char* what; };
    const Want wants[] = {
        {&k.maps, map_bytes, "coil maps"}, {&k.work, work_bytes, "coil work array"}, {&k.ymc, work_bytes, "coil measurements"},
        {&k.aty, BN * sizeof(Cx), "CG arrays"}, {&k.xh, BN * sizeof(Cx), "CG arrays"}, {&k.r, BN * sizeof(Cx), "CG arrays"},
        {&k.p, BN * sizeof(Cx), "CG arrays"}, {&k.gp, BN * sizeof(Cx), "CG arrays"},
        {(void**)&k.coil_id, (size_t)c->Bmax * sizeof(int32_t), "coil_id"}, {(void**)&k.mask_idx, (size_t)c->Bmax * C * sizeof(int32_t), "mask index"},
        {(void**)&k.part_row, (size_t)c->Bmax * cg_row_partials(c->H) * sizeof(double), "CG partials"},
        {(void**)&k.part_rr[0], c->Bmax * nblk * sizeof(double), "CG partials"}, {(void**)&k.part_rr[1], c->Bmax * nblk * sizeof(double), "CG partials"},
        {(void**)&k.part_bb, c->Bmax * nblk * sizeof(double), "CG partials"},
        {(void**)&k.scal, (size_t)c->Bmax * 4 * sizeof(double), "CG scalars"}, {(void**)&k.rel, (size_t)c->Bmax * sizeof(double), "CG residual"},
    };
    for (const Want& w : wants)
        if (int rc = alloc_or_fail(w.p, w.bytes, who, w.what, "Bmax=%d, C=%d, %dx%d", c->Bmax, C, c->H, c->W)) { coils_free(c); return rc; }
    HIPCHK(hipMemsetAsync(k.scal, 0, (size_t)c->Bmax * 4 * sizeof(double), c->stream));
    if (c->any) k.any = c->any;
    else {
        hipError_t e = hipSuccess;
        k.any = anysize_create(c->H, c->W, c->f64, &e);
        if (!k.any) { coils_free(c); return fail(PNP_E_HIP, "%s: transform tables: %s", who, hipGetErrorString(e)); }
        k.own_any = true;
    }
    k.C = C; k.Ks = Ks;                                   // from here on the context has coils
    if (int rc = copy_in(c, k.maps, sens, map_bytes, on_device)) { coils_free(c); return rc; }
    return PNP_OK;
}

// one generic iteration: rows fwd (z-w) -> cols fwd/blend/inv -> rows inv + prox + dual
template <typename R>
static int generic_iteration(pnp_ctx* c, const R* z_in, const R* w_in, RowEpi epi, const ProxParamsT<R>& pp, R cdc, R* x_out,
                             R* z_io, R* w_io) {
    const Bufs<R> b = bufs<R>(c);
    RowArgsT<R> ra{};
    ra.rin0 = z_in; ra.rin1 = w_in; ra.cout = b.work; ra.scale = 1; ra.nrows = c->B * c->H;
    HIPCHK(rows<R>(c, IN_REAL_DIFF, false, EPI_COMPLEX, ra));
    ColArgsT<R> ca{};
    ca.in = b.work; ca.out = b.work; ca.y = b.y; ca.mask_bank = c->mask_bank; ca.mask_id = c->mask_id;
    ca.c = cdc; ca.B = c->B;
    HIPCHK(cols<R>(c, true, MID_BLEND, true, ca));
    RowArgsT<R> rb{};
    rb.cin = b.work; rb.x_out = x_out; rb.z = z_io; rb.w = w_io; rb.scale = (R)1 / (R)c->N;
    rb.prox = pp; rb.nrows = c->B * c->H;
    HIPCHK(rows<R>(c, IN_COMPLEX, true, epi, rb));
    return PNP_OK;
}

// The fast loops (Path::slice, Path::fused) on a float state ...
static hipError_t fast_run(pnp_ctx* c, Path path, int iters, bool cnc, float cdc, const ProxParams& pp) {
    const Bufs<float> b = bufs<float>(c);
    if (path == Path::slice) return slice256_run(c->eng.slice, c->stream, b.z, b.w, b.x, c->B, iters, cnc, cdc, pp, c->sched);
    switch (c->eng.kind) {
    case Engine::fused256:  return fused256_run(c->eng.f256, c->stream, b.z, b.w, b.x, c->B, iters, cnc, cdc, pp, c->sched);
    case Engine::split_f32: return fused256s_run<float>(c->eng.s32, c->stream, b.z, b.w, b.x, c->B, iters, cnc, cdc, pp, c->sched);
    case Engine::fused512:  return fused512_run(c->eng.f512, c->stream, b.z, b.w, b.x, c->B, iters, cnc, cdc, pp, c->sched);
    case Engine::none: case Engine::split_f64: break;
    }
    return hipErrorInvalidValue;
}
// ... and on a double state: the split chain is the one double engine (no slice path in double)
static hipError_t fast_run(pnp_ctx* c, Path, int iters, bool cnc, double cdc, const ProxParamsT<double>& pp) {
    const Bufs<double> b = bufs<double>(c);
    return fused256s_run<double>(c->eng.s64, c->stream, b.z, b.w, b.x, c->B, iters, cnc, cdc, pp, c->sched);
}

// One data-consistency step x = dc(z, w) on pointers in natural order, on the context's own kernels: the two-launch engine of the shape
// and precision where there is one, the generic / any-size kernels otherwise.
template <typename R> static int dc_any(pnp_ctx* c, const R* z, const R* w, R* x, R cdc) {
    if (dc_path(c) == Path::generic || c->eng.kind == Engine::none)
        return generic_iteration<R>(c, z, w, EPI_ABS_REAL, ProxParamsT<R>{}, cdc, x, nullptr, nullptr);
    if (int rc = ensure_tables(c, Path::fused)) return rc;
    if constexpr (std::is_same_v<R, double>) {
        HIPCHK(fused256s_dc<double>(c->eng.s64, c->stream, z, w, x, c->B, cdc));
    } else {
        switch (c->eng.kind) {
        case Engine::fused256:  HIPCHK(fused256_dc(c->eng.f256, c->stream, z, w, x, c->B, cdc)); break;
        case Engine::split_f32: HIPCHK(fused256s_dc<float>(c->eng.s32, c->stream, z, w, x, c->B, cdc)); break;
        case Engine::fused512:  HIPCHK(fused512_dc(c->eng.f512, c->stream, z, w, x, c->B, cdc)); break;
        case Engine::none: case Engine::split_f64: break;
        }
    }
    return PNP_OK;
}

// ---- wavelet-domain sparsity (pnp_set_sparsity; wavelet_plan.h, kernels_wavelet.hip) ----

// The coefficient array of the wavelet prox, real or (cx) complex.  Both are allocated where the setting is made -- the real one by
// pnp_set_sparsity, the complex one by pnp_set_image or pnp_set_sparsity, whichever comes second -- so that no loop and no step-wise
// call allocates; a failure of the complex one is reported in the name of that call, `who`.
static int wavelet_scratch(pnp_ctx* c, bool cx = false, const char* who = "") {
    if (cx ? c->wv_coef_cx : c->wv_coef) return PNP_OK;
    if (cx) return alloc_or_fail(&c->wv_coef_cx, (size_t)c->Bmax * c->N * 2 * (c->f64 ? sizeof(double) : sizeof(float)), who,
                                 "complex wavelet coefficients", "Bmax=%d, %dx%d", c->Bmax, c->H, c->W);
    HIPCHK(hipMalloc(&c->wv_coef, (size_t)c->Bmax * c->N * (c->f64 ? sizeof(double) : sizeof(float))));
    return PNP_OK;
}

// One wavelet prox of the context, wherever one runs (the loops, the coil loop, pnp_prox_*_dual): with a spin setting (pnp_set_spin) in
// the frames of the schedule's current group of shifts, and the cursor moves on; without one the unshifted step.
static int spin_per_prox(const pnp_ctx* c) { return c->spin.empty() ? 1 : c->spin_k; }
template <typename R> static int wavelet_prox_step(pnp_ctx* c, bool cnc, const R* x, R* z, R* w, const ProxParamsT<R>& pp) {
    if (c->spin.empty()) {
        HIPCHK(launch_wavelet_prox<R>(c->stream, c->wavelet, c->wv_levels, cnc, x, z, w, (R*)c->wv_coef, pp, c->B, c->H, c->W));
        return PNP_OK;
    }
    const int n = (int)(c->spin.size() / 2), K = c->spin_k, groups = n / K;
    const int32_t* s = c->spin.data() + 2 * (size_t)wv_spin_first(c->spin_p, n, K);
    HIPCHK(launch_wavelet_prox<R>(c->stream, c->wavelet, c->wv_levels, cnc, x, z, w, (R*)c->wv_coef, pp, c->B, c->H, c->W, s, K, (R*)c->wv_acc));
    c->spin_p = c->spin_p == INT_MAX ? INT_MAX % groups + 1 : c->spin_p + 1;          // the same entries, within int
    return PNP_OK;
}

// One low-rank prox of the context, wherever one runs (the loops, the coil loop, pnp_prox_*_dual): thr and ib scaled, on the grid anchored
// at the shift table's current entry, and the cursor moves on.
template <typename R> static int lowrank_prox_step(pnp_ctx* c, bool cnc, const R* x, R* z, R* w, const ProxParamsT<R>& pp) {
    if (int rc = pnp_lowrank_check(c->tp_frames, c->lr_block, c->H, c->W, c->B, c->f64 ? 1 : 0, cnc ? 1 : 0)) return rc;
    const int n = (int)(c->lr_shifts.size() / 2);
    const int32_t* s = c->lr_shifts.data() + 2 * (size_t)lr_shift_entry(c->lr_p, n);
    ProxParamsT<R> q = pp;
    q.thr = (R)((double)pp.thr * c->lr_scale);
    q.ib = (R)((double)pp.ib * c->lr_scale);
    HIPCHK(launch_lowrank_prox<R>(c->stream, cnc, x, z, w, q, c->tp_frames, c->lr_block, s[0], s[1], c->B, c->H, c->W));
    c->lr_p = c->lr_p == INT_MAX ? INT_MAX % n + 1 : c->lr_p + 1;                      // the same entries, within int
    return PNP_OK;
}

// One z / w step of the loops and the step-wise calls, on real or (CX) complex arrays in natural order: the pixel prox (one launch) or the
// wavelet prox of the context's sparsity setting (two; in real mode by the spin schedule), or the temporal prox of pnp_set_temporal (one),
// or -- ahead of it -- the low-rank prox of pnp_set_lowrank (one; real images).
// Which launcher serves which type ends here.
template <typename R, bool CX>
static int prox_step(pnp_ctx* c, bool cnc, const CoilState<R, CX>* x, CoilState<R, CX>* z, CoilState<R, CX>* w, const ProxParamsT<R>& pp) {
    const size_t n = (size_t)c->B * c->N;
    if (c->lr_block) {
        if constexpr (CX) return fail(PNP_E_STATE, "lowrank: not available in complex image mode (pnp_set_image)");
        else return lowrank_prox_step<R>(c, cnc, x, z, w, pp);
    }
    if (c->tp_frames) {
        if (int rc = pnp_temporal_check(c->tp_frames, c->B)) return rc;
        HIPCHK((launch_temporal_prox<R, CX>(c->stream, cnc, x, z, w, (const R*)c->tp_tw, pp, c->tp_frames, c->tp_keep_dc, c->B, c->N)));
        return PNP_OK;
    }
    if constexpr (CX) {
        if (c->wavelet == WV_NONE) {
            HIPCHK(launch_prox_cx<R>(c->stream, cnc, x, z, w, pp, n));
            return PNP_OK;
        }
        if (!c->wv_coef_cx) return fail(PNP_E_STATE, "complex wavelet prox: no coefficient array (pnp_set_image / pnp_set_sparsity allocate it)");
        HIPCHK(launch_wavelet_prox_cx<R>(c->stream, c->wavelet, c->wv_levels, cnc, x, z, w, state<R, true>(c).wv_coef, pp, c->B, c->H, c->W));
    } else if (c->wavelet != WV_NONE) {
        if (int rc = wavelet_scratch(c)) return rc;
        return wavelet_prox_step<R>(c, cnc, x, z, w, pp);
    } else if constexpr (std::is_same_v<R, double>) {
        HIPCHK(launch_prox_f64(c->stream, cnc, x, z, w, pp, n));
    } else {
        HIPCHK(launch_prox(c->stream, cnc, x, z, w, pp, n));
    }
    return PNP_OK;
}

// Psi / Psi^T on caller pointers, in the frame shifted by (sy, sx).  A tile reads its neighbours' halo, so an in-place call goes through
// the context's scratch.
template <typename R> static int dwt2_any(pnp_ctx* c, const char* who, const R* in, R* out, int B, bool inv, int sy = 0, int sx = 0) {
    if (c->wavelet == WV_NONE) return fail(PNP_E_STATE, "%s: no wavelet set (pnp_set_sparsity)", who);
    if (!wv_shift_ok(c->wv_levels, sy, sx))
        return fail(PNP_E_ARG, "%s: shift (%d, %d) out of range [0, %d) (2^levels)", who, sy, sx, 1 << c->wv_levels);
    if (!in || !out) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (B < 1 || B > c->Bmax) return fail(PNP_E_ARG, "%s: B=%d out of range [1,%d]", who, B, c->Bmax);
    const size_t bytes = (size_t)B * c->N * sizeof(R);
    const char *pi = (const char*)in, *po = (const char*)out;
    if (pi != po && pi < po + bytes && po < pi + bytes) return fail(PNP_E_ARG, "%s: in and out overlap without being equal", who);
    R* dst = out;
    if (pi == po) { if (int rc = wavelet_scratch(c)) return rc; dst = (R*)c->wv_coef; }
    HIPCHK(launch_dwt2<R>(c->stream, c->wavelet, c->wv_levels, inv, in, dst, B, c->H, c->W, sy, sx));
    if (dst != out) HIPCHK(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToDevice, c->stream));
    return PNP_OK;
}

// The loops with a wavelet or frames set (natural_loop): per iteration the data-consistency step and the prox step's launches, on the
// state in natural order.  Every iteration stands alone -- nothing but x, z, w passes from one to the next -- so a run cut anywhere is
// bit-equal to the uncut run.
static bool natural_loop(const pnp_ctx* c) { return c->wavelet != WV_NONE || c->tp_frames != 0; }
template <typename R>
static int run_natural_loop(pnp_ctx* c, int iters, bool cnc, const ProxParamsT<R>& pp, double reo) {
    const Bufs<R> b = bufs<R>(c);
    if (int rc = state_order<R>(c, false)) return rc;
    const R cdc = dc_coeff<R>(reo);
    for (int i = 0; i < iters; ++i) {
        if (int rc = dc_any<R>(c, b.z, b.w, b.x, cdc)) return rc;
        if (int rc = prox_step<R, false>(c, cnc, b.x, b.z, b.w, pp)) return rc;
    }
    c->have_x = true;
    return PNP_OK;
}

// The step-wise calls on caller pointers in natural order (CX: complex, interleaved).  pnp_dc_step[_cx]: one x-step; without coils the
// data-consistency step of the context's own kernels (dc_any).
template <typename R, bool CX> static int dc_step(pnp_ctx* c, const char* who, const R* z, const R* w, R* x, double reo) {
    using T = CoilState<R, CX>;
    if (!z || !w || !x) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (!(reo > 0.0)) return fail(PNP_E_ARG, "%s: reo must be > 0", who);
    if constexpr (CX) {
        if (int rc = cx_aligned<R>(who, z, w, x)) return rc;
    } else {
        if (c->coils.C == 0) return dc_any<R>(c, z, w, x, dc_coeff<R>(reo));
    }
    return coil_xstep<R, CX>(c, (const T*)z, (const T*)w, (T*)x, reo);
}
// pnp_prox_*_dual[_cx]: one prox step.  Complex arrays: 16-byte aligned for the pixel prox, 2 sizeof(R) for the wavelet and the temporal prox; with a wavelet
// set the three arrays must not overlap.
template <typename R, bool CX> static int prox_dual(pnp_ctx* c, const char* who, bool cnc, const R* x, R* z, R* w, const ProxParamsT<R>& pp) {
    using T = CoilState<R, CX>;
    if (!x || !z || !w) return fail(PNP_E_ARG, "%s: null pointer", who);
    if constexpr (CX) if (int rc = cx_aligned<R>(who, x, z, w, (c->wavelet == WV_NONE && !c->tp_frames) ? 16 : 2 * sizeof(R))) return rc;
    if (c->wavelet != WV_NONE) {
        const size_t bytes = (size_t)c->B * c->N * sizeof(T);
        const char *px = (const char*)x, *pz = (const char*)z, *pw = (const char*)w;
        if ((px < pz + bytes && pz < px + bytes) || (px < pw + bytes && pw < px + bytes) || (pz < pw + bytes && pw < pz + bytes))
            return fail(PNP_E_ARG, "%s: x, z and w must not overlap with a wavelet set (tiles read their neighbours' halo)", who);
    }
    // no overlap rule with frames set: a workgroup of the temporal kernel loads its whole run of x, z, w before it stores z+ and w+, and runs
    // are disjoint, so x, z, w that alias one another (the pixel prox's in-place use) are safe
    return prox_step<R, CX>(c, cnc, (const T*)x, (T*)z, (T*)w, pp);
}

// the loops of a coil context: per iteration the x-step and the prox step, on the state in natural order; every iteration stands alone,
// so a run cut anywhere (the trace's legs) is bit-equal to the uncut run
template <typename R, bool CX>
static int run_coil_loop(pnp_ctx* c, int iters, bool cnc, const ProxParamsT<R>& pp, double reo) {
    const State<R, CX> s = state<R, CX>(c);
    if (iters == 0) HIPCHK(hipMemcpyAsync(s.x, s.z, (size_t)c->B * c->N * sizeof(*s.x), hipMemcpyDeviceToDevice, c->stream));
    for (int i = 0; i < iters; ++i) {
        if (int rc = coil_xstep<R, CX>(c, s.z, s.w, s.x, reo)) return rc;
        if (int rc = prox_step<R, CX>(c, cnc, s.x, s.z, s.w, pp)) return rc;
    }
    c->have_x = true;
    return PNP_OK;
}

template <typename R>
static int run_loop(pnp_ctx* c, int iters, bool cnc, const ProxParamsT<R>& pp, double reo) {
    if (c->tp_frames) if (int rc = pnp_temporal_check(c->tp_frames, c->B)) return rc;      // before the first x-step
    if (c->lr_block) if (int rc = pnp_lowrank_check(c->tp_frames, c->lr_block, c->H, c->W, c->B, c->f64 ? 1 : 0, cnc ? 1 : 0)) return rc;
    if (c->coils.C > 0) return cx_mode(c) ? run_coil_loop<R, true>(c, iters, cnc, pp, reo) : run_coil_loop<R, false>(c, iters, cnc, pp, reo);
    if (natural_loop(c) && iters > 0) return run_natural_loop<R>(c, iters, cnc, pp, reo);
    const Bufs<R> b = bufs<R>(c);
    const Path path = iters > 0 ? loop_path(c) : Path::generic;
    if (int rc = ensure_tables(c, path)) return rc;
    if (int rc = state_order<R>(c, path == Path::slice)) return rc;
    const R cdc = dc_coeff<R>(reo);
    switch (path) {
    case Path::generic:
        // iters == 0: the reference's loop body never runs and its x stays the initial x = |ifft2(y)| = z0 (S4:103, 107, 138)
        if (iters == 0) HIPCHK(hipMemcpyAsync(b.x, b.z, (size_t)c->B * c->N * sizeof(R), hipMemcpyDeviceToDevice, c->stream));
        for (int i = 0; i < iters; ++i) {
            int rc = generic_iteration<R>(c, b.z, b.w, cnc ? EPI_CNC : EPI_L1, pp, cdc, (i == iters - 1) ? b.x : nullptr, b.z, b.w);
            if (rc) return rc;
        }
        break;
    case Path::slice:
    case Path::fused:
        HIPCHK(fast_run(c, path, iters, cnc, cdc, pp));
        break;
    }
    c->have_x = true;
    return PNP_OK;
}

// ---- convergence trace: legs of launches by trace_plan.h, one reduction per check ----

// the reduction's scratch, and room for `checks` rows
static int trace_buffers(pnp_ctx* c, int checks) {
    Trace& t = c->trace;
    if (!t.partial) HIPCHK(hipMalloc((void**)&t.partial, trace_scratch_bytes(c->Bmax)));
    if (!t.counter) {
        HIPCHK(hipMalloc((void**)&t.counter, (size_t)c->Bmax * sizeof(unsigned)));
        HIPCHK(hipMemset(t.counter, 0, (size_t)c->Bmax * sizeof(unsigned)));          // every launch leaves it zero again
    }
    if (checks > t.rows_cap) {
        if (t.rows) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(t.rows)); t.rows = nullptr; t.rows_cap = 0; }
        HIPCHK(hipMalloc((void**)&t.rows, (size_t)checks * TRACE_Q * c->Bmax * sizeof(double)));
        t.rows_cap = checks;
    }
    return PNP_OK;
}

// sums of squares [TRACE_Q][B] -> r_pri, r_dual, x_norm, z_norm, w_norm, psnr, re (pnp_metrics' formulas; NaN without a ground truth)
static void trace_values(const double* sums, double* out, int B, size_t N, bool have_gt) {
    for (int b = 0; b < B; ++b) {
        for (int q = TR_XZ; q <= TR_W; ++q) out[(size_t)q * B + b] = sqrt(sums[(size_t)q * B + b]);
        const double se = sums[(size_t)TR_E * B + b], sg = sums[(size_t)TR_G * B + b], mse = se / (double)N;
        out[(size_t)PNP_TRACE_PSNR * B + b] = !have_gt ? NAN : (mse == 0.0) ? INFINITY : 20.0 * log10(255.0 / sqrt(mse));
        out[(size_t)PNP_TRACE_RE * B + b] = !have_gt ? NAN : sqrt(se) / sqrt(sg);
    }
}

// One launch of the chain of the context's two-launch engine (engine_host.h, chain_step), on a float state ...
static hipError_t fast_step(pnp_ctx* c, ChainStep st, const float* z, const float* w, float* zo, float* wo, float* x, bool cnc, float cdc,
                            const ProxParams& pp, bool u_first) {
    switch (c->eng.kind) {
    case Engine::fused256:  return fused256_step(c->eng.f256, c->stream, st, z, w, zo, wo, x, c->B, cnc, cdc, pp, c->sched, u_first);
    case Engine::split_f32: return fused256s_step<float>(c->eng.s32, c->stream, st, z, w, zo, wo, x, c->B, cnc, cdc, pp, c->sched, u_first);
    case Engine::fused512:  return fused512_step(c->eng.f512, c->stream, st, z, w, zo, wo, x, c->B, cnc, cdc, pp, c->sched, u_first);
    case Engine::none: case Engine::split_f64: break;
    }
    return hipErrorInvalidValue;
}
// ... and on a double state
static hipError_t fast_step(pnp_ctx* c, ChainStep st, const double* z, const double* w, double* zo, double* wo, double* x, bool cnc, double cdc,
                            const ProxParamsT<double>& pp, bool u_first) {
    return fused256s_step<double>(c->eng.s64, c->stream, st, z, w, zo, wo, x, c->B, cnc, cdc, pp, c->sched, u_first);
}

struct TraceRun {                     // what run_traced's two drivers share
    int iters, every, checks;
    double tol;
    const uint8_t* gt;                // device, or null
};
// after the reduction of check k into row `out`: with tol, read the row, note who meets the rule; -> 1 = stop, 0 = go on, < 0 error
static int trace_checked(pnp_ctx* c, const TraceRun& r, int iter, const double* out) {
    if (!(r.tol > 0.0)) return 0;                                                  // the whole trace is read after the run
    Trace& t = c->trace;
    const int B = c->B;
    const size_t row = (size_t)TRACE_Q * B;
    std::vector<double> sums(row), vals(row);
    if (int rc = copy_out(c, sums.data(), out, row * sizeof(double), 0)) return rc;      // one small copy and one sync per check
    trace_values(sums.data(), vals.data(), B, c->N, r.gt != nullptr);
    t.iters.push_back(iter);
    t.values.insert(t.values.end(), vals.begin(), vals.end());
    bool all = true;
    for (int s = 0; s < B; ++s) {
        const double rp = vals[(size_t)PNP_TRACE_R_PRI * B + s], rd = vals[(size_t)PNP_TRACE_R_DUAL * B + s];
        const bool met = (rp > rd ? rp : rd) <= r.tol * vals[(size_t)PNP_TRACE_Z_NORM * B + s];
        if (met && t.converged_at[s] == 0) t.converged_at[s] = iter;
        all = all && met;
    }
    return all ? 1 : 0;
}

// The two-launch engines (Path::fused).  Their run is a chain of launches already -- forward rows, then columns and rows per iteration --
// but it is NOT cut: two slices share one complex transform, and the absent partner of an odd batch's last slice lives on in the
// transform buffer from iteration to iteration, so a run cut into launches of fewer iterations rounds that slice differently (DESIGN.md
// section 11).  The chain therefore runs on unbroken, launch for launch what the untraced run enqueues (on one queue: scheduling never
// changes results), and where an iteration's state is wanted -- k a checked iteration, or k + 1 one (its z is that check's z_prev) -- a
// LAST-stage row launch between the iteration's columns and its mid-stage rows writes x, z, w of that iteration into side buffers: the
// very launch that ends an untraced run of k iterations, on the same inputs, so the rows are the norms of exactly that run's state.
template <typename R>
static int run_traced_chain(pnp_ctx* c, const TraceRun& r, bool cnc, const ProxParamsT<R>& pp, R cdc, int* nrows, int* done) {
    Trace& t = c->trace;
    const Bufs<R> b = bufs<R>(c);
    const int B = c->B;
    const size_t row = (size_t)TRACE_Q * B, bytes = (size_t)B * c->N * sizeof(R), cap = (size_t)c->Bmax * c->N * sizeof(R);
    for (void** p : {&t.zprev, &t.zc, &t.wc}) if (!*p) HIPCHK(hipMalloc(p, cap));
    R *zp = (R*)t.zprev, *zc = (R*)t.zc, *wc = (R*)t.wc;
    int k_check = 0, next = trace_check_iter(r.iters, r.every, 0);
    if (next == 1) HIPCHK(hipMemcpyAsync(zp, b.z, bytes, hipMemcpyDeviceToDevice, c->stream));          // z_0
    HIPCHK(fast_step(c, ChainStep::open, b.z, b.w, (R*)nullptr, (R*)nullptr, b.x, cnc, cdc, pp, true));
    for (int k = 1; k <= r.iters; ++k) {
        const bool first = k == 1, last = k == r.iters;
        HIPCHK(fast_step(c, ChainStep::cols, b.z, b.w, (R*)nullptr, (R*)nullptr, b.x, cnc, cdc, pp, first));
        if (k == next) {
            double* out = t.rows + (size_t)k_check * row;
            if (last) {                                                            // the run's own last stage, in place
                HIPCHK(fast_step(c, ChainStep::last, b.z, b.w, b.z, b.w, b.x, cnc, cdc, pp, first));
                HIPCHK(launch_residuals<R>(c->stream, b.x, b.z, zp, b.w, r.gt, 0, B, c->N, c->N, false, t.partial, t.counter, out));
            } else {
                HIPCHK(fast_step(c, ChainStep::last, b.z, b.w, zc, wc, b.x, cnc, cdc, pp, first));
                HIPCHK(launch_residuals<R>(c->stream, b.x, zc, zp, wc, r.gt, 0, B, c->N, c->N, false, t.partial, t.counter, out));
            }
            *nrows = ++k_check; *done = k;
            const int stop = trace_checked(c, r, k, out);
            if (stop < 0) return stop;
            if (stop == 1) {
                if (!last) {                                                       // the state of iteration k becomes the context's
                    HIPCHK(hipMemcpyAsync(b.z, zc, bytes, hipMemcpyDeviceToDevice, c->stream));
                    HIPCHK(hipMemcpyAsync(b.w, wc, bytes, hipMemcpyDeviceToDevice, c->stream));
                }
                return PNP_OK;
            }
            if (last) return PNP_OK;
            next = trace_check_iter(r.iters, r.every, k_check);
            if (next == k + 1) { R* tmp = zp; zp = zc; zc = tmp; t.zprev = zp; t.zc = zc; }      // z_k is the next check's z_prev
        } else if (k + 1 == next) {
            HIPCHK(fast_step(c, ChainStep::last, b.z, b.w, zp, wc, b.x, cnc, cdc, pp, first));      // z_k for the check at k + 1
        }
        HIPCHK(fast_step(c, last ? ChainStep::last : ChainStep::mid, b.z, b.w, b.z, b.w, b.x, cnc, cdc, pp, first));
    }
    return PNP_OK;
}

// A run of `iters` iterations with a check every `every`.  Slice-resident and generic paths: per check a leg of trace_plan.h -- [launch
// of leg.pre iterations], snapshot of z, one iteration, reduction into row c -- all on the context's stream, each behind the join that
// ends the launch before it.  Two-launch engines: run_traced_chain above.  Without tol the host reads nothing until the run is over;
// with tol it reads one row per check and stops once every slice meets the rule.
template <typename R>
static int run_traced(pnp_ctx* c, const char* who, int iters, bool cnc, const ProxParamsT<R>& pp, double reo, int every, double tol,
                      const uint8_t* gt, int gt_on_device, int* checks_out, int* iters_done) {
    if (every < 1) return fail(PNP_E_ARG, "%s: every must be >= 1 (got %d)", who, every);
    if (!checks_out || !iters_done) return fail(PNP_E_ARG, "%s: checks / iters_done is null", who);
    if (tol != tol) return fail(PNP_E_ARG, "%s: tol is NaN", who);
    Trace& t = c->trace;
    const Bufs<R> b = bufs<R>(c);
    const int B = c->B, checks = trace_checks(iters, every);
    const size_t row = (size_t)TRACE_Q * B, state_bytes = (size_t)B * c->N * sizeof(R);
    t.B = B; t.iters.clear(); t.values.clear(); t.converged_at.assign((size_t)B, 0);
    *checks_out = 0; *iters_done = 0;
    if (checks == 0) return run_loop<R>(c, iters, cnc, pp, reo);                    // iters == 0: the untraced call
    if (int rc = trace_buffers(c, checks)) return rc;
    if (gt && !gt_on_device) {
        if (!c->gt) HIPCHK(hipMalloc((void**)&c->gt, (size_t)c->Bmax * c->N));
        if (int rc = copy_in(c, c->gt, gt, (size_t)B * c->N, 0)) return rc;
        gt = c->gt;
    }
    const TraceRun r{iters, every, checks, tol, gt};
    int done = 0, nrows = 0;
    // with a wavelet or frames set every iteration is a launch boundary with the state in natural order: the legs below, on run_loop's
    // natural-order loop
    const Path path = natural_loop(c) ? Path::generic : loop_path(c);
    if (path == Path::fused) {
        if (int rc = ensure_tables(c, Path::fused)) return rc;
        if (int rc = state_order<R>(c, false)) return rc;
        if (int rc = run_traced_chain<R>(c, r, cnc, pp, dc_coeff<R>(reo), &nrows, &done)) return rc;
        c->have_x = true;
    } else for (int k = 0; k < checks; ++k) {
        const TraceLeg leg = trace_leg(iters, every, k);
        if (leg.pre > 0) if (int rc = run_loop<R>(c, leg.pre, cnc, pp, reo)) return rc;
        // z of iteration leg.iter - 1, in the order the coming launch leaves z in
        const bool sliced = path == Path::slice;
        if (int rc = state_order<R>(c, sliced)) return rc;
        if constexpr (std::is_same_v<R, float>) {
            if (sliced) HIPCHK(slice256_trace_snapshot(c->eng.slice, c->stream, b.z, B));
        }
        if (!sliced) {
            if (!t.zprev) HIPCHK(hipMalloc(&t.zprev, (size_t)c->Bmax * c->N * sizeof(R)));
            HIPCHK(hipMemcpyAsync(t.zprev, b.z, state_bytes, hipMemcpyDeviceToDevice, c->stream));
        }
        if (int rc = run_loop<R>(c, 1, cnc, pp, reo)) return rc;
        done = leg.iter;
        double* out = t.rows + (size_t)k * row;
        if constexpr (std::is_same_v<R, float>) {
            if (sliced) HIPCHK(slice256_residuals(c->eng.slice, c->stream, b.x, b.z, b.w, gt, B, t.partial, t.counter, out));
        }
        if (!sliced) HIPCHK(launch_residuals<R>(c->stream, b.x, b.z, (const R*)t.zprev, b.w, gt, 0, B, c->N, c->N, false, t.partial, t.counter, out));
        nrows = k + 1;
        const int stop = trace_checked(c, r, leg.iter, out);
        if (stop < 0) return stop;
        if (stop == 1) break;
    }
    if (!(tol > 0.0)) {                                                              // the whole trace in one copy
        std::vector<double> all((size_t)nrows * row);
        if (int rc = copy_out(c, all.data(), t.rows, all.size() * sizeof(double), 0)) return rc;
        t.values.resize(all.size());
        for (int k = 0; k < nrows; ++k) {
            t.iters.push_back(trace_check_iter(iters, every, k));
            trace_values(all.data() + (size_t)k * row, t.values.data() + (size_t)k * row, B, c->N, gt != nullptr);
        }
    }
    *checks_out = nrows; *iters_done = done;
    return PNP_OK;
}

// pnp_residuals[_f64]: the reduction alone, on caller pointers in natural order
template <typename R>
static int residuals_any(pnp_ctx* c, const char* who, const R* x, const R* z, const R* zp, const R* w, const uint8_t* gt, int gt_on_device,
                         int quantise, double* out, int out_on_device) {
    if (!x || !z || !zp || !w || !out) return fail(PNP_E_ARG, "%s: null pointer", who);
    const size_t row = (size_t)TRACE_Q * c->B;
    if (out_on_device) {
        const char *o0 = (const char*)out, *o1 = o0 + row * sizeof(double);
        const size_t bytes = (size_t)c->B * c->N * sizeof(R);
        for (const void* p : {(const void*)x, (const void*)z, (const void*)zp, (const void*)w})
            if (o0 < (const char*)p + bytes && (const char*)p < o1) return fail(PNP_E_ARG, "%s: out must not alias x, z, z_prev or w", who);
        if (gt && gt_on_device && o0 < (const char*)gt + (size_t)c->B * c->N && (const char*)gt < o1)
            return fail(PNP_E_ARG, "%s: out must not alias gt", who);
        if ((uintptr_t)out % sizeof(double)) return fail(PNP_E_ARG, "%s: out is not aligned to 8 bytes", who);
    }
    if (int rc = trace_buffers(c, 1)) return rc;
    if (gt && !gt_on_device) {
        if (!c->gt) HIPCHK(hipMalloc((void**)&c->gt, (size_t)c->Bmax * c->N));
        if (int rc = copy_in(c, c->gt, gt, (size_t)c->B * c->N, 0)) return rc;
        gt = c->gt;
    }
    double* dst = out_on_device ? out : c->trace.rows;
    HIPCHK(launch_residuals<R>(c->stream, x, z, zp, w, gt, quantise != 0, c->B, c->N, c->N, false, c->trace.partial, c->trace.counter, dst));
    return out_on_device ? PNP_OK : copy_out(c, out, dst, row * sizeof(double), 0);
}

// What the next loop call runs (pnp_get_plan): the plans the engines themselves run by (loop_schedule.h).
static LoopPlan loop_plan(const pnp_ctx* c) {
    // a wavelet prox is two launches per shift of its group (pnp_set_spin; one without)
    const int spin_extra = c->wavelet != WV_NONE ? 2 * (spin_per_prox(c) - 1) : 0;
    if (c->coils.C > 0) return {1, c->B, coil_iteration_launches(c->coils.cg_iters, c->wavelet != WV_NONE) + spin_extra, false, 1, c->B};
    if (c->wavelet != WV_NONE) return {1, c->B, 5 + spin_extra, false, 1, c->B};   // the data-consistency step (three launches on every path) + the prox launches
    if (c->tp_frames) return {1, c->B, 4, false, 1, c->B};                         // ... + the one launch of the temporal prox
    switch (loop_path(c)) {
    case Path::generic: break;
    case Path::slice:   return plan_slice(c->B, c->sched);         // one launch per RUN: the iterations are a loop inside it
    case Path::fused:
        switch (c->eng.kind) {
        case Engine::fused256:  return plan_fused256(c->B, c->sched);
        case Engine::split_f32: return plan_chunked(c->B, c->sched, Chunked::split_f32);
        case Engine::split_f64: return plan_chunked(c->B, c->sched, Chunked::split_f64);
        case Engine::fused512:  return plan_chunked(c->B, c->sched, Chunked::fused512);
        case Engine::none:      break;
        }
        break;
    }
    return {1, c->B, 3, false, 1, c->B};                             // generic: rows, columns, rows
}

// the x (the caller's, or the ctx's own) and the ground truth (the caller's device array, or a copy of its host array) of a metric
template <typename X>
static int metric_inputs(pnp_ctx* c, const char* who, const X*& x, const uint8_t*& gt, int gt_on_device) {
    if (!x) {
        if (!c->have_x) return fail(PNP_E_STATE, "%s: x_dev is null and the ctx holds no x yet", who);
        x = bufs<X>(c).x;
        // complex images: the metrics are taken on |x|, formed into the context's real x (unused in complex mode)
        if (cx_mode(c)) HIPCHK(launch_cabs<X>(c->stream, state<X, true>(c).x, bufs<X>(c).x, (size_t)c->B * c->N));
    }
    if (!gt_on_device) {
        if (!c->gt) HIPCHK(hipMalloc((void**)&c->gt, (size_t)c->Bmax * c->N));
        if (int rc = copy_in(c, c->gt, gt, (size_t)c->B * c->N, 0)) return rc;
        gt = c->gt;
    }
    return PNP_OK;
}

template <typename X>
static int metrics_any(pnp_ctx* c, const X* x, const uint8_t* gt, int gt_on_device, double* psnr, double* re) {
    if (!gt || !psnr || !re) return fail(PNP_E_ARG, "pnp_metrics: null pointer");
    if (int rc = metric_inputs(c, "pnp_metrics", x, gt, gt_on_device)) return rc;
    HIPCHK(launch_metrics<X>(c->stream, x, gt, c->acc, c->B, (int)c->N));
    std::vector<double> h((size_t)c->B * 2);
    int rc = copy_out(c, h.data(), c->acc, h.size() * sizeof(double), 0);
    if (rc) return rc;
    for (int b = 0; b < c->B; ++b) {
        const double mse = h[2 * b] / (double)c->N;
        psnr[b] = (mse == 0.0) ? INFINITY : 20.0 * log10(255.0 / sqrt(mse));
        re[b] = sqrt(h[2 * b]) / sqrt(h[2 * b + 1]);
    }
    return PNP_OK;
}

template <typename X>
static int ssim_any(pnp_ctx* c, const X* x, const uint8_t* gt, int gt_on_device, double* ssim) {
    if (!gt || !ssim) return fail(PNP_E_ARG, "pnp_ssim: null pointer");
    if (int rc = metric_inputs(c, "pnp_ssim", x, gt, gt_on_device)) return rc;
    const int tiles = ((c->W - 10 + 15) / 16) * ((c->H - 10 + 15) / 16);
    if (!c->ssim_part) HIPCHK(hipMalloc((void**)&c->ssim_part, (size_t)c->Bmax * tiles * sizeof(double)));
    HIPCHK(launch_ssim<X>(c->stream, x, gt, c->ssim_part, c->B, c->H, c->W));
    std::vector<double> h((size_t)c->B * tiles);
    int rc = copy_out(c, h.data(), c->ssim_part, h.size() * sizeof(double), 0);
    if (rc) return rc;
    const double npix = (double)(c->H - 10) * (double)(c->W - 10);
    for (int b = 0; b < c->B; ++b) {
        double s = 0.0;
        for (int t = 0; t < tiles; ++t) s += h[(size_t)b * tiles + t];
        ssim[b] = s / npix;
    }
    return PNP_OK;
}

extern "C" {

int pnp_abi_version(void) { return PNP_ABI_VERSION; }
const char* pnp_last_error(void) { return g_err; }

int pnp_device_count(int* n) {
    if (!n) return fail(PNP_E_ARG, "pnp_device_count: null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { (void)hipGetLastError(); c = 0; }
    *n = c;
    return PNP_OK;
}

int pnp_device_info(int device, int* clock_mhz, int* compute_units, char* pci_bus_id, int pci_len, char* arch, int arch_len) {
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    if (clock_mhz) *clock_mhz = p.clockRate / 1000;
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (pci_bus_id && pci_len > 0) { pci_bus_id[0] = 0; HIPCHK(hipDeviceGetPCIBusId(pci_bus_id, pci_len, device)); }
    if (arch && arch_len > 0) { snprintf(arch, (size_t)arch_len, "%s", p.gcnArchName); }
    return PNP_OK;
}

int pnp_calibrate_stream(int device, int slices, double seconds, double* gbs) {
    if (!gbs || slices < 1 || slices > 4096 || !(seconds > 0.0) || seconds > 30.0) return fail(PNP_E_ARG, "pnp_calibrate_stream: 1 <= slices <= 4096, 0 < seconds <= 30, gbs non-null");
    HIPCHK(hipSetDevice(device));
    const size_t bytes = (size_t)slices << 18;
    float *z = nullptr, *w = nullptr, *y = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = PNP_OK;
    double moved = 0.0, ms_total = 0.0;
#define CAL(x) do { if (rc == PNP_OK) { hipError_t e_ = (x); if (e_ != hipSuccess) rc = fail(PNP_E_HIP, "pnp_calibrate_stream: %s: %s", #x, hipGetErrorString(e_)); } } while (0)
    CAL(hipMalloc((void**)&z, bytes)); CAL(hipMalloc((void**)&w, bytes)); CAL(hipMalloc((void**)&y, bytes));
    CAL(hipMemset(z, 0, bytes)); CAL(hipMemset(w, 0, bytes)); CAL(hipMemset(y, 0, bytes));
    CAL(hipEventCreate(&e0)); CAL(hipEventCreate(&e1));
    const int passes = 50;
    CAL(launch_calibrate_stream(nullptr, z, w, y, slices, 5));                           // warm-up
    CAL(hipDeviceSynchronize());
    while (rc == PNP_OK && ms_total < seconds * 1e3) {
        CAL(hipEventRecord(e0, nullptr));
        CAL(launch_calibrate_stream(nullptr, z, w, y, slices, passes));
        CAL(hipEventRecord(e1, nullptr));
        CAL(hipEventSynchronize(e1));
        float ms = 0.f;
        CAL(hipEventElapsedTime(&ms, e0, e1));
        ms_total += ms;
        moved += 5.0 * 262144.0 * slices * passes;
    }
#undef CAL
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (z) (void)hipFree(z);
    if (w) (void)hipFree(w);
    if (y) (void)hipFree(y);
    if (rc == PNP_OK) *gbs = moved / (ms_total * 1e-3) / 1e9;
    return rc;
}

// any_size: pnp_ctx_create_any[_f64] -- H, W in [128, 1024]; pnp_ctx_create[_f64] keep their contract of H, W in {256, 512}
static int ctx_create_impl(int device, int H, int W, int Bmax, pnp_ctx** out, bool f64, bool any_size) {
    if (!out) return fail(PNP_E_ARG, "pnp_ctx_create: out is null");
    *out = nullptr;
    const bool fixed = supported(H) && supported(W);
    if (!any_size && !fixed) return fail(PNP_E_ARG, "pnp_ctx_create: H, W must be 256 or 512 (got %dx%d; pnp_ctx_create_any takes 128..1024)", H, W);
    if (!fixed && !(anysize_supported(H) && anysize_supported(W)))
        return fail(PNP_E_ARG, "pnp_ctx_create_any: H, W must be 256 or 512, or both in [128, 1024] (got %dx%d)", H, W);
    if (Bmax < 1) return fail(PNP_E_ARG, "pnp_ctx_create: Bmax must be >= 1");
    Knobs kn;
    FusedSchedule sched0;
    if (int rk = read_knobs(&kn, &sched0)) return rk;
    HIPCHK(hipSetDevice(device));
    pnp_ctx* c = new (std::nothrow) pnp_ctx();
    if (!c) return fail(PNP_E_NOMEM, "pnp_ctx_create: host allocation failed");
    c->device = device; c->H = H; c->W = W; c->Bmax = Bmax; c->N = (size_t)H * W; c->f64 = f64;
    c->sched = sched0;
    const size_t BN = (size_t)Bmax * c->N, real = f64 ? sizeof(double) : sizeof(float);
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    for (void** p : {&c->y, &c->work}) alloc(p, BN * 2 * real);         // complex
    for (void** p : {&c->z, &c->w, &c->x}) alloc(p, BN * real);
    alloc((void**)&c->mask_id, (size_t)Bmax * sizeof(int32_t));
    alloc((void**)&c->acc, (size_t)Bmax * 2 * sizeof(double));
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = upload_twiddles();
    if (e == hipSuccess) e = upload_gauss();
    if (e == hipSuccess && !fixed) c->any = anysize_create(H, W, f64, &e);
    if (e != hipSuccess) {
        pnp_ctx_destroy(c);
        return fail(e == hipErrorOutOfMemory ? PNP_E_NOMEM : PNP_E_HIP, "pnp_ctx_create: %s", hipGetErrorString(e));
    }
    Engine& g = c->eng;
    if (H == 256 && W == 256) g.kind = f64 ? Engine::split_f64 : (kn.fused_cols == 2 ? Engine::split_f32 : Engine::fused256);
    else if (H == 512 && W == 512 && !f64) g.kind = Engine::fused512;
    hipError_t fe = hipSuccess;
    bool made = true;
    switch (g.kind) {
    case Engine::none:      break;
    case Engine::fused256:  made = (g.f256 = fused256_create(Bmax, &fe)) != nullptr; break;
    case Engine::split_f32: made = (g.s32 = fused256s_create<float>(Bmax, &fe)) != nullptr; break;
    case Engine::split_f64: made = (g.s64 = fused256s_create<double>(Bmax, &fe)) != nullptr; break;
    case Engine::fused512:  made = (g.f512 = fused512_create(Bmax, &fe)) != nullptr; break;
    }
    // Slice-resident loops: one workgroup (= one compute unit) per slice, so they pay off once the batch fills the chip; small batches
    // stay on the two-launch path, which spreads a slice over many CUs.  PNP_SLICE=0 never, =1 always, unset: batches of at least
    // PNP_SLICE_MIN_B slices (slice_pays()).
    if (made && g.kind == Engine::fused256 && kn.slice != 0) {
        g.slice_min_b = kn.slice == 1 ? 1 : kn.slice_min_b;
        if (Bmax >= g.slice_min_b) {
            g.slice = slice256_create(Bmax, kn.slice_pad_kb, kn.slice_yh_pad_kb, &fe);
            // no room for the slice-resident tables (256 KiB per slice on top of the two-launch tables): the context degrades to the
            // two-launch path (pnp_path_name says "fused") -- unless the caller forced PNP_SLICE=1
            if (!g.slice) { (void)hipGetLastError(); made = kn.slice != 1; }
        }
    }
    if (!made) {
        pnp_ctx_destroy(c);
        return fail(PNP_E_HIP, "pnp_ctx_create: fused path: %s", hipGetErrorString(fe));
    }
    *out = c;
    return PNP_OK;
}

int pnp_ctx_create(int device, int H, int W, int Bmax, pnp_ctx** out) { return ctx_create_impl(device, H, W, Bmax, out, false, false); }
int pnp_ctx_create_f64(int device, int H, int W, int Bmax, pnp_ctx** out) { return ctx_create_impl(device, H, W, Bmax, out, true, false); }
int pnp_ctx_create_any(int device, int H, int W, int Bmax, pnp_ctx** out) { return ctx_create_impl(device, H, W, Bmax, out, false, true); }
int pnp_ctx_create_any_f64(int device, int H, int W, int Bmax, pnp_ctx** out) { return ctx_create_impl(device, H, W, Bmax, out, true, true); }

int pnp_ctx_destroy(pnp_ctx* c) {
    if (!c) return PNP_OK;
    (void)hipSetDevice(c->device);
    switch (c->eng.kind) {
    case Engine::none:      break;
    case Engine::fused256:  fused256_destroy(c->eng.f256); break;
    case Engine::split_f32: fused256s_destroy(c->eng.s32); break;
    case Engine::split_f64: fused256s_destroy(c->eng.s64); break;
    case Engine::fused512:  fused512_destroy(c->eng.f512); break;
    }
    slice256_destroy(c->eng.slice);
    coils_free(c);
    anysize_destroy(c->any);
    void* ptrs[] = {c->y, c->work, c->z, c->w, c->x, c->mask_bank, c->mask_id, c->gt, c->acc, c->stage, c->ssim_part,
                    c->trace.partial, c->trace.counter, c->trace.rows, c->trace.zprev, c->trace.zc, c->trace.wc, c->wv_coef, c->wv_acc, c->tp_tw, c->maps_scratch};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (StageTimer* t : {&c->cm_t, &c->es_t})
        for (hipEvent_t e : t->ev) if (e) (void)hipEventDestroy(e);
    delete c;
    return PNP_OK;
}

int pnp_set_stream(pnp_ctx* c, void* s) { CTX(c); c->stream = (hipStream_t)s; return PNP_OK; }
int pnp_sync(pnp_ctx* c) { CTX(c); HIPCHK(hipStreamSynchronize(c->stream)); return PNP_OK; }
int pnp_set_fast_path(pnp_ctx* c, int enable) { CTX(c); c->fast = enable != 0; return PNP_OK; }
int pnp_get_schedule(pnp_ctx* c, int* queues, int* mixed_launches, int* chunk) {
    CTX(c);
    if (queues) *queues = c->sched.queues;
    if (mixed_launches) *mixed_launches = c->sched.mixed;
    if (chunk) *chunk = c->sched.chunk;
    return PNP_OK;
}
int pnp_set_schedule(pnp_ctx* c, int queues, int mixed_launches, int chunk) {
    CTX(c);
    if (queues < 1 || queues > 4) return fail(PNP_E_ARG, "pnp_set_schedule: queues in 1..4");
    c->sched.queues = queues; c->sched.mixed = mixed_launches != 0; c->sched.chunk = chunk;      // the other fields keep their values
    return PNP_OK;
}

int pnp_upload_problem(pnp_ctx* c, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device) {
    CTX(c); F32_ONLY(c); NO_COILS(c, "pnp_upload_problem_mc"); return upload_problem(c, __func__, y, mask_bank, mask_id, B, K, on_device);
}
int pnp_upload_problem_f64(pnp_ctx* c, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device) {
    CTX(c); F64_ONLY(c); NO_COILS(c, "pnp_upload_problem_mc_f64"); return upload_problem(c, __func__, y, mask_bank, mask_id, B, K, on_device);
}

int pnp_synthesize_problem(pnp_ctx* c, const float* img, const float* noise, int noise_per_slice,
                           const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device) {
    CTX(c); F32_ONLY(c); NO_COILS(c, "pnp_synthesize_problem_mc"); return synthesize_problem(c, __func__, img, noise, noise_per_slice, mask_bank, mask_id, B, K, on_device);
}
int pnp_synthesize_problem_f64(pnp_ctx* c, const float* img, const double* noise, int noise_per_slice,
                               const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device) {
    CTX(c); F64_ONLY(c); NO_COILS(c, "pnp_synthesize_problem_mc_f64"); return synthesize_problem(c, __func__, img, noise, noise_per_slice, mask_bank, mask_id, B, K, on_device);
}

int pnp_download_y(pnp_ctx* c, float* y, int on_device) { CTX(c); F32_ONLY(c); NEED_PROBLEM(c); return download_y(c, __func__, y, on_device); }
int pnp_download_y_f64(pnp_ctx* c, double* y, int on_device) { CTX(c); F64_ONLY(c); NEED_PROBLEM(c); return download_y(c, __func__, y, on_device); }

int pnp_init_state(pnp_ctx* c) {
    CTX(c); NEED_PROBLEM(c);
    c->spin_p = 0;                    // a fresh run starts the spin schedule over (pnp_set_state does not)
    c->lr_p = 0;                      // ... and the low-rank shift table
    return c->f64 ? init_state<double>(c) : init_state<float>(c);
}

int pnp_set_state(pnp_ctx* c, const float* z, const float* w, int on_device) { CTX(c); REAL_IMAGE(c, "pnp_set_state_cx"); F32_ONLY(c); NEED_PROBLEM(c); return set_state(c, __func__, z, w, on_device); }
int pnp_set_state_f64(pnp_ctx* c, const double* z, const double* w, int on_device) { CTX(c); REAL_IMAGE(c, "pnp_set_state_cx_f64"); F64_ONLY(c); NEED_PROBLEM(c); return set_state(c, __func__, z, w, on_device); }

int pnp_get_state(pnp_ctx* c, float* z, float* w, int on_device) { CTX(c); REAL_IMAGE(c, "pnp_get_state_cx"); F32_ONLY(c); NEED_PROBLEM(c); NEED_STATE(c); return get_state(c, z, w, on_device); }
int pnp_get_state_f64(pnp_ctx* c, double* z, double* w, int on_device) { CTX(c); REAL_IMAGE(c, "pnp_get_state_cx_f64"); F64_ONLY(c); NEED_PROBLEM(c); NEED_STATE(c); return get_state(c, z, w, on_device); }

// soft(a, thr) is evaluated as a - med3(a, -thr, thr) on the fast paths, which equals the reference's
// fmax(|a| - thr, 0) * sign(a) (S1:18-19) for thr >= 0 only; the reference's own parameters are all positive.
static int check_thresholds(const char* who, double alpha, double lambda1, double reo) {
    if (!(lambda1 >= 0.0)) return fail(PNP_E_ARG, "%s: lambda1 must be >= 0 (got %g)", who, lambda1);
    if (!(alpha >= 0.0)) return fail(PNP_E_ARG, "%s: alpha must be >= 0 (got %g)", who, alpha);
    if (!(reo > 0.0)) return fail(PNP_E_ARG, "%s: reo must be > 0 (got %g)", who, reo);
    return PNP_OK;
}
// the scalars of a CNC call: b first, as every such call has checked them
static int check_cnc(const char* who, double alpha, double lambda1, double reo, double b) {
    if (!(b > 0.0)) return fail(PNP_E_ARG, "%s: b must be > 0", who);
    return check_thresholds(who, alpha, lambda1, reo);
}

int pnp_admm_l1_run(pnp_ctx* c, int iters, double lambda1, double reo) {
    CTX(c); NEED_PROBLEM(c); NEED_STATE(c);
    Range r("pnp_admm_l1_run");
    if (int rv = check_thresholds(__func__, 0.0, lambda1, reo)) return rv;
    if (iters < 0) return fail(PNP_E_ARG, "%s: iters must be >= 0", __func__);
    return c->f64 ? run_loop(c, iters, false, prox_l1<double>(lambda1, reo), reo)
                  : run_loop(c, iters, false, prox_l1<float>(lambda1, reo), reo);
}

int pnp_admm_cnc_run(pnp_ctx* c, int iters, double alpha, double lambda1, double reo, double b) {
    CTX(c); NEED_PROBLEM(c); NEED_STATE(c);
    Range r("pnp_admm_cnc_run");
    if (int rv = check_cnc(__func__, alpha, lambda1, reo, b)) return rv;
    if (iters < 0) return fail(PNP_E_ARG, "%s: iters must be >= 0", __func__);
    return c->f64 ? run_loop(c, iters, true, prox_cnc<double>(alpha, lambda1, reo, b), reo)
                  : run_loop(c, iters, true, prox_cnc<float>(alpha, lambda1, reo, b), reo);
}

int pnp_admm_l1_run_traced(pnp_ctx* c, int iters, double lambda1, double reo, int every, double tol, const uint8_t* gt, int gt_on_device,
                           int* checks, int* iters_done) {
    CTX(c); NOT_IN_COMPLEX(c); NEED_PROBLEM(c); NEED_STATE(c);
    Range r("pnp_admm_l1_run_traced");
    if (int rv = check_thresholds(__func__, 0.0, lambda1, reo)) return rv;
    if (iters < 0) return fail(PNP_E_ARG, "%s: iters must be >= 0", __func__);
    return c->f64 ? run_traced<double>(c, __func__, iters, false, prox_l1<double>(lambda1, reo), reo, every, tol, gt, gt_on_device, checks, iters_done)
                  : run_traced<float>(c, __func__, iters, false, prox_l1<float>(lambda1, reo), reo, every, tol, gt, gt_on_device, checks, iters_done);
}

int pnp_admm_cnc_run_traced(pnp_ctx* c, int iters, double alpha, double lambda1, double reo, double b, int every, double tol,
                            const uint8_t* gt, int gt_on_device, int* checks, int* iters_done) {
    CTX(c); NOT_IN_COMPLEX(c); NEED_PROBLEM(c); NEED_STATE(c);
    Range r("pnp_admm_cnc_run_traced");
    if (int rv = check_cnc(__func__, alpha, lambda1, reo, b)) return rv;
    if (iters < 0) return fail(PNP_E_ARG, "%s: iters must be >= 0", __func__);
    return c->f64 ? run_traced<double>(c, __func__, iters, true, prox_cnc<double>(alpha, lambda1, reo, b), reo, every, tol, gt, gt_on_device, checks, iters_done)
                  : run_traced<float>(c, __func__, iters, true, prox_cnc<float>(alpha, lambda1, reo, b), reo, every, tol, gt, gt_on_device, checks, iters_done);
}

int pnp_trace_read(pnp_ctx* c, int32_t* iters, double* values, int32_t* converged_at) {
    CTX(c);
    const Trace& t = c->trace;
    if (iters) memcpy(iters, t.iters.data(), t.iters.size() * sizeof(int32_t));
    if (values) memcpy(values, t.values.data(), t.values.size() * sizeof(double));
    if (converged_at) memcpy(converged_at, t.converged_at.data(), t.converged_at.size() * sizeof(int32_t));
    return PNP_OK;
}

int pnp_residuals(pnp_ctx* c, const float* x, const float* z, const float* zprev, const float* w, const uint8_t* gt, int gt_on_device,
                  int quantise, double* out, int out_on_device) {
    CTX(c); NOT_IN_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c);
    return residuals_any<float>(c, __func__, x, z, zprev, w, gt, gt_on_device, quantise, out, out_on_device);
}
int pnp_residuals_f64(pnp_ctx* c, const double* x, const double* z, const double* zprev, const double* w, const uint8_t* gt, int gt_on_device,
                      int quantise, double* out, int out_on_device) {
    CTX(c); NOT_IN_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c);
    return residuals_any<double>(c, __func__, x, z, zprev, w, gt, gt_on_device, quantise, out, out_on_device);
}

int pnp_download_x(pnp_ctx* c, float* x, int on_device) { CTX(c); REAL_IMAGE(c, "pnp_download_x_cx"); F32_ONLY(c); NEED_PROBLEM(c); return download_x(c, __func__, x, on_device); }
int pnp_download_x_f64(pnp_ctx* c, double* x, int on_device) { CTX(c); REAL_IMAGE(c, "pnp_download_x_cx_f64"); F64_ONLY(c); NEED_PROBLEM(c); return download_x(c, __func__, x, on_device); }

int pnp_dc_step(pnp_ctx* c, const float* z, const float* w, float* x, double reo) {
    CTX(c); REAL_IMAGE(c, "pnp_dc_step_cx"); F32_ONLY(c); NEED_PROBLEM(c);
    Range r("pnp_dc_step");
    return dc_step<float, false>(c, __func__, z, w, x, reo);
}

// The real prox calls name a null pointer before a bad scalar, the _cx calls after it (prox_dual): that check stays here, in its place.
int pnp_prox_l1_dual(pnp_ctx* c, const float* x, float* z, float* w, double thr) {
    CTX(c); REAL_IMAGE(c, "pnp_prox_l1_dual_cx"); F32_ONLY(c); NEED_PROBLEM(c);
    if (!x || !z || !w) return fail(PNP_E_ARG, "%s: null pointer", __func__);
    if (!(thr >= 0.0)) return fail(PNP_E_ARG, "%s: thr must be >= 0", __func__);
    ProxParams p{}; p.thr = (float)thr;
    return prox_dual<float, false>(c, __func__, false, x, z, w, p);
}

int pnp_prox_cnc_dual(pnp_ctx* c, const float* x, float* z, float* w, double alpha, double lambda1, double reo, double b) {
    CTX(c); REAL_IMAGE(c, "pnp_prox_cnc_dual_cx"); F32_ONLY(c); NEED_PROBLEM(c);
    if (!x || !z || !w) return fail(PNP_E_ARG, "%s: null pointer", __func__);
    if (int rv = check_cnc(__func__, alpha, lambda1, reo, b)) return rv;
    return prox_dual<float, false>(c, __func__, true, x, z, w, prox_cnc<float>(alpha, lambda1, reo, b));
}

int pnp_cnc_combine(pnp_ctx* c, const float* z, const float* x, const float* w, const float* s, float* t,
                    double alpha, double lambda1, double reo, double b) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!z || !x || !w || !s || !t) return fail(PNP_E_ARG, "pnp_cnc_combine: null pointer");
    HIPCHK(launch_combine(c->stream, z, x, w, s, t, (float)(1.0 - alpha), (float)alpha,
                          (float)(alpha * reo * lambda1 * b), (size_t)c->B * c->N));
    return PNP_OK;
}

int pnp_add(pnp_ctx* c, const float* a, const float* b, float* o) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!a || !b || !o) return fail(PNP_E_ARG, "pnp_add: null pointer");
    HIPCHK(launch_add(c->stream, a, b, o, (size_t)c->B * c->N));
    return PNP_OK;
}

int pnp_dual_clamp(pnp_ctx* c, float* x, float* z, float* w) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!x || !z || !w) return fail(PNP_E_ARG, "pnp_dual_clamp: null pointer");
    HIPCHK(launch_dual_clamp(c->stream, x, z, w, (size_t)c->B * c->N));
    return PNP_OK;
}

extern "C++" {
// the 2-D transform of B <= Bmax slices, arguments unchecked: rows in -> out, columns in place, 1/N on the inverse
template <typename R>
static int fft2_run(pnp_ctx* c, const typename CxOf<R>::type* in, typename CxOf<R>::type* out, int B, bool inv) {
    RowArgsT<R> ra{};
    ra.cin = in; ra.cout = out; ra.scale = inv ? R(1) / (R)c->N : R(1); ra.nrows = B * c->H;
    HIPCHK(rows<R>(c, IN_COMPLEX, inv, EPI_COMPLEX, ra));
    ColArgsT<R> ca{};
    ca.in = out; ca.out = out; ca.B = B;
    HIPCHK(cols<R>(c, !inv, MID_NONE, inv, ca));
    return PNP_OK;
}

// the inverse transform of `count` pseudo-slices, src -> dst, in chunks of at most Bmax
template <typename R>
static int ifft2_chunks(pnp_ctx* c, const typename CxOf<R>::type* src, typename CxOf<R>::type* dst, int count) {
    for (int s0 = 0; s0 < count; s0 += c->Bmax)
        if (int rc = fft2_run<R>(c, src + (size_t)s0 * c->N, dst + (size_t)s0 * c->N, count - s0 < c->Bmax ? count - s0 : c->Bmax, true)) return rc;
    return PNP_OK;
}
}  // extern "C++"

static int fft2_any(pnp_ctx* c, const float* in, float* out, int B, bool inv) {
    if (!in || !out) return fail(PNP_E_ARG, "fft2: null pointer");
    if (B < 1 || B > c->Bmax) return fail(PNP_E_ARG, "fft2: B=%d out of range [1,%d]", B, c->Bmax);
    return fft2_run<float>(c, (const float2*)in, (float2*)out, B, inv);
}

int pnp_fft2_fwd(pnp_ctx* c, const float* in, float* out, int B) { CTX(c); F32_ONLY(c); return fft2_any(c, in, out, B, false); }
int pnp_fft2_inv(pnp_ctx* c, const float* in, float* out, int B) { CTX(c); F32_ONLY(c); return fft2_any(c, in, out, B, true); }

int pnp_A(pnp_ctx* c, const float* x, float* k) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!x || !k) return fail(PNP_E_ARG, "pnp_A: null pointer");
    if (c->coils.C > 0) {                              // k: [B][C][H][W]
        CoilRowArgsT<float> ca = coil_rows<float>(c, c->B);
        ca.rin = x; ca.work = (float2*)k;
        HIPCHK(anysize_coil_rows_in<float>(c->coils.any, c->stream, ca));
        HIPCHK(anysize_cols<float>(c->coils.any, c->stream, true, MID_MASK, false, coil_cols<float>(c, k, k)));
        return PNP_OK;
    }
    RowArgs ra{};
    ra.rin0 = x; ra.cout = (float2*)k; ra.scale = 1.0f; ra.nrows = c->B * c->H;
    HIPCHK(rows<float>(c, IN_REAL, false, EPI_COMPLEX, ra));
    ColArgs ca{};
    ca.in = (const float2*)k; ca.out = (float2*)k; ca.mask_bank = c->mask_bank; ca.mask_id = c->mask_id; ca.B = c->B;
    HIPCHK(cols<float>(c, true, MID_MASK, false, ca));
    return PNP_OK;
}

int pnp_AH(pnp_ctx* c, const float* k, float* out) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!k || !out) return fail(PNP_E_ARG, "pnp_AH: null pointer");
    if (c->coils.C > 0) return coil_AH<float>(c, k, out);
    ColArgs ca{};
    ca.in = (const float2*)k; ca.out = (float2*)out; ca.mask_bank = c->mask_bank; ca.mask_id = c->mask_id; ca.B = c->B;
    HIPCHK(cols<float>(c, false, MID_MASK, true, ca));
    RowArgs ra{};
    ra.cin = (const float2*)out; ra.cout = (float2*)out; ra.scale = 1.0f / (float)c->N; ra.nrows = c->B * c->H;
    HIPCHK(rows<float>(c, IN_COMPLEX, true, EPI_COMPLEX, ra));
    return PNP_OK;
}

int pnp_Df(pnp_ctx* c, const float* x, float* out) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!x || !out) return fail(PNP_E_ARG, "pnp_Df: null pointer");
    if (c->coils.C > 0) return fail(PNP_E_STATE, "pnp_Df: not available on a context with coils (pnp_set_coils); compose it from pnp_A and pnp_AH");
    RowArgs ra{};
    ra.rin0 = x; ra.cout = (float2*)out; ra.scale = 1.0f; ra.nrows = c->B * c->H;
    HIPCHK(rows<float>(c, IN_REAL, false, EPI_COMPLEX, ra));
    ColArgs ca{};
    ca.in = (const float2*)out; ca.out = (float2*)out; ca.y = bufs<float>(c).y; ca.mask_bank = c->mask_bank; ca.mask_id = c->mask_id; ca.B = c->B;
    HIPCHK(cols<float>(c, true, MID_RESID, true, ca));
    RowArgs rb{};
    rb.cin = (const float2*)out; rb.cout = (float2*)out; rb.scale = 1.0f / (float)c->N; rb.nrows = c->B * c->H;
    HIPCHK(rows<float>(c, IN_COMPLEX, true, EPI_COMPLEX, rb));
    return PNP_OK;
}

int pnp_metrics(pnp_ctx* c, const float* x, const uint8_t* gt, int gt_on_device, double* psnr, double* re) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    return metrics_any<float>(c, x, gt, gt_on_device, psnr, re);
}
int pnp_ssim(pnp_ctx* c, const float* x, const uint8_t* gt, int gt_on_device, double* ssim) {
    CTX(c); F32_ONLY(c); NEED_PROBLEM(c);
    return ssim_any<float>(c, x, gt, gt_on_device, ssim);
}
int pnp_metrics_f64(pnp_ctx* c, const double* x, const uint8_t* gt, int gt_on_device, double* psnr, double* re) {
    CTX(c); F64_ONLY(c); NEED_PROBLEM(c);
    return metrics_any<double>(c, x, gt, gt_on_device, psnr, re);
}
int pnp_ssim_f64(pnp_ctx* c, const double* x, const uint8_t* gt, int gt_on_device, double* ssim) {
    CTX(c); F64_ONLY(c); NEED_PROBLEM(c);
    return ssim_any<double>(c, x, gt, gt_on_device, ssim);
}

int pnp_is_f64(pnp_ctx* c) { return (c && c->f64) ? 1 : 0; }

int pnp_timer_start(pnp_ctx* c) { CTX(c); HIPCHK(hipEventRecord(c->ev0, c->stream)); return PNP_OK; }
int pnp_timer_stop(pnp_ctx* c, float* ms) {
    CTX(c);
    if (!ms) return fail(PNP_E_ARG, "pnp_timer_stop: null");
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return PNP_OK;
}

// Build now whatever per-problem tables the loops (pnp_admm_*_run) of the uploaded problem will use; they are otherwise built
// by the first loop call (256x256 float contexts only -- every other path prepares at upload).  Benchmarks call it so that a
// timed region with no warm-up holds iterations only.
int pnp_prepare_loops(pnp_ctx* c) { CTX(c); NEED_PROBLEM(c); return ensure_tables(c, loop_path(c)); }

int pnp_get_plan(pnp_ctx* c, int* queues, int* chunk, int* launches_per_iteration) {
    CTX(c);
    const LoopPlan p = loop_plan(c);
    if (queues) *queues = p.queues;
    if (chunk) *chunk = p.chunk;
    if (launches_per_iteration) *launches_per_iteration = p.launches;
    return PNP_OK;
}

int pnp_kernels_per_iteration(pnp_ctx* c) { return c ? loop_plan(c).launches : 0; }

const char* pnp_ctx_path(pnp_ctx* c) {
    if (c && c->any) return "anysize";
    return pnp_path_name(c);
}

int pnp_fft_plan(pnp_ctx* c, int axis, char* buf, int len) {
    if (!c || !buf || len < 1 || axis < 0 || axis > 1) return fail(PNP_E_ARG, "pnp_fft_plan: ctx / buf null, len < 1 or axis not 0 or 1");
    if (c->any) { anysize_describe(c->any, axis, buf, len); return PNP_OK; }
    snprintf(buf, (size_t)len, "fixed %d", axis == 0 ? c->W : c->H);
    return PNP_OK;
}

const char* pnp_path_name(pnp_ctx* c) {
    if (!c) return "generic";
    if (c->coils.C > 0) return "coils";
    switch (loop_path(c)) {
    case Path::generic: return "generic";
    case Path::slice:   return natural_loop(c) ? "fused" : "slice";            // with a wavelet or frames set the loops never run slice-resident
    case Path::fused:   return "fused";
    }
    return "generic";
}

int pnp_sparsity_check(int wavelet, int levels, int H, int W) {
    if (wavelet == PNP_WAVELET_NONE) return PNP_OK;
    switch (wv_check(wavelet, levels, H, W)) {
    case WV_OK:          return PNP_OK;
    case WV_BAD_NAME:    return fail(PNP_E_ARG, "sparsity: wavelet must be PNP_WAVELET_NONE, _HAAR, _DB2 or _DB4 (got %d)", wavelet);
    case WV_BAD_LEVELS:  return fail(PNP_E_ARG, "sparsity: levels must be 1..%d (got %d)", WV_MAX_LEVELS, levels);
    case WV_BAD_DIVISOR: return fail(PNP_E_ARG, "sparsity: H and W must be divisible by 2^levels = %d (got %d x %d)", 1 << levels, H, W);
    default:             return fail(PNP_E_ARG, "sparsity: the input of level %d is %d samples, shorter than the filter (%d taps)", levels,
                                     (H < W ? H : W) >> (levels - 1), wv_taps(wavelet));
    }
}

int pnp_set_sparsity(pnp_ctx* c, int wavelet, int levels) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (int rc = pnp_sparsity_check(wavelet, levels, c->H, c->W)) return rc;         // before any device work
    if (wavelet != PNP_WAVELET_NONE && c->tp_frames)
        return fail(PNP_E_STATE, "%s: a wavelet does not run with temporal sparsity (clear it with pnp_set_temporal(ctx, 0, 1))", __func__);
    if (cx_mode(c)) if (int rc = pnp_image_check(PNP_IMAGE_COMPLEX, wavelet, levels, c->f64)) return rc;
    CTX(c);
    if (wavelet != PNP_WAVELET_NONE) if (int rc = wavelet_scratch(c)) return rc;
    if (wavelet != PNP_WAVELET_NONE && cx_mode(c)) if (int rc = wavelet_scratch(c, true, __func__)) return rc;
    c->wavelet = wavelet;
    c->wv_levels = wavelet == PNP_WAVELET_NONE ? 0 : levels;
    c->spin.clear(); c->spin_k = 1; c->spin_p = 0;                                    // the valid shifts depend on levels
    return PNP_OK;
}

int pnp_get_sparsity(pnp_ctx* c, int* wavelet, int* levels) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (wavelet) *wavelet = c->wavelet;
    if (levels) *levels = c->wv_levels;
    return PNP_OK;
}

int pnp_dwt2_fwd(pnp_ctx* c, const float* in, float* out, int B) { CTX(c); F32_ONLY(c); return dwt2_any<float>(c, __func__, in, out, B, false); }
int pnp_dwt2_inv(pnp_ctx* c, const float* in, float* out, int B) { CTX(c); F32_ONLY(c); return dwt2_any<float>(c, __func__, in, out, B, true); }
int pnp_dwt2_fwd_f64(pnp_ctx* c, const double* in, double* out, int B) { CTX(c); F64_ONLY(c); return dwt2_any<double>(c, __func__, in, out, B, false); }
int pnp_dwt2_inv_f64(pnp_ctx* c, const double* in, double* out, int B) { CTX(c); F64_ONLY(c); return dwt2_any<double>(c, __func__, in, out, B, true); }

// ---- cycle spinning for the wavelet prox (wavelet_plan.h, wv_spin_check) ----

int pnp_spin_check(int levels, const int32_t* shifts, int n, int per_prox) {
    switch (wv_spin_check(levels, shifts, n, per_prox)) {
    case WV_SPIN_OK:           return PNP_OK;
    case WV_SPIN_BAD_LEVELS:   return fail(PNP_E_ARG, "spin: levels must be 1..%d (got %d)", WV_MAX_LEVELS, levels);
    case WV_SPIN_BAD_N:        return fail(PNP_E_ARG, "spin: n must be 1..%d with a table of n shifts (got %d%s)", WV_SPIN_MAX_N, n, shifts ? "" : ", null table");
    case WV_SPIN_BAD_K:        return fail(PNP_E_ARG, "spin: per_prox must be 1..%d (got %d)", WV_SPIN_MAX_K, per_prox);
    case WV_SPIN_BAD_MULTIPLE: return fail(PNP_E_ARG, "spin: the table length must be a multiple of the group size (got %d shifts, groups of %d)", n, per_prox);
    default:
        for (int i = 0; i < n; ++i)
            if (!wv_shift_ok(levels, shifts[2 * i], shifts[2 * i + 1]))
                return fail(PNP_E_ARG, "spin: shift %d = (%d, %d) out of range [0, %d) (2^levels)", i, shifts[2 * i], shifts[2 * i + 1], 1 << levels);
        return fail(PNP_E_ARG, "spin: shift out of range");
    }
}

int pnp_set_spin(pnp_ctx* c, const int32_t* shifts, int n, int per_prox) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (n == 0) { c->spin.clear(); c->spin_k = 1; c->spin_p = 0; return PNP_OK; }
    NOT_IN_COMPLEX(c);
    if (c->tp_frames) return fail(PNP_E_STATE, "%s: a spin table does not run with temporal sparsity (clear it with pnp_set_temporal(ctx, 0, 1))", __func__);
    if (c->wavelet == WV_NONE) return fail(PNP_E_STATE, "%s: no wavelet set (pnp_set_sparsity)", __func__);
    if (int rc = pnp_spin_check(c->wv_levels, shifts, n, per_prox)) return rc;          // before any device work
    CTX(c);
    if (per_prox > 1 && !c->wv_acc) HIPCHK(hipMalloc(&c->wv_acc, (size_t)c->Bmax * c->N * (c->f64 ? sizeof(double) : sizeof(float))));
    c->spin.assign(shifts, shifts + 2 * (size_t)n);
    c->spin_k = per_prox;
    c->spin_p = 0;
    return PNP_OK;
}

int pnp_get_spin(pnp_ctx* c, int* n, int* per_prox, int* cursor) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (n) *n = (int)(c->spin.size() / 2);
    if (per_prox) *per_prox = spin_per_prox(c);
    if (cursor) *cursor = c->spin_p;
    return PNP_OK;
}

int pnp_set_spin_cursor(pnp_ctx* c, int cursor) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (c->spin.empty()) return fail(PNP_E_STATE, "%s: no spin setting (pnp_set_spin)", __func__);
    if (cursor < 0) return fail(PNP_E_ARG, "%s: cursor must be >= 0 (got %d)", __func__, cursor);
    c->spin_p = cursor;
    return PNP_OK;
}

// ---- temporal sparsity (temporal_plan.h, kernels_temporal.hip) ----

static void lowrank_clear(pnp_ctx* c) { c->lr_block = 0; c->lr_scale = 1.0; c->lr_shifts.clear(); c->lr_p = 0; }

int pnp_temporal_check(int frames, int B) {
    switch (tp_check(frames, B)) {
    case TP_OK:         return PNP_OK;
    case TP_BAD_FRAMES: return fail(PNP_E_ARG, "temporal: frames must be %d..%d (got %d)", TP_MIN_FRAMES, TP_MAX_FRAMES, frames);
    case TP_BAD_BATCH:  return fail(PNP_E_STATE, "temporal: the batch of %d slices is not a whole number of series of %d frames", B, frames);
    }
    return fail(PNP_E_ARG, "temporal: invalid setting");
}

int pnp_set_temporal(pnp_ctx* c, int frames, int keep_dc) {
    CTX(c);
    if (frames == 0) { c->tp_frames = 0; c->tp_keep_dc = true; lowrank_clear(c); return PNP_OK; }
    if (int rc = pnp_temporal_check(frames, frames)) return rc;                       // the range alone, before any device work
    if (c->lr_block) if (int rc = pnp_lowrank_check(frames, c->lr_block, c->H, c->W, frames, c->f64 ? 1 : 0, 0)) return rc;   // the block must fit the new length
    if (c->wavelet != WV_NONE)
        return fail(PNP_E_STATE, "%s: temporal sparsity does not run with a wavelet%s (clear it with pnp_set_sparsity(ctx, PNP_WAVELET_NONE, 0))",
                    __func__, c->spin.empty() ? "" : " and its spin table");
    const size_t real = c->f64 ? sizeof(double) : sizeof(float);
    if (!c->tp_tw)
        if (int rc = alloc_or_fail(&c->tp_tw, TP_MATRIX_MAX * real, __func__, "twiddle matrix", "frames=%d", frames)) return rc;
    const size_t count = 2 * (size_t)frames * frames;
    std::vector<double> tw64(c->f64 ? count : 0);
    std::vector<float> tw32(c->f64 ? 0 : count);
    if (c->f64) tp_twiddle_matrix<double>(frames, tw64.data()); else tp_twiddle_matrix<float>(frames, tw32.data());
    c->tp_frames = 0;                                                                   // no setting if the copy fails
    // copy_in of a host array synchronises, so the vectors may die at the end of this call
    if (int rc = copy_in(c, c->tp_tw, c->f64 ? (const void*)tw64.data() : (const void*)tw32.data(), count * real, 0)) return rc;
    c->tp_frames = frames;
    c->tp_keep_dc = keep_dc != 0;
    return PNP_OK;
}

int pnp_get_temporal(pnp_ctx* c, int* frames, int* keep_dc) {
    CTX(c);
    if (frames) *frames = c->tp_frames;
    if (keep_dc) *keep_dc = c->tp_keep_dc ? 1 : 0;
    return PNP_OK;
}

// ---- locally low-rank prox (lowrank_plan.h, kernels_lowrank.hip) ----

int pnp_lowrank_check(int frames, int block, int H, int W, int B, int f64, int cnc) {
    switch (lr_check(frames, block, H, W, B, f64 ? sizeof(double) : sizeof(float), cnc != 0)) {
    case LR_OK:         return PNP_OK;
    case LR_BAD_FRAMES: return pnp_temporal_check(frames, frames);
    case LR_BAD_BLOCK:  return fail(PNP_E_ARG, "lowrank: block must be %d..%d (got %d)", LR_MIN_BLOCK, LR_MAX_BLOCK, block);
    case LR_BAD_SHAPE:  return fail(PNP_E_ARG, "lowrank: block %d exceeds the image (%d x %d)", block, H, W);
    case LR_BAD_LDS:    return fail(PNP_E_ARG, "lowrank: a patch of %d x %d pixels over %d frames does not fit the LDS of a workgroup in %s (%s)",
                                    block, block, frames, f64 ? "double" : "float", cnc ? "CNC" : "L1");
    case LR_BAD_BATCH:  return pnp_temporal_check(frames, B);
    }
    return fail(PNP_E_ARG, "lowrank: invalid setting");
}

int pnp_set_lowrank(pnp_ctx* c, int block, double scale, const int32_t* shifts, int n_shifts) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (block == 0) { lowrank_clear(c); return PNP_OK; }
    NOT_IN_COMPLEX(c);
    if (!c->tp_frames) return fail(PNP_E_STATE, "%s: no series length set (pnp_set_temporal)", __func__);
    if (int rc = pnp_lowrank_check(c->tp_frames, block, c->H, c->W, c->tp_frames, c->f64 ? 1 : 0, 0)) return rc;
    if (!(scale > 0.0) || !(scale <= 1e30)) return fail(PNP_E_ARG, "%s: scale must be a positive number (got %g)", __func__, scale);
    if (!shifts || n_shifts < 1 || n_shifts > LR_MAX_SHIFTS)
        return fail(PNP_E_ARG, "%s: shifts must be a table of 1..%d pairs (got %d%s)", __func__, LR_MAX_SHIFTS, n_shifts, shifts ? "" : ", null");
    for (int i = 0; i < n_shifts; ++i)
        if (!lr_shift_ok(block, shifts[2 * i], shifts[2 * i + 1]))
            return fail(PNP_E_ARG, "%s: shift %d = (%d, %d) out of range [0, %d)", __func__, i, shifts[2 * i], shifts[2 * i + 1], block);
    c->lr_block = block;
    c->lr_scale = scale;
    c->lr_shifts.assign(shifts, shifts + 2 * (size_t)n_shifts);
    c->lr_p = 0;
    return PNP_OK;
}

int pnp_get_lowrank(pnp_ctx* c, int* block, double* scale, int* n_shifts, int* cursor) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (block) *block = c->lr_block;
    if (scale) *scale = c->lr_scale;
    if (n_shifts) *n_shifts = (int)(c->lr_shifts.size() / 2);
    if (cursor) *cursor = c->lr_p;
    return PNP_OK;
}

int pnp_set_lowrank_cursor(pnp_ctx* c, int cursor) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (!c->lr_block) return fail(PNP_E_STATE, "%s: no low-rank setting (pnp_set_lowrank)", __func__);
    if (cursor < 0) return fail(PNP_E_ARG, "%s: cursor must be >= 0 (got %d)", __func__, cursor);
    c->lr_p = cursor;
    return PNP_OK;
}

int pnp_dwt2_shifted(pnp_ctx* c, const float* in, float* out, int B, int inverse, int sy, int sx) {
    CTX(c); F32_ONLY(c); return dwt2_any<float>(c, __func__, in, out, B, inverse != 0, sy, sx);
}
int pnp_dwt2_shifted_f64(pnp_ctx* c, const double* in, double* out, int B, int inverse, int sy, int sx) {
    CTX(c); F64_ONLY(c); return dwt2_any<double>(c, __func__, in, out, B, inverse != 0, sy, sx);
}

// ---- multi-coil (SENSE) data consistency ----

int pnp_coils_check(int C, int Ks, int H, int W) {
    switch (coil_check(C, Ks, H, W)) {
    case COIL_OK:       return PNP_OK;
    case COIL_BAD_C:    return fail(PNP_E_ARG, "coils: C must be 1..%d (got %d)", COIL_MAX_C, C);
    case COIL_BAD_SETS: return fail(PNP_E_ARG, "coils: Ks must be >= 1 (got %d)", Ks);
    default:            return fail(PNP_E_ARG, "coils: H, W must be in [128, 1024] (got %d x %d)", H, W);
    }
}

static int set_coils_checked(pnp_ctx* c, const char* who, const void* sens, int C, int Ks, int on_device, bool f64) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", who);
    if (C != 0) {
        if (int rc = pnp_coils_check(C, Ks, c->H, c->W)) return rc;                  // before any device work
        if (!sens) return fail(PNP_E_ARG, "%s: sens is null", who);
    }
    if (c->f64 != f64) return fail(PNP_E_STATE, f64 ? "%s: needs a context made by pnp_ctx_create_f64" : "%s: not available on an fp64 validation context", who);
    HIPCHK(hipSetDevice(c->device));
    return f64 ? set_coils<double>(c, who, (const double*)sens, C, Ks, on_device) : set_coils<float>(c, who, (const float*)sens, C, Ks, on_device);
}
int pnp_set_coils(pnp_ctx* c, const float* sens, int C, int Ks, int on_device) { return set_coils_checked(c, __func__, sens, C, Ks, on_device, false); }
int pnp_set_coils_f64(pnp_ctx* c, const double* sens, int C, int Ks, int on_device) { return set_coils_checked(c, __func__, sens, C, Ks, on_device, true); }

int pnp_set_cg(pnp_ctx* c, int iters) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (iters < 1 || iters > CG_MAX_ITERS) return fail(PNP_E_ARG, "pnp_set_cg: iters must be 1..%d (got %d)", CG_MAX_ITERS, iters);
    c->coils.cg_iters = iters;
    return PNP_OK;
}

int pnp_get_coils(pnp_ctx* c, int* C, int* Ks, int* cg_iters) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (C) *C = c->coils.C;
    if (Ks) *Ks = c->coils.Ks;
    if (cg_iters) *cg_iters = c->coils.cg_iters;
    return PNP_OK;
}

int pnp_upload_problem_mc(pnp_ctx* c, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, const int32_t* coil_id, int B, int K, int on_device) {
    CTX(c); F32_ONLY(c); NEED_COILS(c); return upload_problem_mc<float>(c, __func__, y, mask_bank, mask_id, coil_id, B, K, on_device);
}
int pnp_upload_problem_mc_f64(pnp_ctx* c, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, const int32_t* coil_id, int B, int K, int on_device) {
    CTX(c); F64_ONLY(c); NEED_COILS(c); return upload_problem_mc<double>(c, __func__, y, mask_bank, mask_id, coil_id, B, K, on_device);
}
int pnp_synthesize_problem_mc(pnp_ctx* c, const float* img, const float* noise, int noise_mode, const uint8_t* mask_bank, const int32_t* mask_id,
                              const int32_t* coil_id, int B, int K, int on_device) {
    CTX(c); F32_ONLY(c); NEED_COILS(c); return synthesize_problem_mc<float>(c, __func__, img, noise, noise_mode, mask_bank, mask_id, coil_id, B, K, on_device);
}
int pnp_synthesize_problem_mc_f64(pnp_ctx* c, const float* img, const double* noise, int noise_mode, const uint8_t* mask_bank, const int32_t* mask_id,
                                  const int32_t* coil_id, int B, int K, int on_device) {
    CTX(c); F64_ONLY(c); NEED_COILS(c); return synthesize_problem_mc<double>(c, __func__, img, noise, noise_mode, mask_bank, mask_id, coil_id, B, K, on_device);
}

int pnp_cg_residual(pnp_ctx* c, double* rel) {
    CTX(c); NEED_COILS(c); NEED_PROBLEM(c);
    if (!rel) return fail(PNP_E_ARG, "pnp_cg_residual: rel is null");
    if (!c->coils.have_rel) return fail(PNP_E_STATE, "pnp_cg_residual: no x-step has run on the uploaded problem");
    return copy_out(c, rel, c->coils.rel, (size_t)c->B * sizeof(double), 0);
}

// ---- complex-valued images on a coil context: kernels_complex.hip, the CX roles of kernels_coils.hip ----

int pnp_image_check(int mode, int wavelet, int levels, int f64) {
    if (mode != PNP_IMAGE_REAL && mode != PNP_IMAGE_COMPLEX)
        return fail(PNP_E_ARG, "image: mode must be PNP_IMAGE_REAL (0) or PNP_IMAGE_COMPLEX (1) (got %d)", mode);
    if (mode == PNP_IMAGE_COMPLEX && wavelet != PNP_WAVELET_NONE && wv_taps(wavelet) != 0 && levels >= 1 && levels <= WV_MAX_LEVELS &&
        !wavelet_cx_fits(wavelet, levels, f64 != 0))
        return fail(PNP_E_ARG, "image: with complex images the tile of this wavelet at %d levels does not fit the LDS in %s", levels, f64 ? "double" : "float");
    return PNP_OK;
}

int pnp_set_image(pnp_ctx* c, int mode) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (int rc = pnp_image_check(mode, PNP_WAVELET_NONE, 0, 0)) return rc;
    if (mode == PNP_IMAGE_COMPLEX) {
        if (c->coils.C == 0) return fail(PNP_E_STATE, "%s: complex images need a context with coils (pnp_set_coils)", __func__);
        if (!c->spin.empty()) return fail(PNP_E_STATE, "%s: complex images do not run with a spin table (clear it with pnp_set_spin(ctx, NULL, 0, 1))", __func__);
        if (c->lr_block) return fail(PNP_E_STATE, "%s: complex images do not run with a low-rank block (clear it with pnp_set_lowrank(ctx, 0, 0, NULL, 0))", __func__);
        if (int rc = pnp_image_check(mode, c->wavelet, c->wv_levels, c->f64)) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->B = 0; c->prob = Problem{};                        // the uploaded problem is dropped, as by pnp_set_coils
    c->state_sliced = c->have_x = c->have_state = false;
    c->coils.have_rel = false;
    if (mode == PNP_IMAGE_COMPLEX && !c->zc) {
        const size_t bytes = (size_t)c->Bmax * c->N * 2 * (c->f64 ? sizeof(double) : sizeof(float));
        void** want[] = {&c->zc, &c->wc, &c->xc};
        for (void** p : want)
            if (int rc = alloc_or_fail(p, bytes, __func__, "complex state", "Bmax=%d, %dx%d", c->Bmax, c->H, c->W)) {
                for (void** q : want) { if (*q) (void)hipFree(*q); *q = nullptr; }
                return rc;
            }
    }
    if (mode == PNP_IMAGE_COMPLEX && c->wavelet != WV_NONE) if (int rc = wavelet_scratch(c, true, __func__)) return rc;
    c->image = mode;
    return PNP_OK;
}

int pnp_get_image(pnp_ctx* c, int* mode) {
    if (!c) return fail(PNP_E_ARG, "%s: ctx is null", __func__);
    if (mode) *mode = c->image;
    return PNP_OK;
}

int pnp_set_state_cx(pnp_ctx* c, const float* z, const float* w, int on_device) { CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c); return set_state<float, true>(c, __func__, z, w, on_device); }
int pnp_set_state_cx_f64(pnp_ctx* c, const double* z, const double* w, int on_device) { CTX(c); NEED_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c); return set_state<double, true>(c, __func__, z, w, on_device); }
int pnp_get_state_cx(pnp_ctx* c, float* z, float* w, int on_device) { CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c); NEED_STATE(c); return get_state<float, true>(c, z, w, on_device); }
int pnp_get_state_cx_f64(pnp_ctx* c, double* z, double* w, int on_device) { CTX(c); NEED_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c); NEED_STATE(c); return get_state<double, true>(c, z, w, on_device); }
int pnp_download_x_cx(pnp_ctx* c, float* x, int on_device) { CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c); return download_x<float, true>(c, __func__, x, on_device); }
int pnp_download_x_cx_f64(pnp_ctx* c, double* x, int on_device) { CTX(c); NEED_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c); return download_x<double, true>(c, __func__, x, on_device); }

int pnp_dc_step_cx(pnp_ctx* c, const float* z, const float* w, float* x, double reo) {
    CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c);
    Range r("pnp_dc_step_cx");
    return dc_step<float, true>(c, __func__, z, w, x, reo);
}
int pnp_dc_step_cx_f64(pnp_ctx* c, const double* z, const double* w, double* x, double reo) {
    CTX(c); NEED_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c);
    Range r("pnp_dc_step_cx_f64");
    return dc_step<double, true>(c, __func__, z, w, x, reo);
}

int pnp_prox_l1_dual_cx(pnp_ctx* c, const float* x, float* z, float* w, double thr) {
    CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!(thr >= 0.0)) return fail(PNP_E_ARG, "%s: thr must be >= 0", __func__);
    ProxParams p{}; p.thr = (float)thr;
    return prox_dual<float, true>(c, __func__, false, x, z, w, p);
}
int pnp_prox_l1_dual_cx_f64(pnp_ctx* c, const double* x, double* z, double* w, double thr) {
    CTX(c); NEED_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c);
    if (!(thr >= 0.0)) return fail(PNP_E_ARG, "%s: thr must be >= 0", __func__);
    ProxParamsT<double> p{}; p.thr = thr;
    return prox_dual<double, true>(c, __func__, false, x, z, w, p);
}
int pnp_prox_cnc_dual_cx(pnp_ctx* c, const float* x, float* z, float* w, double alpha, double lambda1, double reo, double b) {
    CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (int rv = check_cnc(__func__, alpha, lambda1, reo, b)) return rv;
    return prox_dual<float, true>(c, __func__, true, x, z, w, prox_cnc<float>(alpha, lambda1, reo, b));
}
int pnp_prox_cnc_dual_cx_f64(pnp_ctx* c, const double* x, double* z, double* w, double alpha, double lambda1, double reo, double b) {
    CTX(c); NEED_COMPLEX(c); F64_ONLY(c); NEED_PROBLEM(c);
    if (int rv = check_cnc(__func__, alpha, lambda1, reo, b)) return rv;
    return prox_dual<double, true>(c, __func__, true, x, z, w, prox_cnc<double>(alpha, lambda1, reo, b));
}

int pnp_A_cx(pnp_ctx* c, const float* x, float* k) {        // x: [B][H][W] complex, k: [B][C][H][W]
    CTX(c); NEED_COMPLEX(c); F32_ONLY(c); NEED_PROBLEM(c);
    if (!x || !k) return fail(PNP_E_ARG, "%s: null pointer", __func__);
    if (int rc = cx_aligned<float>(__func__, x, k)) return rc;
    CoilRowArgsT<float> ca = coil_rows<float>(c, c->B);
    ca.cin = (const float2*)x; ca.work = (float2*)k;
    HIPCHK(anysize_coil_rows_in<float>(c->coils.any, c->stream, ca));
    HIPCHK(anysize_cols<float>(c->coils.any, c->stream, true, MID_MASK, false, coil_cols<float>(c, k, k)));
    return PNP_OK;
}

// ---- PnP denoisers on complex images: pnp_cx_ops.h, kernels_pnp_cx.hip.  The rules in the header's order: pointers, state, scalars, alignment ----

static int cx_den_rules(pnp_ctx* c, const char* who, bool ptrs_ok, int mode, double gain) {
    if (!ptrs_ok) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (!cx_mode(c)) return fail(PNP_E_STATE, "%s: needs complex image mode (pnp_set_image)", who);
    if (c->f64) return fail(PNP_E_STATE, "%s: not available on an fp64 validation context", who);
    if (c->B <= 0) return fail(PNP_E_STATE, "%s: no problem uploaded", who);
    if (mode != PNP_CX_DENOISE_MODULUS && mode != PNP_CX_DENOISE_PARTS)
        return fail(PNP_E_ARG, "%s: mode must be PNP_CX_DENOISE_MODULUS (0) or PNP_CX_DENOISE_PARTS (1) (got %d)", who, mode);
    const float g = (float)gain;
    if (!(gain > 0.0) || !std::isfinite(gain) || !(g > 0.0f) || !std::isfinite(g)) return fail(PNP_E_ARG, "%s: gain must be finite and > 0 (got %g)", who, gain);
    return PNP_OK;
}
static int cx_den_aligned(const char* who, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* q : ptrs) bits |= (uintptr_t)q;
    if (bits & 15) return fail(PNP_E_ARG, "%s: the complex arrays and the plane base must be 16-byte aligned", who);
    return PNP_OK;
}

int pnp_cx_den_in(pnp_ctx* c, const float* a, const float* b, float* planes, int mode, double gain) {
    CTX(c);
    if (int rc = cx_den_rules(c, __func__, a && planes, mode, gain)) return rc;
    if (int rc = cx_den_aligned(__func__, { a, b, planes })) return rc;
    HIPCHK(launch_cx_den_in(c->stream, mode, (const float2*)a, (const float2*)b, planes, (float)gain, (size_t)c->B * c->N));
    return PNP_OK;
}
int pnp_cx_den_out(pnp_ctx* c, const float* q, const float* a, const float* b, float* z, int mode, double gain) {
    CTX(c);
    if (int rc = cx_den_rules(c, __func__, q && a && z, mode, gain)) return rc;
    if (int rc = cx_den_aligned(__func__, { q, a, b, z })) return rc;
    HIPCHK(launch_cx_den_out(c->stream, mode, q, (const float2*)a, (const float2*)b, (float2*)z, (float)gain, (size_t)c->B * c->N));
    return PNP_OK;
}
int pnp_cx_den_out_dual(pnp_ctx* c, const float* q, const float* a, const float* b, float* x, float* z, float* w, int mode, double gain) {
    CTX(c);
    if (int rc = cx_den_rules(c, __func__, q && a && x && z && w, mode, gain)) return rc;
    if (int rc = cx_den_aligned(__func__, { q, a, b, x, z, w })) return rc;
    HIPCHK(launch_cx_den_out_dual(c->stream, mode, q, (const float2*)a, (const float2*)b, (float2*)x, (float2*)z, (float2*)w, (float)gain,
                                  (size_t)c->B * c->N));
    return PNP_OK;
}
int pnp_cnc_combine_cx(pnp_ctx* c, const float* z, const float* x, const float* w, const float* s, float* t, double alpha, double lambda1,
                       double reo, double b) {
    CTX(c);
    if (int rc = cx_den_rules(c, __func__, z && x && w && s && t, PNP_CX_DENOISE_MODULUS, 1.0)) return rc;
    if (int rc = cx_den_aligned(__func__, { z, x, w, s, t })) return rc;
    HIPCHK(launch_combine(c->stream, z, x, w, s, t, (float)(1.0 - alpha), (float)alpha, (float)(alpha * reo * lambda1 * b),
                          2 * (size_t)c->B * c->N));                  // component-wise: k_combine on 2 n floats
    return PNP_OK;
}

// ---- coil mixing ahead of the multi-coil solve: coilmix_plan.h, kernels_coilmix.hip.  No context: caller-owned device arrays ----

int pnp_coilmix_check(int C_in, int C_out, int Ks, int ncal, int H, int W) {
    switch (coilmix_check(C_in, C_out, Ks, ncal, H, W)) {
    case COILMIX_OK:        return PNP_OK;
    case COILMIX_BAD_IN:    return fail(PNP_E_ARG, "coil mixing: C_in must be 1..%d (got %d)", COILMIX_MAX_IN, C_in);
    case COILMIX_BAD_OUT:   return fail(PNP_E_ARG, "coil mixing: C_out must be 1..min(C_in, %d) (got %d of %d)", COIL_MAX_C, C_out, C_in);
    case COILMIX_BAD_SETS:  return fail(PNP_E_ARG, "coil mixing: Ks must be >= 1 (got %d)", Ks);
    case COILMIX_BAD_NCAL:  return fail(PNP_E_ARG, "coil mixing: ncal must be %d..%d and <= min(H, W) (got %d at %d x %d)", COILMIX_NCAL_MIN,
                                        COILMIX_NCAL_MAX, ncal, H, W);
    default:                return fail(PNP_E_ARG, "coil mixing: H, W must be in [128, 1024] (got %d x %d)", H, W);
    }
}

extern "C++" {
template <typename R>
static int coil_mix_any(const char* who, void* stream, const R* in, const R* m, const int32_t* set_id, R* out, int B, int C_in, int C_out, size_t N) {
    if (!in || !m || !out) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (B < 1 || B > 65535) return fail(PNP_E_ARG, "%s: B must be 1..65535 (got %d)", who, B);
    if (C_in < 1 || C_in > COILMIX_MAX_IN) return fail(PNP_E_ARG, "%s: C_in must be 1..%d (got %d)", who, COILMIX_MAX_IN, C_in);
    if (C_out < 1 || C_out > C_in || C_out > COIL_MAX_C) return fail(PNP_E_ARG, "%s: C_out must be 1..min(C_in, %d) (got %d of %d)", who, COIL_MAX_C, C_out, C_in);
    if (N < 1 || coilmix_mix_blocks(N, sizeof(R) == 8) > 0x7fffffffu) return fail(PNP_E_ARG, "%s: N must be >= 1 and make fewer than 2^31 workgroups (got %zu)", who, N);
    if ((uintptr_t)in % (2 * sizeof(R)) || (uintptr_t)out % (2 * sizeof(R)) || (uintptr_t)m % (2 * sizeof(R)))
        return fail(PNP_E_ARG, "%s: in, m and out must be aligned to one complex value", who);
    const char *i0 = (const char*)in, *o0 = (const char*)out;
    const size_t ib = (size_t)B * C_in * N * 2 * sizeof(R), ob = (size_t)B * C_out * N * 2 * sizeof(R);
    if (i0 < o0 + ob && o0 < i0 + ib) return fail(PNP_E_ARG, "%s: in and out must not overlap", who);
    HIPCHK(launch_coil_mix<R>((hipStream_t)stream, in, m, set_id, out, B, C_in, C_out, N));
    return PNP_OK;
}
}  // extern "C++"
int pnp_coil_mix(void* stream, const float* in, const float* m, const int32_t* set_id, float* out, int B, int C_in, int C_out, size_t N) {
    return coil_mix_any<float>(__func__, stream, in, m, set_id, out, B, C_in, C_out, N);
}
int pnp_coil_mix_f64(void* stream, const double* in, const double* m, const int32_t* set_id, double* out, int B, int C_in, int C_out, size_t N) {
    return coil_mix_any<double>(__func__, stream, in, m, set_id, out, B, C_in, C_out, N);
}

extern "C++" {
template <typename R>
static int coil_gram_any(const char* who, void* stream, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int C,
                         int H, int W, int ncal) {
    if (!y || !mask_bank || !gram) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (B < 1 || B > 65535) return fail(PNP_E_ARG, "%s: B must be 1..65535 (got %d)", who, B);
    if (int rc = pnp_coilmix_check(C, 1, 1, ncal, H, W)) return rc;
    if ((uintptr_t)y % (2 * sizeof(R)) || (uintptr_t)gram % 16) return fail(PNP_E_ARG, "%s: y and gram must be aligned to one complex value", who);
    HIPCHK(launch_coil_gram<R>((hipStream_t)stream, y, mask_bank, mask_id, gram, B, C, H, W, ncal));
    return PNP_OK;
}
}  // extern "C++"
int pnp_coil_gram(void* stream, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int C, int H, int W, int ncal) {
    return coil_gram_any<float>(__func__, stream, y, mask_bank, mask_id, gram, B, C, H, W, ncal);
}
int pnp_coil_gram_f64(void* stream, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int C, int H, int W, int ncal) {
    return coil_gram_any<double>(__func__, stream, y, mask_bank, mask_id, gram, B, C, H, W, ncal);
}

int pnp_coilmix_whiten(const double* noise_cov, int C, double* m_out) {
    if (!noise_cov || !m_out || noise_cov == m_out) return fail(PNP_E_ARG, "pnp_coilmix_whiten: null or aliased pointers");
    if (C < 1 || C > COILMIX_MAX_IN) return fail(PNP_E_ARG, "pnp_coilmix_whiten: C must be 1..%d (got %d)", COILMIX_MAX_IN, C);
    if (!coilmix_all_finite(noise_cov, 2 * (size_t)C * C)) return fail(PNP_E_ARG, "pnp_coilmix_whiten: the covariance has a non-finite entry");
    if (int at = coilmix_inv_chol(noise_cov, C, m_out))
        return fail(PNP_E_ARG, "pnp_coilmix_whiten: the covariance is not positive definite (pivot %d of the Cholesky factor)", at - 1);
    return PNP_OK;
}

int pnp_coilmix_compress(const double* gram, int C, int C_out, double* m_out, double* eig_out) {
    if (!gram || !m_out || !eig_out) return fail(PNP_E_ARG, "pnp_coilmix_compress: null pointer");
    if (C < 1 || C > COILMIX_MAX_IN) return fail(PNP_E_ARG, "pnp_coilmix_compress: C must be 1..%d (got %d)", COILMIX_MAX_IN, C);
    if (C_out < 1 || C_out > C || C_out > COIL_MAX_C) return fail(PNP_E_ARG, "pnp_coilmix_compress: C_out must be 1..min(C, %d) (got %d of %d)", COIL_MAX_C, C_out, C);
    if (!coilmix_all_finite(gram, 2 * (size_t)C * C)) return fail(PNP_E_ARG, "pnp_coilmix_compress: the Gram matrix has a non-finite entry");
    std::vector<double> work(4 * (size_t)C * C);
    if (coilmix_compress(gram, C, C_out, m_out, eig_out, work.data())) return fail(PNP_E_ARG, "pnp_coilmix_compress: the Jacobi sweeps did not converge");
    return PNP_OK;
}

// ---- coil sensitivity maps from the calibration region: coilmaps_plan.h, kernels_coilmaps.hip.  On a context: its transforms, its stream ----

int pnp_coilmaps_check(int C, int ncal, int radius, int power_iters, double thresh, int H, int W) {
    switch (coilmaps_check(C, ncal, radius, power_iters, thresh, H, W)) {
    case COILMAPS_OK:         return PNP_OK;
    case COILMAPS_BAD_C:      return fail(PNP_E_ARG, "coil maps: C must be 1..%d (got %d)", COIL_MAX_C, C);
    case COILMAPS_BAD_NCAL:   return fail(PNP_E_ARG, "coil maps: ncal must be %d..%d and <= min(H, W) (got %d at %d x %d)", COILMIX_NCAL_MIN,
                                          COILMIX_NCAL_MAX, ncal, H, W);
    case COILMAPS_BAD_RADIUS: return fail(PNP_E_ARG, "coil maps: radius must be 0..%d (got %d)", COILMAPS_MAX_RADIUS, radius);
    case COILMAPS_BAD_ITERS:  return fail(PNP_E_ARG, "coil maps: power_iters must be 1..%d (got %d)", COILMAPS_MAX_ITERS, power_iters);
    case COILMAPS_BAD_THRESH: return fail(PNP_E_ARG, "coil maps: thresh must be in [0, 1) (got %g)", thresh);
    default:                  return fail(PNP_E_ARG, "coil maps: H, W must be in [128, 1024] (got %d x %d)", H, W);
    }
}

// ---- what pnp_coil_maps and pnp_espirit_maps share on the host: argument rules, scratch array, missing-point report, stage timers (the
// calibration pass itself is launch_calib_window and ifft2_chunks) ----
extern "C++" {
// The pointer rules of both estimators (lambda may be null).  `rule` is the estimator's own pnp_*_check of its scalars, made by the caller:
// it is reported where it always was, after the null and range rules and before alignment and overlap.
template <typename R>
static int maps_args(const char* who, const pnp_ctx* c, const R* y, const uint8_t* mask_bank, const R* maps, const R* lambda, int B, int C, int rule) {
    using Cx = typename CxOf<R>::type;
    if (c->f64 != (sizeof(R) == 8))
        return fail(PNP_E_STATE, sizeof(R) == 8 ? "%s: needs a context made by pnp_ctx_create_any_f64" : "%s: not available on an fp64 validation context", who);
    if (!y || !mask_bank || !maps) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (B < 1 || B > 65535) return fail(PNP_E_ARG, "%s: B must be 1..65535 (got %d)", who, B);
    if (rule) return rule;
    if ((uintptr_t)y % sizeof(Cx) || (uintptr_t)maps % sizeof(Cx) || (lambda && (uintptr_t)lambda % sizeof(R)))
        return fail(PNP_E_ARG, "%s: y and maps_out must be aligned to one complex value, lambda_out to one real", who);
    const size_t N = c->N, bytes = (size_t)B * C * N * sizeof(Cx);
    const char *y0 = (const char*)y, *m0 = (const char*)maps, *l0 = (const char*)lambda;
    if (y0 < m0 + bytes && m0 < y0 + bytes) return fail(PNP_E_ARG, "%s: maps_out and y must not overlap", who);
    if (lambda) {
        const size_t lb = (size_t)B * N * sizeof(R);
        if ((l0 < m0 + bytes && m0 < l0 + lb) || (l0 < y0 + bytes && y0 < l0 + lb)) return fail(PNP_E_ARG, "%s: lambda_out must not overlap y or maps_out", who);
    }
    return PNP_OK;
}

// the context's scratch array of the estimators, grown on demand
static int maps_reserve(const char* who, pnp_ctx* c, size_t bytes, int B, int C) {
    if (c->maps_bytes >= bytes) return PNP_OK;
    HIPCHK(hipStreamSynchronize(c->stream));             // an earlier call on this stream may still read the old array
    if (c->maps_scratch) (void)hipFree(c->maps_scratch);
    c->maps_scratch = nullptr; c->maps_bytes = 0;
    if (int rc = alloc_or_fail(&c->maps_scratch, bytes, who, "scratch array", "B=%d, C=%d, Bmax=%d, %dx%d", B, C, c->Bmax, c->H, c->W)) return rc;
    c->maps_bytes = bytes;
    return PNP_OK;
}

// k_calib_window's report of slices b0 .. b0 + n - 1, read back to the host: the first slice whose mask has a hole in the region
static int maps_missing(const char* who, const pnp_ctx* c, const int32_t* miss, int b0, int n, int ncal) {
    for (int b = 0; b < n; ++b)
        if (miss[b] >= 0)
            return fail(PNP_E_ARG, "%s: the mask of slice %d does not sample calibration point (%d, %d) of the %d x %d region: every point of it must be measured",
                        who, b0 + b, miss[b] / c->W, miss[b] % c->W, ncal, ncal);
    return PNP_OK;
}

static int stage_times(StageTimer& t, int enable, float* ms_out) {
    if (enable)
        for (hipEvent_t& e : t.ev) if (!e) HIPCHK(hipEventCreate(&e));
    if (ms_out) for (int k = 0; k < 3; ++k) ms_out[k] = t.ms[k];
    for (float& v : t.ms) v = 0.f;
    t.on = enable != 0;
    return PNP_OK;
}

template <typename R>
static int coil_maps_any(const char* who, pnp_ctx* c, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, R* maps, R* lambda, int B,
                         int C, int ncal, int radius, int power_iters, double thresh) {
    using Cx = typename CxOf<R>::type;
    if (int rc = maps_args<R>(who, c, y, mask_bank, maps, lambda, B, C, pnp_coilmaps_check(C, ncal, radius, power_iters, thresh, c->H, c->W))) return rc;
    const size_t N = c->N;
    const CoilmapsScratch lay = coilmaps_scratch(B, C, c->Bmax, N, c->f64);
    if (int rc = maps_reserve(who, c, lay.bytes, B, C)) return rc;
    StageTimer& tm = c->cm_t;
    char* base = (char*)c->maps_scratch;
    Cx* img = (Cx*)(base + lay.img);
    R* part = (R*)(base + lay.part);
    int32_t* miss = (int32_t*)(base + lay.miss);
    const int nb = coilmaps_pass_slices(B, C, c->Bmax);
    const R tau2 = (R)(thresh * thresh);
    for (int b0 = 0; b0 < B; b0 += nb) {
        const int n = B - b0 < nb ? B - b0 : nb;             // slices of this pass: n C pseudo-slices
        const R* yb = y + 2 * (size_t)b0 * C * N;
        R* mb = maps + 2 * (size_t)b0 * C * N;
        R* lam = lambda ? lambda + (size_t)b0 * N : (R*)(base + lay.lambda);
        // the windowed region goes through maps_out: rows maps_out -> scratch, columns in place, the eigenvector kernel scratch -> maps_out
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[0], c->stream));
        HIPCHK(launch_calib_window<R>(c->stream, yb, mask_bank, mask_id ? mask_id + b0 : nullptr, mb, miss + b0, n, C, c->H, c->W, ncal));
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[1], c->stream));
        if (int rc = ifft2_chunks<R>(c, (const Cx*)mb, img, n * C)) return rc;
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[2], c->stream));
        HIPCHK(launch_coil_eigmaps<R>(c->stream, (const R*)img, mb, lam, n, C, c->H, c->W, radius, power_iters));
        HIPCHK(launch_maps_support<R>(c->stream, nullptr, R(0), lam, tau2, part, mb, n, C, N));
        if (tm.on) {
            HIPCHK(hipEventRecord(tm.ev[3], c->stream));
            HIPCHK(hipEventSynchronize(tm.ev[3]));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, tm.ev[k], tm.ev[k + 1]));
                tm.ms[k] += ms;
            }
        }
    }
    std::vector<int32_t> host((size_t)B);
    HIPCHK(hipMemcpyAsync(host.data(), miss, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return maps_missing(who, c, host.data(), 0, B, ncal);
}
}  // extern "C++"

int pnp_coil_maps_stage_times(pnp_ctx* c, int enable, float* ms_out) { CTX(c); return stage_times(c->cm_t, enable, ms_out); }

int pnp_coil_maps(pnp_ctx* c, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, float* maps_out, float* lambda_out, int B, int C,
                  int ncal, int radius, int power_iters, double thresh) {
    CTX(c);
    return coil_maps_any<float>(__func__, c, y, mask_bank, mask_id, maps_out, lambda_out, B, C, ncal, radius, power_iters, thresh);
}
int pnp_coil_maps_f64(pnp_ctx* c, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, double* maps_out, double* lambda_out, int B,
                      int C, int ncal, int radius, int power_iters, double thresh) {
    CTX(c);
    return coil_maps_any<double>(__func__, c, y, mask_bank, mask_id, maps_out, lambda_out, B, C, ncal, radius, power_iters, thresh);
}

// ---- ESPIRiT coil maps: espirit_plan.h, kernels_espirit.hip.  Patch Gram on the device, signal space and kernels on the host, pixels on the device ----

int pnp_espirit_check(int C, int ncal, int kernel, int power_iters, double sigma, double crop, double thresh, int H, int W) {
    switch (espirit_check(C, ncal, kernel, power_iters, sigma, crop, thresh, H, W)) {
    case ESPIRIT_OK:               return PNP_OK;
    case ESPIRIT_BAD_C:            return fail(PNP_E_ARG, "espirit: C must be 1..%d (got %d)", COIL_MAX_C, C);
    case ESPIRIT_BAD_SHAPE:        return fail(PNP_E_ARG, "espirit: H, W must be in [128, 1024] (got %d x %d)", H, W);
    case ESPIRIT_BAD_NCAL:         return fail(PNP_E_ARG, "espirit: ncal must be %d..%d and <= min(H, W) (got %d at %d x %d)", COILMIX_NCAL_MIN,
                                               COILMIX_NCAL_MAX, ncal, H, W);
    case ESPIRIT_BAD_KERNEL:       return fail(PNP_E_ARG, "espirit: kernel must be %d..%d (got %d)", ESPIRIT_MIN_KERNEL, ESPIRIT_MAX_KERNEL, kernel);
    case ESPIRIT_KERNEL_OVER_NCAL: return fail(PNP_E_ARG, "espirit: kernel must be <= ncal (got %d with ncal %d)", kernel, ncal);
    case ESPIRIT_BAD_SIZE:         return fail(PNP_E_ARG, "espirit: C * kernel^2 must be <= %d, the size of the host eigen-solver (got %d * %d^2 = %d): "
                                               "compress the channels with virtual_coils= first", ESPIRIT_MAX_N, C, kernel, C * kernel * kernel);
    case ESPIRIT_BAD_ITERS:        return fail(PNP_E_ARG, "espirit: power_iters must be 1..%d (got %d)", ESPIRIT_MAX_ITERS, power_iters);
    case ESPIRIT_BAD_SIGMA:        return fail(PNP_E_ARG, "espirit: sigma must be in (0, 1) (got %g)", sigma);
    case ESPIRIT_BAD_CROP:         return fail(PNP_E_ARG, "espirit: crop must be in [0, 1] (got %g)", crop);
    default:                       return fail(PNP_E_ARG, "espirit: thresh must be in [0, 1) (got %g)", thresh);
    }
}

extern "C++" {
// the rules of espirit_check that the Gram stage alone depends on
static int espirit_gram_rule(int C, int ncal, int kernel, int H, int W) { return pnp_espirit_check(C, ncal, kernel, 1, 0.5, 0.0, 0.0, H, W); }

template <typename R>
static int patch_gram_any(const char* who, void* stream, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int C,
                          int H, int W, int ncal, int kernel) {
    if (!y || !mask_bank || !gram) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (B < 1 || B > 65535) return fail(PNP_E_ARG, "%s: B must be 1..65535 (got %d)", who, B);
    if (int rc = espirit_gram_rule(C, ncal, kernel, H, W)) return rc;
    if ((uintptr_t)y % (2 * sizeof(R)) || (uintptr_t)gram % 16) return fail(PNP_E_ARG, "%s: y and gram must be aligned to one complex value", who);
    HIPCHK(launch_calib_patch_gram<R>((hipStream_t)stream, y, mask_bank, mask_id, gram, B, C, H, W, ncal, kernel));
    return PNP_OK;
}

// the phasor tables of the context's shape into the scratch array; the host copies live in `keep` until the caller has synchronised
template <typename R>
static int espirit_tables(pnp_ctx* c, const EspiritScratch& lay, int kernel, std::vector<R>& keep) {
    const size_t D = (size_t)espirit_side(kernel), nh = 2 * (size_t)c->H * D, nw = 2 * (size_t)c->W * D;
    keep.resize(nh + nw);
    espirit_phasor_table<R>(c->H, kernel, keep.data());
    espirit_phasor_table<R>(c->W, kernel, keep.data() + nh);
    char* base = (char*)c->maps_scratch;
    HIPCHK(hipMemcpyAsync(base + lay.eh, keep.data(), nh * sizeof(R), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(base + lay.ew, keep.data() + nh, nw * sizeof(R), hipMemcpyHostToDevice, c->stream));
    return PNP_OK;
}

template <typename R>
static int espirit_eigmaps_any(const char* who, pnp_ctx* c, const R* img, const R* w, R* maps, R* lambda, int B, int C, int kernel, int power_iters) {
    using Cx = typename CxOf<R>::type;
    if (c->f64 != (sizeof(R) == 8))
        return fail(PNP_E_STATE, sizeof(R) == 8 ? "%s: needs a context made by pnp_ctx_create_any_f64" : "%s: not available on an fp64 validation context", who);
    if (!img || !w || !maps || !lambda) return fail(PNP_E_ARG, "%s: null pointer", who);
    if (B < 1 || B > 65535) return fail(PNP_E_ARG, "%s: B must be 1..65535 (got %d)", who, B);
    if (int rc = pnp_espirit_check(C, kernel > COILMIX_NCAL_MIN ? kernel : COILMIX_NCAL_MIN, kernel, power_iters, 0.5, 0.0, 0.0, c->H, c->W)) return rc;
    if ((uintptr_t)img % sizeof(Cx) || (uintptr_t)maps % sizeof(Cx) || (uintptr_t)w % sizeof(Cx) || (uintptr_t)lambda % sizeof(R))
        return fail(PNP_E_ARG, "%s: the complex arrays must be aligned to one complex value, lambda_out to one real", who);
    const size_t N = c->N, bytes = (size_t)B * C * N * sizeof(Cx);
    const char *i0 = (const char*)img, *m0 = (const char*)maps;
    if (i0 < m0 + bytes && m0 < i0 + bytes) return fail(PNP_E_ARG, "%s: maps_out and the images must not overlap", who);
    const EspiritScratch lay = espirit_scratch(B, B, C, kernel, c->H, c->W, c->f64, false);
    if (int rc = maps_reserve(who, c, lay.bytes, B, C)) return rc;
    char* base = (char*)c->maps_scratch;
    std::vector<R> keep;
    if (int rc = espirit_tables<R>(c, lay, kernel, keep)) return rc;
    R* inorm = (R*)(base + lay.inorm);
    HIPCHK(launch_espirit_maps<R>(c->stream, img, w, (const R*)(base + lay.eh), (const R*)(base + lay.ew), maps, lambda, inorm, B, C, c->H, c->W,
                                  kernel, power_iters));
    HIPCHK(hipStreamSynchronize(c->stream));             // the tables' host copies go out of scope
    return PNP_OK;
}

template <typename R>
static int espirit_maps_any(const char* who, pnp_ctx* c, const R* y, const uint8_t* mask_bank, const int32_t* mask_id, R* maps, R* lambda, int B,
                            int C, int ncal, int kernel, int power_iters, double sigma, double crop, double thresh) {
    using Cx = typename CxOf<R>::type;
    if (int rc = maps_args<R>(who, c, y, mask_bank, maps, lambda, B, C, pnp_espirit_check(C, ncal, kernel, power_iters, sigma, crop, thresh, c->H, c->W)))
        return rc;
    const size_t N = c->N;
    const int nb = coilmaps_pass_slices(B, C, c->Bmax), n = espirit_columns(C, kernel);
    const EspiritScratch lay = espirit_scratch(B, nb, C, kernel, c->H, c->W, c->f64, true);
    if (int rc = maps_reserve(who, c, lay.bytes, B, C)) return rc;
    StageTimer& tm = c->es_t;
    char* base = (char*)c->maps_scratch;
    Cx* img = (Cx*)(base + lay.img);
    R* inorm = (R*)(base + lay.inorm);
    R* part = (R*)(base + lay.part);
    int32_t* miss = (int32_t*)(base + lay.miss);
    double* gram = (double*)(base + lay.gram);
    R* wdev = (R*)(base + lay.w);
    std::vector<R> keep;
    if (int rc = espirit_tables<R>(c, lay, kernel, keep)) return rc;
    const size_t wn = espirit_w_count(C, kernel);
    std::vector<double> hgram((size_t)nb * n * n * 2), hw64((size_t)ESPIRIT_HOST_THREADS * wn * 2),
        work((size_t)ESPIRIT_HOST_THREADS * (espirit_work_doubles(n) + n));
    std::vector<R> hw((size_t)nb * wn * 2);
    std::vector<int32_t> hmiss((size_t)nb), rank((size_t)B, 0);
    std::vector<int> status((size_t)nb);
    for (int b0 = 0; b0 < B; b0 += nb) {
        const int ns = B - b0 < nb ? B - b0 : nb;            // slices of this pass: ns C pseudo-slices
        const R* yb = y + 2 * (size_t)b0 * C * N;
        R* mb = maps + 2 * (size_t)b0 * C * N;
        R* lam = lambda ? lambda + (size_t)b0 * N : (R*)(base + lay.lambda);
        // the windowed region goes through maps_out: rows maps_out -> scratch, columns in place; the per-pixel kernel scratch -> maps_out
        HIPCHK(launch_calib_window<R>(c->stream, yb, mask_bank, mask_id ? mask_id + b0 : nullptr, mb, miss + b0, ns, C, c->H, c->W, ncal));
        if (int rc = ifft2_chunks<R>(c, (const Cx*)mb, img, ns * C)) return rc;
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[0], c->stream));
        HIPCHK(launch_calib_patch_gram<R>(c->stream, yb, mask_bank, mask_id ? mask_id + b0 : nullptr, gram, ns, C, c->H, c->W, ncal, kernel));
        HIPCHK(hipMemcpyAsync(hgram.data(), gram, (size_t)ns * n * n * 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(hmiss.data(), miss + b0, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[1], c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (int rc = maps_missing(who, c, hmiss.data(), b0, ns, ncal)) return rc;
        if (!coilmix_all_finite(hgram.data(), (size_t)ns * n * n * 2)) return fail(PNP_E_ARG, "%s: the calibration region has a non-finite entry", who);
        // the host stage: slice b of the pass on thread b % threads, every slice on its own arrays
        const auto t0 = std::chrono::steady_clock::now();
        const int threads = ns < ESPIRIT_HOST_THREADS ? ns : ESPIRIT_HOST_THREADS;
        auto job = [&](int t) {
            double* w64 = hw64.data() + (size_t)t * wn * 2;
            double* wk = work.data() + (size_t)t * (espirit_work_doubles(n) + n);
            for (int b = t; b < ns; b += threads) {
                status[b] = espirit_kernels(hgram.data() + (size_t)b * n * n * 2, C, kernel, sigma, w64, &rank[b0 + b], wk + espirit_work_doubles(n), wk);
                for (size_t i = 0; i < wn * 2; ++i) hw[(size_t)b * wn * 2 + i] = (R)w64[i];
            }
        };
        if (threads == 1) job(0);
        else {
            std::vector<std::thread> pool;
            for (int t = 1; t < threads; ++t) pool.emplace_back(job, t);
            job(0);
            for (std::thread& t : pool) t.join();
        }
        for (int b = 0; b < ns; ++b)
            if (status[b]) return fail(PNP_E_ARG, "%s: the Jacobi sweeps did not converge on the Gram matrix of slice %d", who, b0 + b);
        if (tm.on) tm.ms[1] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        HIPCHK(hipMemcpyAsync(wdev, hw.data(), (size_t)ns * wn * 2 * sizeof(R), hipMemcpyHostToDevice, c->stream));
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[2], c->stream));
        HIPCHK(launch_espirit_maps<R>(c->stream, (const R*)img, wdev, (const R*)(base + lay.eh), (const R*)(base + lay.ew), mb, lam, inorm, ns, C,
                                      c->H, c->W, kernel, power_iters));
        HIPCHK(launch_maps_support<R>(c->stream, lam, (R)crop, inorm, (R)thresh, part, mb, ns, C, N));
        if (tm.on) HIPCHK(hipEventRecord(tm.ev[3], c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));             // the next pass rewrites the host arrays the copies read
        if (tm.on) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, tm.ev[0], tm.ev[1]));
            tm.ms[0] += ms;
            HIPCHK(hipEventElapsedTime(&ms, tm.ev[2], tm.ev[3]));
            tm.ms[2] += ms;
        }
    }
    c->es_rank = rank;
    return PNP_OK;
}
}  // extern "C++"

int pnp_calib_patch_gram(void* stream, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int C, int H, int W,
                         int ncal, int kernel) {
    return patch_gram_any<float>(__func__, stream, y, mask_bank, mask_id, gram, B, C, H, W, ncal, kernel);
}
int pnp_calib_patch_gram_f64(void* stream, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, double* gram, int B, int C, int H,
                             int W, int ncal, int kernel) {
    return patch_gram_any<double>(__func__, stream, y, mask_bank, mask_id, gram, B, C, H, W, ncal, kernel);
}

int pnp_espirit_kernels(const double* gram, int C, int kernel, double sigma, double* w_out, int* rank_out, double* sing_out) {
    if (!gram || !w_out || !rank_out || !sing_out) return fail(PNP_E_ARG, "pnp_espirit_kernels: null pointer");
    if (int rc = pnp_espirit_check(C, kernel > COILMIX_NCAL_MIN ? kernel : COILMIX_NCAL_MIN, kernel, 1, sigma, 0.0, 0.0, 128, 128)) return rc;
    const int n = espirit_columns(C, kernel);
    if (!coilmix_all_finite(gram, 2 * (size_t)n * n)) return fail(PNP_E_ARG, "pnp_espirit_kernels: the Gram matrix has a non-finite entry");
    std::vector<double> work(espirit_work_doubles(n));
    if (espirit_kernels(gram, C, kernel, sigma, w_out, rank_out, sing_out, work.data()))
        return fail(PNP_E_ARG, "pnp_espirit_kernels: the Jacobi sweeps did not converge");
    return PNP_OK;
}

int pnp_espirit_eigmaps(pnp_ctx* c, const float* lowres_images, const float* w, float* maps_out, float* lambda_out, int B, int C, int kernel,
                        int power_iters) {
    CTX(c);
    return espirit_eigmaps_any<float>(__func__, c, lowres_images, w, maps_out, lambda_out, B, C, kernel, power_iters);
}
int pnp_espirit_eigmaps_f64(pnp_ctx* c, const double* lowres_images, const double* w, double* maps_out, double* lambda_out, int B, int C, int kernel,
                            int power_iters) {
    CTX(c);
    return espirit_eigmaps_any<double>(__func__, c, lowres_images, w, maps_out, lambda_out, B, C, kernel, power_iters);
}

int pnp_espirit_maps(pnp_ctx* c, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, float* maps_out, float* lambda_out, int B, int C,
                     int ncal, int kernel, int power_iters, double sigma, double crop, double thresh) {
    CTX(c);
    return espirit_maps_any<float>(__func__, c, y, mask_bank, mask_id, maps_out, lambda_out, B, C, ncal, kernel, power_iters, sigma, crop, thresh);
}
int pnp_espirit_maps_f64(pnp_ctx* c, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, double* maps_out, double* lambda_out, int B,
                         int C, int ncal, int kernel, int power_iters, double sigma, double crop, double thresh) {
    CTX(c);
    return espirit_maps_any<double>(__func__, c, y, mask_bank, mask_id, maps_out, lambda_out, B, C, ncal, kernel, power_iters, sigma, crop, thresh);
}

int pnp_espirit_ranks(pnp_ctx* c, int32_t* rank_out, int B) {
    CTX(c);
    if (!rank_out || B < 1 || (size_t)B != c->es_rank.size())
        return fail(PNP_E_ARG, "pnp_espirit_ranks: rank_out must hold the %zu slices of the most recent pnp_espirit_maps (got %d)", c->es_rank.size(), B);
    for (int b = 0; b < B; ++b) rank_out[b] = c->es_rank[b];
    return PNP_OK;
}

int pnp_espirit_stage_times(pnp_ctx* c, int enable, float* ms_out) { CTX(c); return stage_times(c->es_t, enable, ms_out); }

}  // extern "C"
