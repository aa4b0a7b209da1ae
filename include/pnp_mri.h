/*
 * pnp_mri.h -- C ABI of libpnpmri.so: the MI355X (gfx950) hot path of PnP-ADMM-CNC MRI
 * reconstruction.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * What it replaces.  zj15001/PNP_ADMM_CNC_MRI has no FFI on this path: the per-iteration loop is
 * ~15 lines of NumPy pasted inline into every solver function.  Each entry point below cites the
 * reference lines (aliases of SURVEY.md: S1 = "【1】ADMM_L1.py", S3 = "【3】PNP_ADMM_L1_D  .py",
 * S4 = "【4】ADMM_CNC .py", S6 = "【6】PNP_ADMM_CNC_D .py") it stands in for.  The only C-ABI
 * precedent in the reference is BM3D's ctypes layer (bm3d307/bm3d/bm3d_py.h:4-16,
 * bm3d_ctypes.py:194-240); INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (PNP_E_*); pnp_last_error() gives the
 *     thread-local message.  No exceptions, no aborts.
 *   - complex data = interleaved (re,im) float pairs ("complex64"), layout [B][H][W] row-major,
 *     k-space in un-shifted FFT order (DC at [0,0]), forward transform unnormalised, inverse
 *     carrying 1/(H*W) -- exactly np.fft.fft2 / np.fft.ifft2.
 *   - "dev" pointers are device pointers borrowed from the caller (never freed by the library);
 *     functions taking `on_device` accept either host or device memory.
 *   - all kernels are asynchronous on the ctx stream (pnp_set_stream); only pnp_sync,
 *     host-side downloads and pnp_timer_stop block.
 *   - one ctx per device per host thread; a ctx is not re-entrant.
 *   - hyper-parameters (alpha, lambda1, reo, b, thresholds) are C doubles, as the Python floats of
 *     the reference are; derived coefficients are formed in double and rounded to float once.
 *   - H, W in {256, 512} (pnp_ctx_create[_f64]), or both in [128, 1024] (pnp_ctx_create_any[_f64], since ABI 12).
 *     B <= Bmax.  256x256 and 512x512 keep their fast paths; every other shape of an any-size context runs the generic
 *     three-launch iteration on the any-size FFT kernels: mixed-radix (2, 3, 4, 5, 7) Stockham transforms for 7-smooth
 *     lengths, Bluestein (a power-of-two convolution of length <= 2048) for the rest (pnp_ctx_path, pnp_fft_plan).
 */
#ifndef PNP_MRI_H
#define PNP_MRI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNP_OK            0
#define PNP_E_ARG        -1   /* bad argument (null, size, unsupported H/W) */
#define PNP_E_HIP        -2   /* a HIP runtime call failed                  */
#define PNP_E_STATE      -3   /* call order (e.g. run before upload)        */
#define PNP_E_NOMEM      -4

#define PNP_ABI_VERSION   13

typedef struct pnp_ctx pnp_ctx;

/* ---- library / context ------------------------------------------------------------------ */
int         pnp_abi_version(void);
const char* pnp_last_error(void);
/* number of HIP devices visible (0 and PNP_OK when there is none). */
int         pnp_device_count(int* n);
/* What a measurement needs to be attributable to a card (bench.py's `config.device`): the shader clock the driver reports (MHz), the number of
 * compute units, the PCI bus id ("0000:05:00.0") and the architecture name ("gfx950...").  Strings are truncated to their buffers.  ABI 11. */
int         pnp_device_info(int device, int* clock_mhz, int* compute_units, char* pci_bus_id, int pci_len, char* arch, int arch_len);
/* CALIBRATION, not product: a streaming kernel with the slice-resident loop's ACCESS SHAPE and none of its arithmetic -- one 512-thread
 * workgroup per "slice" (256 KiB), 16 bytes per lane, eight accesses in flight per wave; per pass it reads z, w and a table and writes z, w
 * back (5 x 256 KiB) -- run back to back on `slices` slices for at least `seconds`; *gbs = bytes moved / HIP-event time.  What this card's
 * memory system gives such a kernel today: bench.py prints its own fraction of 8 TB/s next to the fraction of THIS number (boxes of a pool
 * differ by several per cent).  Allocates and frees 3 x slices x 256 KiB.  ABI 11. */
int         pnp_calibrate_stream(int device, int slices, double seconds, double* gbs);

int pnp_ctx_create(int device, int H, int W, int Bmax, pnp_ctx** out);
int pnp_ctx_destroy(pnp_ctx* ctx);
/* hipStream_t as void*; NULL = the default stream.  PnP solvers pass torch's current stream. */
int pnp_set_stream(pnp_ctx* ctx, void* hip_stream);
int pnp_sync(pnp_ctx* ctx);
/* 0 = generic kernels only, 1 = allow the fused gfx950 kernels where shapes permit (default). */
int pnp_set_fast_path(pnp_ctx* ctx, int enable);
/* Scheduling of the fused loops (results are bit-identical for every setting):
 *   queues          1..4 HIP queues the batch is split over (default 2; forked/joined on the ctx stream)
 *   mixed_launches  256x256 two-launch path: row workgroups of one half of a part share each launch with the column
 *                   workgroups of its other half (default 0: retired in round 2 -- measured within noise of plain row and
 *                   column launches on two queues; kept as a knob)
 *   chunk           >0: a queue runs all iterations on `chunk` slices before its next chunk; 0 (default): the path's own
 *                   default -- at 512x512 and for the double-precision 256x256 engine the chunks go round-robin to 4 queues
 *                   (16 resp. 24 slices each with queues >= 2; 48 resp. 96 on one queue), so the chunks in flight fit the
 *                   256 MiB Infinity Cache for a whole run; whole batch otherwise; <0: whole batch
 * Environment defaults read (once, range-checked: a malformed value fails pnp_ctx_create with PNP_E_ARG) at pnp_ctx_create:
 * PNP_FUSED_STREAMS, PNP_FUSED_SCHED, PNP_FUSED_CHUNK; PNP_SLICE (0 / 1), PNP_SLICE_MIN_B, PNP_SLICE_PAD_KB, PNP_SLICE_YH_PAD_KB,
 * PNP_FUSED_COLS.  The experiment knobs of the profiling scripts exist only in -DPNP_EXPERIMENT_KNOBS builds. */
int pnp_set_schedule(pnp_ctx* ctx, int queues, int mixed_launches, int chunk);
/* the schedule in force (any pointer may be NULL) */
int pnp_get_schedule(pnp_ctx* ctx, int* queues, int* mixed_launches, int* chunk);
/* what the next pnp_admm_*_run will do for the uploaded batch on the path in use: HIP queues, slices per chunk (the batch
 * size when it is not chunked), kernel launches per batched iteration (0: slice-resident, the iterations are a loop inside one
 * launch).  Any pointer may be NULL.  New in ABI 7; no counterpart in the reference. */
int pnp_get_plan(pnp_ctx* ctx, int* queues, int* chunk, int* launches_per_iteration);

/* ---- problem upload ---------------------------------------------------------------------- */
/* y: [B][H][W] complex64, the measurements  y = fft2(img)*mask + noises  (S4:102).
 * mask_bank: [K][H][W] uint8 in {0,1}, FFT-native layout (CS_MRI/Q_*.mat variable Q1; S4:185).
 * mask_id:   [B] int32 in [0,K): which mask each slice uses (NULL = all slices use mask 0);
 *            validated for host and device inputs alike (PNP_E_ARG when out of range).
 * Replaces the per-image `y`, `index = np.nonzero(mask)` set-up of S4:101-106.
 * A new problem (this call, pnp_synthesize_problem and their _f64 forms) INVALIDATES the ADMM state and x of the problem before it:
 * z, w and x are undefined until pnp_init_state, or pnp_set_state with BOTH z and w, has run -- the reference likewise builds z and w
 * anew per image (S4:103-109).  Until then every entry point that would read them (pnp_admm_l1_run, pnp_admm_cnc_run, pnp_get_state,
 * pnp_set_state with only one of z / w, and their _f64 forms) returns PNP_E_STATE. */
int pnp_upload_problem(pnp_ctx* ctx, const float* y, const uint8_t* mask_bank,
                       const int32_t* mask_id, int B, int K, int on_device);

/* On-device measurement synthesis (S4:102, "noise on all points"):
 * y = fft2(img)*mask + noise.  img: [B][H][W] float32; noise: [B][H][W] complex64 or, with
 * noise_per_slice = 0, one [H][W] complex64 array shared by all slices (the reference's
 * noises.mat).  Masks as in pnp_upload_problem.  Leaves y in the ctx like pnp_upload_problem. */
int pnp_synthesize_problem(pnp_ctx* ctx, const float* img, const float* noise, int noise_per_slice,
                           const uint8_t* mask_bank, const int32_t* mask_id, int B, int K,
                           int on_device);
/* copy the ctx's y back ([B][H][W] complex64). */
int pnp_download_y(pnp_ctx* ctx, float* y, int on_device);

/* z0 = |ifft2(y)| (complex modulus), w0 = 0                                     (S4:103-109) */
int pnp_init_state(pnp_ctx* ctx);
/* overwrite / read the ctx-owned ADMM state z, w ([B][H][W] float32 each); NULL skips one. */
int pnp_set_state(pnp_ctx* ctx, const float* z, const float* w, int on_device);
int pnp_get_state(pnp_ctx* ctx, float* z, float* w, int on_device);

/* Build now the per-problem tables the whole loops below will use (256x256 float contexts build them on the first loop call
 * otherwise: the slice-resident tables only when a loop really takes that path, so that step-wise PnP users never pay for
 * them).  Optional; benchmarks call it to keep table building out of a timed region without warm-up.  New in ABI 8. */
int pnp_prepare_loops(pnp_ctx* ctx);

/* ---- whole loops on the ctx-owned state (no host sync inside) ----------------------------- */
/* iters = 0: the loop body never runs; x is set to the current z (the reference's x = |ifft2(y)| = z0
 * straight after pnp_init_state, S4:103-107, 138).
 * ADMM_L1 main loop, S1:111-126:  x = dc(z,w); z = soft(x+w, reo*lambda1); w += x - z. */
int pnp_admm_l1_run(pnp_ctx* ctx, int iters, double lambda1, double reo);
/* ADMM_CNC main loop, S4:115-132: x = dc(z,w); s = soft(z,1/b);
 * t = (1-alpha) z + alpha (x+w) + alpha*reo*lambda1*b (z-s); z = soft(t, alpha*reo*lambda1);
 * w += x - z. */
int pnp_admm_cnc_run(pnp_ctx* ctx, int iters, double alpha, double lambda1, double reo, double b);
/* ---- convergence trace and residual-based stopping (new in ABI 13; the reference has no counterpart: its loops, S1:111-126 and
 * S4:115-132, run a fixed iter_num and keep nothing but the last x) ---------------------------------------------------------
 * The same loops as pnp_admm_l1_run / pnp_admm_cnc_run (S4:115-132 is the loop they observe), with the state reduced at CHECKED
 * iterations: every multiple of `every` (>= 1) that is <= the iterations run, plus the last iteration run if it is not one.
 * Row of a check at iteration k (k completed iterations, 1-based), per slice, PNP_TRACE_Q values:
 *   r_pri = ||x_k - z_k||, r_dual = ||z_k - z_{k-1}|| (z_0: the state the call started from), ||x_k||, ||z_k||, ||w_k||, and --
 *   with a ground truth gt (uint8 [B][H][W], host or device as for pnp_metrics; NULL: none, the two values are NaN) -- PSNR and
 *   RE of img_E = 255 x_k by pnp_metrics' formulas, so the row of the last iteration equals pnp_metrics of the returned x.
 * x, z, w are what the loop holds after iteration k -- what pnp_download_x / pnp_get_state return after an untraced run of k
 * iterations, bit for bit: the run is cut into launches at k - 1 and k (a run split into launches equals one launch), z of
 * k - 1 is copied, and ONE reduction kernel per check (all slices, double accumulation, a fixed tree: the same inputs give the
 * same bits) reads the state where it lies.  No loop kernel differs from the untraced call's.
 * tol <= 0: no stopping rule; the host reads nothing until the run is over.  tol > 0: slice b MEETS the rule at a check when
 *   max(r_pri, r_dual) <= tol * ||z_k||;  the run stops after the first check at which every slice meets it (all slices always
 *   run the same number of iterations); one small copy and one synchronisation per check.
 * Outputs: *checks = rows recorded, *iters_done = iterations run (= iters unless stopped).  iters = 0: zero checks and exactly
 * pnp_admm_*_run(iters = 0).  every < 1: PNP_E_ARG.  The rows are kept by the context until its next traced run: */
#define PNP_TRACE_R_PRI   0
#define PNP_TRACE_R_DUAL  1
#define PNP_TRACE_X_NORM  2
#define PNP_TRACE_Z_NORM  3
#define PNP_TRACE_W_NORM  4
#define PNP_TRACE_PSNR    5
#define PNP_TRACE_RE      6
#define PNP_TRACE_Q       7
int pnp_admm_l1_run_traced(pnp_ctx* ctx, int iters, double lambda1, double reo, int every, double tol,
                           const uint8_t* gt, int gt_on_device, int* checks, int* iters_done);
int pnp_admm_cnc_run_traced(pnp_ctx* ctx, int iters, double alpha, double lambda1, double reo, double b, int every, double tol,
                            const uint8_t* gt, int gt_on_device, int* checks, int* iters_done);
/* The last traced run of the context (host arrays; any pointer may be NULL): iters [checks] the checked iterations,
 * values [checks][PNP_TRACE_Q][B] as above, converged_at [B] the first checked iteration at which the slice met the rule (0: never,
 * or no tol). */
int pnp_trace_read(pnp_ctx* ctx, int32_t* iters, double* values, int32_t* converged_at);
/* x of the last iteration ([B][H][W] float32) -- what the solvers return (S4:138). */
int pnp_download_x(pnp_ctx* ctx, float* x, int on_device);

/* ---- step-wise operators on caller-owned device pointers (the PnP path) ------------------- */
/* x-update / data-consistency solve, S4:119-124 == S6:266-271:
 *   X = fft2(z - w); X[mask] = (La2*X[mask] + y[mask])/(1+La2), La2 = 1/(2 reo);
 *   x = |Re ifft2(X)|.      z, w, x: [B][H][W] float32 device pointers (x may alias neither). */
int pnp_dc_step(pnp_ctx* ctx, const float* z_dev, const float* w_dev, float* x_dev, double reo);
/* The five pointwise calls below (pnp_prox_l1_dual, pnp_prox_cnc_dual, pnp_cnc_combine, pnp_add, pnp_dual_clamp) accept any float
 * pointer: arrays that are all aligned to 16 bytes take the vector path, others a slower scalar one with the same results. */
/* z = soft(x + w, thr); w = w + x - z                                           (S1:123,126) */
int pnp_prox_l1_dual(pnp_ctx* ctx, const float* x_dev, float* z_dev, float* w_dev, double thr);
/* CNC z-update + dual update                                                 (S4:127-129,132) */
int pnp_prox_cnc_dual(pnp_ctx* ctx, const float* x_dev, float* z_dev, float* w_dev,
                      double alpha, double lambda1, double reo, double b);
/* t = (1-alpha) z + alpha (x+w) + alpha*reo*lambda1*b (z - s)                       (S6:301) */
int pnp_cnc_combine(pnp_ctx* ctx, const float* z_dev, const float* x_dev, const float* w_dev,
                    const float* s_dev, float* t_dev, double alpha, double lambda1, double reo, double b);
/* t = x + w  (the denoiser input of PNP_ADMM_L1_D, S3:290) */
int pnp_add(pnp_ctx* ctx, const float* a_dev, const float* b_dev, float* out_dev);
/* w = w + x - z, then x,z,w <- clamp(.,0,1) with torch.clamp_'s semantics: NaN stays NaN, +-inf go to the bounds, so a
 * non-finite denoiser output reaches the returned x instead of turning into 0                (S6:305-308) */
int pnp_dual_clamp(pnp_ctx* ctx, float* x_dev, float* z_dev, float* w_dev);

/* The reduction of the traced loops alone, on caller-owned device tensors in natural order (what the PnP solvers call after
 * pnp_dual_clamp; new in ABI 13): out [PNP_TRACE_Q][B] doubles, the SUMS OF SQUARES behind a trace row, per slice --
 *   sum (x - z)^2, sum (z - z_prev)^2, sum x^2, sum z^2, sum w^2, sum (255 x' - gt)^2, sum gt^2
 * -- the last two 0 with gt = NULL; x' = x, or with quantise != 0 round(255 x) * (1 / 255) in the state's arithmetic (the img_E the PnP solvers
 * score, S6:314, as torch forms round(x * 255) / 255 on the device: half to even, times the reciprocal).
 * out is host memory (the call synchronises) or, with out_on_device, device memory (asynchronous on the ctx stream; it must not
 * overlap an input: PNP_E_ARG).  The inputs may alias each other.  One launch, deterministic. */
int pnp_residuals(pnp_ctx* ctx, const float* x_dev, const float* z_dev, const float* zprev_dev, const float* w_dev,
                  const uint8_t* gt, int gt_on_device, int quantise, double* out, int out_on_device);

/* ---- operator API (batched; B slices of the ctx's H x W; complex64 device pointers) ------- */
int pnp_fft2_fwd(pnp_ctx* ctx, const float* in_dev, float* out_dev, int B);   /* np.fft.fft2  */
int pnp_fft2_inv(pnp_ctx* ctx, const float* in_dev, float* out_dev, int B);   /* np.fft.ifft2 */
/* A x = fft2(x) * mask (x real [B][H][W]); uses the uploaded masks.                 (S4:102) */
int pnp_A(pnp_ctx* ctx, const float* x_dev, float* k_dev);
/* A^H k = ifft2(k * mask) -> complex [B][H][W]                         (utils/utils.py:54) */
int pnp_AH(pnp_ctx* ctx, const float* k_dev, float* out_dev);
/* Df(x, mask, y) = ifft2(mask*fft2(x) - mask*y), x real -> complex    (utils/utils.py:50-55) */
int pnp_Df(pnp_ctx* ctx, const float* x_dev, float* out_dev);

/* ---- metrics (utils/utils_image.py:543-556, 622-636), per slice -------------------------- */
/* img_E = x*255 vs ground truth gt (uint8 [B][H][W]); writes psnr[b] (dB) and re[b].
 * x_dev = NULL means the ctx-owned x of the last pnp_admm_*_run. */
int pnp_metrics(pnp_ctx* ctx, const float* x_dev, const uint8_t* gt, int gt_on_device,
                double* psnr_host, double* re_host);

/* SSIM of img_E = x*255 vs gt per slice (utils/utils_image.py:570-615: Gaussian 11/1.5 window,
 * valid region, gray images), computed in double on the device.  x_dev = NULL: the ctx-owned x. */
int pnp_ssim(pnp_ctx* ctx, const float* x_dev, const uint8_t* gt, int gt_on_device, double* ssim_host);

/* ---- double-precision context -------------------------------------------------------------
 * The same loops (pnp_init_state, pnp_admm_l1_run, pnp_admm_cnc_run) with every buffer and every
 * arithmetic step in double / complex128: the reference itself runs in float64 (S4:109
 * `w = np.zeros(..., dtype=np.float64)`), and its committed CNC presets amplify fp32 round-off
 * ~1.08x per iteration, so this is the mode in which 100-iteration CNC runs meet 1e-5 end to end.
 * 256x256 runs on the fused two-launch kernels in double (a throughput path: ~2500 batched
 * iterations/s at 512 slices); other shapes on the generic kernels in double.
 * Since ABI 8 everything the whole-solver entry points need exists in double (synthesis, metrics, SSIM), so
 * ADMM_L1 / ADMM_CNC (precision='f64') run the reference's own arithmetic end to end; the step-wise / operator entry points
 * (PnP path: the reference itself switches to float32 there, S6:273-285) are float-only and return PNP_E_STATE on such a context. */
int pnp_ctx_create_f64(int device, int H, int W, int Bmax, pnp_ctx** out);
/* The same two creations for any H, W in [128, 1024] (since ABI 12); shapes in {256, 512}^2 get exactly the context the calls
 * above make.  Outside the range: PNP_E_ARG. */
int pnp_ctx_create_any(int device, int H, int W, int Bmax, pnp_ctx** out);
int pnp_ctx_create_any_f64(int device, int H, int W, int Bmax, pnp_ctx** out);
/* y: [B][H][W] complex128 (interleaved doubles); masks as pnp_upload_problem. */
int pnp_upload_problem_f64(pnp_ctx* ctx, const double* y, const uint8_t* mask_bank,
                           const int32_t* mask_id, int B, int K, int on_device);
/* y = fft2(img)*mask + noise in double (S4:102): img [B][H][W] float32 (the reference's img_L is float32,
 * utils/utils_image.py:181-182), noise complex128 [H][W] (noise_per_slice = 0: the reference's noises.mat) or [B][H][W].
 * The float32 image is widened exactly and transformed in double; NumPy >= 2 runs this one transform in complex64 before
 * promoting it, so the two y differ by that transform's float32 round-off (~1e-7 relative), which the committed CNC presets
 * amplify to ~2e-6 after 50 iterations -- inside the 1e-5 bar (tests/test_gpu_f64.py).  New in ABI 8. */
int pnp_synthesize_problem_f64(pnp_ctx* ctx, const float* img, const double* noise, int noise_per_slice,
                               const uint8_t* mask_bank, const int32_t* mask_id, int B, int K, int on_device);
/* copy the ctx's y back ([B][H][W] complex128).  New in ABI 8. */
int pnp_download_y_f64(pnp_ctx* ctx, double* y, int on_device);
int pnp_set_state_f64(pnp_ctx* ctx, const double* z, const double* w, int on_device);
int pnp_get_state_f64(pnp_ctx* ctx, double* z, double* w, int on_device);
int pnp_download_x_f64(pnp_ctx* ctx, double* x, int on_device);
int pnp_is_f64(pnp_ctx* ctx);
/* pnp_metrics / pnp_ssim on a double-precision context: img_E = x*255 formed in double from the float64 x, exactly as the
 * reference does (S4:139, 149-151).  x_dev = NULL: the ctx-owned x.  New in ABI 8. */
int pnp_metrics_f64(pnp_ctx* ctx, const double* x_dev, const uint8_t* gt, int gt_on_device,
                    double* psnr_host, double* re_host);
int pnp_ssim_f64(pnp_ctx* ctx, const double* x_dev, const uint8_t* gt, int gt_on_device, double* ssim_host);
/* pnp_residuals on a double-precision context (double device tensors).  New in ABI 13. */
int pnp_residuals_f64(pnp_ctx* ctx, const double* x_dev, const double* z_dev, const double* zprev_dev, const double* w_dev,
                      const uint8_t* gt, int gt_on_device, int quantise, double* out, int out_on_device);

/* ---- wavelet-domain sparsity (added after ABI 13, additive) -------------------------------------
 * ADMM_L1 / ADMM_CNC with their penalty on the WAVELET COEFFICIENTS of the image instead of its pixels.  This regulariser has NO
 * counterpart in the reference scripts (their prox acts on the pixels: S1:123, S4:127-129); with PNP_WAVELET_NONE -- the default --
 * every entry point is bit for bit what it was.
 * Psi is the orthonormal periodic 2-D DWT with low-pass filter h of length T and g[n] = (-1)^n h[T-1-n]:
 *   haar  T = 2  [1, 1] / sqrt 2
 *   db2   T = 4  [1 + sqrt 3, 3 + sqrt 3, 3 - sqrt 3, 1 - sqrt 3] / (4 sqrt 2)
 *   db4   T = 8  minimum-phase Daubechies, four vanishing moments: 0.2303778133, 0.7148465706, 0.6308807679, -0.0279837694, ...
 * one level along an axis of length M:  a[k] = sum_n h[n] s[(2k + n) mod M],  d[k] = sum_n g[n] s[(2k + n) mod M],  k < M / 2;
 * synthesis is the transpose.  2-D, `levels` levels, Mallat layout: level l = 0 .. levels - 1 works on the top-left
 * (H >> l) x (W >> l) block, rows first ([a | d]), then columns ([a ; d]); the final LL band is the top-left
 * (H >> levels) x (W >> levels) and is never thresholded.  With u = x + w and "detail" = every coefficient outside that band:
 *   L1   c = Psi u;  c <- soft(c, thr) on detail;  z+ = Psi^T c;  w+ = u - z+
 *   CNC  cz = Psi z, cu = Psi u;  t = (1 - alpha) cz + alpha cu  [+ alpha reo lambda1 b clip(cz, -1/b, 1/b) on detail];
 *        z+ = Psi^T (soft(t, alpha reo lambda1) on detail, t on LL);  w+ = u - z+
 * (scalars combined in double and rounded once, as for the pixel-domain step).  Two launches per prox, both precisions.
 * Valid: 1 <= levels <= 4, H and W divisible by 2^levels, min(H, W) >> (levels - 1) >= T; anything else is PNP_E_ARG, decided by
 * pnp_sparsity_check -- no context, no device -- which pnp_set_sparsity calls before any device work. */
#define PNP_WAVELET_NONE 0
#define PNP_WAVELET_HAAR 1
#define PNP_WAVELET_DB2  2
#define PNP_WAVELET_DB4  3
int pnp_sparsity_check(int wavelet, int levels, int H, int W);
/* PNP_WAVELET_NONE (the default): `levels` is ignored and everything is as before.  With a wavelet set
 *   - pnp_admm_l1_run, pnp_admm_cnc_run and their _traced forms run, per iteration, the context's own data-consistency step (what
 *     pnp_dc_step launches: the two-launch engine where the shape has one, the generic / any-size kernels otherwise; three launches)
 *     and the two prox launches: five launches per iteration, which pnp_get_plan / pnp_kernels_per_iteration report.  The state
 *     stays in natural order, the slice-resident path is never taken (pnp_path_name says "fused"), a run cut into calls is bit-equal
 *     to one call, and the same loop body runs in double on a double-precision context.  The traced forms check the iterations they
 *     always check, with pnp_residuals' reduction.  iters = 0 behaves as without a wavelet.
 *   - pnp_prox_l1_dual and pnp_prox_cnc_dual apply the wavelet-domain step (x, z, w must not overlap).
 * The setting belongs to the context and survives uploads.  The first non-NONE setting allocates one scratch array of Bmax slices. */
int pnp_set_sparsity(pnp_ctx* ctx, int wavelet, int levels);
int pnp_get_sparsity(pnp_ctx* ctx, int* wavelet, int* levels);
/* Psi / Psi^T alone with the context's setting on B <= Bmax real slices [B][H][W] (no problem needed); in_dev may EQUAL out_dev
 * (bit-equal to the out-of-place call), any other overlap is PNP_E_ARG.  PNP_WAVELET_NONE set: PNP_E_STATE. */
int pnp_dwt2_fwd(pnp_ctx* ctx, const float* in_dev, float* out_dev, int B);
int pnp_dwt2_inv(pnp_ctx* ctx, const float* in_dev, float* out_dev, int B);
/* the same on a double-precision context (double tensors) */
int pnp_dwt2_fwd_f64(pnp_ctx* ctx, const double* in_dev, double* out_dev, int B);
int pnp_dwt2_inv_f64(pnp_ctx* ctx, const double* in_dev, double* out_dev, int B);

/* ---- cycle spinning for the wavelet prox (added after ABI 13, additive) ---------------------------
 * The decimated transform above is not translation invariant: its prox leaves artefacts tied to the 2^levels grid.  Cycle spinning
 * applies the prox in a circularly shifted frame, another shift every prox step, optionally averaging a few shifts per step.
 * Shift s = (sy, sx), 0 <= sy, sx < 2^levels:  (R_s v)[i, j] = v[(i + sy) mod H, (j + sx) mod W];  Psi_s = Psi R_s.  The shifted prox step
 * is the step above in that frame: x, z, w rolled by (-sy, -sx), the step, z+ and w+ rolled back -- done by addressing, the kernels,
 * their two launches and their bytes are those of the unshifted step, and s = (0, 0) gives its bits.
 * Schedule: a table shifts[n][2] (sy, sx), 1 <= n <= 4096, a group size per_prox = K, 1 <= K <= 16, n a multiple of K, and a cursor p
 * that counts prox steps: step p uses entries (p mod (n / K)) K + j, j = 0 .. K - 1, then p += 1.  pnp_init_state and pnp_set_spin
 * set p = 0, pnp_set_state leaves it, pnp_set_spin_cursor sets it: a run cut into calls stays bit-equal to one call.
 * Averaging (K > 1): with z_j the z+ of shift j, all K from the same (x, z, w):  acc = z_0;  acc = acc + z_j, j = 1 .. K - 2, in order;
 * z+ = (acc + z_(K-1)) r,  r = 1 / K rounded once to the context's precision;  w+ = (x + w) - z+.  K = 1 multiplies nothing.  A prox
 * is 2 K launches; z and w are written by the last one only.  The first K > 1 allocates one more array of Bmax slices.
 * The rules are decided by pnp_spin_check -- no context, no device; PNP_E_ARG with a message that names the rule: "n", "per_prox",
 * "multiple", "range" -- which pnp_set_spin calls with the context's levels before any device work. */
int pnp_spin_check(int levels, const int32_t* shifts, int n, int per_prox);
/* n = 0 clears the setting (shifts_host is not read).  No wavelet set: PNP_E_STATE.  pnp_set_sparsity clears the setting (the valid
 * range depends on levels).  With a setting, every wavelet prox of the context follows and advances the schedule: the loops, their
 * _traced forms, the loops of a coil context, and pnp_prox_l1_dual / pnp_prox_cnc_dual.  pnp_get_plan / pnp_kernels_per_iteration
 * report 3 + 2 K launches per iteration, 5 + 5 cg_iters + 2 K on a coil context. */
int pnp_set_spin(pnp_ctx* ctx, const int32_t* shifts_host, int n, int per_prox);
/* n = 0, per_prox = 1 without a setting; any pointer may be null */
int pnp_get_spin(pnp_ctx* ctx, int* n, int* per_prox, int* cursor);
/* cursor >= 0; PNP_E_STATE without a setting */
int pnp_set_spin_cursor(pnp_ctx* ctx, int cursor);
/* Psi_s (inverse = 0) / Psi_s^T (inverse != 0) alone, as pnp_dwt2_fwd / _inv (in_dev may equal out_dev); (sy, sx) outside
 * [0, 2^levels) is PNP_E_ARG.  pnp_dwt2_fwd / _inv stay unshifted whatever the spin setting. */
int pnp_dwt2_shifted(pnp_ctx* ctx, const float* in_dev, float* out_dev, int B, int inverse, int sy, int sx);
int pnp_dwt2_shifted_f64(pnp_ctx* ctx, const double* in_dev, double* out_dev, int B, int inverse, int sy, int sx);

/* ---- multi-coil (SENSE) data consistency (added after ABI 13, additive) --------------------------
 * Measurements from C receive coils with complex sensitivity maps S_c:  y_c = m . fft2(S_c . x),  c = 0 .. C - 1.  NOT in the reference
 * scripts, whose forward model is one coil of uniform sensitivity; without coils -- the default -- every entry point is bit for bit what
 * it was.  Conventions as everywhere here: fft2 unnormalised, ifft2 carries 1 / (H W); La2 = 1 / (2 reo); v = z - w is real.
 *   (A x)_c = m . fft2(S_c . x)         A^H k = sum_c conj(S_c) . ifft2(m . k_c)         G p = A^H A p + La2 p
 * The x-step solves  G x^ = A^H y + La2 v  over complex x^ by `cg_iters` iterations of plain conjugate gradients warm-started at x^ = v
 *   r = A^H y + La2 v - G v, p = r;  per iteration  alpha = <r,r> / Re<p,Gp>,  x^ += alpha p,  r -= alpha Gp,  beta = <r+,r+> / <r,r>,
 *   p = r+ + beta p   (a zero denominator gives alpha resp. beta = 0, never a NaN)
 * and returns x = |Re x^|.  With C = 1 and S = 1 this is the reference's closed form after ONE iteration.  The initial state is
 * z = |A^H y|, w = 0.  The z- and w-steps are untouched (pixel prox, wavelet prox, the denoisers of the PnP solvers).
 * Convergence (maps normalised to sum_c |S_c|^2 = 1, 30 % sampling): the relative distance from the converged solve after 1 / 2 / 3
 * iterations is 1.1e-4 / 2.8e-6 / 4.9e-8 at reo = 0.05 and 1.1e-5 / 8.6e-8 / 4.7e-10 at reo = 0.015: the default is 3.  UNNORMALISED MAPS
 * OR A LARGE reo (2.75: condition number about 6.5) NEED MORE: raise cg_iters and watch pnp_cg_residual.
 * Layout: maps [Ks][C][H][W] interleaved complex in the context's precision -- a bank of Ks coil sets, slice b uses set coil_id[b]
 * (null: set 0); every k-space argument of a coil context is [B][C][H][W].  On the device one application of G is three launches of the
 * any-size transform kernels AT EVERY SHAPE (a 256 x 256 or 512 x 512 coil context never enters the slice-resident or two-launch
 * engines; pnp_path_name says "coils"), an x-step is 5 + 5 cg_iters launches with no host synchronisation, and every sum runs in a
 * fixed order that depends on (H, W) alone: results are bit-equal from run to run and for a slice alone or inside a batch.
 * pnp_coils_check: the argument rule (1 <= C <= 32, Ks >= 1, H and W in [128, 1024]) without a context or a device. */
int pnp_coils_check(int C, int Ks, int H, int W);
/* Sets (C >= 1) or clears (C = 0; sens and Ks ignored) the coils of the context.  Either way the uploaded problem is dropped (the next
 * call that needs one returns PNP_E_STATE until an upload).  Setting allocates two [Bmax][C][H][W] complex arrays (transform
 * intermediate, measurements) and five [Bmax][H][W] complex ones; an allocation that fails is PNP_E_NOMEM with the number of bytes asked
 * for in the message, and leaves the context without coils.  A batch whose arrays do not fit is not chunked. */
int pnp_set_coils(pnp_ctx* ctx, const float* sens, int C, int Ks, int on_device);
int pnp_set_coils_f64(pnp_ctx* ctx, const double* sens, int C, int Ks, int on_device);
/* CG iterations per x-step, 1 .. 64 (default 3); belongs to the context, survives pnp_set_coils. */
int pnp_set_cg(pnp_ctx* ctx, int iters);
int pnp_get_coils(pnp_ctx* ctx, int* C, int* Ks, int* cg_iters);          /* C = 0: no coils */
/* The problem of a coil context: y [B][C][H][W]; coil_id [B] or null.  A^H y is formed here, once.  The single-coil entry points
 * (pnp_upload_problem, pnp_synthesize_problem and their _f64 forms) fail with PNP_E_STATE on a coil context, these on one without. */
int pnp_upload_problem_mc(pnp_ctx* ctx, const float* y, const uint8_t* mask_bank, const int32_t* mask_id, const int32_t* coil_id,
                          int B, int K, int on_device);
int pnp_upload_problem_mc_f64(pnp_ctx* ctx, const double* y, const uint8_t* mask_bank, const int32_t* mask_id, const int32_t* coil_id,
                              int B, int K, int on_device);
/* y_c = m . fft2(S_c . img) + noise (the noise is added at EVERY k-space point, as pnp_synthesize_problem does).  noise_mode 0: one
 * [H][W] array for all coils and slices; 1: [C][H][W], shared by the slices; 2: [B][C][H][W]. */
int pnp_synthesize_problem_mc(pnp_ctx* ctx, const float* img, const float* noise, int noise_mode, const uint8_t* mask_bank,
                              const int32_t* mask_id, const int32_t* coil_id, int B, int K, int on_device);
int pnp_synthesize_problem_mc_f64(pnp_ctx* ctx, const float* img, const double* noise, int noise_mode, const uint8_t* mask_bank,
                                  const int32_t* mask_id, const int32_t* coil_id, int B, int K, int on_device);
/* On a coil context pnp_init_state, pnp_admm_l1_run, pnp_admm_cnc_run, their _traced forms and pnp_dc_step follow the mathematics
 * above; pnp_A takes x [B][H][W] real to k [B][C][H][W], pnp_AH takes k to a complex image [B][H][W] (k is not modified);
 * pnp_download_y[_f64] returns [B][C][H][W]; pnp_get_plan / pnp_kernels_per_iteration report 5 + 5 cg_iters launches plus the prox (1, or
 * 2 with a wavelet); pnp_Df fails with PNP_E_STATE.
 * pnp_cg_residual: ||r|| / ||A^H y + La2 v|| of the most recent x-step, per slice, rel [B] on the host (synchronises). */
int pnp_cg_residual(pnp_ctx* ctx, double* rel);

/* ---- complex-valued images on a coil context (added after ABI 13, additive) ----------------------
 * The loops above return a real, non-negative image: x = |Re x^|, z0 = |A^H y|.  Measured multi-coil data has an image phase that the
 * maps do not absorb (flow, off-resonance, a step at a tissue boundary); complex mode keeps it.  NOT in the reference scripts.  Opt-in per
 * context (pnp_set_image); with the mode off -- the default -- nothing here is called and every result is bit for bit what it was.
 * State: x, z, w are [B][H][W] interleaved complex in the context's precision.  z0 = A^H y (no modulus), w0 = 0.
 * x-step:  G x^ = A^H y + La2 (z - w)  by the CG above, warm-started at x^ = z - w (complex);  x = x^ (no |Re .|).  The CG arithmetic, its
 *   sums and pnp_cg_residual are those of the real mode.
 * csoft(u, c), the prox of c |.| on a complex number:  m2 = u.re u.re + u.im u.im  (two rounded products, one sum, no fma),  m = sqrt(m2),
 *   s = (m - c) / m  where m > c  and  s = 0  otherwise (m = 0 included);  csoft = (s u.re, s u.im).
 * cclip(z, ib), the projection onto the disc of radius ib (= z - csoft(z, ib)):  z (ib / m)  where m > ib,  z otherwise;  m as above.
 * L1 step:   u = x + w;  z+ = csoft(u, thr);  w+ = u - z+.                                    thr = reo lambda1
 * CNC step:  u = x + w;  t = c1 z + c2 u + c3 cclip(z, ib), component-wise, each component fma(c1, z, fma(c2, u, c3 * clip));
 *            z+ = csoft(t, thr);  w+ = u - z+.        thr = alpha reo lambda1, c1 = 1 - alpha, c2 = alpha, c3 = thr b, ib = 1 / b
 *   With zero imaginary parts both are the real steps (soft, clip) up to the rounding of (m - c) / m and ib / m.
 * Wavelet prox (pnp_set_sparsity):  Psi is real-linear and acts on the real and the imaginary part alike;  detail coefficients are
 *   thresholded by csoft on the COMPLEX coefficient (L1: csoft(c_u, thr); CNC: the CNC step on the coefficients c_z, c_u), approximation
 *   coefficients pass through (L1: c_u; CNC: c1 c_z + c2 c_u);  z+ = Psi^T of the result,  w+ = u - z+.  Two launches, as in real mode.
 *   One setting does not fit the LDS on complex doubles -- db4 with 4 levels on an fp64 context -- and is PNP_E_ARG from whichever of
 *   pnp_set_image / pnp_set_sparsity comes second; pnp_image_check(mode, wavelet, levels, f64) decides it without a context or a device.
 *   That second call also allocates the [Bmax][H][W] complex coefficient array (PNP_E_NOMEM names the bytes): no loop allocates.
 * pnp_set_image rules, the first broken one is named:  ctx null: PNP_E_ARG;  mode not PNP_IMAGE_REAL / PNP_IMAGE_COMPLEX: PNP_E_ARG;
 *   complex mode on a context without coils: PNP_E_STATE (set them first: pnp_set_coils);  complex mode with a spin table set
 *   (pnp_set_spin): PNP_E_STATE.  The call drops the uploaded problem, as pnp_set_coils does; the first complex one allocates three
 *   [Bmax][H][W] complex arrays (PNP_E_NOMEM names the bytes).  pnp_set_coils -- clearing or setting -- returns the context to real mode.
 * In complex mode
 *   pnp_init_state, pnp_admm_l1_run, pnp_admm_cnc_run follow the mathematics above; pnp_get_plan reports the same launch counts as in
 *     real mode (the complex steps are launch for launch the real ones); pnp_path_name stays "coils"; pnp_metrics / pnp_ssim with
 *     x_dev = null score |x|;
 *   the real state calls (pnp_set_state, pnp_get_state), pnp_download_x, pnp_dc_step, pnp_prox_l1_dual, pnp_prox_cnc_dual and their _f64
 *     forms return PNP_E_STATE and name their _cx counterpart;
 *   pnp_admm_l1_run_traced, pnp_admm_cnc_run_traced, pnp_residuals[_f64] and pnp_set_spin return PNP_E_STATE ("not available in complex
 *     image mode").
 * The _cx calls mirror their real namesakes on interleaved complex arrays (float: 2 floats per pixel) and return PNP_E_STATE in real
 * mode.  EVERY complex array a caller hands to a _cx call on device pointers (pnp_dc_step_cx, pnp_prox_*_dual_cx, pnp_A_cx) must be
 * aligned to one complex value, 2 sizeof(real) = 8 bytes in float and 16 in double (PNP_E_ARG otherwise); pnp_prox_*_dual_cx without a
 * wavelet asks for 16 bytes in either precision (the kernel moves 16 bytes per access), with one x, z, w must not overlap.  pnp_A_cx: x [B][H][W] complex -> k [B][C][H][W], float only, like pnp_A.  pnp_synthesize_problem_mc
 * stays real-input: complex mode is for uploaded y. */
#define PNP_IMAGE_REAL    0
#define PNP_IMAGE_COMPLEX 1
int pnp_image_check(int mode, int wavelet, int levels, int f64);
int pnp_set_image(pnp_ctx* ctx, int mode);
int pnp_get_image(pnp_ctx* ctx, int* mode);
int pnp_set_state_cx(pnp_ctx* ctx, const float* z, const float* w, int on_device);
int pnp_set_state_cx_f64(pnp_ctx* ctx, const double* z, const double* w, int on_device);
int pnp_get_state_cx(pnp_ctx* ctx, float* z, float* w, int on_device);
int pnp_get_state_cx_f64(pnp_ctx* ctx, double* z, double* w, int on_device);
int pnp_download_x_cx(pnp_ctx* ctx, float* x, int on_device);
int pnp_download_x_cx_f64(pnp_ctx* ctx, double* x, int on_device);
int pnp_dc_step_cx(pnp_ctx* ctx, const float* z_dev, const float* w_dev, float* x_dev, double reo);
int pnp_dc_step_cx_f64(pnp_ctx* ctx, const double* z_dev, const double* w_dev, double* x_dev, double reo);
int pnp_prox_l1_dual_cx(pnp_ctx* ctx, const float* x_dev, float* z_dev, float* w_dev, double thr);
int pnp_prox_l1_dual_cx_f64(pnp_ctx* ctx, const double* x_dev, double* z_dev, double* w_dev, double thr);
int pnp_prox_cnc_dual_cx(pnp_ctx* ctx, const float* x_dev, float* z_dev, float* w_dev, double alpha, double lambda1, double reo, double b);
int pnp_prox_cnc_dual_cx_f64(pnp_ctx* ctx, const double* x_dev, double* z_dev, double* w_dev, double alpha, double lambda1, double reo,
                             double b);
int pnp_A_cx(pnp_ctx* ctx, const float* x_dev, float* k_dev);

/* ---- temporal sparsity (added after ABI 13, additive) ---------------------------------------------
 * Everything above treats the slices of a batch as strangers.  A dynamic series (cine, perfusion) is a batch whose frames are nearly
 * the same image; this regulariser penalises the coefficients of a unitary DFT along time of every pixel's series (k-t sparsity).  NOT in
 * the reference scripts.  Opt-in per context (pnp_set_temporal); without the setting -- the default -- nothing here is called and every
 * result is bit for bit what it was.
 * The batch is S series of T = `frames` consecutive slices: slice b = s T + t.  For every series and pixel, with u = x + w:
 *   U_k = T^(-1/2) sum_t u_t e^(-2 pi i k t / T);   the penalty is thr sum_k |U_k| over all T coefficients; with keep_dc (the default)
 *   k = 0 carries none, as the LL band of the wavelet prox never does.
 *   L1   Z_k = csoft(U_k, thr);   z+ = F^H Z,  z+_t = T^(-1/2) sum_k Z_k e^(+2 pi i k t / T);   w+ = u - z+.
 *   CNC  z^ = F z;  t^_k = c1 z^_k + c2 U_k + c3 cclip(z^_k, ib), component-wise, each component fma(c1, z^, fma(c2, U, c3 * clip));
 *        Z_k = csoft(t^_k, thr);  z+ and w+ as above.   thr, c1, c2, c3, ib are the scalars of the pixel-domain step.
 *   An unpenalised coefficient is Z_0 = U_0 -- NOT t^_0.
 * Real images: only k = 0 .. floor(T / 2) are formed and
 *   z+_t = T^(-1/2) [Z_0 + 2 sum_{0<k<T/2} Re(Z_k e^(+2 pi i k t / T)) + (T even) Z_(T/2) (-1)^t],
 *   so z stays exactly real; the real coefficients (0 and, T even, T / 2) take soft / clip on their real part.
 * Complex images (pnp_set_image): the full complex spectrum, csoft / cclip as defined above.
 * Arithmetic: direct sums, t ascending (analysis) and k ascending (synthesis); every product is one fma onto the running sum, which
 *   starts at 0 -- analysis: re = fma(u, c, re), im = fma(-u, s, im) for real u, and re = fma(u.re, c, re), re = fma(u.im, s, re),
 *   im = fma(u.im, c, im), im = fma(-u.re, s, im) for complex u; synthesis: re = fma(Z.re, c, re), re = fma(-Z.im, s, re) (and, complex
 *   images, im = fma(Z.re, s, im), im = fma(Z.im, c, im)); real images end with v = fma(2, re, Z_0) [+- Z_(T/2)].  T^(-1/2), rounded
 *   once to the context's precision, multiplies every finished sum once.  (c, s) = (cos, sin)(2 pi j / T), j = (k t) mod T, from a table
 *   of T entries computed in double on the host and rounded once.  2 <= T <= 64, any T (primes included).
 * One launch per prox, in both precisions, moving the pixel prox's bytes.  pnp_temporal_check: the argument rules without a context or
 * a device -- frames outside 2..64: PNP_E_ARG ("temporal: frames must be 2..64 (got %d)"); B < 1 or not a multiple of frames:
 * PNP_E_STATE ("temporal: the batch of %d slices is not a whole number of series of %d frames"). */
int pnp_temporal_check(int frames, int B);
/* frames = 0 clears the setting (keep_dc is not read); frames outside 2..64: PNP_E_ARG.  The setting excludes a wavelet and a spin table,
 * in either order of setting: pnp_set_temporal on a context with a wavelet set, and pnp_set_sparsity (other than PNP_WAVELET_NONE) or
 * pnp_set_spin on a context with frames set, return PNP_E_STATE.  It belongs to the context and survives uploads, pnp_set_coils and
 * pnp_set_image.  With frames set
 *   - pnp_admm_l1_run, pnp_admm_cnc_run and their _traced forms run, per iteration, the context's own data-consistency step (three
 *     launches, as with a wavelet) and ONE prox launch: four launches per iteration, which pnp_get_plan / pnp_kernels_per_iteration
 *     report.  The state stays in natural order, the slice-resident path is never taken (pnp_path_name never says "slice": it says
 *     "fused", or "generic" where the shape has no two-launch engine), a run cut into
 *     calls is bit-equal to one call.  On a coil context the x-step is followed by the same launch (5 + 5 cg_iters + 1), in real and in
 *     complex image mode.
 *   - pnp_prox_l1_dual, pnp_prox_cnc_dual and their _cx forms apply the temporal step to the uploaded problem's B slices (complex arrays
 *     aligned to one complex value).
 *   - a loop or prox call on a batch that is not a multiple of frames returns PNP_E_STATE with pnp_temporal_check's message. */
int pnp_set_temporal(pnp_ctx* ctx, int frames, int keep_dc);
/* frames = 0 without a setting (keep_dc then reads 1); either pointer may be null */
int pnp_get_temporal(pnp_ctx* ctx, int* frames, int* keep_dc);

/* ---- low-rank: the locally low-rank prox of a dynamic series (added after ABI 13, additive) ---------
 * The temporal DFT above fits periodic motion.  A contrast that changes without a period (uptake, relaxation, perfusion) is not sparse
 * under it; the regulariser for that case is LOCALLY LOW-RANK: the image is cut into block x block patches, a patch across the T frames
 * of its series is a P x T (Casorati) matrix, the penalty is its nuclear norm, the prox singular-value thresholding.  NOT in the
 * reference scripts.  Opt-in per context (pnp_set_lowrank, on a context with pnp_set_temporal's series length); without the setting
 * nothing here is called and every result is bit for bit what it was.  Real images only.
 * Convention.  The grid is anchored at a shift (sy, sx), 0 <= sy, sx < b = block: patch (i, j) holds the pixels in rows
 *   (sy + i b + r) mod H and columns (sx + j b + c) mod W, r, c < b.  Where b does not divide H or W the last patch row or column is
 *   partial (H mod b rows, W mod b columns); it does not wrap onto the first patch, so the patches partition the image exactly.
 *   X is the P x T matrix of one patch (P <= b^2 pixels, T frames), X = U diag(sigma) V^T, and for a function g on singular values
 *   S_g(X) = X V diag(g(sigma)) V^T.  With thr, c1, c2, c3, ib the scalars of the pixel-domain step and s = `scale`:
 *   thr <- s thr, ib <- s ib (each product formed in double from the rounded scalar and rounded once), c1, c2, c3 as they are -- which is
 *   lambda <- s lambda, b_cnc <- b_cnc / s, so the clipped term still stays below the threshold.
 *   L1    z+ = S_shrink(u), u = x + w, shrink(sigma) = max(1 - thr / sigma, 0): exactly 0 for sigma <= thr and for sigma = 0.
 *   CNC   t = c1 z + c2 u + c3 S_clip(z) [fma(c1, z, fma(c2, u, c3 * S_clip(z)))], clip(sigma) = min(1, ib / sigma), clip(0) = 1;
 *         z+ = S_shrink(t).
 *   both  w+ = u - z+.
 *   There is no keep_dc notion here (pnp_set_temporal's keep_dc is not read), and both maps are continuous in X.
 * Arithmetic.  G = X^T X (T x T; every entry one chain of fma over the pixels p = r pw + c ascending, pw the patch's width) is
 *   diagonalised by cyclic Jacobi in the round-robin ordering (an odd T padded by an index whose pairs are skipped), a sweep = T' - 1
 *   rounds of T' / 2 disjoint rotations, T' = T rounded up to even; before every sweep the off-diagonal sum of squares is tested against
 *   (eps ||G||_F)^2, eps = the precision's machine epsilon / 64, under a cap of 20 sweeps, so the result depends on the patch alone.  The
 *   vectors V and the rotations are held in double in both precisions (V stays orthogonal; G turns in the context's precision).
 *   Negative eigenvalues are clamped to 0, sigma = sqrt(lambda), M = V diag(g(sigma)) V^T (summed in double, rounded once), and
 *   S_g(X) = X M row by row.  CNC solves twice, for z and for t.  One launch per prox in both precisions; z+ and w+ are written once.
 * Limits: 2 <= frames <= 64 as for pnp_set_temporal; 2 <= block <= 32 and block <= min(H, W); a (frames, block, precision, L1 / CNC)
 *   whose patch does not fit the LDS one workgroup may declare (160 KiB) is refused.  Admitted at least: block <= 8 at every frames <= 64
 *   and block = 16 at every frames <= 16, in both precisions, for L1 and CNC.
 * pnp_lowrank_check: the argument rules without a context or a device, in this order -- frames outside 2..64: PNP_E_ARG with
 *   pnp_temporal_check's message; block outside 2..32: PNP_E_ARG ("lowrank: block must be 2..32 (got %d)"); block > H or W: PNP_E_ARG
 *   ("lowrank: block %d exceeds the image (%d x %d)"); LDS: PNP_E_ARG ("lowrank: a patch of %d x %d pixels over %d frames does not fit
 *   the LDS of a workgroup in float|double (L1|CNC)"); B < 1 or not a multiple of frames: PNP_E_STATE with pnp_temporal_check's message. */
int pnp_lowrank_check(int frames, int block, int H, int W, int B, int f64, int cnc);
/* block = 0 clears the setting (nothing else is read).  Needs pnp_set_temporal first (PNP_E_STATE otherwise) and is checked against that
 * series length for the L1 step (a CNC loop or prox call whose patch does not fit is refused where it is made, PNP_E_ARG).  scale > 0.
 * shifts: a table of n_shifts >= 1 pairs (sy, sx), each in [0, block) (PNP_E_ARG otherwise; at most 65536 pairs); it is copied.  The
 * table is walked one entry per prox step by a cursor: prox step p since the cursor was last set uses entry p mod n_shifts.  The cursor
 * is 0 after pnp_set_lowrank and after pnp_init_state; pnp_set_state keeps it, so a run cut into calls is bit-equal to one call.
 * With a block set
 *   - the prox step of pnp_admm_l1_run, pnp_admm_cnc_run, their _traced forms, the coil loop in real image mode and pnp_prox_l1_dual /
 *     pnp_prox_cnc_dual is the low-rank step instead of the temporal DFT step: the same four launches per iteration (5 + 5 cg_iters + 1
 *     with coils), which pnp_get_plan / pnp_kernels_per_iteration report;
 *   - complex image mode is refused in either order: pnp_set_lowrank on a context in complex mode, and pnp_set_image(PNP_IMAGE_COMPLEX)
 *     on a context with a block set, return PNP_E_STATE;
 *   - a wavelet and a spin table are refused as with pnp_set_temporal alone (its rules hold: the block needs the series length);
 *   - a batch that is not a whole number of series is PNP_E_STATE with pnp_temporal_check's message;
 *   - pnp_set_temporal(ctx, 0, ..) clears the block too; pnp_set_temporal with another length keeps it if the patch still fits
 *     (PNP_E_ARG and no change otherwise).
 * The step-wise real prox calls exist in float only, as before. */
int pnp_set_lowrank(pnp_ctx* ctx, int block, double scale, const int32_t* shifts, int n_shifts);
/* block = 0 without a setting (scale then reads 1, n_shifts and cursor 0); any pointer may be null */
int pnp_get_lowrank(pnp_ctx* ctx, int* block, double* scale, int* n_shifts, int* cursor);
/* cursor >= 0; PNP_E_STATE without a block */
int pnp_set_lowrank_cursor(pnp_ctx* ctx, int cursor);

/* ---- PnP denoisers on complex images (added after ABI 13, additive) -------------------------------
 * NOT in the reference scripts.  The denoisers are real networks on [n][1][H][W] float planes; these four calls are the glue between
 * them and the complex state of a context in complex image mode, so that the plug-and-play loops (solvers_pnp.py, image='complex')
 * run on device pointers with no other elementwise launch.  Float only; B, H, W are the uploaded problem's, n = B H W.  Two ways to
 * put a complex v through a real network D (mode):
 *   PNP_CX_DENOISE_MODULUS  one plane of B slices, m = |v| (two rounded squares, a sum, a square root);  d = D(m);
 *                           result (d / m) v where m != 0 -- one division, then two products; d may be negative and is not clamped --
 *                           and (d, 0) where m == 0 (both signs of zero, components whose squares underflow).  Phase-equivariant; the
 *                           network cost of the real loop.  `gain` is checked and not used.
 *   PNP_CX_DENOISE_PARTS    two planes, plane-major [2 B][1][H][W]: P[0:B] = 0.5 + g Re v, P[B:2B] = 0.5 + g Im v (the second plane
 *                           starts n floats behind the first);  Q = D(P) in one call on 2 B slices;  result ((Q[0:B] - 0.5) / g,
 *                           (Q[B:2B] - 0.5) / g).  g = gain, finite and > 0 (also as a float).  The network's noise level acts on the
 *                           planes, i.e. scaled by 1 / g on the image.  Not phase-equivariant.
 * pnp_cx_den_in        v = a (+ b when b is not null) -> planes.
 * pnp_cx_den_out       the network's planes q and the same a (+ b) -> complex z ('parts' does not read a, b; a must still be given).
 * pnp_cx_den_out_dual  the same join, then w <- w + x - z from the unclipped values, left to right, and x, z, w <- their projection onto
 *                      the unit disc (the complex counterpart of S6:305-308's clamp(0, 1)): x and w in place, z written.  a, b may be x, w.
 * pnp_cnc_combine_cx   S6:301 component-wise on interleaved complex arrays, pnp_cnc_combine's expression and order on 2 n floats.
 * Every operation is one correctly rounded float operation in the order given, no fma: results are bit-stable.
 * Rules, the first broken one is named:  ctx or a required pointer null: PNP_E_ARG;  real image mode, an fp64 context or no uploaded
 * problem: PNP_E_STATE;  mode not one of the two, gain not finite or <= 0: PNP_E_ARG;  a complex array or the plane base not 16-byte
 * aligned: PNP_E_ARG (the kernels move 16 bytes per access; the SECOND plane of 'parts' may lie anywhere: n need not be a multiple of 4).
 * The real pnp_cnc_combine / pnp_dual_clamp / pnp_add on a complex-mode context answer what they always did. */
#define PNP_CX_DENOISE_MODULUS 0
#define PNP_CX_DENOISE_PARTS   1
int pnp_cx_den_in(pnp_ctx* ctx, const float* a_dev, const float* b_dev, float* planes_dev, int mode, double gain);
int pnp_cx_den_out(pnp_ctx* ctx, const float* q_dev, const float* a_dev, const float* b_dev, float* z_dev, int mode, double gain);
int pnp_cx_den_out_dual(pnp_ctx* ctx, const float* q_dev, const float* a_dev, const float* b_dev, float* x_dev, float* z_dev, float* w_dev,
                        int mode, double gain);
int pnp_cnc_combine_cx(pnp_ctx* ctx, const float* z_dev, const float* x_dev, const float* w_dev, const float* s_dev, float* t_dev,
                       double alpha, double lambda1, double reo, double b);

/* ---- coil mixing ahead of the multi-coil solve: noise prewhitening and coil compression (added after ABI 13, additive) ----
 * NOT in the reference scripts.  Array data has 32 to 128 channels, the solve above takes at most 32 and costs time linear in C.  Both
 * standard remedies are ONE operation: a C_out x C_in complex matrix M applied per k-space point to the measurements and per pixel to
 * the maps.  The forward model is linear in the coil index, so with y' = M y and S' = M S it is again exactly y'_j = m . fft2(S'_j . x):
 * nothing after pnp_set_coils changes, which is handed S' (C_out <= 32 virtual coils) and y'.
 *   prewhitening   M_w = L^-1, L the lower Cholesky factor of the channels' noise covariance Psi (M_w Psi M_w^H = I)
 *   compression    M_c [C_out][C_in]: the conjugated eigenvectors of the C_out largest eigenvalues of the Gram matrix
 *                  R = sum_{p in calibration} mask(p) y(p) y(p)^H of the data (M_c M_c^H = I; eig_k / sum eig is virtual coil k's share of
 *                  the calibration energy)
 *   both           the Gram of the whitened data is M_w R M_w^H -- compress THAT, then M = M_c M_w.  The consumer multiplies these small
 *                  matrices itself (host, C x C) and mixes the data ONCE, C_in -> C_out: no whitened intermediate is ever written.
 * Calibration region (k-space un-shifted, DC at (0, 0)): rows 0 .. ceil(ncal / 2) - 1 and H - floor(ncal / 2) .. H - 1, columns by the same
 * rule with W.  Limits: 1 <= C_in <= 128, 1 <= C_out <= min(C_in, 32), Ks >= 1, 4 <= ncal <= 64 (and <= min(H, W)), H and W in
 * [128, 1024]; pnp_coilmix_check is that rule without a context or a device, anything else is PNP_E_ARG and pnp_last_error names the rule.
 * The device entry points are stateless like the conv layers': caller-owned device arrays, any HIP stream, no allocation, no
 * synchronisation, one launch.  Complex arrays are interleaved (re, im) in the precision of the entry point. */
int pnp_coilmix_check(int C_in, int C_out, int Ks, int ncal, int H, int W);
/* out[b][j][p] = sum_c m[set_id[b]][j][c] in[b][c][p]:  in [B][C_in][N], m [Ks][C_out][C_in] (device, the arrays' precision), set_id [B]
 * on the device or null (set 0; the entries are NOT range-checked: that would synchronise), out [B][C_out][N].  Any N >= 1: the call does
 * not know about H, W (measurements: N = H W; a bank of maps: B = Ks, set_id = 0 .. Ks - 1).  The coils are accumulated in the order
 * c = 0 .. C_in - 1 with fused multiply-adds, per point: a slice alone and the same slice in a batch are bit-equal.  in and out must not
 * overlap (PNP_E_ARG).  B <= 65535. */
int pnp_coil_mix(void* hip_stream, const float* in_dev, const float* m_dev, const int32_t* set_id_dev, float* out_dev, int B, int C_in,
                 int C_out, size_t N);
int pnp_coil_mix_f64(void* hip_stream, const double* in_dev, const double* m_dev, const int32_t* set_id_dev, double* out_dev, int B, int C_in,
                     int C_out, size_t N);
/* gram[b][i][j] = sum_{p in calibration} mask_b(p) y[b][i][p] conj(y[b][j][p]):  y [B][C][H][W], mask_bank [K][H][W] and mask_id [B] (or
 * null: mask 0; not range-checked) on the device, gram [B][C][C] complex DOUBLE.  Products and sums in double for both input precisions,
 * in a fixed order that depends on (ncal, H, W) alone; both triangles are stored, gram[b][j][i] is bit for bit the conjugate of
 * gram[b][i][j] and the diagonal's imaginary part is 0.  One matrix per SLICE: a consumer sums those of the slices that share a coil set
 * (on the host, in slice order, when the result must not depend on how the batch was cut). */
int pnp_coil_gram(void* hip_stream, const float* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, double* gram_dev, int B,
                  int C, int H, int W, int ncal);
int pnp_coil_gram_f64(void* hip_stream, const double* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, double* gram_dev, int B,
                      int C, int H, int W, int ncal);
/* Host, double, no device: m_out [C][C] = L^-1 of the Hermitian noise_cov [C][C] (its lower triangle is read), C <= 128.  A covariance
 * that is not positive definite, or not finite, is PNP_E_ARG. */
int pnp_coilmix_whiten(const double* noise_cov, int C, double* m_out);
/* Host, double, no device: cyclic Jacobi on the Hermitian gram [C][C] ((gram + gram^H) / 2 is what is decomposed).  eig_out [C]: all
 * eigenvalues, descending; m_out [C_out][C]: row j the conjugated eigenvector of eig_out[j], its phase fixed so that the eigenvector's
 * entry of largest modulus is real and positive (on a tie the first such entry). */
int pnp_coilmix_compress(const double* gram, int C, int C_out, double* m_out, double* eig_out);

/* ---- coil sensitivity maps from the calibration region of k-space (added after ABI 13, additive) ----
 * NOT in the reference scripts.  The solvers above need maps [C][H][W]; a scanner delivers k-space.  The estimator is the local
 * dominant-eigenvector method (Walsh's adaptive combination) in matrix-free form on low-resolution coil images: no calibration-matrix
 * SVD, no per-pixel eigendecomposition.  The solvers reconstruct a REAL non-negative image (x = |Re x^|), so the maps carry all of the
 * phase.  One slice, y [C][H][W] un-shifted (DC at (0, 0)), mask [H][W], ncal, radius r, power_iters n, thresh tau:
 *   1 window    calibration line i = 0 .. ncal - 1 of an axis of length n sits at line i (i < ceil(ncal / 2)) or n - ncal + i, its signed
 *               frequency is f = i resp. i - ncal, its weight w(f) = cos^2(pi f / (ncal + 1)).  K_c = w_H (x) w_W . y_c on the ncal x ncal
 *               region, 0 elsewhere.  EVERY point of the region must be sampled (mask != 0): otherwise PNP_E_ARG, and pnp_last_error names
 *               the first missing point (lowest offset).  No silent zero-filling.
 *   2 images    I_c = ifft2(K_c) with the context's own inverse transform (it carries 1 / (H W)).
 *   3 vectors   the patch of pixel p: the (2r + 1)^2 pixels around it, offsets in row-major order (dy, dx) = (-r, -r) .. (r, r), wrapped
 *               periodically on both axes.  v = I(p) / ||I(p)|| (e_0 when I(p) = 0); n times: g_q = sum_c conj(I_c(q)) v_c for every q of
 *               the patch in order (coils in order), u = sum_q I(q) g_q (patch points in order), lambda = ||u||, v = u / lambda (v stays
 *               when lambda = 0): power iteration on R(p) = sum_q I(q) I(q)^H, which is never formed.
 *   4 phase     g = sum_c conj(v_c) I_c(p); v <- v g / |g| (unchanged when g = 0).  Then v^H I(p) >= 0: a real non-negative image is
 *               consistent with the maps.
 *   5 support   lambda_max = the slice's largest lambda; S(p) = v(p) where lambda(p) >= tau^2 lambda_max, else exactly +0 in every coil.
 *               Inside the support sum_c |S_c|^2 = 1, the normalisation the x-step's 3 CG iterations assume; maps that vanish on a
 *               region are what the multi-coil solve already handles.
 * r = 0, n = 1 is S = I / ||I||, the classical low-resolution sum-of-squares maps; C = 1 is S = I / |I|.  Every sum is taken in an order
 * that depends on (C, r, n) alone (csrc/coilmaps_plan.h states each): a slice alone is bit-equal to the slice in a batch.
 * Limits, one message per rule (pnp_coilmaps_check: no context, no device): 1 <= C <= 32, ncal as for coil mixing, 0 <= radius <= 3,
 * 1 <= power_iters <= 16, 0 <= thresh < 1, H and W in [128, 1024].
 * pnp_coil_maps runs on `ctx` (any shape; the context's precision must be the entry point's) and on its stream, and touches neither the
 * uploaded problem nor the state: y [B][C][H][W], mask_bank [K][H][W] with mask_id [B] (or null: mask 0; not range-checked), maps_out
 * [B][C][H][W], lambda_out [B][H][W] or null -- all DEVICE arrays, interleaved complex.  The window kernel, the context's inverse
 * transform over the B C pseudo-slices in chunks of at most Bmax, the eigenvector kernel and the support kernels; the context keeps one
 * scratch array for min(B C, Bmax) pseudo-slices (at least C), allocated on first use -- a failure names the byte count.  maps_out must
 * not overlap y (PNP_E_ARG); B <= 65535.  The call synchronises the stream once, at its end, to read the missing-point check back. */
int pnp_coilmaps_check(int C, int ncal, int radius, int power_iters, double thresh, int H, int W);
int pnp_coil_maps(pnp_ctx* ctx, const float* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, float* maps_out_dev,
                  float* lambda_out_dev, int B, int C, int ncal, int radius, int power_iters, double thresh);
int pnp_coil_maps_f64(pnp_ctx* ctx, const double* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, double* maps_out_dev,
                      double* lambda_out_dev, int B, int C, int ncal, int radius, int power_iters, double thresh);
/* MEASUREMENT, not product (profiles/coilmaps_rate.py): enable != 0 brackets the three stages of every later pnp_coil_maps call on ctx --
 * window, inverse transform, eigenvectors with support -- by HIP events and synchronises after every pass; ms_out (or NULL) gets the three
 * times accumulated since the previous call of this function, which also resets them.  Results are bit for bit the same either way. */
int pnp_coil_maps_stage_times(pnp_ctx* ctx, int enable, float* ms_out);

/* ---- ESPIRiT coil sensitivity maps: calibration kernels wider than one pixel (added after ABI 13, additive) ----
 * NOT in the reference scripts.  The estimator above is local to a pixel of the low-resolution images; this one uses the correlations
 * between neighbouring k-space samples and gives an eigenvalue ~ 1 test for where the maps are valid.  It needs neither a per-pixel
 * eigendecomposition of stored matrices nor an image-sized transform of every calibration kernel.  One slice, y [C][H][W] un-shifted (DC
 * at (0, 0)), ncal, kernel side k, power_iters n, sigma, crop, thresh tau:
 *   1 block     the ncal x ncal calibration region (as above; EVERY point must be sampled, same PNP_E_ARG and message) re-ordered to
 *               ascending signed frequency on both axes (a roll by ncal / 2): K [C][ncal][ncal].  Not windowed.
 *   2 Gram      the (ncal - k + 1)^2 patch positions (i, j), not wrapped; row (i, j) of the calibration matrix A is K[c][i + a][j + b] at
 *               column (c k + a) k + b (c slowest), N = C k^2 columns.  Gram = A^H A, [N][N] complex DOUBLE for both input precisions, the
 *               positions summed in row-major order by one chain per entry, an order that depends on (ncal, k) alone; exactly Hermitian:
 *               the lower triangle is the conjugate of the upper to the bit, the diagonal's imaginary part is +0.
 *   3 space     (host, double, the cyclic Jacobi of pnp_coilmix_compress) eigenvalues e_j of Gram, s_j = sqrt(max(e_j, 0)); the signal
 *               space keeps the eigenvectors with s_j >= sigma s_max (their number is the rank); P = V V^H over them, symmetrised.
 *   4 kernels   (host, double) w_cc'(d) = (1 / k^2) sum_{a - a' = d} conj(P)[(c, a), (c', a')], d in [-(k - 1), k - 1]^2, stored
 *               [C][C][2k-1][2k-1] with entry (dy + k - 1, dx + k - 1); the upper triangle c <= c' from the sum, the lower as
 *               w_c'c(-d) = conj(w_cc'(d)).  Every k-space patch r of a signal in the calibration's span obeys conj(P) r = r; summed over
 *               the patch positions that is the k-space convolution with w.  Rounded once to the per-pixel stage's precision.
 *   5 operator  G_cc'(q) = sum_dy E_H(q_y, dy) [sum_dx w_cc'(dy, dx) E_W(q_x, dx)], E_n(q, d) = exp(+2 pi i ((q d) mod n) / n) formed in double
 *               from the reduced integer and rounded once; the inner chain over dx ascending, the outer over dy ascending, fused
 *               multiply-adds; the upper triangle is computed, the lower is its conjugate, the diagonal's imaginary part is +0.  The coil
 *               images S(q) x(q) are eigenvectors of G(q) with eigenvalue 1.
 *   6 vectors   v = I(q) / ||I(q)|| with I the windowed low-resolution images of the estimator above (e_0 where I = 0); n times: u = G v
 *               (c' ascending), lambda = ||u||, v = u / lambda (v stays where lambda = 0); then the phase rule above, v^H I(q) >= 0.
 *   7 support   S(q) = v(q) where lambda(q) >= crop AND ||I(q)|| >= tau max_q ||I(q)|| of the slice; elsewhere exactly +0 in every coil.
 * Every order is a function of (C, k, n, ncal) alone (csrc/espirit_plan.h states each): a slice alone is bit-equal to the slice in a batch.
 * Limits, one message per rule (pnp_espirit_check: no context, no device): 1 <= C <= 32, ncal as for coil mixing, 2 <= kernel <= 8,
 * kernel <= ncal, C kernel^2 <= 128 (the size of the host Jacobi: more channels go through coil compression first), 1 <= power_iters <= 16,
 * 0 < sigma < 1, 0 <= crop <= 1, 0 <= thresh < 1, H and W in [128, 1024].
 * pnp_calib_patch_gram: step 2 alone, no context; y [B][C][H][W], mask_bank [K][H][W] with mask_id [B] (or null: mask 0), gram [B][N][N]
 * complex double, all DEVICE arrays.  A calibration point the mask does not sample enters as +0 here; pnp_espirit_maps refuses such a mask.
 * pnp_espirit_kernels: steps 3 and 4, HOST arrays, double: gram [N][N] -> w_out [C][C][2k-1][2k-1] complex, *rank_out, sing_out [N] (the
 * s_j, descending).
 * pnp_espirit_eigmaps: steps 5 and 6 alone on the caller's DEVICE arrays, on ctx's stream: lowres_images [B][C][H][W], w [B][C][C][2k-1][2k-1]
 * in the context's precision -> maps_out [B][C][H][W] (the unit vectors, NO support applied), lambda_out [B][H][W].  Synchronises at its end.
 * pnp_espirit_maps: the whole pipeline on ctx and its stream, the arrays as for pnp_coil_maps (lambda_out or null).  Per pass of as many
 * slices as fit min(B C, Bmax) pseudo-slices: window and inverse transform, patch Gram, one read-back, the host stage for the slices of the
 * pass on at most 16 threads (never the machine's CPU count), the per-pixel and support kernels.  The context keeps one scratch array,
 * allocated on first use -- a failure names the byte count; the uploaded problem and the state are not touched.  maps_out must not overlap
 * y (PNP_E_ARG); B <= 65535.  pnp_espirit_ranks: the rank of every slice of the most recent pnp_espirit_maps on ctx (rank_out [B], host). */
int pnp_espirit_check(int C, int ncal, int kernel, int power_iters, double sigma, double crop, double thresh, int H, int W);
int pnp_calib_patch_gram(void* hip_stream, const float* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, double* gram_dev, int B,
                         int C, int H, int W, int ncal, int kernel);
int pnp_calib_patch_gram_f64(void* hip_stream, const double* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, double* gram_dev,
                             int B, int C, int H, int W, int ncal, int kernel);
int pnp_espirit_kernels(const double* gram, int C, int kernel, double sigma, double* w_out, int* rank_out, double* sing_out);
int pnp_espirit_eigmaps(pnp_ctx* ctx, const float* lowres_images_dev, const float* w_dev, float* maps_out_dev, float* lambda_out_dev, int B, int C,
                        int kernel, int power_iters);
int pnp_espirit_eigmaps_f64(pnp_ctx* ctx, const double* lowres_images_dev, const double* w_dev, double* maps_out_dev, double* lambda_out_dev, int B,
                            int C, int kernel, int power_iters);
int pnp_espirit_maps(pnp_ctx* ctx, const float* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, float* maps_out_dev,
                     float* lambda_out_dev, int B, int C, int ncal, int kernel, int power_iters, double sigma, double crop, double thresh);
int pnp_espirit_maps_f64(pnp_ctx* ctx, const double* y_dev, const uint8_t* mask_bank_dev, const int32_t* mask_id_dev, double* maps_out_dev,
                         double* lambda_out_dev, int B, int C, int ncal, int kernel, int power_iters, double sigma, double crop, double thresh);
int pnp_espirit_ranks(pnp_ctx* ctx, int32_t* rank_out, int B);
/* MEASUREMENT, not product (profiles/espirit_rate.py): enable != 0 times three stages of every later pnp_espirit_maps pass on ctx -- patch
 * Gram with its read-back (HIP events), the host stage (host clock), per-pixel and support kernels (HIP events); ms_out (or NULL) gets the
 * three times accumulated since the previous call of this function, which also resets them.  Results are the same bits either way. */
int pnp_espirit_stage_times(pnp_ctx* ctx, int enable, float* ms_out);

/* ---- optional HIP backend of the denoisers' plain conv stacks ------------------------------
 * The north star keeps the CNN forward pass in PyTorch-ROCm; these two entry points are the opt-in `Denoiser(backend='hip')`
 * for the 64 -> 64 channel conv3x3 (+ bias, + ReLU) body layers of FFDNet / DnCNN / FDnCNN (models/network_ffdnet.py:58-73,
 * models/network_dncnn.py:36-67, models/basicblock.py:63-100 mode 'CR'), where configs 3-5 spend 99.8 % of their time:
 * an implicit GEMM on the fp32 matrix cores (exact f32 fma chains).  No ctx: caller-owned device tensors, any HIP stream.
 *   y = relu?( conv3x3(x, w) + bias + skip ),  stride 1, dilation d = 1..4, zero padding d (torch.nn.Conv2d(64, 64, 3, 1, d, dilation=d):
 *   d = 1 the plain stacks and DRUNet, d = 2..4 IRCNN's dilated layers, models/network_dncnn.py:87-101)
 *   x, y, skip: [n][H][W][64] float32 (NHWC); w_packed: 36 864 floats written by pnp_conv3x3_c64_pack (the kernel streams
 *   its weights from L2 in matrix-core fragment order); bias [64] or NULL; skip NULL or a tensor of y's shape added before the
 *   ReLU; y must alias neither x nor skip.  New in ABI 8.
 * Size rule of EVERY conv-layer entry point of this header (float32, f16x3 and half alike; csrc/conv_plan.h): one image with 16 more rows
 * must stay below 2 GiB as a float32 tensor, (H + 16) W C 4 <= 2^31 - 1 (C = 64 for the first / last layers; the 2 x 2 layers: input and
 * result both) -- the kernels let the byte offsets of halo and overhang rows fall out of the buffer's range, and those must not wrap
 * around 2^32.  A larger image is PNP_E_ARG with a message that names the 16 rows.  (The float32 and f16x3 entry points used to bound
 * H W C 4 only -- 2896 x 2896 at C = 64, now 2888 x 2888 -- and pnp_conv3x3_c64_nhwc, pnp_conv3x3_c64_nhwc_f16x3, pnp_conv3x3_head_nhwc,
 * pnp_conv3x3_tail_nchw and pnp_conv3x3_tail_nchw_f16x3 reported an oversize image as PNP_E_HIP from the launch.) */
int pnp_conv3x3_c64_nhwc(void* hip_stream, const float* x_dev, const float* w_packed_dev, const float* bias_dev,
                         const float* skip_dev, float* y_dev, int n, int H, int W, int relu, int dilation);
/* w_oihw_dev: a torch.nn.Conv2d(64, 64, 3) weight, [64 out][64 in][3][3] contiguous -> w_packed_dev (36 864 floats).  Once
 * per model (again after the weights change). */
int pnp_conv3x3_c64_pack(void* hip_stream, const float* w_oihw_dev, float* w_packed_dev);
/* The same layer in SPLIT-HALF arithmetic on the f16 matrix cores ("f16x3"; csrc/kernels_conv_f16x3.hip): every float32 operand
 * is split into two halves, x = hi + lo / 2048, and a product becomes three v_mfma_f32_16x16x32_f16 (hi*hi, hi*lo, lo*hi: exact
 * products, float32 accumulation) -- float32-level results (operands carried to 2^-22, tests/test_gpu_conv.py measures the
 * distance from float64 beside the float32 kernel's) at several times the float32 matrix rate.  Same arguments and semantics as
 * pnp_conv3x3_c64_nhwc; w_packed from pnp_conv3x3_c64_pack_f16x3 (36 864 floats of storage, a different order: the two packings
 * are not interchangeable).  Operands must lie within the half range (|x|, |w| <= 65504): beyond it the result is inf / NaN.
 * New in ABI 9. */
int pnp_conv3x3_c64_nhwc_f16x3(void* hip_stream, const float* x_dev, const float* w_packed_dev, const float* bias_dev,
                               const float* skip_dev, float* y_dev, int n, int H, int W, int relu, int dilation);
int pnp_conv3x3_c64_pack_f16x3(void* hip_stream, const float* w_oihw_dev, float* w_packed_dev);
/* The f16x3 layer for C -> C channels, C a multiple of 64 up to 1024 (DRUNet's residual blocks at 128 / 256 / 512 channels,
 * models/network_unet.py:36-58 with models/basicblock.py:213-225): dilation 1, zero padding 1; x, y, skip [n][H][W][C] float32
 * (NHWC); w_packed: 9 C C floats of storage written by pnp_conv3x3_pack_f16x3 from a torch Conv2d(C, C, 3) weight; bias [C] or
 * NULL.  A workgroup computes 8 x 16 pixels x 64 output channels, its K loop runs over the C / 64 chunks of input channels; one
 * image with 16 more rows must stay below 2 GiB ((H + 16) W C floats: the size rule above).  C = 64 is the layer above (same packing).
 * New in ABI 9. */
int pnp_conv3x3_nhwc_f16x3(void* hip_stream, const float* x_dev, const float* w_packed_dev, const float* bias_dev,
                           const float* skip_dev, float* y_dev, int n, int C, int H, int W, int relu);
int pnp_conv3x3_pack_f16x3(void* hip_stream, const float* w_oihw_dev, float* w_packed_dev, int C);
/* The f16x3 layer with its tensors in the SPLIT ACTIVATION FORMAT, for chains of such layers (a plain stack's body, DRUNet's residual
 * blocks): a tensor keeps its shape and bytes -- [n][H][W][C], 256 bytes per pixel and block of 64 channels -- but a block holds
 * [64 hi halves][64 lo halves] of its 64 values, value = hi + lo / 2048 (the float32 result rounded to 2^-22 relative: what the
 * consuming layer's operands carry anyway).  The PRODUCING layer splits each output once in its epilogue; a consuming layer copies
 * 16-byte runs of halves into its operand tile instead of splitting every value of every tile again for every block of output
 * channels.  fmt: a mask saying which of x, skip, y are split (0 = all float32 = pnp_conv3x3_nhwc_f16x3); dilation 1..4 at C = 64, 1
 * otherwise.  New in ABI 10. */
#define PNP_FMT_X_SPLIT    1
#define PNP_FMT_SKIP_SPLIT 2
#define PNP_FMT_Y_SPLIT    4
int pnp_conv3x3_nhwc_f16x3_fmt(void* hip_stream, const float* x_dev, const float* w_packed_dev, const float* bias_dev,
                               const float* skip_dev, float* y_dev, int n, int C, int H, int W, int relu, int dilation, int fmt);
/* Which kernel the three f16x3 conv3x3 entry points above launch at dilation 1 (the results are bit-equal; tests and A/B measurements pin
 * one): -1 = by size (default: the WIDE kernel -- 16 x 16 pixel tiles, 64 x 64 wave tiles, compute + helper waves, kernels_conv_f16x3_wide.hip --
 * once every compute unit has an item (16 x 16 pixels x 64 output channels) of its own, the narrow one -- 8 x 16 tiles, two workgroups per unit -- below that), 0 = narrow always,
 * 1 = wide always.  Process-wide; returns the previous setting.  The environment variable PNP_CONV_WIDE sets the initial value.  New in ABI 11. */
int pnp_conv3x3_f16x3_set_variant(int variant);
/* pnp_conv3x3_tail_nchw (below) in the f16x3 arithmetic: x [n][H][W][64] (NHWC), w a torch Conv2d(64, cout, 3) weight (split inside the
 * kernel), 1 <= cout <= 4 -> y [n][cout][H][W] (NCHW), + bias.  On the vector units this layer costs as much as a 64 -> 64 layer of the
 * f16x3 kernel; as a 16-column matrix product it is bound by reading its input.  Same operand range and size rule as above.  New in ABI 9. */
int pnp_conv3x3_tail_nchw_f16x3(void* hip_stream, const float* x_nhwc_dev, const float* w_oihw_dev, const float* bias_dev,
                                float* y_nchw_dev, int n, int cout, int H, int W);
/* The same with a second input ADDED to x while it is staged (the U-Net's last skip sum, models/network_unet.py:134-135: the sum never
 * goes to memory).  New in ABI 10. */
int pnp_conv3x3_tail_add_nchw_f16x3(void* hip_stream, const float* x_nhwc_dev, const float* x2_nhwc_dev, const float* w_oihw_dev,
                                    const float* bias_dev, float* y_nchw_dev, int n, int cout, int H, int W);
/* DRUNet's scale changes in the f16x3 arithmetic (csrc/kernels_pix2x2_f16x3.hip), bias-free as in models/network_unet.py:95-107 with
 * models/basicblock.py:415-421, 439-445 -- with them `Denoiser(backend='hip_f16x3')` runs DRUNet without a MIOpen call:
 *   pnp_conv2x2s2_nhwc_f16x3    torch.nn.Conv2d(C, 2C, 2, 2, 0):           x [n][H][W][C] -> y [n][H/2][W/2][2C]  (H, W even; C = 64 k)
 *   pnp_convT2x2s2_nhwc_f16x3   torch.nn.ConvTranspose2d(C, C/2, 2, 2, 0): x [n][H][W][C] -> y [n][2H][2W][C/2]   (C = 128 k)
 * x2_dev: NULL, or a tensor of x's shape that is added to x while it is staged (the skip sums `m_up(x + x_skip)`,
 * models/network_unet.py:131-133).  w_packed from pnp_conv2x2_pack_f16x3 (transposed = 0: a Conv2d weight [2C][C][2][2], 8 C C floats
 * of storage; 1: a ConvTranspose2d weight [C][C/2][2][2], 2 C C floats).  Same operand range as the layers above.  New in ABI 10. */
int pnp_conv2x2s2_nhwc_f16x3(void* hip_stream, const float* x_dev, const float* x2_dev, const float* w_packed_dev, float* y_dev,
                             int n, int C, int H, int W);
int pnp_convT2x2s2_nhwc_f16x3(void* hip_stream, const float* x_dev, const float* x2_dev, const float* w_packed_dev, float* y_dev,
                              int n, int C, int H, int W);
int pnp_conv2x2_pack_f16x3(void* hip_stream, const float* w_dev, float* w_packed_dev, int C, int transposed);
/* First and last layer of the plain stacks (models/network_dncnn.py:52-62, models/network_ffdnet.py:50-56), direct convolutions:
 *   head: x [n][cin][H][W] (NCHW, 1 <= cin <= 8), w a torch Conv2d(cin, 64, 3) weight [64][cin][3][3] -> y [n][H][W][64] (NHWC), + bias, ReLU
 *   tail: x [n][H][W][64] (NHWC), w a torch Conv2d(64, cout, 3) weight [cout][64][3][3], 1 <= cout <= 4 -> y [n][cout][H][W] (NCHW), + bias
 * With them `Denoiser(backend='hip')` runs DnCNN / FDnCNN / FFDNet without a MIOpen call.  The size rule above applies with C = 64.
 * New in ABI 8. */
int pnp_conv3x3_head_nhwc(void* hip_stream, const float* x_nchw_dev, const float* w_oihw_dev, const float* bias_dev,
                          float* y_nhwc_dev, int n, int cin, int H, int W, int relu);
int pnp_conv3x3_tail_nchw(void* hip_stream, const float* x_nhwc_dev, const float* w_oihw_dev, const float* bias_dev,
                          float* y_nchw_dev, int n, int cout, int H, int W);
/* FFDNet's input and output stages folded into its first and last layer (models/network_ffdnet.py:58-73): no pad / pixel-unshuffle / concatenation
 * / pixel-shuffle / crop launches and no intermediate tensors around the stack.
 *   pnp_ffdnet_head_nhwc   x [n][1][h][w] (full resolution, any h, w >= 1: odd sizes are replicate-padded as the reference does), sigma_dev [n] or [1]
 *                          (sigma_per_image = 1 / 0): the layer's five input channels are the four pixel-unshuffled quarters of x and the noise
 *                          level; w a torch Conv2d(5, 64, 3) weight -> y [n][ceil(h/2)][ceil(w/2)][64] (NHWC), + bias, ReLU
 *   pnp_ffdnet_tail_f16x3  x [n][ceil(h/2)][ceil(w/2)][64] (NHWC), w a torch Conv2d(64, 4, 3) weight -> y [n][1][h][w]: the four output channels
 *                          written pixel-shuffled and cropped, in the f16x3 arithmetic of pnp_conv3x3_tail_nchw_f16x3.   New in ABI 10. */
int pnp_ffdnet_head_nhwc(void* hip_stream, const float* x_dev, const float* sigma_dev, int sigma_per_image, const float* w_oihw_dev,
                         const float* bias_dev, float* y_nhwc_dev, int n, int h, int w, int relu);
int pnp_ffdnet_tail_f16x3(void* hip_stream, const float* x_nhwc_dev, const float* w_oihw_dev, const float* bias_dev, float* y_dev, int n, int h, int w);
/* ---- the denoisers' layers in HALF precision: `Denoiser(backend='hip_f16')`.  Added after ABI 13, additive (PNP_ABI_VERSION stays) ----
 * csrc/kernels_conv_f16.hip, csrc/kernels_pix2x2_f16.hip.  Activations between layers are IEEE halves, NHWC, 128 bytes per pixel and
 * block of 64 channels (passed as void*); weights are rounded to half (round to nearest even) once, at pack time.  A layer computes
 *     y = round_half( relu?( sum_fp32( x_half * w_half ) + bias_fp32 + float(skip_half) ) )
 * on v_mfma_f32_16x16x32_f16: exact products, float32 accumulation, ONE rounding on store.  A value beyond +-65504 is stored as inf,
 * NaN propagates.  A network's first layer keeps the float32 direct arithmetic on the float32 network input and stores halves; its
 * last layer stores float32.  A throughput mode: it does NOT meet the 1e-5 parity bar of the float32 backends.
 *
 * pnp_conv3x3_nhwc_f16: torch.nn.Conv2d(C, C, 3, 1, d, dilation=d), C a multiple of 64 up to 1024; dilation 1..4 at C = 64, 1 otherwise.
 * x, skip, y [n][H][W][C]; w_packed: 9 C C halves from pnp_conv3x3_pack_f16; bias [C] float32 or NULL; skip NULL or added before the
 * ReLU; y must alias neither x nor skip.  fmt says which tensors are float32 INSTEAD of half (0 = all half): a float32 x is rounded
 * to half while it is staged (same bits as a pre-rounded x), a float32 y is the accumulator result without the final rounding.  One
 * image with 16 more rows must stay below 2 GiB as a float32 tensor ((H + 16) W C floats), whatever its format: the kernels let the
 * byte offsets of halo and overhang rows fall out of the buffer's range, and those must not wrap around 2^32. */
#define PNP_F16_X_F32    1
#define PNP_F16_SKIP_F32 2
#define PNP_F16_Y_F32    4
int pnp_conv3x3_nhwc_f16(void* hip_stream, const void* x_dev, const void* w_packed_dev, const float* bias_dev, const void* skip_dev,
                         void* y_dev, int n, int C, int H, int W, int relu, int dilation, int fmt);
/* w_oihw_dev: a torch Conv2d(C, C, 3) weight, float32 [C][C][3][3] contiguous -> 9 C C halves in the kernel's fragment order. */
int pnp_conv3x3_pack_f16(void* hip_stream, const float* w_oihw_dev, void* w_packed_dev, int C);
/* First layers: pnp_conv3x3_head_nhwc / pnp_ffdnet_head_nhwc with the same float32 arithmetic, y [n][H][W][64] stored as halves. */
int pnp_conv3x3_head_nhwc_f16(void* hip_stream, const float* x_nchw_dev, const float* w_oihw_dev, const float* bias_dev,
                              void* y_nhwc_dev, int n, int cin, int H, int W, int relu);
int pnp_ffdnet_head_nhwc_f16(void* hip_stream, const float* x_dev, const float* sigma_dev, int sigma_per_image, const float* w_oihw_dev,
                             const float* bias_dev, void* y_nhwc_dev, int n, int h, int w, int relu);
/* Last layers: x [n][H][W][64] halves, w a float32 torch Conv2d(64, cout, 3) weight (rounded to half inside the kernel), 1 <= cout <= 4
 * -> y float32.  pnp_conv3x3_tail_nchw_f16: y [n][cout][H][W]; x2_dev NULL, or a half tensor of x's shape added to x in float32 while
 * it is staged, the sum rounded to half once (the U-Net's last skip sum).  pnp_ffdnet_tail_f16: x at ceil(h/2) x ceil(w/2), the four
 * output channels written pixel-shuffled and cropped into y [n][1][h][w]. */
int pnp_conv3x3_tail_nchw_f16(void* hip_stream, const void* x_nhwc_dev, const void* x2_nhwc_dev, const float* w_oihw_dev,
                              const float* bias_dev, float* y_nchw_dev, int n, int cout, int H, int W);
int pnp_ffdnet_tail_f16(void* hip_stream, const void* x_nhwc_dev, const float* w_oihw_dev, const float* bias_dev, float* y_dev, int n, int h, int w);
/* DRUNet's scale changes on halves (shapes and x2 as pnp_conv2x2s2_nhwc_f16x3 / pnp_convT2x2s2_nhwc_f16x3; x, x2, y halves; the sum
 * x + x2 is formed in float32 and rounded to half once, as the operand; y_f32 != 0: y is float32, the accumulator result without the
 * final rounding -- what the one-layer tests compare with float64).  w_packed from pnp_conv2x2_pack_f16: 8 C C halves
 * (transposed = 0, a Conv2d weight [2C][C][2][2]) or 2 C C halves (1, a ConvTranspose2d weight [C][C/2][2][2]). */
int pnp_conv2x2s2_nhwc_f16(void* hip_stream, const void* x_dev, const void* x2_dev, const void* w_packed_dev, void* y_dev,
                           int n, int C, int H, int W, int y_f32);
int pnp_convT2x2s2_nhwc_f16(void* hip_stream, const void* x_dev, const void* x2_dev, const void* w_packed_dev, void* y_dev,
                            int n, int C, int H, int W, int y_f32);
int pnp_conv2x2_pack_f16(void* hip_stream, const float* w_dev, void* w_packed_dev, int C, int transposed);
/* [n][64][H][W] <-> [n][H][W][64] (to_nhwc = 1 / 0): hand-over between PyTorch layers (NCHW) and the kernels above. */
int pnp_relayout_c64(void* hip_stream, const float* in_dev, float* out_dev, int n, int H, int W, int to_nhwc);

/* ---- timing on the ctx stream (HIP events) ------------------------------------------------ */
int pnp_timer_start(pnp_ctx* ctx);
int pnp_timer_stop(pnp_ctx* ctx, float* elapsed_ms);    /* records, synchronises, returns ms */

/* ---- introspection ------------------------------------------------------------------------ */
/* launches per batched ADMM iteration on the current path and schedule (0 = the iterations of a call are a
 * loop inside ONE launch), and which kernel family the loops take for the uploaded problem:
 *   "slice"   256x256 float, batches of >= 64 slices: one workgroup keeps a slice in registers for the whole run
 *   "fused"   two launches per iteration (256x256 float / double, 512x512 float)
 *   "generic" three launches per iteration (any H, W; pnp_set_fast_path(ctx, 0)) */
int         pnp_kernels_per_iteration(pnp_ctx* ctx);
const char* pnp_path_name(pnp_ctx* ctx);
/* Which kernels a context runs on, fixed at creation: "anysize" (H, W not both in {256, 512}: the any-size FFT kernels,
 * generic iteration) or, for the fixed-size kernels, pnp_path_name's answer. */
const char* pnp_ctx_path(pnp_ctx* ctx);
/* The transform plan of one axis (0 = rows, length W; 1 = columns, length H) as text, e.g. "stockham 320 = 4*4*4*5",
 * "bluestein 218 -> 512 = 4*4*4*4*2", or "fixed 256" for the fixed-size kernels.  buf gets at most len bytes, NUL included. */
int         pnp_fft_plan(pnp_ctx* ctx, int axis, char* buf, int len);

#ifdef __cplusplus
}
#endif
#endif /* PNP_MRI_H */
