"""GPU tests of the two parts of csrc/kernels_generic.hip that the public ABI reaches and nothing else compared with a reference.

A. Rectangular fixed shapes, 256 x 512 and 512 x 256: contexts that are NOT any-size and have no fast engine, so every call runs the
   fixed-size row kernels of one length with the column kernels of the other, and the column kernels take W as a run-time argument (tile
   count, slice stride, mask-bank stride, in k_cols16 the dword pitch of the mask rows).  B = 3 slices in a context of Bmax = 4, a bank
   of the three synthetic masks used in the order mask_id = [2, 0, 1]: a wrong bank or slice stride reads another mask.  Every test
   first asserts the path it runs on ('generic', plans 'fixed W' / 'fixed H', not 'anysize').  Operators, one x-step, synthesis and
   initial state (float and double), whole loops (float: 1e-5 at 10 iterations, double: 1e-8 at 100 CNC / 20 L1 iterations) against
   oracle/admm_oracle.py, the transposed problem on the transposed context, metrics and SSIM, the trace, the solver entry point.  Every bar
   is the bar the same operation has at a square shape (tests/test_gpu_parity.py, tests/test_gpu_anysize.py, tests/test_gpu_trace.py).

B. The float32 pointwise kernels on caller pointers (k_prox<L1>, k_prox<CNC>, k_combine, k_add, k_dual_clamp): element counts of
   every remainder mod 4 (the scalar tail), counts above 2048 * 256 * 4 (a second grid stride, with and without a tail), the last
   vector and the tail compared element by element, every device array a view inside a larger allocation with 64 sentinel floats on
   either side.  References: the float64 NumPy expressions (O.l1_step, O.cnc_step, the S6:301 line) with the absolute bars of
   test_prox_kernels (2e-7, 5e-7) and test_glue_kernels (2e-7); pnp_add and pnp_dual_clamp equal the float32 torch expressions.

C. Caller pointers that are float-aligned but not 16-byte aligned: every argument in turn one float past a 16-byte boundary; the result
   equals the aligned call's bit for bit, within the same bars and sentinels."""
import functools
import time

import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(256, 512), (512, 256)]
KINDS = ('random', 'radial', 'cartesian')
B, BMAX = 3, 4
MID = np.array([2, 0, 1], np.int32)
CNC = (0.45, 0.5, 0.05, 64)                                        # S4:176
L1 = (0.1, 0.015)                                                  # S1:171
NAMES = ('r_pri', 'r_dual', 'x_norm', 'z_norm', 'w_norm')


@pytest.fixture(scope='module')
def env():
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib, utils_pnp
    assert _lib.device_count() >= 1 and torch.cuda.is_available(), 'no HIP device visible: GPU tests must not pass silently'
    return dict(torch=torch, P=P, U=utils_pnp)


# ------------------------------------------------------------------------------------------------------------------------------------
# A. rectangular fixed shapes
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(H, W):
    """-> masks [3,H,W] uint8, imgs [B,H,W] float32, ys [B,H,W] complex128 (slice b measured with mask MID[b]), noise [B,H,W] complex128,
    gt [B,H,W] uint8.  The masks differ from each other, and the random and the Cartesian one from their own point reflection k -> -k
    (the radial one, lines through DC, is point-symmetric by construction), so a wrong mask or a mirrored index shows."""
    masks = np.stack([O.synthetic_mask(k, H, W) for k in KINDS]).astype(np.uint8)
    for i, m in enumerate(masks):
        assert KINDS[i] == 'radial' or not np.array_equal(m, np.roll(m[::-1, ::-1], (1, 1), (0, 1))), KINDS[i]
        assert all(not np.array_equal(m, o) for o in masks[i + 1:])
    imgs, ys = zip(*(O.synthetic_problem(b, masks[MID[b]], H, W) for b in range(B)))
    noise = np.stack([O.kspace_noise(b, H, W) for b in range(B)])
    imgs = np.stack(imgs)
    gt = np.round(imgs.astype(np.float64) * 255).astype(np.uint8)
    return masks, imgs, np.stack(ys), noise, gt


def _path(eng):
    return eng.ctx_path, eng.path_name, eng.fft_plan(0), eng.fft_plan(1)


def _assert_fixed_generic(path, H, W):
    """the code under test: fixed-size kernels of two different lengths, no fast engine, no any-size plan"""
    ctx_path, path_name, plan0, plan1 = path
    assert ctx_path != 'anysize' and path_name == 'generic' and plan0 == 'fixed %d' % W and plan1 == 'fixed %d' % H, path


@pytest.mark.parametrize('H, W', SHAPES)
def test_operators_float_against_oracle(env, H, W):
    """A, A^H, Df per slice (the bars of test_operators_A_AH_Df: 2e-6, 2e-6, 5e-6) and <A x, k> = N <x, A^H k> with N = H W."""
    torch, P, U = env['torch'], env['P'], env['U']
    masks, imgs, ys, _, _ = _problem(H, W)
    with P.Engine(H, W, Bmax=BMAX) as eng:
        eng.upload(ys, masks, MID)
        _assert_fixed_generic(_path(eng), H, W)
        x = torch.from_numpy(imgs).cuda()
        k = U.A(eng, x).cpu().numpy()
        kk = torch.from_numpy(ys.astype(np.complex64)).cuda()
        ah = U.AH(eng, kk).cpu().numpy()
        df = U.Df(eng, x).cpu().numpy()
    assert k.shape == ah.shape == df.shape == (B, H, W)
    for b in range(B):
        m = masks[MID[b]]
        # the device holds y as complex64: compare against the oracle on the same y
        y64 = ys[b].astype(np.complex64).astype(np.complex128)
        e = (rel_l2(k[b], O.A(imgs[b].astype(np.float64), m)), rel_l2(ah[b], O.AH(y64, m)),
             rel_l2(df[b], O.Df(imgs[b].astype(np.float64), m.astype(np.float64), y64)))
        print('%dx%d slice %d (mask %d): A %.2e (<= 2e-6), AH %.2e (<= 2e-6), Df %.2e (<= 5e-6)' % (H, W, b, MID[b], *e))
        assert e[0] <= 2e-6 and e[1] <= 2e-6 and e[2] <= 5e-6, (b, e)
        lhs = np.vdot(k[b], ys[b])
        rhs = H * W * np.vdot(imgs[b].astype(np.complex128), ah[b])
        assert abs(lhs - rhs) <= 1e-4 * abs(lhs), (b, lhs, rhs)


@pytest.mark.parametrize('H, W', SHAPES)
def test_dc_step_teacher_forced(env, H, W):
    """One x-update from given (z, w): IN_REAL_DIFF rows, MID_BLEND columns, EPI_ABS_REAL rows; bar and inputs of the square test."""
    torch, P, U = env['torch'], env['P'], env['U']
    masks, _, ys, _, _ = _problem(H, W)
    rng = np.random.default_rng(5)
    z = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    w = rng.uniform(-0.1, 0.1, (B, H, W)).astype(np.float32)
    with P.Engine(H, W, Bmax=BMAX) as eng:
        eng.upload(ys, masks, MID)
        _assert_fixed_generic(_path(eng), H, W)
        x = U.dc_solve(eng, torch.from_numpy(z).cuda(), torch.from_numpy(w).cuda(), 0.05).cpu().numpy()
    for b in range(B):
        ref = O.dc_step(z[b].astype(np.float64), w[b].astype(np.float64), ys[b].astype(np.complex64).astype(np.complex128),
                        masks[MID[b]], 0.05)
        e = rel_l2(x[b], ref)
        print('%dx%d slice %d: dc_step %.2e (<= 5e-7)' % (H, W, b, e))
        assert e <= 5e-7, (b, e)


@pytest.mark.parametrize('H, W', SHAPES)
def test_dc_step_double_through_a_wavelet_iteration(env, H, W):
    """EPI_ABS_REAL rows in double (k_rows<W, IN_COMPLEX, inverse, EPI_ABS_REAL, double>): there is no double pnp_dc_step, and the plain
    double loops take x from the prox epilogues, so the one way in is a loop with a wavelet set, whose iteration is the x-step on the
    context's kernels and then the prox.  x of the first iteration is dc(z0, 0) whatever the prox does to z and w.  Per slice against
    O.dc_step on the y the device holds; bar 1e-12, the double bar of this file for one application of an operator (synthesis, z0)."""
    P = env['P']
    masks, _, ys, _, _ = _problem(H, W)
    with P.Engine(H, W, Bmax=BMAX, precision='f64') as eng:
        eng.set_sparsity('haar', 1)
        eng.upload(ys, masks, MID)
        _assert_fixed_generic(_path(eng), H, W)
        eng.init_state()
        z0, w0 = eng.get_state()
        eng.admm_l1(1, 0.1, 0.05)
        x = eng.x()
    assert x.dtype == np.float64 and not w0.any()
    for b in range(B):
        ref = O.dc_step(z0[b], w0[b], ys[b], masks[MID[b]], 0.05)
        e = rel_l2(x[b], ref)
        print('%dx%d double slice %d: dc_step %.2e (<= 1e-12)' % (H, W, b, e))
        assert e <= 1e-12, (b, e)


@pytest.mark.parametrize('per_slice', [False, True], ids=['shared_noise', 'per_slice_noise'])
@pytest.mark.parametrize('precision, bar', [('f32', 2e-6), ('f64', 1e-12)])
@pytest.mark.parametrize('H, W', SHAPES)
def test_synthesis_and_initial_state(env, H, W, precision, bar, per_slice):
    """y = fft2(img) mask + noise (IN_REAL rows, MID_MASK_ADD columns with one noise array for the batch or one per slice) and
    z0 = |ifft2(y)| (EPI_ABS_COMPLEX rows), w0 = 0: float 2e-6 (test_synthesize_and_init), double 1e-12."""
    P = env['P']
    masks, imgs, _, noise, _ = _problem(H, W)
    with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
        eng.synthesize(imgs, noise if per_slice else noise[0], masks, MID)
        _assert_fixed_generic(_path(eng), H, W)
        y = eng.download_y()
        eng.init_state()
        z, w = eng.get_state()
    assert y.shape == z.shape == w.shape == (B, H, W)
    for b in range(B):
        y_ref = O.synthesize(imgs[b].astype(np.float64), masks[MID[b]].astype(np.float64), noise[b if per_slice else 0])
        x0, _, _ = O.init_state(y_ref)
        e = rel_l2(y[b], y_ref), rel_l2(z[b], x0)
        print('%dx%d %s slice %d: y %.2e, z0 %.2e (<= %g)' % (H, W, precision, b, *e, bar))
        assert e[0] <= bar and e[1] <= bar, (b, e)
    assert not w.any()


@functools.lru_cache(maxsize=None)
def _loops(H, W, precision):
    """The loops of one shape and precision, run once and shared: float 10 CNC + 10 L1 iterations on the synthesised problem, double
    100 CNC + 20 L1 on the uploaded one; with them the split run (4 then 6), slice 1 alone on a context of Bmax = 1, the device metrics
    of the CNC result and the oracle's results for the y the device holds."""
    import pnp_admm_cnc_mri_amd as P
    masks, imgs, ys, noise, gt = _problem(H, W)
    f64 = precision == 'f64'
    n_cnc, n_l1 = (100, 20) if f64 else (10, 10)
    out = dict(n_cnc=n_cnc, n_l1=n_l1)

    def run(eng, solver, parts):
        eng.init_state()
        for n in parts:
            eng.admm_cnc(n, *CNC) if solver == 'cnc' else eng.admm_l1(n, *L1)
        return (eng.x(), *eng.get_state())

    t0 = time.perf_counter()
    with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
        if f64:
            eng.upload(ys, masks, MID)
        else:
            eng.synthesize(imgs, noise.astype(np.complex64), masks, MID)
        out['path'] = _path(eng)
        y = eng.download_y()
        out['cnc'] = run(eng, 'cnc', (n_cnc,))
        out['psnr'], out['re'] = eng.metrics(None, gt)
        out['ssim'] = eng.ssim(None, gt)
        out['l1'] = run(eng, 'l1', (n_l1,))
        if not f64:
            out['cnc_split'] = run(eng, 'cnc', (4, 6))
            out['l1_split'] = run(eng, 'l1', (4, 6))
    if not f64:
        with P.Engine(H, W, Bmax=1) as eng:
            eng.upload(y[1:2], masks, MID[1:2])
            out['path_one'] = _path(eng)
            out['cnc_one'] = run(eng, 'cnc', (n_cnc,))
            out['l1_one'] = run(eng, 'l1', (n_l1,))
    out['gpu_seconds'] = time.perf_counter() - t0
    out['y'] = y
    y128 = y.astype(np.complex128)
    out['ref_cnc'] = [O.admm_cnc(y128[b], masks[MID[b]], n_cnc, *CNC) for b in range(B)]
    out['ref_l1'] = [O.admm_l1(y128[b], masks[MID[b]], n_l1, *L1) for b in range(B)]
    return out


@pytest.mark.parametrize('H, W', SHAPES)
def test_admm_loops_float_against_oracle(env, H, W):
    """10 iterations of both loops per slice against the float64 oracle, <= 1e-5 (test_admm_loops_float_against_oracle; NumPy's own
    float32 run of these problems is 4.1e-7 .. 7.7e-7 from the oracle); x, z, w finite; 10 iterations = 4 then 6 and slice 1 alone on a
    context of Bmax = 1 = slice 1 of the batch, bit for bit."""
    r = _loops(H, W, 'f32')
    _assert_fixed_generic(r['path'], H, W)
    _assert_fixed_generic(r['path_one'], H, W)
    for b in range(B):
        ec, el = rel_l2(r['cnc'][0][b], r['ref_cnc'][b]), rel_l2(r['l1'][0][b], r['ref_l1'][b])
        print('%dx%d slice %d (mask %d): CNC %.2e, L1 %.2e (<= 1e-5)' % (H, W, b, MID[b], ec, el))
        assert ec <= 1e-5 and el <= 1e-5, (b, ec, el)
    for solver in ('cnc', 'l1'):
        for a, s, o in zip(r[solver], r[solver + '_split'], r[solver + '_one']):
            assert a.shape == (B, H, W) and np.isfinite(a).all()
            assert np.array_equal(a, s), solver
            assert np.array_equal(a[1], o[0]), solver


@pytest.mark.parametrize('H, W', SHAPES)
def test_admm_loops_double_against_oracle(env, H, W):
    """100 CNC and 20 L1 iterations on a double context, <= 1e-8 (test_admm_cnc_double_100_iterations_against_oracle): k_cols<512, double>
    with 8 columns per tile and k_cols<256, double> at W != H."""
    r = _loops(H, W, 'f64')
    _assert_fixed_generic(r['path'], H, W)
    print('%dx%d double: device part of the loops (100 CNC + 20 L1, metrics) %.2f s' % (H, W, r['gpu_seconds']))
    for b in range(B):
        ec, el = rel_l2(r['cnc'][0][b], r['ref_cnc'][b]), rel_l2(r['l1'][0][b], r['ref_l1'][b])
        print('%dx%d double slice %d (mask %d): CNC %.2e, L1 %.2e (<= 1e-8)' % (H, W, b, MID[b], ec, el))
        assert ec <= 1e-8 and el <= 1e-8, (b, ec, el)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in r['cnc'] + r['l1'])


@pytest.mark.parametrize('H, W', SHAPES)
def test_transposed_problem_gives_the_transposed_image(env, H, W):
    """(y^T, mask^T) on the (W, H) context returns x^T of the (H, W) context within twice the float loop bar: the rows of one shape are the
    columns of the other, so an error both contexts share with respect to the oracle comparison does not cancel here.  No bit-equality:
    the two contexts run different kernels."""
    P = env['P']
    masks, _, _, _, _ = _problem(H, W)
    r = _loops(H, W, 'f32')
    _assert_fixed_generic(r['path'], H, W)
    yt = np.ascontiguousarray(r['y'].transpose(0, 2, 1))
    mt = np.ascontiguousarray(masks.transpose(0, 2, 1))
    with P.Engine(W, H, Bmax=BMAX) as eng:
        eng.upload(yt, mt, MID)
        _assert_fixed_generic(_path(eng), W, H)
        eng.init_state()
        eng.admm_cnc(10, *CNC)
        xc = eng.x()
        eng.init_state()
        eng.admm_l1(10, *L1)
        xl = eng.x()
    for b in range(B):
        ec, el = rel_l2(xc[b].T, r['cnc'][0][b]), rel_l2(xl[b].T, r['l1'][0][b])
        print('%dx%d slice %d: transposed CNC %.2e, L1 %.2e (<= 2e-5)' % (H, W, b, ec, el))
        assert ec <= 2e-5 and el <= 2e-5, (b, ec, el)


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('H, W', SHAPES)
def test_metrics_and_ssim_match_the_reference_formulas(env, H, W, precision):
    """pnp_metrics / pnp_ssim of the context's x after the CNC loop against the reference formulas on the returned x
    (the bars of test_sub_batch_is_bit_equal_and_metrics_match_reference: 1e-9, 1e-12, 1e-9)."""
    gt = _problem(H, W)[4]
    r = _loops(H, W, precision)
    _assert_fixed_generic(r['path'], H, W)
    for b in range(B):
        e = r['cnc'][0][b].astype(np.float64) * 255
        d = (abs(r['psnr'][b] - O.calculate_psnr(e, gt[b])), abs(r['re'][b] - O.calculate_re(e, gt[b])),
             abs(r['ssim'][b] - O.calculate_ssim(e, gt[b])))
        print('%dx%d %s slice %d: |dPSNR| %.2e (<= 1e-9), |dRE| %.2e (<= 1e-12), |dSSIM| %.2e (<= 1e-9)' % (H, W, precision, b, *d))
        assert d[0] <= 1e-9 and d[1] <= 1e-12 and d[2] <= 1e-9, (b, d)


@pytest.mark.parametrize('solver', ['l1', 'cnc'])
def test_traced_run_is_bit_identical_to_the_untraced_run(env, solver):
    """256 x 512, float: the assertions of the 'generic' case of tests/test_gpu_trace.py, and the z_norm / w_norm of the last row are the
    norms of get_state()."""
    P = env['P']
    H, W, K = 256, 512, 15
    masks, imgs, _, noise, gt = _problem(H, W)

    def run(eng, **kw):
        return eng.admm_cnc(K, *CNC, **kw) if solver == 'cnc' else eng.admm_l1(K, *L1, **kw)

    def norm(a):
        return np.sqrt((np.asarray(a, np.float64).reshape(len(a), -1) ** 2).sum(1))

    with P.Engine(H, W, Bmax=BMAX) as eng:
        eng.synthesize(imgs, noise.astype(np.complex64), masks, MID)
        _assert_fixed_generic(_path(eng), H, W)
        eng.init_state()
        assert run(eng) is None
        ref = (eng.x(), *eng.get_state())
        traces = {}
        for every, with_gt in ((1, True), (7, False)):
            eng.init_state()
            tr = run(eng, trace_every=every, gt=gt if with_gt else None)
            got = (eng.x(), *eng.get_state())
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))
            assert tr['iters_done'] == K and list(tr['iter']) == ([k for k in range(every, K + 1, every)] + ([K] if K % every else []))
            assert (tr['converged_at'] == 0).all() and ('psnr' in tr) == with_gt
            assert all(np.isfinite(tr[n]).all() and tr[n].shape == (len(tr['iter']), B) for n in NAMES)
            for n, a in (('x_norm', got[0]), ('z_norm', got[1]), ('w_norm', got[2])):
                want = norm(a)
                assert (np.abs(tr[n][-1] - want) <= 1e-12 * want).all(), (n, tr[n][-1], want)
            traces[every] = tr
        psnr, re = eng.metrics(None, gt)
        assert np.abs(traces[1]['psnr'][-1] - psnr).max() <= 1e-9 and np.abs(traces[1]['re'][-1] - re).max() <= 1e-9
        for k in (7, 14, 15):
            for n in NAMES:
                assert np.array_equal(traces[1][n][list(traces[1]['iter']).index(k)], traces[7][n][list(traces[7]['iter']).index(k)]), (k, n)


def test_solver_entry_point_on_a_rectangular_fixed_shape(env):
    """ADMM_CNC the way a caller uses it, 256 x 512: solvers.py on a fixed-size context with H != W."""
    P = env['P']
    H, W = 256, 512
    masks, _, ys, _, gt = _problem(H, W)
    with P.Engine(H, W, Bmax=B) as eng:                                 # the context the solver opens: Bmax = B
        eng.upload(ys, masks, MID)
        _assert_fixed_generic(_path(eng), H, W)
    out, info = P.ADMM_CNC(masks, None, y=ys, mask_id=MID, images=gt, return_info=True, iter_num=10, alpha=CNC[0], lambda1=CNC[1],
                           reo=CNC[2], b=CNC[3])
    for b in range(B):
        assert out[b].shape == (H, W)
        ref = O.admm_cnc(ys[b].astype(np.complex64).astype(np.complex128), masks[MID[b]], 10, *CNC)
        e = rel_l2(out[b], ref)
        d = abs(info['psnr'][b] - O.calculate_psnr(out[b] * 255, gt[b])), abs(info['ssim'][b] - O.calculate_ssim(out[b] * 255, gt[b]))
        print('ADMM_CNC 256x512 slice %d: %.2e (<= 1e-5), |dPSNR| %.2e, |dSSIM| %.2e (<= 1e-9)' % (b, e, *d))
        assert e <= 1e-5 and d[0] <= 1e-9 and d[1] <= 1e-9, (b, e, d)


# ------------------------------------------------------------------------------------------------------------------------------------
# B. / C. the pointwise kernels on caller pointers
# ------------------------------------------------------------------------------------------------------------------------------------
#          H    W    B      n        n % 4   grid strides
CASES = [(129, 131, 1),   # 16 899     3       1
         (129, 130, 1),   # 16 770     2       1
         (129, 131, 3),   # 50 697     1       1
         (256, 256, 2),   # 131 072    0       1
         (512, 512, 9),   # 2 359 296  0       2   (2048 blocks x 256 lanes x 4 floats = 2 097 152 per stride)
         (837, 837, 3)]   # 2 101 707  3       2   a second stride and a tail in one launch
COUNTS = {(129, 131, 1): (16899, 3), (129, 130, 1): (16770, 2), (129, 131, 3): (50697, 1), (256, 256, 2): (131072, 0),
          (512, 512, 9): (2359296, 0), (837, 837, 3): (2101707, 3)}
MISALIGNED_CASES = [(129, 131, 1), (256, 256, 2)]
PAD = 64
GLUE = (0.9, 1.35, 0.45, 0.3)                                      # alpha, lambda1, reo, b of test_glue_kernels
# argument order of the call, and which of the arguments it writes
OPS = {'prox_l1': (('x', 'z', 'w'), ('z', 'w')), 'prox_cnc': (('x', 'z', 'w'), ('z', 'w')), 'cnc_combine': (('z', 'x', 'w', 's', 't'), ('t',)),
       'add': (('a', 'b', 'o'), ('o',)), 'dual_clamp': (('x', 'z', 'w'), ('x', 'z', 'w'))}
BARS = {'prox_l1': 2e-7, 'prox_cnc': 5e-7, 'cnc_combine': 2e-7, 'add': 0.0, 'dual_clamp': 0.0}          # absolute; 0: equality


@pytest.fixture(scope='module')
def engines(env):
    """one context per case, shared by the tests: no coils, an all-zero y -- the pointwise calls need a problem only for B"""
    P = env['P']
    cache = {}

    def get(H, W, nb):
        if (H, W, nb) not in cache:
            eng = P.Engine(H, W, Bmax=nb)
            eng.upload(np.zeros((nb, H, W), np.complex64), np.ones((H, W), np.uint8))
            cache[(H, W, nb)] = eng
        n, rem = COUNTS[(H, W, nb)]
        assert n == nb * H * W and n % 4 == rem
        return cache[(H, W, nb)], n

    yield get
    for eng in cache.values():
        eng.close()


class _Guarded:
    """n floats on the device as a view inside a larger allocation: at least PAD sentinel floats on either side (every one a different
    finite value), the first element `shift` floats past a 16-byte boundary."""

    def __init__(self, torch, host, shift=0):
        self.torch = torch
        host = np.ascontiguousarray(host, np.float32).reshape(-1)
        self.n = host.size
        self.buf = torch.empty(self.n + 2 * PAD + 8, dtype=torch.float32, device='cuda')
        assert self.buf.data_ptr() % 4 == 0
        self.off = PAD + (-(self.buf.data_ptr() // 4 + PAD)) % 4 + shift
        bits = self.buf.view(torch.int32)
        bits.copy_(torch.arange(bits.numel(), dtype=torch.int32, device='cuda') + 0x4B000000)          # the floats 8388608 + k
        self.view = self.buf[self.off:self.off + self.n]
        self.view.copy_(torch.from_numpy(host).cuda())
        assert self.view.data_ptr() % 16 == 4 * shift and self.view.numel() == self.n
        assert self.off >= PAD and self.buf.numel() - self.off - self.n >= PAD
        self.before = self.buf.clone()

    def host(self):
        return self.view.cpu().numpy()

    def sentinels_intact(self):
        a, b, end = self.buf.view(self.torch.int32), self.before.view(self.torch.int32), self.off + self.n
        return bool(self.torch.equal(a[:self.off], b[:self.off]) and self.torch.equal(a[end:], b[end:]))

    def unchanged(self):
        return bool(self.torch.equal(self.buf.view(self.torch.int32), self.before.view(self.torch.int32)))


def _inputs(op, n):
    """host inputs by argument name.  prox: the generator and ranges of test_prox_kernels.  cnc_combine: z, x, s in [0, 0.25], w in
    [-0.05, 0.05], so that every intermediate of c1 z + c2 (x + w) + c3 (z - s) stays below 0.5: seven float32 roundings of at most
    2^-26 = 1.5e-8 each and the three rounded coefficients (6e-8 relative on terms <= 0.3) stay below 1.6e-7, inside the 2e-7 bar for
    any correct float32 evaluation; a misplaced element is off by ~0.1.  add, dual_clamp: the range of test_glue_kernels."""
    rng = np.random.default_rng(7)

    def u(lo, hi):
        return rng.uniform(lo, hi, n).astype(np.float32)

    if op in ('prox_l1', 'prox_cnc'):
        return dict(x=u(0, 1), z=u(-0.05, 1), w=u(-0.2, 0.2))
    if op == 'cnc_combine':
        return dict(z=u(0, 0.25), x=u(0, 0.25), w=u(-0.05, 0.05), s=u(0, 0.25), t=np.full(n, 777.0, np.float32))
    if op == 'add':
        return dict(a=u(-0.2, 1.2), b=u(-0.2, 1.2), o=np.full(n, 777.0, np.float32))
    return dict(x=u(-0.2, 1.2), z=u(-0.2, 1.2), w=u(-0.2, 1.2))


def _reference(torch, op, h):
    """the outputs by name: float64 NumPy for the calls with a bar, the float32 torch expressions (S6:305-308, as test_glue_kernels) for
    the two that are asserted equal"""
    d = {k: v.astype(np.float64) for k, v in h.items()}
    if op == 'prox_l1':
        z, w = O.l1_step(d['x'], d['z'], d['w'], *L1)
        return dict(z=z, w=w)
    if op == 'prox_cnc':
        z, w = O.cnc_step(d['x'], d['z'], d['w'], *CNC)
        return dict(z=z, w=w)
    if op == 'cnc_combine':
        alpha, lam, reo, b = GLUE
        return dict(t=(1 - alpha) * d['z'] + alpha * (d['x'] + d['w']) + alpha * reo * lam * b * (d['z'] - d['s']))
    t = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
    if op == 'add':
        return dict(o=(t['a'] + t['b']).cpu().numpy())
    wr = t['w'] + t['x'] - t['z']
    return dict(x=t['x'].clamp(0, 1).cpu().numpy(), z=t['z'].clamp(0, 1).cpu().numpy(), w=wr.clamp(0, 1).cpu().numpy())


def _run(env, eng, op, h, shifts=None):
    """the call on guarded device arrays holding h -> the written arguments as host arrays.  Asserts on the way: the sentinels of every
    array are unchanged, the arguments the call only reads are unchanged bit for bit."""
    torch = env['torch']
    args, outs = OPS[op]
    g = {k: _Guarded(torch, h[k], (shifts or {}).get(k, 0)) for k in args}
    v = {k: a.view for k, a in g.items()}
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    if op == 'prox_l1':
        eng.prox_l1_dual(v['x'], v['z'], v['w'], 0.0015)
    elif op == 'prox_cnc':
        eng.prox_cnc_dual(v['x'], v['z'], v['w'], *CNC)
    elif op == 'cnc_combine':
        eng.cnc_combine(v['z'], v['x'], v['w'], v['s'], v['t'], *GLUE)
    elif op == 'add':
        eng.add(v['a'], v['b'], v['o'])
    else:
        eng.dual_clamp(v['x'], v['z'], v['w'])
    torch.cuda.synchronize()
    for k in args:
        assert g[k].sentinels_intact(), (op, k, 'sentinels')
        if k not in outs:
            assert g[k].unchanged(), (op, k, 'an input was written')
    return {k: g[k].host() for k in outs}


def _same(a, b):
    """element-wise: equal, or both NaN"""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _compare(label, op, got, ref, n):
    """the whole array within the bar of the call, then the last vector and the tail -- the elements 4 (n / 4) - 4 .. n - 1 -- one by one"""
    bar = BARS[op]
    lo = 4 * (n // 4) - 4
    for k, r in ref.items():
        a = got[k]
        assert a.shape == r.shape == (n,)
        if bar == 0:
            err = (~_same(a, r)).astype(np.float64)
            what = 'elements that differ'
        else:
            err = np.abs(a.astype(np.float64) - r)
            what = 'max abs error'
        print('%s %s %s: %s %.3g whole array, %.3g over the last vector and the tail [%d, %d) (bar %g)' % (
            label, op, k, what, err.max(), err[lo:].max(), lo, n, bar))
        assert err.max() <= bar, (op, k, float(err.max()), int(err.argmax()))
        for i in range(lo, n):
            assert err[i] <= bar, (op, k, i, a[i], r[i])


@pytest.mark.parametrize('op', list(OPS))
@pytest.mark.parametrize('H, W, nb', CASES)
def test_pointwise_kernels_tail_and_grid_stride(env, engines, H, W, nb, op):
    eng, n = engines(H, W, nb)
    h = _inputs(op, n)
    got = _run(env, eng, op, h)
    _compare('%dx%d B=%d n=%d (n %% 4 = %d)' % (H, W, nb, n, n % 4), op, got, _reference(env['torch'], op, h), n)


@pytest.mark.parametrize('which', ['x', 'z', 'w'])
@pytest.mark.parametrize('H, W, nb', CASES)
def test_dual_clamp_special_values_in_the_tail(env, engines, H, W, nb, which):
    """The special values of test_glue_kernels (NaN, +-inf, +-0, denormals, +-3.4e38) as the last 16 elements -- the last vectors and
    the tail -- of x, z or w: tensor.clamp_(0, 1) keeps NaN and sends +-inf to the bounds (S6:306-308), and so must every element."""
    eng, n = engines(H, W, nb)
    nan, inf = float('nan'), float('inf')
    special = np.array([nan, inf, -inf, -0.0, 0.0, 1.0, 2.5, -3.0, 0.25, nan, inf, -inf, 1e-45, -1e-45, 3.4e38, -3.4e38], np.float32)
    h = _inputs('dual_clamp', n)
    special = np.roll(special, 6)                                       # a NaN is the very last element: in the tail whenever there is one
    h[which][-special.size:] = special
    got = _run(env, eng, 'dual_clamp', h)
    _compare('%dx%d B=%d n=%d (n %% 4 = %d) specials in %s' % (H, W, nb, n, n % 4, which), 'dual_clamp', got,
             _reference(env['torch'], 'dual_clamp', h), n)
    at = n - special.size + np.flatnonzero(np.isnan(special))
    assert at.size == 2 and at[-1] == n - 1
    for k in {which, 'w'}:                                              # NaN in -> NaN out: in the array itself and in w = w + x - z
        assert np.isnan(got[k][at]).all(), (k, got[k][at])
    for k in ('x', 'z', 'w'):
        assert np.isfinite(got[k][:n - special.size]).all()


@pytest.mark.parametrize('op', list(OPS))
@pytest.mark.parametrize('H, W, nb', MISALIGNED_CASES)
def test_misaligned_pointers_take_the_scalar_path(env, engines, H, W, nb, op):
    """include/pnp_mri.h promises the C type and nothing more: every argument in turn one float past a 16-byte boundary.  The result equals
    the aligned call's bit for bit, within the bar of the call, sentinels and inputs untouched."""
    eng, n = engines(H, W, nb)
    h = _inputs(op, n)
    ref = _reference(env['torch'], op, h)
    aligned = _run(env, eng, op, h)
    for k in OPS[op][0]:
        got = _run(env, eng, op, h, {k: 1})
        _compare('n=%d, %s 4 bytes past a 16-byte boundary:' % (n, k), op, got, ref, n)
        for name, a in got.items():
            assert np.array_equal(a.view(np.int32), aligned[name].view(np.int32)), (op, k, name)
    got = _run(env, eng, op, h, {k: 1 + i % 3 for i, k in enumerate(OPS[op][0])})          # every argument off, by 4, 8 and 12 bytes
    for name, a in got.items():
        assert np.array_equal(a.view(np.int32), aligned[name].view(np.int32)), (op, 'all', name)
