"""GPU tests of the any-size path (csrc/kernels_anysize.hip): slices of any H, W in [128, 1024] -- 7-smooth lengths on the
mixed-radix Stockham kernels (252 = 4 * 3 * 3 * 7 with a radix-7 stage, 135 = 3 * 3 * 3 * 5 with no even stage), the others
(218 = 2 * 109, 170 = 2 * 5 * 17, 1021) on Bluestein.  Every length on both axes: test_gpu_anysize_sweep.py.

  operators  fft2 / ifft2 / A / A^H / Df against NumPy (float, <= 2e-6 relative); synthesis and z0 = |ifft2(y)| of a double
             context against NumPy (<= 1e-12)
  loops      ADMM_L1 / ADMM_CNC against oracle/admm_oracle.py at B = 3, seeded masks and noise: float <= 1e-5 at 10 iterations,
             double <= 1e-8 at 100 CNC iterations
  PnP        PNP_ADMM_CNC_D with FFDNet (contractive fixture weights) against the oracle loop driven by the same GPU denoiser
  the rest   sub-batch bit-equality, PSNR / RE / SSIM against the reference formulas, the path and plan queries"""
import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import rel_l2, weights50

pytestmark = pytest.mark.gpu

OP_SHAPES = [(128, 128), (320, 320), (384, 384), (218, 170), (640, 368), (192, 256), (1021, 1000), (256, 320), (252, 135)]
LOOP_SHAPES = [(320, 320), (218, 170), (640, 368), (252, 135)]
KINDS = ('random', 'radial', 'cartesian')


@pytest.fixture(scope='module')
def env():
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib, utils_pnp
    assert _lib.device_count() >= 1 and torch.cuda.is_available()
    return dict(torch=torch, P=P, U=utils_pnp)


def _problem(H, W, B):
    masks = np.stack([O.synthetic_mask(k, H, W) for k in KINDS]).astype(np.uint8)
    mid = (np.arange(B) % 3).astype(np.int32)
    imgs, ys = zip(*(O.synthetic_problem(b, masks[mid[b]], H, W) for b in range(B)))
    return masks, mid, np.stack(imgs), np.stack(ys)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@pytest.mark.parametrize('H, W', OP_SHAPES)
def test_operators_against_numpy(env, H, W):
    torch, P, U = env['torch'], env['P'], env['U']
    B = 3
    masks, mid, imgs, ys = _problem(H, W, B)
    rng = np.random.default_rng(H * 4096 + W)
    xc = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
    xr = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    with P.Engine(H, W, Bmax=B) as eng:
        assert eng.ctx_path == ('anysize' if (H, W) not in ((256, 256), (512, 512)) else eng.path_name)
        eng.upload(ys.astype(np.complex64), masks, mid)
        dc, dr = torch.from_numpy(xc).cuda(), torch.from_numpy(xr).cuda()
        x64, r64 = xc.astype(np.complex128), xr.astype(np.float64)
        got = {'fft2': U.fft2(eng, dc), 'ifft2': U.ifft2(eng, dc), 'A': U.A(eng, dr), 'AH': U.AH(eng, dc), 'Df': U.Df(eng, dr)}
        torch.cuda.synchronize()
        for b in range(B):
            m, y = masks[mid[b]].astype(np.float64), ys[b].astype(np.complex64).astype(np.complex128)
            ref = {'fft2': np.fft.fft2(x64[b]), 'ifft2': np.fft.ifft2(x64[b]), 'A': O.A(r64[b], m), 'AH': O.AH(x64[b], m),
                   'Df': O.Df(r64[b], m, y)}
            for k, v in got.items():
                e = _rel(v[b].cpu().numpy(), ref[k])
                assert e <= 2e-6, (k, b, e)


def _plans_ok(eng, H, W):
    for axis, n in ((0, W), (1, H)):
        p = eng.fft_plan(axis)
        smooth = all(q in (2, 3, 5, 7) for q in _primes(n))
        assert p.startswith('stockham %d =' % n if smooth else 'bluestein %d ->' % n), p


def _primes(n):
    out, q = [], 2
    while n > 1:
        while n % q == 0:
            out.append(q)
            n //= q
        q += 1
    return out


@pytest.mark.parametrize('H, W', [(218, 170), (320, 320), (1021, 1000), (640, 368)])
def test_double_context_synthesis_and_init_against_numpy(env, H, W):
    P = env['P']
    B = 2
    masks, mid, imgs, _ = _problem(H, W, B)
    noise = np.stack([O.kspace_noise(b, H, W) for b in range(B)])
    with P.Engine(H, W, Bmax=B, precision='f64') as eng:
        _plans_ok(eng, H, W)
        eng.synthesize(imgs, noise, masks, mid)
        y = eng.download_y()
        eng.init_state()
        z, w = eng.get_state()
    for b in range(B):
        m = masks[mid[b]].astype(np.float64)
        ref = np.fft.fft2(imgs[b].astype(np.float64)) * m + noise[b]
        assert _rel(y[b], ref) <= 1e-12
        assert _rel(z[b], np.abs(np.fft.ifft2(y[b]))) <= 1e-12 and not np.any(w[b])


@pytest.mark.parametrize('H, W', LOOP_SHAPES)
def test_admm_loops_float_against_oracle(env, H, W):
    P = env['P']
    B = 3
    masks, mid, imgs, _ = _problem(H, W, B)
    noise = np.stack([O.kspace_noise(b, H, W) for b in range(B)]).astype(np.complex64)
    with P.Engine(H, W, Bmax=B) as eng:
        assert eng.ctx_path == 'anysize' and eng.path_name == 'generic' and eng.kernels_per_iteration == 3
        eng.synthesize(imgs, noise, masks, mid)
        y = eng.download_y()
        eng.init_state()
        eng.admm_cnc(10, 0.45, 0.5, 0.05, 64)
        xc = eng.x()
        eng.init_state()
        eng.admm_l1(10, 0.1, 0.015)
        xl = eng.x()
    for b in range(B):
        y64 = y[b].astype(np.complex128)
        assert _rel(xc[b], O.admm_cnc(y64, masks[mid[b]], 10)) <= 1e-5
        assert _rel(xl[b], O.admm_l1(y64, masks[mid[b]], 10)) <= 1e-5


@pytest.mark.parametrize('H, W', LOOP_SHAPES)
def test_admm_cnc_double_100_iterations_against_oracle(env, H, W):
    P = env['P']
    B = 3
    masks, mid, _, ys = _problem(H, W, B)
    with P.Engine(H, W, Bmax=B, precision='f64') as eng:
        eng.upload(ys, masks, mid)
        eng.init_state()
        eng.admm_cnc(100, 0.45, 0.5, 0.05, 64)
        xc = eng.x()
        eng.init_state()
        eng.admm_l1(20, 0.1, 0.015)
        xl = eng.x()
    for b in range(B):
        assert _rel(xc[b], O.admm_cnc(ys[b], masks[mid[b]], 100)) <= 1e-8
        assert _rel(xl[b], O.admm_l1(ys[b], masks[mid[b]], 20)) <= 1e-8


def test_sub_batch_is_bit_equal_and_metrics_match_reference(env):
    P = env['P']
    H, W = 218, 170
    B = 3
    masks, mid, imgs, ys = _problem(H, W, B)
    gt = np.round(imgs.astype(np.float64) * 255).astype(np.uint8)
    y32 = ys.astype(np.complex64)
    with P.Engine(H, W, Bmax=B) as eng:
        eng.upload(y32, masks, mid)
        eng.init_state()
        eng.admm_cnc(6, 0.45, 0.5, 0.05, 64)
        full = eng.x()
        psnr, re = eng.metrics(None, gt)
        ssim = eng.ssim(None, gt)
        eng.upload(y32[1:2], masks, mid[1:2])
        eng.init_state()
        eng.admm_cnc(6, 0.45, 0.5, 0.05, 64)
        one = eng.x()
    assert np.array_equal(full[1], one[0])
    for b in range(B):
        e = full[b].astype(np.float64) * 255
        assert abs(psnr[b] - O.calculate_psnr(e, gt[b])) <= 1e-9
        assert abs(re[b] - O.calculate_re(e, gt[b])) <= 1e-12
        assert abs(ssim[b] - O.calculate_ssim(e, gt[b])) <= 1e-9


def test_fixed_shapes_keep_their_kernels(env):
    P = env['P']
    for H, W in ((256, 256), (512, 512), (256, 512)):
        with P.Engine(H, W, Bmax=1) as eng:
            assert eng.ctx_path != 'anysize' and eng.fft_plan(0) == 'fixed %d' % W and eng.fft_plan(1) == 'fixed %d' % H


@pytest.mark.parametrize('H, W, backend', [(320, 320, 'hip_f16x3'), (218, 170, 'auto')])
def test_pnp_admm_cnc_d_ffdnet_against_oracle_loop(env, H, W, backend, tmp_path):
    """PNP_ADMM_CNC_D at a new shape, B = 3 with three seeded masks, the contractive FFDNet fixture: the batched device loop equals
    the oracle's per-slice loop driven by the same GPU denoiser (<= 1e-5).  218 x 170 is not a multiple of 8: 'auto' takes PyTorch."""
    torch = env['torch']
    from pnp_admm_cnc_mri_amd import denoisers as D, solvers_pnp as S
    name = 'ffdnet_gray'
    B = 3
    masks, mid, _, ys = _problem(H, W, B)
    ys = ys.astype(np.complex64)
    sd = weights50(name)
    net, nlm, _ = D.build(name)
    net.load_state_dict(sd)
    resolved = D.auto_backend(net, None, None, None, (H, W))[0] if backend == 'auto' else backend
    if backend == 'auto':
        assert resolved == 'torch'
    den = D.Denoiser(name, net.eval(), nlm, backend=resolved).to(torch.device('cuda'))

    def denoise(a, i):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None].cuda()
        return den(t, i)[0, 0].cpu().numpy()

    alpha, lam, reo, b_ = 0.9, 1.35, 0.45, 0.3
    iters = 5
    out, _ = S.PNP_ADMM_CNC_D(name, masks, None, y=ys, mask_id=mid, model=sd, results=str(tmp_path), cnn_backend=backend,
                              alpha=alpha, iter_num=iters, lambda1=lam, reo=reo, b=b_)
    for b in range(B):
        assert out[b].shape == (H, W)
        ref = O.pnp_admm_cnc(ys[b].astype(np.complex128), masks[mid[b]], denoise, iters, alpha, lam, reo, b_)
        assert rel_l2(out[b], ref) <= 1e-5, (b, rel_l2(out[b], ref))
