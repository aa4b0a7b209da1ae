"""Complex-valued images on a coil context (pnp_set_image, image='complex') on the GPU against tests/complex_oracle.py.

Set-up: B = 3 slices of the phase phantom with the true maps, a bank of two masks with mask_id = [1, 0, 1], contexts of Bmax = 7.  Maps and
y are rounded to complex64 once, so that a float engine, a double engine and the oracle start from the same numbers.
Shapes: 128 x 128 (radix-2), 128 x 130 (mixed radix), 131 x 128 (Bluestein), 140 x 160, with C = 5, 5, 8, 1.  The wavelet prox needs H and W
divisible by 2^levels, so it runs at 128 x 128 (levels 1 and 3), 128 x 130 (1) and 140 x 160 (1 and 2); 131 x 128 admits no level at all
(pnp_sparsity_check refuses it) and runs the pixel prox only.  The pixel prox is pointwise: 128 x 128 and 131 x 128 with B = 3, and B = 1
at 129 x 131 -- an odd element count -- for the float kernel's tail.
Bars: float 4 x the distance of the oracle's complex64 restatement from its complex128 form ON THE SAME CASE (computed here, per case);
double 1e-12 for single steps, 1e-10 for ten iterations."""
import ctypes
import functools

import numpy as np
import pytest

import coilmix_oracle as CO
import complex_oracle as X
import multicoil_oracle as M
from conftest import rel_l2

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
B, BMAX = 3, 7
MID = np.array([1, 0, 1], np.int32)
SHAPES = [(128, 128, 5), (128, 130, 5), (131, 128, 8), (140, 160, 1)]          # H, W, C
CNC = dict(alpha=0.5, lambda1=1.25, reo=1.0, b=4.0)                            # thr = 0.625, c3 = 2.5, ib = 0.25: all exact in float


def cdt(precision):
    return C128 if precision == 'f64' else C64


def tdt(precision):
    import torch
    return torch.complex128 if precision == 'f64' else torch.complex64


def dev(a, precision='f32'):
    import torch
    return torch.from_numpy(np.array(a, dtype=cdt(precision), order='C')).to('cuda')          # a copy: the cached inputs are read-only


def bar_of(fn, precision, double=1e-12):
    """4 x the complex64 restatement's distance from the oracle (fn(dt) -> array); `double` on a double engine.  -> (reference, bar)"""
    ref = fn(C128)
    return ref, (double if precision == 'f64' else 4 * X.rel(fn(C64), ref))


@functools.lru_cache(maxsize=None)
def case(H, W, C, cal=0):
    """-> S [C,H,W], masks [2,H,W], truth [B,H,W], y [B,C,H,W]; complex128 holding complex64 values.  cal: a sampled calibration square"""
    S = M.coil_maps(C, H, W, H + C).astype(C64).astype(C128)
    masks = np.stack([M.mask(H + k, H, W) for k in range(2)])
    if cal:
        masks = np.stack([(m.astype(bool) | CO.cal_region(cal, H, W)).astype(np.uint8) for m in masks])
    t = np.stack([X.truth(10 * H + b, H, W) for b in range(B)])
    y = np.stack([M.A(t[b], S, masks[MID[b]]) + M.noise(b, C, masks[MID[b]]) for b in range(B)]).astype(C64).astype(C128)
    for a in (S, masks, t, y):
        a.setflags(write=False)
    return S, masks, t, y


def open_engine(H, W, C, precision='f32', Bmax=BMAX, upload=True, cg_iters=3):
    import pnp_admm_cnc_mri_amd as P
    S, masks, t, y = case(H, W, C)
    eng = P.Engine(H, W, Bmax=Bmax, precision=precision)
    eng.set_coils(S, cg_iters)
    eng.set_image_mode('complex')
    if upload:
        eng.upload(y, masks, MID)
    return eng


def state(H, W, C):
    """a complex state with a non-trivial dual, in complex64 values: z = A^H y, w a tenth of it with a turning phase"""
    S, masks, t, y = case(H, W, C)
    z = np.stack([M.AH(y[b], S, masks[MID[b]]) for b in range(B)]).astype(C64)
    w = (0.1 * z * np.exp(1j * np.arange(W) / 9.0)[None, None, :]).astype(C64)
    return z.astype(C128), w.astype(C128)


# ---- 1. initial state, A on a complex image ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,C', SHAPES)
@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_init_state_is_AHy_without_the_modulus(H, W, C, precision):
    import torch
    from pnp_admm_cnc_mri_amd import utils_pnp as U
    S, masks, t, y = case(H, W, C)
    with open_engine(H, W, C, precision) as eng:
        assert eng.image_mode == 'complex' and eng.path_name == 'coils' and eng.plan['launches_per_iteration'] == 5 + 5 * 3 + 1
        eng.init_state()
        z, w = eng.get_state()
        kA = U.A(eng, dev(t)).cpu().numpy() if precision == 'f32' else None
        zt, wt = (torch.empty((B, H, W), dtype=tdt(precision), device='cuda') for _ in range(2))
        eng.get_state(zt, wt)
        eng.sync()
        assert np.array_equal(zt.cpu().numpy(), z) and not wt.cpu().numpy().any()
    assert z.dtype == cdt(precision) and z.shape == (B, H, W) and not w.any()
    for b in range(B):
        m = masks[MID[b]]
        ref, bar = bar_of(lambda dt: M.AH(y[b].astype(dt), S, m, dt), precision)
        err = rel_l2(z[b], ref)
        print('z0 %s slice %d: %.2e (bar %.2e)' % (precision, b, err, bar))
        assert err <= bar and np.abs(z[b].imag).max() > 0.01 * np.abs(z[b]).max(), (b, err, bar)
        if kA is not None:
            t32 = t[b].astype(C64)
            refA, barA = bar_of(lambda dt: M.A(t32, S, m, dt), precision)
            assert rel_l2(kA[b], refA) <= barA, (b, rel_l2(kA[b], refA), barA)


# ---- 2. one x-step ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,C', SHAPES)
@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_one_x_step(H, W, C, precision):
    """pnp_dc_step_cx on device tensors against the oracle's x-step; pnp_cg_residual to three digits in double.  THE FLOAT BOUND DEPARTS
    FROM THE ISSUE, which asks for three digits: a residual of 1.7e-7 of the right-hand side sits at the rounding floor of float sums
    and cannot agree to three digits with a float64 oracle, so in float it is held within a factor of 2 of the oracle's
    (tests/test_gpu_multicoil.py's rule), and below one float epsilon where the oracle's is (C = 1)."""
    import torch
    S, masks, t, y = case(H, W, C)
    z, w = state(H, W, C)
    reo = 0.05
    with open_engine(H, W, C, precision) as eng:
        x = torch.empty((B, H, W), dtype=tdt(precision), device='cuda')
        eng.dc_step(dev(z, precision), dev(w, precision), x, reo)
        eng.sync()
        got, res = x.cpu().numpy(), eng.cg_residual()
    for b in range(B):
        m = masks[MID[b]]
        step = lambda dt: X.x_step(z[b], w[b], M.AH(y[b].astype(dt), S, m, dt), S, m, reo, 3, dt, residual=True)
        ref, bar = bar_of(lambda dt: step(dt)[0], precision)
        rel = step(C128)[1]
        err = rel_l2(got[b], ref)
        print('%s x-step slice %d: %.2e (bar %.2e)  residual %.4e (oracle %.4e)' % (precision, b, err, bar, res[b], rel))
        assert err <= bar, (b, err, bar)
        assert np.abs(got[b].imag).max() > 0.01 * np.abs(got[b]).max()
        if precision == 'f64':
            assert abs(res[b] - rel) <= 5e-4 * rel, (b, res[b], rel)
        elif rel >= 2.0 ** -23:
            assert rel / 2 <= res[b] <= rel * 2, (b, res[b], rel)
        else:                                                  # C = 1, |S| = 1: the first CG iteration is the closed form and the residual is
            assert res[b] < 2.0 ** -23, (b, res[b], rel)       # rounding alone, below one float epsilon in either arithmetic


# ---- 3. the pixel prox alone -----------------------------------------------------------------------------------------------------------

def prox_inputs(n, seed):
    """x, z, w [n] complex in float32 values; the first entries: u = 0, |u| exactly thr = 0.625 (3-4-5 over 8), |z| exactly ib = 0.25"""
    rng = np.random.default_rng(seed)
    x, z, w = ((s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(C64) for s in (0.5, 0.3, 0.3))
    x[0], w[0] = 0.25 - 0.5j, -0.25 + 0.5j                    # u = 0
    x[1], w[1] = 0.125 + 0.75j, 0.25 - 0.25j                  # u = 3/8 + 4/8 i
    x[2], w[2] = -0.375, -0.5j                                # u = -3/8 - 4/8 i
    z[3], z[4], z[5], z[6] = 0.25, -0.25j, 0, 0.15 + 0.2j     # |z| = ib on both axes, z = 0, |z| = ib up to rounding
    x[7] = w[7] = z[7] = 0
    return x.astype(C128), z.astype(C128), w.astype(C128)


@pytest.mark.parametrize('H,W,nb', [(128, 128, 3), (131, 128, 3), (129, 131, 1)])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_pixel_prox(H, W, nb, kind, precision):
    """pnp_prox_l1_dual_cx / pnp_prox_cnc_dual_cx on device tensors: finite everywhere, exact zeros exactly where the oracle of the same
    precision has them (L1: nothing but correctly rounded operations in the same order, so the zeros of the restatement; CNC in double),
    values within the bar."""
    import pnp_admm_cnc_mri_amd as P
    C = 2
    S = M.coil_maps(C, H, W, 1)
    m = M.mask(1, H, W)
    n = nb * H * W
    assert (n % 2 == 1) == (nb == 1)
    x, z, w = prox_inputs(n, H * W + nb)
    with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
        eng.set_coils(S)
        eng.set_image_mode('complex')
        eng.upload(np.zeros((nb, C, H, W), C64), m)
        zt, wt = dev(z.reshape(nb, H, W), precision), dev(w.reshape(nb, H, W), precision)
        if kind == 'l1':
            eng.prox_l1_dual(dev(x.reshape(nb, H, W), precision), zt, wt, 0.625)
        else:
            eng.prox_cnc_dual(dev(x.reshape(nb, H, W), precision), zt, wt, **CNC)
        eng.sync()
        gz, gw = zt.cpu().numpy().ravel(), wt.cpu().numpy().ravel()
    step = (lambda dt: X.l1_step(x, z, w, 0.625, dt)) if kind == 'l1' else (lambda dt: X.cnc_step(x, z, w, dt=dt, **CNC))
    (rz, rw), same = step(C128), step(cdt(precision))
    bar_z = 1e-12 if precision == 'f64' else 4 * X.rel(step(C64)[0], rz)
    bar_w = 1e-12 if precision == 'f64' else 4 * X.rel(step(C64)[1], rw)
    ez, ew = rel_l2(gz, rz), rel_l2(gw, rw)
    print('%s %s %dx%dx%d: z %.2e (bar %.2e)  w %.2e (bar %.2e)  zeros %d' % (kind, precision, nb, H, W, ez, bar_z, ew, bar_w, int((gz == 0).sum())))
    assert np.isfinite(gz.view(gz.real.dtype)).all() and np.isfinite(gw.view(gw.real.dtype)).all()
    assert ez <= bar_z and ew <= bar_w, (ez, bar_z, ew, bar_w)
    assert rz[7] == 0 and gz[7] == 0 and 0 < (gz == 0).sum() < n
    if kind == 'l1' or precision == 'f64':
        assert np.array_equal(gz == 0, same[0] == 0)
    if kind == 'l1':                                           # u = 0 and |u| == thr give exact zeros; the same operations in the same
        assert (rz[:3] == 0).all() and (gz[:3] == 0).all() and (gw[:3] == (x + w)[:3]).all() and 0.1 * n < (gz == 0).sum() < 0.9 * n
        assert np.array_equal(gz, same[0]) and np.array_equal(gw, same[1])          # order: the restatement's bits


# ---- 4. the wavelet prox alone ---------------------------------------------------------------------------------------------------------

WV = [(128, 128, 'haar', 1), (128, 128, 'haar', 3), (128, 128, 'db2', 1), (128, 128, 'db2', 3), (128, 128, 'db4', 1), (128, 128, 'db4', 3),
      (128, 130, 'db2', 1), (140, 160, 'db4', 1), (140, 160, 'db2', 2)]
WCNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)          # thr = 0.225, clip at 0.25: both sides of both populated


@pytest.mark.parametrize('H,W,name,L', WV)
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_wavelet_prox(H, W, name, L, kind, precision):
    """The fused complex wavelet prox against the oracle, and against a composition from the public dwt2 / idwt2 on the real and the
    imaginary plane with the threshold in NumPy (the oracle's csoft in the engine's precision)."""
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import utils_pnp as U
    C = 2
    rng = np.random.default_rng(H + W + L)
    x, z, w = ((s * (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W)))).astype(C64).astype(C128) for s in (0.5, 0.5, 0.3))
    dt, R = cdt(precision), X._real(cdt(precision))
    thr = 0.3
    with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
        eng.set_coils(M.coil_maps(C, H, W, 1))
        eng.set_sparsity(name, L)
        eng.set_image_mode('complex')
        eng.upload(np.zeros((B, C, H, W), C64), M.mask(1, H, W))
        assert eng.plan['launches_per_iteration'] == 5 + 5 * 3 + 2
        xt, zt, wt = dev(x, precision), dev(z, precision), dev(w, precision)
        if kind == 'l1':
            eng.prox_l1_dual(xt, zt, wt, thr)
        else:
            eng.prox_cnc_dual(xt, zt, wt, **WCNC)
        eng.sync()
        gz, gw = zt.cpu().numpy(), wt.cpu().numpy()
        # the composition: Psi on the planes, the threshold in NumPy, Psi^T on the planes
        def psi(v, inverse=False):
            f = U.idwt2 if inverse else U.dwt2
            v = np.asarray(v, dt)
            re, im = (f(eng, torch.from_numpy(np.ascontiguousarray(p)).to('cuda')).cpu().numpy() for p in (v.real, v.imag))
            return (re + 1j * im).astype(dt)
        u = (x + w).astype(dt)
        cu = psi(u)
        det = X.W.detail_mask(H, W, L)
        if kind == 'l1':
            c = np.where(det, X.csoft(cu, thr, dt), cu)
        else:
            t_, c1, c2, c3, ib = X.cnc_scalars(dt=dt, **WCNC)
            cz = psi(z)
            c = np.where(det, X.csoft(X._combine(cz, cu, c1, c2, c3, ib, dt), t_, dt), (c1 * cz + (c2 * cu).astype(dt)).astype(dt))
        comp = psi(c, inverse=True)
    for b in range(B):
        step = (lambda d: X.wl1_step(x[b], z[b], w[b], thr, name, L, d)) if kind == 'l1' else (lambda d: X.wcnc_step(x[b], z[b], w[b], name=name, levels=L, dt=d, **WCNC))
        rz, rw = step(C128)
        s32 = step(C64)
        bar_z = 1e-12 if precision == 'f64' else 4 * X.rel(s32[0], rz)
        bar_w = 1e-12 if precision == 'f64' else 4 * X.rel(s32[1], rw)
        ez, ew, ec = rel_l2(gz[b], rz), rel_l2(gw[b], rw), rel_l2(gz[b], comp[b])
        print('%s %s %s L=%d %dx%d slice %d: z %.2e (bar %.2e)  w %.2e (bar %.2e)  vs composition %.2e' % (kind, precision, name, L, H, W, b, ez, bar_z, ew, bar_w, ec))
        assert np.isfinite(gz[b].view(R)).all() and ez <= bar_z and ew <= bar_w and ec <= bar_z, (b, ez, bar_z, ew, bar_w, ec)


# ---- 5. ten iterations through the solvers -----------------------------------------------------------------------------------------------

def solve(kind, y, masks, precision='f32', **kw):
    import pnp_admm_cnc_mri_amd as P
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    out, info = solver(masks, None, y=y, mask_id=MID, precision=precision, image='complex', return_info=True, iter_num=10, **kw, **M.O_PRESETS[kind])
    return np.stack(out[:len(y)]), info


@functools.lru_cache(maxsize=None)
def loop_refs(H, W, C, kind, transform, levels):
    """per slice: the oracle's ten iterations and the complex64 restatement's distance from them"""
    S, masks, t, y = case(H, W, C)
    rows = []
    for b in range(B):
        f = lambda dt: X.admm(y[b].astype(dt), S, masks[MID[b]], 10, kind, dt=dt, transform=transform, levels=levels)
        ref = f(C128)
        rows.append((ref, X.rel(f(C64), ref)))
    return rows


LOOPS = [s + (None, 0) for s in SHAPES] + [(128, 128, 5, 'db2', 3), (128, 130, 5, 'db2', 1), (140, 160, 1, 'db2', 2)]


@pytest.mark.parametrize('H,W,C,transform,levels', LOOPS)
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_ten_iterations_at_the_presets(H, W, C, transform, levels, kind, precision):
    """ADMM_L1 / ADMM_CNC with image='complex' against the oracle: float within 4 x the restatement's distance, double 1e-10; the magnitude
    error against the truth is the oracle's."""
    S, masks, t, y = case(H, W, C)
    kw = dict(transform=transform, levels=levels) if transform else {}
    got, info = solve(kind, y, masks, precision, coils=S, **kw)
    assert got.dtype == C128 and got.shape == (B, H, W) and info['image'] == 'complex'
    assert len(info['cg_residual']) == B and all(0 < r < 1e-5 for r in info['cg_residual']), info['cg_residual']
    for b, (ref, d32) in enumerate(loop_refs(H, W, C, kind, transform, levels)):
        bar = 1e-10 if precision == 'f64' else 4 * d32
        err = rel_l2(got[b], ref)
        print('%s %s %dx%d %s slice %d: %.2e (bar %.2e)  magnitude error %.4f' % (kind, precision, H, W, transform, b, err, bar, X.mag_err(got[b], t[b])))
        assert err <= bar, (b, err, bar)
        assert abs(X.mag_err(got[b], t[b]) - X.mag_err(ref, t[b])) <= 1e-4


def test_metrics_are_taken_on_the_modulus_and_the_tensor_is_complex():
    """images= with image='complex': PSNR / RE of |x|; return_device=True: one complex tensor with the same bits"""
    import torch
    import pnp_admm_cnc_mri_amd as P
    H, W, C = SHAPES[0]
    S, masks, t, y = case(H, W, C)
    gt = np.round(np.abs(t) * 255).astype(np.uint8)
    kw = dict(y=y, mask_id=MID, coils=S, image='complex', iter_num=10, **M.O_PRESETS['cnc'])
    out, info = P.ADMM_CNC(masks, None, images=gt, return_info=True, **kw)
    xt = P.ADMM_CNC(masks, None, return_device=True, **kw)
    assert torch.is_tensor(xt) and xt.dtype == torch.complex64 and xt.shape == (B, H, W)
    for b in range(B):
        assert np.array_equal(xt[b].cpu().numpy().astype(C128), out[b])
        re = np.linalg.norm(np.abs(out[b]) * 255 - gt[b]) / np.linalg.norm(gt[b].astype(np.float64))
        assert abs(info['re'][b] - re) <= 0.02 * re and 10 < info['psnr'][b] < 40 and 0 < info['ssim'][b] < 1, (b, info['re'][b], re)


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_with_estimated_espirit_maps(kind):
    """coils='estimate', maps_method='espirit', image='complex' against the oracle fed the SAME maps (coilmaps.estimate's, which the
    solver calls with these settings)."""
    from pnp_admm_cnc_mri_amd import coilmaps
    H, W, C = 128, 130, 5
    S, masks, t, y = case(H, W, C, 24)
    got, info = solve(kind, y, masks, coils='estimate', maps_method='espirit')
    maps = coilmaps.estimate(y, masks, MID, method='espirit')
    assert info['coil_maps']['method'] == 'espirit' and info['image'] == 'complex' and maps.shape == (B, C, H, W)
    for b in range(B):
        Sb = np.asarray(maps[b]).astype(C128)
        f = lambda dt: X.admm(y[b].astype(dt), Sb, masks[MID[b]], 10, kind, dt=dt)
        ref = f(C128)
        bar, err = 4 * X.rel(f(C64), ref), rel_l2(got[b], ref)
        print('%s espirit slice %d: %.2e (bar %.2e)' % (kind, b, err, bar))
        assert err <= bar, (b, err, bar)


# ---- 6. bit-equality: batch and Bmax, run to run, host and device y; phase equivariance ------------------------------------------------

def run_cnc(eng, iters=10):
    eng.init_state()
    eng.admm_cnc(iters, **M.O_PRESETS['cnc'])
    return eng.x()


@pytest.mark.parametrize('H,W,C,wavelet', [(131, 128, 8, None), (128, 128, 5, 'db2')])
def test_bit_equal_alone_again_and_from_a_device_y(H, W, C, wavelet):
    import torch
    import pnp_admm_cnc_mri_amd as P
    S, masks, t, y = case(H, W, C)
    with open_engine(H, W, C, upload=False) as eng:
        if wavelet:
            eng.set_sparsity(wavelet, 3)
        eng.upload(y, masks, MID)
        batch = run_cnc(eng)
        again = run_cnc(eng)
        # the same problem from device tensors, through the ABI
        yd, md, idd = dev(y), torch.from_numpy(masks.copy()).to('cuda'), torch.from_numpy(MID.copy()).to('cuda')
        P._lib.check(eng._L.pnp_upload_problem_mc(eng._ctx, ctypes.c_void_p(yd.data_ptr()), ctypes.c_void_p(md.data_ptr()),
                                                  ctypes.c_void_p(idd.data_ptr()), None, B, 2, 1))
        from_dev = run_cnc(eng)
    assert np.array_equal(batch, again) and np.array_equal(batch, from_dev)
    with P.Engine(H, W, Bmax=2) as eng:                       # slice 1 alone, on a context of another Bmax
        eng.set_coils(S)
        eng.set_image_mode('complex')
        if wavelet:
            eng.set_sparsity(wavelet, 3)
        eng.upload(y[1:2], masks, MID[1:2])
        alone = run_cnc(eng)
    assert np.array_equal(alone[0], batch[1])


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_phase_equivariance_on_the_card(kind):
    """y e^{i theta} -> x e^{i theta} inside the float bar (y e^{i theta} is rounded to complex64 again, which the bar covers)"""
    H, W, C = SHAPES[1]
    S, masks, t, y = case(H, W, C)
    th = np.exp(0.7j)
    a, _ = solve(kind, y, masks, coils=S)
    b, _ = solve(kind, (y * th).astype(C64), masks, coils=S)
    for s, (ref, d32) in enumerate(loop_refs(H, W, C, kind, None, 0)):
        err = rel_l2(b[s], a[s] * th)
        print('%s slice %d: %.2e (bar %.2e)' % (kind, s, err, 4 * d32))
        assert err <= 4 * d32, (s, err, d32)


# ---- 7. the default path is what it was ---------------------------------------------------------------------------------------------------

def test_real_mode_is_bit_equal_around_a_complex_solve():
    """On ONE engine: a single-coil 256 x 256 solve on the fused path, a coil solve and a wavelet coil solve in real mode; then complex
    solves; then pnp_set_image(REAL) and the same real solves: same bits, same pnp_path_name.  Clearing the coils returns to real mode."""
    import pnp_admm_cnc_mri_amd as P
    H = W = 256
    C = 3
    S, masks, t, y = case(H, W, C)
    y1 = np.stack([np.fft.fft2(np.abs(t[b])) * masks[MID[b]] for b in range(B)]).astype(C64)

    def single_solve(eng):
        eng.set_coils(None)
        assert eng.image_mode == 'real'
        eng.upload(y1, masks, MID)
        eng.init_state()
        eng.admm_cnc(5, **M.O_PRESETS['cnc'])
        return {'single': (eng.path_name, eng.x())}

    def coil_solves(eng):
        """on an engine that has its coils and is in real mode"""
        res = {}
        assert eng.image_mode == 'real' and eng.C == C
        eng.upload(y, masks, MID)
        eng.init_state()
        eng.admm_l1(5, **M.O_PRESETS['l1'])
        res['coil'] = (eng.path_name, eng.x())
        eng.set_sparsity('db2', 3)
        eng.init_state()
        eng.admm_cnc(5, **M.O_PRESETS['cnc'])
        res['wavelet'] = (eng.path_name, eng.x())
        eng.set_sparsity(None)
        return res

    def real_solves(eng):
        res = single_solve(eng)
        eng.set_coils(S)
        res.update(coil_solves(eng))
        return res

    with P.Engine(H, W, Bmax=BMAX) as eng:
        before = real_solves(eng)
        assert [before[k][0] for k in ('single', 'coil', 'wavelet')] == ['fused', 'coils', 'coils']
        eng.set_image_mode('complex')
        with pytest.raises(P._lib.PnpError, match='no problem uploaded'):       # the call drops the uploaded problem
            eng.init_state()
        eng.upload(y, masks, MID)
        xc = run_cnc(eng, 5)
        eng.set_sparsity('db2', 3)
        xw = run_cnc(eng, 5)
        eng.set_sparsity(None)
        assert eng.path_name == 'coils' and xc.dtype == C64 and np.abs(xc.imag).max() > 0.01 and not np.array_equal(xc, xw)
        eng.set_image_mode('real')                                 # the same coils, the same context: all three solves, directly
        direct = coil_solves(eng)
        direct.update(single_solve(eng))
        eng.set_coils(S)
        eng.set_image_mode('complex')
        after = real_solves(eng)                                   # set_coils(None) inside: back to real mode
    for k in before:
        for res in (direct, after):
            assert res[k][0] == before[k][0] and np.array_equal(res[k][1], before[k][1]) and res[k][1].dtype == np.float32, k


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------

def test_state_refusals():
    import torch
    import pnp_admm_cnc_mri_amd as P
    H, W, C = SHAPES[0]
    S, masks, t, y = case(H, W, C)

    def refused(rc, *words):
        msg = L.pnp_last_error().decode()
        assert rc == -3 and all(wd in msg for wd in words), (rc, msg)

    for precision, sfx in (('f32', ''), ('f64', '_f64')):
        with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
            L, ctx = eng._L, eng._ctx
            fn = lambda name: getattr(L, name + sfx)
            # the rules of pnp_set_image, in order
            assert L.pnp_set_image(ctx, 7) == -1 and 'PNP_IMAGE_COMPLEX' in L.pnp_last_error().decode()
            refused(L.pnp_set_image(ctx, 1), 'pnp_set_coils')
            assert L.pnp_set_image(ctx, 0) == 0
            buf = torch.zeros((B, H, W), dtype=tdt(precision), device='cuda')
            p = ctypes.c_void_p(buf.data_ptr())
            eng.set_coils(S)
            eng.upload(y, masks, MID)
            for name in ('pnp_set_state_cx', 'pnp_get_state_cx'):                   # the _cx calls need the mode
                refused(fn(name)(ctx, p, p, 1), 'pnp_set_image')
            refused(fn('pnp_download_x_cx')(ctx, p, 1), 'pnp_set_image')
            refused(fn('pnp_dc_step_cx')(ctx, p, p, p, 0.05), 'pnp_set_image')
            refused(fn('pnp_prox_l1_dual_cx')(ctx, p, p, p, 0.1), 'pnp_set_image')
            refused(fn('pnp_prox_cnc_dual_cx')(ctx, p, p, p, 0.45, 0.5, 0.05, 64.0), 'pnp_set_image')
            if precision == 'f32':
                refused(L.pnp_A_cx(ctx, p, p), 'pnp_set_image')
            eng.set_sparsity('db2', 3)
            eng.set_spin(np.array([[1, 2], [0, 3]]))
            refused(L.pnp_set_image(ctx, 1), 'spin')
            eng.set_spin(None)
            eng.set_image_mode('complex')
            eng.upload(y, masks, MID)
            eng.init_state()
            eng.admm_l1(1, **M.O_PRESETS['l1'])
            # the real calls name their _cx counterpart
            refused(fn('pnp_set_state')(ctx, p, p, 1), 'pnp_set_state_cx' + sfx)
            refused(fn('pnp_get_state')(ctx, p, p, 1), 'pnp_get_state_cx' + sfx)
            refused(fn('pnp_download_x')(ctx, p, 1), 'pnp_download_x_cx' + sfx)
            refused(L.pnp_dc_step(ctx, p, p, p, 0.05), 'pnp_dc_step_cx')
            refused(L.pnp_prox_l1_dual(ctx, p, p, p, 0.1), 'pnp_prox_l1_dual_cx')
            refused(L.pnp_prox_cnc_dual(ctx, p, p, p, 0.45, 0.5, 0.05, 64.0), 'pnp_prox_cnc_dual_cx')
            # not available in complex mode
            n1, n2 = ctypes.c_int(0), ctypes.c_int(0)
            refused(L.pnp_admm_l1_run_traced(ctx, 2, 0.1, 0.015, 1, 0.0, None, 0, ctypes.byref(n1), ctypes.byref(n2)), 'not available in complex')
            refused(L.pnp_admm_cnc_run_traced(ctx, 2, 0.45, 0.5, 0.05, 64.0, 1, 0.0, None, 0, ctypes.byref(n1), ctypes.byref(n2)), 'not available in complex')
            refused(fn('pnp_residuals')(ctx, p, p, p, p, None, 0, 0, p, 1), 'not available in complex')
            tab = (ctypes.c_int32 * 4)(1, 2, 0, 3)
            refused(L.pnp_set_spin(ctx, tab, 2, 1), 'not available in complex')
            with pytest.raises(P._lib.PnpError, match='not available in complex'):
                eng.admm_cnc(2, trace_every=1, **M.O_PRESETS['cnc'])
            # every complex array of a step-wise call is aligned to one complex value; the pixel prox to 16 bytes
            off = ctypes.c_void_p(buf.data_ptr() + (8 if precision == 'f64' else 4))
            assert fn('pnp_dc_step_cx')(ctx, off, p, p, 0.05) == -1 and 'aligned' in L.pnp_last_error().decode()
            assert fn('pnp_prox_l1_dual_cx')(ctx, p, off, p, 0.1) == -1 and 'aligned' in L.pnp_last_error().decode()
            if precision == 'f32':
                assert L.pnp_A_cx(ctx, off, p) == -1 and 'aligned' in L.pnp_last_error().decode()
                eng.set_sparsity(None)
                off8 = ctypes.c_void_p(buf.data_ptr() + 8)
                assert L.pnp_prox_l1_dual_cx(ctx, p, p, off8, 0.1) == -1 and '16-byte' in L.pnp_last_error().decode()
                eng.set_sparsity('db2', 3)
            # db4 with 4 levels does not fit the LDS on complex doubles: PNP_E_ARG from whichever call comes second
            rc = L.pnp_set_sparsity(ctx, 3, 4)
            assert rc == (-1 if precision == 'f64' else 0), L.pnp_last_error().decode()
            eng.set_image_mode('real')
            eng.set_sparsity('db4', 4)
            assert L.pnp_set_image(ctx, 1) == (-1 if precision == 'f64' else 0)
            eng.set_coils(None)
            assert eng.image_mode == 'real'
        assert L.pnp_image_check(1, 3, 4, 1 if precision == 'f64' else 0) == (-1 if precision == 'f64' else 0)
    with pytest.raises(ValueError, match='does not fit the LDS'):                 # the solvers refuse it before an engine is opened
        P.ADMM_CNC(masks, None, y=y, mask_id=MID, coils=S, image='complex', precision='f64', transform='db4', levels=4, iter_num=1)
