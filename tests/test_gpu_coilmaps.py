"""Coil map estimation on the GPU (pnp_coil_maps, coilmaps.estimate, coils='estimate' on the solvers) against tests/coilmaps_oracle.py and
tests/multicoil_oracle.py.

Shapes: the smallest that still exercise every branch -- 128 x 128, 131 x 128 and 140 x 160 (Bluestein and mixed-radix lengths, an odd H,
tile remainders on both axes); (C, radius, power_iters) = (1, 0, 1), (2, 1, 2), (5, 2, 4), (8, 3, 4), (32, 1, 4), (32, 3, 2): every
register bucket but the one of 16, for which (16, 2, 2) is added, and every tile (16 x 16 down to the 128 KiB fall-back of C = 32 in
double at radius 3); ncal 4, 5 and 24; B = 3 with a bank of two masks and mask_id = [1, 0, 1]; contexts of Bmax = 7, so that the
transform runs in ragged chunks and, from C = 5 on, one slice per pass.
Float bars: 4 x the distance of the oracle's own complex64 restatement from its float64 form on the same inputs (computed here, per case,
over the case's three slices); double: 1e-12.  Pixels within 1e-3 of the support's threshold in the oracle are left out of the
comparison (at most 0.1 % of a slice); everywhere else the support agrees exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import coilmaps_oracle as CM
import coilmix_oracle as CO
import multicoil_oracle as M
from conftest import rel_l2, weights_trained

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
B = 3
MID = np.array([1, 0, 1], np.int32)
THRESH = 0.05
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
#        C, r, n,  H,   W,  ncal
CASES = [(1, 0, 1, 128, 128, 4), (2, 1, 2, 131, 128, 5), (5, 2, 4, 140, 160, 24), (8, 3, 4, 131, 128, 24), (32, 1, 4, 128, 128, 5),
         (32, 3, 2, 140, 160, 4), (16, 2, 2, 128, 128, 24)]


def cdt(precision):
    return C128 if precision == 'f64' else C64


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda')


@functools.lru_cache(maxsize=None)
def scene(Cn, H, W, ncal, shift=False):
    """-> (masks [2,H,W] with the calibration square, imgs [B,H,W], maps [B,C,H,W], y [B,C,H,W] complex128); shift: the body rolled by
    (H / 2, W / 2), so that it crosses the image edges"""
    masks = np.stack([(M.mask(H + k, H, W).astype(bool) | CO.cal_region(ncal, H, W)).astype(np.uint8) for k in range(2)])
    imgs = np.stack([M.phantom(10 * H + b, H, W) for b in range(B)])
    S = np.stack([M.coil_maps(Cn, H, W, b) for b in range(B)])
    if shift:
        imgs, S = np.roll(imgs, (H // 2, W // 2), axis=(1, 2)), np.roll(S, (H // 2, W // 2), axis=(2, 3))
    y = np.stack([M.synthesize(imgs[b], S[b], masks[MID[b]], M.noise(b, Cn, masks[MID[b]])) for b in range(B)])
    return masks, imgs, S, y


@functools.lru_cache(maxsize=None)
def oracle(Cn, r, n, H, W, ncal, shift=False):
    """the float64 oracle and its complex64 restatement of every slice: [(maps, lambda, support)], [(maps32, lambda32, support32)]"""
    masks, _, _, y = scene(Cn, H, W, ncal, shift)
    o64 = [CM.estimate(y[b], masks[MID[b]], ncal, r, n, THRESH, full=True)[:3] for b in range(B)]
    o32 = [CM.estimate(y[b].astype(C64), masks[MID[b]], ncal, r, n, THRESH, C64, full=True)[:3] for b in range(B)]
    return o64, o32


def raw_maps(y, masks, mid, ncal, r, n, precision, Bmax=7, thresh=THRESH, want_lambda=True, eng=None):
    """pnp_coil_maps[_f64] on device copies; -> (maps, lambda) host arrays, NaN-filled before the call"""
    import torch
    from pnp_admm_cnc_mri_amd import Engine
    y = np.ascontiguousarray(y, dtype=cdt(precision))
    nb, Cn, H, W = y.shape
    y_t, bank_t = dev(y), dev(np.ascontiguousarray(masks, dtype=np.uint8))
    mid_t = None if mid is None else dev(np.asarray(mid, np.int32))
    out = torch.full(y.shape, float('nan'), dtype=y_t.dtype, device='cuda')
    lam = torch.full((nb, H, W), float('nan'), dtype=out.real.dtype, device='cuda') if want_lambda else None
    torch.cuda.synchronize()
    own = eng is None
    eng = eng or Engine(H, W, Bmax=Bmax, precision=precision)
    try:
        eng.coil_maps(y_t, bank_t, mid_t, out, lam, nb, Cn, ncal, r, n, thresh)
    finally:
        if own:
            eng.close()
    return out.cpu().numpy(), None if lam is None else lam.cpu().numpy()


def compare(got, lam, o64, o32, precision, what):
    """the rules of the module docstring for one case of B slices"""
    num = den = lnum = lden = 0.0
    rows = []
    for b in range(B):
        S, l, sup = o64[b]
        near = np.abs(l / (THRESH ** 2 * l.max()) - 1) < 1e-3
        assert near.mean() <= 1e-3, (what, b, int(near.sum()))
        gsup = (got[b] != 0).any(0)
        assert np.array_equal(gsup[~near], sup[~near]), (what, b, int((gsup != sup)[~near].sum()))
        assert np.isfinite(got[b]).all() and np.isfinite(lam[b]).all()
        both = gsup & sup & ~near
        rows.append((b, M.rel(got[b][:, both], S[:, both]), M.rel(lam[b], l)))
        S32, l32, sup32 = o32[b]
        b32 = sup32 & sup & ~near
        num, den = num + np.sum(np.abs(S32[:, b32] - S[:, b32]) ** 2), den + np.sum(np.abs(S[:, b32]) ** 2)
        lnum, lden = lnum + np.sum((l32.astype(np.float64) - l) ** 2), lden + np.sum(l ** 2)
    bar, lbar = (4 * np.sqrt(num / den), 4 * np.sqrt(lnum / lden)) if precision == 'f32' else (1e-12, 1e-12)
    worst = max(r[1] for r in rows), max(r[2] for r in rows)
    print('%s %s: maps worst slice %.2e (bar %.2e), lambda %.2e (bar %.2e)' % (what, precision, worst[0], bar, worst[1], lbar))
    for b, err, lerr in rows:
        assert err <= bar, (what, b, err, bar)
        assert lerr <= lbar, (what, b, lerr, lbar)


# ---- 1. pnp_coil_maps against the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,r,n,H,W,ncal', CASES)
def test_coil_maps_against_the_oracle(Cn, r, n, H, W, ncal, precision):
    """Measured on an MI355X (worst slice, maps / lambda; float bar = 4 x the complex64 restatement): see DESIGN.md section 17."""
    masks, _, _, y = scene(Cn, H, W, ncal)
    o64, o32 = oracle(Cn, r, n, H, W, ncal)
    got, lam = raw_maps(y, masks, MID, ncal, r, n, precision)
    compare(got, lam, o64, o32, precision, 'C=%d r=%d n=%d %dx%d ncal=%d' % (Cn, r, n, H, W, ncal))


def test_coil_maps_on_a_fixed_size_double_context():
    """256 x 256 in double: the calibration's inverse transform is the one double entry point that runs the fixed-size row kernel with a
    complex input and a complex output (k_rows<256, IN_COMPLEX, inverse, EPI_COMPLEX, double>, then the Stockham k_cols<256, double>);
    every other shape of this file is an any-size one.  The rules and the double bar (1e-12) of the cases above."""
    from pnp_admm_cnc_mri_amd import Engine
    Cn, r, n, H, W, ncal = 2, 1, 2, 256, 256, 5
    masks, _, _, y = scene(Cn, H, W, ncal)
    o64, o32 = oracle(Cn, r, n, H, W, ncal)
    with Engine(H, W, Bmax=7, precision='f64') as eng:
        assert eng.ctx_path != 'anysize' and eng.fft_plan(0) == 'fixed 256' and eng.fft_plan(1) == 'fixed 256'
        got, lam = raw_maps(y, masks, MID, ncal, r, n, 'f64', eng=eng)
    compare(got, lam, o64, o32, 'f64', 'C=%d r=%d n=%d %dx%d ncal=%d (fixed-size kernels)' % (Cn, r, n, H, W, ncal))


# ---- 2. exact statements ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,r,n,H,W,ncal', [CASES[0], CASES[2], CASES[3], CASES[5]])
def test_exact_statements(Cn, r, n, H, W, ncal, precision):
    """Outside the support every entry is +0.0 to the bit; inside, sum_c |S_c|^2 is within 4 C ulp of 1; a slice alone (on a context of
    another Bmax, with a null mask_id, without lambda_out) is bit-equal to the slice in the batch; two runs are bit-equal."""
    masks, _, _, y = scene(Cn, H, W, ncal)
    got, lam = raw_maps(y, masks, MID, ncal, r, n, precision)
    again, lam2 = raw_maps(y, masks, MID, ncal, r, n, precision)
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8)) and np.array_equal(lam.view(np.uint8), lam2.view(np.uint8))
    for b in range(B):
        sup = (got[b] != 0).any(0)
        assert 0 < sup.sum() < sup.size
        assert not np.ascontiguousarray(got[b][:, ~sup]).view(np.uint8).any(), b      # +0.0 exactly, no -0.0
        g = got[b].astype(np.clongdouble)                                        # measured in extended precision: float64 sums would add an ulp of their own
        n2 = (g.real ** 2 + g.imag ** 2).sum(0)[sup]
        off = float(np.abs(n2 - 1).max() / EPS[precision])
        print('C=%d %s slice %d: |sum |S|^2 - 1| <= %.2f ulp (bar %d)' % (Cn, precision, b, off, 4 * Cn))
        assert off <= 4 * Cn, (b, off)
        assert (lam[b] >= 0).all() and np.array_equal(sup, lam[b] >= lam[b].dtype.type(THRESH * THRESH) * lam[b].max())
    alone, _ = raw_maps(y[1:2], masks[MID[1]][None], None, ncal, r, n, precision, Bmax=64, want_lambda=False)
    assert np.array_equal(alone[0].view(np.uint8), got[1].view(np.uint8))


@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_wrapper_on_host_arrays_and_device_tensors(precision):
    """coilmaps.estimate: a host y walked one slice at a time equals the walk in one piece, a device tensor gives device tensors, an engine
    of the caller's gives the same -- all bit for bit, and equal to the raw call."""
    import torch
    from pnp_admm_cnc_mri_amd import Engine, coilmaps, utils_pnp as U
    Cn, r, n, H, W, ncal = CASES[2]
    masks, _, _, y = scene(Cn, H, W, ncal)
    raw, raw_lam = raw_maps(y, masks, MID, ncal, r, n, precision)
    kw = dict(calib=ncal, radius=r, power_iters=n, thresh=THRESH, precision=precision)
    whole, lam = coilmaps.estimate(y, masks, MID, return_lambda=True, **kw)
    pieces = coilmaps.estimate(y, masks, MID, chunk_bytes=1, **kw)
    assert isinstance(whole, np.ndarray) and whole.dtype == cdt(precision) and whole.shape == y.shape and lam.shape == (B, H, W)
    assert np.array_equal(whole.view(np.uint8), raw.view(np.uint8)) and np.array_equal(lam.view(np.uint8), raw_lam.view(np.uint8))
    assert np.array_equal(whole.view(np.uint8), pieces.view(np.uint8))
    on_dev = U.estimate_coil_maps(dev(y.astype(cdt(precision))), masks, MID, **kw)
    assert torch.is_tensor(on_dev) and np.array_equal(on_dev.cpu().numpy().view(np.uint8), raw.view(np.uint8))
    with Engine(H, W, Bmax=B, precision=precision) as eng:
        mine = coilmaps.estimate(y, masks, MID, engine=eng, **kw)
    assert np.array_equal(mine.view(np.uint8), raw.view(np.uint8))
    share = coilmaps.support_share(whole)
    assert share == coilmaps.support_share(on_dev) and all(0.2 < s < 0.9 for s in share)
    if precision == 'f32':
        with pytest.raises(ValueError, match='complex type'):
            coilmaps.estimate(dev(y), masks, MID, **kw)                          # a complex128 tensor on the float path


# ---- 3. borders --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,r,n,H,W,ncal', [(5, 2, 4, 131, 128, 24), (8, 3, 4, 140, 160, 24)])
def test_a_body_across_the_image_edges(Cn, r, n, H, W, ncal, precision):
    """The phantom and its maps rolled by (H / 2, W / 2): the body and the support cross all four edges, where the halo's wrap indexing is
    what is read.  The same bars."""
    masks, imgs, _, y = scene(Cn, H, W, ncal, True)
    o64, o32 = oracle(Cn, r, n, H, W, ncal, True)
    assert all(o64[b][2][0].any() and o64[b][2][-1].any() and o64[b][2][:, 0].any() and o64[b][2][:, -1].any() for b in range(B))
    got, lam = raw_maps(y, masks, MID, ncal, r, n, precision)
    compare(got, lam, o64, o32, precision, 'rolled C=%d r=%d %dx%d' % (Cn, r, H, W))


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------------

def test_a_hole_in_the_calibration_region_and_overlapping_arrays_are_arg_errors():
    import torch
    from pnp_admm_cnc_mri_amd import Engine
    from pnp_admm_cnc_mri_amd._lib import PnpError
    Cn, r, n, H, W, ncal = CASES[1]
    masks, _, _, y = scene(Cn, H, W, ncal)
    bad = masks.copy()
    bad[1, H - 1, 2] = 0                                                         # mask 1 serves slices 0 and 2
    bad[1, H - 2, 1] = 0
    with pytest.raises(PnpError) as e:
        raw_maps(y, bad, MID, ncal, r, n, 'f32')
    assert e.value.code == -1 and 'slice 0' in str(e.value) and '(%d, 1)' % (H - 2) in str(e.value), str(e.value)
    with pytest.raises(PnpError) as e:
        raw_maps(y[1:], bad, MID[1:], ncal, r, n, 'f64')
    assert e.value.code == -1 and 'slice 1' in str(e.value) and '(%d, 1)' % (H - 2) in str(e.value), str(e.value)
    buf = torch.zeros((2 * B, Cn, H, W), dtype=torch.complex64, device='cuda')
    bank_t = dev(masks)
    with Engine(H, W, Bmax=7) as eng:
        for out in (buf[:B], buf[1:B + 1], buf[B - 1:2 * B - 1]):
            with pytest.raises(PnpError) as e:
                eng.coil_maps(buf[:B], bank_t, None, out, None, B, Cn, ncal, r, n, THRESH)
            assert e.value.code == -1 and 'overlap' in str(e.value)
        eng.coil_maps(buf[:B], bank_t, None, buf[B:], None, B, Cn, ncal, r, n, THRESH)          # adjacent is fine (all-zero data: e_0, lambda = 0)
        with pytest.raises(PnpError) as e:
            eng.coil_maps(buf[:B], bank_t, None, buf[B:], None, B, Cn, 3, r, n, THRESH)
        assert e.value.code == -1 and 'ncal must be' in str(e.value)
    torch.cuda.synchronize()
    zero = buf[B:].cpu().numpy()
    assert (zero[:, 0] == 1).all() and not zero[:, 1:].any()                      # lambda = 0 >= 0: every pixel is kept, with v = e_0
    with Engine(H, W, Bmax=7, precision='f64') as eng:                            # the precision of the entry point is the context's
        rc = eng._L.pnp_coil_maps(eng._ctx, C.c_void_p(buf.data_ptr()), C.c_void_p(bank_t.data_ptr()), None, C.c_void_p(buf[B:].data_ptr()),
                                  None, B, Cn, ncal, r, n, THRESH)
        assert rc == -3 and 'fp64' in eng._L.pnp_last_error().decode()


# ---- 5. end to end: ten iterations at the presets, 128 x 130, B = 3, C = 5 -----------------------------------------------------------------------

H5, W5, C5 = 128, 130, 5


def psnr(x, img):
    return float(10 * np.log10(1.0 / np.mean((np.asarray(x, np.float64) - img) ** 2)))


def solve(kind, y, masks, precision='f32', **kw):
    import pnp_admm_cnc_mri_amd as P
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    out, info = solver(masks, None, y=y, mask_id=MID, precision=precision, return_info=True, iter_num=10, **kw, **M.O_PRESETS[kind])
    return np.stack(out[:B]), info


@functools.lru_cache(maxsize=None)
def oracle_solves(kind):
    """per slice: the float64 oracle's solve with the ORACLE's estimated maps, its float32 restatement's distance from it (estimate and
    solve in complex64), and the PSNR of the oracle's solve with the TRUE maps"""
    masks, imgs, S, y = scene(C5, H5, W5, 24)
    rows = []
    for b in range(B):
        m = masks[MID[b]]
        ref = M.admm(y[b], CM.estimate(y[b], m), m, 10, kind)
        y32 = y[b].astype(C64)
        r32 = M.admm(y32, CM.estimate(y32, m, dt=C64), m, 10, kind, dt=C64)
        rows.append((ref, M.rel(r32, ref), psnr(M.admm(y[b], S[b], m, 10, kind), imgs[b])))
    return rows


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_solvers_with_estimated_maps(kind, precision):
    """coils='estimate' against the oracle's ADMM run with the oracle's estimated maps: within 4 x the float32 restatement's distance of
    that whole pipeline (double: 1e-10); the PSNR is no lower than the oracle's with the TRUE maps minus 0.1 dB."""
    masks, imgs, S, y = scene(C5, H5, W5, 24)
    got, info = solve(kind, y, masks, precision, coils='estimate', images=imgs)
    cm = info['coil_maps']
    assert (cm['calib'], cm['radius'], cm['power_iters'], cm['thresh']) == (24, 2, 4, 0.05) and len(cm['support']) == B
    assert all(0.3 < s < 0.7 for s in cm['support']) and len(info['cg_residual']) == B
    for b, (ref, d32, psnr_true) in enumerate(oracle_solves(kind)):
        bar = 4 * d32 if precision == 'f32' else 1e-10
        err, p = rel_l2(got[b], ref), psnr(got[b], imgs[b])
        print('%s %s slice %d: %.2e (bar %.2e); PSNR %.2f dB, with the true maps %.2f dB' % (kind, precision, b, err, bar, p, psnr_true))
        assert err <= bar, (b, err, bar)
        assert p >= psnr_true - 0.1, (b, p, psnr_true)


def test_pnp_with_estimated_maps_equals_the_call_with_those_maps():
    """PNP_ADMM_L1_D with coils='estimate' equals, bit for bit, the same call given coilmaps.estimate's output as coils= with
    coil_id = arange(B); the options dict swallows unknown keywords, so the arguments must not be among them."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import coilmaps
    Hn = Wn = 128
    masks, imgs, S, y = scene(4, Hn, Wn, 16)
    kw = dict(model=weights_trained(), iter_num=3, reo=0.25, mask_id=MID)
    got, info = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y, coils='estimate', calib=16, maps_radius=1, maps_power_iters=3, maps_thresh=0.1,
                                return_info=True, **kw)
    assert info['coil_maps']['radius'] == 1 and info['coil_maps']['power_iters'] == 3 and info['coil_maps']['thresh'] == 0.1
    maps = coilmaps.estimate(y, masks, MID, calib=16, radius=1, power_iters=3, thresh=0.1)
    want = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y, coils=maps, coil_id=np.arange(B), **kw)
    other = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y, coils='estimate', calib=16, **kw)          # the defaults: other maps
    for b in range(B):
        assert np.array_equal(np.asarray(got[b]), np.asarray(want[b])), b
        assert rel_l2(other[b], got[b]) > 1e-6, b


# ---- 6. with mixing ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_40_channels_of_rank_4_with_estimated_maps(kind):
    """40 physical channels spanning a 4-dimensional map space, virtual_coils = 4, coils='estimate': y is mixed by ONE matrix from the Gram
    matrices of the whole batch, the maps are estimated from the mixed y.  Equals the oracle pipeline (mix with the M the solver returned,
    estimate, solve) at the bars of the end-to-end test."""
    masks, imgs, _, _ = scene(C5, H5, W5, 24)
    S = CO.rank4_maps(40, H5, W5, 4)
    y = np.stack([M.synthesize(imgs[b], S, masks[MID[b]], M.noise(b, 40, masks[MID[b]])) for b in range(B)])
    got, info = solve(kind, y, masks, coils='estimate', virtual_coils=4, images=imgs)
    Mx = info['coil_mix']['M']
    assert Mx.shape == (4, 40) and info['coil_mix']['energy'] > 0.99 and np.abs(Mx @ Mx.conj().T - np.eye(4)).max() <= 1e-12
    assert len(info['coil_maps']['support']) == B
    for b in range(B):
        m = masks[MID[b]]
        y2 = CO.mix(y[b], Mx)
        ref = M.admm(y2, CM.estimate(y2, m), m, 10, kind)
        y32 = CO.mix(y[b].astype(C64), Mx, C64)
        bar = 4 * M.rel(M.admm(y32, CM.estimate(y32, m, dt=C64), m, 10, kind, dt=C64), ref)
        err = rel_l2(got[b], ref)
        print('rank 4 of 40, estimated maps, %s slice %d: %.2e (bar %.2e), PSNR %.2f dB' % (kind, b, err, bar, psnr(got[b], imgs[b])))
        assert err <= bar, (b, err, bar)


# ---- 7. defaults untouched --------------------------------------------------------------------------------------------------------------------

def test_an_estimate_on_an_engine_leaves_no_state_behind():
    """A single-coil solve (256 x 256, the fused path) and a coils=array solve (128 x 130) give the same bits and the same path before and
    after coilmaps.estimate ran on the same engine, between the runs and on the uploaded problem."""
    from pnp_admm_cnc_mri_amd import Engine, coilmaps
    rng = np.random.default_rng(7)
    par = M.O_PRESETS['cnc']

    def run(eng, upload):
        upload()
        eng.init_state()
        eng.admm_cnc(5, par['alpha'], par['lambda1'], par['reo'], par['b'])
        return eng.x().copy(), eng.path_name, eng.ctx_path

    Hn = Wn = 256
    m1 = (M.mask(3, Hn, Wn).astype(bool) | CO.cal_region(24, Hn, Wn)).astype(np.uint8)
    img = M.phantom(3, Hn, Wn)
    y1 = np.stack([np.fft.fft2(img) * m1, np.fft.fft2(img[::-1]) * m1]).astype(C64)
    ymc = (rng.standard_normal((2, 4, Hn, Wn)) + 1j * rng.standard_normal((2, 4, Hn, Wn))).astype(C64)
    with Engine(Hn, Wn, Bmax=2) as eng:
        before = run(eng, lambda: eng.upload(y1, m1))
        first = coilmaps.estimate(ymc, m1, engine=eng)
        middle = run(eng, lambda: eng.upload(y1, m1))
        eng.upload(y1, m1)
        eng.init_state()
        second = coilmaps.estimate(ymc, m1, engine=eng)                         # between init_state and the loop
        eng.admm_cnc(5, par['alpha'], par['lambda1'], par['reo'], par['b'])
        after = (eng.x().copy(), eng.path_name, eng.ctx_path)
    assert before[1:] == middle[1:] == after[1:]
    assert np.array_equal(before[0], middle[0]) and np.array_equal(before[0], after[0]) and np.array_equal(first, second)

    masks, imgs, S, y = scene(C5, H5, W5, 24)
    with Engine(H5, W5, Bmax=B) as eng:
        eng.set_coils(S[0])
        up = lambda: eng.upload(y, masks, MID)
        before = run(eng, up)
        est = coilmaps.estimate(y, masks, MID, engine=eng)
        after = run(eng, up)
        assert eng.coils['C'] == C5 and eng.coils['Ks'] == 1
    assert before[1:] == after[1:] and np.array_equal(before[0], after[0])
    assert np.array_equal(est, coilmaps.estimate(y, masks, MID))
