"""ESPIRiT coil map estimation on the GPU (pnp_calib_patch_gram, pnp_espirit_eigmaps, pnp_espirit_maps, coilmaps.estimate(method='espirit'),
maps_method='espirit' on the solvers) against tests/espirit_oracle.py and tests/multicoil_oracle.py.

Cases (C, k, n, H, W, ncal): (1, 2, 1, 128, 128, 4), (2, 8, 2, 131, 128, 16), (5, 5, 4, 140, 160, 32), (8, 4, 8, 128, 130, 24),
(8, 3, 16, 131, 128, 16), (32, 2, 4, 128, 128, 5): every register bucket, the smallest and the largest kernel, the 128-column limit of the
host eigen-solver, Bluestein and mixed-radix lengths, tile remainders on both axes, the 8 x 8 tile of C = 32 (16 x 16 elsewhere) and the
opt-in to more than 64 KiB of LDS (C = 32 in double); B = 3 with a bank of two masks and mask_id = [1, 0, 1]; contexts of Bmax = 7, so that
the transform runs in ragged chunks and, from C = 5 on, one slice per pass.  One more case with the phantom rolled by (H / 2, W / 2).
Bars.  Patch Gram: 1e-13 of its norm (double sums of at most 3 721 terms).  Per-pixel stage fed the oracle's w and images: float 4 x the
distance of the oracle's complex64 restatement from its float64 form on the same case, double 1e-12.  End to end: the larger of that and
16 x the oracle's own sensitivity to the Gram matrix's rounding -- the distance between its maps from the Gram matrix summed in forward and
in reverse patch order -- given that no singular value lies within 1e-6 relative of the cut (asserted).  Support: pixels with lambda
within 1e-5 of crop or ||I|| within 1e-5 relative of its threshold in the oracle are left out (at most 0.1 % of a slice); everywhere else
the support agrees exactly.  Maps and lambda are compared on the common support: outside it the low-resolution image is below 5 % of its
largest value, its relative rounding error is unbounded there, and with it that of the start vector and of lambda."""
import ctypes as C
import functools

import numpy as np
import pytest

import coilmaps_oracle as CM
import coilmix_oracle as CO
import espirit_oracle as E
import multicoil_oracle as M
from conftest import rel_l2, weights_trained

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
B = 3
MID = np.array([1, 0, 1], np.int32)
SIGMA, CROP, THRESH = 0.02, 0.9, 0.05
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
#        C, k, n,  H,   W,  ncal
CASES = [(1, 2, 1, 128, 128, 4), (2, 8, 2, 131, 128, 16), (5, 5, 4, 140, 160, 32), (8, 4, 8, 128, 130, 24), (8, 3, 16, 131, 128, 16),
         (32, 2, 4, 128, 128, 5)]
ROLLED = (5, 4, 4, 131, 128, 24)


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
def oracle(Cn, k, n, H, W, ncal, shift=False):
    """per slice: the float64 oracle, its complex64 restatement (from y rounded to complex64), and the float64 oracle's unit vectors from the
    Gram matrix summed in reverse patch order"""
    masks, _, _, y = scene(Cn, H, W, ncal, shift)
    o64 = [E.estimate(y[b], masks[MID[b]], ncal, k, n, SIGMA, CROP, THRESH, full=True) for b in range(B)]
    o32 = [E.estimate(y[b].astype(C64), masks[MID[b]], ncal, k, n, SIGMA, CROP, THRESH, C64, full=True) for b in range(B)]
    rev = []
    for b in range(B):
        P, _, _ = E.signal_space(E.gram(y[b], masks[MID[b]], ncal, k, reverse=True), SIGMA)
        rev.append(E.eigmaps(o64[b]['I'], E.kernels(P, Cn, k), n)[0])
    for b in range(B):                                       # the cut must be clear of every singular value
        s = o64[b]['sing']
        assert np.min(np.abs(s / (SIGMA * s[0]) - 1)) > 1e-6, (b, s)
    return o64, o32, rev


def near_edges(o):
    """the pixels of one oracle slice that the support comparison leaves out"""
    return (np.abs(o['lam'] - CROP) < 1e-5) | (np.abs(o['inorm'] / (THRESH * o['inorm'].max()) - 1) < 1e-5)


def stage_bars(o64, o32, precision):
    """(maps, lambda): 4 x the complex64 restatement's distance over the case's slices on the common support; double: 1e-12"""
    if precision == 'f64':
        return 1e-12, 1e-12
    num = den = lnum = lden = 0.0
    for a, r in zip(o64, o32):
        both = a['sup'] & r['sup']
        num, den = num + np.sum(np.abs(r['v'][:, both] - a['v'][:, both]) ** 2), den + np.sum(np.abs(a['v'][:, both]) ** 2)
        lnum, lden = lnum + np.sum((r['lam'][both].astype(np.float64) - a['lam'][both]) ** 2), lden + np.sum(a['lam'][both] ** 2)
    return 4 * np.sqrt(num / den), 4 * np.sqrt(lnum / lden)


def engine(H, W, precision, Bmax=7):
    from pnp_admm_cnc_mri_amd import Engine
    return Engine(H, W, Bmax=Bmax, precision=precision)


def raw_maps(y, masks, mid, ncal, k, n, precision, Bmax=7, want_lambda=True, eng=None, sigma=SIGMA, crop=CROP, thresh=THRESH):
    """pnp_espirit_maps[_f64] on device copies; -> (maps, lambda, rank) host arrays, NaN-filled before the call"""
    import torch
    y = np.ascontiguousarray(y, dtype=cdt(precision))
    nb, Cn, H, W = y.shape
    y_t, bank_t = dev(y), dev(np.ascontiguousarray(masks, dtype=np.uint8))
    mid_t = None if mid is None else dev(np.asarray(mid, np.int32))
    out = torch.full(y.shape, float('nan'), dtype=y_t.dtype, device='cuda')
    lam = torch.full((nb, H, W), float('nan'), dtype=out.real.dtype, device='cuda') if want_lambda else None
    torch.cuda.synchronize()
    own = eng is None
    eng = eng or engine(H, W, precision, Bmax)
    try:
        rank = eng.espirit_maps(y_t, bank_t, mid_t, out, lam, nb, Cn, ncal, k, n, sigma, crop, thresh)
    finally:
        if own:
            eng.close()
    return out.cpu().numpy(), None if lam is None else lam.cpu().numpy(), rank


# ---- 1. the stages ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,k,n,H,W,ncal', CASES)
def test_patch_gram_against_the_oracle(Cn, k, n, H, W, ncal, precision):
    """pnp_calib_patch_gram: within 1e-13 of the oracle's A^H A in norm (the oracle gets the data as the kernel reads them: rounded to the
    input precision, summed in double); exactly Hermitian with +0 on the diagonal's imaginary part; a slice alone equals the slice in the
    batch; a point the mask does not sample enters as 0."""
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    masks, _, _, y = scene(Cn, H, W, ncal)
    yp = np.ascontiguousarray(y, dtype=cdt(precision))
    fn = L.pnp_calib_patch_gram_f64 if precision == 'f64' else L.pnp_calib_patch_gram
    N = Cn * k * k

    def run(yy, bank, mid):
        y_t, bank_t, mid_t = dev(yy), dev(bank), None if mid is None else dev(mid)
        g = torch.full((len(yy), N, N), float('nan'), dtype=torch.complex128, device='cuda')
        torch.cuda.synchronize()
        _lib.check(fn(None, C.c_void_p(y_t.data_ptr()), C.c_void_p(bank_t.data_ptr()), None if mid is None else C.c_void_p(mid_t.data_ptr()),
                      C.c_void_p(g.data_ptr()), len(yy), Cn, H, W, ncal, k))
        torch.cuda.synchronize()
        return g.cpu().numpy()

    got = run(yp, masks, MID)
    worst = 0.0
    for b in range(B):
        want = E.gram(yp[b].astype(C128), masks[MID[b]], ncal, k)
        worst = max(worst, M.rel(got[b], want))
        assert np.array_equal(got[b], np.conj(got[b].T)), b
        assert not np.ascontiguousarray(np.diagonal(got[b]).imag).view(np.uint8).any(), b          # +0.0, not -0.0
    print('C=%d k=%d %dx%d ncal=%d %s: patch Gram worst slice %.2e (bar 1e-13)' % (Cn, k, H, W, ncal, precision, worst))
    assert worst <= 1e-13
    alone = run(yp[1:2], masks[MID[1]][None], None)
    assert np.array_equal(alone[0].view(np.uint8), got[1].view(np.uint8))
    hole = masks.copy()
    hole[0, 0, 1] = 0                                        # DC's neighbour in mask 0: slice 1
    yz = yp.copy()
    yz[1, :, 0, 1] = 0
    assert np.array_equal(run(yp, hole, MID).view(np.uint8), run(yz, masks, MID).view(np.uint8))


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,k,n,H,W,ncal', CASES)
def test_eigmaps_fed_the_oracles_kernels_and_images(Cn, k, n, H, W, ncal, precision):
    """pnp_espirit_eigmaps alone on the oracle's w and low-resolution images (rounded to the precision): unit vectors and lambda on the
    common support.  Measured on an MI355X: see DESIGN.md section 19."""
    import torch
    o64, o32, _ = oracle(Cn, k, n, H, W, ncal)
    src = o64 if precision == 'f64' else o32
    dt = cdt(precision)
    img_t = dev(np.stack([o['I'] for o in src]).astype(dt))
    w_t = dev(np.stack([o['w'] for o in src]).astype(dt))
    out = torch.full((B, Cn, H, W), float('nan'), dtype=img_t.dtype, device='cuda')
    lam = torch.full((B, H, W), float('nan'), dtype=out.real.dtype, device='cuda')
    torch.cuda.synchronize()
    with engine(H, W, precision) as eng:
        eng.espirit_eigmaps(img_t, w_t, out, lam, B, Cn, k, n)
    got, lam = out.cpu().numpy(), lam.cpu().numpy()
    bar, lbar = stage_bars(o64, o32, precision)
    assert np.isfinite(got).all() and np.isfinite(lam).all()
    rows = []
    for b in range(B):
        both = o64[b]['sup'] & o32[b]['sup']
        rows.append((M.rel(got[b][:, both], o64[b]['v'][:, both]), M.rel(lam[b][both], o64[b]['lam'][both])))
    print('C=%d k=%d n=%d %dx%d %s: eigmaps worst slice %.2e (bar %.2e), lambda %.2e (bar %.2e)'
          % (Cn, k, n, H, W, precision, max(r[0] for r in rows), bar, max(r[1] for r in rows), lbar))
    for b, (err, lerr) in enumerate(rows):
        assert err <= bar, (b, err, bar)
        assert lerr <= lbar, (b, lerr, lbar)


def compare(got, lam, rank, o64, o32, rev, precision, what):
    """the end-to-end rules of the module docstring for one case of B slices"""
    bar, lbar = stage_bars(o64, o32, precision)
    sens = max(M.rel(rev[b][:, o64[b]['sup']], o64[b]['v'][:, o64[b]['sup']]) for b in range(B))
    bar, lbar = max(bar, 16 * sens), max(lbar, 16 * sens)
    rows = []
    for b in range(B):
        o = o64[b]
        near = near_edges(o)
        assert near.mean() <= 1e-3, (what, b, int(near.sum()))
        gsup = (got[b] != 0).any(0)
        assert np.array_equal(gsup[~near], o['sup'][~near]), (what, b, int((gsup != o['sup'])[~near].sum()))
        assert not np.ascontiguousarray(got[b][:, ~gsup]).view(np.uint8).any(), (what, b)          # +0.0 exactly, no -0.0
        assert np.isfinite(got[b]).all() and np.isfinite(lam[b]).all()
        assert int(rank[b]) == o['rank'], (what, b, rank[b], o['rank'])
        both = gsup & o['sup'] & o32[b]['sup'] & ~near
        rows.append((M.rel(got[b][:, both], o['maps'][:, both]), M.rel(lam[b][both], o['lam'][both])))
    print('%s %s: maps worst slice %.2e (bar %.2e), lambda %.2e (bar %.2e), Gram-order sensitivity %.2e, ranks %s'
          % (what, precision, max(r[0] for r in rows), bar, max(r[1] for r in rows), lbar, sens, list(map(int, rank))))
    for b, (err, lerr) in enumerate(rows):
        assert err <= bar, (what, b, err, bar)
        assert lerr <= lbar, (what, b, lerr, lbar)


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,k,n,H,W,ncal', CASES)
def test_espirit_maps_against_the_oracle(Cn, k, n, H, W, ncal, precision):
    """pnp_espirit_maps end to end.  Measured on an MI355X: see DESIGN.md section 19."""
    masks, _, _, y = scene(Cn, H, W, ncal)
    o64, o32, rev = oracle(Cn, k, n, H, W, ncal)
    got, lam, rank = raw_maps(y, masks, MID, ncal, k, n, precision)
    compare(got, lam, rank, o64, o32, rev, precision, 'C=%d k=%d n=%d %dx%d ncal=%d' % (Cn, k, n, H, W, ncal))


@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_a_body_across_the_image_edges(precision):
    """The phantom and its maps rolled by (H / 2, W / 2): the body and the support cross all four edges.  The same bars."""
    Cn, k, n, H, W, ncal = ROLLED
    masks, imgs, _, y = scene(Cn, H, W, ncal, True)
    o64, o32, rev = oracle(Cn, k, n, H, W, ncal, True)
    assert all(o['sup'][0].any() and o['sup'][-1].any() and o['sup'][:, 0].any() and o['sup'][:, -1].any() for o in o64)
    assert all(o['sup'][imgs[b] > 0].all() for b, o in enumerate(o64))
    got, lam, rank = raw_maps(y, masks, MID, ncal, k, n, precision)
    compare(got, lam, rank, o64, o32, rev, precision, 'rolled C=%d k=%d %dx%d' % (Cn, k, H, W))


# ---- 2. exact statements ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn,k,n,H,W,ncal', [CASES[0], CASES[2], CASES[3], CASES[5]])
def test_exact_statements(Cn, k, n, H, W, ncal, precision):
    """Outside the support every entry is +0.0 to the bit; inside, sum_c |S_c|^2 is within 4 C ulp of 1; the support is the stated rule on
    the returned lambda; a slice alone (on a context of another Bmax, with a null mask_id, without lambda_out) is bit-equal to the slice in
    the batch; two runs are bit-equal."""
    masks, _, _, y = scene(Cn, H, W, ncal)
    got, lam, rank = raw_maps(y, masks, MID, ncal, k, n, precision)
    again, lam2, rank2 = raw_maps(y, masks, MID, ncal, k, n, precision)
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8)) and np.array_equal(lam.view(np.uint8), lam2.view(np.uint8))
    assert np.array_equal(rank, rank2)
    for b in range(B):
        sup = (got[b] != 0).any(0)
        assert 0 < sup.sum() < sup.size
        assert not np.ascontiguousarray(got[b][:, ~sup]).view(np.uint8).any(), b
        g = got[b].astype(np.clongdouble)                    # measured in extended precision: float64 sums would add an ulp of their own
        n2 = (g.real ** 2 + g.imag ** 2).sum(0)[sup]
        off = float(np.abs(n2 - 1).max() / EPS[precision])
        print('C=%d %s slice %d: |sum |S|^2 - 1| <= %.2f ulp (bar %d)' % (Cn, precision, b, off, 4 * Cn))
        assert off <= 4 * Cn, (b, off)
        assert (lam[b] >= 0).all() and not (sup & ~(lam[b] >= lam[b].dtype.type(CROP))).any()
    alone, _, rank1 = raw_maps(y[1:2], masks[MID[1]][None], None, ncal, k, n, precision, Bmax=64, want_lambda=False)
    assert np.array_equal(alone[0].view(np.uint8), got[1].view(np.uint8)) and rank1[0] == rank[1]


@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_wrapper_on_host_arrays_and_device_tensors(precision):
    """coilmaps.estimate(method='espirit'): a host y walked one slice at a time equals the walk in one piece, a device tensor gives device
    tensors, an engine of the caller's gives the same -- all bit for bit, and equal to the raw call; radius is ignored."""
    import torch
    from pnp_admm_cnc_mri_amd import Engine, coilmaps, utils_pnp as U
    Cn, k, n, H, W, ncal = CASES[2]
    masks, _, _, y = scene(Cn, H, W, ncal)
    raw, raw_lam, raw_rank = raw_maps(y, masks, MID, ncal, k, n, precision)
    kw = dict(calib=ncal, power_iters=n, thresh=THRESH, precision=precision, method='espirit', kernel=k, sigma=SIGMA, crop=CROP)
    whole, lam, rank = coilmaps.estimate(y, masks, MID, return_lambda=True, return_rank=True, **kw)
    pieces = coilmaps.estimate(y, masks, MID, chunk_bytes=1, radius=3, **kw)
    assert isinstance(whole, np.ndarray) and whole.dtype == cdt(precision) and whole.shape == y.shape and lam.shape == (B, H, W)
    assert np.array_equal(whole.view(np.uint8), raw.view(np.uint8)) and np.array_equal(lam.view(np.uint8), raw_lam.view(np.uint8))
    assert np.array_equal(whole.view(np.uint8), pieces.view(np.uint8)) and np.array_equal(rank, raw_rank)
    on_dev = U.estimate_coil_maps(dev(y.astype(cdt(precision))), masks, MID, **kw)
    assert torch.is_tensor(on_dev) and np.array_equal(on_dev.cpu().numpy().view(np.uint8), raw.view(np.uint8))
    with Engine(H, W, Bmax=B, precision=precision) as eng:
        mine = coilmaps.estimate(y, masks, MID, engine=eng, **kw)
    assert np.array_equal(mine.view(np.uint8), raw.view(np.uint8))


# ---- 3. errors ---------------------------------------------------------------------------------------------------------------------------------

def test_a_hole_in_the_calibration_region_and_overlapping_arrays_are_arg_errors():
    import torch
    from pnp_admm_cnc_mri_amd import Engine
    from pnp_admm_cnc_mri_amd._lib import PnpError
    Cn, k, n, H, W, ncal = CASES[1]
    masks, _, _, y = scene(Cn, H, W, ncal)
    bad = masks.copy()
    bad[1, H - 1, 2] = 0                                     # mask 1 serves slices 0 and 2
    bad[1, H - 2, 1] = 0
    with pytest.raises(PnpError) as e:
        raw_maps(y, bad, MID, ncal, k, n, 'f32')
    assert e.value.code == -1 and 'slice 0' in str(e.value) and '(%d, 1)' % (H - 2) in str(e.value), str(e.value)
    with pytest.raises(PnpError) as e:
        raw_maps(y[1:], bad, MID[1:], ncal, k, n, 'f64')
    assert e.value.code == -1 and 'slice 1' in str(e.value) and '(%d, 1)' % (H - 2) in str(e.value), str(e.value)
    buf = torch.zeros((2 * B, Cn, H, W), dtype=torch.complex64, device='cuda')
    bank_t = dev(masks)
    with Engine(H, W, Bmax=7) as eng:
        for out in (buf[:B], buf[1:B + 1], buf[B - 1:2 * B - 1]):
            with pytest.raises(PnpError) as e:
                eng.espirit_maps(buf[:B], bank_t, None, out, None, B, Cn, ncal, k, n, SIGMA, CROP, THRESH)
            assert e.value.code == -1 and 'overlap' in str(e.value)
        rank = eng.espirit_maps(buf[:B], bank_t, None, buf[B:], None, B, Cn, ncal, k, n, SIGMA, CROP, THRESH)          # adjacent is fine
        with pytest.raises(PnpError) as e:
            eng.espirit_maps(buf[:B], bank_t, None, buf[B:], None, B, Cn, ncal, 9, n, SIGMA, CROP, THRESH)
        assert e.value.code == -1 and 'kernel must be' in str(e.value)
    torch.cuda.synchronize()
    zero = buf[B:].cpu().numpy()
    # all-zero data: every singular value is 0 and is kept, P = 1, G = 1: v = e_0 with lambda = 1 >= crop, ||I|| = 0 >= 0
    assert (zero[:, 0] == 1).all() and not zero[:, 1:].any() and list(rank) == [Cn * k * k] * B
    with Engine(H, W, Bmax=7, precision='f64') as eng:      # the precision of the entry point is the context's
        rc = eng._L.pnp_espirit_maps(eng._ctx, C.c_void_p(buf.data_ptr()), C.c_void_p(bank_t.data_ptr()), None, C.c_void_p(buf[B:].data_ptr()),
                                     None, B, Cn, ncal, k, n, SIGMA, CROP, THRESH)
        assert rc == -3 and 'fp64' in eng._L.pnp_last_error().decode()


# ---- 4. end to end: ten iterations at the presets, 128 x 130, B = 3, C = 5 -----------------------------------------------------------------------

H5, W5, C5 = 128, 130, 5
ESP = dict(k=4, n=4)


def psnr(x, img):
    return float(10 * np.log10(1.0 / np.mean((np.asarray(x, np.float64) - img) ** 2)))


def solve(kind, y, masks, precision='f32', **kw):
    import pnp_admm_cnc_mri_amd as P
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    out, info = solver(masks, None, y=y, mask_id=MID, precision=precision, return_info=True, iter_num=10, **kw, **M.O_PRESETS[kind])
    return np.stack(out[:B]), info


def oracle_maps(y, m, dt=C128):
    return E.estimate(y, m, 24, ESP['k'], ESP['n'], SIGMA, CROP, THRESH, dt)


@functools.lru_cache(maxsize=None)
def oracle_solves(kind):
    """per slice: the float64 oracle's solve with the ORACLE's ESPIRiT maps, its float32 restatement's distance from it (estimate and solve
    in complex64), and the PSNR of the oracle's solve with the TRUE maps"""
    masks, imgs, S, y = scene(C5, H5, W5, 24)
    rows = []
    for b in range(B):
        m = masks[MID[b]]
        ref = M.admm(y[b], oracle_maps(y[b], m), m, 10, kind)
        y32 = y[b].astype(C64)
        r32 = M.admm(y32, oracle_maps(y32, m, C64), m, 10, kind, dt=C64)
        rows.append((ref, M.rel(r32, ref), psnr(M.admm(y[b], S[b], m, 10, kind), imgs[b])))
    return rows


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_solvers_with_espirit_maps(kind, precision):
    """coils='estimate', maps_method='espirit' against the oracle's ADMM run with the oracle's ESPIRiT maps: within 4 x the float32
    restatement's distance of that whole pipeline (double: 1e-10); the PSNR is no lower than the oracle's with the TRUE maps minus 0.1 dB."""
    masks, imgs, S, y = scene(C5, H5, W5, 24)
    got, info = solve(kind, y, masks, precision, coils='estimate', maps_method='espirit', images=imgs)
    cm = info['coil_maps']
    assert (cm['method'], cm['calib'], cm['kernel'], cm['sigma'], cm['crop'], cm['power_iters'], cm['thresh']) == ('espirit', 24, 4, 0.02, 0.9, 4, 0.05)
    assert len(cm['support']) == B and len(cm['rank']) == B and all(0 < r < C5 * 16 for r in cm['rank'])
    assert all(0.3 < s < 0.7 for s in cm['support']) and len(info['cg_residual']) == B
    for b, (ref, d32, psnr_true) in enumerate(oracle_solves(kind)):
        bar = 4 * d32 if precision == 'f32' else 1e-10
        err, p = rel_l2(got[b], ref), psnr(got[b], imgs[b])
        print('%s %s slice %d: %.2e (bar %.2e); PSNR %.2f dB, with the true maps %.2f dB' % (kind, precision, b, err, bar, p, psnr_true))
        assert err <= bar, (b, err, bar)
        assert p >= psnr_true - 0.1, (b, p, psnr_true)


def test_pnp_with_espirit_maps_equals_the_call_with_those_maps():
    """PNP_ADMM_L1_D with coils='estimate', maps_method='espirit' equals, bit for bit, the same call given
    coilmaps.estimate(method='espirit')'s output as coils= with coil_id = arange(B)."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import coilmaps
    Hn = Wn = 128
    masks, imgs, S, y = scene(4, Hn, Wn, 16)
    kw = dict(model=weights_trained(), iter_num=3, reo=0.25, mask_id=MID)
    got, info = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y, coils='estimate', calib=16, maps_method='espirit', maps_kernel=3,
                                maps_power_iters=3, maps_sigma=0.03, maps_crop=0.8, maps_thresh=0.1, return_info=True, **kw)
    cm = info['coil_maps']
    assert (cm['method'], cm['kernel'], cm['power_iters'], cm['sigma'], cm['crop'], cm['thresh']) == ('espirit', 3, 3, 0.03, 0.8, 0.1)
    maps = coilmaps.estimate(y, masks, MID, calib=16, method='espirit', kernel=3, power_iters=3, sigma=0.03, crop=0.8, thresh=0.1)
    want = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y, coils=maps, coil_id=np.arange(B), **kw)
    walsh = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y, coils='estimate', calib=16, **kw)          # the default method: other maps
    for b in range(B):
        assert np.array_equal(np.asarray(got[b]), np.asarray(want[b])), b
        assert rel_l2(walsh[b], got[b]) > 1e-6, b


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_40_channels_of_rank_4_with_espirit_maps(kind):
    """40 physical channels spanning a 4-dimensional map space, virtual_coils = 4, maps_method='espirit': y is mixed by ONE matrix, the maps
    come from the mixed y (4 * 16 = 64 columns; 40 channels alone would be refused).  Equals the oracle pipeline at the end-to-end bars."""
    masks, imgs, _, _ = scene(C5, H5, W5, 24)
    S = CO.rank4_maps(40, H5, W5, 4)
    y = np.stack([M.synthesize(imgs[b], S, masks[MID[b]], M.noise(b, 40, masks[MID[b]])) for b in range(B)])
    got, info = solve(kind, y, masks, coils='estimate', maps_method='espirit', virtual_coils=4, images=imgs)
    Mx = info['coil_mix']['M']
    assert Mx.shape == (4, 40) and info['coil_mix']['energy'] > 0.99 and len(info['coil_maps']['rank']) == B
    for b in range(B):
        m = masks[MID[b]]
        y2 = CO.mix(y[b], Mx)
        ref = M.admm(y2, oracle_maps(y2, m), m, 10, kind)
        y32 = CO.mix(y[b].astype(C64), Mx, C64)
        bar = 4 * M.rel(M.admm(y32, oracle_maps(y32, m, C64), m, 10, kind, dt=C64), ref)
        err = rel_l2(got[b], ref)
        print('rank 4 of 40, ESPIRiT maps, %s slice %d: %.2e (bar %.2e), PSNR %.2f dB' % (kind, b, err, bar, psnr(got[b], imgs[b])))
        assert err <= bar, (b, err, bar)


# ---- 5. Walsh and the fast paths untouched ------------------------------------------------------------------------------------------------------

def test_an_espirit_call_on_an_engine_leaves_no_state_behind():
    """A single-coil solve (256 x 256, the fused path), a coils=array solve and a Walsh estimate give the same bits and the same path before
    and after coilmaps.estimate(method='espirit') ran on the same engine; maps_method='walsh' is the call without the argument."""
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
        walsh0 = coilmaps.estimate(ymc, m1, engine=eng)
        first = coilmaps.estimate(ymc, m1, engine=eng, method='espirit')
        middle = run(eng, lambda: eng.upload(y1, m1))
        eng.upload(y1, m1)
        eng.init_state()
        second = coilmaps.estimate(ymc, m1, engine=eng, method='espirit')          # between init_state and the loop
        eng.admm_cnc(5, par['alpha'], par['lambda1'], par['reo'], par['b'])
        after = (eng.x().copy(), eng.path_name, eng.ctx_path)
        walsh1 = coilmaps.estimate(ymc, m1, engine=eng, method='walsh')
    assert before[1:] == middle[1:] == after[1:]
    assert np.array_equal(before[0], middle[0]) and np.array_equal(before[0], after[0]) and np.array_equal(first, second)
    assert np.array_equal(walsh0, walsh1)

    masks, imgs, S, y = scene(C5, H5, W5, 24)
    with Engine(H5, W5, Bmax=B) as eng:
        eng.set_coils(S[0])
        up = lambda: eng.upload(y, masks, MID)
        before = run(eng, up)
        est = coilmaps.estimate(y, masks, MID, engine=eng, method='espirit')
        after = run(eng, up)
        assert eng.coils['C'] == C5 and eng.coils['Ks'] == 1
    assert before[1:] == after[1:] and np.array_equal(before[0], after[0])
    assert np.array_equal(est, coilmaps.estimate(y, masks, MID, method='espirit'))
    a, ia = solve('cnc', y, masks, coils='estimate', images=imgs)
    b, ib = solve('cnc', y, masks, coils='estimate', maps_method='walsh', images=imgs)
    assert np.array_equal(a, b) and ia['coil_maps'] == ib['coil_maps'] and 'method' not in ia['coil_maps']


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Bmax', [2, 4])
def test_the_estimators_share_one_scratch_array(Bmax, precision):
    """The context keeps ONE scratch array for pnp_coil_maps, pnp_espirit_maps and pnp_espirit_eigmaps, and each call lays it out anew.  On
    one engine, in this order: Walsh without lambda_out (lambda lives in the array), ESPIRiT without lambda_out (the array grows),
    espirit_eigmaps (another layout of it), Walsh with lambda_out -- every output is bit for bit that of the same call on a fresh engine.
    128 x 128, C = 2, B = 3, calib 8, kernel 2.  Bmax = 2: three passes of one slice; Bmax = 4: a pass of two slices and one of one."""
    import torch
    from pnp_admm_cnc_mri_amd import Engine
    Cn, k, n, H, W, ncal = 2, 2, 2, 128, 128, 8
    masks, _, _, y = scene(Cn, H, W, ncal)
    rng = np.random.default_rng(11)
    D = 2 * k - 1
    cplx = lambda *shape: dev((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt(precision)))
    y_t, bank_t, mid_t, img_t, w_t = dev(y.astype(cdt(precision))), dev(masks), dev(MID), cplx(B, Cn, H, W), cplx(B, Cn, Cn, D, D)

    def call(eng, which):
        out = torch.full((B, Cn, H, W), float('nan'), dtype=y_t.dtype, device='cuda')
        lam = torch.full((B, H, W), float('nan'), dtype=out.real.dtype, device='cuda')
        if which == 'walsh':
            eng.coil_maps(y_t, bank_t, mid_t, out, None, B, Cn, ncal)
        elif which == 'espirit':
            eng.espirit_maps(y_t, bank_t, mid_t, out, None, B, Cn, ncal, k, n, SIGMA, CROP, THRESH)
        elif which == 'eigmaps':
            eng.espirit_eigmaps(img_t, w_t, out, lam, B, Cn, k, n)
        else:
            eng.coil_maps(y_t, bank_t, mid_t, out, lam, B, Cn, ncal)
        torch.cuda.synchronize()
        return [out.cpu().numpy()] + ([] if which in ('walsh', 'espirit') else [lam.cpu().numpy()])

    order = ['walsh', 'espirit', 'eigmaps', 'walsh_lambda']
    with Engine(H, W, Bmax=Bmax, precision=precision) as eng:
        shared = [call(eng, which) for which in order]
    for which, got in zip(order, shared):
        with Engine(H, W, Bmax=Bmax, precision=precision) as eng:
            want = call(eng, which)
        assert all(np.isfinite(a).all() for a in got), which
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), which
