"""Coil mixing on the GPU (pnp_coil_mix, pnp_coil_gram, virtual_coils= / noise_cov= on the solvers) against tests/coilmix_oracle.py and
tests/multicoil_oracle.py.

Shapes: the smallest at which the kernels can still go wrong -- N = 1, 63, 64, 65 (one thread, the two-point tail, odd N: the path
without 16-byte accesses), 1025 (more than one workgroup in double, an odd tail), 128 x 130 (the slices of the end-to-end cases);
C_out in every accumulator bucket (1, 3, 5, 8, 32) with C_in below, at and above the 32-column chunk of M; Gram matrices with one tile of
pairs (C = 1, 2), three tiles with a ragged edge (33) and 36 tiles (128), ncal even / odd / below and above the 64 points staged at a
time.  Float bars: 4 x the distance of the oracle's own complex64 restatement from its float64 form on the same inputs (computed here, per
case); double: the element-wise rounding bounds of a chain of the case's length, stated at each test."""
import ctypes as C
import functools

import numpy as np
import pytest

import coilmix_oracle as CO
import multicoil_oracle as M
from conftest import rel_l2, weights_trained

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
H, W, B = 128, 130, 3
MID = np.array([0, 1, 0], np.int32)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda')


# ---- 1. pnp_coil_mix on plain arrays ----------------------------------------------------------------------------------------------------

def raw_mix(k, Mx, set_id=None):
    """pnp_coil_mix[_f64] on device copies of k [B,C_in,N] and Mx [Ks,C_out,C_in]; -> host array"""
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    fn = L.pnp_coil_mix_f64 if k.dtype == C128 else L.pnp_coil_mix
    k_t, m_t = dev(k), dev(Mx.astype(k.dtype))
    s_t = None if set_id is None else dev(np.asarray(set_id, np.int32))
    out = torch.full((k.shape[0], Mx.shape[1], k.shape[2]), float('nan'), dtype=k_t.dtype, device='cuda')
    _lib.check(fn(None, C.c_void_p(k_t.data_ptr()), C.c_void_p(m_t.data_ptr()), None if s_t is None else C.c_void_p(s_t.data_ptr()),
                  C.c_void_p(out.data_ptr()), k.shape[0], k.shape[1], Mx.shape[1], k.shape[2]))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('C_in,C_out', [(1, 1), (2, 1), (5, 3), (33, 5), (64, 8), (128, 32), (32, 32)])
def test_coil_mix_on_plain_arrays(C_in, C_out, precision):
    """B = 3 with set_id = [1, 0, 1] into Ks = 2 matrices, B = 3 and B = 1 with a null set_id, at every N.
    Float: the relative L2 distance of every slice's result from the float64 oracle is within 4 x the complex64 restatement's own
    distance.  The restatement's distance is ONE number per case (C_in, C_out): sqrt(sum |r32 - r64|^2 / sum |r64|^2) over all the
    case's inputs, every N and slice -- with N = 1 and C_out = 1 a slice's result is a single complex number, whose rounding error in
    EITHER arithmetic is anything from 0 to a few ulps, so the ratio of two such numbers says nothing (one came out as 9.0e-8 against
    1.1e-8); over the case's 10^5 .. 10^6 values the restatement's distance is the root-mean-square rounding error of a C_in-term chain.
    Double: |got - ref| <= (C_in + 4) 2^-52 sum_c |M_jc| |in_c| element-wise -- a chain of 2 C_in fused multiply-adds per component has the
    a-priori bound 2 C_in u = C_in 2^-52 times that sum; a bound, not a measurement.
    A slice mixed alone is bit-equal to the same slice inside the batch."""
    dt = C64 if precision == 'f32' else C128
    sid = np.array([1, 0, 1], np.int32)
    runs, num, den = [], 0.0, 0.0
    for N in (1, 63, 64, 65, 1025, 128 * 130):
        rng = np.random.default_rng(1000 * C_in + C_out + N)
        k = (rng.standard_normal((3, C_in, N)) + 1j * rng.standard_normal((3, C_in, N))).astype(dt)
        Mx = ((rng.standard_normal((2, C_out, C_in)) + 1j * rng.standard_normal((2, C_out, C_in))) / np.sqrt(C_in)).astype(dt)
        got = raw_mix(k, Mx, sid)
        got0 = raw_mix(k, Mx[:1], None)                              # null set_id: set 0 for every slice
        alone = raw_mix(k[1:2], Mx[:1], None)                        # B = 1; slice 1 uses set 0 in the batch as well
        assert got.shape == (3, C_out, N) and np.isfinite(got).all() and np.isfinite(got0).all()
        assert np.array_equal(alone[0], got[1]) and np.array_equal(alone[0], got0[1]), N
        for b, res, s in ((0, got, 1), (1, got, 0), (2, got, 1), (0, got0, 0), (2, got0, 0)):
            ref = CO.mix(k[b].astype(C128), Mx[s].astype(C128))
            if precision == 'f32':
                r32 = CO.mix(k[b], Mx[s], C64)
                num, den = num + np.sum(np.abs(r32 - ref) ** 2), den + np.sum(np.abs(ref) ** 2)
                runs.append((N, b, s, M.rel(res[b], ref)))
            else:
                bound = (C_in + 4) * 2.0 ** -52 * CO.mix_abs(k[b], Mx[s])
                excess = (np.abs(res[b] - ref) / bound).max()
                assert excess <= 1.0, (N, b, excess)
    if precision == 'f32':
        bar = 4 * np.sqrt(num / den)
        worst = max(runs, key=lambda r: r[3])
        print('f32 %d -> %d: restatement %.2e, worst slice %.2e at N = %d' % (C_in, C_out, bar / 4, worst[3], worst[0]))
        for N, b, s, err in runs:
            assert err <= bar, (N, b, s, err, bar)


def test_coil_mix_wrapper_on_device_tensors_and_host_arrays():
    """coilmix.mix: a device tensor gives a device tensor, a host array a host array, chunked or not, all bit-equal; a bank of maps is
    mixed with coil_id = arange(Ks)."""
    import torch
    from pnp_admm_cnc_mri_amd import coilmix as CM, utils_pnp as U
    rng = np.random.default_rng(3)
    k = (rng.standard_normal((4, 6, 128, 130)) + 1j * rng.standard_normal((4, 6, 128, 130))).astype(C64)
    Mx = rng.standard_normal((2, 3, 6)) + 1j * rng.standard_normal((2, 3, 6))
    cid = np.array([1, 0, 0, 1], np.int32)
    host = CM.mix(k, Mx, cid)
    small = CM.mix(k, Mx, cid, chunk_bytes=1)                        # one slice per chunk
    on_dev = U.coil_mix(dev(k), Mx, cid)
    assert isinstance(host, np.ndarray) and host.dtype == C64 and host.shape == (4, 3, 128, 130) and torch.is_tensor(on_dev)
    assert np.array_equal(host, small) and np.array_equal(host, on_dev.cpu().numpy())
    assert np.array_equal(host, raw_mix(k.reshape(4, 6, -1), Mx, cid).reshape(host.shape))
    with pytest.raises(ValueError, match='coil_id'):
        CM.mix(k, Mx)
    with pytest.raises(ValueError, match='coil_id out of range'):
        CM.mix(k, Mx, [0, 1, 2, 0])
    with pytest.raises(ValueError, match='C_out must be'):
        CM.mix(k, np.ones((7, 6)))


# ---- 2. pnp_coil_gram ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def gram_data(Cn, Hn, Wn):
    rng = np.random.default_rng(Cn + Hn + Wn)
    y = rng.standard_normal((B, Cn, Hn, Wn), dtype=np.float32) + 1j * rng.standard_normal((B, Cn, Hn, Wn), dtype=np.float32)
    masks = np.stack([M.mask(Hn + s, Hn, Wn) for s in range(3)])     # full lines 0 .. 2 and H - 3 .. H - 1, 30 % elsewhere: holes inside the region
    return y.astype(C64), masks


def raw_gram(y_t, masks_t, mid, ncal):
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    fn = L.pnp_coil_gram_f64 if y_t.dtype == torch.complex128 else L.pnp_coil_gram
    Bn, Cn, Hn, Wn = y_t.shape
    out = torch.full((Bn, Cn, Cn), float('nan'), dtype=torch.complex128, device='cuda')
    mid_t = None if mid is None else dev(np.asarray(mid, np.int32))
    _lib.check(fn(None, C.c_void_p(y_t.data_ptr()), C.c_void_p(masks_t.data_ptr()), None if mid_t is None else C.c_void_p(mid_t.data_ptr()),
                  C.c_void_p(out.data_ptr()), Bn, Cn, Hn, Wn, ncal))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('Cn', [1, 2, 33, 128])
@pytest.mark.parametrize('Hn,Wn', [(128, 128), (131, 128), (140, 160)])
def test_coil_gram(Hn, Wn, Cn, precision):
    """B = 3 slices with three different masks, against NumPy float64: |got - ref| <= (ncal^2 + 4) 2^-51 sum_p |y_i| |y_j| element-wise (a
    chain of ncal^2 terms, each the rounded sum of two rounded products, plus the reference's own error of the same form); exactly
    Hermitian, the diagonal exactly real; a slice alone is bit-equal to the slice in the batch."""
    y32, masks = gram_data(Cn, Hn, Wn)
    y = y32 if precision == 'f32' else y32.astype(C128) * (1.0 + 1.0 / 3.0)          # double inputs that are no float32 values
    mid = np.array([2, 0, 1], np.int32)
    y_t, masks_t = dev(y), dev(masks)
    for ncal in ((4, 5) if Cn == 128 else (4, 5, 24, 64)):
        got = raw_gram(y_t, masks_t, mid, ncal)
        assert np.isfinite(got).all()
        alone = raw_gram(y_t[1:2].contiguous(), masks_t[mid[1]:mid[1] + 1].contiguous(), None, ncal)
        assert np.array_equal(alone[0], got[1]), ncal
        for b in range(B):
            ref, scale = CO.gram(y[b], masks[mid[b]], ncal)
            excess = (np.abs(got[b] - ref) / ((ncal * ncal + 4) * 2.0 ** -51 * scale)).max()
            assert excess <= 1.0, (ncal, b, excess)
            assert np.array_equal(got[b], got[b].conj().T) and not got[b].diagonal().imag.any(), (ncal, b)
            assert (got[b].diagonal().real > 0).all()


def test_calibration_gram_sums_per_coil_set_in_slice_order():
    from pnp_admm_cnc_mri_amd import coilmix as CM
    y, masks = gram_data(2, 128, 128)
    mid, cid = np.array([2, 0, 1], np.int32), np.array([1, 0, 1], np.int32)
    per = CM.calibration_gram(y, masks, mid, ncal=24, per_slice=True)
    got = CM.calibration_gram(y, masks, mid, cid, Ks=2, ncal=24)
    assert got.shape == (2, 2, 2) and np.array_equal(got[0], per[1]) and np.array_equal(got[1], per[0] + per[2])
    assert np.array_equal(got, CM.calibration_gram(y, masks, mid, cid, Ks=2, ncal=24, chunk_bytes=1))
    assert np.array_equal(got, CM.calibration_gram(dev(y), masks, mid, cid, Ks=2, ncal=24))
    assert np.array_equal(CM.calibration_gram(y, masks, mid, ncal=24)[0], per[0] + per[1] + per[2])


# ---- 3. end to end: ten iterations at the presets, 128 x 130, B = 3 ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene():
    masks = np.stack([M.mask(H, H, W), M.mask(H + 1, H, W)])
    imgs = np.stack([M.phantom(10 * H + b, H, W) for b in range(B)])
    return masks, imgs


def measure(S, noise_of=None, cid=None):
    """y [B,C,H,W] complex128 through the maps S ([C,H,W], or a bank with cid)"""
    masks, imgs = scene()
    out = []
    for b in range(B):
        Sb, m = (S if cid is None else S[cid[b]]), masks[MID[b]]
        out.append(M.synthesize(imgs[b], Sb, m, M.noise(b, len(Sb), m) if noise_of is None else noise_of(b, m)))
    return np.stack(out)


def solve(kind, y, S, precision='f32', **kw):
    import pnp_admm_cnc_mri_amd as P
    masks, _ = scene()
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    out, info = solver(masks, None, y=y, mask_id=MID, coils=S, precision=precision, return_info=True, iter_num=10, **kw, **M.O_PRESETS[kind])
    return np.stack(out[:B]), info


def against_oracle(kind, got, y, S_of, M_of, what):
    """every slice against the oracle run on the oracle-mixed data, within 4 x the float32 restatement's own distance on those data"""
    masks, _ = scene()
    for b in range(B):
        m, Mb = masks[MID[b]], M_of(b)
        y2, S2 = CO.mix(y[b], Mb), CO.mix(S_of(b), Mb)
        ref = M.admm(y2, S2, m, 10, kind)
        bar = 4 * M.rel(M.admm(y2.astype(C64), S2.astype(C64), m, 10, kind, dt=C64), ref)
        err = rel_l2(got[b], ref)
        print('%s %s slice %d: %.2e (bar %.2e)' % (what, kind, b, err, bar))
        assert err <= bar, (what, b, err, bar)


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_a_unitary_mix_agrees_with_the_unmixed_solve(kind):
    """C_out = C_in = 5: the compression matrix is unitary and the mixed solve is the unmixed one -- in float within 4 x the float32
    restatement's distance, in double to 1e-12 (the float64 oracle gives 1e-15)."""
    S = M.coil_maps(5, H, W, 21)
    y = measure(S)
    masks, _ = scene()
    plain, _ = solve(kind, y, S)
    mixed, info = solve(kind, y, S, virtual_coils=5)
    Mx = info['coil_mix']['M']
    assert Mx.shape == (5, 5) and np.abs(Mx @ Mx.conj().T - np.eye(5)).max() <= 1e-12 and abs(info['coil_mix']['energy'] - 1.0) <= 1e-12
    for b in range(B):
        ref = M.admm(y[b], S, masks[MID[b]], 10, kind)
        bar = 4 * M.rel(M.admm(y[b].astype(C64), S.astype(C64), masks[MID[b]], 10, kind, dt=C64), ref)
        err = rel_l2(mixed[b], plain[b])
        print('unitary %s slice %d: mixed vs unmixed %.2e (bar %.2e)' % (kind, b, err, bar))
        assert err <= bar, (b, err, bar)
    plain64, _ = solve(kind, y, S, precision='f64')
    mixed64, _ = solve(kind, y, S, precision='f64', virtual_coils=5)
    for b in range(B):
        err = rel_l2(mixed64[b], plain64[b])
        print('unitary %s slice %d double: %.2e' % (kind, b, err))
        assert err <= 1e-12, (b, err)


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_40_channels_of_rank_4_compress_to_4_virtual_coils(kind):
    """40 physical channels (more than the solve takes) spanning a 4-dimensional map space, virtual_coils = 4: the solve agrees with the
    oracle run on the oracle-mixed data, with the M the solver returned."""
    S = CO.rank4_maps(40, H, W, 4)
    y = measure(S)
    got, info = solve(kind, y, S, virtual_coils=4)
    cm = info['coil_mix']
    assert cm['M'].shape == (4, 40) and cm['eigvals'].shape == (40,) and cm['energy'] > 0.999
    assert np.abs(cm['M'] @ cm['M'].conj().T - np.eye(4)).max() <= 1e-12
    print('eigenvalues / largest:', cm['eigvals'][:6] / cm['eigvals'][0], 'energy', cm['energy'])
    against_oracle(kind, got, y, lambda b: S, lambda b: cm['M'], 'rank 4 of 40')


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_prewhitening_with_correlated_noise(kind):
    """noise_cov= alone (C_out = C_in = 5): the solve equals the oracle's on the whitened data, M = L^-1."""
    S = M.coil_maps(5, H, W, 22)
    psi = CO.hpd(5, 9)
    y = measure(S, noise_of=lambda b, m: CO.correlated_noise(b, psi, m))
    got, info = solve(kind, y, S, noise_cov=psi)
    Mw = info['coil_mix']['M']
    assert np.abs(Mw - CO.whitening_matrix(psi)).max() <= 1e-12 and info['coil_mix']['eigvals'] is None
    against_oracle(kind, got, y, lambda b: S, lambda b: Mw, 'whitened')


def test_a_two_set_bank_with_whitening_and_compression():
    """Ks = 2 sets of 6 maps, coil_id = [1, 0, 1], 6 -> 3 virtual coils after whitening: one matrix per set, from the Gram matrices of the
    slices that use the set; every slice agrees with the oracle on its set's mixed data."""
    from pnp_admm_cnc_mri_amd import coilmix as CM
    bank = np.stack([M.coil_maps(6, H, W, 31), M.coil_maps(6, H, W, 32)])
    cid = np.array([1, 0, 1], np.int32)
    psi = CO.hpd(6, 5)
    y = measure(bank, noise_of=lambda b, m: CO.correlated_noise(b, psi, m), cid=cid)
    masks, _ = scene()
    got, info = solve('cnc', y, bank, coil_id=cid, virtual_coils=3, noise_cov=psi)
    Mx = info['coil_mix']['M']
    assert Mx.shape == (2, 3, 6) and len(info['coil_mix']['energy']) == 2 and info['coil_mix']['eigvals'].shape == (2, 6)
    gram = CM.calibration_gram(y.astype(C64), masks, MID, cid, Ks=2, ncal=24)
    want, _ = CM.compression_matrix(gram, 3, CM.whitening_matrix(psi))
    assert np.array_equal(Mx, want)
    Mw = CO.whitening_matrix(psi)                                    # set 0 is slice 1's alone: NumPy on the same float32 data
    ref_M0, _ = CO.compression(Mw @ CO.gram(y[1].astype(C64), masks[MID[1]], 24)[0] @ Mw.conj().T, 3)
    assert np.abs(CO.projector(ref_M0 @ Mw) - CO.projector(Mx[0])).max() <= 1e-8
    against_oracle('cnc', got, y, lambda b: bank[cid[b]], lambda b: Mx[cid[b]], 'bank')


def test_pnp_takes_the_coil_mixing_arguments():
    """PNP_ADMM_L1_D with virtual_coils= / noise_cov= equals, bit for bit, the same call on data mixed beforehand with coilmix.prepare;
    the options dict swallows unknown keywords, so the arguments must not be among them."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import coilmix as CM
    Hn = Wn = 128
    S = M.coil_maps(6, Hn, Wn, 5)
    m = M.mask(128, Hn, Wn)
    imgs = np.stack([M.phantom(10 * 128 + b, Hn, Wn) for b in range(B)])
    y = np.stack([M.synthesize(imgs[b], S, m, M.noise(b, 6, m)) for b in range(B)])
    psi = CO.hpd(6, 2)
    kw = dict(model=weights_trained(), iter_num=3, reo=0.25)
    got, info = P.PNP_ADMM_L1_D('ffdnet_gray', m, None, y=y, coils=S, virtual_coils=2, noise_cov=psi, return_info=True, **kw)
    y2, S2, pinfo = CM.prepare(y, S, m, virtual_coils=2, noise_cov=psi)
    assert y2.shape == (B, 2, Hn, Wn) and S2.shape == (2, Hn, Wn) and np.array_equal(info['coil_mix']['M'], pinfo['M'])
    want = P.PNP_ADMM_L1_D('ffdnet_gray', m, None, y=y2, coils=S2, **kw)
    plain = P.PNP_ADMM_L1_D('ffdnet_gray', m, None, y=y, coils=S, **kw)
    for b in range(B):
        assert np.array_equal(np.asarray(got[b]), np.asarray(want[b])), b
        assert rel_l2(got[b], plain[b]) > 1e-6, b


def test_host_y_chunked_equals_unchunked():
    """prepare() on a host array walked one slice at a time equals the walk in one piece, bit for bit: y', the maps and M."""
    from pnp_admm_cnc_mri_amd import coilmix as CM
    bank = np.stack([M.coil_maps(6, H, W, 41), M.coil_maps(6, H, W, 42)])
    cid = np.array([1, 0, 1], np.int32)
    y = measure(bank, cid=cid)
    masks, _ = scene()
    a = CM.prepare(y, bank, masks, MID, cid, virtual_coils=3, noise_cov=CO.hpd(6, 1))
    b = CM.prepare(y, bank, masks, MID, cid, virtual_coils=3, noise_cov=CO.hpd(6, 1), chunk_bytes=1)
    c = CM.prepare(y.astype(C64), bank, masks, MID, cid, virtual_coils=3, noise_cov=CO.hpd(6, 1), chunk_bytes=6 * H * W * 8 * 2)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and np.array_equal(a[2]['M'], other[2]['M'])
    assert a[0].dtype == C64 and a[0].shape == (B, 3, H, W) and a[1].shape == (2, 3, H, W)
