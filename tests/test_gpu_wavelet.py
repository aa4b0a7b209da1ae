"""GPU tests of the wavelet-domain sparsity (pnp_set_sparsity, pnp_dwt2_*, the transform= / levels= keywords of ADMM_L1 / ADMM_CNC) against
the NumPy restatement tests/wavelet_oracle.py.  Every figure printed before an assertion is what the card gave.

float32 bars of the transform and the single prox step: 4 x the distance of the float32 restatement from the float64 one on the same inputs
(the factor is for the freedom in the order of the sums), measured on the CPU by
    python tests/wavelet_oracle.py
and held below as DWT_F32 / PROX_F32.  Double contexts: 1e-12, three orders above the round-off of a 2 L T-term double chain; an
indexing error is O(1).  Whole loops of 10 iterations: 1e-5 in float32 (the project's bar for <= 10 iterations), 1e-10 in double."""
import functools
import os

import numpy as np
import pytest

import wavelet_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DWT_F32 = {   # (H, W, name, L): (Psi, Psi^T, Psi^T Psi)
    (128, 128, 'haar', 1): (6.32e-08, 6.29e-08, 9.43e-08),
    (128, 128, 'haar', 4): (7.88e-08, 7.87e-08, 1.25e-07),
    (128, 128, 'db2', 1): (7.40e-08, 7.15e-08, 1.01e-07),
    (128, 128, 'db2', 4): (8.70e-08, 8.41e-08, 1.22e-07),
    (128, 128, 'db4', 1): (9.27e-08, 9.08e-08, 1.28e-07),
    (128, 128, 'db4', 4): (1.09e-07, 1.06e-07, 1.52e-07),
    (128, 160, 'haar', 1): (6.27e-08, 6.27e-08, 9.45e-08),
    (128, 160, 'haar', 4): (7.87e-08, 7.96e-08, 1.25e-07),
    (128, 160, 'db2', 1): (7.44e-08, 7.10e-08, 1.02e-07),
    (128, 160, 'db2', 4): (8.75e-08, 8.42e-08, 1.22e-07),
    (128, 160, 'db4', 1): (9.23e-08, 9.10e-08, 1.27e-07),
    (128, 160, 'db4', 4): (1.09e-07, 1.06e-07, 1.51e-07),
    (256, 192, 'haar', 1): (6.28e-08, 6.35e-08, 9.54e-08),
    (256, 192, 'haar', 4): (7.92e-08, 7.94e-08, 1.26e-07),
    (256, 192, 'db2', 1): (7.49e-08, 7.12e-08, 1.02e-07),
    (256, 192, 'db2', 4): (8.80e-08, 8.38e-08, 1.22e-07),
    (256, 192, 'db4', 1): (9.19e-08, 9.05e-08, 1.27e-07),
    (256, 192, 'db4', 4): (1.08e-07, 1.06e-07, 1.53e-07),
    (256, 256, 'haar', 1): (6.32e-08, 6.34e-08, 9.55e-08),
    (256, 256, 'haar', 4): (7.95e-08, 7.96e-08, 1.26e-07),
    (256, 256, 'db2', 1): (7.42e-08, 7.12e-08, 1.01e-07),
    (256, 256, 'db2', 4): (8.70e-08, 8.40e-08, 1.21e-07),
    (256, 256, 'db4', 1): (9.19e-08, 9.02e-08, 1.28e-07),
    (256, 256, 'db4', 4): (1.08e-07, 1.06e-07, 1.53e-07),
    (512, 512, 'haar', 1): (6.29e-08, 6.33e-08, 9.53e-08),
    (512, 512, 'db2', 1): (7.44e-08, 7.09e-08, 1.01e-07),
    (512, 512, 'db4', 1): (9.21e-08, 9.02e-08, 1.28e-07),
}
PROX_F32 = {   # (kind, name, L, H, W): (z+, w+)
    ('l1', 'db4', 4, 128, 128): (3.40e-07, 6.48e-07),
    ('cnc', 'db4', 4, 128, 128): (3.49e-07, 4.44e-07),
    ('l1', 'db2', 3, 128, 160): (1.67e-07, 3.24e-07),
    ('cnc', 'db2', 3, 128, 160): (1.71e-07, 2.21e-07),
    ('l1', 'haar', 4, 256, 192): (2.72e-07, 5.20e-07),
    ('cnc', 'haar', 4, 256, 192): (2.76e-07, 3.50e-07),
    ('l1', 'db4', 3, 256, 256): (2.81e-07, 5.44e-07),
    ('cnc', 'db4', 3, 256, 256): (2.85e-07, 3.61e-07),
    ('l1', 'db2', 1, 512, 512): (1.10e-07, 2.56e-07),
    ('cnc', 'db2', 1, 512, 512): (1.08e-07, 1.48e-07),
}
FREEDOM = 4.0            # order of the sums
F64_BAR = 1e-12


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


@pytest.fixture(scope='module')
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', 0))


def _dummy_problem(eng, B):
    eng.upload(np.zeros((B, eng.H, eng.W), np.complex64), np.ones((eng.H, eng.W), np.uint8))


# ---- 1. the transform -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('H,W', O.GPU_SHAPES)
def test_dwt2_and_idwt2_against_the_oracle(P, torch, H, W, name, precision):
    """Psi, Psi^T and Psi^T Psi against the float64 oracle at L = 1 and the largest valid L; the in-place call equals the out-of-place call
    bit for bit."""
    from pnp_admm_cnc_mri_amd import utils_pnp as U
    v = O.field(H, W)
    B = len(v)
    real = np.float64 if precision == 'f64' else np.float32
    with P.Engine(H, W, Bmax=B, precision=precision) as eng:
        vt = _dev(torch, v.astype(real))
        for L in O.gpu_levels(name, H, W):
            eng.set_sparsity(name, L)
            assert eng.sparsity == (name, L)
            bars = (F64_BAR,) * 3 if precision == 'f64' else tuple(FREEDOM * b for b in DWT_F32[(H, W, name, L)])
            want = O.fwd(v, name, L)
            ct = U.dwt2(eng, vt)
            c = ct.cpu().numpy()
            c_in = want.astype(real)                                     # Psi^T is tested on the oracle's coefficients, not the card's
            back = U.idwt2(eng, _dev(torch, c_in)).cpu().numpy()
            round_trip = U.idwt2(eng, ct).cpu().numpy()
            errs = (rel_l2(c, want), rel_l2(back, O.inv(c_in, name, L)), rel_l2(round_trip, v))
            print('dwt2 %dx%d %s L=%d %s: rel-L2 Psi %.2e, Psi^T %.2e, Psi^T Psi %.2e (bars %.2e %.2e %.2e)' % (
                (H, W, name, L, precision) + errs + bars))
            assert c.dtype == real and all(e <= b for e, b in zip(errs, bars)), (errs, bars)
            for fn, src, ref in ((eng.dwt2, v.astype(real), c), (eng.idwt2, c_in, back)):
                t = _dev(torch, src)
                fn(t, t, B)
                eng.sync()
                assert np.array_equal(t.cpu().numpy(), ref)
        eng.set_sparsity(None)
        assert eng.sparsity == (None, 0)
        with pytest.raises(P._lib.PnpError) as e:
            eng.dwt2(vt, vt, B)
        assert e.value.code == -3                                         # PNP_E_STATE


# ---- 2. one prox step -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _prox_reference(kind, name, L, H, W):
    x, z, w = O.prox_inputs(H, W)
    if kind == 'l1':
        cu = O.fwd(x.astype(np.float64) + w, name, L)
        det = O.detail_mask(H, W, L)
        frac = float((np.abs(cu[:, det]) > O.PROX_L1_THR).mean())
        assert 0.05 < frac < 0.95, frac                                  # both branches of soft
        return O.prox_l1(x, z, w, O.PROX_L1_THR, name, L)
    p = O.PROX_CNC
    cz = O.fwd(z, name, L)
    det = O.detail_mask(H, W, L)
    clipped = float((np.abs(cz[:, det]) > 1.0 / p['b']).mean())
    thr = p['alpha'] * p['reo'] * p['lambda1']
    t = (1 - p['alpha']) * cz + p['alpha'] * O.fwd(x.astype(np.float64) + w, name, L) + thr * p['b'] * np.clip(cz, -1 / p['b'], 1 / p['b'])
    kept = float((np.abs(t[:, det]) > thr).mean())
    assert 0.02 < clipped < 0.98 and 0.02 < kept < 0.98, (clipped, kept)                 # both branches of clip and of soft
    zn, wn = O.prox_cnc(x, z, w, name=name, levels=L, **p)
    return zn, wn


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('name,L,H,W', O.PROX_CASES)
def test_prox_step_against_the_oracle(P, torch, name, L, H, W, kind):
    """prox_l1_dual / prox_cnc_dual with a wavelet set, from random x, z, w with both branches of soft and clip populated: z+ and w+
    against the float64 oracle, every element counted."""
    x, z, w = O.prox_inputs(H, W)
    B = len(x)
    want = _prox_reference(kind, name, L, H, W)
    with P.Engine(H, W, Bmax=B) as eng:
        _dummy_problem(eng, B)
        eng.set_sparsity(name, L)
        xt, zt, wt = (_dev(torch, a) for a in (x, z, w))
        if kind == 'l1':
            eng.prox_l1_dual(xt, zt, wt, O.PROX_L1_THR)
        else:
            p = O.PROX_CNC
            eng.prox_cnc_dual(xt, zt, wt, p['alpha'], p['lambda1'], p['reo'], p['b'])
        eng.sync()
        got = (zt.cpu().numpy(), wt.cpu().numpy())
        assert np.array_equal(xt.cpu().numpy(), x)
    errs = tuple(rel_l2(g, r) for g, r in zip(got, want))
    bars = tuple(FREEDOM * b for b in PROX_F32[(kind, name, L, H, W)])
    print('prox %s %s L=%d %dx%d: rel-L2 z+ %.2e, w+ %.2e (bars %.2e %.2e)' % ((kind, name, L, H, W) + errs + bars))
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)


# ---- 3. whole loops ---------------------------------------------------------------------------------------------------------------

ITERS, LEVELS, LOOP_B = 10, 3, 2


def _params(P, kind):
    p = dict(P.solvers.PRESETS['ADMM_L1' if kind == 'l1' else 'ADMM_CNC'])
    p.pop('iter_num')
    return p


def _run(eng, kind, p, iters, **kw):
    if kind == 'l1':
        return eng.admm_l1(iters, p['lambda1'], p['reo'], **kw)
    return eng.admm_cnc(iters, p['alpha'], p['lambda1'], p['reo'], p['b'], **kw)


@functools.lru_cache(maxsize=None)
def _problem(H, W, B=LOOP_B):
    return O.problem(B, H, W)


@functools.lru_cache(maxsize=None)
def _loop_reference(kind, name, H, W, params):
    y, mask, _ = _problem(H, W)
    return O.loop(y, mask, ITERS, kind, dict(params), name, LEVELS)[0]


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('H,W', [(128, 128), (256, 256)])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_loops_against_the_oracle(P, kind, name, H, W, precision):
    """10 iterations at the presets on a 30 % random mask, a piecewise-constant phantom and complex noise, L = 3: rel-L2 of x against the
    float64 oracle loop <= 1e-5 in float32, <= 1e-10 in double; 4 + 6 iterations through get_state equal 10 bit for bit."""
    y, mask, _ = _problem(H, W)
    p = _params(P, kind)
    want = _loop_reference(kind, name, H, W, tuple(sorted(p.items())))
    with P.Engine(H, W, Bmax=LOOP_B, precision=precision) as eng:
        eng.upload(y, mask)
        eng.set_sparsity(name, LEVELS)
        assert eng.plan['launches_per_iteration'] == 5 == eng.kernels_per_iteration
        eng.init_state()
        _run(eng, kind, p, ITERS)
        x = eng.x()
        state = eng.get_state()
        err = rel_l2(x, want)
        print('loop %s %s %dx%d %s (%s): rel-L2 of x after %d iterations %.3e' % (kind, name, H, W, precision, eng.ctx_path, ITERS, err))
        assert err <= (1e-10 if precision == 'f64' else 1e-5), err
        eng.init_state()
        _run(eng, kind, p, 4)
        z4, w4 = eng.get_state()
        eng.set_state(z4, w4)
        _run(eng, kind, p, 6)
        assert np.array_equal(eng.x(), x) and all(np.array_equal(a, b) for a, b in zip(eng.get_state(), state))


# ---- 4. traced runs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,precision', [(256, 256, 'f32'), (128, 160, 'f32'), (256, 256, 'f64')])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_traced_run(P, torch, kind, H, W, precision):
    """The rows of a traced run equal trace_rows(Engine.residuals(...)) of an untraced run stopped at the checked iteration; x, z, w are
    bit-equal to the untraced run; tol stops all slices together, at the first check every slice meets the rule."""
    from pnp_admm_cnc_mri_amd.engine import trace_rows, trace_meets
    B, K, every = 3, 7, 3
    y, mask, gt = _problem(H, W, B)
    p = _params(P, kind)
    real = np.float64 if precision == 'f64' else np.float32
    with P.Engine(H, W, Bmax=B, precision=precision) as eng:
        eng.upload(y, mask)
        eng.set_sparsity('db2', 3)
        eng.init_state()
        tr = _run(eng, kind, p, K, trace_every=every, gt=gt)
        traced = (eng.x(), *eng.get_state())
        assert list(tr['iter']) == [3, 6, 7] and tr['iters_done'] == K
        for row, k in enumerate(tr['iter']):
            eng.init_state()
            _run(eng, kind, p, int(k) - 1)
            zp = eng.get_state()[0] if k > 1 else None
            _run(eng, kind, p, 1)
            x, (z, w) = eng.x(), eng.get_state()
            rows = trace_rows(eng.residuals(*(_dev(torch, a.astype(real)) for a in (x, z, zp, w)), gt=gt), H * W)
            for n in ('r_pri', 'r_dual', 'x_norm', 'z_norm', 'w_norm', 're'):
                assert np.array_equal(tr[n][row], rows[n]), (k, n)
            assert np.abs(tr['psnr'][row] - rows['psnr']).max() <= 1e-9
        assert all(np.array_equal(a, b) for a, b in zip(traced, (x, z, w)))           # the last check is iteration K itself
        # the stopping rule: a tolerance that the slices meet at different checks
        eng.init_state()
        full = _run(eng, kind, p, K, trace_every=1)
        worse = np.maximum(full['r_pri'], full['r_dual'])                               # [K, B]
        tol = float(np.median(worse / full['z_norm'])) * (1 + 1e-9)
        met = worse <= tol * full['z_norm']                                             # the rule as the library evaluates it
        stop = next((k + 1 for k in range(K) if met[k].all()), K)
        first = [next((k + 1 for k in range(stop) if met[k, s]), 0) for s in range(B)]
        eng.init_state()
        tr = _run(eng, kind, p, K, tol=tol)
        print('traced %s %dx%d %s: tol %.3e stops at %d of %d, converged_at %s' % (kind, H, W, precision, tol, tr['iters_done'], K,
                                                                                 list(tr['converged_at'])))
        assert tr['iters_done'] == stop and list(tr['converged_at']) == first and len(tr['iter']) == stop
        assert np.array_equal(trace_meets({n: tr[n][-1] for n in ('r_pri', 'r_dual', 'z_norm')}, tol), met[stop - 1])
        stopped = (eng.x(), *eng.get_state())
        eng.init_state()
        _run(eng, kind, p, stop)
        assert all(np.array_equal(a, b) for a, b in zip(stopped, (eng.x(), *eng.get_state())))


# ---- 5. nothing else moved --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,path', [(64, 'slice'), (3, 'fused')])
def test_no_transform_is_what_it_was(P, B, path):
    """set_sparsity(None) after a wavelet run, on the slice-resident and the two-launch path: results bit-equal to a context that never
    had a wavelet, the path and the plan are back, and with the wavelet set the path reads 'fused' at five launches per iteration."""
    from pnp_admm_cnc_mri_amd import synthetic as S
    img, noise = S.batch(0, 4)
    img, noise = np.tile(img, (B // 4 + 1, 1, 1))[:B], np.tile(noise, (B // 4 + 1, 1, 1))[:B]
    mask = S.reference_masks()['Q_Random30'].astype(np.uint8)
    p = _params(P, 'cnc')
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, mask)
        assert eng.path_name == path and eng.sparsity == (None, 0)
        plan = eng.plan
        eng.init_state()
        _run(eng, 'cnc', p, 5)
        ref = (eng.x(), *eng.get_state())
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, mask)
        eng.set_sparsity('db4', 3)
        assert eng.path_name == 'fused' and eng.plan['launches_per_iteration'] == 5
        eng.init_state()
        _run(eng, 'cnc', p, 2)
        assert not np.array_equal(eng.x(), ref[0])
        eng.set_sparsity(None)
        assert eng.path_name == path and eng.plan == plan
        eng.init_state()
        _run(eng, 'cnc', p, 5)
        assert all(np.array_equal(a, b) for a, b in zip((eng.x(), *eng.get_state()), ref))


def test_solver_keyword_none_is_the_omitted_keyword(P):
    """ADMM_L1 / ADMM_CNC with transform=None and without the keyword return the same bits; a transform changes them."""
    y, mask, gt = _problem(256, 256)
    for solver, name in ((P.ADMM_L1, 'ADMM_L1'), (P.ADMM_CNC, 'ADMM_CNC')):
        opts = dict(P.solvers.PRESETS[name], iter_num=5)
        a = solver(mask, None, images=gt, y=y, **opts)
        b = solver(mask, None, images=gt, y=y, transform=None, levels=2, **opts)
        c = solver(mask, None, images=gt, y=y, transform='haar', levels=2, **opts)
        assert all(np.array_equal(a[n], b[n]) for n in range(LOOP_B))
        assert not np.array_equal(a[0], c[0])


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------

def test_solver_end_to_end(P, torch, tmp_path):
    """ADMM_L1(transform='db2', images=..., mask_id= over a bank of two masks, return_info=True): the log names the transform, its average
    PSNR is pnp_metrics of the returned x, and every slice follows its own mask."""
    B, H, W = 3, 256, 256
    y, mask, gt = _problem(H, W, B)
    rng = np.random.default_rng(5)
    bank = np.stack([mask, (rng.uniform(size=(H, W)) < 0.5).astype(np.uint8)])
    mid = np.array([0, 1, 0], np.int32)
    noises = (rng.standard_normal((H, W)) + 1j * rng.standard_normal((H, W))) * 0.5
    opts = dict(P.solvers.PRESETS['ADMM_L1'], iter_num=10)
    out, info = P.ADMM_L1(bank, noises, images=gt, mask_id=mid, transform='db2', levels=3, return_info=True, save_E=True,
                          results=str(tmp_path), testset_name='wv', **opts)
    x = np.stack([out[n] for n in range(B)]).astype(np.float32)
    with P.Engine(H, W, Bmax=B) as eng:
        _dummy_problem(eng, B)
        psnr, _ = eng.metrics(_dev(torch, x), gt)
    assert np.abs(psnr - np.asarray(info['psnr'])).max() <= 1e-9
    log = open(os.path.join(str(tmp_path), 'wv_dn_ADMM_L1', 'wv_dn_ADMM_L1.log')).read()
    assert 'sparsity transform: db2, 3 levels' in log
    assert 'Average PSNR:({:.3f})dB'.format(sum(info['psnr']) / B) in log and abs(float(np.mean(psnr)) - sum(info['psnr']) / B) <= 1e-9
    # the same call slice by slice with each slice's own mask gives the same reconstruction: mask_id reached the loop
    for n in (0, 1):
        one = P.ADMM_L1(bank[mid[n]], noises, images=gt[n:n + 1], transform='db2', levels=3, **opts)
        assert rel_l2(one[0], out[n]) <= 1e-5
    plain = P.ADMM_L1(bank, noises, images=gt, mask_id=mid, **opts)
    print('end to end: PSNR with db2 %s dB, pixel-domain %s dB' % (np.round(psnr, 2), np.round(
        [20 * np.log10(255.0 / np.sqrt(np.mean((plain[n] * 255 - gt[n]) ** 2))) for n in range(B)], 2)))
