"""GPU tests of the convergence trace and the residual-based stopping rule (pnp_admm_*_run_traced, pnp_residuals, the trace_every= /
tol= keywords of the five solvers).  Every number printed before an assertion is what the card gave (DESIGN.md section 11 quotes them)."""
import json
import os

import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import GOLD

pytestmark = pytest.mark.gpu

NAMES = ('r_pri', 'r_dual', 'x_norm', 'z_norm', 'w_norm')
L1 = dict(lambda1=0.1, reo=0.015)                                  # S1:171
CNC = dict(alpha=0.45, lambda1=0.5, reo=0.05, b=64)                # S4:176
MASKS = ('Q_Random30', 'Q_Radial30', 'Q_Cartesian30')


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


def _run(eng, solver, iters, **kw):
    if solver == 'cnc':
        return eng.admm_cnc(iters, CNC['alpha'], CNC['lambda1'], CNC['reo'], CNC['b'], **kw)
    return eng.admm_l1(iters, L1['lambda1'], L1['reo'], **kw)


def _norm(a):
    return np.sqrt((np.asarray(a, np.float64).reshape(len(a), -1) ** 2).sum(1))


def _rows_of_states(x, z, w, zp):
    x, z, w, zp = (np.asarray(a, np.float64) for a in (x, z, w, zp))
    return dict(r_pri=_norm(x - z), r_dual=_norm(z - zp), x_norm=_norm(x), z_norm=_norm(z), w_norm=_norm(w))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the kernel alone
# ------------------------------------------------------------------------------------------------------------------------------------
def _sums(x, z, zp, w, gt, quantise=False):
    B = len(x)
    x, z, zp, w = (a.reshape(B, -1) for a in (x, z, zp, w))
    x64, z64, zp64, w64, g64 = (a.astype(np.float64) for a in (x, z, zp, w, gt.reshape(B, -1)))
    xq = (np.round(x * x.dtype.type(255)) * (x.dtype.type(1) / x.dtype.type(255))).astype(np.float64) if quantise else x64      # pnp_mri.h
    return np.stack([((x64 - z64) ** 2).sum(1), ((z64 - zp64) ** 2).sum(1), (x64 ** 2).sum(1), (z64 ** 2).sum(1), (w64 ** 2).sum(1),
                     ((xq * 255.0 - g64) ** 2).sum(1), (g64 ** 2).sum(1)])


@pytest.mark.parametrize('H,W,B,precision', [(256, 256, 1, 'f32'), (256, 256, 3, 'f32'), (256, 256, 64, 'f32'), (256, 256, 512, 'f32'),
                                             (218, 170, 3, 'f32'), (321, 255, 2, 'f32'), (256, 256, 3, 'f64'), (321, 255, 2, 'f64')])
def test_residual_kernel_against_numpy(P, H, W, B, precision):
    """pnp_residuals on random tensors: every sum within 1e-12 relative of NumPy's float64 sums of the same arrays (the kernel accumulates in
    double; only the order of the additions differs), with and without a ground truth, plain and quantised; two calls give identical bits; a
    device-side output equals the host-side one."""
    import torch
    rng = np.random.default_rng(H + B)
    real = np.float64 if precision == 'f64' else np.float32
    x, z, zp, w = (rng.uniform(-1, 1, (B, H, W)).astype(real) for _ in range(4))
    x = np.abs(x)
    gt = rng.integers(0, 256, (B, H, W), dtype=np.uint8)
    dev = torch.device('cuda', 0)
    xt, zt, zpt, wt = (torch.from_numpy(a).to(dev) for a in (x, z, zp, w))
    with P.Engine(H, W, Bmax=B, precision=precision) as eng:
        eng.upload(np.zeros((B, H, W), np.complex64), np.ones((H, W), np.uint8))
        for quantise in (False, True):
            got = eng.residuals(xt, zt, zpt, wt, gt=gt, quantise=quantise)
            want = _sums(x, z, zp, w, gt, quantise)
            err = np.abs(got / want - 1).max()
            print('residuals %dx%d B=%d %s quantise=%d: max rel err %.2e' % (H, W, B, precision, quantise, err))
            assert err <= 1e-12, err
            assert np.array_equal(got, eng.residuals(xt, zt, zpt, wt, gt=gt, quantise=quantise))
        out = torch.full((7, B), -1.0, dtype=torch.float64, device=dev)
        eng.residuals(xt, zt, zpt, wt, gt=torch.from_numpy(gt).to(dev), quantise=True, out=out)
        eng.sync()
        assert np.array_equal(out.cpu().numpy(), got)
        bare = eng.residuals(xt, zt, zpt, wt)
        assert np.array_equal(bare[:5], got[:5]) and (bare[5:] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. / 6. the traced run is the untraced run, and a row does not depend on `every`
# ------------------------------------------------------------------------------------------------------------------------------------
def _batch(P, H, W, B):
    from pnp_admm_cnc_mri_amd import synthetic as S
    if (H, W) == (256, 256):
        m = S.reference_masks()
        masks = np.stack([m[k] for k in MASKS]).astype(np.uint8)
    else:
        masks = np.stack([O.synthetic_mask(k, H, W) for k in ('random', 'radial', 'cartesian')])
    n = min(B, 8)
    img, noise = S.batch(0, n, H, W)
    reps = (B + n - 1) // n
    return np.tile(img, (reps, 1, 1))[:B], np.tile(noise, (reps, 1, 1))[:B], masks, (np.arange(B) % 3).astype(np.int32)


CASES = [('slice', 256, 256, 64, 'f32'), ('slice', 256, 256, 512, 'f32'), ('fused', 256, 256, 3, 'f32'), ('fused', 256, 256, 3, 'f64'),
         ('fused', 256, 256, 4, 'f32'), ('fused', 256, 256, 4, 'f64'), ('fused', 512, 512, 2, 'f32'), ('fused', 512, 512, 3, 'f32'),
         ('generic', 218, 170, 2, 'f32')]

# The two-launch engines (256 x 256 float and double, 512 x 512) pack two slices into one complex transform, and with untraced calls a run
# cut into launches is NOT bit-identical to one launch for the LAST slice of an ODD batch there (profiles/experiments/
# trace_split_vs_single.txt: 15 iterations, B = 3, slice 2 off by 1.5e-6 for L1 and 3.0e-5 for CNC; every other slice and path: 0).  The
# traced run on those engines therefore never cuts the chain (api.hip, run_traced_chain): the B = 3 cases below are the check of that.


@pytest.mark.parametrize('path,H,W,B,precision', CASES)
@pytest.mark.parametrize('solver', ['l1', 'cnc'])
def test_traced_run_is_bit_identical_to_the_untraced_run(P, solver, path, H, W, B, precision):
    """K iterations traced (every = 1 and 7, with and without a ground truth) leave x, z, w bit-equal to the untraced K iterations -- on
    the slice-resident, two-launch, double, 512 x 512 and any-size paths; and the rows of the iterations both traces check are equal
    bit for bit.  Odd batches on the two-launch engines are the cases in which a run cut into launches would differ (note above CASES)."""
    K = 15
    img, noise, masks, mid = _batch(P, H, W, B)
    gt = np.round(img * 255).astype(np.uint8)
    with P.Engine(H, W, Bmax=B, precision=precision) as eng:
        eng.synthesize(img, noise, masks, mid)
        assert eng.path_name == path
        eng.init_state()
        assert _run(eng, solver, K) is None
        ref = (eng.x(), *eng.get_state())
        traces = {}
        for every, with_gt in ((1, True), (7, False)):
            eng.init_state()
            tr = _run(eng, solver, K, trace_every=every, gt=gt if with_gt else None)
            got = (eng.x(), *eng.get_state())
            diff = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, ref)]
            off = sorted({int(i) for a, b in zip(got, ref) for i in np.flatnonzero((a != b).reshape(B, -1).any(1))})
            print('%s %s %dx%d B=%d %s every=%d: max |traced - untraced| of x, z, w = %s, slices that differ: %s' % (
                solver, path, H, W, B, precision, every, diff, off))
            assert all(np.array_equal(a, b) for a, b in zip(got, ref)), diff
            assert tr['iters_done'] == K and list(tr['iter']) == ([k for k in range(every, K + 1, every)] + ([K] if K % every else []))
            assert (tr['converged_at'] == 0).all() and ('psnr' in tr) == with_gt
            assert all(np.isfinite(tr[n]).all() and tr[n].shape == (len(tr['iter']), B) for n in NAMES)
            traces[every] = tr
        psnr, re = eng.metrics(None, gt)
        assert np.abs(traces[1]['psnr'][-1] - psnr).max() <= 1e-9 and np.abs(traces[1]['re'][-1] - re).max() <= 1e-9
        for k in (7, 14, 15):
            for n in NAMES:
                assert np.array_equal(traces[1][n][list(traces[1]['iter']).index(k)], traces[7][n][list(traces[7]['iter']).index(k)]), (k, n)


@pytest.mark.parametrize('path,B', [('slice', 64), ('fused', 3), ('fused', 4)])
@pytest.mark.parametrize('solver', ['l1', 'cnc'])
def test_rows_do_not_depend_on_every(P, solver, path, B):
    """The rows of iterations 7, 14 and 21 from every = 7 equal the same rows from every = 1 bit for bit (same path, same batch)."""
    img, noise, masks, mid = _batch(P, 256, 256, B)
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, masks, mid)
        assert eng.path_name == path
        eng.init_state()
        t1 = _run(eng, solver, 21, trace_every=1)
        eng.init_state()
        t7 = _run(eng, solver, 21, trace_every=7)
    assert list(t7['iter']) == [7, 14, 21] and list(t1['iter']) == list(range(1, 22))
    for c, k in enumerate((7, 14, 21)):
        for n in NAMES:
            print('%s %s B=%d k=%d %s: relative difference per slice %s' % (solver, path, B, k, n, np.abs(t7[n][c] / t1[n][k - 1] - 1)))
    for c, k in enumerate((7, 14, 21)):
        for n in NAMES:
            assert np.array_equal(t7[n][c], t1[n][k - 1]), (k, n, t7[n][c], t1[n][k - 1])


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. the rows are the norms of the states the run really held
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path,B', [('slice', 64), ('fused', 3), ('fused', 4)])
@pytest.mark.parametrize('solver', ['l1', 'cnc'])
def test_rows_are_the_norms_of_the_states(P, solver, path, B):
    """Untraced runs of k - 1 and k iterations give x_k, z_k, w_k and z_{k-1} on the host; every entry of row k equals NumPy's float64 norm
    of those arrays to 1e-12 relative (k = 5 and 20)."""
    img, noise, masks, mid = _batch(P, 256, 256, B)
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, masks, mid)
        assert eng.path_name == path
        eng.init_state()
        tr = _run(eng, solver, 20, trace_every=1)
        for k in (5, 20):
            eng.init_state()
            _run(eng, solver, k - 1)
            zp, _ = eng.get_state()
            eng.init_state()
            _run(eng, solver, k)
            x = eng.x()
            z, w = eng.get_state()
            want = _rows_of_states(x, z, w, zp)
            for n in NAMES:
                got = tr[n][k - 1]
                err = np.abs(got - want[n]) / np.where(want[n] > 0, want[n], 1.0)
                print('%s %s k=%d %s: max rel err %.2e (min value %.3e)' % (solver, path, k, n, err.max(), want[n].min()))
                assert (np.abs(got - want[n]) <= 1e-12 * want[n]).all(), (k, n, err.max())


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. against the float64 oracle
# ------------------------------------------------------------------------------------------------------------------------------------
def _oracle_rows(y, mask, solver, ks, gray=None, f32=False):
    """rows of the oracle's loop at the iterations ks: the float64 reference, or (f32) the same NumPy lines in complex64 / float32 as
    oracle.admm_l1_f32 / admm_cnc_f32 run them -- the precision control"""
    if f32:
        y = y.astype(np.complex64)
    x, z, w = O.init_state(y, np.float32 if f32 else np.float64)
    rows = {}
    for i in range(max(ks)):
        zp = z
        p = L1 if solver == 'l1' else CNC
        x = O.dc_step(z, w, y, mask, p['reo'])
        z, w = O.l1_step(x, z, w, p['lambda1'], p['reo']) if solver == 'l1' else O.cnc_step(x, z, w, p['alpha'], p['lambda1'], p['reo'], p['b'])
        if f32:
            assert x.dtype == z.dtype == w.dtype == np.float32
        if (i + 1) in ks:
            r = {n: float(v[0]) for n, v in _rows_of_states(x[None], z[None], w[None], zp[None]).items()}
            if gray is not None:
                r['psnr'] = O.calculate_psnr(np.asarray(x, np.float64) * 255, gray)
            rows[i + 1] = r
    return rows


def _deviation(rows, ref):
    """largest relative deviation of any entry beyond the bar's absolute allowance 1e-6 * x_norm (an entry whose reference is exactly zero --
    ADMM_L1's r_pri once x == z in float64 -- has no relative deviation and is held by the absolute term alone)"""
    worst = 0.0
    for k in ref:
        for n in NAMES:
            if ref[k][n] > 0:
                worst = max(worst, max(abs(rows[k][n] - ref[k][n]) - 1e-6 * ref[k]['x_norm'], 0.0) / ref[k][n])
    return worst


@pytest.mark.parametrize('solver,ks', [('l1', (1, 2, 5, 10, 50, 100)), ('cnc', (1, 2, 5, 10, 20, 35))])
def test_rows_against_the_float64_oracle(P, golden_inputs, solver, ks, tmp_path):
    """Float contexts on the golden inputs (three masks, committed presets): |got - want| <= rtol want + 1e-6 x_norm per entry, rtol =
    max(4 x the oracle's own float32 control, 2e-5) computed here on the CPU; psnr rows within 0.01 dB of the oracle's, the last one and
    re equal to the solver's info to 1e-9."""
    gray = golden_inputs['gray']
    masks = np.stack([golden_inputs['masks'][k] for k in MASKS]).astype(np.uint8)
    img_L = O.requantise(gray)
    ref, ctl = [], []
    for m in masks:
        y = O.synthesize(img_L, m.astype(np.float64), golden_inputs['noises'])
        ref.append(_oracle_rows(y, m, solver, ks, gray))
        ctl.append(_oracle_rows(y, m, solver, ks, f32=True))
    control = max(_deviation(c, r) for c, r in zip(ctl, ref))
    rtol = max(4 * control, 2e-5)
    solve = P.ADMM_L1 if solver == 'l1' else P.ADMM_CNC
    opts = dict(L1 if solver == 'l1' else CNC, iter_num=max(ks))
    _, info = solve(masks, golden_inputs['noises'], images=np.stack([gray] * 3), mask_id=np.arange(3), results=str(tmp_path),
                    return_info=True, trace_every=1, **opts)
    tr = info['trace']
    worst = 0.0
    for b in range(3):
        for k in ks:
            for n in NAMES:
                got, want = tr[n][k - 1, b], ref[b][k][n]
                if want > 0:
                    worst = max(worst, abs(got - want) / want)
                assert abs(got - want) <= rtol * want + 1e-6 * ref[b][k]['x_norm'], (b, k, n, got, want, rtol)
            assert abs(tr['psnr'][k - 1, b] - ref[b][k]['psnr']) <= 0.01, (b, k)
    print('%s: float32 control %.2e -> rtol %.2e; worst relative deviation of a GPU row %.2e' % (solver, control, rtol, worst))
    assert np.abs(tr['psnr'][-1] - info['psnr']).max() <= 1e-9 and np.abs(tr['re'][-1] - info['re']).max() <= 1e-9


@pytest.mark.parametrize('solver', ['l1', 'cnc'])
def test_rows_against_the_float64_oracle_in_double(P, golden_inputs, solver, tmp_path):
    """Double contexts: 1e-9 want + 1e-12 x_norm at k = 1, 2, 5, 10, 20, 35, 50, 100."""
    ks = (1, 2, 5, 10, 20, 35, 50, 100)
    masks = np.stack([golden_inputs['masks'][k] for k in MASKS]).astype(np.uint8)
    img_L = O.requantise(golden_inputs['gray'])
    ys = np.stack([O.synthesize(img_L, m.astype(np.float64), golden_inputs['noises']) for m in masks])
    ref = [_oracle_rows(y, m, solver, ks) for y, m in zip(ys, masks)]
    solve = P.ADMM_L1 if solver == 'l1' else P.ADMM_CNC
    opts = dict(L1 if solver == 'l1' else CNC, iter_num=max(ks))
    _, info = solve(masks, None, y=ys, mask_id=np.arange(3), results=str(tmp_path), return_info=True, trace_every=1, precision='f64', **opts)
    tr, worst = info['trace'], 0.0
    for b in range(3):
        for k in ks:
            for n in NAMES:
                got, want = tr[n][k - 1, b], ref[b][k][n]
                if want > 0:
                    worst = max(worst, abs(got - want) / want)
                assert abs(got - want) <= 1e-9 * want + 1e-12 * ref[b][k]['x_norm'], (b, k, n, got, want)
    print('%s f64: worst relative deviation of a GPU row %.2e' % (solver, worst))


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. stopping
# ------------------------------------------------------------------------------------------------------------------------------------
TOL = 2.1e-3


def _oracle_ratios(ys, mask, solver, iters):
    out = np.empty((iters, len(ys)))
    for b, y in enumerate(ys):
        rows = _oracle_rows(y, mask, solver, tuple(range(1, iters + 1)))
        out[:, b] = [max(rows[k]['r_pri'], rows[k]['r_dual']) / rows[k]['z_norm'] for k in range(1, iters + 1)]
    return out


def test_stopping_rule_admm_l1(P, golden_inputs):
    """ADMM_L1 preset, Q_Random30, six synthetic slices, iter_num = 60, tol = 2.1e-3: from the float64 oracle, every = 1 must stop at 33 and
    every = 5 at 35 (the oracle's worst ratio clears tol by >= 1 % on either side of both: asserted first), converged_at is the oracle's
    first-met iteration per slice, and x equals the untraced run of that many iterations bit for bit."""
    mask = golden_inputs['masks']['Q_Random30'].astype(np.uint8)
    ys = np.stack([O.synthetic_problem(b, mask)[1] for b in range(6)])
    ratio = _oracle_ratios(ys, mask, 'l1', 60)
    met = ratio <= TOL
    worst = ratio.max(1)
    assert all(abs(worst[k - 1] / TOL - 1) >= 0.01 for k in (32, 33, 30, 35))             # the batch's stop: >= 1 % either side of tol
    # converged_at is per slice: no slice's ratio at any iteration sits within 1e-4 of tol -- ten times the ~1e-5 a float32 run moves it
    assert (np.abs(ratio / TOL - 1) >= 1e-4).all(), np.abs(ratio / TOL - 1).min()
    stops = {}
    for every in (1, 5):
        checked = [k for k in range(every, 61, every)]
        stops[every] = next(k for k in checked if met[k - 1].all())
        first = [next((k for k in checked if k <= stops[every] and met[k - 1, b]), 0) for b in range(6)]
        stops[every] = (stops[every], first)
    assert stops[1][0] == 33 and stops[5][0] == 35, stops
    print('oracle: worst ratio at 32, 33: %.4e %.4e; at 30, 35: %.4e %.4e' % tuple(ratio[k - 1].max() for k in (32, 33, 30, 35)))
    with P.Engine(256, 256, Bmax=6) as eng:
        eng.upload(ys.astype(np.complex64), mask)
        for every in (1, 5):
            want_done, want_first = stops[every]
            eng.init_state()
            tr = eng.admm_l1(60, L1['lambda1'], L1['reo'], trace_every=every, tol=TOL)
            x = eng.x()
            print('every=%d: iters_done %d converged_at %s (oracle %s)' % (every, tr['iters_done'], list(tr['converged_at']), want_first))
            assert tr['iters_done'] == want_done and list(tr['iter']) == list(range(every, want_done + 1, every))
            assert list(tr['converged_at']) == want_first
            eng.init_state()
            eng.admm_l1(want_done, L1['lambda1'], L1['reo'])
            assert np.array_equal(x, eng.x())
        eng.init_state()
        tr = eng.admm_l1(60, L1['lambda1'], L1['reo'], tol=TOL)                  # tol alone: a check every iteration
        assert tr['iters_done'] == 33 and len(tr['iter']) == 33


def test_stopping_rule_never_met_by_the_cnc_preset(P, golden_inputs):
    """The CNC preset does not settle: with the same tol the run goes to iter_num and no slice ever meets the rule (oracle: the smallest
    ratio of the six slices over 60 iterations stays above 1.5 x tol)."""
    mask = golden_inputs['masks']['Q_Random30'].astype(np.uint8)
    ys = np.stack([O.synthetic_problem(b, mask)[1] for b in range(6)])
    ratio = _oracle_ratios(ys, mask, 'cnc', 60)
    print('oracle: smallest CNC ratio %.4e at iteration %d' % (ratio.min(), 1 + int(np.argmin(ratio.min(1)))))
    assert ratio.min() >= 1.01 * TOL
    with P.Engine(256, 256, Bmax=6) as eng:
        eng.upload(ys.astype(np.complex64), mask)
        eng.init_state()
        tr = eng.admm_cnc(60, CNC['alpha'], CNC['lambda1'], CNC['reo'], CNC['b'], trace_every=1, tol=TOL)
    assert tr['iters_done'] == 60 and (tr['converged_at'] == 0).all() and len(tr['iter']) == 60


def test_early_stop_reaches_the_solver_outputs(P, golden_inputs, tmp_path):
    """ADMM_L1(tol=) returns out, metrics, PNGs and log lines of iteration iters_done, and one extra log line says so."""
    mask = golden_inputs['masks']['Q_Random30'].astype(np.uint8)
    probs = [O.synthetic_problem(b, mask) for b in range(6)]
    imgs, ys = np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs])
    kw = dict(images=imgs, y=ys, return_info=True, save_E=True, **L1)
    out, info = P.ADMM_L1(mask, None, results=str(tmp_path / 'a'), testset_name='stop', tol=TOL, iter_num=60, **kw)
    assert info['trace']['iters_done'] == 33
    ref, ref_info = P.ADMM_L1(mask, None, results=str(tmp_path / 'b'), testset_name='stop33', iter_num=33, **kw)
    assert all(np.array_equal(out[b], ref[b]) for b in range(6)) and info['psnr'] == ref_info['psnr'] and info['re'] == ref_info['re']
    assert np.abs(info['trace']['psnr'][-1] - info['psnr']).max() <= 1e-9
    log = open(str(tmp_path / 'a' / 'stop_dn_ADMM_L1' / 'stop_dn_ADMM_L1.log')).read()
    assert log.count('stopped after iteration 33 of 60') == 1
    assert 'stopped after' not in open(str(tmp_path / 'b' / 'stop33_dn_ADMM_L1' / 'stop33_dn_ADMM_L1.log')).read()


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. PnP: rows are the norms of the loop's tensors, and as close to the oracle's as the states are
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pnp_env():
    import torch
    from pnp_admm_cnc_mri_amd import solvers_pnp
    assert torch.cuda.is_available()
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    return dict(torch=torch, S=solvers_pnp, known=json.load(open(os.path.join(GOLD, 'pnp_known.json')))['known50'])


def _pnp_case(case, env, golden_inputs):
    from conftest import weights50, weights_trained
    S, known = env['S'], env['known']

    def opts(tag):
        o = dict(known[tag + '_opts'])
        o['iter_num'] = 10
        return o
    if case == 'cnc_ffdnet_contractive':
        return (lambda **kw: S.PNP_ADMM_CNC_D('ffdnet_gray', **kw)), opts('cnc_d_ffdnet_gray'), weights50('ffdnet_gray'), True
    if case == 'cnc_ffdnet_trained':
        return (lambda **kw: S.PNP_ADMM_CNC_D('ffdnet_gray', **kw)), opts('trained_cnc_d_ffdnet_gray'), weights_trained(), True
    if case == 'l1_ffdnet':
        return (lambda **kw: S.PNP_ADMM_L1_D('ffdnet_gray', **kw)), opts('l1_d_ffdnet_gray'), weights50('ffdnet_gray'), False
    return (lambda **kw: S.PNP_ADMM_CNC_DnCNN('dncnn_25', 'dncnn_15', **kw)), opts('cnc_dncnn_pair'), weights50('dncnn_25'), True


@pytest.mark.parametrize('case', ['cnc_ffdnet_contractive', 'cnc_ffdnet_trained', 'l1_ffdnet', 'dncnn_pair'])
def test_pnp_rows_are_the_norms_of_the_loop_tensors(pnp_env, golden_inputs, case, tmp_path):
    """Rows 3 and 10 of a traced 10-iteration run (every = 1) against the states x_k, z_k, w_k, z_{k-1} of the same loop: 1e-12 relative.
    The state of iteration 10 is the untraced run's (info['z'], info['w'], out).  The networks' noise-level schedule is a function of
    iter_num, so an untraced run of j < 10 iterations is a DIFFERENT loop; the state after iteration j of THIS loop comes from a run that
    the stopping rule ends there (tol = 1e30 at every = j: the first check is met) -- the reductions only read, the loop is the same.
    For the two FFDNet CNC cases the rows are also held against oracle.pnp_admm_cnc with the same network on the CPU, by the triangle
    inequality on the states: nothing measured goes into the bar."""
    solve, opts, sd, pair = _pnp_case(case, pnp_env, golden_inputs)
    gray = golden_inputs['gray']
    mask = golden_inputs['masks']['Q_Random30'].astype(np.float64)
    kw = dict(mask=mask, noises=golden_inputs['noises'], images=gray[None], model=sd, results=str(tmp_path), return_info=True, **opts)

    def unpack(res):
        return (res[0], res[-1])                                       # (out, info) of (out, info) / (out, psnr1, info)
    out, info = unpack(solve(trace_every=1, **kw))
    tr = info['trace']
    assert list(tr['iter']) == list(range(1, 11)) and tr['iters_done'] == 10
    states = {10: (out[0], info['z'][0], info['w'][0])}
    plain_out, plain = unpack(solve(**kw))
    assert np.array_equal(plain_out[0], out[0]) and np.array_equal(plain['z'], info['z']) and np.array_equal(plain['w'], info['w'])
    assert abs(tr['psnr'][-1, 0] - info['psnr'][0]) <= 1e-9 and abs(tr['re'][-1, 0] - info['re'][0]) <= 1e-9
    for j in (2, 3, 9):
        o, i = unpack(solve(trace_every=j, tol=1e30, **kw))
        assert i['trace']['iters_done'] == j and list(i['trace']['converged_at']) == [j]
        states[j] = (o[0], i['z'][0], i['w'][0])
    for k in (3, 10):
        (x, z, w), zp = states[k], states[k - 1][1]
        want = _rows_of_states(x[None], z[None], w[None], zp[None])
        for n in NAMES:
            got = tr[n][k - 1, 0]
            print('%s k=%d %s: got %.12e want %.12e' % (case, k, n, got, want[n][0]))
            assert abs(got - want[n][0]) <= 1e-12 * want[n][0], (k, n)
    if case == 'cnc_ffdnet_trained':
        print('psnr row of the trained FFDNet:', np.round(tr['psnr'][:, 0], 2))
        assert int(np.argmax(tr['psnr'][:, 0])) < 9                    # the loop peaks before its last iteration
    if case.startswith('cnc_ffdnet'):
        torch = pnp_env['torch']
        den = pnp_env['S']._load_model('ffdnet_gray', sd, 'model_zoo', 10, golden_inputs['noises'], False, None, torch.device('cpu'),
                                       cnn_backend='torch')

        def denoise(a, i):
            with torch.no_grad():
                return den(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None], i)[0, 0].numpy()
        y = O.synthesize(O.requantise(gray), mask, golden_inputs['noises'])
        _, rec = O.pnp_admm_cnc(y, mask, denoise, 10, opts['alpha'], opts['lambda1'], opts['reo'], opts['b'], trace=(2, 3, 9, 10))
        n2 = lambda a: float(np.linalg.norm(np.asarray(a, np.float64)))
        for k in (3, 10):
            (x, z, w), zp = states[k], states[k - 1][1]
            (xr, zr, wr), zpr = rec[k], rec[k - 1][1]
            ref = {n: v[0] for n, v in _rows_of_states(xr[None], zr[None], wr[None], zpr[None]).items()}
            dx, dz, dw, dzp = n2(x - xr), n2(z - zr), n2(w - wr), n2(zp - zpr)
            bars = dict(r_pri=dx + dz, r_dual=dz + dzp, x_norm=dx, z_norm=dz, w_norm=dw)
            for n in NAMES:
                got = tr[n][k - 1, 0]
                print('%s k=%d %s: |got - oracle| %.3e, bar %.3e' % (case, k, n, abs(got - ref[n]), bars[n] + 1e-9 * ref['x_norm']))
                assert abs(got - ref[n]) <= bars[n] + 1e-9 * ref['x_norm'], (k, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# 10. errors
# ------------------------------------------------------------------------------------------------------------------------------------
def test_trace_errors(P, golden_inputs):
    import ctypes as C
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    dev = torch.device('cuda', 0)
    t = [torch.zeros((2, 256, 256), device=dev) for _ in range(4)]
    out = torch.zeros((7, 2), dtype=torch.float64, device=dev)
    with P.Engine(256, 256, Bmax=2) as eng:
        with pytest.raises(_lib.PnpError) as e:                        # before a problem is uploaded
            eng.residuals(*t)
        assert e.value.code == -3
        eng.upload(np.zeros((2, 256, 256), np.complex64), np.ones((256, 256), np.uint8))
        with pytest.raises(_lib.PnpError) as e:                        # the run needs a state
            eng.admm_l1(5, 0.1, 0.015, trace_every=1)
        assert e.value.code == -3
        eng.init_state()
        with pytest.raises(ValueError):
            eng.admm_l1(5, 0.1, 0.015, trace_every=-2)
        n, d = C.c_int(7), C.c_int(7)
        assert L.pnp_admm_l1_run_traced(eng._ctx, 5, 0.1, 0.015, 0, 0.0, None, 0, C.byref(n), C.byref(d)) == -1       # every < 1: PNP_E_ARG
        assert b'every' in L.pnp_last_error()
        assert L.pnp_admm_cnc_run_traced(eng._ctx, 5, 0.45, 0.5, 0.05, 64.0, -3, 0.0, None, 0, C.byref(n), C.byref(d)) == -1
        x64 = torch.zeros((2, 256, 256), dtype=torch.float64, device=dev)
        with pytest.raises(_lib.PnpError) as e:                        # out aliases an input
            eng.residuals(x64, t[1], t[2], t[3], out=x64)
        assert e.value.code == -1 and 'alias' in str(e.value)
        with pytest.raises(_lib.PnpError) as e:
            eng.residuals(t[0], None, t[2], t[3], out=out)
        assert e.value.code == -1
        assert eng.admm_l1(0, 0.1, 0.015, trace_every=1)['iters_done'] == 0          # iters = 0: zero checks, the untraced behaviour
        z, _ = eng.get_state()
        assert np.array_equal(eng.x(), z)
    with P.Engine(256, 256, Bmax=2, precision='f64') as eng:
        eng.upload(np.zeros((2, 256, 256), np.complex128), np.ones((256, 256), np.uint8))
        assert L.pnp_residuals(eng._ctx, *[C.c_void_p(a.data_ptr()) for a in t], None, 0, 0, C.c_void_p(out.data_ptr()), 1) == -3     # float call, double context
    with pytest.raises(ValueError, match='return_info'):
        P.ADMM_CNC(np.ones((256, 256)), np.zeros((256, 256), complex), images=np.zeros((1, 256, 256), np.uint8), trace_every=2)
