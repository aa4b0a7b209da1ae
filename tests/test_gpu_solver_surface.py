"""The five solver entry points, locked against the commit before their shared drivers (solvers.py: _solve, solvers_pnp.py: _solve_pnp).

tests/golden/solver_surface.json was recorded ONCE, at that commit, by running `run_case` of this module twice per case; every case here
runs again on the code as it stands and must give the same

    type and length of the returned tuple and of `out`, list(info.keys()), the names of the files written, the log file's lines (time
    stamp removed, every decimal number replaced by '#'; the integers -- coil counts, iteration numbers -- stay), the ordered list of
    Engine / Denoiser methods called around and in the loop (no call more per iteration, none less), and the numbers: out, info['z'],
    info['w'], psnr1 and the metrics of info.

The numbers: where the two recorded runs agreed bit for bit (`rel` 0 in the JSON) the array must be bit-equal to them -- the JSON has the
SHA-256 of its bytes, and solver_surface.npz every eighth pixel of it, compared first so that a failure shows its size.  (Whole arrays of
every case would be 6 MB of fixtures.)  Where they did not, the npz has the whole array of the first run and the bar is ten times the
recorded relative L2 distance of the two runs.

128 x 128, B = 2, C = 2, 2 iterations, cnn_backend='hip', the committed trained weights; one case at 256 x 256 (the fixed-size engine)."""
import functools
import hashlib
import json
import os
import re

import numpy as np
import pytest

import coilmix_oracle as CO
import multicoil_oracle as M
from conftest import GOLD, rel_l2, weights_trained

pytestmark = pytest.mark.gpu

B, C, ITERS, CALIB = 2, 2, 2, 16
PLAIN = {'ADMM_L1': dict(iter_num=ITERS, lambda1=0.1, reo=0.015),                                                   # S1:171
         'ADMM_CNC': dict(iter_num=ITERS, alpha=0.45, lambda1=0.5, reo=0.05, b=64)}                                 # S4:176
PNP = {'PNP_ADMM_L1_D': (('ffdnet_gray',), 'ffdnet_gray', dict(iter_num=ITERS, reo=0.25)),                          # S3:343
       'PNP_ADMM_CNC_D': (('ffdnet_gray',), 'ffdnet_gray', dict(iter_num=ITERS, alpha=0.9, lambda1=1.35, reo=0.45, b=0.3)),    # S6:573
       'PNP_ADMM_CNC_DnCNN': (('dncnn_25', 'dncnn_15'), 'dncnn_25', dict(iter_num=ITERS, alpha=1.2, lambda1=4, reo=0.45, b=0.3))}   # S6:571
SOLVERS = tuple(PLAIN) + tuple(PNP)
ENGINE_CALLS = ('admm_l1', 'admm_cnc', 'dc_step', 'add', 'cnc_combine', 'dual_clamp', 'residuals', 'get_state')


@functools.lru_cache(maxsize=None)
def scene(n):
    """-> (mask [n,n] with the calibration square, imgs [B,n,n] float32 on the 1/255 grid, noise [n,n], maps [C,n,n], y [B,C,n,n])"""
    mask = (M.mask(n, n, n).astype(bool) | CO.cal_region(CALIB, n, n)).astype(np.uint8)
    imgs = np.stack([M.phantom(40 + b, n, n) for b in range(B)])
    S = M.coil_maps(C, n, n, 3)
    y = np.stack([M.synthesize(imgs[b], S, mask, M.noise(b, C, mask, 0.5)) for b in range(B)])
    return mask, imgs, M.noise_full(1, (n, n), 2.0), S, y


def inputs(kind, n=128):
    mask, imgs, noise, S, y = scene(n)
    if kind == 'images':
        return mask, noise, dict(images=imgs)
    coils = dict(coils=S) if kind == 'coils' else dict(coils='estimate', virtual_coils=C, calib=CALIB)
    return mask, None, dict(y=y, images=imgs, **coils)


def state0():
    """a state as it might stand after iteration 1: z near the images, w small"""
    _, imgs, _, _, _ = scene(128)
    return imgs.copy(), np.float32(0.02) * imgs[::-1]


#        id                      solver               inputs     further keywords
CASES = ([(s + '-images', s, 'images', {}) for s in SOLVERS] + [(s + '-coils', s, 'coils', {}) for s in SOLVERS] + [
    ('ADMM_CNC-estimate', 'ADMM_CNC', 'estimate', {}),
    ('PNP_ADMM_L1_D-estimate', 'PNP_ADMM_L1_D', 'estimate', {}),
    ('ADMM_L1-complex', 'ADMM_L1', 'coils', dict(image='complex')),
    ('ADMM_CNC-haar-spin', 'ADMM_CNC', 'images', dict(transform='haar', spin='random')),
    ('ADMM_L1-tol', 'ADMM_L1', 'images', dict(trace_every=1, tol=10.0)),                  # met at the first check: stops after iteration 1
    ('PNP_ADMM_CNC_D-tol', 'PNP_ADMM_CNC_D', 'images', dict(trace_every=1, tol=10.0)),
    ('PNP_ADMM_L1_D-resume', 'PNP_ADMM_L1_D', 'images', dict(state0=state0, iter_start=1)),
    ('ADMM_CNC-device', 'ADMM_CNC', 'images', dict(return_device=True)),
    ('PNP_ADMM_CNC_D-device', 'PNP_ADMM_CNC_D', 'images', dict(return_device=True)),
    ('ADMM_CNC-256', 'ADMM_CNC', 'images', dict(n=256)),
])
IDS = [c[0] for c in CASES]


def spy(setattr_, calls):
    """wrap the loop's Engine and Denoiser methods (setattr_: monkeypatch.setattr) so that each call appends its name to `calls`"""
    from pnp_admm_cnc_mri_amd import denoisers as D
    from pnp_admm_cnc_mri_amd.engine import Engine

    def wrap(cls, attr, label):
        inner = getattr(cls, attr)

        def outer(self, *a, **kw):
            calls.append(label)
            return inner(self, *a, **kw)
        setattr_(cls, attr, outer)
    for name in ENGINE_CALLS:
        wrap(Engine, name, name)
    wrap(D.Denoiser, '__call__', 'Denoiser.__call__')
    wrap(D.Denoiser, 'select_bank', 'select_bank')


def log_lines(text):
    """the log file's lines without the time stamp, every decimal number replaced by '#'"""
    lines = [re.sub(r'^\d\d-\d\d-\d\d \d\d:\d\d:\d\d\.\d{3} : ', '', ln) for ln in text.splitlines()]
    return [re.sub(r'-?\d+\.\d+(?:[eE][-+]?\d+)?', '#', ln) for ln in lines]


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def sample(a):
    """every eighth pixel of an image stack; a short vector whole"""
    return a[..., ::8, ::8] if a.ndim >= 3 else a


def run_case(case, results, setattr_):
    """One solve of CASES' `case` writing under `results`.  -> (what the JSON holds of it, {name: array})"""
    import torch
    import pnp_admm_cnc_mri_amd as P
    _, solver, kind, more = CASES[IDS.index(case)]
    more = dict(more)
    mask, noises, kw = inputs(kind, more.pop('n', 128))
    if 'state0' in more:
        more['state0'] = more['state0']()
    kw.update(more, results=str(results), save_E=True, return_info=True)
    calls = []
    spy(setattr_, calls)
    if solver in PLAIN:
        res = getattr(P, solver)(mask, noises, **kw, **PLAIN[solver])
    else:
        names, weights, opts = PNP[solver]
        res = getattr(P, solver)(*names, mask, noises, model=weights_trained(weights), cnn_backend='hip', **kw, **opts)
    out, info = res[0], res[-1]
    rec = dict(result=[type(res).__name__, len(res)], info_keys=list(info.keys()), calls=calls)
    arrays = {}
    if isinstance(out, torch.Tensor):
        rec['out'] = ['Tensor', str(out.dtype), list(out.shape)]
        arrays['out'] = out.cpu().numpy()
    else:
        rec['out'] = [type(out).__name__, len(out)]
        arrays['out'] = np.stack([np.asarray(o) for o in out[:B]])
        arrays['out_rest'] = np.stack([np.asarray(o) for o in out[B:]])          # the unused slots of the pre-sized list
    if len(res) == 3:
        rec['psnr1'] = [type(res[1]).__name__, len(res[1])]
        arrays['psnr1'] = np.asarray(res[1], np.float64)
    for k in ('z', 'w', 'psnr', 'ssim', 're', 'cg_residual'):
        if k in info and len(info[k]):
            arrays[k] = np.asarray(info[k])
    if 'trace' in info:
        tr = info['trace']
        rec['trace'] = dict(keys=list(tr.keys()), iter=[int(v) for v in tr['iter']], iters_done=int(tr['iters_done']),
                            converged_at=[int(v) for v in tr['converged_at']])
    files = sorted(os.path.relpath(os.path.join(d, f), str(results)) for d, _, fs in os.walk(str(results)) for f in fs)
    rec['files'] = files
    rec['log'] = []
    for f in files:
        if f.endswith('.log'):
            with open(os.path.join(str(results), f)) as fh:
                rec['log'] += log_lines(fh.read())
    return rec, arrays


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLD, 'solver_surface.json')) as f:
        return json.load(f)['cases'], np.load(os.path.join(GOLD, 'solver_surface.npz'))


def test_every_case_is_recorded(golden):
    assert sorted(golden[0]) == sorted(IDS)


@pytest.mark.parametrize('case', IDS)
def test_the_surface_is_what_it_was(case, golden, tmp_path, monkeypatch):
    want, npz = golden[0][case], golden[1]
    got, arrays = run_case(case, tmp_path, monkeypatch.setattr)
    for k in ('result', 'out', 'psnr1', 'info_keys', 'files', 'log', 'calls', 'trace'):
        assert got.get(k) == want.get(k), k
    assert sorted(arrays) == sorted(want['arrays'])
    for name, a in arrays.items():
        rule, gold = want['arrays'][name], npz[case + '/' + name]
        assert [a.dtype.str, list(a.shape)] == rule['type'], name
        if rule['rel'] == 0.0:                                       # the two recorded runs were bit-equal: so is this one
            s = sample(a)
            assert np.array_equal(s, gold), (name, float(np.abs(s - gold).max()))
            assert digest(a) == rule['sha256'], name
        else:
            err = rel_l2(a, gold)
            print('%s %s: %.3e from the recorded run; the two recorded runs differed by %.3e' % (case, name, err, rule['rel']))
            assert err <= 10 * rule['rel'], (name, err, rule['rel'])
