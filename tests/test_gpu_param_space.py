"""The ADMM_L1 / ADMM_CNC loops of every kernel family across their parameter space, per element (tests/param_space_oracle.py).

Every other loop test runs the z / w update and the data-consistency blend at the committed presets, on natural images, and compares
whole-image norms.  Here every engine runs ten CNC points and five L1 points -- alpha in {0, 1, 1.5}, lambda1 = 0, b = 0.5 (clip never
active) and 1e4 (always active), reo from 1e-3 to 100 -- from a state with z of both signs over four decades, and x, z+ and w+ are compared
per element and per slice with the float64 oracle:

  float engines    max |got - ref| <= max(FREEDOM x the float32 NumPy restatement's own distance, FLOOR) x max |ref|
  double engines   max |got - ref| <= F64_BAR x max |ref|

The float32 distances are the committed constants S.BARS_F32, measured on the CPU against the float64 oracle and never against a kernel;
FREEDOM is the suite's margin for another order of the sums (tests/test_gpu_wavelet.py, tests/test_gpu_anysize_sweep.py), FLOOR the 2e-6
the suite holds one dc_step to.  B = 3: the last pair of the paired engines is half empty; slices 0 and 1 share a pair and have different
masks.  Every case prints its worst ratio to the bar (pytest -s)."""
import numpy as np
import pytest

import param_space_oracle as S

pytestmark = pytest.mark.gpu

FREEDOM, FLOOR, F64_BAR = S.FREEDOM, S.FLOOR, S.F64_BAR          # 4 x the float32 distance, floor 2e-6; 1e-12 in double (S.bar)
KNOBS = ('PNP_SLICE', 'PNP_SLICE_MIN_B', 'PNP_FUSED_COLS', 'PNP_FUSED_L1_TWO_STATE')

S256, S512, SANY = (256, 256), (512, 512), (218, 170)
# name: shape, environment knobs, fast path, precision, pnp_path_name, pnp_ctx_path, solvers
ENGINES = {
    'slice':              (S256, {'PNP_SLICE': '1'}, 1, 'f32', 'slice', 'slice', ('cnc', 'l1')),
    'slice_l1_two_state': (S256, {'PNP_SLICE': '1', 'PNP_FUSED_L1_TWO_STATE': '1'}, 1, 'f32', 'slice', 'slice', ('l1',)),
    'fused256':           (S256, {'PNP_SLICE': '0'}, 1, 'f32', 'fused', 'fused', ('cnc', 'l1')),
    'fused256_l1_two_state': (S256, {'PNP_SLICE': '0', 'PNP_FUSED_L1_TWO_STATE': '1'}, 1, 'f32', 'fused', 'fused', ('l1',)),
    'split_chain':        (S256, {'PNP_SLICE': '0', 'PNP_FUSED_COLS': '2'}, 1, 'f32', 'fused', 'fused', ('cnc', 'l1')),
    'fused512':           (S512, {}, 1, 'f32', 'fused', 'fused', ('cnc', 'l1')),
    'generic256':         (S256, {}, 0, 'f32', 'generic', 'generic', ('cnc', 'l1')),
    'anysize':            (SANY, {}, 1, 'f32', 'generic', 'anysize', ('cnc', 'l1')),
    'f64_fused256':       (S256, {}, 1, 'f64', 'fused', 'fused', ('cnc', 'l1')),
    'f64_generic256':     (S256, {}, 0, 'f64', 'generic', 'generic', ('cnc', 'l1')),
    'f64_anysize':        (SANY, {}, 1, 'f64', 'generic', 'anysize', ('cnc', 'l1')),
}
ENGINE_KINDS = [(name, kind) for name, e in ENGINES.items() for kind in e[6]]
SWITCH_ENGINES = ('slice', 'fused256', 'fused512')


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


def open_engine(P, monkeypatch, name):
    """a fresh context of engine `name` with the problem of its shape uploaded"""
    shape, env, fast, precision, path, ctx_path, _ = ENGINES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    y, masks, mid = S.problem(S.B, *shape)
    eng = P.Engine(shape[0], shape[1], Bmax=S.B, precision=precision)
    try:
        eng.set_fast_path(fast)
        eng.upload(y, masks, mid)
        assert eng.path_name == path and eng.ctx_path == ctx_path, (name, eng.path_name, eng.ctx_path)
    except BaseException:
        eng.close()
        raise
    return eng


def run(eng, kind, point, iters):
    if kind == 'cnc':
        eng.admm_cnc(iters, *point)
    else:
        eng.admm_l1(iters, *point)


def compare(got, ref, key, f64, label, bad):
    """-> the worst ratio of max |got - ref| to its bar over x, z, w and the slices; cases beyond their bar are appended to `bad`"""
    worst = 0.0
    for k, name in enumerate('xzw'):
        if got[k] is None:
            continue
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (label, name)
        bar = S.bar(key, k, f64)
        ratio = S.distance(got[k], ref[k]) / bar
        worst = max(worst, float(ratio.max()))
        print('    %-60s %s %.3f' % (label, name, float(ratio.max())))
        for s in np.flatnonzero(~(ratio <= 1.0)):
            bad.append('%s %s slice %d: %.3g x its bar of %.3g' % (label, name, s, ratio[s], bar[s]))
    return worst


def report(what, worst, bad):
    print('\nparam-space %s: worst ratio to the bar %.3f' % (what, worst))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('name,kind', ENGINE_KINDS)
def test_one_teacher_forced_step_per_element(P, monkeypatch, name, kind):
    """(a) set_state(z, w) of the designed state, ONE iteration at every point, x, z+ and w+ per element against the float64 step."""
    shape, f64 = ENGINES[name][0], ENGINES[name][3] == 'f64'
    z0, w0 = S.state(S.B, *shape)
    worst, bad = 0.0, []
    with open_engine(P, monkeypatch, name) as eng:
        for idx in range(len(S.POINTS[kind])):
            eng.set_state(z0, w0)
            run(eng, kind, S.params(kind, idx), 1)
            got = (eng.x(),) + tuple(eng.get_state())
            key = (kind, idx, shape, 'step')
            worst = max(worst, compare(got, S.reference(*key), key, f64, '%s %s point %d %r step' % (name, kind, idx, S.params(kind, idx)), bad))
    report('%s %s step' % (name, kind), worst, bad)


@pytest.mark.parametrize('name,kind', ENGINE_KINDS)
def test_five_iterations_per_element(P, monkeypatch, name, kind):
    """(b) init_state and five iterations at every point: an expansive point is held to its own float32 growth."""
    shape, f64 = ENGINES[name][0], ENGINES[name][3] == 'f64'
    worst, bad = 0.0, []
    with open_engine(P, monkeypatch, name) as eng:
        for idx in range(len(S.POINTS[kind])):
            eng.init_state()
            run(eng, kind, S.params(kind, idx), S.LOOP_ITERS)
            got = (eng.x(),) + tuple(eng.get_state())
            key = (kind, idx, shape, 'loop')
            worst = max(worst, compare(got, S.reference(*key), key, f64, '%s %s point %d %r loop' % (name, kind, idx, S.params(kind, idx)), bad))
    report('%s %s loop' % (name, kind), worst, bad)


@pytest.mark.parametrize('sw', range(len(S.SWITCHES)))
@pytest.mark.parametrize('name', SWITCH_ENGINES)
def test_parameters_changed_between_calls_do_not_outlive_their_call(P, monkeypatch, name, sw):
    """(c) k1 iterations at point A, then k2 at point B on the same context and the same upload, nothing read in between: bit-equal to a
    fresh context that is handed the intermediate state and runs the k2 iterations, and within (b)'s bars of the oracle doing the same.
    What a call derives from its parameters -- the u buffer of the single-state L1 form, the resident share of w, the blend coefficients,
    the prox scalars -- must not reach the next call."""
    (ka, ia), (kb, ib) = S.SWITCHES[sw]
    k1, k2 = S.SWITCH_K
    shape = ENGINES[name][0]
    with open_engine(P, monkeypatch, name) as eng:
        eng.init_state()
        run(eng, ka, S.params(ka, ia), k1)
        run(eng, kb, S.params(kb, ib), k2)
        got = (eng.x(),) + tuple(eng.get_state())
    with open_engine(P, monkeypatch, name) as eng:
        eng.init_state()
        run(eng, ka, S.params(ka, ia), k1)
        z1, w1 = eng.get_state()
    with open_engine(P, monkeypatch, name) as eng:
        eng.set_state(z1, w1)
        run(eng, kb, S.params(kb, ib), k2)
        fresh = (eng.x(),) + tuple(eng.get_state())
    for arr, a, b in zip('xzw', got, fresh):
        assert np.array_equal(a, b), (name, S.SWITCHES[sw], arr, int((a != b).sum()), float(np.abs(a - b).max()))
    bad = []
    key = ('switch', sw, shape, 'loop')
    worst = compare(got, S.reference(*key), key, False, '%s %s%d -> %s%d' % (name, ka, ia, kb, ib), bad)
    report('%s switch %s%d -> %s%d' % (name, ka, ia, kb, ib), worst, bad)


@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_one_point_through_the_solver_entry_points(P, monkeypatch, tmp_path, precision):
    """(d) ADMM_CNC(alpha=, lambda1=, reo=, b=) and ADMM_L1(lambda1=, reo=) on measured y= at a point that is no preset (CNC 9: reo = 100,
    b = 8; L1 3: lambda1 = 100, reo = 1e-3), five iterations, x per element against the oracle loop at (b)'s bars."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    y, masks, mid = S.problem(S.B, *S256)
    f64 = precision == 'f64'
    worst, bad = 0.0, []
    for kind, idx, fn in (('cnc', 9, P.ADMM_CNC), ('l1', 3, P.ADMM_L1)):
        point = S.params(kind, idx)
        opts = dict(zip(('alpha', 'lambda1', 'reo', 'b') if kind == 'cnc' else ('lambda1', 'reo'), point), iter_num=S.LOOP_ITERS)
        out = fn(masks, None, y=y, mask_id=mid, results=str(tmp_path), precision=precision, **opts)
        x = np.stack(out[:S.B])
        assert x.dtype == np.float64
        key = (kind, idx, S256, 'loop')
        worst = max(worst, compare((x, None, None), S.reference(*key), key, f64, 'ADMM_%s %s' % (kind.upper(), precision), bad))
    report('entry points %s' % precision, worst, bad)
