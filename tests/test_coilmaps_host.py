"""CPU tests of the coil map estimation: csrc/coilmaps_plan.h through g++, plain and with sanitizers (tests/host/coilmaps_emulation.cpp:
the whole-slice restatement against a long-hand loop, the tile choice, the window, the patch indices at the image corners, the argument
rule); the binding and the argument checks of the library and of the solvers; the estimator's properties on the NumPy oracle."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import coilmaps_oracle as CM
import multicoil_oracle as M

SRC = os.path.join(ROOT, 'tests', 'host', 'coilmaps_emulation.cpp')
PLAIN = ['-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror']
SAN = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
E_ARG = -1
NEW = ('pnp_coilmaps_check', 'pnp_coil_maps', 'pnp_coil_maps_f64', 'pnp_coil_maps_stage_times')
# the issue's four CPU cases: (H, W, C, ncal, radius, power_iters)
CASES = [(128, 128, 4, 24, 2, 4), (128, 130, 8, 24, 3, 4), (128, 128, 8, 16, 1, 4), (140, 160, 5, 32, 2, 4)]
SHAPES = [(128, 128), (131, 128), (128, 130), (140, 160)]


# ---- coilmaps_plan.h under g++ ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_coilmaps_' + request.param) / 'coilmaps_emulation')
    subprocess.check_call(['g++'] + (PLAIN if request.param == 'plain' else SAN) + ['-o', out, SRC])
    return out


def _run(args):
    r = subprocess.run(args, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    return r.stdout.decode()


def test_slice_restatement_against_a_long_hand_loop(exe):
    """coilmaps_slice equals the loop restated in the emulation bit for bit (float and double, C = 1, 3, 5, every radius, 1 .. 3 power
    steps, with and without a support threshold); unit norm inside the support, +0 outside, v^H I real and >= 0."""
    assert _run([exe, 'slice']).strip() == 'ok slice'


@pytest.mark.parametrize('H,W', SHAPES)
def test_tile_choice_and_patch_indices_at_the_corners(exe, H, W):
    """every (C, radius, precision): the largest tile within 64 KiB or the smallest within 128 KiB, an odd slot stride; the staging walk
    fills the staged image once; every patch read of the four corner tiles stays inside it and lands on the wrapped pixel the plan names."""
    assert _run([exe, 'tiles', str(H), str(W)]).split() == ['ok', 'tiles', str(H), str(W)]


def test_window_symmetry_and_region(exe):
    assert _run([exe, 'window']).strip() == 'ok window'


def test_argument_rule_in_the_plan(exe):
    assert _run([exe, 'check']).strip() == 'ok check'


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def _lib():
    from pnp_admm_cnc_mri_amd import _lib as L
    return L


def test_binding_declares_the_coil_map_calls():
    lib = _lib()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read(), flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in lib.SIGNATURES, name
        assert hasattr(lib.lib(), name), name
    assert lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == lib.lib().pnp_abi_version()
    import pnp_admm_cnc_mri_amd as P
    for solver in (P.ADMM_L1, P.ADMM_CNC, P.PNP_ADMM_L1_D, P.PNP_ADMM_CNC_D, P.PNP_ADMM_CNC_DnCNN):
        sig = inspect.signature(solver).parameters
        assert (sig['maps_radius'].default, sig['maps_power_iters'].default, sig['maps_thresh'].default, sig['calib'].default) == (2, 4, 0.05, 24), solver
    sig = inspect.signature(P.coilmaps.estimate).parameters
    assert [sig[k].default for k in ('calib', 'radius', 'power_iters', 'thresh', 'precision', 'return_lambda')] == [24, 2, 4, 0.05, 'f32', False]
    assert P.estimate_coil_maps is P.coilmaps.estimate and hasattr(P.utils_pnp, 'estimate_coil_maps')
    assert hasattr(P.coilmaps, 'check') and hasattr(P.coilmaps, 'describe')


def test_every_rule_of_pnp_coilmaps_check():
    L = _lib().lib()
    for ok in ((1, 4, 0, 1, 0.0, 128, 128), (32, 64, 3, 16, 0.99, 1024, 1024), (5, 24, 2, 4, 0.05, 131, 140), (8, 5, 1, 2, 0.5, 128, 1024)):
        assert L.pnp_coilmaps_check(*ok) == 0, ok
    for bad, word in (((0, 24, 2, 4, 0.05, 128, 128), 'C must be'), ((33, 24, 2, 4, 0.05, 128, 128), 'C must be'),
                      ((8, 3, 2, 4, 0.05, 128, 128), 'ncal must be'), ((8, 65, 2, 4, 0.05, 128, 128), 'ncal must be'),
                      ((8, 24, -1, 4, 0.05, 128, 128), 'radius must be'), ((8, 24, 4, 4, 0.05, 128, 128), 'radius must be'),
                      ((8, 24, 2, 0, 0.05, 128, 128), 'power_iters must be'), ((8, 24, 2, 17, 0.05, 128, 128), 'power_iters must be'),
                      ((8, 24, 2, 4, -0.01, 128, 128), 'thresh must be'), ((8, 24, 2, 4, 1.0, 128, 128), 'thresh must be'),
                      ((8, 24, 2, 4, float('nan'), 128, 128), 'thresh must be'),
                      ((8, 24, 2, 4, 0.05, 127, 128), '[128, 1024]'), ((8, 24, 2, 4, 0.05, 128, 1025), '[128, 1024]')):
        assert L.pnp_coilmaps_check(*bad) == E_ARG, bad
        assert word in L.pnp_last_error().decode(), (bad, L.pnp_last_error())
    assert L.pnp_coil_maps(None, None, None, None, None, None, 1, 1, 24, 2, 4, 0.05) == E_ARG and 'ctx is null' in L.pnp_last_error().decode()


def test_solvers_refuse_before_any_engine_is_opened(monkeypatch):
    """coils='estimate' needs measured y= and takes no coil_id=; the bounds of the estimator, the limit of 32 on the (mixed) coil count and a
    hole in the calibration region are all ValueErrors before an Engine exists."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import coilmaps, solvers

    def no_engine(*a, **k):
        raise AssertionError('an engine was opened')
    monkeypatch.setattr(solvers, 'Engine', no_engine)
    m = np.ones((128, 128), np.uint8)
    y4, y40 = np.zeros((2, 4, 128, 128), np.complex64), np.zeros((1, 40, 128, 128), np.complex64)
    with pytest.raises(ValueError, match='needs y='):
        P.ADMM_CNC(m, None, coils='estimate')
    with pytest.raises(ValueError, match='needs y='):
        P.ADMM_L1(m, None, images=np.zeros((1, 128, 128), np.uint8), coils='estimate')
    with pytest.raises(ValueError, match='coil_id= cannot be given'):
        P.ADMM_CNC(m, None, y=y4, coils='estimate', coil_id=[0, 1])
    with pytest.raises(ValueError, match="or 'estimate'"):
        P.ADMM_CNC(m, None, y=y4, coils='espirit')
    for kw, word in ((dict(maps_radius=4), 'radius must be'), (dict(maps_radius=-1), 'radius must be'), (dict(maps_power_iters=0), 'power_iters must be'),
                     (dict(maps_power_iters=17), 'power_iters must be'), (dict(maps_thresh=1.0), 'thresh must be'), (dict(maps_thresh=-0.5), 'thresh must be'),
                     (dict(calib=3), 'ncal must be'), (dict(calib=65), 'ncal must be'), (dict(maps_radius=1.5), 'integers'), (dict(cg_iters=0), 'cg_iters')):
        with pytest.raises(ValueError, match=re.escape(word)):
            P.ADMM_CNC(m, None, y=y4, coils='estimate', **kw)
    with pytest.raises(ValueError, match='C must be'):                  # 40 channels need virtual_coils=
        P.ADMM_CNC(m, None, y=y40, coils='estimate')
    with pytest.raises(ValueError, match='C_out must be'):
        P.ADMM_CNC(m, None, y=y40, coils='estimate', virtual_coils=33)
    with pytest.raises(ValueError, match='noise_cov must be'):
        P.ADMM_CNC(m, None, y=y40, coils='estimate', virtual_coils=4, noise_cov=np.eye(39))
    with pytest.raises(ValueError, match='radius must be'):             # the estimator's bounds hold with mixing as well
        P.ADMM_CNC(m, None, y=y40, coils='estimate', virtual_coils=4, maps_radius=7)
    hole = m.copy()
    hole[127, 2] = 0                                                    # row 127 is calibration line 23, column 2 line 2
    with pytest.raises(ValueError, match=re.escape('calibration point (127, 2)')):
        P.ADMM_CNC(hole, None, y=y4, coils='estimate')
    bank = np.stack([m, hole])
    with pytest.raises(ValueError, match='mask 1 does not sample'):
        P.ADMM_L1(bank, None, y=y4, coils='estimate', mask_id=[0, 1])
    with pytest.raises(ValueError, match=re.escape('calibration point (127, 2)')):
        coilmaps.estimate(y4, hole)
    with pytest.raises(ValueError, match='radius must be'):
        coilmaps.estimate(y4, m, radius=4)
    with pytest.raises(ValueError, match=r'\[B,C,H,W\]'):
        coilmaps.estimate(y4[0], m)
    coilmaps.check_region(bank, [0, 0], 24)                             # the mask with the hole is not in use
    hole2 = m.copy()
    hole2[64, 64] = 0                                                   # outside the region: fine
    coilmaps.check_region(hole2, None, 24)


# ---- the estimator, on the oracle ---------------------------------------------------------------------------------------------------------

def _case(H, W, C, ncal):
    return CM.problem_cal(1, C, H, W, ncal)


def test_radius_0_one_step_is_the_sum_of_squares_map():
    """r = 0, n = 1: S = I / ||I|| (the classical low-resolution sum-of-squares maps), to 1e-15 per entry; C = 1: S = I / |I|."""
    img, S, m, nz, y = _case(128, 130, 5, 24)
    est, lam, sup, v, I = CM.estimate(y, m, 24, 0, 1, 0.0, full=True)
    assert sup.all() and np.abs(est - I / np.sqrt((np.abs(I) ** 2).sum(0))).max() <= 1e-15
    for r, n in ((0, 1), (2, 4)):
        est1, _, sup1, _, I1 = CM.estimate(y[:1], m, 24, r, n, 0.0, full=True)
        assert sup1.all() and np.abs(est1 - I1 / np.abs(I1)).max() <= 1e-14, (r, n)


@pytest.mark.parametrize('H,W,C,ncal,r,n', CASES)
def test_oracle_properties_on_the_four_cases(H, W, C, ncal, r, n):
    """Unit norm inside the support and exact zeros outside; v^H I(p) real and >= 0; a global phase on the DATA comes out as that phase on
    the maps; 4 power iterations are within 1e-7 of 12 (measured: 3.4e-11, 3.9e-10, 3.7e-14, 3.7e-12 on the four cases); the complex64
    restatement is 1.5 .. 1.8e-7 from the float64 form; the support contains every phantom pixel, and at most 2 pixels lie within 1e-3 of
    its threshold; the distance from the TRUE maps inside the body is the method's (5.9 %, 7.2 %, 11.5 %, 3.6 %)."""
    img, S, m, nz, y = _case(H, W, C, ncal)
    est, lam, sup, v, I = CM.estimate(y, m, ncal, r, n, 0.05, full=True)
    n2 = (np.abs(est) ** 2).sum(0)
    assert np.abs(n2[sup] - 1).max() <= 1e-14 and not est[:, ~sup].any() and 0 < sup.sum() < sup.size
    g = (np.conj(v) * I).sum(0)
    assert (g.real >= 0).all() and np.abs(g.imag).max() <= 1e-15 * np.abs(g).max()
    ph = np.exp(0.7j)
    est_ph = CM.estimate(ph * y, m, ncal, r, n, 0.05)
    assert M.rel(est_ph, ph * est) <= 1e-13
    est12 = CM.estimate(y, m, ncal, r, 12, 0.05)
    d12 = M.rel(est[:, sup], est12[:, sup])
    est32, lam32, sup32, _, _ = CM.estimate(y, m, ncal, r, n, 0.05, np.complex64, full=True)
    both = sup & sup32
    d32 = M.rel(est32[:, both], est[:, both])
    near = int((np.abs(lam / (0.05 ** 2 * lam.max()) - 1) < 1e-3).sum())
    body = img > 0
    dist = CM.aligned_distance(est, S, body)
    print('%dx%d C=%d %d/%d/%d: n=4 vs 12 %.2e, complex64 %.2e, near the threshold %d, support %.3f, from the true maps %.3f'
          % (H, W, C, ncal, r, n, d12, d32, near, sup.mean(), dist))
    assert d12 <= 1e-7 and d32 <= 1e-6 and near <= 2
    assert sup[body].all()
    assert dist <= 0.15


def test_a_hole_in_the_region_is_refused_by_the_oracle_as_well():
    img, S, m, nz, y = _case(128, 128, 4, 24)
    m = m.copy()
    m[1, 126] = 0
    assert CM.first_hole(m, 24) == (1, 126)
    with pytest.raises(ValueError, match=r'\(1, 126\)'):
        CM.lowres(y, m, 24)
