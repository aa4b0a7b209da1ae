"""CPU tests of the ESPIRiT coil map estimation: csrc/espirit_plan.h through g++, plain and with sanitizers (tests/host/espirit_emulation.cpp:
the argument rule, the index maps and LDS layouts for every valid size, the Gram kernel's staging walk against the plan's restatement, the
host stage on a matrix of known rank, the whole-slice restatement against a long-hand loop); the binding, the argument checks of the
library and of the solvers; the host pnp_espirit_kernels against numpy.linalg.eigh; the estimator's properties on the NumPy oracle."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import coilmaps_oracle as CM
import espirit_oracle as E
import multicoil_oracle as M

SRC = os.path.join(ROOT, 'tests', 'host', 'espirit_emulation.cpp')
PLAIN = ['-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-Werror']
SAN = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
E_ARG = -1
NEW = ('pnp_espirit_check', 'pnp_calib_patch_gram', 'pnp_calib_patch_gram_f64', 'pnp_espirit_kernels', 'pnp_espirit_eigmaps',
       'pnp_espirit_eigmaps_f64', 'pnp_espirit_maps', 'pnp_espirit_maps_f64', 'pnp_espirit_ranks', 'pnp_espirit_stage_times')
# the four prototype cases: (H, W, C, ncal, k), the distance from the true maps of Walsh (24 / 2 / 4 on the case's ncal) and of ESPIRiT
# (sigma = 0.02, converged) that the feature request states
CASES = [(128, 128, 4, 24, 4, 0.059, 0.031), (128, 130, 8, 24, 4, 0.066, 0.034), (140, 160, 5, 32, 5, 0.033, 0.019), (128, 128, 8, 16, 3, 0.118, 0.059)]
SIGMA, CROP, THRESH = 0.02, 0.9, 0.05


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_espirit_' + request.param) / 'espirit_emulation')
    subprocess.check_call(['g++'] + (PLAIN if request.param == 'plain' else SAN) + ['-o', out, SRC])
    return out


@pytest.mark.parametrize('mode', ['check', 'index', 'gram', 'kernels', 'slice'])
def test_plan_under_gxx(exe, mode):
    """the stand-alone program, run directly with nothing preloaded: see the head of tests/host/espirit_emulation.cpp for what each mode holds"""
    r = subprocess.run([exe, mode], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    assert r.stdout.decode().strip() == 'ok ' + mode


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------

def _lib():
    from pnp_admm_cnc_mri_amd import _lib as L
    return L


def test_binding_declares_the_espirit_calls_and_the_defaults():
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
        assert [sig[k].default for k in ('maps_method', 'maps_kernel', 'maps_sigma', 'maps_crop')] == ['walsh', 4, 0.02, 0.9], solver
    sig = inspect.signature(P.coilmaps.estimate).parameters
    assert [sig[k].default for k in ('method', 'kernel', 'sigma', 'crop')] == ['walsh', 4, 0.02, 0.9]
    assert 'radius' in P.coilmaps.estimate.__doc__ and 'IGNORED' in P.coilmaps.estimate.__doc__


def test_every_rule_of_pnp_espirit_check():
    L = _lib().lib()
    for ok in ((1, 4, 2, 1, 0.5, 0.0, 0.0, 128, 128), (32, 64, 2, 16, 0.02, 1.0, 0.99, 1024, 1024), (8, 24, 4, 8, 0.02, 0.9, 0.05, 128, 130),
               (2, 16, 8, 2, 0.02, 0.9, 0.05, 131, 128), (5, 32, 5, 4, 0.02, 0.9, 0.05, 140, 160)):
        assert L.pnp_espirit_check(*ok) == 0, ok
    for bad, word in (((0, 24, 4, 4, .02, .9, .05, 128, 128), 'C must be'), ((33, 24, 2, 4, .02, .9, .05, 128, 128), 'C must be'),
                      ((8, 3, 2, 4, .02, .9, .05, 128, 128), 'ncal must be'), ((8, 65, 4, 4, .02, .9, .05, 128, 128), 'ncal must be'),
                      ((8, 24, 1, 4, .02, .9, .05, 128, 128), 'kernel must be 2..8'), ((1, 24, 9, 4, .02, .9, .05, 128, 128), 'kernel must be 2..8'),
                      ((1, 5, 6, 4, .02, .9, .05, 128, 128), 'kernel must be <= ncal'),
                      ((9, 24, 4, 4, .02, .9, .05, 128, 128), 'C * kernel^2 must be <= 128'), ((32, 24, 3, 4, .02, .9, .05, 128, 128), 'virtual_coils='),
                      ((8, 24, 4, 0, .02, .9, .05, 128, 128), 'power_iters must be'), ((8, 24, 4, 17, .02, .9, .05, 128, 128), 'power_iters must be'),
                      ((8, 24, 4, 4, 0.0, .9, .05, 128, 128), 'sigma must be'), ((8, 24, 4, 4, 1.0, .9, .05, 128, 128), 'sigma must be'),
                      ((8, 24, 4, 4, float('nan'), .9, .05, 128, 128), 'sigma must be'),
                      ((8, 24, 4, 4, .02, -0.1, .05, 128, 128), 'crop must be'), ((8, 24, 4, 4, .02, 1.5, .05, 128, 128), 'crop must be'),
                      ((8, 24, 4, 4, .02, .9, -0.01, 128, 128), 'thresh must be'), ((8, 24, 4, 4, .02, .9, 1.0, 128, 128), 'thresh must be'),
                      ((8, 24, 4, 4, .02, .9, .05, 127, 128), '[128, 1024]'), ((8, 24, 4, 4, .02, .9, .05, 128, 1025), '[128, 1024]')):
        assert L.pnp_espirit_check(*bad) == E_ARG, bad
        assert word in L.pnp_last_error().decode(), (bad, L.pnp_last_error())
    assert L.pnp_espirit_maps(None, None, None, None, None, None, 1, 1, 24, 4, 4, 0.02, 0.9, 0.05) == E_ARG and 'ctx is null' in L.pnp_last_error().decode()
    assert L.pnp_espirit_eigmaps(None, None, None, None, None, 1, 1, 4, 4) == E_ARG and 'ctx is null' in L.pnp_last_error().decode()
    assert L.pnp_espirit_kernels(None, 1, 2, 0.02, None, None, None) == E_ARG and 'null pointer' in L.pnp_last_error().decode()
    assert L.pnp_calib_patch_gram(None, None, None, None, None, 1, 1, 128, 128, 24, 4) == E_ARG and 'null pointer' in L.pnp_last_error().decode()


def test_solvers_refuse_before_any_engine_is_opened(monkeypatch):
    """every ESPIRiT argument error is a ValueError before an Engine exists; coils='espirit' stays refused; the Walsh rules are untouched"""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import coilmaps, solvers

    def no_engine(*a, **k):
        raise AssertionError('an engine was opened')
    monkeypatch.setattr(solvers, 'Engine', no_engine)
    m = np.ones((128, 128), np.uint8)
    y4, y40 = np.zeros((2, 4, 128, 128), np.complex64), np.zeros((1, 40, 128, 128), np.complex64)
    with pytest.raises(ValueError, match="or 'estimate'"):
        P.ADMM_CNC(m, None, y=y4, coils='espirit')
    with pytest.raises(ValueError, match="'walsh' or 'espirit'"):
        P.ADMM_CNC(m, None, y=y4, coils='estimate', maps_method='grappa')
    for kw, word in ((dict(maps_kernel=1), 'kernel must be 2..8'), (dict(maps_kernel=9), 'kernel must be 2..8'), (dict(maps_kernel=6), 'C * kernel^2'),
                     (dict(maps_kernel=5, calib=4), 'kernel must be <= ncal'), (dict(maps_kernel=2.5), 'integers'),
                     (dict(maps_power_iters=17), 'power_iters must be'), (dict(maps_power_iters=0), 'power_iters must be'),
                     (dict(maps_sigma=0.0), 'sigma must be'), (dict(maps_sigma=1.0), 'sigma must be'), (dict(maps_crop=1.1), 'crop must be'),
                     (dict(maps_crop=-0.1), 'crop must be'), (dict(maps_thresh=1.0), 'thresh must be'), (dict(calib=3), 'ncal must be'),
                     (dict(cg_iters=0), 'cg_iters')):
        with pytest.raises(ValueError, match=re.escape(word)):
            P.ADMM_CNC(m, None, y=y4, coils='estimate', maps_method='espirit', **kw)
        with pytest.raises(ValueError, match=re.escape(word)):
            P.ADMM_L1(m, None, y=y4, coils='estimate', maps_method='espirit', **kw)
    with pytest.raises(ValueError, match='coil_id= cannot be given'):
        P.ADMM_CNC(m, None, y=y4, coils='estimate', maps_method='espirit', coil_id=[0, 1])
    with pytest.raises(ValueError, match='needs y='):
        P.ADMM_CNC(m, None, coils='estimate', maps_method='espirit')
    with pytest.raises(ValueError, match='C must be'):                  # 40 channels need virtual_coils=
        P.ADMM_CNC(m, None, y=y40, coils='estimate', maps_method='espirit')
    with pytest.raises(ValueError, match=re.escape('virtual_coils=')):  # 16 virtual coils at k = 4: 256 columns
        P.ADMM_CNC(m, None, y=y40, coils='estimate', maps_method='espirit', virtual_coils=16)
    with pytest.raises(ValueError, match='kernel must be 2..8'):         # the estimator's bounds hold with mixing as well
        P.ADMM_CNC(m, None, y=y40, coils='estimate', maps_method='espirit', virtual_coils=4, maps_kernel=11)
    # maps_radius is not used by 'espirit' -- and the ESPIRiT arguments are not looked at by 'walsh'
    with pytest.raises(ValueError, match='radius must be'):
        P.ADMM_CNC(m, None, y=y4, coils='estimate', maps_radius=4, maps_kernel=99, maps_sigma=7.0)
    hole = m.copy()
    hole[127, 2] = 0
    with pytest.raises(ValueError, match=re.escape('calibration point (127, 2)')):
        P.ADMM_CNC(hole, None, y=y4, coils='estimate', maps_method='espirit')
    with pytest.raises(ValueError, match=re.escape('calibration point (127, 2)')):
        coilmaps.estimate(y4, hole, method='espirit')
    with pytest.raises(ValueError, match='kernel must be 2..8'):
        coilmaps.estimate(y4, m, method='espirit', kernel=1)
    with pytest.raises(ValueError, match="'walsh' or 'espirit'"):
        coilmaps.estimate(y4, m, method='sos')
    coilmaps.check(4, 24, 99, 4, 0.05, 128, 128, method='espirit')      # radius is ignored
    with pytest.raises(ValueError, match='radius must be'):
        coilmaps.check(4, 24, 99, 4, 0.05, 128, 128)
    info = dict(method='espirit', calib=24, kernel=4, sigma=0.02, crop=0.9, thresh=0.05, power_iters=4, radius=2, rank=[31, 33], support=[0.4, 0.5])
    line = coilmaps.describe(info)
    assert 'ESPIRiT' in line and 'kernel 4' in line and 'rank 31 .. 33' in line and '45.0 %' in line
    assert 'ESPIRiT' not in coilmaps.describe(dict(calib=24, radius=2, power_iters=4, thresh=0.05, support=[0.4]))


# ---- the estimator, on the oracle ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(H, W, Cn, ncal, k, n):
    img, S, m, nz, y = CM.problem_cal(1, Cn, H, W, ncal)
    return img, S, m, y, E.estimate(y, m, ncal, k, n, SIGMA, CROP, THRESH, full=True)


@pytest.mark.parametrize('H,W,Cn,ncal,k,walsh,espirit', CASES)
def test_oracle_properties_on_the_four_cases(H, W, Cn, ncal, k, walsh, espirit):
    """Measured (converged = 30 power steps; 4 steps in brackets): distance from the true maps inside the body 3.1 % (3.3), 3.4 % (3.5),
    1.3 % (1.3), 5.9 % (6.6) against Walsh's 5.9 %, 6.6 %, 3.7 %, 11.8 %; the largest eigenvalue is 0.995 .. 1.000 in the body; the
    support holds the whole phantom and 11 .. 22 % of the background; ||G S x - S x|| / ||S x|| = 0.36 %, 0.51 %, 0.33 %, 0.60 %; unit
    norm inside the support, exact zeros outside, v^H I >= 0; the nearest singular value is 1.9 .. 2.3 % from the cut."""
    img, S, m, y, o = _case(H, W, Cn, ncal, k, 30)
    body = img > 0
    dist = CM.aligned_distance(o['v'], S, body)
    o4 = _case(H, W, Cn, ncal, k, 4)[4]
    dist4 = CM.aligned_distance(o4['v'], S, body)
    dwalsh = CM.aligned_distance(CM.estimate(y, m, ncal, 2, 4, 0.05, full=True)[3], S, body)
    Sx = S * img[None]
    G = E.operator(o['w'], H, W)
    fix = float(np.linalg.norm(np.einsum('abyx,byx->ayx', G, Sx) - Sx) / np.linalg.norm(Sx))
    assert np.abs(G - np.conj(G.transpose(1, 0, 2, 3))).max() == 0.0          # Hermitian by construction
    near = float(np.min(np.abs(o['sing'] / (SIGMA * o['sing'][0]) - 1)))
    print('%dx%d C=%d ncal=%d k=%d: from the true maps %.4f (4 steps %.4f; Walsh %.4f), lambda in the body %.4f .. %.4f, rank %d (nearest to '
          'the cut %.3f), background kept %.3f, ||G S - S|| / ||S|| %.4f' % (H, W, Cn, ncal, k, dist, dist4, dwalsh, o['lam'][body].min(),
                                                                             o['lam'].max(), o['rank'], near, o['sup'][~body].mean(), fix))
    assert dist <= 2 * espirit and dist4 <= 2 * espirit and dwalsh <= 2 * walsh
    assert dist < dwalsh and dist4 < dwalsh                                  # ESPIRiT is closer than Walsh
    assert o['lam'][body].min() >= 0.99 and o4['lam'][body].min() >= 0.99 and o['lam'].max() <= 1 + 1e-9
    assert o['sup'][body].all() and o4['sup'][body].all() and o['sup'][~body].mean() <= 0.30
    assert fix <= 0.01
    assert near >= 1e-6
    for r in (o, o4):
        n2 = (np.abs(r['maps']) ** 2).sum(0)
        assert np.abs(n2[r['sup']] - 1).max() <= 1e-14 and not r['maps'][:, ~r['sup']].any() and 0 < r['sup'].sum() < r['sup'].size
        g = (np.conj(r['v']) * r['I']).sum(0)
        assert (g.real >= 0).all() and np.abs(g.imag).max() <= 1e-15 * np.abs(g).max()


@pytest.mark.parametrize('H,W,Cn,ncal,k,walsh,espirit', CASES)
def test_host_kernels_against_eigh_on_the_same_gram(H, W, Cn, ncal, k, walsh, espirit):
    """pnp_espirit_kernels (cyclic Jacobi) against the oracle's w from numpy.linalg.eigh on the SAME Gram matrix: P depends on the subspace
    alone, so the two agree to rounding -- measured 3 .. 6e-14 of ||w||, bar 1e-11 (the cut's nearest neighbour is 2 % away; a gap of g
    amplifies the eigenvectors' rounding by about 1 / g); the singular values to 1e-12 of the largest; the same rank."""
    L = _lib().lib()
    o = _case(H, W, Cn, ncal, k, 4)[4]
    n, D = Cn * k * k, 2 * k - 1
    g = np.ascontiguousarray(o['gram'])
    w, rank, sing = np.full((Cn, Cn, D, D), np.nan, np.complex128), C.c_int(-1), np.full(n, np.nan)
    assert L.pnp_espirit_kernels(g.ctypes.data_as(C.c_void_p), Cn, k, SIGMA, w.ctypes.data_as(C.c_void_p), C.byref(rank),
                                 sing.ctypes.data_as(C.c_void_p)) == 0
    dw, ds = M.rel(w, o['w']), float(np.abs(sing - o['sing']).max() / o['sing'][0])
    print('C=%d k=%d n=%d: rank %d, w %.2e, singular values %.2e' % (Cn, k, n, rank.value, dw, ds))
    assert rank.value == o['rank'] and dw <= 1e-11 and ds <= 1e-12
    for c in range(Cn):
        for c2 in range(Cn):
            assert np.array_equal(w[c2, c], np.conj(w[c, c2][::-1, ::-1])), (c, c2)
    bad = g.copy()
    bad[0, 0] = np.nan
    assert L.pnp_espirit_kernels(bad.ctypes.data_as(C.c_void_p), Cn, k, SIGMA, w.ctypes.data_as(C.c_void_p), C.byref(rank),
                                 sing.ctypes.data_as(C.c_void_p)) == E_ARG and 'non-finite' in L.pnp_last_error().decode()


def test_complex64_restatement_and_gram_order_sensitivity():
    """the two yardsticks of the GPU tests on the second case: the complex64 restatement is 1.1e-7 (maps) and 1.3e-6 (lambda) from the
    float64 form; the maps from the Gram matrix summed in reverse patch order are 9e-14 away"""
    H, W, Cn, ncal, k = CASES[1][:5]
    img, S, m, y, o = _case(H, W, Cn, ncal, k, 4)
    o32 = E.estimate(y.astype(np.complex64), m, ncal, k, 4, SIGMA, CROP, THRESH, np.complex64, full=True)
    both = o32['sup'] & o['sup']
    d32, l32 = M.rel(o32['maps'][:, both], o['maps'][:, both]), M.rel(o32['lam'], o['lam'])
    rev = E.estimate(y, m, ncal, k, 4, SIGMA, CROP, THRESH, full=True, reverse=True)
    drev = M.rel(rev['v'], o['v'])
    print('complex64 restatement: maps %.2e, lambda %.2e; reverse patch order: %.2e' % (d32, l32, drev))
    assert o32['maps'].dtype == np.complex64 and o32['lam'].dtype == np.float32
    assert d32 <= 1e-6 and l32 <= 1e-5 and drev <= 1e-11
    assert (o32['sup'] != o['sup']).mean() <= 1e-3


def test_a_hole_in_the_region_is_refused_by_the_oracle_as_well():
    img, S, m, y, _ = _case(*CASES[0][:5], 4)
    m = m.copy()
    m[1, 126] = 0
    with pytest.raises(ValueError, match=r'\(1, 126\)'):
        E.gram(y, m, 24, 4)
