"""CPU tests of the plug-and-play solvers on complex images (image='complex' on PNP_ADMM_L1_D / PNP_ADMM_CNC_D / PNP_ADMM_CNC_DnCNN;
include/pnp_mri.h, "PnP denoisers on complex images"): the item functions of csrc/pnp_cx_ops.h through g++ as a stand-alone program
(tests/host/pnp_cx_emulation.cpp, plain and with the sanitizer flags of test_host_cores.py), the binding, the solvers' refusals before an
engine is opened, the rules of the C calls that need no device, and the properties of the NumPy oracle (tests/pnp_complex_oracle.py)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rel_l2, weights_trained
import pnp_complex_oracle as PO

SRC = os.path.join(ROOT, 'tests', 'host', 'pnp_cx_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
PLAIN = ['-O2', '-std=c++17', '-ffp-contract=off']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
C64, C128 = np.complex64, np.complex128
NEW = ('pnp_cx_den_in', 'pnp_cx_den_out', 'pnp_cx_den_out_dual', 'pnp_cnc_combine_cx')
SOLVERS = ('PNP_ADMM_L1_D', 'PNP_ADMM_CNC_D', 'PNP_ADMM_CNC_DnCNN')


# ---- host emulation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', [PLAIN, SAN], ids=['plain', 'sanitized'])
def test_host_emulation(flags, tmp_path):
    """the special values of the modulus join, the parts round trip against long double, the fused dual update and the kernels' index map
    for every residue of n mod 4 -- as a stand-alone program: nothing is preloaded"""
    exe = str(tmp_path / 'pnp_cx_emulation')
    subprocess.check_call(['g++'] + flags + ['-o', exe, SRC])
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    out = r.stdout.decode()
    assert out.rstrip().endswith('ok')
    maps = [line for line in out.splitlines() if line.startswith('index map')]
    assert len(maps) == 28 and all(line.endswith(' 0 bad') for line in maps)
    for mode in ('modulus', 'parts'):
        assert {int(re.search(r'n mod 4 = (\d)', line).group(1)) for line in maps if mode in line} == {0, 1, 2, 3}
    # 'parts' takes the vector arm exactly when its second plane is aligned; 'modulus' always
    assert all(('vector arm' in line) == ('modulus' in line or 'n mod 4 = 0' in line) for line in maps)


# ---- the binding ----------------------------------------------------------------------------------------------------------------------

def test_binding_declares_the_calls():
    from pnp_admm_cnc_mri_amd import _lib
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd.engine import CX_DENOISE, Engine
    raw = open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read()
    src = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert re.search(r'#define PNP_CX_DENOISE_MODULUS\s+0\b', src) and re.search(r'#define PNP_CX_DENOISE_PARTS\s+1\b', src)
    assert CX_DENOISE == {'modulus': 0, 'parts': 1}
    assert _lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.lib().pnp_abi_version()
    for name in ('cx_den_in', 'cx_den_out', 'cx_den_out_dual'):
        assert callable(getattr(Engine, name))
    from pnp_admm_cnc_mri_amd import solvers_pnp, sharding
    assert solvers_pnp.CX_KEYS == {'image': 'real', 'cx_denoise': 'modulus', 'cx_gain': 0.5}
    for name in SOLVERS:                        # taken by name from the options: solve_sharded can hand them over
        assert all(sharding._accepts(getattr(P, name), k) for k in solvers_pnp.CX_KEYS), name
    call, opts = type('C', (), {})(), dict(image='complex', cx_gain=2, iter_num=3)
    solvers_pnp.cx_keywords(call, opts)
    assert (call.image, call.cx_denoise, call.cx_gain) == ('complex', 'modulus', 2) and opts == dict(iter_num=3)


def test_null_arguments_are_argument_errors():
    """the rules that need no device: a null context, named by every new call"""
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    for name in NEW:
        args = [0 if t in (_lib.C.c_int, _lib.C.c_double) else None for t in _lib.SIGNATURES[name][1][1:]]
        assert getattr(L, name)(None, *args) == -1, name
        assert L.pnp_last_error() == ('%s: ctx is null' % name).encode(), name


# ---- the solvers' refusals, before an engine is opened ----------------------------------------------------------------------------------

def _boom(*a, **k):
    raise AssertionError('an engine was opened')


def _call(P, solver, *args, **kw):
    lead = ('dncnn_15', 'dncnn_15') if solver == 'PNP_ADMM_CNC_DnCNN' else ('ffdnet_gray',)
    return getattr(P, solver)(*lead, *args, model_zoo='/nonexistent', **kw)


@pytest.mark.parametrize('solver', SOLVERS)
def test_solver_refusals_come_before_an_engine(solver, monkeypatch):
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import solvers
    monkeypatch.setattr(solvers, 'Engine', _boom)
    H = W = 128
    rng = np.random.default_rng(1)
    m = np.ones((H, W), np.uint8)
    S = (rng.standard_normal((2, H, W)) + 1j * rng.standard_normal((2, H, W))).astype(C64)
    y = (rng.standard_normal((1, 2, H, W)) + 1j * rng.standard_normal((1, 2, H, W))).astype(C64)
    img = rng.uniform(0, 1, (1, H, W)).astype(np.float32)
    ok = dict(y=y, coils=S, image='complex', iter_num=1)
    call = functools.partial(_call, P, solver)
    with pytest.raises(ValueError, match="'real' or 'complex'"):
        call(m, None, **dict(ok, image='phase'))
    # image='complex' is not swallowed by the options dict: without coils it is refused, it does not run the real loop
    with pytest.raises(ValueError, match='coils='):
        call(m, None, y=y[:, 0], image='complex', iter_num=1)
    with pytest.raises(ValueError, match='y='):
        call(m, np.zeros((H, W), complex), images=img, coils=S, image='complex', iter_num=1)
    with pytest.raises(ValueError, match='trace_every='):
        call(m, None, trace_every=2, return_info=True, **ok)
    with pytest.raises(ValueError, match='tol='):
        call(m, None, tol=1e-3, return_info=True, **ok)
    with pytest.raises(ValueError, match="cx_denoise must be 'modulus' or 'parts'"):
        call(m, None, cx_denoise='phase', **ok)
    for gain in (0, -0.5, float('inf'), float('nan'), 1e-60, 1e60, None, 'big'):
        with pytest.raises(ValueError, match='cx_gain must be finite and > 0'):
            call(m, None, cx_denoise='parts', cx_gain=gain, **ok)
    # cx_denoise / cx_gain say how the denoiser acts on a complex image: with a real one they are refused, not ignored
    with pytest.raises(ValueError, match="need image='complex'"):
        call(m, None, images=img, cx_denoise='parts', iter_num=1)
    with pytest.raises(ValueError, match="need image='complex'"):
        call(m, None, images=img, cx_gain=0.25, iter_num=1)
    with pytest.raises(ValueError, match="need image='complex'"):
        call(m, None, y=y, coils=S, image='real', cx_gain=2, iter_num=1)


@pytest.mark.parametrize('solver', SOLVERS)
def test_complex_hidden_in_a_partial_is_a_type_error(solver, monkeypatch):
    """solve_sharded must know the dtype of the gather on every rank: image='complex' bound into the solver is refused before it runs"""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import solvers
    monkeypatch.setattr(solvers, 'Engine', _boom)
    lead = ('dncnn_15', 'dncnn_15') if solver == 'PNP_ADMM_CNC_DnCNN' else ('ffdnet_gray',)
    bound = functools.partial(getattr(P, solver), *lead, image='complex')
    y = np.zeros((2, 2, 128, 128), C64)
    with pytest.raises(TypeError, match="image='complex'"):
        P.sharding.solve_sharded(bound, np.ones((128, 128), np.uint8), None, y=y, coils=np.ones((2, 128, 128), C64))
    with pytest.raises(TypeError, match="image='complex'"):                      # a partial of a partial
        P.sharding.solve_sharded(functools.partial(bound, iter_num=1), np.ones((128, 128), np.uint8), None, y=y, coils=np.ones((2, 128, 128), C64))
    # given to solve_sharded it reaches the solver by name -- never its options dict -- and the solver's own rules answer
    with pytest.raises(ValueError, match='coils='):
        P.sharding.solve_sharded(functools.partial(getattr(P, solver), *lead), np.ones((128, 128), np.uint8), None, y=y, image='complex')


def test_engine_names_a_bad_mode_without_a_call():
    from pnp_admm_cnc_mri_amd import engine
    with pytest.raises(ValueError, match="cx_denoise must be 'modulus' or 'parts'"):
        engine._cx_denoise('phase')
    assert engine._cx_denoise('parts') == 1 and engine._cx_denoise(7) == 7


# ---- the oracle's own properties ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net64():
    return PO.cpu_net('ffdnet_gray', weights_trained('ffdnet_gray'), C128)


def test_glue_restatement_special_values():
    """the float32 restatement on the values the emulation plants: (d, 0) at m = 0 and where the squares underflow, negative d kept,
    NaN through; the parts round trip to two roundings"""
    den = np.float32(1e-45)
    v = np.array([0, -0.0, den - 2j * den, 1, -1j, 0.3 + 0.4j, np.nan, 0.25], C64)
    d = np.array([0.75, -0.25, 0.5, -0.5, 0.25, np.nan, 0.5, 0.5], np.float32)
    z = PO.den_out(d[None], v, 'modulus', dt=C64)
    assert z.dtype == C64 and np.array_equal(z[:3], np.array([0.75, -0.25, 0.5], C64)) and z[3] == -0.5 and z[4] == -0.25j
    assert np.isnan(z[5].real) and np.isnan(z[6].real) and z[7] == 0.5
    rng = np.random.default_rng(3)
    u = (rng.uniform(-1, 1, 4000) + 1j * rng.uniform(-1, 1, 4000)).astype(C64)
    for g in (0.5, 0.3, 2.0):
        back = PO.den_out(PO.den_in(u, 'parts', g, C64), u, 'parts', g, C64)
        assert np.abs(back - u).max() <= 2 * 2.0 ** -23 * (0.5 + g) / g, g
    assert rel_l2(PO.den_out(PO.den_in(u, 'modulus', dt=C64), u, 'modulus', dt=C64), u) <= 2.0 ** -22      # the identity network


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_oracle_phase_equivariance(kind):
    """y e^{i theta} -> x e^{i theta} through the 'modulus' loop in float64 to 1e-12: the network only ever sees |v|.  'parts' is NOT
    equivariant -- the network sees the two components, and the offset 0.5 prefers a phase."""
    par = dict(reo=0.25) if kind == 'l1' else dict(alpha=0.9, lambda1=1.35, reo=0.45, b=0.3)
    S, masks, y = PO.case(128, 128)
    th, m, net = np.exp(0.7j), masks[1], (_net64(),)
    a = PO.pnp(y[0], S, m, 3, kind, net, 'modulus', **par)
    b = PO.pnp(y[0] * th, S, m, 3, kind, net, 'modulus', **par)
    for u, v in zip(a, b):
        assert rel_l2(v, u * th) <= 1e-12
    assert np.abs(a[0].imag).max() > 0.01 * np.abs(a[0]).max() and np.abs(a[0]).max() <= 1 + 1e-12
    pa = PO.pnp(y[0], S, m, 3, kind, net, 'parts', **par)[0]
    pb = PO.pnp(y[0] * th, S, m, 3, kind, net, 'parts', **par)[0]
    assert rel_l2(pb, pa * th) > 1e-3
