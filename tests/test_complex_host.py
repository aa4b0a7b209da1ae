"""CPU tests of the complex-valued image mode (pnp_set_image; include/pnp_mri.h, "complex-valued images on a coil context"): the NumPy
oracle itself (tests/complex_oracle.py) against the committed real oracles, its phase equivariance, the prox identity and the quality it
buys on the phase phantom; the binding and the rules that need no device through the real library; the solvers' refusals before an engine
is opened; and csoft / cclip / the complex wavelet item functions through g++ (tests/host/complex_emulation.cpp, plain and with the
sanitizer flags of test_host_cores.py)."""
import inspect
import os
import re
import socket
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rel_l2
import complex_oracle as X
import multicoil_oracle as M
import wavelet_oracle as W
from oracle import admm_oracle as O

SRC = os.path.join(ROOT, 'tests', 'host', 'complex_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
PLAIN = ['-O2', '-std=c++17', '-ffp-contract=off']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
CNC = dict(alpha=0.45, lambda1=0.5, reo=0.05, b=64)


def _fields(H, W, seed=0):
    """x, z, w real [H,W] in (-1, 1) on which both branches of soft and of clip (1 / b = 1 / 64, thr ~ 0.01) are taken"""
    rng = np.random.default_rng(seed + 31 * H + W)
    return rng.uniform(-1, 1, (H, W)), 0.05 * rng.uniform(-1, 1, (H, W)), 0.3 * rng.uniform(-1, 1, (H, W))


# ---- the oracle against the committed oracles, and against itself -------------------------------------------------------------------

def test_zero_imaginary_parts_give_the_real_steps():
    """With zero imaginary parts the complex steps are oracle/admm_oracle.py's and tests/wavelet_oracle.py's: 1e-15 (values in (-1, 1);
    what differs is the rounding of (m - c) / m and ib / m)."""
    x, z, w = _fields(96, 80)
    cz, cw = X.l1_step(x, z, w, 0.05 * 0.5)
    rz, rw = O.l1_step(x, z, w, 0.5, 0.05)
    assert np.abs(cz - rz).max() <= 1e-15 and np.abs(cw - rw).max() <= 1e-15 and not cz.imag.any() and not cw.imag.any()
    assert (rz == 0).any() and (rz != 0).any()
    cz, cw = X.cnc_step(x, z, w, **CNC)
    rz, rw = O.cnc_step(x, z, w, **CNC)
    assert np.abs(cz - rz).max() <= 1e-15 and np.abs(cw - rw).max() <= 1e-15 and not cz.imag.any()
    assert (np.abs(z) > 1 / 64).any() and (np.abs(z) < 1 / 64).any()
    for name, L in (('haar', 1), ('db2', 3), ('db4', 2)):
        cz, cw = X.wl1_step(x, z, w, 0.3, name, L)
        rz, rw = W.prox_l1(x, z, w, 0.3, name, L)
        assert np.abs(cz - rz).max() <= 1e-15 and np.abs(cw - rw).max() <= 1e-15, (name, L)
        cz, cw = X.wcnc_step(x, z, w, name=name, levels=L, **W.PROX_CNC)
        rz, rw = W.prox_cnc(x, z, w, name=name, levels=L, **W.PROX_CNC)
        assert np.abs(cz - rz).max() <= 1e-15 and np.abs(cw - rw).max() <= 1e-15, (name, L)


def test_csoft_is_the_prox_of_the_modulus():
    """z = csoft(u, c):  z + c z / |z| = u where z != 0,  |u| <= c where z = 0;  cclip = u - csoft."""
    rng = np.random.default_rng(5)
    u = rng.uniform(-1, 1, 4000) + 1j * rng.uniform(-1, 1, 4000)
    u[:3] = (0, 0.3 + 0.4j, -0.0 + 0j)                         # zero, |u| == c exactly (0.5 in binary: 3-4-5 scaled), minus zero
    u[1] = 3 / 8 + 4j / 8
    for c in (0.0, 0.25, 0.625):
        z = X.csoft(u, c)
        nz = z != 0
        assert np.isfinite(z.view(np.float64)).all()
        assert np.abs(z[nz] + c * z[nz] / np.abs(z[nz]) - u[nz]).max() <= 1e-15
        assert (np.abs(u[~nz]) <= c).all() and (np.abs(u[nz]) > c).all()
        assert np.abs(u - z - X.cclip(u, c)).max() <= 1e-15
    assert X.csoft(u[1], 0.625) == 0 and X.cclip(u[1], 0.625) == u[1]


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_oracle_phase_equivariance(kind):
    """y e^{i theta} -> x e^{i theta}: nothing in the complex loop prefers a phase.  1e-12 after ten iterations, pixels and db2."""
    t, S, m, y = X.problem(2, 3, 128, 128)
    th = np.exp(0.7j)
    for tr in (None, 'db2'):
        a, b = X.admm(y, S, m, 10, kind, transform=tr), X.admm(y * th, S, m, 10, kind, transform=tr)
        assert rel_l2(b, a * th) <= 1e-12, tr
    # the real-mode loop does prefer one: |Re .| is not equivariant
    assert rel_l2(M.admm(y * th, S, m, 10, kind), M.admm(y, S, m, 10, kind)) > 1e-3


def test_real_data_stays_close_to_the_real_loop():
    """On the phantom without a phase the complex loop reconstructs the magnitude about as well as the real one (0.145 -> 0.149 measured)."""
    t, S, m, y = X.problem(1, 5, 128, 130, real=True)
    e_real = rel_l2(M.admm(y, S, m, 10, 'l1'), np.abs(t))
    e_cx = X.mag_err(X.admm(y, S, m, 10, 'l1'), t)
    assert 0.1446 / 2 <= e_real <= 0.1446 * 2 and 0.1486 / 2 <= e_cx <= 0.1486 * 2 and e_cx <= 1.1 * e_real


# (H, W, C, kind): real mode || x - |t| || / ||t||,  complex mode || |x| - |t| || / ||t||,  || x - t || / ||t||,  complex64 restatement's distance
QUALITY = {
    (128, 130, 5, 'l1'): (0.2660, 0.2228, 0.2617, 3.87e-7), (128, 130, 5, 'cnc'): (0.2749, 0.2154, 0.2533, 3.66e-7),
    (128, 128, 4, 'l1'): (0.2649, 0.2252, 0.2772, 3.91e-7), (128, 128, 4, 'cnc'): (0.2746, 0.2204, 0.2713, 4.11e-7),
}


@pytest.mark.parametrize('case', sorted(QUALITY))
def test_complex_mode_recovers_more_of_the_magnitude(case):
    """Ten iterations at the presets on the phase phantom: the complex mode's magnitude error is strictly below the real mode's, and the
    figures of DESIGN.md section 20 hold within a factor of 2; so does the distance of the complex64 restatement, the yardstick of the
    float GPU tests."""
    H, Wd, C, kind = case
    t, S, m, y = X.problem(1, C, H, Wd)
    xr, xc = M.admm(y, S, m, 10, kind), X.admm(y, S, m, 10, kind)
    got = (rel_l2(xr, np.abs(t)), X.mag_err(xc, t), rel_l2(xc, t), rel_l2(X.admm(y, S, m, 10, kind, dt=np.complex64), xc))
    assert got[1] < got[0], got
    for g, want in zip(got, QUALITY[case]):
        assert want / 2 <= g <= want * 2, (got, QUALITY[case])


def test_strong_phase_is_where_it_matters():
    """phi with a ramp and sine amplitude 2.5: 0.596 -> 0.416 (L1), 0.648 -> 0.395 (CNC)"""
    t, S, m, y = X.problem(1, 5, 128, 130, strong=True)
    for kind, (r, c) in (('l1', (0.5958, 0.4159)), ('cnc', (0.6483, 0.3946))):
        e_r, e_c = rel_l2(M.admm(y, S, m, 10, kind), np.abs(t)), X.mag_err(X.admm(y, S, m, 10, kind), t)
        assert r / 2 <= e_r <= r * 2 and c / 2 <= e_c <= c * 2 and e_c < e_r, (kind, e_r, e_c)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------

NEW = ('pnp_image_check', 'pnp_set_image', 'pnp_get_image', 'pnp_set_state_cx', 'pnp_set_state_cx_f64', 'pnp_get_state_cx', 'pnp_get_state_cx_f64',
       'pnp_download_x_cx', 'pnp_download_x_cx_f64', 'pnp_dc_step_cx', 'pnp_dc_step_cx_f64', 'pnp_prox_l1_dual_cx', 'pnp_prox_l1_dual_cx_f64',
       'pnp_prox_cnc_dual_cx', 'pnp_prox_cnc_dual_cx_f64', 'pnp_A_cx')


def test_binding_declares_the_complex_calls():
    from pnp_admm_cnc_mri_amd import _lib
    import pnp_admm_cnc_mri_amd as P
    raw = open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read()
    src = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r'#define PNP_IMAGE_REAL\s+0\b', src) and re.search(r'#define PNP_IMAGE_COMPLEX\s+1\b', src)
    assert _lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.lib().pnp_abi_version()
    for solver in (P.ADMM_L1, P.ADMM_CNC):
        assert inspect.signature(solver).parameters['image'].default == 'real', solver
    for solver in (P.PNP_ADMM_L1_D, P.PNP_ADMM_CNC_D, P.PNP_ADMM_CNC_DnCNN):
        assert 'image' not in inspect.signature(solver).parameters, solver
    from pnp_admm_cnc_mri_amd.engine import Engine, IMAGE_MODES
    assert IMAGE_MODES == {'real': 0, 'complex': 1} and hasattr(Engine, 'set_image_mode') and isinstance(Engine.image_mode, property)


def test_null_context_is_an_argument_error():
    """the rule of pnp_set_image that needs no device, and the null check of every new call"""
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    for mode in (0, 1, 7):
        assert L.pnp_set_image(None, mode) == -1 and b'pnp_set_image: ctx is null' in L.pnp_last_error()
    assert L.pnp_get_image(None, None) == -1
    # pnp_image_check: the mode, and the one setting whose tile does not fit the LDS on complex doubles
    assert L.pnp_image_check(7, 0, 0, 0) == -1 and L.pnp_image_check(0, 3, 4, 1) == 0 and L.pnp_image_check(1, 3, 4, 0) == 0
    assert L.pnp_image_check(1, 3, 4, 1) == -1 and b'does not fit the LDS' in L.pnp_last_error()
    assert all(L.pnp_image_check(1, wv, lv, f) == 0 for wv in (0, 1, 2, 3) for lv in (1, 2, 3, 4) for f in (0, 1) if (wv, lv, f) != (3, 4, 1))
    for name in NEW[3:]:
        args = [0 if t in (_lib.C.c_int, _lib.C.c_double) else None for t in _lib.SIGNATURES[name][1][1:]]
        assert getattr(L, name)(None, *args) == -1 and name.encode() in L.pnp_last_error(), name


def _boom(*a, **k):
    raise AssertionError('an engine was opened')


@pytest.mark.parametrize('solver', ['ADMM_L1', 'ADMM_CNC'])
def test_solver_refusals_come_before_an_engine(solver, monkeypatch):
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import solvers
    monkeypatch.setattr(solvers, 'Engine', _boom)
    fn = getattr(P, solver)
    H = Wd = 128
    t, S, m, y = X.problem(3, 2, H, Wd)
    img = np.abs(t).astype(np.float32)
    ok = dict(y=y[None], coils=S, image='complex', iter_num=1)
    with pytest.raises(ValueError, match="'real' or 'complex'"):
        fn(m, None, **dict(ok, image='phase'))
    with pytest.raises(ValueError, match='coils='):
        fn(m, None, y=y[:1], image='complex', iter_num=1)
    with pytest.raises(ValueError, match='y='):
        fn(m, np.zeros((H, Wd), complex), images=img[None], coils=S, image='complex', iter_num=1)
    with pytest.raises(ValueError, match='spin='):
        fn(m, None, transform='db2', spin='random', **ok)
    with pytest.raises(ValueError, match='trace_every='):
        fn(m, None, trace_every=2, return_info=True, **ok)
    with pytest.raises(ValueError, match='tol='):
        fn(m, None, tol=1e-3, return_info=True, **ok)
    with pytest.raises(ValueError, match='does not fit the LDS'):
        fn(m, None, transform='db4', levels=4, precision='f64', **ok)
    # the accepted forms get as far as the engine: an array of maps, and 'estimate' (with and without mixing)
    with pytest.raises(AssertionError, match='an engine was opened'):
        fn(m, None, **ok)
    with pytest.raises(AssertionError, match='an engine was opened'):
        fn(m, None, transform='db2', **ok)
    mfull = np.ones((H, Wd), np.uint8)
    with pytest.raises(AssertionError, match='an engine was opened'):
        fn(mfull, None, y=y[None], coils='estimate', image='complex', iter_num=1)


def _cx_solver(mask, noises, images=None, y=None, mask_id=None, return_device=False, image='real', **opts):
    """entry-point-shaped stand-in on the CPU: slice n -> y[n, 0] * (1 + 2i), complex64 -- as a list, or as one tensor"""
    import torch
    out = [(np.asarray(y[n, 0]) * (1 + 2j)).astype(np.complex64 if image == 'complex' else np.float32) for n in range(len(y))]
    return torch.from_numpy(np.stack(out)) if return_device else out


def _cx_y(B):
    rng = np.random.default_rng(B)
    return (rng.standard_normal((B, 1, 8, 6)) + 1j * rng.standard_normal((B, 1, 8, 6))).astype(np.complex64)


def _cx_worker(rank, world, port, B, q):
    import torch.distributed as dist
    import pnp_admm_cnc_mri_amd as P
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        x = P.sharding.solve_sharded(_cx_solver, np.ones((8, 6), np.uint8), None, y=_cx_y(B), image='complex', coils=1)
        if rank == 0:
            q.put(x)
        else:
            assert x is None
        dist.monitored_barrier()                      # gloo-only, CPU: dist.barrier() probes for an accelerator and opens the GPU
    finally:
        dist.destroy_process_group()


def test_sharded_entry_passes_the_keyword_through():
    import functools
    import pnp_admm_cnc_mri_amd as P
    seen = {}

    def solver(mask, noises, **kw):
        seen.update(kw)
        return [np.zeros((4, 4), np.complex128)] * len(kw['y'])

    out = P.sharding.solve_sharded(solver, np.ones((4, 4), np.uint8), None, y=np.zeros((2, 1, 4, 4), complex), image='complex', coils=1)
    assert seen['image'] == 'complex' and out.dtype == np.complex64 and out.shape == (2, 4, 4)
    # image='complex' hidden in a partial: the gather's dtype is unknown to solve_sharded, and a cast would drop the phase
    with pytest.raises(TypeError, match="image='complex'"):
        P.sharding.solve_sharded(functools.partial(_cx_solver, image='complex'), np.ones((8, 6), np.uint8), None, y=_cx_y(2), coils=1)


@pytest.mark.parametrize('world,B', [(2, 5), (3, 2)])
def test_sharded_complex_result_through_a_process_group(world, B):
    """The complex reconstructions travel through dist.gather (which takes no complex dtype) over gloo: uneven shards (3 + 2) and an
    empty one (1 + 1 + 0), equal to the plain call bit for bit."""
    import torch.multiprocessing as mp
    import pnp_admm_cnc_mri_amd as P
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_cx_worker, args=(r, world, port, B, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    ref = P.sharding.solve_sharded(_cx_solver, np.ones((8, 6), np.uint8), None, y=_cx_y(B), image='complex', coils=1)
    assert got.dtype == np.complex64 and got.shape == (B, 8, 6) and np.array_equal(got, ref) and np.abs(got.imag).max() > 0


# ---- host emulation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flags', [PLAIN, SAN], ids=['plain', 'sanitized'])
def test_host_emulation(flags, tmp_path):
    """csoft / cclip / the complex steps of prox_ops.h on their edge cases and the wavelet item functions on Cpx<S> against the real
    instances on the two planes, as a stand-alone program: nothing is preloaded."""
    exe = str(tmp_path / 'complex_emulation')
    subprocess.check_call(['g++'] + flags + ['-o', exe, SRC])
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    out = r.stdout.decode()
    assert out.rstrip().endswith('ok') and out.count(' differ') == 24 and 'float scalar' in out and 'double scalar' in out
    assert all(line.endswith(' 0 differ') for line in out.splitlines() if 'differ' in line)
