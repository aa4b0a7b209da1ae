"""CPU tests of the coil mixing (noise prewhitening, coil compression): csrc/coilmix_plan.h through g++ with sanitizers
(tests/host/coilmix_emulation.cpp: the calibration index map, the Gram sum order, the two host solvers, the argument rule); the host
solvers of the real library against NumPy; the binding and the argument checks; the algebra itself on the NumPy oracles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rel_l2
import coilmix_oracle as CO
import multicoil_oracle as M

SRC = os.path.join(ROOT, 'tests', 'host', 'coilmix_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
E_ARG = -1
NEW = ('pnp_coilmix_check', 'pnp_coil_mix', 'pnp_coil_mix_f64', 'pnp_coil_gram', 'pnp_coil_gram_f64', 'pnp_coilmix_whiten',
       'pnp_coilmix_compress')


# ---- coilmix_plan.h under g++ with sanitizers -----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_coilmix') / 'coilmix_emulation')
    subprocess.check_call(['g++'] + SAN + ['-o', out, SRC])
    return out


def _run(args):
    r = subprocess.run(args, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    return r.stdout.decode()


@pytest.mark.parametrize('H,W', [(128, 128), (131, 128), (140, 160), (1024, 1024)])
def test_calibration_index_map_for_every_ncal(exe, H, W):
    """ncal = 4 .. 64, odd and even: exactly ncal^2 points, each once, in the documented order; the kernel's staging walk stays inside
    its tile."""
    assert _run([exe, 'index', str(H), str(W)]).split() == ['ok', 'index', str(H), str(W)]


def test_gram_sum_order_and_tile_walk(exe):
    """coilmix_gram_slice equals the loop restated in the emulation bit for bit (float and double data, masks with holes), is exact on
    integers and Hermitian to the bit; every pair (i <= j) has one owner for C = 1 .. 128; the mixing kernel's point map covers N once."""
    assert _run([exe, 'gram']).strip() == 'ok gram'


@pytest.mark.parametrize('n', [1, 2, 6, 33, 128])
def test_host_solvers_under_sanitizers(exe, n):
    """M Psi M^H = I, A v = lambda v and V^H V = I to 1e-12, descending order, the phase rule, the tie rule, the refusals."""
    assert _run([exe, 'solve', str(n)]).split() == ['ok', 'solve', str(n)]


def test_argument_rule_in_the_plan(exe):
    assert _run([exe, 'check']).strip() == 'ok check'


# ---- the library's host solvers against NumPy -------------------------------------------------------------------------------------------

def _lib():
    from pnp_admm_cnc_mri_amd import _lib as L
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize('n', [1, 2, 6, 33, 128])
def test_whitening_and_compression_against_numpy(n):
    from pnp_admm_cnc_mri_amd import coilmix as CM
    psi = CO.hpd(n, n)
    Mw = CM.whitening_matrix(psi)
    assert np.abs(Mw @ psi @ Mw.conj().T - np.eye(n)).max() <= 1e-12
    assert np.abs(Mw - CO.whitening_matrix(psi)).max() <= 1e-12 * np.abs(Mw).max()
    assert not np.triu(Mw, 1).any()
    k = min(n, 32)
    Mc, eig = CM.compression_matrix(psi, k)
    ref_M, ref_eig = CO.compression(psi, k)
    assert Mc.shape == (k, n) and eig.shape == (n,) and (np.diff(eig) <= 0).all()
    assert np.abs(eig - ref_eig).max() <= 1e-10 * ref_eig[0]
    assert np.abs(Mc @ Mc.conj().T - np.eye(k)).max() <= 1e-12
    for j in range(k):                                               # the phase rule: the first entry of largest modulus is real and positive
        v = Mc[j].conj()
        at = int(np.argmax(np.abs(v)))
        assert v[at].imag == 0.0 and v[at].real > 0.0 and abs(v[at]) == np.abs(v).max()
    # whitening composes on the host: the Gram of the whitened data is M_w R M_w^H and the combined matrix M_c M_w
    R = CO.hpd(n, n + 1, floor=0.01)
    Mx, e2 = CM.compression_matrix(R, k, whiten=Mw)
    Mc2, e2b = CM.compression_matrix(Mw @ R @ Mw.conj().T, k)
    assert np.array_equal(e2, e2b) and np.abs(Mx - Mc2 @ Mw).max() <= 1e-13 * np.abs(Mx).max()


def test_rank_4_of_40_channels_gives_numpys_projector():
    """40 channels spanning the 4-dimensional space of the oracle's 4 maps, 128 x 130, calibration 24 x 24: four eigenvalues carry the
    signal, the fifth is the noise's; the projector M_c^H M_c on the 4 virtual coils is NumPy's to 1e-8."""
    from pnp_admm_cnc_mri_amd import coilmix as CM
    H, W = 128, 130
    S, m = CO.rank4_maps(40, H, W, 3), M.mask(3, H, W)
    y = M.synthesize(M.phantom(3, H, W), S, m, M.noise(3, 40, m))
    R, _ = CO.gram(y, m, 24)
    Mc, eig = CM.compression_matrix(R, 4)
    ref_M, ref_eig = CO.compression(R, 4)
    print('eigenvalues / largest:', eig[:6] / eig[0])
    assert eig[3] > 1e-2 * eig[0] and eig[4] < 1e-3 * eig[0]          # the gap the problem is built to have
    assert np.abs(eig - ref_eig).max() <= 1e-10 * ref_eig[0]
    assert np.abs(CO.projector(Mc) - CO.projector(ref_M)).max() <= 1e-8
    assert np.abs(Mc - ref_M).max() <= 1e-8                          # with the phase rule the vectors themselves agree


def test_bad_covariances_and_gram_matrices_are_arg_errors():
    L = _lib().lib()
    out, eig = np.empty((3, 3), np.complex128), np.empty(3)
    good = np.ascontiguousarray(CO.hpd(3, 1))
    assert L.pnp_coilmix_whiten(_p(good), 3, _p(out)) == 0
    for bad, word in ((np.diag([1.0, -1.0, 1.0]), 'positive definite'), (np.zeros((3, 3)), 'positive definite'),
                      (np.array([[1, 2, 0], [2, 1, 0], [0, 0, 1.0]]), 'positive definite'),
                      (np.diag([1.0, np.nan, 1.0]), 'non-finite'), (np.diag([1.0, np.inf, 1.0]), 'non-finite')):
        a = np.ascontiguousarray(bad, dtype=np.complex128)
        assert L.pnp_coilmix_whiten(_p(a), 3, _p(out)) == E_ARG and word in L.pnp_last_error().decode(), bad
        if 'non-finite' in word:
            assert L.pnp_coilmix_compress(_p(a), 3, 2, _p(out), _p(eig)) == E_ARG and word in L.pnp_last_error().decode()
    assert L.pnp_coilmix_whiten(None, 3, _p(out)) == E_ARG and L.pnp_coilmix_whiten(_p(good), 3, _p(good)) == E_ARG
    assert L.pnp_coilmix_whiten(_p(good), 0, _p(out)) == E_ARG and L.pnp_coilmix_whiten(_p(good), 129, _p(out)) == E_ARG
    assert L.pnp_coilmix_compress(_p(good), 3, 0, _p(out), _p(eig)) == E_ARG and L.pnp_coilmix_compress(_p(good), 3, 4, _p(out), _p(eig)) == E_ARG
    assert L.pnp_coilmix_compress(_p(good), 3, 2, None, _p(eig)) == E_ARG and L.pnp_coilmix_compress(_p(good), 3, 3, _p(out), _p(eig)) == 0
    from pnp_admm_cnc_mri_amd import coilmix as CM
    with pytest.raises(ValueError, match='positive definite'):
        CM.whitening_matrix(np.diag([1.0, -1.0]))
    with pytest.raises(ValueError, match='square'):
        CM.whitening_matrix(np.ones((2, 3)))


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------

def test_binding_declares_the_coil_mixing_calls():
    lib = _lib()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read(), flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in lib.SIGNATURES, name
        assert hasattr(lib.lib(), name), name
    for name in sorted(set(re.findall(r'\b(pnp_[A-Za-z0-9_]+)\s*\(', src))):          # every declared symbol is exported
        assert hasattr(lib.lib(), name), name
    assert lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == lib.lib().pnp_abi_version()
    import pnp_admm_cnc_mri_amd as P
    for solver in (P.ADMM_L1, P.ADMM_CNC, P.PNP_ADMM_L1_D, P.PNP_ADMM_CNC_D, P.PNP_ADMM_CNC_DnCNN):
        sig = inspect.signature(solver).parameters
        assert sig['virtual_coils'].default is None and sig['noise_cov'].default is None and sig['calib'].default == 24, solver
    for name in ('whitening_matrix', 'calibration_gram', 'compression_matrix', 'coil_mix', 'coil_prepare', 'coilmix'):
        assert hasattr(P, name), name
    for name in ('coil_mix', 'whitening_matrix', 'compression_matrix'):
        assert hasattr(P.utils_pnp, name), name


def test_every_rule_of_pnp_coilmix_check():
    L = _lib().lib()
    for ok in ((1, 1, 1, 4, 128, 128), (64, 8, 1, 24, 256, 256), (128, 32, 7, 64, 1024, 128), (32, 32, 2, 5, 131, 140), (40, 4, 1, 24, 128, 130)):
        assert L.pnp_coilmix_check(*ok) == 0, ok
    for bad, word in (((0, 1, 1, 24, 128, 128), 'C_in must be'), ((129, 8, 1, 24, 128, 128), 'C_in must be'), ((-3, 1, 1, 24, 128, 128), 'C_in must be'),
                      ((8, 0, 1, 24, 128, 128), 'C_out must be'), ((8, 9, 1, 24, 128, 128), 'C_out must be'), ((64, 33, 1, 24, 128, 128), 'C_out must be'),
                      ((8, 4, 0, 24, 128, 128), 'Ks must be'), ((8, 4, 1, 3, 128, 128), 'ncal must be'), ((8, 4, 1, 65, 128, 128), 'ncal must be'),
                      ((8, 4, 1, 24, 127, 128), '[128, 1024]'), ((8, 4, 1, 24, 128, 1025), '[128, 1024]')):
        assert L.pnp_coilmix_check(*bad) == E_ARG, bad
        assert word in L.pnp_last_error().decode(), (bad, L.pnp_last_error())


def test_device_entry_points_refuse_bad_arguments_without_a_device():
    """Null pointers, sizes outside the rule and overlapping in / out are PNP_E_ARG before anything is launched (host buffers stand in for
    device arrays: they are never touched)."""
    L = _lib().lib()
    a, b = np.zeros(4096, np.complex128), np.zeros(4096, np.complex128)
    mixes = (L.pnp_coil_mix, L.pnp_coil_mix_f64)
    for fn in mixes:
        assert fn(None, None, _p(b), None, _p(b), 1, 2, 1, 8) == E_ARG and 'null' in L.pnp_last_error().decode()
        assert fn(None, _p(a), _p(b), None, _p(a), 1, 2, 1, 8) == E_ARG and 'overlap' in L.pnp_last_error().decode()
        assert fn(None, _p(a), _p(b), None, C.c_void_p(a.ctypes.data + 64), 1, 2, 1, 8) == E_ARG and 'overlap' in L.pnp_last_error().decode()
        for B, ci, co, N, word in ((0, 2, 1, 8, 'B must be'), (1, 0, 1, 8, 'C_in must be'), (1, 129, 1, 8, 'C_in must be'), (1, 4, 5, 8, 'C_out must be'),
                                   (1, 64, 33, 8, 'C_out must be'), (1, 2, 1, 0, 'N must be')):
            assert fn(None, _p(a), _p(b), None, _p(b), B, ci, co, N) == E_ARG and word in L.pnp_last_error().decode(), (B, ci, co, N)
    for fn in (L.pnp_coil_gram, L.pnp_coil_gram_f64):
        assert fn(None, None, _p(b), None, _p(b), 1, 2, 128, 128, 24) == E_ARG and 'null' in L.pnp_last_error().decode()
        assert fn(None, _p(a), None, None, _p(b), 1, 2, 128, 128, 24) == E_ARG
        for B, Cn, H, W, ncal, word in ((0, 2, 128, 128, 24, 'B must be'), (1, 129, 128, 128, 24, 'C_in must be'), (1, 2, 127, 128, 24, '[128, 1024]'),
                                        (1, 2, 128, 128, 3, 'ncal must be'), (1, 2, 128, 128, 65, 'ncal must be')):
            assert fn(None, _p(a), _p(b), None, _p(b), B, Cn, H, W, ncal) == E_ARG and word in L.pnp_last_error().decode(), (B, Cn, H, W, ncal)


def test_solvers_refuse_before_any_engine_is_opened(monkeypatch):
    """virtual_coils= / noise_cov= need coils= and measured y=; the limit of 32 applies to the MIXED count; all of it is a ValueError
    before an Engine exists."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import solvers

    def no_engine(*a, **k):
        raise AssertionError('an engine was opened')
    monkeypatch.setattr(solvers, 'Engine', no_engine)
    m = np.ones((128, 128), np.uint8)
    S40, y40 = np.ones((40, 128, 128), np.complex64), np.zeros((1, 40, 128, 128), np.complex64)
    with pytest.raises(ValueError, match='need coils= and y='):
        P.ADMM_CNC(m, None, coils=S40, virtual_coils=4)
    with pytest.raises(ValueError, match='need coils= and y='):
        P.ADMM_CNC(m, None, y=y40, virtual_coils=4)
    with pytest.raises(ValueError, match='need coils= and y='):
        P.ADMM_L1(m, None, images=np.zeros((1, 128, 128), np.uint8), coils=S40, noise_cov=np.eye(40))
    for kw, word in ((dict(virtual_coils=33), 'C_out must be'), (dict(virtual_coils=0), 'C_out must be'), (dict(virtual_coils=41), 'C_out must be'),
                     (dict(noise_cov=np.eye(40)), 'C_out must be'),            # noise_cov alone: C_out = C_in = 40 > 32
                     (dict(virtual_coils=4, calib=3), 'ncal must be'), (dict(virtual_coils=4, calib=65), 'ncal must be'),
                     (dict(virtual_coils=4, noise_cov=np.eye(39)), 'noise_cov must be'), (dict(virtual_coils=4, cg_iters=0), 'cg_iters'),
                     (dict(virtual_coils=2.5), 'integers')):
        with pytest.raises(ValueError, match=re.escape(word)):
            P.ADMM_CNC(m, None, y=y40, coils=S40, **kw)
    with pytest.raises(ValueError, match='C must be'):                  # without mixing the limit is what it was
        P.ADMM_CNC(m, None, y=y40, coils=S40)
    with pytest.raises(ValueError, match='C_in must be'):
        P.ADMM_CNC(m, None, y=np.zeros((1, 129, 128, 128), np.complex64), coils=np.ones((129, 128, 128), np.complex64), virtual_coils=4)


# ---- the algebra, on the oracles ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_a_unitary_mix_leaves_the_reconstruction_unchanged(kind):
    """y' = M y, S' = M S with a unitary M: ten iterations of the float64 oracle agree to 1e-12 (the forward model is linear in the coil
    index and A^H A is unchanged)."""
    H, W, Cn = 128, 130, 5
    img, S, m, nz, y = M.problem(11, Cn, H, W)
    U = CO.unitary(Cn, 1)
    assert rel_l2(M.admm(CO.mix(y, U), CO.mix(S, U), m, 10, kind), M.admm(y, S, m, 10, kind)) <= 1e-12


def test_oracle_region_and_restatement():
    for ncal, n in ((4, 128), (5, 131), (24, 140), (64, 128)):
        lines = CO.cal_lines(ncal, n)
        assert len(lines) == ncal == len(set(lines)) and lines[0] == 0 and lines[-1] == n - 1 and (lines < n).all()
        assert CO.cal_region(ncal, n, n + 3).sum() == ncal * ncal
    rng = np.random.default_rng(5)
    k = rng.standard_normal((6, 7, 9)) + 1j * rng.standard_normal((6, 7, 9))
    Mx = rng.standard_normal((3, 6)) + 1j * rng.standard_normal((3, 6))
    ref = np.tensordot(Mx, k, axes=(1, 0))
    assert np.abs(CO.mix(k, Mx) - ref).max() <= 1e-14 and np.abs(CO.mix(k, Mx, np.complex64) - ref).max() <= 1e-5
    assert (np.abs(ref) <= CO.mix_abs(k, Mx) * (1 + 1e-12)).all()
