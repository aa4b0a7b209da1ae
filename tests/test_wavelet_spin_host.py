"""CPU tests of cycle spinning for the wavelet prox (pnp_set_spin, pnp_dwt2_shifted, the spin= keywords of ADMM_L1 / ADMM_CNC): the shifted
index maps of csrc/wavelet_plan.h through g++ (tests/host/wavelet_spin_emulation.cpp, sanitizer flags of test_wavelet_host.py) against the
rolled NumPy oracle (tests/wavelet_spin_oracle.py), every rule of pnp_spin_check through the real library without a device, the binding,
and engine.spin_table."""
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rel_l2
import wavelet_oracle as O
import wavelet_spin_oracle as S

SRC = os.path.join(ROOT, 'tests', 'host', 'wavelet_spin_emulation.cpp')
SRC_UNSHIFTED = os.path.join(ROOT, 'tests', 'host', 'wavelet_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
CODE = {'haar': 1, 'db2': 2, 'db4': 3}
SHAPES = [(128, 128), (128, 160), (256, 192)]
# the partial-tile sizes of tests/test_gpu_wavelet_edges.py that take L = 3 and L = 4: shifts_of(L) holds (2^L - 1, 2^L - 1)
EDGE_SHAPES = [O.EDGE_SIZES[3], O.EDGE_SIZES[4]]
EDGE_PROX = [(name, L) + O.EDGE_SIZES[L] for L in (3, 4) for name in O.NAMES]
L1_THR = 0.4
CNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)
CNC_P = (CNC['alpha'] * CNC['reo'] * CNC['lambda1'], 1 - CNC['alpha'], CNC['alpha'], CNC['alpha'] * CNC['reo'] * CNC['lambda1'] * CNC['b'],
         1 / CNC['b'])


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_wavelet_spin') / 'wavelet_spin_emulation')
    subprocess.check_call(['g++'] + SAN + ['-o', out, SRC])
    return out


@pytest.fixture(scope='module')
def exe_unshifted(tmp_path_factory):
    """the emulation as it was before cycle spinning, compiled unchanged against the header with the two new members"""
    out = str(tmp_path_factory.mktemp('emu_wavelet_plain') / 'wavelet_emulation')
    subprocess.check_call(['g++'] + SAN + ['-o', out, SRC_UNSHIFTED])
    return out


def _run(args):
    r = subprocess.run(args, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    return r.stdout.decode()


def emulate(exe, tmp_path, name, L, mode, arrays, shifts, params=(0, 0, 0, 0, 0), f64=True):
    dt = np.float64 if f64 else np.float32
    B, H, W = arrays[0].shape
    inp, out = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(inp, 'wb') as f:
        f.write(struct.pack('<8i', CODE[name], L, H, W, B, mode, 1 if f64 else 0, len(shifts)))
        f.write(np.asarray(shifts, np.int32).tobytes())
        f.write(struct.pack('<5d', *params))
        for a in arrays:
            f.write(np.ascontiguousarray(a, dt).tobytes())
    _run([exe, 'run', inp, out])
    return np.fromfile(out, dt).reshape(-1, B, H, W)


def emulate_unshifted(exe, tmp_path, name, L, mode, arrays, params=(0, 0, 0, 0, 0)):
    B, H, W = arrays[0].shape
    inp, out = str(tmp_path / 'in0.bin'), str(tmp_path / 'out0.bin')
    with open(inp, 'wb') as f:
        f.write(struct.pack('<7i', CODE[name], L, H, W, B, mode, 1))
        f.write(struct.pack('<5d', *params))
        for a in arrays:
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    _run([exe, 'run', inp, out])
    return np.fromfile(out, np.float64).reshape(-1, B, H, W)


# ---- the shifted index maps against the rolled oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize('H,W', SHAPES + EDGE_SHAPES)
@pytest.mark.parametrize('name', O.NAMES)
def test_shifted_transform_matches_rolled_oracle(exe, exe_unshifted, tmp_path, name, H, W):
    """Psi_s and Psi_s^T tile by tile through wavelet_plan.h's item functions, every valid L = 1..4 and the five shifts, against the oracle
    on the rolled input / rolled back (double: 1e-12; an indexing error is O(1)); s = (0, 0) equals the unshifted emulation bit for bit."""
    rng = np.random.default_rng(H * 7 + W)
    v = rng.standard_normal((2, H, W))
    for L in range(1, 5):
        if not O.valid(name, L, H, W):
            continue
        c_in = O.fwd(v, name, L)
        plain = (emulate_unshifted(exe_unshifted, tmp_path, name, L, 0, [v])[0], emulate_unshifted(exe_unshifted, tmp_path, name, L, 1, [c_in])[0])
        for s in S.shifts_of(L):
            got = emulate(exe, tmp_path, name, L, 0, [v], [s])[0]
            back = emulate(exe, tmp_path, name, L, 1, [c_in], [s])[0]
            assert np.isfinite(got).all() and np.isfinite(back).all()
            errs = (rel_l2(got, S.fwd(v, name, L, s)), rel_l2(back, S.inv(c_in, name, L, s)))
            assert max(errs) <= 1e-12, (L, s, errs)
            if s == (0, 0):
                assert np.array_equal(got, plain[0]) and np.array_equal(back, plain[1]), L
            else:
                assert not np.array_equal(got, plain[0]), (L, s)


@pytest.mark.parametrize('name,L,H,W', [('db4', 4, 128, 128), ('db2', 3, 128, 160), ('haar', 2, 256, 192), ('db4', 1, 128, 160), ('haar', 4, 128, 128)] + EDGE_PROX)
def test_shifted_prox_matches_rolled_oracle(exe, exe_unshifted, tmp_path, name, L, H, W):
    """Both prox steps in the five shifted frames (CNC: z first, then x + w through the same arrays) against the rolled oracle to 1e-12 in
    double; s = (0, 0) equals the unshifted emulation bit for bit."""
    rng = np.random.default_rng(3)
    x, z, w = (rng.uniform(-1, 1, (2, H, W)) * k for k in (1.0, 1.0, 0.3))
    plain = (emulate_unshifted(exe_unshifted, tmp_path, name, L, 2, [x, z, w], (L1_THR, 0, 0, 0, 0)),
             emulate_unshifted(exe_unshifted, tmp_path, name, L, 3, [x, z, w], CNC_P))
    for s in S.shifts_of(L):
        for k, (kind, mode, pd, po) in enumerate((('l1', 2, (L1_THR, 0, 0, 0, 0), dict(thr=L1_THR)), ('cnc', 3, CNC_P, CNC))):
            got = emulate(exe, tmp_path, name, L, mode, [x, z, w], [s], pd)
            want = S.prox(kind, x, z, w, po, name, L, [s])
            assert np.isfinite(got).all()
            errs = (rel_l2(got[0], want[0]), rel_l2(got[1], want[1]))
            assert max(errs) <= 1e-12, (kind, s, errs)
            if s == (0, 0):
                assert np.array_equal(got, plain[k]), kind


@pytest.mark.parametrize('K', [2, 3, 4])
@pytest.mark.parametrize('f64', [True, False])
def test_averaged_prox_follows_the_composition_rule(exe, tmp_path, K, f64):
    """K shifts per prox, accumulated in the order of the synthesis launches: bit-equal to acc = z_0; acc += z_j; z+ = (acc + z_(K-1)) r,
    w+ = (x + w) - z+ built from the emulation's own single-shift steps in the same precision, and 1e-12 from the oracle in double."""
    name, L, H, W = 'db2', 3, 128, 160
    dt = np.float64 if f64 else np.float32
    rng = np.random.default_rng(5)
    x, z, w = ((rng.uniform(-1, 1, (2, H, W)) * k).astype(dt) for k in (1.0, 1.0, 0.3))
    shifts = list(S.shifts_of(L))[1:1 + K]
    for kind, mode, pd, po in (('l1', 2, (L1_THR, 0, 0, 0, 0), dict(thr=L1_THR)), ('cnc', 3, CNC_P, CNC)):
        got = emulate(exe, tmp_path, name, L, mode, [x, z, w], shifts, pd, f64)
        zs = [emulate(exe, tmp_path, name, L, mode, [x, z, w], [s], pd, f64)[0] for s in shifts]
        acc = zs[0]
        for j in range(1, K - 1):
            acc = acc + zs[j]
        zn = (acc + zs[K - 1]) * dt(1.0 / K)
        assert zn.dtype == dt and np.array_equal(got[0], zn) and np.array_equal(got[1], (x + w) - zn), kind
        if f64:
            want = S.prox(kind, x, z, w, po, name, L, shifts)
            assert rel_l2(got[0], want[0]) <= 1e-12 and rel_l2(got[1], want[1]) <= 1e-12, kind


# ---- the rules, the schedule and the binding ------------------------------------------------------------------------------------

def _table(rows):
    import ctypes as C
    t = np.ascontiguousarray(rows, np.int32).reshape(-1, 2)
    return t, t.ctypes.data_as(C.POINTER(C.c_int32))


BAD = [  # levels, shifts, n (None: len), per_prox, the word of the rule
    (3, [(0, 0)], 0, 1, 'n must'), (3, [(0, 0)], -1, 1, 'n must'), (3, [(0, 0)] * 4097, None, 1, 'n must'), (3, None, 4, 1, 'n must'),
    (3, [(0, 0)] * 4, None, 0, 'per_prox'), (3, [(0, 0)] * 34, None, 17, 'per_prox'),
    (3, [(0, 0)] * 7, None, 2, 'multiple'), (3, [(0, 0)] * 4, None, 3, 'multiple'),
    (3, [(0, 0), (8, 0)], None, 1, 'range'), (3, [(0, 8)], None, 1, 'range'), (2, [(0, 0), (1, -1)], None, 2, 'range'),
    (1, [(2, 0)], None, 1, 'range'), (4, [(15, 16)], None, 1, 'range'),
    (0, [(0, 0)], None, 1, 'levels'), (5, [(0, 0)], None, 1, 'levels'),
]


def test_spin_rules_are_decided_without_a_device(exe):
    """Every rule of pnp_spin_check through the real library, no context: PNP_E_ARG with a message that names the rule; the plan's own
    check (g++) agrees; valid tables pass; the four context calls refuse a null context."""
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    for levels, rows, n, k, word in BAD:
        t, p = _table(rows) if rows is not None else (None, None)
        n = len(t) if n is None else n
        assert L.pnp_spin_check(levels, p, n, k) == -1, (levels, n, k)                     # PNP_E_ARG
        assert word in L.pnp_last_error().decode(), (word, L.pnp_last_error())
    assert int(_run([exe, 'check', '3', '2', '7', '0', '0'])) == 4 and int(_run([exe, 'check', '3', '1', '2', '8', '0'])) == 5
    assert int(_run([exe, 'check', '3', '0', '4', '0', '0'])) == 3 and int(_run([exe, 'check', '3', '1', '0', '0', '0'])) == 2
    assert int(_run([exe, 'check', '3', '4', '8', '7', '7'])) == 0
    for levels in range(1, 5):
        m = 1 << levels
        t, p = _table([(a % m, (3 * a) % m) for a in range(48)])
        for k in (1, 2, 3, 4, 16):
            assert L.pnp_spin_check(levels, p, 48, k) == 0, (levels, k)
        t, p = _table([(m - 1, m - 1)] * 4096)
        assert L.pnp_spin_check(levels, p, 4096, 16) == 0
        t, p = _table([(m, 0)])
        assert L.pnp_spin_check(levels, p, 1, 1) == -1
    t, p = _table([(0, 0)])
    assert L.pnp_set_spin(None, p, 1, 1) == -1 and L.pnp_get_spin(None, None, None, None) == -1 and L.pnp_set_spin_cursor(None, 0) == -1
    assert L.pnp_dwt2_shifted(None, None, None, 1, 0, 0, 0) == -1 and L.pnp_dwt2_shifted_f64(None, None, None, 1, 1, 0, 0) == -1


def test_schedule_walks_the_table_in_groups(exe):
    """Prox step p uses entries (p mod (n / K)) K + j: the plan's wv_spin_first and the oracle's group agree, and a short table wraps."""
    table = np.arange(24).reshape(12, 2)
    for K in (1, 2, 3, 4):
        for p in (0, 1, 5, 12 // K - 1, 12 // K, 1000, 2 ** 31 - 1):
            first = int(_run([exe, 'first', str(p), '12', str(K)]))
            assert first == (p % (12 // K)) * K
            assert S.group(table, K, p) == [tuple(table[first + j]) for j in range(K)]


def test_solver_keywords_are_checked_before_an_engine_is_opened():
    """spin= without transform=, a shift out of range, spin_average outside 1..16 and a table that is no multiple of spin_average are
    ValueErrors of ADMM_L1 / ADMM_CNC on a machine without a device; 'sym8' still is no transform."""
    import pnp_admm_cnc_mri_amd as P
    mask = np.ones((128, 128), np.uint8)
    img = np.zeros((1, 128, 128), np.uint8)
    y = np.zeros((128, 128), np.complex128)
    for solver in (P.ADMM_L1, P.ADMM_CNC):
        with pytest.raises(ValueError, match='transform'):
            solver(mask, y, images=img, spin='random')
        with pytest.raises(ValueError, match='transform'):
            solver(mask, y, images=img, spin=[(0, 0)])
        with pytest.raises(ValueError, match='range'):
            solver(mask, y, images=img, transform='haar', levels=2, spin=[(0, 0), (4, 0)])
        with pytest.raises(ValueError, match='range'):
            solver(mask, y, images=img, transform='haar', levels=2, spin=[(0, -1)])
        for bad in (0, 17, -1, 2.5):
            with pytest.raises(ValueError, match='spin_average'):
                solver(mask, y, images=img, transform='db2', levels=3, spin='random', spin_average=bad)
        with pytest.raises(ValueError, match='multiple'):
            solver(mask, y, images=img, transform='db2', levels=3, spin=[(0, 0), (1, 1), (2, 2)], spin_average=2)
        with pytest.raises(ValueError, match='spin'):
            solver(mask, y, images=img, transform='db2', levels=3, spin='sobol')
        with pytest.raises(ValueError, match='spin'):
            solver(mask, y, images=img, transform='db2', levels=3, spin=[0, 1, 2])
        with pytest.raises(ValueError, match='transform'):
            solver(mask, y, images=img, transform='sym8', spin='random')


def test_binding_declares_the_spin_calls():
    from pnp_admm_cnc_mri_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read(), flags=re.S)
    new = ('pnp_spin_check', 'pnp_set_spin', 'pnp_get_spin', 'pnp_set_spin_cursor', 'pnp_dwt2_shifted', 'pnp_dwt2_shifted_f64')
    for name in new:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.lib().pnp_abi_version()
    assert _lib.lib().pnp_sparsity_check(7, 3, 256, 256) == -1                              # no new filter came with it
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import utils_pnp as U
    for solver in (P.ADMM_L1, P.ADMM_CNC):
        par = inspect.signature(solver).parameters
        assert par['spin'].default is None and par['spin_average'].default == 1 and par['spin_seed'].default == 0
        assert par['transform'].default is None and par['levels'].default == 3
        names = list(par)
        assert names.index('spin') > names.index('maps_thresh') and names.index('spin') > names.index('levels')
    for fn in (U.dwt2, U.idwt2):
        assert inspect.signature(fn).parameters['shift'].default == (0, 0)
    for attr in ('set_spin', 'spin', 'spin_cursor'):
        assert hasattr(P.Engine, attr), attr
    assert isinstance(P.Engine.spin_cursor, property) and P.Engine.spin_cursor.fset is not None
    par = inspect.signature(P.Engine.set_spin).parameters
    assert par['shifts'].default is None and par['per_prox'].default == 1


def test_spin_table():
    """'random': the documented draw, deterministic for a seed, in range, [iters * average, 2] int32; an explicit table passes through
    unchanged after checking; None -> None."""
    from pnp_admm_cnc_mri_amd.engine import spin_table
    assert spin_table(None, 3, 50) is None and spin_table(None, 3, 50, average=99) is None
    for levels in (1, 2, 3, 4):
        for iters, avg, seed in ((50, 1, 0), (10, 3, 7), (7, 16, 99)):
            t = spin_table('random', levels, iters, avg, seed)
            assert t.dtype == np.int32 and t.shape == (iters * avg, 2) and t.min() >= 0 and t.max() < 2 ** levels
            assert np.array_equal(t, np.random.default_rng(seed).integers(0, 2 ** levels, size=(iters * avg, 2)))
            assert np.array_equal(t, spin_table('random', levels, iters, avg, seed))
            assert not np.array_equal(t, spin_table('random', levels, iters, avg, seed + 1))         # 60 draws or more: never equal
    t = spin_table('random', 3, 200)
    assert set(t[:, 0]) == set(t[:, 1]) == set(range(8))                                    # both coordinates use the whole range
    mine = [(0, 0), (1, 2), (7, 7), (3, 5)]
    for avg in (1, 2, 4):
        t = spin_table(mine, 3, 50, avg)
        assert t.dtype == np.int32 and np.array_equal(t, mine)
    t64 = np.asarray(mine, np.int64)
    assert np.array_equal(spin_table(t64, 3, 1), mine) and t64.dtype == np.int64
    for bad, word in (([(0, 8)], 'range'), (mine[:3], 'multiple'), (np.zeros((2, 3), int), 'spin'), (np.zeros((2, 2)), 'spin')):
        with pytest.raises(ValueError, match=word):
            spin_table(bad, 3, 10, 2 if word == 'multiple' else 1)
    with pytest.raises(ValueError, match='spin_average'):
        spin_table('random', 3, 10, 0)
