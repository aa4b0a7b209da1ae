"""CPU tests of the locally low-rank prox (pnp_set_lowrank; include/pnp_mri.h, "low-rank"): the NumPy oracle itself
(tests/lowrank_oracle.py) -- its patch partition, the Gram route against the SVD route, the prox by its optimality condition --, the rules
that need no device through the real library and the solvers' ValueErrors before an engine is opened, the binding, and the plan's item
functions through g++ (tests/host/lowrank_emulation.cpp, plain and with the sanitizer flags of test_host_cores.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import lowrank_oracle as LO

SRC = os.path.join(ROOT, 'tests', 'host', 'lowrank_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
PLAIN = ['-O2', '-std=c++17', '-ffp-contract=off']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
L1, CNC = LO.PROX_L1, LO.PROX_CNC
SHAPES = ((128, 128), (128, 130), (130, 129), (129, 131))


def _fields(B, H, W, seed=0):
    rng = np.random.default_rng(seed + 131 * B + H + W)
    g = lambda s: s * rng.standard_normal((B, H, W))
    return g(0.5), g(0.5), g(0.3)


# ---- the oracle against itself -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('b', [5, 8, 16])
@pytest.mark.parametrize('H,W', SHAPES)
def test_partition_covers_every_pixel_once(H, W, b):
    for sy, sx in ((0, 0), (3, 2), (b - 1, b - 1), (0, b - 1), (1, 0)):
        hits = np.zeros((H, W), int)
        grid = LO.partition(H, W, b, sy, sx)
        for rows, cols in grid:
            assert 1 <= len(rows) <= b and 1 <= len(cols) <= b
            hits[rows[:, None], cols[None, :]] += 1
        assert (hits == 1).all() and len(grid) == -(-H // b) * -(-W // b)
        assert (len(grid[-1][0]), len(grid[-1][1])) == (H % b or b, W % b or b) and grid[0][0][0] == sy and grid[0][1][0] == sx


@pytest.mark.parametrize('T,b,H,W', [(2, 5, 24, 26), (5, 8, 26, 24), (16, 16, 35, 33), (17, 5, 21, 23), (64, 8, 20, 17)])
def test_gram_route_equals_svd_route(T, b, H, W):
    """G = X^T X, its eigen-decomposition, X (V g V^T) == the SVD, in double: 1e-12 (partial patches with fewer than T pixels included)"""
    x, z, w = _fields(2 * T, H, W, seed=T)
    for kind, pr in (('l1', L1), ('cnc', CNC)):
        a, c = LO.prox(kind, x, z, w, pr, T, b, (b - 1, 1)), LO.prox(kind, x, z, w, pr, T, b, (b - 1, 1), route='gram')
        assert a[0].dtype == np.float64 and LO.rel(c[0], a[0]) <= 1e-12 and LO.rel(c[1], a[1]) <= 1e-12, (kind, T)
        assert np.abs(a[0]).max() > 0.05


@pytest.mark.parametrize('T,b', [(3, 5), (8, 8), (16, 16), (40, 5)])
def test_prox_by_its_optimality_condition(T, b):
    """z+ minimises 1/2 ||z - u||_F^2 + thr ||z||_* on every patch: u - z+ = thr (U1 V1^T + R) with U1, V1 the singular vectors z+ keeps,
    ||R||_2 <= 1, and R orthogonal to the kept spaces (U1^T R = 0, R V1 = 0); w+ = u - z+."""
    H, W, shift = 22, 27, (2, b - 1)
    scale = LO.default_scale(b)
    thr = L1['reo'] * L1['lambda1'] * scale
    # the singular values of a full patch of this noise lie around 0.58 f (sqrt(P) +- sqrt(T)): f puts thr among them
    x, z, w = (thr / (0.58 * b) * a for a in _fields(T, H, W, seed=5))
    zn, wn = LO.prox('l1', x, z, w, L1, T, b, shift)
    u = x + w
    assert np.abs(wn - (u - zn)).max() <= 1e-15
    kept = dropped = 0
    for rows, cols in LO.partition(H, W, b, *shift):
        X = lambda a: a[:, rows[:, None], cols[None, :]].reshape(T, -1).T
        Z, D = X(zn), X(u) - X(zn)
        U, s, Vt = np.linalg.svd(Z, full_matrices=False)
        k = int((s > 1e-10).sum())
        kept, dropped = kept + k, dropped + len(s) - k
        U1, V1 = U[:, :k], Vt[:k].T
        Rm = D / thr - U1 @ V1.T
        assert np.linalg.norm(Rm, 2) <= 1 + 1e-10
        assert np.abs(U1.T @ Rm).max(initial=0) <= 1e-10 and np.abs(Rm @ V1).max(initial=0) <= 1e-10
    assert kept > 0 and dropped > 0


def test_float_restatement_is_close_and_distinct():
    x, z, w = _fields(10, 24, 27, seed=3)
    a, c = LO.prox('cnc', x, z, w, CNC, 5, 8), LO.prox('cnc', x, z, w, CNC, 5, 8, R=np.float32)
    assert c[0].dtype == np.float32 and 0 < LO.rel(c[0], a[0]) < 1e-5


def test_shift_table():
    t = LO.shift_table('random', 8, 0)
    assert t.shape == (64, 2) and t.dtype == np.int32 and t.min() >= 0 and t.max() < 8
    assert np.array_equal(t, np.random.default_rng(0).integers(0, 8, size=(64, 2)))
    assert np.array_equal(LO.shift_table(None, 8), [[0, 0]])


def test_oracle_psnr_gap_on_the_relaxation_phantom():
    """the regulariser does what it is for, in the oracle: after the 50 iterations of DESIGN.md's table low-rank ADMM_L1 (b = 8, the random
    table of seed 0) ends at least 2.3 dB above pixel ADMM_L1, so that the GPU test's bound (this gap - 0.5 dB) stays near the 2 dB asked
    of the library"""
    img, masks, y = LO.relaxation_problem(16, 128, 128)
    pix = LO.TO.loop(y, masks, 50, 'l1', LO.PRESETS['l1'])[0]
    llr = LO.loop(y, masks, 50, 'l1', LO.PRESETS['l1'], 16, 8, 'random')[0]
    assert LO.psnr(llr, img) - LO.psnr(pix, img) >= 2.3


# ---- the library's rules without a device ----------------------------------------------------------------------------------------------

def test_lowrank_check_codes_and_messages():
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    msg = lambda: L.pnp_last_error().decode()
    E_ARG, E_STATE = -1, -3
    for T in (2, 3, 17, 64):
        for f64 in (0, 1):
            for cnc in (0, 1):
                for b in (2, 5, 8):
                    assert L.pnp_lowrank_check(T, b, 128, 130, 3 * T, f64, cnc) == 0
                if T <= 16:
                    assert L.pnp_lowrank_check(T, 16, 128, 130, T, f64, cnc) == 0
    for f in (-1, 0, 1, 65):
        assert L.pnp_lowrank_check(f, 8, 128, 128, 128, 0, 0) == E_ARG and msg() == 'temporal: frames must be 2..64 (got %d)' % f
    for b in (-3, 0, 1, 33):
        assert L.pnp_lowrank_check(4, b, 128, 128, 8, 0, 0) == E_ARG and msg() == 'lowrank: block must be 2..32 (got %d)' % b
    assert L.pnp_lowrank_check(4, 16, 128, 12, 8, 0, 0) == E_ARG and msg() == 'lowrank: block 16 exceeds the image (128 x 12)'
    assert L.pnp_lowrank_check(64, 32, 128, 128, 64, 0, 0) == E_ARG
    assert msg() == 'lowrank: a patch of 32 x 32 pixels over 64 frames does not fit the LDS of a workgroup in float (L1)'
    assert L.pnp_lowrank_check(64, 16, 128, 128, 64, 1, 1) == E_ARG
    assert msg() == 'lowrank: a patch of 16 x 16 pixels over 64 frames does not fit the LDS of a workgroup in double (CNC)'
    for f, B in ((4, 6), (16, 17), (5, 0)):
        assert L.pnp_lowrank_check(f, 8, 128, 128, B, 0, 0) == E_STATE
        assert msg() == 'temporal: the batch of %d slices is not a whole number of series of %d frames' % (B, f)


def test_symbols_in_header_and_binding():
    from pnp_admm_cnc_mri_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read()
    assert 'low-rank' in hdr and re.search(r'#define PNP_ABI_VERSION\s+13\b', hdr)
    for name, proto in (('pnp_lowrank_check', 'int pnp_lowrank_check(int frames, int block, int H, int W, int B, int f64, int cnc);'),
                        ('pnp_set_lowrank', 'int pnp_set_lowrank(pnp_ctx* ctx, int block, double scale, const int32_t* shifts, int n_shifts);'),
                        ('pnp_get_lowrank', 'int pnp_get_lowrank(pnp_ctx* ctx, int* block, double* scale, int* n_shifts, int* cursor);'),
                        ('pnp_set_lowrank_cursor', 'int pnp_set_lowrank_cursor(pnp_ctx* ctx, int cursor);')):
        assert proto in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)


def _refuse_engine(monkeypatch):
    import pnp_admm_cnc_mri_amd.solvers as S

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError('an engine was opened')
    monkeypatch.setattr(S, 'Engine', NoEngine)


@pytest.mark.parametrize('name', ['ADMM_L1', 'ADMM_CNC'])
def test_lowrank_value_errors_before_an_engine(name, monkeypatch):
    import pnp_admm_cnc_mri_amd as P
    _refuse_engine(monkeypatch)
    fn = getattr(P, name)
    m, y = np.ones((128, 128), np.uint8), np.zeros((6, 128, 128), np.complex64)
    with pytest.raises(ValueError, match=r'^lowrank= \(locally low-rank prox\) needs frames= \(the series length\)$'):
        fn(m, None, y=y, lowrank=8)
    for kw in (dict(transform='haar'), dict(transform='db2', spin='random')):
        with pytest.raises(ValueError, match=r'^frames= \(temporal sparsity\) does not run with transform= / spin= '):
            fn(m, None, y=y, frames=3, lowrank=8, **kw)
    with pytest.raises(ValueError, match=r'^lowrank= does not run with image=\'complex\' \(real images only\)$'):
        fn(m, None, y=y, frames=3, lowrank=8, image='complex', coils=np.ones((2, 128, 128), np.complex64))
    with pytest.raises(ValueError, match=r'^lowrank= has no unpenalised coefficient: temporal_keep_dc=False does not apply$'):
        fn(m, None, y=y, frames=3, lowrank=8, temporal_keep_dc=False)
    for b in (1, 33):
        with pytest.raises(ValueError, match=r'^lowrank: block must be 2\.\.32 \(got %d\)$' % b):
            fn(m, None, y=y, frames=3, lowrank=b)
    with pytest.raises(ValueError, match=r'^lowrank must be an integer \(got 2\.5\)$'):
        fn(m, None, y=y, frames=3, lowrank=2.5)
    with pytest.raises(ValueError, match=r'^temporal: the batch of 6 slices is not a whole number of series of 4 frames$'):
        fn(m, None, y=y, frames=4, lowrank=8)
    with pytest.raises(ValueError, match=r'^lowrank: a patch of 32 x 32 pixels over 64 frames does not fit the LDS of a workgroup in double'):
        fn(m, None, y=y, frames=64, lowrank=32, precision='f64')
    with pytest.raises(ValueError, match=r'^lowrank_shift: entry 1 = \(8, 0\) out of range \[0, 8\)$'):
        fn(m, None, y=y, frames=3, lowrank=8, lowrank_shift=[[0, 0], [8, 0]])
    with pytest.raises(ValueError, match=r'^lowrank_scale must be a positive number \(got -1\)$'):
        fn(m, None, y=y, frames=3, lowrank=8, lowrank_scale=-1)
    with pytest.raises(AssertionError, match='an engine was opened'):          # a valid request reaches the engine ...
        fn(m, None, y=y, frames=3, lowrank=8)
    with pytest.raises(AssertionError, match='an engine was opened'):          # ... and lowrank=None asks nothing
        fn(m, None, y=y, frames=3, lowrank=None)


def test_engine_table_is_the_oracles():
    from pnp_admm_cnc_mri_amd import engine
    for b, seed in ((8, 0), (5, 3)):
        assert np.array_equal(engine.lowrank_table('random', b, seed), LO.shift_table('random', b, seed))
    assert np.array_equal(engine.lowrank_table(None, 8), [[0, 0]])
    assert np.array_equal(engine.lowrank_table([[1, 2], [3, 4]], 8), [[1, 2], [3, 4]])


# ---- host emulation --------------------------------------------------------------------------------------------------------------------

# (T, S, H, W, b, shift, kind): partial last patch rows and columns (fewer than T pixels at T = 17, 64), every group size from one patch
# (b = 16, T = 16 in double) to sixteen, an odd T (a padded ordering), shifts that wrap both axes
EMU_CASES = ((2, 2, 13, 19, 5, (0, 0), 'l1'), (3, 1, 17, 22, 8, (3, 2), 'cnc'), (5, 2, 12, 21, 5, (4, 4), 'cnc'),
             (16, 1, 35, 33, 16, (15, 15), 'cnc'), (16, 1, 20, 37, 16, (0, 7), 'l1'), (17, 1, 11, 18, 5, (3, 2), 'l1'),
             (64, 1, 9, 26, 8, (7, 7), 'cnc'), (64, 1, 10, 9, 8, (2, 5), 'l1'), (8, 1, 9, 150, 2, (1, 1), 'cnc'))


def _write_case(path, T, S, H, W, b, shift, kind):
    x, z, w = _fields(S * T, H, W, seed=T)
    x[:, :b, :b] = z[:, :b, :b] = w[:, :b, :b] = 0                                  # a zero patch somewhere
    pr = L1 if kind == 'l1' else CNC
    zn, wn = LO.prox(kind, x, z, w, pr, T, b, shift)
    sc = [float(v) for v in LO.scalars(kind, pr, LO.default_scale(b))]
    np.concatenate([np.array([T, S, H, W, b, shift[0], shift[1], int(kind == 'cnc')] + sc, np.float64)] + [a.ravel() for a in (x, z, w, zn, wn)]).tofile(path)


@pytest.mark.parametrize('flags', [PLAIN, SAN], ids=['plain', 'sanitized'])
def test_host_emulation(flags, tmp_path):
    """lowrank_plan.h's item functions group by group as a stand-alone program (nothing is preloaded): arrays of exactly the plan's sizes,
    the LDS block poisoned with NaN before every group, every pixel-frame written exactly once and nothing else touched, the result equal
    to the oracle's SVD to 1e-12 in double (2e-5 in float); the plan's promises (b <= 8 at every T, b = 16 up to T = 16) and the
    round-robin ordering (every pair once a sweep) are checked by the program itself."""
    exe = str(tmp_path / 'lowrank_emulation')
    subprocess.check_call(['g++'] + flags + ['-o', exe, SRC])
    paths = []
    for i, c in enumerate(EMU_CASES):
        paths.append(str(tmp_path / ('case%d.bin' % i)))
        _write_case(paths[-1], *c)
    r = subprocess.run([exe] + paths, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stdout.decode()[-1500:], r.stderr.decode()[-1500:])
    out = r.stdout.decode()
    assert out.rstrip().endswith('ok') and '%d cases, 0 bad' % len(EMU_CASES) in out and 'DIFFER' not in out and 'COVERAGE' not in out
    for p, (T, S, H, W, b, shift, kind) in zip(paths, EMU_CASES):
        for prec in ('double', 'float'):
            assert re.search(r'%s %s T=%d S=%d %dx%d b=%d shift=\(%d,%d\) %s Q=\d+ lds=\d+ err=\S+ relz=\S+ ok' % (re.escape(p), prec, T, S, H, W, b, shift[0], shift[1], kind), out)
    groups = {int(v) for v in re.findall(r' Q=(\d+) ', out)}
    assert 1 in groups and 16 in groups and len(groups) >= 4
