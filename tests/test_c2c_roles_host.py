"""CPU tests of the row / column roles of the c2c kernels (csrc/c2c_roles.h, the header kernels_generic.hip and kernels_anysize.hip
include): compiled with g++ and checked against NumPy expressions of the same formulas -- the operators' definitions for the inputs,
epilogues and k-space ops, oracle/admm_oracle.py for the prox -- in double and in float, and the two lists of legal triples.

Results are compared exactly wherever NumPy rounds as the header does (one rounding per operation, -ffp-contract=off).  The header's
fused multiply-adds (MID_BLEND, the CNC combination) are not NumPy's: there the tolerances are those tests/test_host_cores.py uses for
the same formulas (relative L2 of x and z, worst |w|: 2e-6 in float; 2e-15 / 2e-14 in double)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import rel_l2, ROOT

SRC = os.path.join(ROOT, 'tests', 'host', 'c2c_roles_emulation.cpp')
N = 4099                       # odd; every mask / sign / clip case occurs many times

IN_COMPLEX, IN_REAL, IN_REAL_DIFF = 0, 1, 2
EPI_COMPLEX, EPI_ABS_REAL, EPI_ABS_COMPLEX, EPI_L1, EPI_CNC = 0, 1, 2, 3, 4
MID_NONE, MID_BLEND, MID_MASK, MID_RESID, MID_MASK_ADD = 0, 1, 2, 3, 4

# the legal triples and their one user each (csrc/api.hip)
ROW_TRIPLES = {
    (IN_COMPLEX, 0, EPI_COMPLEX),         # fft2
    (IN_REAL, 0, EPI_COMPLEX),            # A, synthesis
    (IN_REAL_DIFF, 0, EPI_COMPLEX),       # the iteration: z - w
    (IN_COMPLEX, 1, EPI_COMPLEX),         # ifft2
    (IN_COMPLEX, 1, EPI_ABS_REAL),        # the iteration's x
    (IN_COMPLEX, 1, EPI_ABS_COMPLEX),     # the initial state
    (IN_COMPLEX, 1, EPI_L1),
    (IN_COMPLEX, 1, EPI_CNC),
}
COL_TRIPLES = {
    (1, MID_NONE, 0), (0, MID_NONE, 1),   # fft2, ifft2
    (1, MID_BLEND, 1),                    # the iteration's data consistency
    (1, MID_MASK, 0), (0, MID_MASK, 1),   # A, A^H
    (1, MID_MASK, 1),                     # the coil columns of G
    (1, MID_RESID, 1),                    # Df
    (1, MID_MASK_ADD, 0),                 # synthesis
}

REO, LAM, ALPHA, B = 0.0625, 0.5, 0.5, 64           # exact in float, as in test_host_cores.py
SCALE = 1.0 / 256
C_DC = 1.0 / (1.0 + 1.0 / 2.0 / REO)


def _compile(d, extra=()):
    exe = str(d / 'c2c_roles_emulation')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off'] + list(extra) + ['-o', exe, SRC])
    return exe


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp('c2c_roles')
    return _compile(d), d


def _inputs():
    rng = np.random.default_rng(2024)
    cplx = lambda s=1.0: (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * s
    d = dict(cin=cplx(), rin0=rng.uniform(0, 1, N), rin1=rng.uniform(-0.1, 0.1, N),
             v=cplx(100.0),                                     # unnormalised transform output: x = |Re v * scale| up to ~1
             z=rng.uniform(-0.2, 1, N), w=rng.uniform(-0.1, 0.1, N), X=cplx(10.0), y=cplx(10.0),
             mask=(rng.uniform(0, 1, N) < 0.3).astype(np.uint8))
    d['z'][:64] = np.linspace(-2.0 / B, 2.0 / B, 64)            # both sides of the inner clip level 1 / b
    d['v'][:8] = 0                                              # x = 0
    return d


def _prox_scalars(dtype):
    """thr, c1, c2, c3, ib as the host combines them: in double, rounded once"""
    return [dtype(v) for v in (ALPHA * REO * LAM, 1 - ALPHA, ALPHA, ALPHA * REO * LAM * B, 1.0 / B)]


def _run(emu, d, l1):
    """-> {precision: {name: array}}; the L1 run takes thr = reo * lambda1, the CNC run the CNC scalars (one ProxParams per run)"""
    exe, tmp = emu
    inp, out = str(tmp / 'in.bin'), str(tmp / 'out.bin')
    prox = [REO * LAM, 0, 0, 0, 0] if l1 else [float(v) for v in _prox_scalars(np.float64)]
    with open(inp, 'wb') as f:
        f.write(struct.pack('<i7d', N, SCALE, C_DC, *prox))
        for k in ('cin', 'rin0', 'rin1', 'v', 'z', 'w', 'X', 'y'):
            a = d[k]
            f.write(np.ascontiguousarray(a, np.complex128 if np.iscomplexobj(a) else np.float64).tobytes())
        f.write(d['mask'].tobytes())
    subprocess.check_call([exe, inp, out])
    raw, o, res = np.fromfile(out, np.float64), 0, {}
    assert raw.size == 52 * N
    for prec in ('double', 'float'):
        r = {}
        for name, cplx in (('load0', 1), ('load1', 1), ('load2', 1), ('cout', 1), ('abs_real', 0), ('abs_complex', 0),
                           ('l1_z', 0), ('l1_w', 0), ('l1_x', 0), ('cnc_z', 0), ('cnc_w', 0), ('cnc_x', 0),
                           ('none', 1), ('blend', 1), ('mask', 1), ('resid', 1), ('mask_add', 1)):
            n = N * (2 if cplx else 1)
            a = raw[o:o + n]; o += n
            r[name] = a.view(np.complex128) if cplx else a
        res[prec] = r
    return res


def _typed(d, prec):
    """the values the run of `prec` received: rounded to float for the float run"""
    rt, ct = (np.float64, np.complex128) if prec == 'double' else (np.float32, np.complex64)
    return {k: (a if k == 'mask' else a.astype(ct if np.iscomplexobj(a) else rt)) for k, a in d.items()}, rt, ct


def _same(a, b):
    """equal as values, NaN nowhere (-0 == +0: soft of the header and of the oracle differ in the sign of a zero)"""
    return a.shape == b.shape and bool(np.all(np.asarray(a) == np.asarray(b)))


@pytest.fixture(scope='module')
def runs(emu):
    d = _inputs()
    return d, _run(emu, d, l1=True), _run(emu, d, l1=False)


@pytest.mark.parametrize('prec', ['double', 'float'])
def test_row_inputs_and_plain_epilogues(runs, prec):
    d, r, _ = runs
    t, rt, ct = _typed(d, prec)
    got = r[prec]
    assert _same(got['load0'], t['cin'].astype(np.complex128))
    assert _same(got['load1'], t['rin0'].astype(np.complex128))
    assert _same(got['load2'], (t['rin0'] - t['rin1']).astype(np.complex128))          # one subtraction in the run's precision
    s = rt(SCALE)
    assert _same(got['cout'].real, (t['v'].real * s).astype(np.float64)) and _same(got['cout'].imag, (t['v'].imag * s).astype(np.float64))
    assert _same(got['abs_real'], np.abs(t['v'].real * s).astype(np.float64))
    re, im = t['v'].real, t['v'].imag
    assert _same(got['abs_complex'], (np.sqrt(re * re + im * im) * s).astype(np.float64))


@pytest.mark.parametrize('prec', ['double', 'float'])
def test_prox_epilogues_against_oracle(runs, prec):
    d, r_l1, r_cnc = runs
    t, rt, _ = _typed(d, prec)
    x = np.abs(t['v'].real * rt(SCALE))
    # L1: x + w, |u| - thr, u - z are single operations: the oracle evaluated in the run's precision is the same arithmetic
    zr, wr = O.l1_step(x, t['z'], t['w'], rt(LAM), rt(REO))
    assert zr.dtype == rt and wr.dtype == rt
    got = r_l1[prec]
    assert _same(got['l1_x'], x.astype(np.float64))
    assert _same(got['l1_z'], zr.astype(np.float64)) and _same(got['l1_w'], wr.astype(np.float64))
    assert np.count_nonzero(zr) > N // 4 and np.count_nonzero(zr == 0) > N // 100
    # CNC: the header combines c1 z + c2 u + c3 clip(z) with fused multiply-adds on pre-combined scalars: the bounds of test_host_cores.py
    tol = 2e-6 if prec == 'float' else 2e-14
    z64, w64, x64 = (a.astype(np.float64) for a in (t['z'], t['w'], x))
    zr, wr = O.cnc_step(x64, z64, w64, ALPHA, LAM, REO, B)
    got = r_cnc[prec]
    assert _same(got['cnc_x'], x64)
    print(prec, 'cnc: z', rel_l2(got['cnc_z'], zr), 'w', np.abs(got['cnc_w'] - wr).max())
    assert rel_l2(got['cnc_z'], zr) <= tol
    assert np.abs(got['cnc_w'] - wr).max() <= tol
    assert np.count_nonzero(np.abs(z64) > 1.0 / B) > N // 4 and np.count_nonzero(np.abs(z64) < 1.0 / B) >= 30


def _mid_reference(t, rt):
    """the k-space ops from the operators' definitions, on the run's inputs widened to double (exact ops: in the run's precision)"""
    X, y, m = t['X'], t['y'], t['mask'] != 0
    zero = np.zeros_like(X)
    X128, y128 = X.astype(np.complex128), y.astype(np.complex128)
    La2 = 1.0 / 2.0 / REO
    blend = X128.copy()
    blend[m] = (La2 * X128[m] + y128[m]) / (1.0 + La2)           # oracle dc_step
    return dict(none=X, blend=blend, mask=np.where(m, X, zero), resid=np.where(m, X - y, zero), mask_add=np.where(m, X + y, y))


@pytest.mark.parametrize('prec', ['double', 'float'])
def test_column_ops(runs, prec):
    d, r, _ = runs
    t, rt, _ = _typed(d, prec)
    ref, got = _mid_reference(t, rt), r[prec]
    for name in ('none', 'mask', 'resid', 'mask_add'):
        assert _same(got[name], ref[name].astype(np.complex128)), name
    m = t['mask'] != 0
    assert _same(got['blend'][~m], t['X'][~m].astype(np.complex128))             # unsampled: untouched
    tol = 2e-6 if prec == 'float' else 2e-15
    print(prec, 'blend', rel_l2(got['blend'], ref['blend']))
    assert rel_l2(got['blend'][m], ref['blend'][m]) <= tol
    assert 0 < np.count_nonzero(m) < N


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_unsampled_measurements_never_reach_the_result(emu, runs, bad):
    d, clean, _ = runs
    dirty = dict(d)
    dirty['y'] = d['y'].copy()
    dirty['y'][d['mask'] == 0] = complex(bad, bad)
    r = _run(emu, dirty, l1=True)
    for prec in ('double', 'float'):
        for name in ('blend', 'resid', 'mask'):
            assert np.all(np.isfinite(r[prec][name])), (prec, name)
            assert _same(r[prec][name], clean[prec][name]), (prec, name)
        # MASK_ADD: y is the noise, added where sampled and returned alone elsewhere
        m = d['mask'] != 0
        _, rt, ct = _typed(d, prec)
        assert _same(r[prec]['mask_add'][m], clean[prec]['mask_add'][m])
        un = r[prec]['mask_add'][~m]
        assert np.all(np.isnan(un.real) & np.isnan(un.imag)) if np.isnan(bad) else np.all((un.real == bad) & (un.imag == bad))
        assert _same(clean[prec]['mask_add'][~m], d['y'][~m].astype(ct).astype(np.complex128))


def test_dispatchers_reach_exactly_the_listed_triples(emu):
    lines = subprocess.check_output([emu[0], 'triples']).decode().split('\n')
    rows = [l.split() for l in lines if l.startswith('row')]
    cols = [l.split() for l in lines if l.startswith('col')]
    assert len(rows) == 3 * 2 * 5 and len(cols) == 2 * 5 * 2
    for listed, table in ((ROW_TRIPLES, rows), (COL_TRIPLES, cols)):
        seen = set()
        for l in table:
            asked = tuple(int(v) for v in l[1:4])
            assert asked not in seen
            seen.add(asked)
            if asked in listed:
                assert l[4] == '->' and tuple(int(v) for v in l[5:8]) == asked, l       # the callee got the constants of the triple
            else:
                assert l[4:] == ['->', 'invalid'], l
        assert listed <= seen
    assert len(ROW_TRIPLES) == 8 and len(COL_TRIPLES) == 8


def test_roles_under_address_and_ub_sanitizers(emu, runs, tmp_path):
    """the stand-alone program built with -fsanitize=address,undefined: y is a null pointer wherever a role must not read it"""
    exe = _compile(tmp_path, ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    d, clean, _ = runs
    r = _run((exe, tmp_path), d, l1=True)
    for prec in ('double', 'float'):
        for name, a in clean[prec].items():
            assert _same(r[prec][name], a), (prec, name)
    subprocess.check_call([exe, 'triples'], stdout=subprocess.DEVNULL)
