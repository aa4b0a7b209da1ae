"""CPU tests of the any-size FFT's host plan and butterfly arithmetic (csrc/anysize_plan.h, the header kernels_anysize.hip
includes): compiled with g++, checked against np.fft.  Pins the factorisation, the Bluestein length, the fp64 twiddle, chirp
and kernel tables, and one forward and one inverse line transform per length, before anything runs on a GPU.

The sweep runs every length from 128 to 1024 in double and in float (the float tables and butterflies of a float context) and
bounds two error measures per length: the relative L2 norm of a line and its worst single bin against the line's rms.  A fixed
subset of shapes is also transformed in two dimensions; its worst figures are the recorded results of
tests/golden/anysize_sweep_bounds.json, over which the GPU sweep sets its per-element bounds.  Regenerate that file with
    python tests/test_anysize_host.py --write-bounds"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import anysize_common as AC

SRC = os.path.join(ROOT, 'tests', 'host', 'anysize_emulation.cpp')
SIZES = (128, 170, 192, 218, 320, 368, 384, 640, 1000, 1021, 1024, 224, 243, 343, 729, 945)

# Bounds of the 1-D sweep: 4 x the worst value measured over all 897 lengths (seeded inputs, g++ -O2 -ffp-contract=off, against
# np.fft in complex128).  The error is a sum of independent roundings; its worst case over 897 inputs moves by a small factor with
# the seed, which the 4 covers.  Measured worst values, forward and inverse together:
#   double  relative L2  6.982e-16 (n = 971, inverse)  (bound: the 1e-12 of the per-length test)
#   double  per bin      2.505e-15 (n = 1002, inverse)
#   float   relative L2  1.851e-7  (n = 1010, forward)
#   float   per bin      7.489e-7  (n = 703, inverse)
L2_DOUBLE = 1e-12
MAX_DOUBLE = 4 * 2.505e-15
L2_FLOAT = 4 * 1.851e-7
MAX_FLOAT = 4 * 7.489e-7


def _compile(d):
    """-ffp-contract=off: only the header's own fma calls are fused.  -mfma where the CPU has the instruction makes those calls one
    instruction, not a library call (the same correctly rounded result, several times as fast)."""
    exe = str(d / 'anysize_emulation')
    try:
        fma = ['-mfma'] if ' fma ' in open('/proc/cpuinfo').read() else []
    except OSError:
        fma = []
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off'] + fma + ['-o', exe, SRC])
    return exe


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp('anysize')
    return _compile(d), d


def _run(emu, n, x):
    exe, d = emu
    inp, out = str(d / 'in.bin'), str(d / 'out.bin')
    np.ascontiguousarray(x, np.complex128).tofile(inp)
    subprocess.check_call([exe, str(n), inp, out])
    raw = open(out, 'rb').read()
    hdr = np.frombuffer(raw[:16 * 4], np.int32)
    body = np.frombuffer(raw[16 * 4:], np.complex128)
    nn, blue, m, ns = (int(v) for v in hdr[:4])
    radix = [int(r) for r in hdr[4:4 + ns]]
    parts, o = [], 0
    for ln in (m, n, m, n, n):
        parts.append(body[o:o + ln]); o += ln
    assert o == body.size
    return dict(n=nn, bluestein=blue, m=m, radix=radix, tw=parts[0], chirp=parts[1], kern=parts[2], fwd=parts[3], inv=parts[4])


def _smooth7(n):
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def _check_plan(r, n):
    """plan: a Stockham length, factorised into the supported radices"""
    assert r['n'] == n
    assert r['bluestein'] == (0 if _smooth7(n) else 1)
    if r['bluestein']:
        m = r['m']
        assert m & (m - 1) == 0 and m >= 2 * n - 1 and m // 2 < 2 * n - 1 and m <= 2048
    else:
        assert r['m'] == n
    assert all(q in (2, 3, 4, 5, 7) for q in r['radix']) and int(np.prod(r['radix'])) == r['m']


def _table_error(table, k, L):
    """max |table - exp(-2 pi i k / L)| against roots computed in extended precision.  np.exp of the same angle in float64 is itself
    off by up to 1.5e-15 (the angle, up to 2 pi, is rounded twice before cos and sin see it), more than the bound on the table."""
    LD = np.longdouble
    assert np.finfo(LD).eps < 1e-18, 'this check needs a long double wider than double'
    a = 2 * LD('3.14159265358979323846264338327950288') * k.astype(LD) / L
    return float(np.max(np.hypot(table.real - np.cos(a), table.imag + np.sin(a))))


@pytest.mark.parametrize('n', SIZES)
def test_plan_tables_and_transform(emu, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    r = _run(emu, n, x)
    _check_plan(r, n)
    # tables in fp64
    m = r['m']
    assert _table_error(r['tw'], np.arange(m), m) <= 1e-15
    if r['bluestein']:
        j = np.arange(n)
        assert _table_error(r['chirp'], j * j % (2 * n), 2 * n) <= 1e-15
        b = np.zeros(m, np.complex128)
        b[:n] = np.conj(r['chirp'])
        b[m - n + 1:] = np.conj(r['chirp'][1:])[::-1]
        kern = np.fft.fft(b) / m
        assert np.max(np.abs(r['kern'] - kern)) <= 1e-12 * np.max(np.abs(kern))
    # one line transform, forward (np.fft.fft) and unnormalised inverse (n * np.fft.ifft)
    ref_f, ref_i = np.fft.fft(x), np.fft.ifft(x) * n
    assert np.linalg.norm(r['fwd'] - ref_f) / np.linalg.norm(ref_f) <= 1e-12
    assert np.linalg.norm(r['inv'] - ref_i) / np.linalg.norm(ref_i) <= 1e-12


# ------------------------------------------------------------------------------------------------
# every length, both precisions
# ------------------------------------------------------------------------------------------------
def _line_input(n):
    rng = np.random.default_rng(n)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _run_sweep(exe, d):
    """-> {n: plan facts and, per precision, ((L2, max, bin) forward, (L2, max, bin) inverse)} for every length"""
    inp, out = str(d / 'sweep_in.bin'), str(d / 'sweep_out.bin')
    xs = {n: _line_input(n) for n in AC.LENGTHS}
    np.concatenate([xs[n] for n in AC.LENGTHS]).tofile(inp)
    subprocess.check_call([exe, 'sweep', inp, out])
    raw, o, res = open(out, 'rb').read(), 0, {}
    for n in AC.LENGTHS:
        hdr = np.frombuffer(raw, np.int32, 16, o); o += 64
        r = dict(n=int(hdr[0]), bluestein=int(hdr[1]), m=int(hdr[2]), radix=[int(q) for q in hdr[4:4 + int(hdr[3])]])
        for name, dt, x in (('double', np.complex128, xs[n]), ('float', np.complex64, xs[n].astype(np.complex64))):
            got = np.frombuffer(raw, dt, 2 * n, o); o += 2 * n * np.dtype(dt).itemsize
            x = x.astype(np.complex128)                   # the values the emulation received, widened
            r[name] = (AC.errors(got[:n], np.fft.fft(x)), AC.errors(got[n:], np.fft.ifft(x) * n))
        res[n] = r
    assert o == len(raw)
    return res


@pytest.fixture(scope='module')
def swept(emu):
    return _run_sweep(*emu)


def _worst(swept, prec, k):
    """(worst value, its length, 'fwd' or 'inv') of measure k (0: relative L2, 1: per bin) over the sweep"""
    return max((swept[n][prec][d][k], n, ('fwd', 'inv')[d]) for n in AC.LENGTHS for d in (0, 1))


def test_sweep_plans(swept):
    assert sorted(swept) == list(AC.LENGTHS) and len(swept) == 897
    for n in AC.LENGTHS:
        _check_plan(swept[n], n)
        assert swept[n]['m'] == AC.stockham_length(n) and swept[n]['radix'] == AC.radices(swept[n]['m']), n
    # what the sweep must reach: every radix, a plan of one odd radix alone, and the three Bluestein lengths
    assert {q for n in AC.LENGTHS for q in swept[n]['radix']} == {2, 3, 4, 5, 7}
    assert {swept[n]['m'] for n in AC.LENGTHS if swept[n]['bluestein']} == {512, 1024, 2048}
    assert swept[343]['radix'] == [7, 7, 7] and swept[729]['radix'] == [3] * 6 and swept[625]['radix'] == [5] * 4


@pytest.mark.parametrize('prec, l2_bound, max_bound', [('double', L2_DOUBLE, MAX_DOUBLE), ('float', L2_FLOAT, MAX_FLOAT)])
def test_sweep_every_length_against_numpy(swept, prec, l2_bound, max_bound):
    print('worst over 897 lengths, %s: relative L2 %.3e (n = %d, %s), per bin %.3e (n = %d, %s)'
          % ((prec,) + _worst(swept, prec, 0) + _worst(swept, prec, 1)))
    for n in AC.LENGTHS:
        for d, (l2, mx, at) in zip(('fwd', 'inv'), swept[n][prec]):
            assert l2 <= l2_bound, (prec, n, d, l2)
            assert mx <= max_bound, (prec, n, d, mx, 'bin %d' % at[0])


# ------------------------------------------------------------------------------------------------
# two dimensions: the figures the GPU sweep's per-element bounds stand on
# ------------------------------------------------------------------------------------------------
def grid_input(H, W):
    rng = np.random.default_rng(AC.shape_seed(H, W))
    return rng.standard_normal((H, W)) + 1j * rng.standard_normal((H, W))


def _grid_shape(exe, d, H):
    """{precision: {'fwd' | 'inv': (relative L2, per bin)}} of the emulation's fft2 / ifft2 (rows, then columns) of one seeded
    (H, pair(H)) array against np.fft.fft2 / np.fft.ifft2 of the values the emulation received."""
    W = AC.pair(H)
    inp, out = str(d / ('grid_in_%d.bin' % H)), str(d / ('grid_out_%d.bin' % H))
    x = grid_input(H, W)
    x.tofile(inp)
    subprocess.check_call([exe, 'grid', str(H), str(W), inp, out])
    raw, o, res = np.fromfile(out, np.uint8), 0, {}
    for prec, dt, xin in (('double', np.complex128, x), ('float', np.complex64, x.astype(np.complex64))):
        got = np.frombuffer(raw, dt, 2 * H * W, o).reshape(2, H, W); o += 2 * H * W * np.dtype(dt).itemsize
        xin = xin.astype(np.complex128)
        res[prec] = {'fwd': AC.errors(got[0], np.fft.fft2(xin))[:2],
                     'inv': AC.errors(got[1].astype(np.complex128) / (H * W), np.fft.ifft2(xin))[:2]}
    assert o == raw.size
    os.remove(inp)
    os.remove(out)
    return res


def _grid_figures(exe, d):
    """Worst relative L2 and worst per-bin error over the shapes (H, pair(H)), H in GRID_LENGTHS, and where.  The shapes are
    independent: a few run at a time (the emulation is a process of its own and np.fft releases the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        per = list(pool.map(lambda H: _grid_shape(exe, d, H), AC.GRID_LENGTHS))
    fig = {p: {k: {} for k in ('fwd', 'inv')} for p in ('double', 'float')}
    for prec in fig:
        for k in fig[prec]:
            for i, meas in enumerate(('l2', 'max')):
                v, H = max((r[prec][k][i], H) for r, H in zip(per, AC.GRID_LENGTHS))
                fig[prec][k][meas], fig[prec][k][meas + '_shape'] = v, [H, AC.pair(H)]
    return fig


def test_grid_subset_reaches_every_plan_kind():
    for axis in (lambda H: H, AC.pair):
        ns = [axis(H) for H in AC.GRID_LENGTHS]
        assert {q for n in ns for q in AC.radices(AC.stockham_length(n))} == {2, 3, 4, 5, 7}
        assert {AC.stockham_length(n) for n in ns if not AC.smooth7(n)} == {512, 1024, 2048}
        assert any(AC.smooth7(n) and n % 2 for n in ns)
    assert len(AC.GRID_LENGTHS) >= 100


def test_grid_bounds_file_is_not_stale(emu):
    fig, rec = _grid_figures(*emu), AC.load_bounds()
    print(json.dumps(fig))
    assert rec['lengths'] == list(AC.GRID_LENGTHS)
    for prec in ('double', 'float'):
        for k in ('fwd', 'inv'):
            for meas in ('l2', 'max'):
                a, b = fig[prec][k][meas], rec[prec][k][meas]
                assert abs(a - b) <= 0.01 * b, (prec, k, meas, a, b)
    # two dimensions cost no more than the two line transforms they are made of
    assert rec['double']['fwd']['l2'] <= L2_DOUBLE and rec['double']['inv']['l2'] <= L2_DOUBLE
    assert max(rec['float'][k]['l2'] for k in ('fwd', 'inv')) <= 2 * L2_FLOAT


if __name__ == '__main__':
    import pathlib
    import tempfile
    if sys.argv[1:] != ['--write-bounds']:
        sys.exit('usage: python tests/test_anysize_host.py --write-bounds')
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        exe = _compile(tmp)
        res = _run_sweep(exe, tmp)
        for prec in ('double', 'float'):
            print('1-D worst, %s: relative L2 %.3e (n = %d, %s), per bin %.3e (n = %d, %s)'
                  % ((prec,) + _worst(res, prec, 0) + _worst(res, prec, 1)))
        fig = _grid_figures(exe, tmp)
    rec = {'what': 'worst errors of fft2 / ifft2 by the CPU emulation of the any-size FFT (tests/host/anysize_emulation.cpp) over the shapes '
                   '(H, pair(H)) of tests/anysize_common.py, H in lengths, against np.fft in complex128: l2 = relative L2 of a slice, '
                   'max = worst |error| of one bin / rms of the reference slice',
           'command': 'python tests/test_anysize_host.py --write-bounds',
           'lengths': list(AC.GRID_LENGTHS)}
    rec.update(fig)
    with open(AC.BOUNDS, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(fig, indent=1))
