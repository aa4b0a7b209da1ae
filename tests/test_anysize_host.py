"""CPU tests of the any-size FFT's host plan and butterfly arithmetic (csrc/anysize_plan.h, the header kernels_anysize.hip
includes): compiled with g++, checked against np.fft.  Pins the factorisation, the Bluestein length, the fp64 twiddle, chirp
and kernel tables, and one forward and one inverse line transform per length, before anything runs on a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'host', 'anysize_emulation.cpp')
SIZES = (128, 170, 192, 218, 320, 368, 384, 640, 1000, 1021, 1024)


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp('anysize')
    exe = str(d / 'anysize_emulation')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-o', exe, SRC])
    return exe, d


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


@pytest.mark.parametrize('n', SIZES)
def test_plan_tables_and_transform(emu, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    r = _run(emu, n, x)
    assert r['n'] == n
    # plan: a Stockham length, factorised into the supported radices
    assert r['bluestein'] == (0 if _smooth7(n) else 1)
    if r['bluestein']:
        m = r['m']
        assert m & (m - 1) == 0 and m >= 2 * n - 1 and m // 2 < 2 * n - 1 and m <= 2048
    else:
        assert r['m'] == n
    assert all(q in (2, 3, 4, 5, 7) for q in r['radix']) and int(np.prod(r['radix'])) == r['m']
    # tables in fp64
    m = r['m']
    assert np.max(np.abs(r['tw'] - np.exp(-2j * np.pi * np.arange(m) / m))) <= 1e-15
    if r['bluestein']:
        j = np.arange(n)
        assert np.max(np.abs(r['chirp'] - np.exp(-1j * np.pi * (j * j % (2 * n)) / n))) <= 1e-15
        b = np.zeros(m, np.complex128)
        b[:n] = np.conj(r['chirp'])
        b[m - n + 1:] = np.conj(r['chirp'][1:])[::-1]
        kern = np.fft.fft(b) / m
        assert np.max(np.abs(r['kern'] - kern)) <= 1e-12 * np.max(np.abs(kern))
    # one line transform, forward (np.fft.fft) and unnormalised inverse (n * np.fft.ifft)
    ref_f, ref_i = np.fft.fft(x), np.fft.ifft(x) * n
    assert np.linalg.norm(r['fwd'] - ref_f) / np.linalg.norm(ref_f) <= 1e-12
    assert np.linalg.norm(r['inv'] - ref_i) / np.linalg.norm(ref_i) <= 1e-12
