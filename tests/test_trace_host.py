"""CPU tests of the convergence trace (pnp_admm_*_run_traced, pnp_residuals): the split plan of csrc/trace_plan.h and the slice-order
reduction of kernels_trace.hip through g++ (tests/host/trace_emulation.cpp, sanitizer flags of test_host_cores.py), and the binding."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'host', 'trace_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_trace') / 'trace_emulation')
    subprocess.check_call(['g++'] + SAN + ['-o', out, SRC])
    return out


def _run(args):
    r = subprocess.run(args, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    return r.stdout.decode()


def expected_checks(iters, every):
    """every multiple of `every` that is <= iters, plus iters if it is not one"""
    ks = list(range(every, iters + 1, every))
    if iters > 0 and (not ks or ks[-1] != iters):
        ks.append(iters)
    return ks


GRID = [(50, 10), (23, 10), (5, 10), (1, 1), (7, 1), (0, 3), (100, 7), (21, 7), (22, 7), (2, 1), (10, 10), (11, 10), (9, 10), (60, 5),
        (33, 1), (3, 2), (1, 5)]


@pytest.mark.parametrize('iters,every', GRID)
def test_split_plan(exe, iters, every):
    """The launches sum to iters; the checks fall exactly on the iterations the contract names; every check is preceded by a launch
    boundary at k - 1 (where z is copied) and ends a launch of one iteration."""
    lines = _run([exe, 'plan', str(iters), str(every)]).split('\n')
    want = expected_checks(iters, every)
    assert lines[0] == 'checks %d' % len(want)
    legs = [tuple(map(int, l.split()[1:])) for l in lines[1:] if l.startswith('leg')]
    assert len(legs) == len(want)
    at, boundaries, launched = 0, {0}, 0
    for (pre, k), k_want in zip(legs, want):
        assert pre >= 0 and k == k_want
        if pre:
            at += pre
            launched += pre
            boundaries.add(at)
        assert at == k - 1 and (k - 1) in boundaries          # the snapshot of z_{k-1} is taken at a launch boundary
        at += 1
        launched += 1
        boundaries.add(at)
        assert at == k
    assert launched == iters and at == iters


@pytest.mark.parametrize('B,pad', [(1, 1024), (3, 1024), (2, 0), (70, 1024)])
def test_slice_order_reduction_matches_natural_sums(exe, tmp_path, B, pad):
    """The slice-order flavour walked as the kernel addresses it (tiles of four row pairs, x through the tile buffer by the index map, z by
    16-byte access, padded stride) gives the natural-order NumPy sums to 1e-15 relative, with the padding poisoned: no NaN reaches a sum."""
    rng = np.random.default_rng(5 + B)
    N = 65536
    x, z, zp, w = (rng.uniform(-1, 1, (B, N)).astype(np.float32) for _ in range(4))
    gt = rng.integers(0, 256, (B, N), dtype=np.uint8)
    inp, out = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(inp, 'wb') as f:
        f.write(struct.pack('<ii', B, pad))
        for a in (x, z, zp, w, gt):
            f.write(a.tobytes())
    _run([exe, 'slice', inp, out])
    got = np.fromfile(out, np.float64).reshape(7, B)
    x64, z64, zp64, w64, g64 = (a.astype(np.float64) for a in (x, z, zp, w, gt))
    want = np.stack([((x64 - z64) ** 2).sum(1), ((z64 - zp64) ** 2).sum(1), (x64 ** 2).sum(1), (z64 ** 2).sum(1), (w64 ** 2).sum(1),
                     ((x64 * 255.0 - g64) ** 2).sum(1), (g64 ** 2).sum(1)])
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= 1e-15 * want).all(), np.abs(got / want - 1).max()


def test_binding_declares_the_trace_calls():
    from pnp_admm_cnc_mri_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read(), flags=re.S)
    new = ('pnp_admm_l1_run_traced', 'pnp_admm_cnc_run_traced', 'pnp_trace_read', 'pnp_residuals', 'pnp_residuals_f64')
    for name in new:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.lib().pnp_abi_version()
    for q, name in enumerate(('R_PRI', 'R_DUAL', 'X_NORM', 'Z_NORM', 'W_NORM', 'PSNR', 'RE')):
        assert int(re.search(r'#define PNP_TRACE_%s\s+(\d+)' % name, src).group(1)) == q
    from pnp_admm_cnc_mri_amd.engine import TRACE_FIELDS
    assert len(TRACE_FIELDS) == int(re.search(r'#define PNP_TRACE_Q\s+(\d+)', src).group(1))


def test_trace_arguments_are_checked_before_any_device_work():
    """every < 1 and a trace without return_info are refused on the host: no context, no kernel."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    from pnp_admm_cnc_mri_amd.solvers import trace_request
    mask = np.ones((256, 256), np.uint8)
    img = np.zeros((1, 256, 256), np.uint8)
    for solver in (P.ADMM_L1, P.ADMM_CNC):
        with pytest.raises(ValueError, match='return_info'):
            solver(mask, np.zeros((256, 256), np.complex128), images=img, trace_every=5)
        with pytest.raises(ValueError, match='return_info'):
            solver(mask, np.zeros((256, 256), np.complex128), images=img, tol=1e-3)
    with pytest.raises(ValueError, match='trace_every'):
        trace_request(-1, None, True)
    with pytest.raises(ValueError, match='tol'):
        trace_request(0, 0.0, True)
    assert trace_request(0, None, False) is False and trace_request(0, 1e-3, True) and trace_request(7, None, True)
    L = _lib.lib()
    assert L.pnp_admm_l1_run_traced(None, 5, 0.1, 0.015, 1, 0.0, None, 0, None, None) == -1          # PNP_E_ARG: null ctx
    assert L.pnp_residuals(None, None, None, None, None, None, 0, 0, None, 0) == -1
