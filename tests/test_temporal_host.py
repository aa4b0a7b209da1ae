"""CPU tests of temporal sparsity (pnp_set_temporal; include/pnp_mri.h, "temporal sparsity"): the NumPy oracle itself
(tests/temporal_oracle.py) -- its real-image form against the full complex spectrum, the prox identity --, the rules that need no device
through the real library and the solvers' ValueErrors before an engine is opened, the solve_sharded pre-check over gloo, the binding, and
the plan's item functions through g++ (tests/host/temporal_emulation.cpp, plain and with the sanitizer flags of test_host_cores.py)."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import temporal_oracle as TO

SRC = os.path.join(ROOT, 'tests', 'host', 'temporal_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
PLAIN = ['-O2', '-std=c++17', '-ffp-contract=off']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
L1 = dict(lambda1=0.5, reo=0.6)                                   # thr = 0.3
CNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)               # thr = 0.225, clip at 1 / b = 0.25: both sides of both populated
FRAMES = (2, 3, 5, 8, 16, 17, 64)


def _fields(B, n, cx=False, seed=0):
    rng = np.random.default_rng(seed + 131 * B + n)
    g = lambda s: s * rng.standard_normal((B, n)) + (1j * s * rng.standard_normal((B, n)) if cx else 0)
    return g(0.5), g(0.5), g(0.3)


# ---- the oracle against itself -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('keep_dc', [True, False])
@pytest.mark.parametrize('T', FRAMES)
def test_real_form_equals_the_full_spectrum(T, keep_dc):
    """k = 0 .. T / 2 with the doubled real parts == np.fft.fft along time (unitary), thresholded, inverted: 1e-13"""
    x, z, w = _fields(2 * T, 40)
    for kind, pr in (('l1', L1), ('cnc', CNC)):
        a, b = TO.prox(kind, x, z, w, pr, T, keep_dc), TO.prox_full_spectrum(kind, x, z, w, pr, T, keep_dc)
        assert a[0].dtype == np.float64 and np.abs(a[0] - b[0]).max() <= 1e-13 and np.abs(a[1] - b[1]).max() <= 1e-13, (kind, T)
        assert np.abs(a[0]).max() > 0.1


@pytest.mark.parametrize('cx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('keep_dc', [True, False])
@pytest.mark.parametrize('T', FRAMES)
def test_prox_identity(T, keep_dc, cx):
    """z+ minimises 1/2 ||z - u||^2 + thr sum_k |(F z)_k| over the penalised k: with Z = F z+, U = F u (np.fft, not the oracle's own sums)
    U_k - Z_k = thr Z_k / |Z_k| where Z_k != 0, |U_k| <= thr where Z_k = 0, and Z_0 = U_0 unpenalised; w+ = u - z+."""
    x, z, w = _fields(3 * T, 25, cx, seed=7)
    thr = L1['reo'] * L1['lambda1']
    zn, wn = TO.prox('l1', x, z, w, L1, T, keep_dc, cx=cx)
    u = x + w
    ser = lambda a: a.reshape(3, T, 25)
    U, Z = np.fft.fft(ser(u), axis=1, norm='ortho'), np.fft.fft(ser(zn), axis=1, norm='ortho')
    assert np.abs(wn - (u - zn)).max() <= 1e-15 and np.iscomplexobj(zn) == cx
    pen = np.ones(Z.shape, bool)
    if keep_dc:
        pen[:, 0] = False
        assert np.abs(Z[:, 0] - U[:, 0]).max() <= 1e-13
    zero = np.abs(Z) <= 1e-13
    assert (zero & pen).any() and (~zero & pen).any()
    assert (np.abs(U[zero & pen]) <= thr + 1e-13).all()
    nz = ~zero & pen
    assert np.abs(U[nz] - Z[nz] - thr * Z[nz] / np.abs(Z[nz])).max() <= 1e-12


def test_float_restatement_is_close_and_distinct():
    x, z, w = _fields(10, 30, seed=3)
    a, b = TO.prox('cnc', x, z, w, CNC, 5), TO.prox('cnc', x, z, w, CNC, 5, R=np.float32)
    assert b[0].dtype == np.float32 and 0 < TO.rel(b[0], a[0]) < 1e-5


def test_oracle_psnr_gap_on_the_dynamic_phantom():
    """the regulariser does what it is for, in the oracle: after the 50 iterations of DESIGN.md's table temporal ADMM_L1 ends at least 2.5 dB
    above pixel ADMM_L1, so that the GPU test's bound (this gap - 0.5 dB) stays above the 2 dB asked of the library"""
    img, masks, y = TO.dynamic_problem(16, 128, 128)
    pix, tmp = TO.loop(y, masks, 50, 'l1', TO.PRESETS['l1'])[0], TO.loop(y, masks, 50, 'l1', TO.PRESETS['l1'], 16)[0]
    assert TO.psnr(tmp, img) - TO.psnr(pix, img) >= 2.5


# ---- the library's rules without a device ----------------------------------------------------------------------------------------------

def test_temporal_check_codes_and_messages():
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    msg = lambda: L.pnp_last_error().decode()
    for f in (2, 3, 17, 64):
        assert L.pnp_temporal_check(f, 3 * f) == 0
    for f in (-1, 0, 1, 65, 1 << 20):
        assert L.pnp_temporal_check(f, 128) == -1 and msg() == 'temporal: frames must be 2..64 (got %d)' % f          # PNP_E_ARG
    for f, B in ((4, 6), (16, 17), (5, 0), (3, 1)):
        assert L.pnp_temporal_check(f, B) == -3                                                                       # PNP_E_STATE
        assert msg() == 'temporal: the batch of %d slices is not a whole number of series of %d frames' % (B, f)


def test_symbols_in_header_and_binding():
    from pnp_admm_cnc_mri_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read()
    assert 'temporal sparsity' in hdr and re.search(r'#define PNP_ABI_VERSION\s+13\b', hdr)
    for name, proto in (('pnp_temporal_check', 'int pnp_temporal_check(int frames, int B);'),
                        ('pnp_set_temporal', 'int pnp_set_temporal(pnp_ctx* ctx, int frames, int keep_dc);'),
                        ('pnp_get_temporal', 'int pnp_get_temporal(pnp_ctx* ctx, int* frames, int* keep_dc);')):
        assert proto in hdr and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)


def _refuse_engine(monkeypatch):
    import pnp_admm_cnc_mri_amd.solvers as S

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError('an engine was opened')
    monkeypatch.setattr(S, 'Engine', NoEngine)


@pytest.mark.parametrize('name', ['ADMM_L1', 'ADMM_CNC'])
def test_frames_value_errors_before_an_engine(name, monkeypatch):
    import pnp_admm_cnc_mri_amd as P
    _refuse_engine(monkeypatch)
    fn = getattr(P, name)
    m, y = np.ones((128, 128), np.uint8), np.zeros((6, 128, 128), np.complex64)
    with pytest.raises(ValueError, match=r'^temporal: the batch of 6 slices is not a whole number of series of 4 frames$'):
        fn(m, None, y=y, frames=4)
    for f in (1, 65, 0, -3):
        with pytest.raises(ValueError, match=r'^temporal: frames must be 2\.\.64 \(got %d\)$' % f):
            fn(m, None, y=y, frames=f)
    with pytest.raises(ValueError, match=r'^frames must be an integer \(got 2\.5\)$'):
        fn(m, None, y=y, frames=2.5)
    for kw in (dict(transform='haar'), dict(transform='db2', spin='random')):
        with pytest.raises(ValueError, match=r'^frames= \(temporal sparsity\) does not run with transform= / spin= '):
            fn(m, None, y=y, frames=3, **kw)
    with pytest.raises(AssertionError, match='an engine was opened'):          # a valid request reaches the engine ...
        fn(m, None, y=y, frames=3, temporal_keep_dc=False)
    with pytest.raises(AssertionError, match='an engine was opened'):          # ... and frames=None asks nothing
        fn(m, None, y=y, frames=None)


# ---- solve_sharded: no series is cut in two ------------------------------------------------------------------------------------------

def _solver(mask, noises, images=None, y=None, mask_id=None, return_device=False, **opts):
    import torch
    out = np.stack([np.asarray(y[n]).real.astype(np.float32) for n in range(len(y))])
    return torch.from_numpy(out) if return_device else list(out)


def _y(B):
    return np.arange(B * 8 * 6, dtype=np.float32).reshape(B, 8, 6).astype(np.complex64)


def test_sharded_precheck_single_process():
    import pnp_admm_cnc_mri_amd as P
    m = np.ones((8, 6), np.uint8)
    out = P.sharding.solve_sharded(_solver, m, None, y=_y(6), frames=3)
    assert out.shape == (6, 8, 6)
    with pytest.raises(ValueError, match=r'^solve_sharded: frames=4 does not divide the shards \[6\] of 6 slices over 1 ranks'):
        P.sharding.solve_sharded(_solver, m, None, y=_y(6), frames=4)
    with pytest.raises(ValueError, match=r'^temporal: frames must be 2\.\.64 \(got 65\)$'):
        P.sharding.solve_sharded(_solver, m, None, y=_y(6), frames=65)


def _worker(rank, world, port, cases, q):
    import torch.distributed as dist
    import pnp_admm_cnc_mri_amd as P
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        for B, frames in cases:
            try:
                x = P.sharding.solve_sharded(_solver, np.ones((8, 6), np.uint8), None, y=_y(B), frames=frames)
                q.put((rank, B, frames, 'ok', None if x is None else np.asarray(x)))
            except ValueError as e:
                q.put((rank, B, frames, 'ValueError', str(e)))
        dist.monitored_barrier()                      # gloo-only, CPU: dist.barrier() probes for an accelerator and opens the GPU
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world,cases', [(2, ((6, 2), (8, 4), (5, 5))), (3, ((4, 2), (8, 4), (18, 3), (2, 2)))])
def test_sharded_precheck_through_a_process_group(world, cases):
    """Every rank judges every shard before any work: all of them raise the same ValueError (nobody waits in the gather), and a batch
    whose shards are whole series runs as ever.  (2, 2) on three ranks: shards 1, 1, 0 -- an empty shard is no excuse for the others."""
    import torch.multiprocessing as mp
    import pnp_admm_cnc_mri_amd as P
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, cases, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world * len(cases))]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for B, frames in cases:
        mine = sorted((g for g in got if g[1] == B and g[2] == frames), key=lambda g: g[0])
        assert [g[0] for g in mine] == list(range(world))
        sizes = P.sharding.shard_sizes(B, world)
        if any(n % frames for n in sizes):
            assert all(g[3] == 'ValueError' for g in mine) and len({g[4] for g in mine}) == 1
            assert mine[0][4].startswith('solve_sharded: frames=%d does not divide the shards %s of %d slices over %d ranks' % (frames, sizes, B, world))
        else:
            assert all(g[3] == 'ok' for g in mine) and all(g[4] is None for g in mine[1:])
            assert np.array_equal(mine[0][4], _y(B).real)


# ---- host emulation --------------------------------------------------------------------------------------------------------------------

def plan_run(T, cx, real_bytes):
    """tp_run of temporal_plan.h, restated: the largest power of two in [16, 1024] whose run fits 40 KiB of LDS with both tiles, and 64
    pixels where they still fit 52 KiB"""
    pixel = 2 * T * (2 if cx else 1) * real_bytes + (T if cx else T // 2 + 1) * 2 * real_bytes
    p = 1024
    while p > 16 and p * pixel > 40 * 1024:
        p >>= 1
    return 64 if p < 64 and 64 * pixel <= 52 * 1024 else p


# (T, S, N, cx, kind, keep_dc): N = two full runs of the float plan (four of the double one) and a tail; N % 4 = 0, 1, 2; T prime, a power
# of two, 64; an even N on complex floats (8-byte values, 16-byte accesses)
EMU_CASES = ((5, 1, 2 * 512 + 37, False, 'l1', True), (8, 1, 2 * 256 + 6, False, 'cnc', True), (64, 2, 37, True, 'cnc', False),
             (64, 2, 2 * 64 + 8, False, 'cnc', True), (17, 1, 2 * 64 + 5, True, 'l1', True), (16, 2, 2 * 64 + 10, True, 'l1', False),
             (2, 1, 2 * 1024 + 4, False, 'l1', False), (3, 1, 2 * 1024 + 6, False, 'cnc', False))


def _write_case(path, T, S, N, cx, kind, keep_dc):
    x, z, w = _fields(S * T, N, cx, seed=T)
    pr = L1 if kind == 'l1' else CNC
    zn, wn = TO.prox(kind, x, z, w, pr, T, keep_dc, cx=cx)
    sc = [pr['reo'] * pr['lambda1'], 0, 0, 0, 0] if kind == 'l1' else [float(v) for v in TO.CO.cnc_scalars(**pr)]
    flat = lambda a: (np.ascontiguousarray(a, np.complex128).view(np.float64) if cx else np.asarray(a, np.float64)).ravel()
    np.concatenate([np.array([T, S, N, int(cx), int(kind == 'cnc'), int(keep_dc)] + sc, np.float64)] + [flat(a) for a in (x, z, w, zn, wn)]).tofile(path)


@pytest.mark.parametrize('flags', [PLAIN, SAN], ids=['plain', 'sanitized'])
def test_host_emulation(flags, tmp_path):
    """temporal_plan.h's item functions run by run as a stand-alone program (nothing is preloaded): arrays of exactly the plan's sizes, the
    LDS block poisoned with NaN before every run, every access width the plan may choose and the narrower ones, every pixel-frame written
    exactly once and nowhere else, the result equal to the oracle to 1e-12 in double (2e-5 in float)."""
    assert {N % 4 for _, _, N, _, _, _ in EMU_CASES} >= {0, 1, 2}
    for T, S, N, cx, kind, keep_dc in EMU_CASES:
        assert N > 2 * plan_run(T, cx, 4) and N % plan_run(T, cx, 4)                   # more than one run, and a tail
    exe = str(tmp_path / 'temporal_emulation')
    subprocess.check_call(['g++'] + flags + ['-o', exe, SRC])
    paths = []
    for i, c in enumerate(EMU_CASES):
        paths.append(str(tmp_path / ('case%d.bin' % i)))
        _write_case(paths[-1], *c)
    r = subprocess.run([exe] + paths, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stdout.decode()[-1500:], r.stderr.decode()[-1500:])
    out = r.stdout.decode()
    assert out.rstrip().endswith('ok') and '%d cases, 0 bad' % len(EMU_CASES) in out and 'DIFFER' not in out and 'COVERAGE' not in out
    for p, (T, S, N, cx, kind, keep_dc) in zip(paths, EMU_CASES):
        for prec, rb in (('double', 8), ('float', 4)):
            assert re.search(r'%s %s T=%d S=%d N=%d \S+ \S+ keep_dc=%d P=%d VP=1 \S+ err=\S+ ok' % (re.escape(p), prec, T, S, N, keep_dc, plan_run(T, cx, rb)), out)
    assert ' float T=2 ' in out and 'VP=4' in out and 'VP=2' in out and 'VP=1' in out
    widths = lambda prec, what: {int(v) for v in re.findall(r' %s T=\d+ S=\d+ N=\d+ %s \S+ keep_dc=\d P=\d+ VP=(\d)' % (prec, what), out)}
    assert widths('float', 'real') == {4, 2, 1} and widths('double', 'real') == {2, 1}
    assert widths('float', 'complex') == {2, 1} and widths('double', 'complex') == {1}
