"""CPU tests of the wavelet-domain sparsity (pnp_set_sparsity, pnp_dwt2_*): the filter constants and index maps of csrc/wavelet_plan.h
through g++ (tests/host/wavelet_emulation.cpp, sanitizer flags of test_host_cores.py), the NumPy oracle itself (tests/wavelet_oracle.py),
the argument checks through the real library, and the binding."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rel_l2
import wavelet_oracle as O

SRC = os.path.join(ROOT, 'tests', 'host', 'wavelet_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
CODE = {'haar': 1, 'db2': 2, 'db4': 3}
TAPS = {'haar': 2, 'db2': 4, 'db4': 8}
SHAPES = [(128, 128), (128, 160), (256, 192), (256, 256), (512, 512)]          # the shapes of tests/test_gpu_wavelet.py
# the partial-tile sizes of tests/test_gpu_wavelet_edges.py and their transposes: every valid L runs, the table's own L is the largest
EDGE_SHAPES = [hw for _, H, W in O.EDGE_CASES for hw in ((H, W), (W, H))]
EDGE_PROX = [(name, L, H, W) for L, H, W in O.EDGE_CASES for name in O.NAMES]


def valid(name, L, H, W):
    return 1 <= L <= 4 and H % (1 << L) == 0 and W % (1 << L) == 0 and (min(H, W) >> (L - 1)) >= TAPS[name]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_wavelet') / 'wavelet_emulation')
    subprocess.check_call(['g++'] + SAN + ['-o', out, SRC])
    return out


def _run(args):
    r = subprocess.run(args, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    return r.stdout.decode()


# ---- filters -------------------------------------------------------------------------------------------------------------------

def plan_filters(exe):
    vals = [float(v) for v in [l for l in _run([exe, 'plan']).split('\n') if l.startswith('filters')][0].split()[1:]]
    return {'haar': np.array(vals[:2]), 'db2': np.array(vals[2:6]), 'db4': np.array(vals[6:14])}


@pytest.mark.parametrize('name', O.NAMES)
def test_filter_constants(exe, name):
    """The committed constants: sum h = sqrt 2, orthonormal under even shifts to 1e-15, p = T / 2 vanishing moments of g to 1e-12, and equal
    to the oracle's own derivation (closed forms; db4 from the roots of P(y), in extended precision) to one unit in the last place."""
    h = plan_filters(exe)[name]
    T = len(h)
    assert T == TAPS[name]
    g = np.array([(-1) ** n * h[T - 1 - n] for n in range(T)])
    assert abs(h.sum() - np.sqrt(2.0)) <= 1e-15
    for m in range(T // 2):
        assert abs(float(np.dot(h[:T - 2 * m], h[2 * m:])) - (1.0 if m == 0 else 0.0)) <= 1e-15, m
    for j in range(T // 2):
        assert abs(float(np.sum(np.arange(T, dtype=np.float64) ** j * g))) <= 1e-12, j
    ho, go = O.filters(name)
    assert np.abs(h - ho).max() <= 2.3e-16 and np.abs(g - go).max() <= 2.3e-16
    if name == 'db4':
        assert np.allclose(h[:4], [0.2303778133, 0.7148465706, 0.6308807679, -0.0279837694], rtol=0, atol=1e-10)


@pytest.mark.parametrize('name', O.NAMES)
def test_oracle_reconstructs_and_preserves_energy(name):
    """The oracle itself: Psi^T Psi = I and ||Psi v|| = ||v|| to 1e-12, every level count, a non-square shape."""
    rng = np.random.default_rng(11)
    v = rng.standard_normal((2, 128, 160))
    for L in range(1, 5):
        if not valid(name, L, 128, 160):
            continue
        c = O.fwd(v, name, L)
        assert rel_l2(O.inv(c, name, L), v) <= 1e-12
        assert abs(float((c ** 2).sum() / (v ** 2).sum()) - 1.0) <= 1e-12
        # the LL band of a constant image carries all of it (sum h = sqrt 2 per level and axis)
        cc = O.fwd(np.ones((16 << 3, 16 << 3)), name, L)
        assert np.abs(cc[O.detail_mask(128, 128, L)]).max() <= 1e-12


# ---- the plan's tiling against the whole-image oracle --------------------------------------------------------------------------

def emulate(exe, tmp_path, name, L, mode, arrays, params=(0, 0, 0, 0, 0), f64=True):
    dt = np.float64 if f64 else np.float32
    B, H, W = arrays[0].shape
    inp, out = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(inp, 'wb') as f:
        f.write(struct.pack('<7i', CODE[name], L, H, W, B, mode, 1 if f64 else 0))
        f.write(struct.pack('<5d', *params))
        for a in arrays:
            f.write(np.ascontiguousarray(a, dt).tobytes())
    _run([exe, 'run', inp, out])
    got = np.fromfile(out, dt)
    return got.reshape(-1, B, H, W)


def test_plan_fits_the_lds(exe):
    """Every (filter, levels, precision): a tile that is a multiple of 2^L and both kernels' LDS within one compute unit's 160 KiB."""
    rows = [tuple(map(int, l.split())) for l in _run([exe, 'plan']).split('\n') if l and not l.startswith('filters')]
    assert len(rows) == 3 * 4 * 2
    for wv, L, _bytes, tile, halo, lds_fwd, lds_inv in rows:
        assert tile % (1 << L) == 0 and tile in (32, 64)
        assert halo == ({1: 2, 2: 4, 3: 8}[wv] - 2) * ((1 << L) - 1)
        assert 0 < lds_fwd <= 160 * 1024 and 0 < lds_inv <= 160 * 1024, (wv, L, lds_fwd, lds_inv)


@pytest.mark.parametrize('H,W', SHAPES + EDGE_SHAPES)
@pytest.mark.parametrize('name', O.NAMES)
def test_tiled_transform_matches_oracle(exe, tmp_path, name, H, W):
    """Analysis and synthesis tile by tile through wavelet_plan.h's item functions reproduce the whole-image oracle (double: 1e-12; any
    indexing error is O(1)), for every valid level count: L = 1..4, at 512 x 512 L = 1 as on the GPU."""
    rng = np.random.default_rng(H * 7 + W)
    B = 1 if H == 512 else 2
    v = rng.standard_normal((B, H, W))
    for L in ((1,) if H == 512 else range(1, 5)):
        if not valid(name, L, H, W):
            continue
        want = O.fwd(v, name, L)
        got = emulate(exe, tmp_path, name, L, 0, [v])[0]
        assert np.isfinite(got).all()
        assert rel_l2(got, want) <= 1e-12, (L, rel_l2(got, want))
        back = emulate(exe, tmp_path, name, L, 1, [want])[0]
        assert np.isfinite(back).all()
        assert rel_l2(back, v) <= 1e-12, (L, rel_l2(back, v))


@pytest.mark.parametrize('name,L,H,W', [('db4', 4, 128, 128), ('db2', 3, 128, 160), ('haar', 2, 256, 192), ('db4', 2, 144, 176)] + EDGE_PROX)
@pytest.mark.parametrize('f64', [True, False])
def test_tiled_prox_matches_oracle(exe, tmp_path, name, L, H, W, f64):
    """Both prox steps tile by tile (CNC: z first, then x + w through the same arrays) against the oracle; 144 x 176 is no multiple of the
    tile (partial tiles).  float32: against the float64 oracle at a few float32 roundings per term of the 2 L T-term chains."""
    rng = np.random.default_rng(3)
    x, z, w = (rng.uniform(-1, 1, (2, H, W)) * s for s in (1.0, 1.0, 0.3))
    if not f64:
        x, z, w = (a.astype(np.float32).astype(np.float64) for a in (x, z, w))
    bar = 1e-12 if f64 else 2.0 ** -23 * 2 * L * TAPS[name]
    thr = 0.4
    zl, wl = O.prox_l1(x, z, w, thr, name, L)
    got = emulate(exe, tmp_path, name, L, 2, [x, z, w], (thr, 0, 0, 0, 0), f64)
    assert np.isfinite(got).all()
    assert rel_l2(got[0], zl) <= bar and rel_l2(got[1], wl) <= bar, (rel_l2(got[0], zl), rel_l2(got[1], wl))
    alpha, lam, reo, b = 0.45, 0.5, 1.0, 4.0
    zc, wc = O.prox_cnc(x, z, w, alpha, lam, reo, b, name, L)
    p = (alpha * reo * lam, 1 - alpha, alpha, alpha * reo * lam * b, 1 / b)
    got = emulate(exe, tmp_path, name, L, 3, [x, z, w], p, f64)
    assert np.isfinite(got).all()
    assert rel_l2(got[0], zc) <= bar and rel_l2(got[1], wc) <= bar, (rel_l2(got[0], zc), rel_l2(got[1], wc))


# ---- the per-element bars of tests/test_gpu_wavelet_edges.py ------------------------------------------------------------------------

@pytest.mark.parametrize('name,L,H,W', EDGE_PROX)
def test_the_edge_bars_see_one_pixel_of_the_thinnest_tile(name, L, H, W):
    """What the per-element bars are for, shown on the oracle itself on the inputs of the GPU prox test: one pixel of the bottom-right tile
    -- partial on both axes, on one of them 2^L pixels thin or one 2^L short -- moved by 1e-5 of the array's scale is beyond the float bar
    (4 x the float32 restatement's distance, floor 2e-6, never above 5e-6) and is reported as the worst element, in a partial tile; the
    whole-image rel-L2 of the sibling GPU files, at 4 x the restatement's rel-L2, lets the same array pass."""
    x, z, w = O.edge_prox_inputs(H, W)
    assert len(x) == O.EDGE_B and (O.FREEDOM, O.FLOOR, O.F64_BAR, O.F32_CAP) == (4.0, 2e-6, 1e-12, 5e-6)
    t = O.tile(name, L)
    ty, tx = O.last_tile_origin(H, W, name, L)
    part = O.partial_tile_mask(H, W, name, L)
    assert 0 < H - ty < t and 0 < W - tx < t                                                   # both axes partial
    if t == 32 or (L, H, W) == O.EDGE_TILE64:
        assert (H + t - 1) // t != (W + t - 1) // t                                            # tiles_x != tiles_y
    assert sorted((H - ty, W - tx)) == sorted((1 << L, t - (1 << L)))          # one deepest-level coefficient; one short of a full tile
    assert part[ty:, :].all() and part[:, tx:].all() and not part[:ty, :tx].any()
    assert part.sum() == O.partial_tile_mask(H, W, name, L, coef=True).sum()                    # as many coefficients as pixels
    assert np.array_equal(O.partial_tile_mask(H, W, name, L, shifts=((3, 1),)), np.roll(part, (3, 1), (0, 1)))
    p = O.PROX_CNC
    for kind, r64, r32 in (('l1', O.prox_l1(x, z, w, O.PROX_L1_THR, name, L), O.prox_l1(x, z, w, O.PROX_L1_THR, name, L, np.float32)),
                           ('cnc', O.prox_cnc(x, z, w, name=name, levels=L, **p), O.prox_cnc(x, z, w, name=name, levels=L, dtype=np.float32, **p))):
        for k in (0, 1):
            bar = O.float_bar(r32[k], r64[k])                                                   # asserts bar <= F32_CAP
            assert (bar >= O.FLOOR).all() and O.worst(r32[k], r64[k], bar, part)['ratio'] <= 1.0 / O.FREEDOM
            wrong = r64[k].copy()
            wrong[1, ty, tx] += 1e-5 * np.abs(r64[k][1]).max()
            r = O.worst(wrong, r64[k], bar, part)
            assert r['ratio'] >= 2.0 and r['pos'] == (1, ty, tx) and r['partial'] and r['outside'] == 0.0, (kind, k, r)
            assert not (O.distance(wrong, r64[k]) <= bar).all()
            assert rel_l2(wrong, r64[k]) <= 4 * rel_l2(r32[k], r64[k]), (kind, k)               # the whole-image bar does not see it


@pytest.mark.parametrize('H,W,name,L', [(136, 184, 'db4', 3), (144, 176, 'db2', 4)])
def test_the_edge_points_leave_the_branches_they_name_empty(H, W, name, L):
    """wavelet_oracle.edge_points on the inputs of the GPU test: alpha in {0, 1}, b in {0.5, 1e4}, lambda1 = 0 and an L1 threshold of 0 are
    all there, every branch a point names holds < 0.1 % of the detail coefficients, every other one >= 2 %, and no float bar of z+ or
    w+ exceeds 5e-6 (w+ at threshold 0 is ~ 0 and judged against max |x + w|)."""
    x, z, w = O.edge_prox_inputs(H, W)
    pts = O.edge_points()
    cnc = [p for kind, p, _ in pts if kind == 'cnc']
    assert {0.0, 1.0} <= {p[0] for p in cnc} and {0.5, 1e4} <= {p[3] for p in cnc} and 0.0 in {p[1] for p in cnc}
    assert [p[0] * p[1] for kind, p, _ in pts if kind == 'l1'] == [0.0]
    for kind, params, off in pts:
        share = O.check_branches(kind, params, off, x, z, w, name, L)
        assert abs(share['zero'] + share['pass'] - 1.0) <= 1e-12
        if kind == 'l1':
            r64, r32 = (O.prox_l1(x, z, w, params[0] * params[1], name, L, dt) for dt in (np.float64, np.float32))
            scale = np.abs(x.astype(np.float64) + w).reshape(len(x), -1).max(axis=1)
            assert np.abs(r64[1]).max() <= 1e-13 * scale.max()
        else:
            r64, r32 = (O.prox_cnc(x, z, w, *params, name, L, dt) for dt in (np.float64, np.float32))
            scale = None
        assert (O.float_bar(r32[0], r64[0]) <= O.F32_CAP).all() and (O.float_bar(r32[1], r64[1], scale) <= O.F32_CAP).all()


# ---- arguments and binding ------------------------------------------------------------------------------------------------------

BAD = [('haar', 0, 256, 256, 'levels'), ('haar', 5, 256, 256, 'levels'), ('db2', 2, 130, 128, 'divisible'),
       ('db4', 4, 16, 16, 'shorter'), ('db4', 3, 128, 24, 'shorter')]


def test_sparsity_arguments_are_checked_before_any_device_work(exe):
    """L = 0, L = 5, 130 x 128 with L = 2 and a level input shorter than the filter are PNP_E_ARG from the real library without a context or
    a device; the solvers raise ValueError for them and for an unknown name before an engine is opened."""
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    from pnp_admm_cnc_mri_amd.engine import check_sparsity
    L = _lib.lib()
    for name, lv, H, W, word in BAD:
        assert L.pnp_sparsity_check(CODE[name], lv, H, W) == -1, (name, lv, H, W)          # PNP_E_ARG
        assert word in L.pnp_last_error().decode()
        assert int(_run([exe, 'check', str(CODE[name]), str(lv), str(H), str(W)])) != 0
        with pytest.raises(ValueError, match=word):
            check_sparsity(name, lv, H, W)
    assert L.pnp_sparsity_check(7, 3, 256, 256) == -1
    assert L.pnp_sparsity_check(0, 99, 130, 7) == 0                                        # NONE: levels ignored
    for name in O.NAMES:
        for lv in range(1, 5):
            for H, W in SHAPES:
                assert (L.pnp_sparsity_check(CODE[name], lv, H, W) == 0) == valid(name, lv, H, W)
    assert L.pnp_set_sparsity(None, 1, 3) == -1 and L.pnp_get_sparsity(None, None, None) == -1          # null ctx
    assert L.pnp_dwt2_fwd(None, None, None, 1) == -1 and L.pnp_dwt2_inv_f64(None, None, None, 1) == -1
    mask = np.ones((130, 128), np.uint8)
    img = np.zeros((1, 130, 128), np.uint8)
    for solver in (P.ADMM_L1, P.ADMM_CNC):
        with pytest.raises(ValueError, match='divisible'):
            solver(mask, np.zeros((130, 128), np.complex128), images=img, transform='db2', levels=2)
        with pytest.raises(ValueError, match='levels'):
            solver(mask, np.zeros((130, 128), np.complex128), images=img, transform='haar', levels=0)
        with pytest.raises(ValueError, match='transform'):
            solver(mask, np.zeros((130, 128), np.complex128), images=img, transform='sym8')


def test_binding_declares_the_wavelet_calls():
    from pnp_admm_cnc_mri_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pnp_mri.h')).read(), flags=re.S)
    new = ('pnp_sparsity_check', 'pnp_set_sparsity', 'pnp_get_sparsity', 'pnp_dwt2_fwd', 'pnp_dwt2_inv', 'pnp_dwt2_fwd_f64', 'pnp_dwt2_inv_f64')
    for name in new:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.ABI_VERSION == 13 == int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == _lib.lib().pnp_abi_version()
    from pnp_admm_cnc_mri_amd.engine import WAVELETS
    for name, code in (('NONE', None), ('HAAR', 'haar'), ('DB2', 'db2'), ('DB4', 'db4')):
        assert int(re.search(r'#define PNP_WAVELET_%s\s+(\d+)' % name, src).group(1)) == WAVELETS[code]
    import inspect
    import pnp_admm_cnc_mri_amd as P
    for solver in (P.ADMM_L1, P.ADMM_CNC):
        sig = inspect.signature(solver)
        assert sig.parameters['transform'].default is None and sig.parameters['levels'].default == 3
