"""The wavelet-domain prox (kernels_wavelet.hip, wavelet_kernels.h, wavelet_plan.h and the complex twins in kernels_complex.hip) per element
at sizes the tile does not divide.

tests/test_gpu_wavelet.py and tests/test_gpu_wavelet_spin.py run lengths that are multiples of 32 and judge by whole-image rel-L2.  Here
every case has a partial tile on both axes (wavelet_oracle.EDGE_SIZES, one size per level count: one axis ends in a tile that holds a
single coefficient of the deepest level, the other in a tile one such coefficient short of full; tiles_x != tiles_y at tile 32, and at
tile 64 through the added 136 x 248, since 2 . 64 + 2^L and 3 . 64 - 2^L are three tiles each), B = 2 slices on contexts of Bmax = 3,
and every output is compared per element and per slice with the float64 NumPy oracles (tests/wavelet_oracle.py,
tests/wavelet_spin_oracle.py, tests/complex_oracle.py):

    max |got - ref| <= bar x max |ref|
    double   bar = 1e-12
    float    bar = max(4 x the same distance of the oracle's float32 restatement from its float64 form, 2e-6), formed on the CPU inside the
             test on the same case and never from a kernel; no float bar of a single step may exceed 5e-6 (wavelet_oracle.float_bar asserts it)

Where the expected output itself is ~ 0 (w+ at a threshold of 0) max |x + w| stands in for max |ref|.

Guards: every device array handed to a step-wise call is the middle B slices of a [B + 2, H, W] array filled with a finite sentinel; after
the call both outer slices, and every input the call does not write, must be bit-unchanged.

Every comparison prints a line `EDGE ...` with what the card gave beside its bar, the position of the worst element, whether that element
lies in a partial tile, and the worst ratio to the bar over the partial tiles and over the full ones (pytest -s)."""
import functools

import numpy as np
import pytest

import complex_oracle as X
import multicoil_oracle as M
import wavelet_oracle as O
import wavelet_spin_oracle as S

pytestmark = pytest.mark.gpu

B, BMAX = O.EDGE_B, 3
F32 = np.float32
SENTINEL = -7.25
SENTINEL_CX = complex(-7.25, 3.5)
SIZES = O.EDGE_CASES                                                                     # (L, H, W): the four sizes, and 136 x 248 (3 x 4 tiles of 64)
SIZES_T = SIZES + tuple((L, W, H) for L, H, W in SIZES)                                  # and the transposes
SPIN_L = (3, 4)
CX_CASES = ((136, 184, 'haar', 3, ('f32', 'f64')), (136, 184, 'db4', 3, ('f32', 'f64')), (144, 176, 'db2', 4, ('f32', 'f64')),
            (144, 176, 'db4', 4, ('f32',)))               # db4, L = 4 on complex doubles is refused for LDS (tests/test_gpu_complex.py)
POINT_CASES = ((136, 184, 'db4', 3), (144, 176, 'db2', 4))
L1_STEP = (O.PROX_L1_THR, 1.0)                            # (lambda1, reo) of a loop call whose threshold is PROX_L1_THR


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


@pytest.fixture(scope='module')
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- guards and judgement ---------------------------------------------------------------------------------------------------------------

def _guarded(torch, a=None, dtype=None, shape=None):
    """-> (full [B + 2, H, W] of the sentinel on the device, its middle B slices holding `a`, or the sentinel too when a is None)"""
    dt = np.dtype(dtype if a is None else np.asarray(a).dtype)
    shape = tuple(shape if a is None else np.shape(a))
    assert shape[0] == B
    full = np.full((B + 2,) + shape[1:], SENTINEL_CX if dt.kind == 'c' else SENTINEL, dt)
    if a is not None:
        full[1:-1] = a
    full = torch.from_numpy(full).to(torch.device('cuda', 0))
    mid = full[1:-1]
    assert mid.is_contiguous() and mid.data_ptr() == full.data_ptr() + full[0].numel() * full.element_size()
    return full, mid


def _intact(torch, *fulls):
    """both outer slices of every guarded array still hold the sentinel, bit for bit"""
    for full in fulls:
        s = SENTINEL_CX if full.is_complex() else SENTINEL
        want = torch.full_like(full[0], s)
        assert torch.equal(full[0], want) and torch.equal(full[-1], want), 'a write outside the B slices'


def _judge(label, got, ref, bar, part, bad, scale=None):
    """one comparison: prints its EDGE line, appends to `bad` when the worst element is beyond the bar"""
    r = O.worst(got, ref, bar, part, scale)
    d = O.distance(got, ref, scale)
    s = r['pos'][0]
    print('EDGE %-64s card %.2e bar %.2e ratio %.3g at %s %s | partial tiles %.3g full tiles %.3g' % (
        label, d[s], np.broadcast_to(bar, d.shape)[s], r['ratio'], r['pos'], 'PARTIAL' if r['partial'] else 'full', r['inside'], r['outside']))
    if not r['ratio'] <= 1.0:
        bad.append('%s: %.3g x its bar at %s (%s tile)' % (label, r['ratio'], r['pos'], 'partial' if r['partial'] else 'full'))
    return r


def _bars(f64, r32, r64, scale=None):
    return np.full(B, O.F64_BAR) if f64 else O.float_bar(r32, r64, scale)


# ---- 1. Psi and Psi^T -------------------------------------------------------------------------------------------------------------------

def _shifts(L):
    m = (1 << L) - 1
    return ((0, 0), (1, 0), (0, m), (m, m))


@functools.lru_cache(maxsize=None)
def _transform_reference(H, W, name, L):
    """-> v, {shift: (Psi_s v, its float32 restatement, the float32-valued coefficients Psi_s^T is fed, Psi_s^T of them, its restatement)}"""
    v = O.field(H, W)
    assert len(v) == B
    out = {}
    for s in _shifts(L):
        c64 = S.fwd(v, name, L, s)
        c_in = c64.astype(F32)                                            # the oracle's coefficients, not the card's; the same for both precisions
        out[s] = (c64, S.fwd(v, name, L, s, F32), c_in, S.inv(c_in, name, L, s), S.inv(c_in, name, L, s, F32))
    return v, out


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('L,H,W', SIZES_T)
def test_transform_per_element(P, torch, L, H, W, name, precision):
    """dwt2 / idwt2 and their shifted forms at (0, 0), (1, 0), (0, 2^L - 1), (2^L - 1, 2^L - 1) against the (rolled) oracle per element;
    Psi^T on the oracle's coefficients; in place bit-equal to out of place; the unshifted entry point bit-equal to shift (0, 0)."""
    assert O.valid(name, L, H, W)
    f64 = precision == 'f64'
    real = np.float64 if f64 else F32
    v, refs = _transform_reference(H, W, name, L)
    bad = []
    with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
        eng.set_sparsity(name, L)
        plain = {}
        for s in (None,) + _shifts(L):
            c64, c32, c_in, b64, b32 = refs[s or (0, 0)]
            for inverse, src, r64, r32 in ((0, v, c64, c32), (1, c_in, b64, b32)):
                call = eng.idwt2 if inverse else eng.dwt2
                src = src.astype(real)
                in_full, inp = _guarded(torch, src)
                out_full, out = _guarded(torch, dtype=real, shape=src.shape)
                call(inp, out, B, s)
                eng.sync()
                _intact(torch, in_full, out_full)
                assert np.array_equal(inp.cpu().numpy(), src), 'the input of an out-of-place transform changed'
                got = out.cpu().numpy()
                part = O.partial_tile_mask(H, W, name, L, coef=not inverse, shifts=(s or (0, 0),))
                _judge('%s %s L=%d %dx%d %s shift %s' % ('idwt2' if inverse else 'dwt2', name, L, H, W, precision, s), got, r64,
                       _bars(f64, r32, r64), part, bad)
                t_full, t = _guarded(torch, src)
                call(t, t, B, s)
                eng.sync()
                _intact(torch, t_full)
                assert torch.equal(t, out), ('in place differs from out of place', inverse, s)
                if s is None:
                    plain[inverse] = got
                elif s == (0, 0):
                    assert np.array_equal(got, plain[inverse]), ('shift (0, 0) differs from the unshifted call', inverse)
                else:
                    assert not np.array_equal(got, plain[inverse]), (inverse, s)
    assert not bad, '\n'.join(bad)


# ---- 2. one prox step, real, float ------------------------------------------------------------------------------------------------------

def _thr_of(kind, params):
    return params[1] * params[0] if kind == 'l1' else None


def _oracle_prox(kind, params, x, z, w, name, L, dtype=np.float64):
    if kind == 'l1':
        return O.prox_l1(x, z, w, _thr_of(kind, params), name, L, dtype)
    return O.prox_cnc(x, z, w, *params, name, L, dtype)


@functools.lru_cache(maxsize=None)
def _prox_reference(kind, params, off, H, W, name, L):
    """-> ((z+, w+) of the float64 oracle, of its float32 restatement, the scale of w+ or None); the branch structure is asserted here"""
    x, z, w = O.edge_prox_inputs(H, W)
    O.check_branches(kind, params, off, x, z, w, name, L)
    r64, r32 = _oracle_prox(kind, params, x, z, w, name, L), _oracle_prox(kind, params, x, z, w, name, L, F32)
    w_scale = None
    if kind == 'l1' and _thr_of(kind, params) == 0:                    # w+ = u - Psi^T Psi u ~ 0: judged against max |x + w|
        w_scale = np.abs(x.astype(np.float64) + w).reshape(B, -1).max(axis=1)
    return r64, r32, w_scale


def _card_prox(eng, kind, params, xt, zt, wt):
    if kind == 'l1':
        eng.prox_l1_dual(xt, zt, wt, _thr_of(kind, params))
    else:
        eng.prox_cnc_dual(xt, zt, wt, *params)
    eng.sync()


def _dummy_problem(eng):
    eng.upload(np.zeros((B, eng.H, eng.W), np.complex64), np.ones((eng.H, eng.W), np.uint8))


def _float_step(torch, eng, kind, params, off, H, W, name, L, bad, what='prox'):
    """one guarded step-wise prox of a float engine with (name, L) set, judged per element"""
    x, z, w = O.edge_prox_inputs(H, W)
    r64, r32, w_scale = _prox_reference(kind, params, off, H, W, name, L)
    (xf, xt), (zf, zt), (wf, wt) = (_guarded(torch, a) for a in (x, z, w))
    _card_prox(eng, kind, params, xt, zt, wt)
    _intact(torch, xf, zf, wf)
    assert np.array_equal(xt.cpu().numpy(), x), 'x changed'
    part = O.partial_tile_mask(H, W, name, L)
    for arr, t, k, scale in (('z+', zt, 0, None), ('w+', wt, 1, w_scale)):
        _judge('%s %s %r %s L=%d %dx%d f32 %s' % (what, kind, params, name, L, H, W, arr), t.cpu().numpy(), r64[k],
               _bars(False, r32[k], r64[k], scale), part, bad, scale)


STD = {'l1': (L1_STEP, ()), 'cnc': (tuple(O.PROX_CNC[k] for k in ('alpha', 'lambda1', 'reo', 'b')), ())}      # both branches of soft and clip


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('L,H,W', SIZES)
def test_prox_step_per_element(P, torch, L, H, W, name, kind):
    """prox_l1_dual / prox_cnc_dual at wavelet_oracle.PROX_L1_THR / PROX_CNC on inputs built like prox_inputs, every branch of soft and of
    clip populated (asserted on the CPU): z+ and w+ per element, x and the guards untouched."""
    bad = []
    with P.Engine(H, W, Bmax=BMAX) as eng:
        _dummy_problem(eng)
        eng.set_sparsity(name, L)
        _float_step(torch, eng, kind, *STD[kind], H, W, name, L, bad)
    assert not bad, '\n'.join(bad)


# ---- 3. cycle spinning on partial tiles ---------------------------------------------------------------------------------------------------

def _spin_groups(L):
    m = (1 << L) - 1
    return [(m, 1)], [(1, m), (m, 0), (3, 5)]                             # one shift; K = 3: store, add, average-dual


@functools.lru_cache(maxsize=None)
def _spin_reference(kind, H, W, name, L, shifts):
    x, z, w = O.edge_prox_inputs(H, W)
    pr = dict(thr=O.PROX_L1_THR) if kind == 'l1' else O.PROX_CNC
    return S.prox(kind, x, z, w, pr, name, L, list(shifts)), S.prox(kind, x, z, w, pr, name, L, list(shifts), F32)


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('L', SPIN_L)
def test_spun_prox_per_element(P, torch, L, name, kind):
    """One prox in the frame of a single shift with 2^L - 1 on one axis, and one prox that averages K = 3 shifts (the synthesis emitters
    store, add and average-dual, each to a shifted, wrapped pixel of a partial tile), per element against wavelet_spin_oracle.prox."""
    H, W = O.EDGE_SIZES[L]
    x, z, w = O.edge_prox_inputs(H, W)
    bad = []
    with P.Engine(H, W, Bmax=BMAX) as eng:
        _dummy_problem(eng)
        eng.set_sparsity(name, L)
        for shifts in _spin_groups(L):
            r64, r32 = _spin_reference(kind, H, W, name, L, tuple(shifts))
            eng.set_spin(shifts, len(shifts))
            (xf, xt), (zf, zt), (wf, wt) = (_guarded(torch, a) for a in (x, z, w))
            _card_prox(eng, kind, STD[kind][0], xt, zt, wt)
            assert eng.spin_cursor == 1
            _intact(torch, xf, zf, wf)
            assert np.array_equal(xt.cpu().numpy(), x), 'x changed'
            part = O.partial_tile_mask(H, W, name, L, shifts=shifts)
            for arr, t, k in (('z+', zt, 0), ('w+', wt, 1)):
                _judge('spin %s %s L=%d %dx%d f32 K=%d %s' % (kind, name, L, H, W, len(shifts), arr), t.cpu().numpy(), r64[k],
                       _bars(False, r32[k], r64[k]), part, bad)
    assert not bad, '\n'.join(bad)


# ---- 4. the real kernels in double: one iteration from a given state ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loop_problem(H, W):
    """-> y [B, H, W] complex64, masks [B, H, W] uint8 (one per slice), z0, w0 float32"""
    y, mask, _ = O.problem(B, H, W)
    other = (np.random.default_rng(H + W).uniform(size=(H, W)) < 0.4).astype(np.uint8)
    other[0, 0] = 1
    _, z, w = O.edge_prox_inputs(H, W)
    return y, np.stack([mask, other]), z, w


def _loop_params(kind, params):
    return dict(zip(('lambda1', 'reo') if kind == 'l1' else ('alpha', 'lambda1', 'reo', 'b'), params))


def _double_iteration(eng, kind, params, off, H, W, name, L, bad, what='iteration'):
    """ONE iteration of admm_l1 / admm_cnc on a double context from set_state(z, w): x, z+ and w+ per element at 1e-12"""
    y, masks, z, w = _loop_problem(H, W)
    x, zn, wn = O.loop(y, masks, 1, kind, _loop_params(kind, params), name, L, z0=z, w0=w)
    O.check_branches(kind, params, off, x, z, w, name, L)
    eng.set_state(z, w)
    if kind == 'l1':
        eng.admm_l1(1, *params)
    else:
        eng.admm_cnc(1, *params)
    gz, gw = eng.get_state()
    gx = eng.x()
    assert gx.dtype == np.float64 and gz.dtype == np.float64
    w_scale = np.abs(x + w).reshape(B, -1).max(axis=1) if (kind == 'l1' and _thr_of(kind, params) == 0) else None
    part = O.partial_tile_mask(H, W, name, L)
    for arr, g, r, scale in (('x', gx, x, None), ('z+', gz, zn, None), ('w+', gw, wn, w_scale)):
        _judge('%s %s %r %s L=%d %dx%d f64 %s' % (what, kind, params, name, L, H, W, arr), g, r, O.F64_BAR, part, bad, scale)


def _double_engine(P, H, W, name, L):
    y, masks, _, _ = _loop_problem(H, W)
    eng = P.Engine(H, W, Bmax=BMAX, precision='f64')
    try:
        eng.upload(y, masks, np.arange(B, dtype=np.int32))
        eng.set_sparsity(name, L)
        assert eng.plan['launches_per_iteration'] == 5
    except BaseException:
        eng.close()
        raise
    return eng


@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('L,H,W', SIZES)
def test_one_iteration_on_double_contexts(P, L, H, W, name):
    """There is no real double step-wise call: one iteration of admm_l1 and of admm_cnc on a double context from set_state(z, w), a mask
    per slice, against wavelet_oracle.loop(iters=1, z0=, w0=).  Every filter at every size, so each meets every tile it has: haar 64 alone;
    db2 64 at L <= 3 and 32 at L = 4; db4 64 at L = 1 and 32 above."""
    bad = []
    with _double_engine(P, H, W, name, L) as eng:
        for kind in ('l1', 'cnc'):
            _double_iteration(eng, kind, *STD[kind], H, W, name, L, bad)
    assert not bad, '\n'.join(bad)


# ---- 5. the points that change the branch structure ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('H,W,name,L', POINT_CASES)
def test_points_that_change_the_branch_structure(P, torch, H, W, name, L, precision):
    """alpha = 0 and 1, b = 0.5 and 1e4, lambda1 = 0 and an L1 threshold of 0 (wavelet_oracle.edge_points): the branches each point leaves
    empty are asserted on the CPU; float through the step-wise prox, double through one iteration from set_state."""
    bad = []
    if precision == 'f32':
        with P.Engine(H, W, Bmax=BMAX) as eng:
            _dummy_problem(eng)
            eng.set_sparsity(name, L)
            for kind, params, off in O.edge_points():
                _float_step(torch, eng, kind, params, off, H, W, name, L, bad, 'point')
    else:
        with _double_engine(P, H, W, name, L) as eng:
            for kind, params, off in O.edge_points():
                _double_iteration(eng, kind, params, off, H, W, name, L, bad, 'point')
    assert not bad, '\n'.join(bad)


# ---- 6. the complex kernels at the deep levels --------------------------------------------------------------------------------------------

CX_THR = 0.3
CX_CNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)                    # tests/test_gpu_complex.py WCNC


@functools.lru_cache(maxsize=None)
def _complex_reference(kind, H, W, name, L):
    """-> x, z, w complex128 holding complex64 values, (z+, w+) of the oracle in complex128 and in complex64; slice by slice"""
    rng = np.random.default_rng(H + W + L)
    x, z, w = ((s * (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W)))).astype(np.complex64).astype(np.complex128)
               for s in (0.5, 0.5, 0.3))
    def step(b, dt):
        if kind == 'l1':
            return X.wl1_step(x[b], z[b], w[b], CX_THR, name, L, dt)
        return X.wcnc_step(x[b], z[b], w[b], name=name, levels=L, dt=dt, **CX_CNC)
    r64, r32 = ([step(b, dt) for b in range(B)] for dt in (np.complex128, np.complex64))
    stack = lambda r: tuple(np.stack([p[k] for p in r]) for k in (0, 1))
    return x, z, w, stack(r64), stack(r32)


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('H,W,name,L,precisions', CX_CASES)
def test_complex_prox_per_element(P, torch, H, W, name, L, precisions, kind):
    """prox_l1_dual / prox_cnc_dual of a coil context in complex image mode (set up as tests/test_gpu_complex.py::test_wavelet_prox) at
    L = 3 and 4 on partial tiles, per element against complex_oracle.wl1_step / wcnc_step, with guards."""
    C = 2
    x, z, w, r64, r32 = _complex_reference(kind, H, W, name, L)
    part = O.partial_tile_mask(H, W, name, L)
    bad = []
    for precision in precisions:
        f64 = precision == 'f64'
        dt = np.complex128 if f64 else np.complex64
        with P.Engine(H, W, Bmax=BMAX, precision=precision) as eng:
            eng.set_coils(M.coil_maps(C, H, W, 1))
            eng.set_sparsity(name, L)
            eng.set_image_mode('complex')
            eng.upload(np.zeros((B, C, H, W), np.complex64), M.mask(1, H, W))
            (xf, xt), (zf, zt), (wf, wt) = (_guarded(torch, a.astype(dt)) for a in (x, z, w))
            if kind == 'l1':
                eng.prox_l1_dual(xt, zt, wt, CX_THR)
            else:
                eng.prox_cnc_dual(xt, zt, wt, **CX_CNC)
            eng.sync()
            _intact(torch, xf, zf, wf)
            assert np.array_equal(xt.cpu().numpy(), x.astype(dt)), 'x changed'
            for arr, t, k in (('z+', zt, 0), ('w+', wt, 1)):
                _judge('complex %s %s L=%d %dx%d %s %s' % (kind, name, L, H, W, precision, arr), t.cpu().numpy(), r64[k],
                       _bars(f64, r32[k], r64[k]), part, bad)
    assert not bad, '\n'.join(bad)
