"""GPU tests of the locally low-rank prox (pnp_set_lowrank, Engine.set_lowrank, the lowrank= options of ADMM_L1 / ADMM_CNC) against the
NumPy restatement tests/lowrank_oracle.py (float64, by SVD).  Every figure printed before an assertion is what the card gave.

Bars.  Double contexts: rel-L2 <= 1e-12, for one step and for the loops.  Float contexts: 4 x the distance of the float32 restatement of
the oracle (the Gram route, the worse conditioned one, in float32) from the float64 one ON THE SAME CASE, computed here on the CPU and
printed, and never above the project's 1e-5.  For the loops the restatement of ten iterations was not known when the bar was set: where it
exceeds 2.5e-6 the test runs the largest count >= 3 at which it does not (3 if none) and prints the count.
MEASURED on this code (tests/lowrank_oracle.py, CPU): the restatement of ten iterations is 5.3e-6 .. 8.3e-6 and that of three CNC
iterations 3.6e-6 .. 5.1e-6, so L1 runs fewer than ten iterations and CNC three, at a bar capped at 1e-5.
The real step-wise prox call exists in float only (pnp_prox_l1_dual / pnp_prox_cnc_dual), so real double contexts run one whole
iteration from a set state (test_one_iteration_on_real_double_contexts)."""
import functools

import numpy as np
import pytest

import lowrank_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

FREEDOM = 4.0
F64_BAR, F32_CAP, RESTATEMENT_CAP = 1e-12, 1e-5, 2.5e-6
SHAPES = ((128, 128), (128, 130), (130, 129), (129, 131))
FRAMES = (2, 3, 5, 16, 17, 64)
CASES = [(i, s, T, b) for i, s in enumerate(SHAPES) for T in FRAMES for b in (5, 8, 16) if b < 16 or T <= 16]
C = 2


def _shifts(b):
    return ((0, 0), (3, 2), (b - 1, b - 1))


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to('cuda')


def _series(T, i):
    """S in {1, 3}: three series where the batch stays small, and once at T = 16 / 17"""
    return 3 if T <= 5 or (T in (16, 17) and i == 0) else 1


def _state(eng):
    return (eng.x(), *eng.get_state())


def _patch(a, S, T, rows, cols):
    return a.reshape((S, T) + a.shape[1:])[:, :, rows[:, None], cols[None, :]]


# ---- 1. one prox step, per element ---------------------------------------------------------------------------------------------------

def _designed(kind, S, T, b, grid, x, got_z, bar):
    """what the designed patches of lowrank_oracle.prox_inputs must give whatever the route: exact zeros, and the rank-1 scaling"""
    assert not _patch(got_z, S, T, *grid[0]).any()                                   # the all-zero patch
    if kind == 'l1':
        thr = O.PROX_L1['reo'] * O.PROX_L1['lambda1'] * O.default_scale(b)
        assert not _patch(got_z, S, T, *grid[2]).any()                               # rank 1 with sigma = thr (1 - 1e-3)
        u = _patch(x, S, T, *grid[1])                                                # rank 1, sigma = 50 thr: z+ = (1 - thr / sigma) u
        for s_ in range(S):
            sigma = np.linalg.norm(u[s_])
            assert rel_l2(_patch(got_z, S, T, *grid[1])[s_], (1.0 - thr / sigma) * u[s_]) <= bar


@pytest.mark.parametrize('i,shape,T,b', CASES)
def test_prox_step_against_the_oracle(P, i, shape, T, b):
    """prox_l1_dual / prox_cnc_dual with a block set, float, on random data and the designed patches of lowrank_oracle.prox_inputs (all
    zero, rank 1 far above and at thr (1 -+ 1e-3) and thr, z at ib (1 -+ 1e-3), constant in time, the partial last patch), Bmax > B, at
    the shifts (0, 0), (3, 2), (b - 1, b - 1): z+ and w+ against the float64 oracle with every element counted, x untouched."""
    H, W = shape
    S = _series(T, i)
    B = S * T
    with P.Engine(H, W, Bmax=B + 1) as eng:
        eng.upload(np.zeros((B, H, W), np.complex64), np.ones((H, W), np.uint8))
        eng.set_temporal(T)
        for shift in _shifts(b):
            x, z, w, grid = O.prox_inputs(S, T, H, W, b, shift)
            eng.set_lowrank(b, None, [shift])
            assert eng.lowrank == (b, b / 2.0, 1) and eng.temporal == (T, True)
            for kind, pr in (('l1', O.PROX_L1), ('cnc', O.PROX_CNC)):
                r64, r32 = O.prox(kind, x, z, w, pr, T, b, shift), O.prox(kind, x, z, w, pr, T, b, shift, R=np.float32)
                d32 = tuple(O.rel(c, a) for a, c in zip(r64, r32))
                xt, zt, wt = (_dev(a, np.float32) for a in (x, z, w))
                if kind == 'l1':
                    eng.prox_l1_dual(xt, zt, wt, pr['reo'] * pr['lambda1'])
                else:
                    eng.prox_cnc_dual(xt, zt, wt, **pr)
                eng.sync()
                got = (zt.cpu().numpy(), wt.cpu().numpy())
                assert np.array_equal(xt.cpu().numpy(), x.astype(np.float32))
                errs = tuple(rel_l2(g, r) for g, r in zip(got, r64))
                bars = tuple(min(FREEDOM * d, F32_CAP) for d in d32)
                print('prox %s %dx%d T=%d S=%d b=%d shift=%s f32: rel-L2 z+ %.2e, w+ %.2e (bars %.2e %.2e; float restatement %.2e %.2e)'
                      % ((kind, H, W, T, S, b, shift) + errs + bars + d32))
                assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
                assert all(e <= bar for e, bar in zip(errs, bars)), (errs, bars)
                _designed(kind, S, T, b, grid, x, got[0], F32_CAP)


@pytest.mark.parametrize('i,shape,T,b', CASES)
def test_one_iteration_on_real_double_contexts(P, i, shape, T, b):
    """The kernels in double (there is no real double step-wise call): ONE iteration of admm_l1 / admm_cnc on a double context from
    set_state(z, w) with the designed patches of lowrank_oracle.prox_inputs in z and w, a mask per slice -- x, z+ and w+ per element
    against the oracle's dc_step + prox at 1e-12, at every shift."""
    H, W = shape
    S = _series(T, i)
    B = S * T
    y, masks, _ = O.series_problem(S, T, H, W)
    with P.Engine(H, W, Bmax=B + 1, precision='f64') as eng:
        eng.upload(y, masks, np.arange(B, dtype=np.int32))
        eng.set_temporal(T)
        for shift in _shifts(b):
            _, z, w, grid = O.prox_inputs(S, T, H, W, b, shift)
            z = np.abs(z)                               # a state as the loops hold it
            eng.set_lowrank(b, None, [shift])
            for kind, pr in (('l1', O.PROX_L1), ('cnc', O.PROX_CNC)):
                ref = O.loop(y, masks, 1, kind, pr, T, b, [shift], z0=z, w0=w)
                eng.set_state(z, w)
                if kind == 'l1':
                    eng.admm_l1(1, pr['lambda1'], pr['reo'])
                else:
                    eng.admm_cnc(1, pr['alpha'], pr['lambda1'], pr['reo'], pr['b'])
                got = _state(eng)
                errs = tuple(rel_l2(g, r) for g, r in zip(got, ref))
                print('one iteration %s f64 %dx%d T=%d S=%d b=%d shift=%s: rel-L2 x %.2e, z+ %.2e, w+ %.2e (bar %.0e)'
                      % ((kind, H, W, T, S, b, shift) + errs + (F64_BAR,)))
                assert got[1].dtype == np.float64 and all(e <= F64_BAR for e in errs), errs


def test_all_zero_in_double(P):
    """all zero in double: from y = 0 and a zero state, x, z+ and w+ stay exactly zero through one iteration (every Gram matrix is zero,
    the sweep loop ends at once, M = 0), in L1 and CNC"""
    H, W, T, b = 128, 130, 5, 8
    with P.Engine(H, W, Bmax=T, precision='f64') as eng:
        eng.upload(np.zeros((T, H, W), np.complex64), np.ones((H, W), np.uint8))
        eng.set_temporal(T)
        eng.set_lowrank(b, None, [(3, 2)])
        z = np.zeros((T, H, W))
        eng.set_state(z, z)
        eng.admm_l1(1, 0.1, 0.015)
        assert not any(a.any() for a in _state(eng))
        eng.set_state(z, z)
        eng.admm_cnc(1, 0.45, 0.5, 0.05, 64)
        assert not any(a.any() for a in _state(eng))


# ---- 2. the bit rules ------------------------------------------------------------------------------------------------------------------

LOOP_CASES = ((1, 5, 128, 130), (1, 8, 130, 129))                  # (S, T, H, W) of the entry-point tests
BLOCK = 8
ITERS = 10


def _preset(kind):
    return dict(O.PRESETS[kind])


@functools.lru_cache(maxsize=None)
def _loop_case(S, T, H, W, ncoils):
    return O.series_problem(S, T, H, W, ncoils)


def _run(eng, kind, iters, **kw):
    p = _preset(kind)
    if kind == 'l1':
        return eng.admm_l1(iters, p['lambda1'], p['reo'], **kw)
    return eng.admm_cnc(iters, p['alpha'], p['lambda1'], p['reo'], p['b'], **kw)


def _open(P, S, T, H, W, ncoils, precision='f32', frames=True, lowrank=True, table='random'):
    y, masks, maps = _loop_case(S, T, H, W, ncoils)
    eng = P.Engine(H, W, Bmax=S * T + 1, precision=precision)
    if maps is not None:
        eng.set_coils(maps, 3)
    if frames:
        eng.set_temporal(T)
        if lowrank:
            eng.set_lowrank(BLOCK, None, O.shift_table(table, BLOCK))
    eng.upload(y, masks, np.arange(S * T, dtype=np.int32))
    return eng


@pytest.mark.parametrize('ncoils', [0, C], ids=['plain', 'coils'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_loops_are_their_steps_bit_for_bit(P, kind, ncoils):
    """n iterations == n rounds of dc_step + prox_*_dual on device tensors, the cursor walking the table in both; 7 iterations == 3 + 4 in
    two calls with the cursor carried; the plan says what is launched: the data-consistency step (3; with coils 5 + 5 cg_iters) and ONE
    prox launch."""
    import torch
    S, T, H, W = LOOP_CASES[0]
    n, p = 4, _preset(kind)
    with _open(P, S, T, H, W, ncoils) as eng:
        launches = 4 if ncoils == 0 else 5 + 5 * 3 + 1
        assert eng.plan['launches_per_iteration'] == launches == eng.kernels_per_iteration
        assert eng.lowrank == (BLOCK, BLOCK / 2.0, 64)
        eng.init_state()
        z0, w0 = eng.get_state()
        assert eng.lowrank_cursor == 0
        _run(eng, kind, n)
        assert eng.lowrank_cursor == n
        loop = _state(eng)
        zt, wt = _dev(z0, np.float32), _dev(w0, np.float32)
        xt = torch.empty_like(zt)
        eng.lowrank_cursor = 0
        for _ in range(n):
            eng.dc_step(zt, wt, xt, p['reo'])
            if kind == 'l1':
                eng.prox_l1_dual(xt, zt, wt, p['reo'] * p['lambda1'])
            else:
                eng.prox_cnc_dual(xt, zt, wt, p['alpha'], p['lambda1'], p['reo'], p['b'])
        eng.sync()
        assert eng.lowrank_cursor == n
        assert all(np.array_equal(a, c.cpu().numpy()) for a, c in zip(loop, (xt, zt, wt)))
        eng.init_state()
        _run(eng, kind, 7)
        seven = _state(eng)
        eng.init_state()
        _run(eng, kind, 3)
        assert eng.lowrank_cursor == 3
        _run(eng, kind, 4)
        assert eng.lowrank_cursor == 7
        assert all(np.array_equal(a, c) for a, c in zip(seven, _state(eng)))
        assert not np.array_equal(seven[0], loop[0])
        eng.init_state()                                                  # the cursor decides: 4 + 3 from a cursor set back differ
        _run(eng, kind, 3)
        eng.lowrank_cursor = 0
        _run(eng, kind, 4)
        assert not np.array_equal(seven[1], _state(eng)[1])


def _solve(P, kind, y, masks, maps, precision, **kw):
    fn = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    coil = {} if maps is None else dict(coils=maps, cg_iters=3)
    out, info = fn(masks, None, y=y, mask_id=np.arange(len(y)), return_info=True, precision=precision, **coil, **_preset(kind), **kw)
    return np.stack(out[:len(y)]), info


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_one_entry_table_is_no_shift_and_traced_is_untraced(P, kind, precision):
    """lowrank_shift=[[0, 0]] has the bits of lowrank_shift=None; trace_every=2 has the bits of the untraced run, and differs from the
    run on the random table"""
    S, T, H, W = LOOP_CASES[0]
    y, masks, _ = _loop_case(S, T, H, W, 0)
    kw = dict(frames=T, lowrank=BLOCK, iter_num=5)
    none, info = _solve(P, kind, y, masks, None, precision, lowrank_shift=None, **kw)
    one, _ = _solve(P, kind, y, masks, None, precision, lowrank_shift=[[0, 0]], **kw)
    assert np.array_equal(none, one) and info['lowrank']['block'] == BLOCK and info['lowrank']['scale'] == BLOCK / 2.0
    assert np.array_equal(info['lowrank']['shifts'], [[0, 0]]) and info['frames'] == T
    plain, info = _solve(P, kind, y, masks, None, precision, **kw)
    traced, tinfo = _solve(P, kind, y, masks, None, precision, trace_every=2, **kw)
    assert np.array_equal(info['lowrank']['shifts'], O.shift_table('random', BLOCK, 0))
    assert np.array_equal(plain, traced) and list(tinfo['trace']['iter']) == [2, 4, 5] and not np.array_equal(plain, none)


@pytest.mark.parametrize('ncoils', [0, C], ids=['plain', 'coils'])
def test_cleared_block_is_frames_alone_and_cleared_frames_the_pixel_path(P, ncoils):
    S, T, H, W = LOOP_CASES[0]

    def run(eng):
        eng.init_state()
        _run(eng, 'cnc', 4)
        return (eng.path_name, eng.plan, *_state(eng))

    with _open(P, S, T, H, W, ncoils, frames=False) as eng:
        pixel = run(eng)
    with _open(P, S, T, H, W, ncoils, lowrank=False) as eng:
        temporal = run(eng)
    with _open(P, S, T, H, W, ncoils) as eng:
        lowrank = run(eng)
        assert not np.array_equal(lowrank[3], temporal[3]) and lowrank[:2] == temporal[:2]
        eng.set_lowrank(0)
        assert eng.lowrank is None and eng.temporal == (T, True)
        again = run(eng)
        assert again[:2] == temporal[:2] and all(np.array_equal(a, c) for a, c in zip(again[2:], temporal[2:]))
        eng.set_lowrank(BLOCK, None, O.shift_table('random', BLOCK))
        eng.set_temporal(None)                                            # clearing frames clears the block
        assert eng.lowrank is None and eng.temporal == (None, True)
        again = run(eng)
        assert again[:2] == pixel[:2] and all(np.array_equal(a, c) for a, c in zip(again[2:], pixel[2:]))


# ---- 3. the entry points ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loop_reference(S, T, H, W, ncoils, kind):
    """-> (iterations, x of the float64 oracle after them, distance of the float restatement): ten iterations, or the largest count >= 3
    whose restatement stays within 2.5e-6 (3 if none does)"""
    y, masks, maps = _loop_case(S, T, H, W, ncoils)
    every = tuple(range(1, ITERS + 1))
    if maps is None:
        run = lambda R: [s[0] for s in O.loop(y, masks, ITERS, kind, _preset(kind), T, BLOCK, 'random', R=R, states=every)[3]]
    else:
        run = lambda R: O.coil_loop(y, maps, masks, ITERS, kind, _preset(kind), T, BLOCK, 'random', R=R, states=every)[3]
    r64, r32 = run(np.float64), run(np.float32)
    for n in range(ITERS, 2, -1):
        d32 = O.rel(r32[n - 1], r64[n - 1])
        if d32 <= RESTATEMENT_CAP or n == 3:
            return n, r64[n - 1], d32


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('ncoils', [0, C], ids=['plain', 'coils'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('S,T,H,W', LOOP_CASES)
def test_loops_against_the_oracle(P, S, T, H, W, kind, ncoils, precision):
    """ADMM_L1 / ADMM_CNC at the presets through the entry points with frames= and lowrank=8 on the default random table, a mask per slice
    through mask_id, without coils and with coils= (C = 2, cg_iters = 3): x against the oracle's loop with the same table.  Double: ten
    iterations at 1e-12.  Float: the count of _loop_reference (printed), at 4 x its restatement, capped at 1e-5."""
    y, masks, maps = _loop_case(S, T, H, W, ncoils)
    if precision == 'f64':
        iters, d32 = ITERS, float('nan')
        every = (ITERS,)
        ref = (O.loop(y, masks, ITERS, kind, _preset(kind), T, BLOCK, 'random')[0] if maps is None else
               O.coil_loop(y, maps, masks, ITERS, kind, _preset(kind), T, BLOCK, 'random')[0])
        bar = F64_BAR
    else:
        iters, ref, d32 = _loop_reference(S, T, H, W, ncoils, kind)
        bar = min(FREEDOM * d32, F32_CAP)
    got, info = _solve(P, kind, y, masks, maps, precision, frames=T, lowrank=BLOCK, iter_num=iters)
    err = rel_l2(got, ref)
    print('loop %s %s %dx%d T=%d S=%d %s: %d iterations%s, rel-L2 of x %.3e (bar %.3e; float restatement %.3e)'
          % (kind, 'coils' if ncoils else 'plain', H, W, T, S, precision, iters, '' if iters == ITERS else ' (stepped down from %d)' % ITERS,
             err, bar, d32))
    assert info['lowrank']['block'] == BLOCK and info['frames'] == T
    assert err <= bar, (err, bar)


# ---- 4. the regulariser does what it is for ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _phantom_gap():
    img, masks, y = O.relaxation_problem(16, 128, 128)
    pr = O.PRESETS['l1']
    return img, masks, y, O.psnr(O.loop(y, masks, 50, 'l1', pr, 16, 8, 'random')[0], img) - O.psnr(O.TO.loop(y, masks, 50, 'l1', pr)[0], img)


def test_lowrank_l1_beats_pixel_l1_on_the_relaxation_phantom(P):
    """16 x 128 x 128, another column mask per frame through mask_id, 50 iterations at the preset: ADMM_L1 with lowrank=8 ends at least
    2 dB above pixel ADMM_L1, and within 0.5 dB of the gap the float64 oracle finds on the same inputs.  Without the feature lowrank= is
    ignored, both runs are the same run and the gap is 0."""
    img, masks, y, oracle_gap = _phantom_gap()
    kw = dict(y=y, mask_id=np.arange(16), iter_num=50, **O.PRESETS['l1'])
    pix = np.stack(P.ADMM_L1(masks, None, **kw)[:16])
    llr = np.stack(P.ADMM_L1(masks, None, frames=16, lowrank=8, **kw)[:16])
    gap = O.psnr(llr, img) - O.psnr(pix, img)
    print('relaxation phantom: pixel prox %.2f dB, low-rank prox %.2f dB: gap %.2f dB (oracle %.2f dB)' % (O.psnr(pix, img), O.psnr(llr, img), gap, oracle_gap))
    assert gap >= 2.0 and gap >= oracle_gap - 0.5, (gap, oracle_gap)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_refusals(P, precision):
    """every rule with its code and literal message, in both precisions"""
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    H, W = 128, 128
    E_ARG, E_STATE = -1, -3
    f64 = precision == 'f64'

    def refused(code, msg, fn, *a):
        with pytest.raises(_lib.PnpError) as e:
            fn(*a)
        assert e.value.code == code and str(e.value) == 'libpnpmri error %d: %s' % (code, msg), str(e.value)

    with P.Engine(H, W, Bmax=8, precision=precision) as eng:
        refused(E_STATE, 'pnp_set_lowrank: no series length set (pnp_set_temporal)', eng.set_lowrank, 8)
        refused(E_STATE, 'pnp_set_lowrank_cursor: no low-rank setting (pnp_set_lowrank)', lambda: setattr(eng, 'lowrank_cursor', 1))
        eng.set_temporal(4)
        for b in (1, 33, -2):
            refused(E_ARG, 'lowrank: block must be 2..32 (got %d)' % b, eng.set_lowrank, b)
        refused(E_ARG, 'pnp_set_lowrank: scale must be a positive number (got 0)', eng.set_lowrank, 8, 0.0)
        refused(E_ARG, 'pnp_set_lowrank: shift 1 = (0, 8) out of range [0, 8)',
                lambda: _lib.check(eng._L.pnp_set_lowrank(eng._ctx, 8, 4.0, (_lib.C.c_int32 * 4)(0, 0, 0, 8), 2)))
        refused(E_ARG, 'pnp_set_lowrank: shifts must be a table of 1..65536 pairs (got 0, null)',
                lambda: _lib.check(eng._L.pnp_set_lowrank(eng._ctx, 8, 4.0, None, 0)))
        assert eng.lowrank is None
        eng.set_temporal(64)
        refused(E_ARG, 'lowrank: a patch of 32 x 32 pixels over 64 frames does not fit the LDS of a workgroup in %s (L1)' % ('double' if f64 else 'float'),
                eng.set_lowrank, 32)
        eng.set_temporal(4)
        eng.set_lowrank(8)
        assert eng.lowrank == (8, 4.0, 1)
        # a wavelet or a spin table: the rules of the series length
        refused(E_STATE, 'pnp_set_sparsity: a wavelet does not run with temporal sparsity (clear it with pnp_set_temporal(ctx, 0, 1))', eng.set_sparsity, 'haar', 2)
        refused(E_STATE, 'pnp_set_spin: a spin table does not run with temporal sparsity (clear it with pnp_set_temporal(ctx, 0, 1))', eng.set_spin,
                np.zeros((1, 2), np.int32), 1)
        # another series length keeps the block if the patch fits
        eng.set_lowrank(32)
        refused(E_ARG, 'lowrank: a patch of 32 x 32 pixels over 64 frames does not fit the LDS of a workgroup in %s (L1)' % ('double' if f64 else 'float'),
                eng.set_temporal, 64)
        assert eng.temporal == (4, True) and eng.lowrank == (32, 16.0, 1)
        eng.set_lowrank(8)
        # B % frames at a loop and at a prox call
        eng.upload(np.zeros((6, H, W), np.complex64), np.ones((H, W), np.uint8))
        eng.init_state()
        msg = 'temporal: the batch of 6 slices is not a whole number of series of 4 frames'
        refused(E_STATE, msg, eng.admm_l1, 2, 0.1, 0.015)
        refused(E_STATE, msg, eng.admm_cnc, 2, 0.45, 0.5, 0.05, 64)
        refused(E_STATE, msg, lambda: eng.admm_l1(2, 0.1, 0.015, trace_every=1))
        t = [torch.zeros((6, H, W), dtype=torch.float64 if f64 else torch.float32, device='cuda') for _ in range(3)]
        if f64:                                                  # the step-wise real prox in double, as before
            refused(E_STATE, 'pnp_prox_l1_dual: not available on an fp64 validation context', eng.prox_l1_dual, *t, 0.1)
        else:
            refused(E_STATE, msg, eng.prox_l1_dual, *t, 0.1)
            refused(E_STATE, msg, eng.prox_cnc_dual, *t, 0.45, 0.5, 0.05, 64)
        eng.set_temporal(3)                                      # the same batch as two series of three; the block stays
        assert eng.lowrank == (8, 4.0, 1)
        eng.admm_l1(2, 0.1, 0.015)
        eng.set_lowrank(8)
        # complex image mode, in either order
        eng.set_coils(O.M.coil_maps(C, H, W, 1))
        refused(E_STATE, 'pnp_set_image: complex images do not run with a low-rank block (clear it with pnp_set_lowrank(ctx, 0, 0, NULL, 0))',
                eng.set_image_mode, 'complex')
        eng.set_lowrank(0)
        eng.set_image_mode('complex')
        refused(E_STATE, 'pnp_set_lowrank: not available in complex image mode (pnp_set_image)', eng.set_lowrank, 8)
        assert eng.lowrank is None
    # a CNC step whose patch fits for L1 alone (22 x 22 over 20 frames in double, over 40 in float) is refused where it is made
    T = 20 if f64 else 40
    with P.Engine(H, W, Bmax=T, precision=precision) as eng:
        eng.upload(np.zeros((T, H, W), np.complex64), np.ones((H, W), np.uint8))
        eng.set_temporal(T)
        eng.set_lowrank(22)
        eng.init_state()
        eng.admm_l1(1, 0.1, 0.015)
        msg = 'lowrank: a patch of 22 x 22 pixels over %d frames does not fit the LDS of a workgroup in %s (CNC)' % (T, 'double' if f64 else 'float')
        refused(E_ARG, msg, eng.admm_cnc, 1, 0.45, 0.5, 0.05, 64)
        with pytest.raises(ValueError, match='^' + msg.replace('(', r'\(').replace(')', r'\)') + '$'):
            P.ADMM_CNC(np.ones((H, W), np.uint8), None, y=np.zeros((T, H, W), np.complex64), frames=T, lowrank=22, precision=precision)
