"""GPU tests of temporal sparsity (pnp_set_temporal, Engine.set_temporal, the frames= / temporal_keep_dc= options of ADMM_L1 / ADMM_CNC)
against the NumPy restatement tests/temporal_oracle.py.  Every figure printed before an assertion is what the card gave.

Bars.  Double contexts: 1e-12 for one prox step (four orders above the round-off of a 64-term double sum; an indexing error is O(1)),
1e-10 for a loop of ten iterations (the project's bar for double loops).  Float contexts: 4 x the distance of the float32 restatement of
the oracle -- the same direct sums with every product and sum rounded to float32 -- from the float64 one ON THE SAME CASE, computed here
on the CPU and printed (DESIGN.md sections 13, 20: the factor is for the freedom in fma contraction and in the order of independent
sums); for the loops that bar itself must stay within the project's 1e-5, and a CNC case whose restatement exceeded 2.5e-6 at ten
iterations would run at the largest count >= 3 at which it does not (none does: the largest measured is 1.6e-6).
The real step-wise prox call exists in float only (pnp_prox_l1_dual / pnp_prox_cnc_dual), so the one-step test runs double contexts in
complex mode, and real double contexts run one whole iteration from a set state (test_one_iteration_on_real_double_contexts)."""
import functools

import numpy as np
import pytest

import temporal_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

FREEDOM = 4.0
F64_STEP, F64_LOOP, LOOP_BAR_CAP, CNC_RESTATEMENT_CAP = 1e-12, 1e-10, 1e-5, 2.5e-6
SHAPES = ((128, 128), (128, 130), (130, 129), (129, 131))          # N % 4 = 0, 0, 2 and N odd
FRAMES = (2, 3, 5, 16, 17, 64)
C = 2


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to('cuda')


def _real(precision):
    return np.float64 if precision == 'f64' else np.float32


def _cplx(precision):
    return np.complex128 if precision == 'f64' else np.complex64


def _series(T, i):
    """S in {1, 3}: three series where the batch stays small, and once at T = 16 / 17"""
    return 3 if T <= 5 or (T in (16, 17) and i == 0) else 1


def _keep_dc(i, j, cx):
    return bool((i + j + cx) % 2)


# ---- 1. one prox step, per element ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _step_case(S, T, H, W, cx, keep_dc):
    x, z, w = O.prox_inputs(S, T, H, W, cx)
    ref = {}
    for kind, pr in (('l1', O.PROX_L1), ('cnc', O.PROX_CNC)):
        r64, r32 = O.prox(kind, x, z, w, pr, T, keep_dc, cx=cx), O.prox(kind, x, z, w, pr, T, keep_dc, R=np.float32, cx=cx)
        ref[kind] = (r64, O.structural_zeros(kind, x, z, w, pr, T, keep_dc, cx), tuple(O.rel(b, a) for a, b in zip(r64, r32)))
    return x, z, w, ref


def _step(eng, kind, xt, zt, wt):
    if kind == 'l1':
        eng.prox_l1_dual(xt, zt, wt, O.PROX_L1['reo'] * O.PROX_L1['lambda1'])
    else:
        eng.prox_cnc_dual(xt, zt, wt, **O.PROX_CNC)
    eng.sync()


@pytest.mark.parametrize('cx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('j,T', list(enumerate(FRAMES)))
@pytest.mark.parametrize('i,shape', list(enumerate(SHAPES)))
def test_prox_step_against_the_oracle(P, i, shape, j, T, cx):
    """prox_l1_dual / prox_cnc_dual with frames set, on random data and the designed set of temporal_oracle.prox_inputs, Bmax > B: z+ and
    w+ against the float64 oracle with every element counted, exact zeros where the oracle's thresholded spectrum is all zero
    (temporal_oracle.structural_zeros: in both precisions, from the float64 oracle alone), x untouched.  keep_dc alternates over the grid; both values meet every T, every shape, both kinds and both modes."""
    H, W = shape
    S, keep_dc = _series(T, i), _keep_dc(i, j, cx)
    B = S * T
    x, z, w, ref = _step_case(S, T, H, W, cx, keep_dc)
    for precision in (('f32', 'f64') if cx else ('f32',)):
        dt = _cplx(precision) if cx else _real(precision)
        with P.Engine(H, W, Bmax=B + 1, precision=precision) as eng:
            if cx:
                eng.set_coils(O.M.coil_maps(C, H, W, 1))
                eng.set_image_mode('complex')
                eng.upload(np.zeros((B, C, H, W), np.complex64), np.ones((H, W), np.uint8))
            else:
                eng.upload(np.zeros((B, H, W), np.complex64), np.ones((H, W), np.uint8))
            eng.set_temporal(T, keep_dc)
            assert eng.temporal == (T, keep_dc)
            for kind in ('l1', 'cnc'):
                (r64, zero, d32) = ref[kind]
                xt, zt, wt = (_dev(a, dt) for a in (x, z, w))
                _step(eng, kind, xt, zt, wt)
                got = (zt.cpu().numpy(), wt.cpu().numpy())
                assert np.array_equal(xt.cpu().numpy(), x.astype(dt))
                errs = tuple(rel_l2(g, r) for g, r in zip(got, r64))
                bars = (F64_STEP, F64_STEP) if precision == 'f64' else tuple(FREEDOM * d for d in d32)
                print('prox %s %s %dx%d T=%d S=%d keep_dc=%d %s: rel-L2 z+ %.2e, w+ %.2e (bars %.2e %.2e; float restatement %.2e %.2e); '
                      '%d exact zeros' % ((kind, 'complex' if cx else 'real', H, W, T, S, keep_dc, precision) + errs + bars + d32 + (int(zero.sum()),)))
                assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)
                assert zero.sum() >= S * T and not r64[0][zero].any() and not got[0][zero].any()
                assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


@pytest.mark.parametrize('T', [2, 16, 17, 64])
@pytest.mark.parametrize('i,shape', list(enumerate(SHAPES)))
def test_one_iteration_on_real_double_contexts(P, i, shape, T):
    """The real kernels in double (there is no real double step-wise call): ONE iteration of admm_l1 / admm_cnc on a double context from
    set_state(z, w) with the designed set of temporal_oracle.prox_inputs in z and w, a mask per slice -- x, z+ and w+ per element against
    the oracle's dc_step + prox at 1e-12.  Even T runs the real Nyquist coefficient and its (-1)^t term, T = 64 the smallest runs."""
    H, W = shape
    S = _series(T, i)
    B, keep_dc = S * T, bool((i + T) % 2)
    _, z, w = O.prox_inputs(S, T, H, W)
    z = np.abs(z)                                    # a state as the loops hold it: z >= 0 is not required, but x = |.| is what dc returns
    y, masks, _ = O.series_problem(S, T, H, W)
    with P.Engine(H, W, Bmax=B + 1, precision='f64') as eng:
        eng.upload(y, masks, np.arange(B, dtype=np.int32))
        eng.set_temporal(T, keep_dc)
        for kind, pr in (('l1', O.PROX_L1), ('cnc', O.PROX_CNC)):
            ref = O.loop(y, masks, 1, kind, pr, T, keep_dc, z0=z, w0=w)
            eng.set_state(z, w)
            if kind == 'l1':
                eng.admm_l1(1, pr['lambda1'], pr['reo'])
            else:
                eng.admm_cnc(1, pr['alpha'], pr['lambda1'], pr['reo'], pr['b'])
            got = _state(eng)
            errs = tuple(rel_l2(g, r) for g, r in zip(got, ref))
            zero = O.structural_zeros(kind, ref[0], z, w, pr, T, keep_dc)
            print('one iteration %s real f64 %dx%d T=%d S=%d keep_dc=%d: rel-L2 x %.2e, z+ %.2e, w+ %.2e (bar %.0e); %d exact zeros'
                  % ((kind, H, W, T, S, keep_dc) + errs + (F64_STEP, int(zero.sum()))))
            assert got[1].dtype == np.float64 and all(e <= F64_STEP for e in errs), errs
            assert not got[1][zero].any()


# ---- 2. whole loops ------------------------------------------------------------------------------------------------------------------

LOOP_CASES = ((2, 5, 128, 130), (1, 3, 129, 131), (1, 8, 130, 129))   # (S, T, H, W): T odd, prime, even (the real Nyquist coefficient)
MODES = (('plain', 0, False), ('coils', C, False), ('complex', C, True))
ITERS = 10


def _preset(kind):
    return dict(O.PRESETS[kind])


@functools.lru_cache(maxsize=None)
def _loop_case(S, T, H, W, ncoils, cx):
    return O.series_problem(S, T, H, W, ncoils, cx)


def _oracle_loop(y, masks, maps, iters, kind, T, cx, R=np.float64):
    if maps is None:
        return O.loop(y, masks, iters, kind, _preset(kind), T, R=R)[0]
    return O.coil_loop(y, maps, masks, iters, kind, _preset(kind), T, R=R, cx=cx)[0]


@functools.lru_cache(maxsize=None)
def _loop_reference(S, T, H, W, ncoils, cx, kind):
    """-> (iterations, x of the float64 oracle, distance of the float restatement): ten iterations, or for CNC the largest count >= 3 whose
    restatement stays within 2.5e-6"""
    y, masks, maps = _loop_case(S, T, H, W, ncoils, cx)
    for n in range(ITERS, 2, -1):
        ref = _oracle_loop(y, masks, maps, n, kind, T, cx)
        d32 = O.rel(_oracle_loop(y, masks, maps, n, kind, T, cx, np.float32), ref)
        if kind == 'l1' or d32 <= CNC_RESTATEMENT_CAP or n == 3:
            return n, ref, d32


def _solve(P, kind, y, masks, maps, cx, precision, **kw):
    fn = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    coil = {} if maps is None else dict(coils=maps, cg_iters=3)
    if cx:
        coil['image'] = 'complex'
    out, info = fn(masks, None, y=y, mask_id=np.arange(len(y)), return_info=True, precision=precision, **coil, **_preset(kind), **kw)
    return np.stack(out[:len(y)]), info


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('mode,ncoils,cx', MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('S,T,H,W', LOOP_CASES)
def test_loops_against_the_oracle(P, S, T, H, W, kind, mode, ncoils, cx, precision):
    """ADMM_L1 / ADMM_CNC at the presets through the entry points with frames=, a mask per slice through mask_id: without coils, with
    coils= (C = 2, cg_iters = 3), and with image='complex'; x against the oracle loop."""
    y, masks, maps = _loop_case(S, T, H, W, ncoils, cx)
    iters, ref, d32 = _loop_reference(S, T, H, W, ncoils, cx, kind)
    got, info = _solve(P, kind, y, masks, maps, cx, precision, frames=T, iter_num=iters)
    bar = F64_LOOP if precision == 'f64' else FREEDOM * d32
    err = rel_l2(got, ref)
    print('loop %s %s %dx%d T=%d S=%d %s: %d iterations, rel-L2 of x %.3e (bar %.3e; float restatement %.3e)'
          % (kind, mode, H, W, T, S, precision, iters, err, bar, d32))
    assert info['frames'] == T and np.iscomplexobj(got) == cx
    assert FREEDOM * d32 <= LOOP_BAR_CAP and (kind == 'l1' or iters == ITERS or d32 <= CNC_RESTATEMENT_CAP)
    assert err <= bar, (err, bar)


def _run(eng, kind, iters, **kw):
    p = _preset(kind)
    if kind == 'l1':
        return eng.admm_l1(iters, p['lambda1'], p['reo'], **kw)
    return eng.admm_cnc(iters, p['alpha'], p['lambda1'], p['reo'], p['b'], **kw)


def _open(P, S, T, H, W, ncoils, cx, precision='f32', frames=True, keep_dc=True):
    y, masks, maps = _loop_case(S, T, H, W, ncoils, cx)
    eng = P.Engine(H, W, Bmax=S * T + 1, precision=precision)
    if maps is not None:
        eng.set_coils(maps, 3)
    if cx:
        eng.set_image_mode('complex')
    if frames:
        eng.set_temporal(T, keep_dc)
    eng.upload(y, masks, np.arange(S * T, dtype=np.int32))
    return eng


def _state(eng):
    return (eng.x(), *eng.get_state())


@pytest.mark.parametrize('mode,ncoils,cx,precision', [('plain', 0, False, 'f32'), ('coils', C, False, 'f32'), ('complex', C, True, 'f32'),
                                                      ('complex', C, True, 'f64')])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_loops_are_their_steps_bit_for_bit(P, kind, mode, ncoils, cx, precision):
    """n iterations == n rounds of dc_step + prox_*_dual on device tensors; 7 iterations == 3 + 4 in two calls; the plan says what is
    launched: the data-consistency step (3; with coils 5 + 5 cg_iters) and ONE prox launch, never slice-resident."""
    import torch
    S, T, H, W = LOOP_CASES[0]
    n, p = 4, _preset(kind)
    with _open(P, S, T, H, W, ncoils, cx, precision) as eng:
        launches = 4 if ncoils == 0 else 5 + 5 * 3 + 1
        assert eng.plan['launches_per_iteration'] == launches == eng.kernels_per_iteration
        assert eng.path_name == ('coils' if ncoils else 'generic')
        eng.init_state()
        z0, w0 = eng.get_state()
        _run(eng, kind, n)
        loop = _state(eng)
        dt = _cplx(precision) if cx else _real(precision)
        zt, wt = _dev(z0, dt), _dev(w0, dt)
        xt = torch.empty_like(zt)
        for _ in range(n):
            eng.dc_step(zt, wt, xt, p['reo'])
            if kind == 'l1':
                eng.prox_l1_dual(xt, zt, wt, p['reo'] * p['lambda1'])
            else:
                eng.prox_cnc_dual(xt, zt, wt, p['alpha'], p['lambda1'], p['reo'], p['b'])
        eng.sync()
        assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(loop, (xt, zt, wt)))
        eng.init_state()
        _run(eng, kind, 7)
        seven = _state(eng)
        eng.init_state()
        _run(eng, kind, 3)
        _run(eng, kind, 4)
        assert all(np.array_equal(a, b) for a, b in zip(seven, _state(eng)))
        assert not np.array_equal(seven[0], loop[0])


# ---- 3. the regulariser does what it is for ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _phantom_gap():
    img, masks, y = O.dynamic_problem(16, 128, 128)
    pr = O.PRESETS['l1']
    return img, masks, y, O.psnr(O.loop(y, masks, 50, 'l1', pr, 16)[0], img) - O.psnr(O.loop(y, masks, 50, 'l1', pr)[0], img)


def test_temporal_l1_beats_pixel_l1_on_the_dynamic_phantom(P):
    """16 x 128 x 128, another column mask per frame through mask_id, 50 iterations at the preset: temporal ADMM_L1 ends at least 2 dB
    above pixel ADMM_L1, and within 0.5 dB of the gap the float64 oracle finds on the same inputs.  Without the feature frames= is
    ignored, both runs are the same run and the gap is 0."""
    img, masks, y, oracle_gap = _phantom_gap()
    kw = dict(y=y, mask_id=np.arange(16), iter_num=50, **O.PRESETS['l1'])
    pix = np.stack(P.ADMM_L1(masks, None, **kw)[:16])
    tmp = np.stack(P.ADMM_L1(masks, None, frames=16, **kw)[:16])
    gap = O.psnr(tmp, img) - O.psnr(pix, img)
    print('dynamic phantom: pixel prox %.2f dB, temporal prox %.2f dB: gap %.2f dB (oracle %.2f dB)' % (O.psnr(pix, img), O.psnr(tmp, img), gap, oracle_gap))
    assert gap >= 2.0 and gap >= oracle_gap - 0.5, (gap, oracle_gap)


# ---- 4. traced run -------------------------------------------------------------------------------------------------------------------

def _norm(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).reshape(len(a), -1).sum(axis=1))


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_traced_run(P, kind, precision):
    """trace_every=2 with frames= through the entry point: the bits of the untraced run, and rows that are the NumPy norms of the oracle's
    states under the trace tests' bars -- float: max(4 x the float restatement's own deviation, 2e-5) want + 1e-6 x_norm; double: 1e-9
    want + 1e-12 x_norm."""
    S, T, H, W = LOOP_CASES[0]
    y, masks, _ = _loop_case(S, T, H, W, 0, False)
    K, checks = 7, (2, 4, 6, 7)
    plain, _ = _solve(P, kind, y, masks, None, False, precision, frames=T, iter_num=K)
    got, info = _solve(P, kind, y, masks, None, False, precision, frames=T, iter_num=K, trace_every=2)
    tr = info['trace']
    assert np.array_equal(got, plain) and list(tr['iter']) == list(checks) and tr['iters_done'] == K
    rows = lambda R: [dict(r_pri=_norm(x - z), r_dual=_norm(z - zp), x_norm=_norm(x), z_norm=_norm(z), w_norm=_norm(w))
                      for x, z, zp, w in O.loop(y, masks, K, kind, _preset(kind), T, R=R, states=checks)[3]]
    ref, ctl = rows(np.float64), rows(np.float32)
    names = ('r_pri', 'r_dual', 'x_norm', 'z_norm', 'w_norm')
    control = max(float(np.max(np.maximum(np.abs(c[n] - r[n]) - 1e-6 * r['x_norm'], 0) / np.where(r[n] > 0, r[n], 1))) for c, r in zip(ctl, ref) for n in names)
    rtol, atol = (1e-9, 1e-12) if precision == 'f64' else (max(FREEDOM * control, 2e-5), 1e-6)
    worst = 0.0
    for k, r in enumerate(ref):
        for n in names:
            dev = np.abs(tr[n][k] - r[n])
            worst = max(worst, float(np.max(dev / np.where(r[n] > 0, r[n], 1))))
            assert (dev <= rtol * r[n] + atol * r['x_norm']).all(), (checks[k], n, dev, r[n])
    print('traced %s %s: float restatement %.2e -> rtol %.2e; worst relative deviation of a row %.2e' % (kind, precision, control, rtol, worst))


# ---- 5. nothing else moved -------------------------------------------------------------------------------------------------------------

def _synthetic(P, B, H=256, W=256):
    from pnp_admm_cnc_mri_amd import synthetic
    img, noise = synthetic.batch(3, B)
    return img, noise, synthetic.reference_masks()['Q_Random30'].astype(np.uint8)


@pytest.mark.parametrize('B,path', [(64, 'slice'), (4, 'fused')])
def test_set_and_cleared_is_a_fresh_engine(P, B, path):
    """set_temporal(frames) and set_temporal(None) again, on the slice-resident and the two-launch 256 x 256 path: the bits, the path name
    and the plan of an engine that never had the setting; with it set the path reads 'fused' at four launches per iteration."""
    img, noise, mask = _synthetic(P, B)
    p = _preset('cnc')

    def run(eng):
        eng.init_state()
        eng.admm_cnc(5, p['alpha'], p['lambda1'], p['reo'], p['b'])
        return _state(eng)

    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, mask)
        fresh = (eng.path_name, eng.plan, run(eng))
        assert fresh[0] == path
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, mask)
        eng.set_temporal(4)
        assert eng.path_name == 'fused' and eng.plan['launches_per_iteration'] == 4 and eng.temporal == (4, True)
        assert not np.array_equal(run(eng)[0], fresh[2][0])
        eng.set_temporal(None)
        assert eng.temporal == (None, True) and eng.path_name == path and eng.plan == fresh[1]
        assert all(np.array_equal(a, b) for a, b in zip(run(eng), fresh[2]))


@pytest.mark.parametrize('what', ['wavelet', 'coils'])
def test_set_and_cleared_on_a_wavelet_and_a_coil_context(P, what):
    S, T, H, W = LOOP_CASES[0]
    ncoils = C if what == 'coils' else 0

    def prepare(eng):
        if what == 'wavelet':
            eng.set_sparsity('db2', 1)

    def run(eng):
        eng.init_state()
        _run(eng, 'cnc', 4)
        return (eng.path_name, eng.plan, *_state(eng))

    with _open(P, S, T, H, W, ncoils, False, frames=False) as eng:
        prepare(eng)
        fresh = run(eng)
    with _open(P, S, T, H, W, ncoils, False, frames=False) as eng:
        eng.set_temporal(T, False)
        with_frames = run(eng)
        assert not np.array_equal(with_frames[2], fresh[2])
        eng.set_temporal(None)
        prepare(eng)
        again = run(eng)
        assert again[:2] == fresh[:2] and all(np.array_equal(a, b) for a, b in zip(again[2:], fresh[2:]))
        if what == 'coils':                                   # set_coils and set_image_mode keep the setting
            eng.set_temporal(T, False)
            eng.set_coils(_loop_case(S, T, H, W, ncoils, False)[2], 3)
            assert eng.temporal == (T, False)
            eng.set_image_mode('complex')
            assert eng.temporal == (T, False)


@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_refusals(P, precision):
    """every rule with its code and literal message, in both precisions"""
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    H, W = 128, 128
    E_ARG, E_STATE = -1, -3

    def refused(code, msg, fn, *a):
        with pytest.raises(_lib.PnpError) as e:
            fn(*a)
        assert e.value.code == code and str(e.value) == 'libpnpmri error %d: %s' % (code, msg), str(e.value)

    L = _lib.lib()
    with P.Engine(H, W, Bmax=8, precision=precision) as eng:
        for f in (1, 65, -2):
            assert L.pnp_set_temporal(eng._ctx, f, 1) == E_ARG
            assert L.pnp_last_error().decode() == 'temporal: frames must be 2..64 (got %d)' % f
            with pytest.raises(ValueError, match=r'^temporal: frames must be 2\.\.64 \(got %d\)$' % f):
                eng.set_temporal(f)
        assert eng.temporal == (None, True)
        # frames, then a wavelet or a spin table
        eng.set_temporal(4)
        refused(E_STATE, 'pnp_set_sparsity: a wavelet does not run with temporal sparsity (clear it with pnp_set_temporal(ctx, 0, 1))', eng.set_sparsity, 'haar', 2)
        shifts = np.zeros((1, 2), np.int32)
        refused(E_STATE, 'pnp_set_spin: a spin table does not run with temporal sparsity (clear it with pnp_set_temporal(ctx, 0, 1))', eng.set_spin, shifts, 1)
        eng.set_sparsity(None)                                   # clearing a wavelet is no conflict
        assert eng.temporal == (4, True)
        # a wavelet (and its spin table), then frames
        eng.set_temporal(None)
        eng.set_sparsity('haar', 2)
        refused(E_STATE, 'pnp_set_temporal: temporal sparsity does not run with a wavelet (clear it with pnp_set_sparsity(ctx, PNP_WAVELET_NONE, 0))',
                eng.set_temporal, 4)
        eng.set_spin(shifts, 1)
        refused(E_STATE, 'pnp_set_temporal: temporal sparsity does not run with a wavelet and its spin table (clear it with '
                'pnp_set_sparsity(ctx, PNP_WAVELET_NONE, 0))', eng.set_temporal, 4)
        assert eng.temporal == (None, True)
        eng.set_sparsity(None)
        # B % frames at a loop and at a prox call
        eng.set_temporal(4)
        eng.upload(np.zeros((6, H, W), np.complex64), np.ones((H, W), np.uint8))
        eng.init_state()
        msg = 'temporal: the batch of 6 slices is not a whole number of series of 4 frames'
        refused(E_STATE, msg, eng.admm_l1, 2, 0.1, 0.015)
        refused(E_STATE, msg, eng.admm_cnc, 2, 0.45, 0.5, 0.05, 64)
        refused(E_STATE, msg, lambda: eng.admm_l1(2, 0.1, 0.015, trace_every=1))
        if precision == 'f32':
            t = [torch.zeros((6, H, W), dtype=torch.float32, device='cuda') for _ in range(3)]
            refused(E_STATE, msg, eng.prox_l1_dual, *t, 0.1)
            refused(E_STATE, msg, eng.prox_cnc_dual, *t, 0.45, 0.5, 0.05, 64)
        eng.set_temporal(3)                                      # the same batch as two series of three
        eng.admm_l1(2, 0.1, 0.015)
        # a coil context in complex mode: the same rule at its loop and its prox
        eng.set_coils(O.M.coil_maps(C, H, W, 1))
        eng.set_image_mode('complex')
        eng.set_temporal(4)
        eng.upload(np.zeros((6, C, H, W), np.complex64), np.ones((H, W), np.uint8))
        eng.init_state()
        refused(E_STATE, msg, eng.admm_l1, 2, 0.1, 0.015)
        t = [torch.zeros((6, H, W), dtype=torch.complex128 if precision == 'f64' else torch.complex64, device='cuda') for _ in range(3)]
        refused(E_STATE, msg, eng.prox_l1_dual, *t, 0.1)
