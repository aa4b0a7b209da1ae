"""GPU tests of cycle spinning for the wavelet prox (pnp_set_spin, pnp_dwt2_shifted, the spin= keywords of ADMM_L1 / ADMM_CNC).

A shift changes addresses and nothing else, so wherever the unshifted kernels can serve as the reference the comparison is BIT FOR BIT:
the shifted transform against the existing entry point on the rolled input, the shifted prox against the existing prox on rolled copies,
the averaged prox against the composition rule built from unshifted prox calls and torch's elementwise add / multiply.  Beside that the
float64 oracle (tests/wavelet_spin_oracle.py: np.roll around tests/wavelet_oracle.py) with the bars of tests/test_gpu_wavelet.py: transform
4 x the distance of the float32 restatement from the float64 one on the same (rolled) input, 1e-12 in double; loops of 10 iterations 1e-5
in float32, 1e-10 in double.  Every figure printed before an assertion is what the card gave.

The step-wise prox (pnp_prox_l1_dual / pnp_prox_cnc_dual) exists in float32 only, so tests 2 and 3 run in float32; the double kernels are
covered by the transform (1), the schedule (4) and the loops against the oracle (5)."""
import functools
import os

import numpy as np
import pytest

import multicoil_oracle as M
import wavelet_oracle as O
import wavelet_spin_oracle as S
from conftest import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = ((128, 128), (128, 160), (256, 192))
FREEDOM = 4.0            # order of the sums (tests/test_gpu_wavelet.py)
F64_BAR = 1e-12
AX = (-2, -1)


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', 0))


def _dummy_problem(eng, B):
    eng.upload(np.zeros((B, eng.H, eng.W), np.complex64), np.ones((eng.H, eng.W), np.uint8))


def _rin(torch, t, s):
    return torch.roll(t, (-s[0], -s[1]), AX).contiguous()


def _rout(torch, t, s):
    return torch.roll(t, (s[0], s[1]), AX).contiguous()


# ---- 1. the shifted transform ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('H,W', SHAPES)
def test_shifted_transform_is_the_transform_of_the_rolled_input(P, torch, H, W, name, precision):
    """dwt2(x, shift=s) equals dwt2(roll(x, -s)) of the existing entry point and idwt2(c, shift=s) equals roll(idwt2(c), +s), bit for bit, at
    L = 1 and the largest valid L (128 x 128, db4, L = 4: the halo goes once round the image) for the five shifts -- with a spin setting in
    place, which the unshifted entry points must ignore; in place equals out of place; Psi_s against the float64 oracle."""
    from pnp_admm_cnc_mri_amd import utils_pnp as U
    v = O.field(H, W)
    B = len(v)
    real = np.float64 if precision == 'f64' else np.float32
    with P.Engine(H, W, Bmax=B, precision=precision) as eng:
        vt = _dev(torch, v.astype(real))
        for L in O.gpu_levels(name, H, W):
            eng.set_sparsity(name, L)
            eng.set_spin([(1, 1)])                                      # pnp_dwt2_fwd / _inv stay unshifted whatever the setting
            ct = U.dwt2(eng, vt)
            plain_back = U.idwt2(eng, ct)
            for s in S.shifts_of(L):
                got = U.dwt2(eng, vt, shift=s)
                assert torch.equal(got, U.dwt2(eng, _rin(torch, vt, s))), (L, s)
                back = U.idwt2(eng, ct, shift=s)
                assert torch.equal(back, _rout(torch, plain_back, s)), (L, s)
                if s != (0, 0):
                    assert not torch.equal(got, ct), (L, s)
                for inverse, src, ref in ((0, vt, got), (1, ct, back)):
                    t = src.clone()
                    (eng.idwt2 if inverse else eng.dwt2)(t, t, B, s)
                    eng.sync()
                    assert torch.equal(t, ref), (L, s, inverse)
                want = S.fwd(v, name, L, s)
                bar = F64_BAR if precision == 'f64' else FREEDOM * rel_l2(S.fwd(v, name, L, s, np.float32), want)
                err = rel_l2(got.cpu().numpy(), want)
                print('dwt2 %dx%d %s L=%d %s shift %s: rel-L2 Psi_s %.2e (bar %.2e)' % (H, W, name, L, precision, s, err, bar))
                assert got.dtype == vt.dtype and err <= bar, (L, s, err, bar)
            m = 1 << L
            for bad in ((m, 0), (0, m), (-1, 0)):
                with pytest.raises(P._lib.PnpError) as e:
                    U.dwt2(eng, vt, shift=bad)
                assert e.value.code == -1 and 'range' in str(e.value)          # PNP_E_ARG


# ---- 2. / 3. one prox step ------------------------------------------------------------------------------------------------------------

PROX_CASES = tuple(c for c in O.PROX_CASES if c[2:] in SHAPES)          # db4 L=4 128x128, db2 L=3 128x160, haar L=4 256x192


def _prox(eng, kind, xt, zt, wt):
    if kind == 'l1':
        eng.prox_l1_dual(xt, zt, wt, O.PROX_L1_THR)
    else:
        p = O.PROX_CNC
        eng.prox_cnc_dual(xt, zt, wt, p['alpha'], p['lambda1'], p['reo'], p['b'])


def _unshifted_in_frame(torch, eng, kind, x, z, w, s):
    """the existing prox on rolled copies, rolled back -> (z+, w+); the engine has no spin setting"""
    xs, zs, ws = (_rin(torch, t, s) for t in (x, z, w))
    _prox(eng, kind, xs, zs, ws)
    eng.sync()
    return _rout(torch, zs, s), _rout(torch, ws, s)


@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('name,L,H,W', PROX_CASES)
def test_shifted_prox_is_the_prox_of_the_rolled_state(P, torch, name, L, H, W, kind):
    """K = 1: z+ and w+ of a prox in the frame of shift s are bit-equal to: clear the spin, run the existing prox on copies rolled by -s, roll
    back.  B = 3, both branches of soft and clip populated (wavelet_oracle.prox_inputs)."""
    x, z, w = (_dev(torch, a) for a in O.prox_inputs(H, W))
    with P.Engine(H, W, Bmax=len(x)) as eng:
        _dummy_problem(eng, len(x))
        eng.set_sparsity(name, L)
        plain = None
        for s in S.shifts_of(L):
            eng.set_spin(None)
            want = _unshifted_in_frame(torch, eng, kind, x, z, w, s)
            eng.set_spin([s])
            zt, wt = z.clone(), w.clone()
            _prox(eng, kind, x, zt, wt)
            eng.sync()
            assert eng.spin_cursor == 1
            assert torch.equal(zt, want[0]) and torch.equal(wt, want[1]), s
            if s == (0, 0):
                plain = zt
            else:
                assert not torch.equal(zt, plain), s


@pytest.mark.parametrize('K', [2, 3, 4])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('name,L,H,W', PROX_CASES)
def test_averaged_prox_follows_the_composition_rule(P, torch, name, L, H, W, kind, K):
    """K shifts per prox: bit-equal to acc = z_0; acc = acc + z_j, j = 1 .. K - 2; z+ = (acc + z_(K-1)) * r with r = 1 / K rounded once to
    float32; w+ = (x + w) - z+ -- the z_j from K existing unshifted prox calls on rolled copies, the sums and the product by torch.  x, z
    and w are read by every shift and written by the last alone: the second group of the table starts from the same state."""
    x, z, w = (_dev(torch, a) for a in O.prox_inputs(H, W))
    shifts = list(S.shifts_of(L))
    table = shifts[5 - K:] + shifts[:K]                                  # two groups of K, different sets of shifts
    r = torch.tensor(1.0 / K, dtype=torch.float32, device=x.device)
    with P.Engine(H, W, Bmax=len(x)) as eng:
        _dummy_problem(eng, len(x))
        eng.set_sparsity(name, L)
        want = []
        for g in (table[:K], table[K:]):
            zs = [_unshifted_in_frame(torch, eng, kind, x, z, w, s)[0] for s in g]
            acc = zs[0]
            for j in range(1, K - 1):
                acc = acc + zs[j]
            zn = (acc + zs[K - 1]) * r
            want.append((zn, (x + w) - zn))
        eng.set_spin(table, K)
        assert eng.spin == {'n': 2 * K, 'per_prox': K}
        for step, (zn, wn) in enumerate(want):
            zt, wt = z.clone(), w.clone()
            _prox(eng, kind, x, zt, wt)
            eng.sync()
            assert eng.spin_cursor == step + 1
            assert zn.dtype == torch.float32 and torch.equal(zt, zn) and torch.equal(wt, wn), step
        assert not torch.equal(want[0][0], want[1][0])


# ---- 4. schedule and cursor -----------------------------------------------------------------------------------------------------------

def _params(P, kind):
    p = dict(P.solvers.PRESETS['ADMM_L1' if kind == 'l1' else 'ADMM_CNC'])
    p.pop('iter_num')
    return p


def _run(eng, kind, p, iters, **kw):
    if kind == 'l1':
        return eng.admm_l1(iters, p['lambda1'], p['reo'], **kw)
    return eng.admm_cnc(iters, p['alpha'], p['lambda1'], p['reo'], p['b'], **kw)


@functools.lru_cache(maxsize=None)
def _problem(H, W, B=2):
    return O.problem(B, H, W)


def _all(eng):
    return (eng.x(), *eng.get_state())


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_schedule_and_cursor(P, kind, precision):
    """128 x 160 (partial 64-tiles), db2, L = 3, a table of five shifts and a run of seven iterations, so the table wraps: 3 + 4 in two calls
    equal 7 in one; init_state rewinds the cursor, set_state leaves it, spin_cursor = 3 after set_state reproduces the tail; the traced run
    ends bit-equal; an all-zero table equals no spin; plan() reports 3 + 2 K launches; set_sparsity clears the setting."""
    H, W, L = 128, 160, 3
    y, mask, _ = _problem(H, W)
    p = _params(P, kind)
    table = list(S.shifts_of(L))
    with P.Engine(H, W, Bmax=2, precision=precision) as eng:
        eng.upload(y, mask)
        eng.set_sparsity('db2', L)
        assert eng.spin == {'n': 0, 'per_prox': 1} and eng.plan['launches_per_iteration'] == 5
        eng.init_state()
        _run(eng, kind, p, 7)
        none = _all(eng)
        for K in (1, 2):
            tab = table if K == 1 else table + table[:1]                # 5 groups of one, 3 groups of two
            eng.set_spin(tab, K)
            assert eng.spin == {'n': len(tab), 'per_prox': K} and eng.spin_cursor == 0
            assert eng.plan['launches_per_iteration'] == 3 + 2 * K == eng.kernels_per_iteration
            eng.init_state()
            _run(eng, kind, p, 7)
            ref = _all(eng)
            assert eng.spin_cursor == 7 and not _same(ref, none)
            eng.init_state()
            assert eng.spin_cursor == 0                                  # init_state rewinds
            _run(eng, kind, p, 3)
            z3, w3 = eng.get_state()
            eng.set_state(z3, w3)
            assert eng.spin_cursor == 3                                  # set_state does not
            _run(eng, kind, p, 4)
            assert _same(_all(eng), ref), K
            eng.set_spin(tab, K)                                         # rewinds too
            assert eng.spin_cursor == 0
            eng.set_state(z3, w3)
            eng.spin_cursor = 3
            _run(eng, kind, p, 4)
            assert _same(_all(eng), ref) and eng.spin_cursor == 7, K
            eng.set_state(z3, w3)
            eng.spin_cursor = 3 + 5 * len(tab) // K                      # the same groups, whole turns of the table later
            _run(eng, kind, p, 4)
            assert _same(_all(eng), ref), K
            eng.init_state()
            tr = _run(eng, kind, p, 7, trace_every=1)
            assert tr['iters_done'] == 7 and eng.spin_cursor == 7 and _same(_all(eng), ref), K
        for K in (3, 4):
            eng.set_spin(table[:4] * 3, K)
            assert eng.plan['launches_per_iteration'] == 3 + 2 * K == eng.kernels_per_iteration
        eng.set_spin([(0, 0)] * 3, 1)
        eng.init_state()
        _run(eng, kind, p, 7)
        assert _same(_all(eng), none)                                    # the zero shift is no shift
        with pytest.raises(P._lib.PnpError) as e:
            eng.spin_cursor = -1
        assert e.value.code == -1
        eng.set_spin(None)
        assert eng.spin == {'n': 0, 'per_prox': 1} and eng.plan['launches_per_iteration'] == 5
        eng.init_state()
        _run(eng, kind, p, 7)
        assert _same(_all(eng), none)
        with pytest.raises(P._lib.PnpError) as e:
            eng.spin_cursor = 1
        assert e.value.code == -3                                        # PNP_E_STATE: nothing to move
        eng.set_spin(table, 1)
        eng.set_sparsity('db2', 2)                                       # the valid range depends on L: the setting goes
        assert eng.spin == {'n': 0, 'per_prox': 1}
        with pytest.raises(ValueError, match='range'):
            eng.set_spin(table, 1)                                       # (7, 7) is no shift at L = 2
        eng.set_sparsity(None)
        with pytest.raises(P._lib.PnpError) as e:
            eng.set_spin([(0, 0)])
        assert e.value.code == -3                                        # PNP_E_STATE: no wavelet


def test_coil_context_follows_the_schedule(P, torch):
    """C = 2, 128 x 128, cg_iters = 3, db2, L = 2, two averaged shifts per prox: 5 + 5 cg_iters + 2 K launches per iteration, and two
    iterations of ADMM_L1 bit-equal to the same composition of dc_step and step-wise unshifted prox calls on rolled copies."""
    H, W, C, K, L, iters = 128, 128, 2, 2, 2, 2
    _, Sm, m, _, y0 = M.problem(0, C, H, W)
    y1 = M.synthesize(M.phantom(1, H, W), Sm, m, M.noise(1, C, m))
    y = np.stack([y0, y1])
    p = _params(P, 'l1')
    table = [(1, 0), (3, 1), (0, 1), (3, 3)]
    r = torch.tensor(1.0 / K, dtype=torch.float32, device=torch.device('cuda', 0))
    with P.Engine(H, W, Bmax=2) as eng:
        eng.set_coils(Sm, 3)
        eng.upload(y, m)
        eng.set_sparsity('db2', L)
        assert eng.plan['launches_per_iteration'] == 5 + 5 * 3 + 2
        eng.set_spin(table, K)
        assert eng.plan['launches_per_iteration'] == 5 + 5 * 3 + 2 * K == eng.kernels_per_iteration
        eng.init_state()
        z, w = (_dev(torch, a) for a in eng.get_state())
        _run(eng, 'l1', p, iters)
        got = _all(eng)
        assert eng.spin_cursor == iters
        eng.set_spin(None)
        x = torch.empty_like(z)
        for i in range(iters):
            eng.dc_step(z, w, x, p['reo'])
            zs = []
            for s in S.group(table, K, i):
                xs, zr, wr = (_rin(torch, t, s) for t in (x, z, w))
                eng.prox_l1_dual(xs, zr, wr, p['reo'] * p['lambda1'])
                eng.sync()
                zs.append(_rout(torch, zr, s))
            zn = (zs[0] + zs[1]) * r
            z, w = zn, (x + w) - zn
        assert _same(got, (x.cpu().numpy(), z.cpu().numpy(), w.cpu().numpy()))


# ---- 5. whole loops against the oracle ----------------------------------------------------------------------------------------------

ITERS, LEVELS = 10, 3


@functools.lru_cache(maxsize=None)
def _loop_reference(kind, name, K, params):
    from pnp_admm_cnc_mri_amd.engine import spin_table
    y, mask, _ = _problem(128, 128)
    return S.loop(y, mask, ITERS, kind, dict(params), name, LEVELS, spin_table('random', LEVELS, ITERS, K, 0), K)[0]


@pytest.mark.parametrize('precision', ['f32', 'f64'])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('name', O.NAMES)
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_spun_loops_against_the_oracle(P, kind, name, K, precision):
    """10 iterations at the presets, 128 x 128, L = 3, spin='random' with one and with three averaged shifts per prox: rel-L2 of x against
    the float64 rolled-oracle loop <= 1e-5 in float32 (the float32 restatement on these inputs: 1.1 - 1.8e-6), <= 1e-10 in double."""
    from pnp_admm_cnc_mri_amd.engine import spin_table
    y, mask, _ = _problem(128, 128)
    p = _params(P, kind)
    want = _loop_reference(kind, name, K, tuple(sorted(p.items())))
    with P.Engine(128, 128, Bmax=2, precision=precision) as eng:
        eng.upload(y, mask)
        eng.set_sparsity(name, LEVELS)
        eng.set_spin(spin_table('random', LEVELS, ITERS, K, 0), K)
        eng.init_state()
        _run(eng, kind, p, ITERS)
        err = rel_l2(eng.x(), want)
    print('spun loop %s %s K=%d %s: rel-L2 of x after %d iterations %.3e' % (kind, name, K, precision, ITERS, err))
    assert err <= (1e-10 if precision == 'f64' else 1e-5), err


# ---- 6. the point of the feature --------------------------------------------------------------------------------------------------------

def test_spinning_lifts_the_psnr_as_the_oracle_says(P, tmp_path):
    """ADMM_L1, haar, L = 3, lambda1 = 0.2, reo = 0.05, 50 iterations on a piecewise-constant phantom behind a 30 % mask with noise
    (wavelet_spin_oracle.point_problem), spin_seed = 99.  (a) The inputs show the effect in the float64 oracle: one random shift per
    iteration gains at least 2 dB over none (measured +3.12 dB: 25.77 -> 28.88), four averaged shifts are no worse than one (measured
    +0.65 dB: 29.53).  (b) The card's PSNR for none / random / averaged-4 is within 0.05 dB of the oracle's (PSNR, not rel-L2, at this
    length: the float32 restatement agrees to 0.001 dB).  The log names the table."""
    from pnp_admm_cnc_mri_amd.engine import spin_table
    img, y, mask = S.point_problem()
    c = S.POINT
    opts = dict(iter_num=c['iters'], **c['params'])
    oracle, card = {}, {}
    for label, spin, K in (('none', None, 1), ('random', 'random', 1), ('averaged-4', 'random', 4)):
        table = spin_table(spin, c['levels'], c['iters'], K, c['seed'])
        oracle[label] = S.psnr(S.loop(y, mask, c['iters'], 'l1', c['params'], c['name'], c['levels'], table, K)[0][0], img)
        kw = dict(results=str(tmp_path), testset_name='spin', save_E=True) if label == 'random' else {}
        out = P.ADMM_L1(mask, None, y=y, transform=c['name'], levels=c['levels'], spin=spin, spin_average=K, spin_seed=c['seed'], **kw, **opts)
        card[label] = S.psnr(out[0], img)
        print('point %-10s: oracle %.3f dB, card %.3f dB' % (label, oracle[label], card[label]))
    assert oracle['random'] >= oracle['none'] + 2.0 and oracle['averaged-4'] >= oracle['random'], oracle
    for label in oracle:
        assert abs(card[label] - oracle[label]) <= 0.05, (label, card[label], oracle[label])
    log = open(os.path.join(str(tmp_path), 'spin_dn_ADMM_L1', 'spin_dn_ADMM_L1.log')).read()
    assert 'sparsity transform: haar, 3 levels' in log and 'cycle spinning: 50 shifts, 1 averaged per prox' in log
