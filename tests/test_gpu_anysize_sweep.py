"""GPU sweep of the any-size path (csrc/kernels_anysize.hip): every length from 128 to 1024 once as the column length H and once
as the row length W = pair(H), 897 contexts of B = 2 (the smallest batch at which a row workgroup of G lines straddles two
slices and the last one is partial), in float and in double.  What varies with the length -- the radix sequence, Stockham or
Bluestein and its m, the lines G a workgroup holds, the LDS pitch, the partial last row group and column tile -- is all run.

  float   utils_pnp.fft2 / ifft2 of a seeded complex64 batch against np.fft of the widened input, per slice: relative L2 <= 2e-6
          (the bar of test_gpu_anysize.py) and the worst single bin <= 4 x the worst value the CPU emulation of the same float
          arithmetic reaches in two dimensions (tests/golden/anysize_sweep_bounds.json; the kernels run the emulation's fmaf
          sequence and may differ from it only where the compiler contracts a plain multiply-add and in the epilogue's scale)
  dc      one pnp_dc_step against the float64 formula, relative L2 <= 1e-5 (the project's parity bar; L2 only: the emulation has
          no data-consistency step to take a per-element figure from), on one shape at least for every (kind, m, G) on each axis
  double  the double kernels as a double context reaches them: synthesize -> download_y against fft2(img) * mask + noise, and
          upload(random y) -> init_state -> get_state against |ifft2(y)|; relative L2 <= 1e-12, per element as for float

Every case is a contiguous chunk of H."""
import numpy as np
import pytest

from oracle import admm_oracle as O
import anysize_common as AC

pytestmark = pytest.mark.gpu

B = 2
MARGIN = 4


def _chunks(Hs, k):
    """Hs in k contiguous chunks of about the same work: a shape's cost (the NumPy references mostly) grows with H * pair(H), and
    pair(H) scatters about the middle of the range, so the chunks hold about the same sum of H."""
    edges = np.searchsorted(np.cumsum(Hs), np.sum(Hs) * np.arange(1, k) / k)
    return [[int(H) for H in c] for c in np.split(np.asarray(Hs), edges)]


NCHUNK = 16                 # measured on an MI355X machine: 2.4 .. 3.2 s a float case, 3.1 .. 4.2 s a double case
CHUNKS = _chunks(list(AC.LENGTHS), NCHUNK)


def _dc_subset():
    """The first shape (in H) that brings each (kind, m, G) of a float context to the columns, and to the rows."""
    seen, out = (set(), set()), []
    for H in AC.LENGTHS:
        rows, cols = AC.shape_combos(H, AC.pair(H), False)
        if rows not in seen[0] or cols not in seen[1]:
            out.append(H)
        seen[0].add(rows)
        seen[1].add(cols)
    return out


DC_SHAPES = _dc_subset()
DC_NCHUNK = 8               # 1.2 .. 2.2 s a case
DC_CHUNKS = _chunks(DC_SHAPES, DC_NCHUNK)


@pytest.fixture(scope='module')
def env():
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib, utils_pnp
    assert _lib.device_count() >= 1 and torch.cuda.is_available()
    return dict(torch=torch, P=P, U=utils_pnp)


@pytest.fixture(scope='module')
def bounds():
    return AC.load_bounds()


def _check_context(eng, H, W):
    assert eng.ctx_path == 'anysize', (H, W, eng.ctx_path)
    for axis, n in ((0, W), (1, H)):
        p = eng.fft_plan(axis)
        assert p.startswith('stockham %d =' % n if AC.smooth7(n) else 'bluestein %d ->' % n), (H, W, axis, p)


def _check(bad, shape, op, got, ref, l2_bound, max_bound, worst):
    """Both measures of every slice; failures are collected so that one run names every shape that is wrong."""
    for b in range(B):
        l2, mx, at = AC.errors(got[b], ref[b])
        worst[op] = tuple(max(v) for v in zip(worst.get(op, (0.0, 0.0)), (l2, mx)))
        if not l2 <= l2_bound:
            bad.append('%dx%d %s slice %d: relative L2 %.3e > %.3e' % (shape + (op, b, l2, l2_bound)))
        if max_bound is not None and not mx <= max_bound:
            bad.append('%dx%d %s slice %d: bin (row %d, col %d) off by %.3e of the rms > %.3e' % (shape + (op, b) + at + (mx, max_bound)))


def _report(bad, worst):
    print('worst (relative L2, per bin) of the chunk: ' + ', '.join('%s (%.3e, %.3e)' % ((k,) + v) for k, v in sorted(worst.items())))
    assert not bad, '%d failures: %s' % (len(bad), '; '.join(bad[:12]))


def test_pairing_and_chunks_cover_every_length_and_combination():
    Hs = [H for c in CHUNKS for H in c]
    Ws = [AC.pair(H) for H in Hs]
    assert Hs == list(AC.LENGTHS) and sorted(Ws) == list(AC.LENGTHS)               # a bijection: every length on both axes
    assert not any(H in (256, 512) and W in (256, 512) for H, W in zip(Hs, Ws))    # those take the fixed-size kernels
    for f64 in (False, True):
        got = [set(), set()]
        for H, W in zip(Hs, Ws):
            rows, cols = AC.shape_combos(H, W, f64)
            got[0].add(rows)
            got[1].add(cols)
        want = {AC.combo(n, f64) for n in AC.LENGTHS}
        assert got[0] == want and got[1] == want
        assert {m for k, m, g in want if k == 'bluestein'} == {512, 1024, 2048}
    # the lines per workgroup the two precisions reach, the single double line of m = 1024 and of m = 2048 (64 KiB + 32 B of LDS) among them
    assert {AC.lines_per_wg(n, False) for n in AC.LENGTHS} == set(range(1, 17))
    assert {AC.lines_per_wg(n, True) for n in AC.LENGTHS} == set(range(1, 10))
    assert AC.combo(1021, True) == ('bluestein', 2048, 1) and AC.combo(1024, True) == ('stockham', 1024, 1)
    assert 2 * 16 * (2048 + 1) == 64 * 1024 + 32


def test_dc_subset_holds_every_combination_on_each_axis():
    assert [H for c in DC_CHUNKS for H in c] == DC_SHAPES
    shapes = [(H, AC.pair(H)) for H in DC_SHAPES]
    want = {AC.combo(n, False) for n in AC.LENGTHS}
    assert {AC.shape_combos(H, W, False)[0] for H, W in shapes} == want
    assert {AC.shape_combos(H, W, False)[1] for H, W in shapes} == want
    for axis in (0, 1):
        ns = [s[axis] for s in shapes]
        assert any(7 in AC.primes(n) and AC.smooth7(n) for n in ns)               # radix 7
        assert any(n % 2 and AC.smooth7(n) for n in ns)                           # no radix-4 or radix-2 stage at all
        assert any(n % 2 for n in ns)
        assert any(AC.stockham_length(n) == 2048 for n in ns)


@pytest.mark.parametrize('chunk', range(NCHUNK))
def test_fft2_ifft2_every_length_float(env, bounds, chunk):
    torch, P, U = env['torch'], env['P'], env['U']
    bad, worst = [], {}
    for H in CHUNKS[chunk]:
        W = AC.pair(H)
        rng = np.random.default_rng(AC.shape_seed(H, W))
        x = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))).astype(np.complex64)
        with P.Engine(H, W, Bmax=B) as eng:
            _check_context(eng, H, W)
            d = torch.from_numpy(x).cuda()
            fwd, inv = U.fft2(eng, d).cpu().numpy(), U.ifft2(eng, d).cpu().numpy()
        x64 = x.astype(np.complex128)
        _check(bad, (H, W), 'fft2', fwd, np.fft.fft2(x64), 2e-6, MARGIN * bounds['float']['fwd']['max'], worst)
        _check(bad, (H, W), 'ifft2', inv, np.fft.ifft2(x64), 2e-6, MARGIN * bounds['float']['inv']['max'], worst)
    _report(bad, worst)


@pytest.mark.parametrize('chunk', range(DC_NCHUNK))
def test_dc_step_every_combination_float(env, chunk):
    """IN_REAL_DIFF rows, MID_BLEND columns, EPI_ABS_REAL rows at lengths test_dc_step_teacher_forced (256, 512) never sees."""
    torch, P, U = env['torch'], env['P'], env['U']
    bad, worst = [], {}
    for H in DC_CHUNKS[chunk]:
        W = AC.pair(H)
        masks = np.stack([O.synthetic_mask(k, H, W) for k in ('random', 'radial')]).astype(np.uint8)
        mid = np.array([0, 1], np.int32)
        ys = np.stack([O.synthetic_problem(b, masks[mid[b]], H, W)[1] for b in range(B)]).astype(np.complex64)
        rng = np.random.default_rng(AC.shape_seed(H, W))
        z = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
        w = rng.uniform(-0.1, 0.1, (B, H, W)).astype(np.float32)
        with P.Engine(H, W, Bmax=B) as eng:
            _check_context(eng, H, W)
            eng.upload(ys, masks, mid)
            x = U.dc_solve(eng, torch.from_numpy(z).cuda(), torch.from_numpy(w).cuda(), 0.05).cpu().numpy()
        ref = [O.dc_step(z[b].astype(np.float64), w[b].astype(np.float64), ys[b].astype(np.complex128), masks[mid[b]], 0.05) for b in range(B)]
        _check(bad, (H, W), 'dc_step', x, ref, 1e-5, None, worst)
    _report(bad, worst)


@pytest.mark.parametrize('chunk', range(NCHUNK))
def test_synthesis_and_init_every_length_double(env, bounds, chunk):
    P = env['P']
    bad, worst = [], {}
    for H in CHUNKS[chunk]:
        W = AC.pair(H)
        rng = np.random.default_rng(AC.shape_seed(H, W) + 1)
        img = rng.standard_normal((B, H, W)).astype(np.float32)
        noise = 0.1 * np.sqrt(H * W) * (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W)))
        masks = (rng.uniform(size=(2, H, W)) < 0.9).astype(np.uint8)               # a tenth of the bins unsampled: noise alone
        mid = np.array([0, 1], np.int32)
        yr = rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))  # not Hermitian: ifft2 of it is complex
        with P.Engine(H, W, Bmax=B, precision='f64') as eng:
            _check_context(eng, H, W)
            eng.synthesize(img, noise, masks, mid)
            y = eng.download_y()
            eng.upload(yr, masks, mid)
            eng.init_state()
            z, w = eng.get_state()
        ref = np.fft.fft2(img.astype(np.float64)) * masks[mid] + noise
        _check(bad, (H, W), 'synthesize', y, ref, 1e-12, MARGIN * bounds['double']['fwd']['max'], worst)
        _check(bad, (H, W), 'init_state', z, np.abs(np.fft.ifft2(yr)), 1e-12, MARGIN * bounds['double']['inv']['max'], worst)
        if np.any(w):
            bad.append('%dx%d init_state: w is not zero' % (H, W))
    _report(bad, worst)
