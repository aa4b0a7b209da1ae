"""CPU tests of the parameter grid behind tests/test_gpu_param_space.py (tests/param_space_oracle.py): the committed float32 bars are what
the NumPy restatement measures now, every point populates the branches it does not switch off, and the helper's step / loop are the
oracle's own loops."""
import numpy as np
import pytest

from oracle import admm_oracle as O
import param_space_oracle as S

# Committed against re-measured bar.  A bar is the max over 4e4 .. 8e5 elements of float32 round-off, and that maximum moves with the build
# of NumPy's FFT (the butterflies are vectorised by the width of the machine's SIMD unit, which reorders the sums): by tens of per cent, not
# by factors.  A factor of 2 either way is half of the 4 x the GPU tests allow a kernel on top of a bar, so a table that has drifted cannot
# hand a kernel less than 2 x or more than 8 x the float32 distance; on the NumPy build that printed the table the ratio is 1 up to the three
# printed digits.  A bar of 0 (w+ of L1 with lambda1 = 0: u - soft(u, 0)) must be 0 again.
SPREAD = 2.0
MIN_SHARE = 0.05

POINT_IDS = [(kind, idx) for kind in ('cnc', 'l1') for idx in range(len(S.POINTS[kind]))]


def test_the_grid_holds_the_points_it_is_meant_to():
    cnc = [p for p, _ in S.CNC_POINTS]
    assert (0.45, 0.5, 0.05, 64.0) in cnc                                   # the preset
    assert {0.0, 1.0, 1.5} <= {p[0] for p in cnc}                          # alpha
    assert 0.0 in {p[1] for p in cnc}                                       # lambda1
    assert {2.75, 1e-3, 100.0} <= {p[2] for p in cnc}                      # reo: the in-function default and both ends
    assert {0.5, 1e4} <= {p[3] for p in cnc}                               # b: clip off, clip everywhere
    l1 = [p for p, _ in S.L1_POINTS]
    assert 0.0 in {p[0] for p in l1} and {1e-3, 100.0} <= {p[1] for p in l1}
    assert max(p[0] * p[1] for p in l1) >= 0.5                             # a large threshold
    for kind, idx in POINT_IDS:
        assert set(S.POINTS[kind][idx][1]) <= set(S.CLIP + S.SOFT)
    assert set(S.BARS_F32) == set(S.cases())


def test_no_point_is_more_expansive_than_the_preset():
    """z+ has the slope c1 + c3 in z inside the clip's middle branch and c1 outside it: |c1| + c3 <= the preset's 0.55 + 0.72."""
    for (alpha, lambda1, reo, b), _ in S.CNC_POINTS:
        assert abs(1 - alpha) + alpha * reo * lambda1 * b <= S.MAX_SLOPE + 1e-12, (alpha, lambda1, reo, b)
    alpha, lambda1, reo, b = S.CNC_POINTS[0][0]
    assert abs(abs(1 - alpha) + alpha * reo * lambda1 * b - S.MAX_SLOPE) <= 1e-12


def test_the_float64_oracle_is_good_for_the_bar_of_the_double_engines():
    """The double engines are held to 1e-12 x max |ref| (F64_BAR of tests/test_gpu_param_space.py) at 256 x 256 and 218 x 170.  The
    float64 oracle carries round-off of its own: the float32 restatement's distance scaled by the ratio of the unit round-offs, 2^-29.  A
    kernel in double may carry as much again, so the points are chosen to keep that estimate at or below half of the bar."""
    for (kind, idx, shape, mode), v in S.BARS_F32.items():
        if shape in ((256, 256), (218, 170)) and kind != 'switch':
            assert max(max(a) for a in v) * 2.0 ** -29 <= S.F64_BAR / 2, (kind, idx, shape, mode)


@pytest.mark.parametrize('kind,idx', POINT_IDS + [('switch', i) for i in range(len(S.SWITCHES))])
def test_committed_bars_are_what_the_restatement_measures(kind, idx):
    for k, i, shape, mode in S.cases():
        if (k, i) != (kind, idx):
            continue
        now, then = S.measure_case(k, i, shape, mode), S.BARS_F32[(k, i, shape, mode)]
        for name, a, b in zip('xzw', now, then):
            for s, (va, vb) in enumerate(zip(a, b)):
                if vb == 0.0 or va == 0.0:
                    assert va == vb, (shape, mode, name, s, va, vb)
                else:
                    assert vb / SPREAD <= va <= vb * SPREAD, (shape, mode, name, s, va, vb)


@pytest.mark.parametrize('kind,idx', POINT_IDS)
def test_every_branch_a_point_leaves_on_is_populated(kind, idx):
    """On the designed state of the teacher-forced step, counted in the float64 oracle, per slice: a branch the point does not declare off
    holds at least 5 % of the pixels; one it declares off holds less than that (the declaration is not a way around the first rule)."""
    point, off = S.params(kind, idx), S.off(kind, idx)
    for shape in S.SHAPES:
        x, _, _ = S.reference(kind, idx, shape, 'step')
        z0, w0 = S.state(S.B, *shape)
        for b in range(S.B):
            share = S.branches(kind, point, x[b], z0[b], w0[b])
            for name, v in share.items():
                if name in off:
                    assert v < MIN_SHARE, (shape, b, name, v)
                else:
                    assert v >= MIN_SHARE, (shape, b, name, v)


def test_state_and_problem_are_as_described():
    for H, W in S.SHAPES:
        z, w = S.state(S.B, H, W)
        assert z.dtype == np.float32 and w.dtype == np.float32 and z.shape == (S.B, H, W)
        a = np.abs(z)
        assert 0.9e-4 <= a.min() <= 1.2e-4 and 0.9 <= a.max() <= 1.0 and np.abs(w).max() <= 0.3
        for b in range(S.B):
            assert 0.45 <= np.mean(z[b] < 0) <= 0.55
            for lo in (1e-4, 1e-3, 1e-2, 1e-1):                              # four decades, a quarter of the pixels in each
                assert 0.2 <= np.mean((a[b] >= lo) & (a[b] < 10 * lo)) <= 0.3
            for c in range(b):
                assert not np.array_equal(z[b], z[c]) and not np.array_equal(w[b], w[c])
        y, masks, mid = S.problem(S.B, H, W)
        assert y.dtype == np.complex64 and masks.dtype == np.uint8 and masks.shape == (3, H, W)
        assert mid[0] != mid[1] and not np.array_equal(masks[mid[0]], masks[mid[1]])     # the paired slices differ in their masks
        assert S.problem(S.B, H, W)[0] is y                                  # computed once, shared
    with pytest.raises(ValueError):
        S.problem(S.B, 256, 256)[0][0, 0, 0] = 0                             # ... and left unchanged


def test_step_and_loop_are_the_oracles_loops():
    y, masks, mid = S.problem(S.B, 256, 256)
    y0, m0 = y[0].astype(np.complex128), masks[mid[0]]
    x, z, w = S.loop('cnc', (0.45, 0.5, 0.05, 64.0), y0, m0, 3)
    xr, rec = O.admm_cnc(y0, m0, 3, trace=(3,))
    assert np.array_equal(x, xr) and np.array_equal(z, rec[3][1]) and np.array_equal(w, rec[3][2])
    x, z, w = S.loop('l1', (0.1, 0.015), y0, m0, 3)
    xr, rec = O.admm_l1(y0, m0, 3, trace=(3,))
    assert np.array_equal(x, xr) and np.array_equal(z, rec[3][1]) and np.array_equal(w, rec[3][2])
    assert np.array_equal(S.loop('cnc', (0.45, 0.5, 0.05, 64.0), y0, m0, 3, np.float32)[0], O.admm_cnc_f32(y0, m0, 3))
    # a loop continued from a state is the loop; a step with x given is the prox alone
    _, z2, w2 = S.loop('cnc', (1.5, 0.5, 0.05, 64.0), y0, m0, 2)
    a = S.loop('cnc', (1.5, 0.5, 0.05, 64.0), y0, m0, 1, z=z2, w=w2)
    b = S.loop('cnc', (1.5, 0.5, 0.05, 64.0), y0, m0, 3)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    xg = np.full((256, 256), 0.25)
    _, zp, wp = S.step('l1', (5.0, 0.1), xg, z2, w2, y0, m0)
    assert np.array_equal(zp, O.soft(xg + w2, 0.5)) and np.array_equal(wp, w2 + xg - zp)


def test_the_bars_see_a_subtly_wrong_kernel():
    """What the per-element bars are for, shown on the oracle itself at 256 x 256: (1) one pixel of one array off by 1e-4 of the array's
    scale (of w+: by 1e-4) -- a whole-image rel-L2 of 2e-6 .. 5e-6, inside the 1e-5 of the loop tests -- is at least 10 x beyond the bar of every teacher-forced case; (2) an inner
    clip that treats z < -1/b like z > 1/b, (3) a threshold that is the PREVIOUS call's (the preset's, at a point next to it) and (4) a
    blend coefficient left over from the preset are beyond the bar of z+ at every point that has the branch on."""
    assert (S.FREEDOM, S.FLOOR, S.F64_BAR) == (4.0, 2e-6, 1e-12)
    shape = (256, 256)
    y, masks, mid = S.problem(S.B, *shape)
    z0, w0 = S.state(S.B, *shape)
    for kind, idx in POINT_IDS:
        key = (kind, idx, shape, 'step')
        ref = S.reference(*key)
        for k in range(3):
            bad = ref[k].copy()
            bad[1, 100, 37] += 1e-4 * (S.scale(ref[k])[1] if k < 2 else 1.0)          # w+ can be as small as thr: 1e-4 absolute
            ratio = S.distance(bad, ref[k]) / S.bar(key, k)
            assert ratio[1] >= 10 and ratio[0] == 0 and ratio[2] == 0, (key, k, ratio)
            assert k == 2 or np.linalg.norm(bad[1] - ref[k][1]) <= 5e-6 * np.linalg.norm(ref[k][1])
    for idx, ((alpha, lambda1, reo, b), _) in enumerate(S.CNC_POINTS):
        key = ('cnc', idx, shape, 'step')
        x, zp, _ = S.reference(*key)
        if 'lo' not in S.off('cnc', idx) and alpha * reo * lambda1 * b > 0:
            z64, w64 = z0[0].astype(np.float64), w0[0].astype(np.float64)
            t = (1 - alpha) * z64 + alpha * (x[0] + w64) + alpha * reo * lambda1 * b * np.clip(np.abs(z64), -1 / b, 1 / b)   # sign of z lost
            wrong = O.soft(t, alpha * reo * lambda1)
            assert (S.distance(wrong[None], zp[:1]) / S.bar(key, 1)[:1])[0] >= 20, key          # b = 1e4: c3 / b = 4.5e-5, 44 x
    for kind, idx, stale in (('cnc', 8, S.params('cnc', 0)), ('l1', 2, S.params('l1', 0))):
        key = (kind, idx, shape, 'step')
        x, zp, _ = S.reference(*key)
        point = S.params(kind, idx)
        mixed = (point[0], stale[1], stale[2], point[3]) if kind == 'cnc' else stale      # the prox scalars of the call before
        _, wrong, _ = S.step(kind, mixed, x[0], z0[0], w0[0], y[0], masks[mid[0]])
        assert (S.distance(wrong[None], zp[:1]) / S.bar(key, 1)[:1])[0] >= 100, key
        keep = (point[0], point[1], stale[2], point[3]) if kind == 'cnc' else (point[0] * point[1] / stale[1], stale[1])   # same thr, stale reo
        xw, _, _ = S.step(kind, keep, None, z0[0], w0[0], y[0], masks[mid[0]])
        assert (S.distance(xw[None], x[:1]) / S.bar(key, 0)[:1])[0] >= 100, key
