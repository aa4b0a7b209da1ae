"""The parameter grid of the ADMM_L1 / ADMM_CNC loops and its float64 / float32 references -- TEST INFRASTRUCTURE, no GPU.

Every loop test before this one ran the z / w update at one point per solver, (alpha, lambda1, reo, b) = (0.45, 0.5, 0.05, 64) and
(lambda1, reo) = (0.1, 0.015), on natural images (z >= 0, so the z < -1/b side of the inner clip is never taken), and compared whole-image
norms.  This module holds what tests/test_param_space_host.py and tests/test_gpu_param_space.py share:

  CNC_POINTS / L1_POINTS   the points, each with the branches it switches off BY DESIGN ('lo', 'mid', 'hi': the inner clip z < -1/b,
                           |z| <= 1/b, z > 1/b; 'zero', 'pass': the outer soft threshold |t| <= thr, |t| > thr)
  state(B, H, W)           z of both signs with |z| spread over four decades (1e-4 .. 1), w in [-0.3, 0.3]: the designed state of
                           the teacher-forced step, on which every branch a point leaves on holds a real share of the pixels
  problem(B, H, W)         masks and measurements; y holds float32 values, so that the float engines, the double engines and the
                           oracle all start from the same numbers
  step / loop              one iteration from a given state / `iters` iterations from init_state, written on oracle.admm_oracle's
                           dc_step, l1_step and cnc_step, in float64 or -- the same NumPy lines on float32 / complex64 arrays -- float32
  measure_bars()           for every (kind, point, shape, step | loop): max |float32 - float64| per array (x, z+, w+) and per slice over
                           max |float64| of that array and slice.  `python tests/param_space_oracle.py` prints the table that is committed
                           below as BARS_F32.  It is measured against the float64 reference and NEVER against a kernel: the GPU tests
                           allow a kernel 4 x this distance (another order of the sums), with a floor of 2e-6.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import admm_oracle as O                                         # noqa: E402

B = 3                                       # odd: the last pair of the paired engines is half empty
SHAPES = ((256, 256), (512, 512), (218, 170))
LOOP_ITERS = 5
CLIP = ('lo', 'mid', 'hi')
SOFT = ('zero', 'pass')

# (alpha, lambda1, reo, b), branches off by design.  The issue of this grid fixes one coordinate per point; the others are chosen so that
#   * the clip stays two-sided and the threshold sits inside the data wherever the fixed coordinate allows it, and
#   * the map is no more expansive than the committed preset: in the clip's middle branch z+ has the slope c1 + c3 in z, and
#     |c1| + c3 <= 0.55 + 0.72 (MAX_SLOPE).  Five iterations then carry round-off, not amplified round-off, and the float64 oracle's own
#     round-off stays under the fixed bar of the double engines (tests/test_param_space_host.py checks both).
MAX_SLOPE = 1.27
CNC_POINTS = (
    ((0.45, 0.5, 0.05, 64.0), ()),                       # 0  the committed preset (S4:176): thr = 0.01125, c3 = 0.72
    ((0.4, 0.04, 2.75, 8.0), ()),                        # 1  the in-function defaults alpha, lambda1, reo (S4:38-40); b = 8 keeps the clip two-sided
    ((0.0, 0.5, 0.05, 64.0), ('zero',)),                 # 2  alpha = 0: thr = 0, c2 = c3 = 0, t = z
    ((1.0, 0.5, 0.05, 16.0), ()),                        # 3  alpha = 1: c1 = 0; thr = 0.025, c3 = 0.4
    ((1.5, 2.0, 0.05, 4.0), ()),                         # 4  alpha = 1.5: c1 = -0.5; thr = 0.15, c3 = 0.6
    ((0.45, 0.0, 0.05, 64.0), ('zero',)),                # 5  lambda1 = 0: thr = 0 (med3(a, -0, 0)), c3 = 0
    ((0.45, 0.5, 0.05, 0.5), ('lo', 'hi')),              # 6  b = 0.5: 1/b = 2 > |z|, the clip never acts
    ((0.45, 0.002, 0.05, 1e4), ('mid', 'zero')),         # 7  b = 1e4: 1/b = 1e-4 <= |z|, the clip acts everywhere; c3 = thr b = 0.45, thr = 4.5e-5
    ((0.45, 50.0, 1e-3, 32.0), ()),                      # 8  reo = 1e-3: La2 = 500, the blend keeps x^; lambda1 scaled to thr = 0.0225, c3 = 0.72
    ((0.45, 0.002, 100.0, 8.0), ()),                     # 9  reo = 100: La2 = 0.005, the blend keeps y; lambda1 scaled to thr = 0.09, c3 = 0.72
)
# (lambda1, reo), branches off by design (L1 has no inner clip)
L1_POINTS = (
    ((0.1, 0.015), ('zero',)),                           # 0  the committed preset (S1:171): thr = 1.5e-3 is below the data
    ((0.0, 0.015), ('zero',)),                           # 1  lambda1 = 0: thr = 0, z+ = x + w, w+ = 0
    ((5.0, 0.1), ()),                                    # 2  a large threshold, thr = 0.5
    ((100.0, 1e-3), ()),                                 # 3  reo = 1e-3, thr = 0.1
    ((0.002, 100.0), ()),                                # 4  reo = 100, thr = 0.2
)
POINTS = {'cnc': CNC_POINTS, 'l1': L1_POINTS}
# parameters changed between two calls on one context: SWITCH_K[0] iterations at the first point from init_state, then SWITCH_K[1] at the
# second -- L1 -> L1 with another threshold, CNC -> CNC with every scalar changed, and both changes of solver
SWITCHES = ((('l1', 2), ('l1', 4)), (('cnc', 4), ('cnc', 9)), (('l1', 3), ('cnc', 1)), (('cnc', 0), ('l1', 2)))
SWITCH_K = (2, 3)
SWITCH_SHAPES = ((256, 256), (512, 512))


def params(kind, idx):
    return POINTS[kind][idx][0]


def off(kind, idx):
    """the branches point `idx` switches off by design; an L1 point has no clip at all"""
    return frozenset(POINTS[kind][idx][1]) | (frozenset(CLIP) if kind == 'l1' else frozenset())


def state(B, H, W):
    """-> (z, w) float32 [B, H, W]: z = +-10^U(-4, 0), w = U(-0.3, 0.3); seeded by the shape, every slice different."""
    rng = np.random.default_rng(31 * H + W)
    z = np.where(rng.uniform(size=(B, H, W)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-4.0, 0.0, size=(B, H, W))
    w = rng.uniform(-0.3, 0.3, size=(B, H, W))
    return z.astype(np.float32), w.astype(np.float32)


_PROBLEMS = {}


def problem(B, H, W):
    """-> (y complex64 [B, H, W], masks uint8 [3, H, W], mask_id int32 [B]).  256 x 256: the reference's three masks, random / cartesian /
    radial, so that the paired slices 0 and 1 have different masks; other sizes: oracle.admm_oracle.synthetic_mask.  Read-only, shared."""
    key = (B, H, W)
    if key not in _PROBLEMS:
        if (H, W) == (256, 256):
            from pnp_admm_cnc_mri_amd import synthetic as S
            m = S.reference_masks()
            masks = np.stack([m['Q_Random30'], m['Q_Cartesian30'], m['Q_Radial30']]).astype(np.uint8)
        else:
            masks = np.stack([O.synthetic_mask(k, H, W) for k in ('random', 'cartesian', 'radial')])
        mid = (np.arange(B) % 3).astype(np.int32)
        y = np.stack([O.synthetic_problem(b, masks[mid[b]], H, W)[1] for b in range(B)]).astype(np.complex64)
        for a in (y, masks, mid):
            a.setflags(write=False)
        _PROBLEMS[key] = (y, masks, mid)
    return _PROBLEMS[key]


def _prox(kind, point, x, z, w):
    if kind == 'cnc':
        alpha, lambda1, reo, b = point
        return O.cnc_step(x, z, w, alpha, lambda1, reo, b)
    lambda1, reo = point
    return O.l1_step(x, z, w, lambda1, reo)


def step(kind, point, x, z, w, y, mask, dtype=np.float64):
    """One iteration on ONE slice from the state (z, w): x = dc_step(z, w) when x is None (else the given x: the prox alone), then the
    z / w update.  dtype=np.float32 runs the same lines on float32 / complex64 arrays.  -> (x, z+, w+)."""
    cplx = np.complex64 if dtype == np.float32 else np.complex128
    z, w, y = np.asarray(z, dtype), np.asarray(w, dtype), np.asarray(y, cplx)
    reo = point[2] if kind == 'cnc' else point[1]
    x = O.dc_step(z, w, y, mask, reo) if x is None else np.asarray(x, dtype)
    z, w = _prox(kind, point, x, z, w)
    assert x.dtype == dtype and z.dtype == dtype and w.dtype == dtype
    return x, z, w


def loop(kind, point, y, mask, iters, dtype=np.float64, z=None, w=None):
    """`iters` iterations on ONE slice from init_state(y) -- or from (z, w) when given.  -> (x, z, w)."""
    cplx = np.complex64 if dtype == np.float32 else np.complex128
    y = np.asarray(y, cplx)
    if z is None:
        x, z, w = O.init_state(y, dtype)
    else:
        x, z, w = None, np.asarray(z, dtype), np.asarray(w, dtype)
    for _ in range(iters):
        x, z, w = step(kind, point, None, z, w, y, mask, dtype)
    return x, z, w


def branches(kind, point, x, z, w):
    """Share of the pixels of one slice in each branch of the update from (x, z, w), in float64: {'lo', 'mid', 'hi', 'zero', 'pass'}."""
    x, z, w = (np.asarray(a, np.float64) for a in (x, z, w))
    if kind == 'cnc':
        alpha, lambda1, reo, b = point
        t = (1 - alpha) * z + alpha * (x + w) + alpha * reo * lambda1 * b * (z - O.soft(z, 1 / b))
        thr = alpha * reo * lambda1
        out = {'lo': np.mean(z < -1 / b), 'mid': np.mean(np.abs(z) <= 1 / b), 'hi': np.mean(z > 1 / b)}
    else:
        lambda1, reo = point
        t, thr, out = x + w, reo * lambda1, {}
    out.update(zero=np.mean(np.abs(t) <= thr), **{'pass': np.mean(np.abs(t) > thr)})
    return {k: float(v) for k, v in out.items()}


_REFS = {}


def reference(kind, idx, shape, mode, dtype=np.float64):
    """(x, z, w), each [B, H, W], of case (kind, point idx, shape, 'step' | 'loop'): the teacher-forced step from state(), or LOOP_ITERS
    iterations from init_state; kind 'switch': the two calls of SWITCHES[idx].  Computed once per process and shared; read-only."""
    key = (kind, idx, shape, mode, np.dtype(dtype).name)
    if key not in _REFS:
        H, W = shape
        y, masks, mid = problem(B, H, W)
        point = params(kind, idx) if kind != 'switch' else None
        if kind == 'switch':
            (ka, ia), (kb, ib) = SWITCHES[idx]
            per = []
            for b in range(B):
                _, z1, w1 = loop(ka, params(ka, ia), y[b], masks[mid[b]], SWITCH_K[0], dtype)
                per.append(loop(kb, params(kb, ib), y[b], masks[mid[b]], SWITCH_K[1], dtype, z1, w1))
        elif mode == 'step':
            z0, w0 = state(B, H, W)
            per = [step(kind, point, None, z0[b], w0[b], y[b], masks[mid[b]], dtype) for b in range(B)]
        else:
            per = [loop(kind, point, y[b], masks[mid[b]], LOOP_ITERS, dtype) for b in range(B)]
        out = tuple(np.stack([p[k] for p in per]) for k in range(3))
        for a in out:
            a.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def scale(ref):
    """max |ref| per slice, [B]; 1 where a reference array is zero throughout (w+ of lambda1 = 0 in L1: u - soft(u, 0) = 0 exactly), so
    that the distance is an absolute one there."""
    s = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1)
    return np.where(s > 0, s, 1.0)


def distance(got, ref):
    """max |got - ref| / max |ref|, per slice: [B]"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).reshape(ref.shape[0], -1).max(axis=1)
    return d / scale(ref)


# the bars of tests/test_gpu_param_space.py
FREEDOM = 4.0            # another order of the sums (tests/test_gpu_wavelet.py FREEDOM, tests/test_gpu_anysize_sweep.py MARGIN)
FLOOR = 2e-6             # what the suite holds one dc_step to
F64_BAR = 1e-12          # tests/test_gpu_wavelet.py F64_BAR


def bar(key, k, f64=False):
    """The bar of array k (0, 1, 2: x, z+, w+) of case `key`, per slice [B], as a multiple of max |ref|: float engines FREEDOM x the
    committed float32 distance with the floor FLOOR, double engines F64_BAR."""
    if f64:
        return np.full(B, F64_BAR)
    return np.maximum(FREEDOM * np.asarray(BARS_F32[key][k]), FLOOR)


def cases():
    for kind in ('cnc', 'l1'):
        for idx in range(len(POINTS[kind])):
            for shape in SHAPES:
                for mode in ('step', 'loop'):
                    yield kind, idx, shape, mode
    for idx in range(len(SWITCHES)):
        for shape in SWITCH_SHAPES:
            yield 'switch', idx, shape, 'loop'


def measure_case(kind, idx, shape, mode):
    """-> ((x per slice), (z+ per slice), (w+ per slice)): the float32 restatement's distance from the float64 one"""
    r64 = reference(kind, idx, shape, mode)
    r32 = reference(kind, idx, shape, mode, np.float32)
    return tuple(tuple(float(v) for v in distance(a, b)) for a, b in zip(r32, r64))


def measure_bars(out=sys.stdout):
    """Prints BARS_F32 as committed below and returns it."""
    bars = {}
    print('BARS_F32 = {   # (kind, point, (H, W), mode): ((x per slice), (z+ per slice), (w+ per slice))', file=out)
    for kind, idx, shape, mode in cases():
        v = measure_case(kind, idx, shape, mode)
        bars[(kind, idx, shape, mode)] = v
        print('    (%r, %d, %r, %r): (%s),' % (kind, idx, shape, mode, ', '.join('(' + ', '.join('%.2e' % e for e in a) + ')' for a in v)),
              file=out)
    print('}', file=out)
    return bars


# ---- the table `python tests/param_space_oracle.py` prints -----------------------------------------------------------------------------
BARS_F32 = {   # (kind, point, (H, W), mode): ((x per slice), (z+ per slice), (w+ per slice))
    ('cnc', 0, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (1.79e-07, 1.63e-07, 1.68e-07), (1.34e-07, 1.56e-07, 1.70e-07)),
    ('cnc', 0, (256, 256), 'loop'): ((1.32e-06, 1.34e-06, 1.12e-06), (1.65e-06, 1.59e-06, 1.40e-06), (5.30e-05, 5.34e-05, 4.25e-05)),
    ('cnc', 0, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (1.71e-07, 1.72e-07, 1.73e-07), (1.55e-07, 1.66e-07, 1.56e-07)),
    ('cnc', 0, (512, 512), 'loop'): ((1.97e-06, 2.32e-06, 1.94e-06), (2.04e-06, 2.12e-06, 2.08e-06), (1.05e-04, 1.02e-04, 8.84e-05)),
    ('cnc', 0, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (1.74e-07, 1.64e-07, 1.89e-07), (1.59e-07, 1.67e-07, 1.38e-07)),
    ('cnc', 0, (218, 170), 'loop'): ((1.23e-06, 1.13e-06, 9.52e-07), (1.15e-06, 1.03e-06, 1.74e-06), (6.85e-05, 6.12e-05, 4.87e-05)),
    ('cnc', 1, (256, 256), 'step'): ((1.65e-07, 1.91e-07, 1.62e-07), (1.30e-07, 1.36e-07, 1.46e-07), (1.81e-07, 1.96e-07, 1.98e-07)),
    ('cnc', 1, (256, 256), 'loop'): ((1.01e-06, 1.12e-06, 1.00e-06), (1.08e-06, 1.01e-06, 8.39e-07), (1.56e-05, 1.42e-05, 1.50e-05)),
    ('cnc', 1, (512, 512), 'step'): ((1.77e-07, 2.11e-07, 1.86e-07), (1.42e-07, 1.69e-07, 1.57e-07), (2.00e-07, 2.13e-07, 2.00e-07)),
    ('cnc', 1, (512, 512), 'loop'): ((1.41e-06, 1.45e-06, 1.54e-06), (1.36e-06, 1.78e-06, 1.34e-06), (2.02e-05, 2.05e-05, 2.08e-05)),
    ('cnc', 1, (218, 170), 'step'): ((3.34e-07, 2.99e-07, 2.69e-07), (1.88e-07, 1.98e-07, 1.65e-07), (3.76e-07, 2.67e-07, 2.61e-07)),
    ('cnc', 1, (218, 170), 'loop'): ((8.67e-07, 1.27e-06, 1.45e-06), (1.30e-06, 8.24e-07, 1.28e-06), (1.04e-05, 1.88e-05, 2.00e-05)),
    ('cnc', 2, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (0.00e+00, 0.00e+00, 0.00e+00), (1.28e-07, 1.44e-07, 1.43e-07)),
    ('cnc', 2, (256, 256), 'loop'): ((3.75e-06, 2.46e-06, 3.19e-06), (2.51e-07, 3.14e-07, 2.87e-07), (5.36e-05, 3.87e-05, 3.63e-05)),
    ('cnc', 2, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (0.00e+00, 0.00e+00, 0.00e+00), (1.36e-07, 1.40e-07, 1.81e-07)),
    ('cnc', 2, (512, 512), 'loop'): ((2.43e-06, 3.36e-06, 3.75e-06), (3.95e-07, 3.36e-07, 3.52e-07), (3.99e-05, 5.84e-05, 6.43e-05)),
    ('cnc', 2, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (0.00e+00, 0.00e+00, 0.00e+00), (1.54e-07, 1.44e-07, 1.38e-07)),
    ('cnc', 2, (218, 170), 'loop'): ((1.43e-06, 1.67e-06, 4.30e-06), (4.05e-07, 4.06e-07, 4.82e-07), (1.59e-05, 2.15e-05, 3.46e-05)),
    ('cnc', 3, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (1.69e-07, 1.57e-07, 1.72e-07), (3.05e-06, 3.24e-06, 3.38e-06)),
    ('cnc', 3, (256, 256), 'loop'): ((1.16e-06, 1.90e-06, 1.25e-06), (1.96e-06, 2.16e-06, 2.46e-06), (8.25e-05, 6.35e-05, 4.99e-05)),
    ('cnc', 3, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (1.84e-07, 2.13e-07, 2.52e-07), (3.21e-06, 3.46e-06, 3.04e-06)),
    ('cnc', 3, (512, 512), 'loop'): ((2.55e-06, 2.32e-06, 1.92e-06), (3.91e-06, 4.28e-06, 3.77e-06), (1.43e-04, 1.87e-04, 1.38e-04)),
    ('cnc', 3, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (2.64e-07, 2.06e-07, 2.30e-07), (3.60e-06, 3.30e-06, 3.81e-06)),
    ('cnc', 3, (218, 170), 'loop'): ((1.27e-06, 1.49e-06, 1.61e-06), (1.54e-06, 1.27e-06, 1.64e-06), (5.48e-05, 4.19e-05, 5.89e-05)),
    ('cnc', 4, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (2.41e-07, 2.87e-07, 2.25e-07), (4.87e-07, 5.51e-07, 4.49e-07)),
    ('cnc', 4, (256, 256), 'loop'): ((4.56e-06, 6.01e-06, 5.71e-06), (8.14e-06, 9.46e-06, 1.02e-05), (6.58e-05, 9.15e-05, 5.02e-05)),
    ('cnc', 4, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (2.53e-07, 2.71e-07, 3.03e-07), (4.67e-07, 4.83e-07, 4.97e-07)),
    ('cnc', 4, (512, 512), 'loop'): ((7.37e-06, 6.71e-06, 6.61e-06), (1.28e-05, 9.97e-06, 1.00e-05), (7.34e-05, 7.25e-05, 6.87e-05)),
    ('cnc', 4, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (2.64e-07, 2.52e-07, 2.52e-07), (4.44e-07, 5.23e-07, 4.83e-07)),
    ('cnc', 4, (218, 170), 'loop'): ((5.10e-06, 5.50e-06, 6.03e-06), (9.07e-06, 1.06e-05, 1.04e-05), (6.02e-05, 7.01e-05, 7.89e-05)),
    ('cnc', 5, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (1.71e-07, 1.63e-07, 1.67e-07), (1.60e-07, 1.26e-07, 1.49e-07)),
    ('cnc', 5, (256, 256), 'loop'): ((5.25e-07, 5.11e-07, 5.29e-07), (4.03e-07, 4.40e-07, 5.00e-07), (2.19e-05, 2.28e-05, 2.95e-05)),
    ('cnc', 5, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (1.71e-07, 1.59e-07, 1.72e-07), (1.33e-07, 1.49e-07, 1.53e-07)),
    ('cnc', 5, (512, 512), 'loop'): ((5.76e-07, 6.38e-07, 6.26e-07), (5.14e-07, 5.51e-07, 5.09e-07), (4.68e-05, 5.52e-05, 6.14e-05)),
    ('cnc', 5, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (1.74e-07, 1.64e-07, 1.89e-07), (1.42e-07, 1.81e-07, 1.24e-07)),
    ('cnc', 5, (218, 170), 'loop'): ((6.86e-07, 7.44e-07, 7.60e-07), (6.24e-07, 7.22e-07, 6.13e-07), (2.80e-05, 2.20e-05, 2.41e-05)),
    ('cnc', 6, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (1.69e-07, 1.69e-07, 1.80e-07), (1.35e-07, 1.57e-07, 1.71e-07)),
    ('cnc', 6, (256, 256), 'loop'): ((1.01e-06, 1.00e-06, 1.51e-06), (9.18e-07, 1.01e-06, 1.40e-06), (3.16e-05, 3.49e-05, 4.40e-05)),
    ('cnc', 6, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (1.87e-07, 1.82e-07, 1.86e-07), (1.46e-07, 1.82e-07, 1.77e-07)),
    ('cnc', 6, (512, 512), 'loop'): ((2.24e-06, 2.37e-06, 2.11e-06), (1.99e-06, 1.99e-06, 1.91e-06), (1.04e-04, 1.25e-04, 9.67e-05)),
    ('cnc', 6, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (2.01e-07, 1.64e-07, 2.33e-07), (1.73e-07, 2.14e-07, 1.50e-07)),
    ('cnc', 6, (218, 170), 'loop'): ((7.25e-07, 7.05e-07, 8.13e-07), (6.50e-07, 6.36e-07, 9.40e-07), (3.60e-05, 1.54e-05, 1.94e-05)),
    ('cnc', 7, (256, 256), 'step'): ((1.89e-07, 1.82e-07, 1.79e-07), (2.06e-07, 2.05e-07, 2.06e-07), (2.21e-07, 1.92e-07, 1.72e-07)),
    ('cnc', 7, (256, 256), 'loop'): ((8.79e-07, 1.02e-06, 9.27e-07), (8.24e-07, 9.78e-07, 8.83e-07), (3.15e-05, 4.97e-05, 4.78e-05)),
    ('cnc', 7, (512, 512), 'step'): ((2.16e-07, 2.16e-07, 2.37e-07), (2.29e-07, 2.02e-07, 2.49e-07), (1.89e-07, 1.85e-07, 2.38e-07)),
    ('cnc', 7, (512, 512), 'loop'): ((1.09e-06, 1.08e-06, 1.06e-06), (1.00e-06, 1.06e-06, 1.01e-06), (8.48e-05, 1.03e-04, 8.88e-05)),
    ('cnc', 7, (218, 170), 'step'): ((2.27e-07, 2.20e-07, 2.42e-07), (2.25e-07, 1.94e-07, 2.10e-07), (1.95e-07, 1.86e-07, 1.56e-07)),
    ('cnc', 7, (218, 170), 'loop'): ((9.93e-07, 1.11e-06, 1.07e-06), (9.55e-07, 9.17e-07, 1.03e-06), (3.59e-05, 2.72e-05, 3.63e-05)),
    ('cnc', 8, (256, 256), 'step'): ((2.26e-07, 1.98e-07, 2.04e-07), (1.93e-07, 1.61e-07, 1.56e-07), (1.46e-07, 1.68e-07, 1.62e-07)),
    ('cnc', 8, (256, 256), 'loop'): ((1.67e-06, 1.83e-06, 1.84e-06), (1.73e-06, 1.79e-06, 2.03e-06), (3.75e-05, 4.21e-05, 4.73e-05)),
    ('cnc', 8, (512, 512), 'step'): ((2.24e-07, 2.10e-07, 2.51e-07), (1.98e-07, 2.00e-07, 2.22e-07), (1.79e-07, 1.95e-07, 1.76e-07)),
    ('cnc', 8, (512, 512), 'loop'): ((2.72e-06, 2.57e-06, 2.73e-06), (2.55e-06, 3.14e-06, 3.17e-06), (5.28e-05, 5.65e-05, 5.82e-05)),
    ('cnc', 8, (218, 170), 'step'): ((2.71e-07, 2.50e-07, 2.30e-07), (1.81e-07, 2.12e-07, 1.59e-07), (1.87e-07, 2.01e-07, 1.87e-07)),
    ('cnc', 8, (218, 170), 'loop'): ((1.85e-06, 2.20e-06, 1.55e-06), (2.25e-06, 1.96e-06, 1.93e-06), (4.79e-05, 4.22e-05, 3.96e-05)),
    ('cnc', 9, (256, 256), 'step'): ((1.67e-07, 2.01e-07, 1.44e-07), (1.44e-07, 1.78e-07, 1.56e-07), (2.05e-07, 2.16e-07, 2.25e-07)),
    ('cnc', 9, (256, 256), 'loop'): ((1.11e-06, 1.35e-06, 1.16e-06), (1.22e-06, 1.76e-06, 1.41e-06), (1.19e-05, 8.92e-06, 8.80e-06)),
    ('cnc', 9, (512, 512), 'step'): ((1.81e-07, 2.21e-07, 1.88e-07), (1.94e-07, 1.92e-07, 1.80e-07), (2.69e-07, 2.41e-07, 2.07e-07)),
    ('cnc', 9, (512, 512), 'loop'): ((1.46e-06, 1.50e-06, 1.58e-06), (1.61e-06, 1.62e-06, 1.83e-06), (1.32e-05, 1.28e-05, 1.45e-05)),
    ('cnc', 9, (218, 170), 'step'): ((2.68e-07, 2.54e-07, 2.95e-07), (2.12e-07, 2.05e-07, 2.02e-07), (3.19e-07, 3.31e-07, 3.13e-07)),
    ('cnc', 9, (218, 170), 'loop'): ((9.66e-07, 1.54e-06, 1.66e-06), (1.38e-06, 1.40e-06, 1.77e-06), (8.61e-06, 1.62e-05, 1.08e-05)),
    ('l1', 0, (256, 256), 'step'): ((2.01e-07, 2.16e-07, 1.84e-07), (1.98e-07, 2.18e-07, 1.91e-07), (7.96e-05, 9.67e-05, 1.11e-04)),
    ('l1', 0, (256, 256), 'loop'): ((8.69e-07, 8.32e-07, 8.67e-07), (8.69e-07, 8.32e-07, 8.67e-07), (6.99e-06, 6.99e-06, 6.99e-06)),
    ('l1', 0, (512, 512), 'step'): ((2.34e-07, 2.51e-07, 2.12e-07), (2.35e-07, 2.37e-07, 1.82e-07), (9.50e-05, 9.58e-05, 9.35e-05)),
    ('l1', 0, (512, 512), 'loop'): ((9.74e-07, 1.03e-06, 1.15e-06), (9.74e-07, 1.03e-06, 1.15e-06), (6.99e-06, 6.99e-06, 6.99e-06)),
    ('l1', 0, (218, 170), 'step'): ((2.19e-07, 2.57e-07, 2.34e-07), (2.13e-07, 2.15e-07, 1.92e-07), (1.38e-04, 1.15e-04, 1.06e-04)),
    ('l1', 0, (218, 170), 'loop'): ((1.18e-06, 1.22e-06, 1.13e-06), (1.18e-06, 1.22e-06, 1.13e-06), (6.99e-06, 6.99e-06, 6.99e-06)),
    ('l1', 1, (256, 256), 'step'): ((2.01e-07, 2.16e-07, 1.84e-07), (1.91e-07, 2.11e-07, 1.84e-07), (0.00e+00, 0.00e+00, 0.00e+00)),
    ('l1', 1, (256, 256), 'loop'): ((9.80e-07, 9.57e-07, 8.57e-07), (9.80e-07, 9.57e-07, 8.57e-07), (0.00e+00, 0.00e+00, 0.00e+00)),
    ('l1', 1, (512, 512), 'step'): ((2.34e-07, 2.51e-07, 2.12e-07), (2.28e-07, 2.30e-07, 1.76e-07), (0.00e+00, 0.00e+00, 0.00e+00)),
    ('l1', 1, (512, 512), 'loop'): ((8.58e-07, 8.67e-07, 9.85e-07), (8.58e-07, 8.67e-07, 9.85e-07), (0.00e+00, 0.00e+00, 0.00e+00)),
    ('l1', 1, (218, 170), 'step'): ((2.19e-07, 2.57e-07, 2.34e-07), (2.06e-07, 2.08e-07, 1.85e-07), (0.00e+00, 0.00e+00, 0.00e+00)),
    ('l1', 1, (218, 170), 'loop'): ((1.14e-06, 8.96e-07, 1.12e-06), (1.14e-06, 8.96e-07, 1.12e-06), (0.00e+00, 0.00e+00, 0.00e+00)),
    ('l1', 2, (256, 256), 'step'): ((1.67e-07, 1.75e-07, 1.93e-07), (2.61e-07, 2.62e-07, 2.66e-07), (3.66e-07, 3.64e-07, 3.61e-07)),
    ('l1', 2, (256, 256), 'loop'): ((4.51e-06, 4.59e-06, 4.95e-06), (7.89e-06, 9.06e-06, 9.45e-06), (8.66e-06, 8.93e-06, 9.40e-06)),
    ('l1', 2, (512, 512), 'step'): ((1.91e-07, 1.83e-07, 2.20e-07), (2.54e-07, 3.10e-07, 3.10e-07), (4.35e-07, 4.78e-07, 3.76e-07)),
    ('l1', 2, (512, 512), 'loop'): ((5.14e-06, 6.19e-06, 5.45e-06), (1.04e-05, 1.05e-05, 1.12e-05), (9.98e-06, 1.10e-05, 1.06e-05)),
    ('l1', 2, (218, 170), 'step'): ((2.06e-07, 2.28e-07, 2.24e-07), (2.99e-07, 3.51e-07, 3.28e-07), (4.89e-07, 4.97e-07, 6.06e-07)),
    ('l1', 2, (218, 170), 'loop'): ((4.84e-06, 6.82e-06, 4.97e-06), (9.11e-06, 1.12e-05, 9.73e-06), (7.93e-06, 1.05e-05, 8.87e-06)),
    ('l1', 3, (256, 256), 'step'): ((2.26e-07, 1.98e-07, 2.04e-07), (2.13e-07, 2.05e-07, 1.89e-07), (1.42e-06, 1.52e-06, 1.54e-06)),
    ('l1', 3, (256, 256), 'loop'): ((3.60e-06, 3.73e-06, 2.87e-06), (3.88e-06, 7.34e-06, 5.67e-06), (2.84e-05, 3.55e-05, 2.88e-05)),
    ('l1', 3, (512, 512), 'step'): ((2.24e-07, 2.10e-07, 2.51e-07), (2.35e-07, 2.29e-07, 2.64e-07), (1.62e-06, 1.98e-06, 1.71e-06)),
    ('l1', 3, (512, 512), 'loop'): ((5.02e-06, 6.11e-06, 4.22e-06), (9.05e-06, 8.55e-06, 8.44e-06), (4.94e-05, 4.44e-05, 4.13e-05)),
    ('l1', 3, (218, 170), 'step'): ((2.71e-07, 2.50e-07, 2.30e-07), (2.67e-07, 2.20e-07, 2.17e-07), (2.41e-06, 2.06e-06, 2.09e-06)),
    ('l1', 3, (218, 170), 'loop'): ((2.51e-06, 2.86e-06, 3.67e-06), (4.24e-06, 3.98e-06, 6.66e-06), (3.29e-05, 4.55e-05, 3.69e-05)),
    ('l1', 4, (256, 256), 'step'): ((1.67e-07, 2.01e-07, 1.44e-07), (2.21e-07, 2.75e-07, 2.17e-07), (1.27e-06, 1.56e-06, 1.26e-06)),
    ('l1', 4, (256, 256), 'loop'): ((9.51e-07, 1.15e-06, 8.97e-07), (2.21e-06, 2.50e-06, 2.05e-06), (1.09e-05, 1.13e-05, 1.28e-05)),
    ('l1', 4, (512, 512), 'step'): ((1.81e-07, 2.21e-07, 1.88e-07), (2.41e-07, 2.73e-07, 2.64e-07), (1.62e-06, 1.51e-06, 1.51e-06)),
    ('l1', 4, (512, 512), 'loop'): ((1.50e-06, 1.52e-06, 1.46e-06), (3.29e-06, 3.01e-06, 3.08e-06), (1.84e-05, 1.85e-05, 1.89e-05)),
    ('l1', 4, (218, 170), 'step'): ((2.68e-07, 2.54e-07, 2.95e-07), (3.28e-07, 3.43e-07, 3.55e-07), (2.34e-06, 2.14e-06, 1.90e-06)),
    ('l1', 4, (218, 170), 'loop'): ((9.34e-07, 9.54e-07, 1.27e-06), (1.49e-06, 2.34e-06, 1.66e-06), (1.14e-05, 1.34e-05, 1.47e-05)),
    ('switch', 0, (256, 256), 'loop'): ((9.47e-07, 1.11e-06, 8.46e-07), (2.03e-06, 2.05e-06, 1.81e-06), (9.91e-06, 1.65e-05, 1.16e-05)),
    ('switch', 0, (512, 512), 'loop'): ((1.40e-06, 1.39e-06, 1.36e-06), (2.54e-06, 2.60e-06, 2.61e-06), (1.78e-05, 1.60e-05, 1.58e-05)),
    ('switch', 1, (256, 256), 'loop'): ((2.08e-06, 2.43e-06, 2.40e-06), (2.69e-06, 3.27e-06, 3.10e-06), (1.51e-05, 2.09e-05, 1.76e-05)),
    ('switch', 1, (512, 512), 'loop'): ((3.76e-06, 3.69e-06, 2.78e-06), (4.86e-06, 4.88e-06, 3.48e-06), (2.01e-05, 1.99e-05, 1.83e-05)),
    ('switch', 2, (256, 256), 'loop'): ((1.47e-06, 1.26e-06, 1.21e-06), (1.23e-06, 1.44e-06, 1.18e-06), (1.35e-05, 1.08e-05, 1.60e-05)),
    ('switch', 2, (512, 512), 'loop'): ((1.83e-06, 1.82e-06, 1.36e-06), (1.53e-06, 1.43e-06, 1.22e-06), (2.41e-05, 2.69e-05, 1.88e-05)),
    ('switch', 3, (256, 256), 'loop'): ((4.74e-06, 5.89e-06, 3.95e-06), (3.21e-06, 3.07e-06, 3.05e-06), (8.65e-06, 1.04e-05, 6.84e-06)),
    ('switch', 3, (512, 512), 'loop'): ((6.64e-06, 6.41e-06, 5.61e-06), (3.99e-06, 3.72e-06, 3.91e-06), (1.08e-05, 1.04e-05, 9.40e-06)),
}


if __name__ == '__main__':
    measure_bars()
