"""NumPy restatement of the periodic 2-D DWT and the wavelet-domain prox steps of ADMM_L1 / ADMM_CNC (csrc/wavelet_plan.h,
csrc/kernels_wavelet.hip), for the tests.  Deliberately unlike the tiled kernels: every pass is a whole-image `np.roll` over one axis.
This regulariser has no counterpart in the reference scripts; only the x-update (S4:119-124) is theirs.

Convention (one level along an axis of length M, periodic; h of length T, g[n] = (-1)^n h[T-1-n]):
    a[k] = sum_n h[n] s[(2k + n) mod M],   d[k] = sum_n g[n] s[(2k + n) mod M],   k < M / 2
    synthesis = the transpose.
2-D, L levels, Mallat layout in place: level l works on the top-left (H >> l) x (W >> l) block, rows first ([a | d]), then columns
([a ; d]); the inverse undoes the levels in reverse order, columns first.

Everything is computed in `dtype` (float64 or float32): arrays are cast once on entry and the filters are rounded to it.
"""
from math import comb

import numpy as np

NAMES = ('haar', 'db2', 'db4')


def _daubechies(p):
    """Minimum-phase Daubechies low-pass filter with p vanishing moments, in double: (1 + z)^p * prod (1 - z_k z) with z_k the roots
    inside the unit circle from P(y) = sum_{k<p} C(p-1+k, k) y^k, y = (2 - z - 1/z) / 4; normalised to sum h = sqrt(2)."""
    if p == 1:
        h = np.array([1.0, 1.0])
    else:
        py = [comb(p - 1 + k, k) for k in range(p)]                       # P(y), ascending powers of y
        # y = (2 - z - 1/z) / 4  ->  z^(p-1) P(y(z)) is a polynomial of degree 2 (p - 1) in z
        q = np.zeros(2 * (p - 1) + 1)
        base = np.array([-0.25, 0.5, -0.25])                              # z * y(z) = (-1 + 2 z - z^2) / 4, ascending
        for k, ck in enumerate(py):
            term = np.array([1.0])
            for _ in range(k):
                term = np.convolve(term, base)
            term = np.convolve(term, np.eye(1, p - k, p - 1 - k).ravel())  # times z^(p-1-k)
            q[:len(term)] += ck * term
        # roots in double, polished by Newton steps in extended precision; the products below are formed in it too and rounded once
        ld, cld = np.longdouble, np.clongdouble
        qd = q[::-1].astype(ld)                                           # descending powers, exact small rationals
        dq = (qd[:-1] * np.arange(len(qd) - 1, 0, -1).astype(ld))
        roots = np.roots(q[::-1]).astype(cld)
        for _ in range(6):
            roots = roots - np.polyval(qd.astype(cld), roots) / np.polyval(dq.astype(cld), roots)
        inside = roots[np.abs(roots) < 1.0]
        assert len(inside) == p - 1
        h = np.array([1.0], cld)
        for _ in range(p):
            h = np.convolve(h, np.array([1.0, 1.0], cld))
        for zk in inside:
            h = np.convolve(h, np.array([1.0, -zk], cld))
        assert np.abs(h.imag).max() < 1e-15 * np.abs(h.real).max()
        h = h.real
        return (h * (np.sqrt(ld(2.0)) / h.sum())).astype(np.float64)
    return h * (np.sqrt(2.0) / h.sum())


def filters(name, dtype=np.float64):
    """-> (h, g) as arrays of `dtype`."""
    if name == 'haar':
        h = np.array([1.0, 1.0]) * np.sqrt(0.5)
    elif name == 'db2':
        s3 = np.sqrt(3.0)
        h = np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2.0))
    elif name == 'db4':
        h = _daubechies(4)
    else:
        raise ValueError('unknown wavelet %r' % (name,))
    T = len(h)
    g = np.array([(-1) ** n * h[T - 1 - n] for n in range(T)])
    return h.astype(dtype), g.astype(dtype)


def _analysis(s, h, g, axis):
    """one level along `axis` of the whole array -> [a | d] along that axis"""
    a = np.zeros_like(s)
    d = np.zeros_like(s)
    for n in range(len(h)):
        r = np.roll(s, -n, axis=axis)                                     # r[m] = s[(m + n) mod M]
        a = a + h[n] * r
        d = d + g[n] * r
    idx = [slice(None)] * s.ndim
    idx[axis] = slice(0, None, 2)
    return np.concatenate([a[tuple(idx)], d[tuple(idx)]], axis=axis)


def _synthesis(c, h, g, axis):
    """transpose of _analysis: s[m] = sum over 2k + n = m (mod M) of h[n] a[k] + g[n] d[k]"""
    M = c.shape[axis]
    a, d = np.split(c, 2, axis=axis)
    shape = list(c.shape)
    ua = np.zeros(shape, c.dtype)
    ud = np.zeros(shape, c.dtype)
    idx = [slice(None)] * c.ndim
    idx[axis] = slice(0, None, 2)
    ua[tuple(idx)] = a                                                    # ua[2k] = a[k]
    ud[tuple(idx)] = d
    s = np.zeros(shape, c.dtype)
    for n in range(len(h)):
        s = s + h[n] * np.roll(ua, n, axis=axis) + g[n] * np.roll(ud, n, axis=axis)
    assert s.shape[axis] == M
    return s


def fwd(v, name, levels, dtype=np.float64):
    """Psi v for v [..., H, W]"""
    h, g = filters(name, dtype)
    c = np.array(v, dtype=dtype)
    H, W = c.shape[-2:]
    for l in range(levels):
        blk = c[..., :H >> l, :W >> l]
        blk = _analysis(blk, h, g, -1)
        blk = _analysis(blk, h, g, -2)
        c[..., :H >> l, :W >> l] = blk
    return c


def inv(c, name, levels, dtype=np.float64):
    """Psi^T c"""
    h, g = filters(name, dtype)
    v = np.array(c, dtype=dtype)
    H, W = v.shape[-2:]
    for l in reversed(range(levels)):
        blk = v[..., :H >> l, :W >> l]
        blk = _synthesis(blk, h, g, -2)
        blk = _synthesis(blk, h, g, -1)
        v[..., :H >> l, :W >> l] = blk
    return v


def detail_mask(H, W, levels):
    m = np.ones((H, W), bool)
    m[:H >> levels, :W >> levels] = False
    return m


def soft(a, thr):
    return np.sign(a) * np.maximum(np.abs(a) - thr, 0)


def prox_l1(x, z, w, thr, name, levels, dtype=np.float64):
    """-> (z+, w+): c = Psi (x + w), soft on the detail coefficients, z+ = Psi^T c, w+ = (x + w) - z+"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    u = x + w
    c = fwd(u, name, levels, dtype)
    det = detail_mask(*c.shape[-2:], levels)
    c = np.where(det, soft(c, dtype(thr)), c)
    zn = inv(c, name, levels, dtype)
    return zn, u - zn


def prox_cnc(x, z, w, alpha, lambda1, reo, b, name, levels, dtype=np.float64):
    """-> (z+, w+): the CNC pair of thresholds (S4:127-129) coefficient-wise on the detail coefficients"""
    x, z, w = np.asarray(x, dtype), np.asarray(z, dtype), np.asarray(w, dtype)
    thr, c1, c2, c3, ib = (dtype(alpha * reo * lambda1), dtype(1.0 - alpha), dtype(alpha), dtype(alpha * reo * lambda1 * b),
                           dtype(1.0 / b))
    u = x + w
    cz = fwd(z, name, levels, dtype)
    cu = fwd(u, name, levels, dtype)
    det = detail_mask(*cz.shape[-2:], levels)
    t = c1 * cz + c2 * cu
    t = np.where(det, t + c3 * np.clip(cz, -ib, ib), t)
    c = np.where(det, soft(t, thr), t)
    zn = inv(c, name, levels, dtype)
    return zn, u - zn


def dc_step(y, mask, z, w, reo, dtype=np.float64):
    """the x-update of S4:119-124 on one slice or a batch [..., H, W]"""
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    La2 = dtype(1.0 / 2.0 / reo)
    xf = np.fft.fft2(np.asarray(z - w, dtype)).astype(cdt)
    xf = np.where(np.asarray(mask) != 0, (La2 * xf + np.asarray(y, cdt)) / (dtype(1.0) + La2), xf)
    return np.abs(np.real(np.fft.ifft2(xf))).astype(dtype)


def loop(y, mask, iters, kind, params, name, levels, dtype=np.float64, z0=None, w0=None):
    """`iters` iterations of x = dc(z, w); (z, w) = prox(x, z, w) from z0 = |ifft2(y)|, w0 = 0 -> (x, z, w).
    kind 'l1': params = dict(lambda1, reo); 'cnc': dict(alpha, lambda1, reo, b)."""
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    y = np.asarray(y, cdt)
    z = np.abs(np.fft.ifft2(y)).astype(dtype) if z0 is None else np.asarray(z0, dtype)
    w = np.zeros_like(z) if w0 is None else np.asarray(w0, dtype)
    x = z.copy()
    for _ in range(iters):
        x = dc_step(y, mask, z, w, params['reo'], dtype)
        if kind == 'l1':
            z, w = prox_l1(x, z, w, params['reo'] * params['lambda1'], name, levels, dtype)
        else:
            z, w = prox_cnc(x, z, w, params['alpha'], params['lambda1'], params['reo'], params['b'], name, levels, dtype)
    return x, z, w


# ---- shared inputs of tests/test_gpu_wavelet.py and the float32 bars measured on them ---------------------------------------------

GPU_SHAPES = ((128, 128), (128, 160), (256, 192), (256, 256), (512, 512))
TAPS = {'haar': 2, 'db2': 4, 'db4': 8}


def valid(name, levels, H, W):
    return 1 <= levels <= 4 and H % (1 << levels) == 0 and W % (1 << levels) == 0 and (min(H, W) >> (levels - 1)) >= TAPS[name]


def gpu_levels(name, H, W):
    """the level counts the GPU tests run at a shape: 1 and the largest valid one (512 x 512: 1 only)"""
    top = max(l for l in range(1, 5) if valid(name, l, H, W))
    return (1,) if H == 512 else tuple(sorted({1, top}))


def field(H, W):
    """[B, H, W] float32, every slice different (B = 2; 1 at 512 x 512)"""
    rng = np.random.default_rng(1000 * H + W)
    return rng.standard_normal((1 if H == 512 else 2, H, W)).astype(np.float32)


PROX_CASES = (('db4', 4, 128, 128), ('db2', 3, 128, 160), ('haar', 4, 256, 192), ('db4', 3, 256, 256), ('db2', 1, 512, 512))
PROX_L1_THR = 0.3
PROX_CNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)          # thr = 0.225, clip at 1 / b = 0.25: both sides of both populated


def prox_inputs(H, W):
    """x, z, w [B, H, W] float32 from which both branches of soft and of clip are taken"""
    rng = np.random.default_rng(77 * H + W)
    B = 1 if H == 512 else 3
    x = (0.5 * np.abs(rng.standard_normal((B, H, W)))).astype(np.float32)
    z = (0.5 * np.abs(rng.standard_normal((B, H, W)))).astype(np.float32)
    w = (0.3 * rng.standard_normal((B, H, W))).astype(np.float32)
    return x, z, w


def phantom(B, H, W, seed=0):
    """piecewise-constant slices in [0, 1] (rectangles and discs), every slice different"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((B, H, W))
    for b in range(B):
        for _ in range(12):
            cy, cx, r = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.05, 0.3) * min(H, W)
            v = rng.uniform(0.1, 0.5)
            if rng.integers(2):
                out[b][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += v
            else:
                out[b][(np.abs(yy - cy) < r) & (np.abs(xx - cx) < 0.6 * r)] += v
        out[b] /= max(out[b].max(), 1.0)
    return out


def problem(B, H, W, seed=0):
    """-> (y [B,H,W] complex64, mask [H,W] uint8, gt [B,H,W] uint8): 30 % random mask (centre kept), phantom, complex noise.  y holds
    float32 values, so a float32 and a float64 engine and the oracle all start from the same numbers."""
    rng = np.random.default_rng(seed + 17)
    gt = np.round(phantom(B, H, W, seed) * 255).astype(np.uint8)
    img = gt.astype(np.float64) / 255.0
    mask = (rng.uniform(size=(H, W)) < 0.3).astype(np.uint8)
    mask[0, 0] = 1
    noise = (rng.standard_normal((B, H, W)) + 1j * rng.standard_normal((B, H, W))) * 0.5
    y = (np.fft.fft2(img) * mask + noise).astype(np.complex64)
    return y, mask, gt


# ---- the partial-tile cases of tests/test_gpu_wavelet_edges.py: sizes, inputs, the per-element distance and where the partial tiles lie ---
# Helpers only: no arithmetic of the transform or the prox is added here.

# levels: (H, W).  Every length is >= 128 and a multiple of 2^L; at the tile of every filter (tile()) both axes end in a partial tile: one
# in a tile with a single coefficient of the deepest level (2^L pixels), the other in a tile one such coefficient short of full -- at L = 4
# with tile 32 both end in half a tile.  tiles_x != tiles_y where the tile is 32 (5 x 6 tiles); at tile 64 these sizes are 3 x 3 tiles
# (2 . 64 + 2^L and 3 . 64 - 2^L), so EDGE_TILE64 adds one size of 3 x 4 tiles of 64 (2 . 64 + 8, 4 . 64 - 8; 5 x 8 tiles of 32).
EDGE_SIZES = {1: (130, 190), 2: (132, 188), 3: (136, 184), 4: (144, 176)}
EDGE_TILE64 = (3, 136, 248)                  # (L, H, W)
EDGE_CASES = tuple((L,) + hw for L, hw in sorted(EDGE_SIZES.items())) + (EDGE_TILE64,)          # (L, H, W)
EDGE_B = 2                                   # slices of every edge case, on contexts of Bmax = 3
FREEDOM, FLOOR, F64_BAR = 4.0, 2e-6, 1e-12   # tests/param_space_oracle.py: 4 x the float32 restatement's distance, floor 2e-6; 1e-12 in double
F32_CAP = 5e-6                               # no float bar of a single step may exceed this (asserted where the bar is formed)


def tile(name, levels):
    """the tile edge of csrc/wavelet_plan.h (wv_tile): 64 while the analysis halo (T - 2)(2^L - 1) is at most 16 pixels, else 32"""
    return 64 if (TAPS[name] - 2) * ((1 << levels) - 1) <= 16 else 32


def edge_prox_inputs(H, W):
    """the first EDGE_B slices of prox_inputs(H, W)"""
    return tuple(a[:EDGE_B] for a in prox_inputs(H, W))


def edge_points():
    """The points of the partial-tile tests that change the branch structure of the prox: (kind, parameters, the branches the point
    leaves empty) -- 'lo', 'mid', 'hi' of the inner clip, 'zero', 'pass' of the soft threshold (tests/param_space_oracle.py, whose points
    these are wherever it names one).  kind 'cnc': (alpha, lambda1, reo, b); 'l1': (lambda1, reo)."""
    import param_space_oracle as PS
    return (
        ('cnc', PS.params('cnc', 2), ('zero',)),             # alpha = 0: thr = 0, c2 = c3 = 0, the coefficients of z pass through
        # alpha = 1 (c1 = 0).  Not the grid's point 3 (reo = 0.05, thr = 0.025): there w+ = u - z+ is small against u, the float32
        # restatement's distance is 6.1e-6 of max |w+| on these inputs, and 4 x that is beyond F32_CAP.  thr = 0.3, c3 = 1.2:
        ('cnc', (1.0, 0.3, 1.0, 4.0), ()),
        ('cnc', PS.params('cnc', 5), ('zero',)),             # lambda1 = 0: thr = 0, c3 = 0
        ('cnc', PS.params('cnc', 6), ('lo', 'hi')),          # b = 0.5: the clip never acts
        ('cnc', PS.params('cnc', 7), ('mid', 'zero')),       # b = 1e4: the clip acts everywhere, thr = 4.5e-5
        ('l1', PS.params('l1', 1), ('zero',)),               # lambda1 = 0: thr = 0, z+ = Psi^T Psi (x + w), w+ ~ 0
    )


BRANCH_ON, BRANCH_OFF = 0.02, 0.001          # a populated branch holds >= 2 % of the detail coefficients (test_gpu_wavelet), an empty one < 0.1 %


def prox_branches(kind, params, x, z, w, name, levels):
    """Share of the detail coefficients in each branch of one prox step, counted in float64: {'zero', 'pass'} and for CNC
    {'lo', 'mid', 'hi'}."""
    det = detail_mask(*np.shape(x)[-2:], levels)
    cu = fwd(np.asarray(x, np.float64) + np.asarray(w, np.float64), name, levels)[..., det]
    if kind == 'cnc':
        alpha, lambda1, reo, b = params
        cz = fwd(z, name, levels)[..., det]
        thr = alpha * reo * lambda1
        t = (1 - alpha) * cz + alpha * cu + thr * b * np.clip(cz, -1 / b, 1 / b)
        out = {'lo': np.mean(cz < -1 / b), 'mid': np.mean(np.abs(cz) <= 1 / b), 'hi': np.mean(cz > 1 / b)}
    else:
        lambda1, reo = params
        t, thr, out = cu, reo * lambda1, {}
    out.update(zero=np.mean(np.abs(t) <= thr), **{'pass': np.mean(np.abs(t) > thr)})
    return {k: float(v) for k, v in out.items()}


def check_branches(kind, params, off, x, z, w, name, levels):
    """assert that the branches in `off` are empty and every other one is populated -> the shares"""
    share = prox_branches(kind, params, x, z, w, name, levels)
    for k, v in share.items():
        assert (v < BRANCH_OFF) if k in off else (v >= BRANCH_ON), (kind, params, k, v, share)
    return share


def _axis_level(n, levels):
    """level of the Mallat band each index of an axis of length n falls in when the other axis lies in an approximation part"""
    idx = np.arange(n)
    lv = np.full(n, levels)
    for l in range(levels, 0, -1):
        lv[idx >= (n >> l)] = l
    return lv


def partial_tile_mask(H, W, name, levels, coef=False, shifts=((0, 0),)):
    """-> bool [H, W]: the elements a workgroup with a partial tile writes -- a tile that the image ends inside, on either axis.
    coef=False: pixels; with cycle spinning the synthesis emits pixel (i, j) of a tile to (i + sy, j + sx), so the strip moves with every
    shift of `shifts` (their union).  coef=True: coefficients in Mallat layout -- a band of level l is cut into tiles of tile >> l, in the
    frame of the shift, so `shifts` does not move them."""
    t = tile(name, levels)
    if not coef:
        m = np.zeros((H, W), bool)
        if H % t:
            m[H - H % t:, :] = True
        if W % t:
            m[:, W - W % t:] = True
        out = np.zeros((H, W), bool)
        for sy, sx in shifts:
            out |= np.roll(m, (int(sy), int(sx)), (0, 1))
        return out
    lv = np.minimum(_axis_level(H, levels)[:, None], _axis_level(W, levels)[None, :])
    yy, xx = np.mgrid[:H, :W]
    py = np.where(yy >= (H >> lv), yy - (H >> lv), yy)
    px = np.where(xx >= (W >> lv), xx - (W >> lv), xx)
    return ((H % t != 0) & (py // (t >> lv) == H // t)) | ((W % t != 0) & (px // (t >> lv) == W // t))


def last_tile_origin(H, W, name, levels):
    """first pixel of the bottom-right tile: partial on both axes at every EDGE_SIZES case"""
    t = tile(name, levels)
    return (H - 1) // t * t, (W - 1) // t * t


def distance(got, ref, scale=None):
    """max |got - ref| / max |ref| per slice, [B]; scale [B]: in place of max |ref|, where the reference itself is ~ 0"""
    ref = np.asarray(ref)
    d = np.abs(np.asarray(got).astype(ref.dtype) - ref).reshape(ref.shape[0], -1).max(axis=1)
    s = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1) if scale is None else np.asarray(scale, np.float64)
    return d / s


def float_bar(r32, r64, scale=None, cap=True):
    """The bar of a float kernel, per slice [B], as a multiple of max |ref| (or `scale`): FREEDOM x the distance of the float32
    restatement r32 from the float64 oracle r64 on the same case, floor FLOOR.  cap: a bar beyond F32_CAP is an error of the case."""
    bar = np.maximum(FREEDOM * distance(r32, r64, scale), FLOOR)
    assert not cap or (bar <= F32_CAP).all(), bar
    return bar


def worst(got, ref, bar, part, scale=None):
    """Per-element comparison of got with ref [B, H, W] at bar [B] (or a number) -> dict: 'ratio' the worst max |got - ref| / (bar x
    max |ref|) over the slices, 'pos' (slice, row, column) of the worst element, 'partial' whether it lies in `part` (bool [H, W]: the
    partial tiles), 'inside' / 'outside' the worst ratio over the elements in / not in `part`."""
    ref = np.asarray(ref)
    got = np.asarray(got)
    assert got.shape == ref.shape and np.isfinite(got.view(got.real.dtype)).all(), (got.shape, ref.shape)
    s = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1) if scale is None else np.asarray(scale, np.float64)
    r = np.abs(got.astype(ref.dtype) - ref) / (np.broadcast_to(np.asarray(bar, np.float64), s.shape) * s)[:, None, None]
    pos = tuple(int(v) for v in np.unravel_index(int(np.argmax(r)), r.shape))
    inside = float(r[:, part].max()) if part.any() else 0.0
    outside = float(r[:, ~part].max()) if not part.all() else 0.0
    return {'ratio': float(r.max()), 'pos': pos, 'partial': bool(part[pos[1], pos[2]]), 'inside': inside, 'outside': outside}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def measure_bars():
    """Distance of the float32 restatement from the float64 one on the GPU tests' own inputs (CPU only): what `python
    tests/wavelet_oracle.py` prints and tests/test_gpu_wavelet.py holds as constants (the tests multiply by 4)."""
    f32 = np.float32
    print('DWT_F32 = {   # (H, W, name, L): (Psi, Psi^T, Psi^T Psi)')
    for H, W in GPU_SHAPES:
        v = field(H, W)
        for name in NAMES:
            for L in gpu_levels(name, H, W):
                c64 = fwd(v, name, L)
                c = c64.astype(f32)
                print('    (%d, %d, %r, %d): (%.2e, %.2e, %.2e),' % (H, W, name, L, _rel(fwd(v, name, L, f32), c64),
                                                                      _rel(inv(c, name, L, f32), inv(c, name, L)),
                                                                      _rel(inv(fwd(v, name, L, f32), name, L, f32), v)))
    print('}')
    print('PROX_F32 = {   # (kind, name, L, H, W): (z+, w+)')
    for name, L, H, W in PROX_CASES:
        x, z, w = prox_inputs(H, W)
        a, b = prox_l1(x, z, w, PROX_L1_THR, name, L), prox_l1(x, z, w, PROX_L1_THR, name, L, f32)
        print("    ('l1', %r, %d, %d, %d): (%.2e, %.2e)," % (name, L, H, W, _rel(b[0], a[0]), _rel(b[1], a[1])))
        a, b = prox_cnc(x, z, w, name=name, levels=L, **PROX_CNC), prox_cnc(x, z, w, name=name, levels=L, dtype=f32, **PROX_CNC)
        print("    ('cnc', %r, %d, %d, %d): (%.2e, %.2e)," % (name, L, H, W, _rel(b[0], a[0]), _rel(b[1], a[1])))
    print('}')


if __name__ == '__main__':
    measure_bars()
