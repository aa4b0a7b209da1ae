"""NumPy oracle of the locally low-rank prox and its loops -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the mathematics of include/pnp_mri.h ("low-rank"), written from that text and not from the kernels:

    batch = S series of T consecutive slices.  The grid of b x b patches is anchored at the shift (sy, sx), 0 <= sy, sx < b: patch (i, j)
    holds the rows (sy + i b + r) mod H and the columns (sx + j b + c) mod W, r, c < b; where b does not divide H or W the last patch row
    or column is partial (H mod b rows, W mod b columns) and does not wrap onto the first patch.  X [P, T] is one patch across the frames,
    X = U diag(sigma) V^T, S_g(X) = X V diag(g(sigma)) V^T.
    thr, c1, c2, c3, ib are the scalars of the pixel-domain step with thr <- scale thr, ib <- scale ib.
    L1:   z+ = S_shrink(x + w),  shrink(s) = max(1 - thr / s, 0), 0 at s = 0
    CNC:  t = c1 z + c2 u + c3 S_clip(z),  clip(s) = min(1, ib / s), 1 at s = 0;  z+ = S_shrink(t)
    both: w+ = u - z+

R = np.float64 is the oracle, by np.linalg.svd.  R = np.float32 is the float restatement by the Gram route -- G = X^T X, its symmetric
eigen-decomposition, sigma = sqrt(max(lambda, 0)), S_g(X) = X (V g(sigma) V^T), everything in float32 -- which squares the condition of
X and is therefore the worse conditioned of the two routes; its distance from the oracle ON THE SAME CASE sets the bar of a float GPU
test (4 x that distance; DESIGN.md sections 13, 20, 22).  route='gram' with R = np.float64 is that route in double.

`python tests/lowrank_oracle.py` re-measures the PSNR table of DESIGN.md section 23 and the float restatement's distances (CPU only).
"""
import os
import sys

import numpy as np

if __name__ == '__main__':                      # run as a script: the repository root, for multicoil_oracle's `oracle` package
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import complex_oracle as CO
import multicoil_oracle as M
import temporal_oracle as TO
import wavelet_oracle as WO

PRESETS = M.O_PRESETS
MIN_BLOCK, MAX_BLOCK = 2, 32
TABLE = 64                                      # entries of the 'random' shift table
rel, psnr = M.rel, TO.psnr


def _cdt(R):
    return np.complex128 if R == np.float64 else np.complex64


# ---- the patch partition ---------------------------------------------------------------------------------------------------------------

def partition(H, W, b, sy=0, sx=0):
    """-> list of (rows, cols): the index vectors of every patch of the grid anchored at (sy, sx)"""
    if not (MIN_BLOCK <= b <= MAX_BLOCK and b <= min(H, W) and 0 <= sy < b and 0 <= sx < b):
        raise ValueError('bad block or shift')
    out = []
    for y0 in range(0, H, b):
        rows = (sy + y0 + np.arange(min(b, H - y0))) % H
        for x0 in range(0, W, b):
            out.append((rows, (sx + x0 + np.arange(min(b, W - x0))) % W))
    return out


def default_scale(b):
    return b / 2.0


def shift_table(shift, b, seed=0):
    """the table of lowrank_shift=: 'random' -> np.random.default_rng(seed).integers(0, b, size=(64, 2)); None -> [[0, 0]]; an array-like
    [n, 2] is passed through.  -> int32 [n, 2]"""
    if shift is None:
        return np.zeros((1, 2), np.int32)
    if isinstance(shift, str):
        if shift != 'random':
            raise ValueError('bad shift')
        return np.random.default_rng(seed).integers(0, b, size=(TABLE, 2)).astype(np.int32)
    return np.asarray(shift, np.int32).reshape(-1, 2)


# ---- the spectral maps -------------------------------------------------------------------------------------------------------------------

def shrink(s, thr):
    with np.errstate(all='ignore'):
        return np.where(s > thr, (s - thr) / np.where(s > thr, s, 1), 0).astype(s.dtype)


def clip(s, ib):
    with np.errstate(all='ignore'):
        return np.where(s > ib, ib / np.where(s > ib, s, 1), 1).astype(s.dtype)


def spectral(X, g, route='svd'):
    """S_g of a stack of matrices X [..., P, T], in X's precision"""
    if route == 'svd':
        U, s, Vt = np.linalg.svd(X, full_matrices=False)
        return (U * (s * g(s))[..., None, :]) @ Vt
    G = np.swapaxes(X, -1, -2) @ X
    lam, V = np.linalg.eigh(G)
    s = np.sqrt(np.maximum(lam, 0)).astype(X.dtype)
    return (X @ ((V * g(s)[..., None, :]) @ np.swapaxes(V, -1, -2)).astype(X.dtype)).astype(X.dtype)


def _patchwise(a, T, b, shift, fn):
    """fn on the [n, P, T] stacks of equally shaped patches of a [S T, H, W] -> the array put together again"""
    B, H, W = a.shape
    ser = a.reshape(B // T, T, H, W)
    out = np.empty_like(ser)
    shapes = {}
    for rows, cols in partition(H, W, b, *shift):
        shapes.setdefault((len(rows), len(cols)), []).append((rows, cols))
    for (ph, pw), group in shapes.items():
        for s_ in range(B // T):
            X = np.stack([ser[s_][:, rows[:, None], cols[None, :]].reshape(T, ph * pw).T for rows, cols in group])
            Y = fn(X)
            for (rows, cols), y in zip(group, Y):
                out[s_][:, rows[:, None], cols[None, :]] = y.T.reshape(T, ph, pw)
    return out.reshape(B, H, W)


def scalars(kind, pr, scale, R=np.float64):
    """thr, c1, c2, c3, ib of the step in R, thr and ib scaled (the product formed in double from the rounded scalar, rounded once)"""
    if kind == 'l1':
        thr, c1, c2, c3, ib = R(pr['reo'] * pr['lambda1']), R(0), R(0), R(0), R(0)
    else:
        thr, c1, c2, c3, ib = CO.cnc_scalars(pr['alpha'], pr['lambda1'], pr['reo'], pr['b'], _cdt(R))
    return R(float(thr) * scale), c1, c2, c3, R(float(ib) * scale)


def prox(kind, x, z, w, pr, T, b, shift=(0, 0), scale=None, R=np.float64, route=None):
    """one prox step on a real batch [B, H, W], B a multiple of T.  kind 'l1': pr = dict(lambda1, reo); 'cnc': dict(alpha, lambda1, reo,
    b).  -> (z+, w+) in R"""
    x, z, w = (np.asarray(a).astype(R) for a in (x, z, w))
    if x.shape[0] % T or T < 2 or T > 64:
        raise ValueError('bad frames')
    route = route or ('svd' if R == np.float64 else 'gram')
    thr, c1, c2, c3, ib = scalars(kind, pr, default_scale(b) if scale is None else scale, R)
    u = (x + w).astype(R)
    t = u
    if kind == 'cnc':
        sc = _patchwise(z, T, b, shift, lambda X: spectral(X, lambda s: clip(s, ib), route))
        t = (c1 * z + (c2 * u + (c3 * sc).astype(R)).astype(R)).astype(R)
    zn = _patchwise(t, T, b, shift, lambda X: spectral(X, lambda s: shrink(s, thr), route)).astype(R)
    return zn, (u - zn).astype(R)


# ---- the loops -------------------------------------------------------------------------------------------------------------------------

def loop(y, masks, iters, kind, pr, T, b, table=None, scale=None, R=np.float64, z0=None, w0=None, cursor=0, states=()):
    """`iters` iterations of x = dc(z, w); (z, w) = prox(x, z, w) without coils, from z0 = |ifft2(y)|, w0 = 0; prox step k uses entry
    (cursor + k) mod n of the shift table.  y, masks [B, H, W].  -> (x, z, w); states: iterations at which (x, z, z_prev, w) are kept"""
    table = shift_table(table, b)
    y = np.asarray(y, _cdt(R))
    z = np.abs(np.fft.ifft2(y)).astype(R) if z0 is None else np.asarray(z0, R)
    w = np.zeros_like(z) if w0 is None else np.asarray(w0, R)
    x, kept = z.copy(), []
    for k in range(iters):
        zp = z
        x = WO.dc_step(y, masks, z, w, pr['reo'], R)
        z, w = prox(kind, x, z, w, pr, T, b, tuple(table[(cursor + k) % len(table)]), scale, R)
        if k + 1 in states:
            kept.append((x, z, zp, w))
    return (x, z, w, kept) if states else (x, z, w)


def coil_loop(y, S, masks, iters, kind, pr, T, b, table=None, scale=None, R=np.float64, cg_iters=3, states=()):
    """the same with the multi-coil x-step of tests/multicoil_oracle.py, one coil set S [C, H, W].  y [B, C, H, W] -> (x, z, w); states:
    iterations after which x is kept (a fourth value, the list of them)"""
    table, dt = shift_table(table, b), _cdt(R)
    B = y.shape[0]
    st = [M.init_state(y[i], S, masks[i], dt) for i in range(B)]
    aty, z, w = (np.stack([s[i] for s in st]) for i in range(3))
    x, kept = z.copy(), []
    for k in range(iters):
        x = np.stack([M.x_step(z[i], w[i], aty[i], S, masks[i], pr['reo'], cg_iters, dt) for i in range(B)])
        z, w = prox(kind, x, z, w, pr, T, b, tuple(table[k % len(table)]), scale, R)
        if k + 1 in states:
            kept.append(x)
    return (x, z, w, kept) if states else (x, z, w)


# ---- the relaxation phantom of DESIGN.md section 23 -----------------------------------------------------------------------------------

def relaxation_phantom(T, H, W):
    """[T, H, W] float64 in [0, 1]: four regions -- a body ellipse and three inserts -- each a (1 - e^(-(t + 1) / tau)) with its own
    amplitude a and time constant tau: a contrast that changes without a period"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (yy - H / 2) / H, (xx - W / 2) / W
    regions = ((((u / 0.40) ** 2 + (v / 0.32) ** 2 <= 1.0), 0.45, 2.0),
               ((((u + 0.15) / 0.10) ** 2 + ((v - 0.05) / 0.16) ** 2 <= 1.0), 0.90, 6.0),
               (((u - 0.2) ** 2 + (v + 0.1) ** 2 <= 0.06 ** 2), 0.75, 12.0),
               (((u - 0.05) ** 2 + (v - 0.14) ** 2 <= 0.05 ** 2), 1.00, 3.5))
    amp, tau = np.zeros((H, W)), np.ones((H, W))
    for where, a, tc in regions:                   # a later region replaces the body under it
        amp[where], tau[where] = a, tc
    t = np.arange(T, dtype=np.float64)[:, None, None]
    return np.clip(amp * (1.0 - np.exp(-(t + 1.0) / tau)), 0.0, 1.0)


def relaxation_problem(T, H, W, sigma=1.0, seed=0):
    """-> (img [T, H, W] float64, masks [T, H, W] uint8, y [T, H, W] complex64): the column masks of temporal_oracle.column_masks,
    y = mask . fft2(img) + mask . noise, holding float32 values"""
    rng = np.random.default_rng(8900 + seed)
    img, masks = relaxation_phantom(T, H, W), TO.column_masks(T, H, W, seed=seed)
    nz = sigma * (rng.standard_normal((T, H, W)) + 1j * rng.standard_normal((T, H, W)))
    return img, masks, ((np.fft.fft2(img) + nz) * masks).astype(np.complex64)


# ---- shared inputs of tests/test_gpu_lowrank.py ----------------------------------------------------------------------------------------

PROX_L1 = dict(lambda1=0.5, reo=0.6)                               # thr = 0.3 (times the scale)
PROX_CNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)           # thr = 0.225, ib = 0.25 (times the scale)
DESIGNED = 8                                                        # patches prox_inputs designs in every series


def prox_inputs(S, T, H, W, b, shift=(0, 0), scale=None, seed=0):
    """x, z, w [S T, H, W] holding float32 values: random data, every series different, and designed patches of the grid anchored at
    `shift`, w = 0 and x = u there.  With thr, ib the scaled L1 threshold and clip level, a (unit, over the patch) and v (unit, over time):
      patch 0  all zero in x, z and w: z+ is exactly 0
            1  rank 1 far above the threshold, 50 thr a v^T: z+ = (1 - thr / sigma) u (L1)
        2 3 4  rank 1 with sigma at thr (1 - 1e-3), thr, thr (1 + 1e-3)
        5 6    z rank 1 with sigma at ib (1 - 1e-3), ib (1 + 1e-3)
            7  constant in time
      the last patch of the grid (partial where b does not divide H and W; fewer than T pixels make it rank-deficient) keeps its random
      data.  -> (x, z, w, patches): the (rows, cols) of the grid"""
    scale = default_scale(b) if scale is None else scale
    rng = np.random.default_rng(9100 + 131 * T + 7 * S + H + W + 3 * b + seed)
    g = lambda sc: sc * rng.standard_normal((S, T, H, W))
    x, z, w = g(0.5), g(0.5), g(0.3)
    grid = partition(H, W, b, *shift)
    thr, ib = PROX_L1['reo'] * PROX_L1['lambda1'] * scale, scale / PROX_CNC['b']

    def rank1(rows, cols, sigma):
        a, v = rng.standard_normal((len(rows), len(cols))), rng.standard_normal(T)
        return sigma * (v / np.linalg.norm(v))[:, None, None] * (a / np.linalg.norm(a))[None]

    def put(arr, s_, k, val):
        rows, cols = grid[k]
        arr[s_][:, rows[:, None], cols[None, :]] = val

    for s_ in range(S):
        for k in range(DESIGNED):
            put(w, s_, k, 0.0)
        put(x, s_, 0, 0.0)
        put(z, s_, 0, 0.0)
        put(x, s_, 1, rank1(*grid[1], 50.0 * thr))
        for k, f in ((2, 1 - 1e-3), (3, 1.0), (4, 1 + 1e-3)):
            put(x, s_, k, rank1(*grid[k], f * thr))
        for k, f in ((5, 1 - 1e-3), (6, 1 + 1e-3)):
            put(z, s_, k, rank1(*grid[k], f * ib))
        rows, cols = grid[7]
        put(x, s_, 7, np.broadcast_to((1.0 + 0.1 * s_) * rng.standard_normal((len(rows), len(cols))), (T, len(rows), len(cols))))
    f32 = lambda a: a.reshape(S * T, H, W).astype(np.float32).astype(np.float64)
    return f32(x), f32(z), f32(w), grid


def series_problem(S, T, H, W, C=0, seed=0):
    """-> (y, masks [S T, H, W] uint8, maps [C, H, W] or None): S series of the relaxation phantom (every series scaled and rolled
    differently), another column mask on every slice, complex noise of sigma 1 on the sampled points; complex128 holding float32 values"""
    rng = np.random.default_rng(6700 + seed + 31 * T + S)
    base = relaxation_phantom(T, H, W)
    img = np.concatenate([(1.0 - 0.15 * s_) * np.roll(base, (3 * s_, -2 * s_), axis=(1, 2)) for s_ in range(S)])
    masks = TO.column_masks(S * T, H, W, seed=seed + T)
    nz = lambda shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if C == 0:
        y, maps = (np.fft.fft2(img) + nz(img.shape)) * masks, None
    else:
        maps = M.coil_maps(C, H, W, seed).astype(np.complex64).astype(np.complex128)
        y = np.stack([M.A(img[i], maps, masks[i]) + nz((C, H, W)) * masks[i] for i in range(S * T)])
    return y.astype(np.complex64).astype(np.complex128), masks, maps


def measure():
    T, H, W, b = 16, 128, 128, 8
    table = shift_table('random', b, 0)
    for name, (img, masks, y) in (('relaxation phantom', relaxation_problem(T, H, W)), ('periodic phantom', TO.dynamic_problem(T, H, W))):
        print('%s, %d frames of %d x %d: zero-filled %.2f dB' % (name, T, H, W, psnr(np.abs(np.fft.ifft2(y)), img)))
        for kind in ('l1', 'cnc'):
            pix = TO.loop(y, masks, 50, kind, PRESETS[kind])[0]
            tmp = TO.loop(y, masks, 50, kind, PRESETS[kind], T)[0]
            llr = loop(y, masks, 50, kind, PRESETS[kind], T, b, table)[0]
            print('  %-3s 50 iterations: pixel prox %.2f dB, temporal prox %.2f dB, low-rank b = %d %.2f dB'
                  % (kind, psnr(pix, img), psnr(tmp, img), b, psnr(llr, img)))
    print('one prox step, float restatement by the Gram route and the Gram route in double (rel-L2 of z+ from the SVD in float64):')
    for T, H, W, b in ((5, 128, 130, 8), (16, 128, 128, 16), (64, 129, 131, 8), (17, 130, 129, 5)):
        x, z, w, _ = prox_inputs(1, T, H, W, b)
        for kind, pr in (('l1', PROX_L1), ('cnc', PROX_CNC)):
            ref = prox(kind, x, z, w, pr, T, b)[0]
            print('  T = %2d %dx%d b = %2d %-3s: float %.2e, double %.2e' % (T, H, W, b, kind, rel(prox(kind, x, z, w, pr, T, b, R=np.float32)[0], ref),
                                                                          rel(prox(kind, x, z, w, pr, T, b, route='gram')[0], ref)))
    print('float restatement of the loops at the presets (rel-L2 of x from the float64 oracle):')
    for S_, T, H, W in ((1, 5, 128, 130), (1, 8, 130, 129)):
        y, masks, _ = series_problem(S_, T, H, W)
        for kind in ('l1', 'cnc'):
            for n in (3, 5, 10):
                a, c = loop(y, masks, n, kind, PRESETS[kind], T, 8, 'random')[0], loop(y, masks, n, kind, PRESETS[kind], T, 8, 'random', R=np.float32)[0]
                print('  T = %2d %dx%d %-3s %2d iterations: %.2e' % (T, H, W, kind, n, rel(c, a)))


if __name__ == '__main__':
    measure()
