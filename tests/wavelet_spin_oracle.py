"""NumPy restatement of cycle spinning for the wavelet prox (include/pnp_mri.h, "cycle spinning"), for the tests: nothing but `np.roll`
around tests/wavelet_oracle.py's fwd / inv / prox_l1 / prox_cnc / dc_step, the averaging rule and the schedule.

Shift s = (sy, sx): (R_s v)[i, j] = v[(i + sy) mod H, (j + sx) mod W] = np.roll(v, (-sy, -sx), (-2, -1)); Psi_s = Psi R_s.  The shifted prox is
the unshifted one on rolled x, z, w, its z+ and w+ rolled back.  K > 1 shifts per prox: acc = z_0; acc += z_j, j = 1 .. K - 2, in order;
z+ = (acc + z_(K-1)) * r with r = 1 / K rounded once to `dtype`; w+ = (x + w) - z+.  Prox step p of a run uses table entries
(p mod (n / K)) K + j, j < K."""
import numpy as np

import wavelet_oracle as O

AX = (-2, -1)


def shifts_of(levels):
    """the five shifts every test uses: none, one row, one column, the largest, and a mixed one"""
    m = 1 << levels
    return ((0, 0), (1, 0), (0, 1), (m - 1, m - 1), (3 % m, 5 % m))


def roll_in(v, s):
    """R_s v: into the shifted frame"""
    return np.roll(v, (-int(s[0]), -int(s[1])), AX)


def roll_out(v, s):
    """R_s^T v: back"""
    return np.roll(v, (int(s[0]), int(s[1])), AX)


def fwd(v, name, levels, s, dtype=np.float64):
    """Psi_s v"""
    return O.fwd(roll_in(np.asarray(v), s), name, levels, dtype)


def inv(c, name, levels, s, dtype=np.float64):
    """Psi_s^T c"""
    return roll_out(O.inv(c, name, levels, dtype), s)


def _one(kind, x, z, w, params, name, levels, s, dtype):
    xs, zs, ws = (roll_in(np.asarray(a, dtype), s) for a in (x, z, w))
    if kind == 'l1':
        zn, wn = O.prox_l1(xs, zs, ws, params['thr'], name, levels, dtype)
    else:
        zn, wn = O.prox_cnc(xs, zs, ws, params['alpha'], params['lambda1'], params['reo'], params['b'], name, levels, dtype)
    return roll_out(zn, s), roll_out(wn, s)


def prox(kind, x, z, w, params, name, levels, shifts, dtype=np.float64):
    """-> (z+, w+) of one prox step that averages the K = len(shifts) shifts.  kind 'l1': params = dict(thr); 'cnc': dict(alpha, lambda1,
    reo, b)."""
    K = len(shifts)
    if K == 1:
        return _one(kind, x, z, w, params, name, levels, shifts[0], dtype)
    zs = [_one(kind, x, z, w, params, name, levels, s, dtype)[0] for s in shifts]
    acc = zs[0]
    for j in range(1, K - 1):
        acc = acc + zs[j]
    zn = ((acc + zs[K - 1]) * dtype(1.0 / K)).astype(dtype)
    u = np.asarray(x, dtype) + np.asarray(w, dtype)
    return zn, u - zn


def group(table, per_prox, p):
    """the shifts of prox step p"""
    table = np.asarray(table)
    first = (p % (len(table) // per_prox)) * per_prox
    return [tuple(int(v) for v in table[first + j]) for j in range(per_prox)]


def loop(y, mask, iters, kind, params, name, levels, table=None, per_prox=1, dtype=np.float64, cursor=0):
    """wavelet_oracle.loop with the prox of iteration i in the frames of group(table, per_prox, cursor + i); table None: no spin.
    params as wavelet_oracle.loop's.  -> (x, z, w)"""
    if table is None:
        return O.loop(y, mask, iters, kind, params, name, levels, dtype)
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    y = np.asarray(y, cdt)
    z = np.abs(np.fft.ifft2(y)).astype(dtype)
    w = np.zeros_like(z)
    x = z.copy()
    pp = dict(thr=params['reo'] * params['lambda1']) if kind == 'l1' else params
    for i in range(iters):
        x = O.dc_step(y, mask, z, w, params['reo'], dtype)
        z, w = prox(kind, x, z, w, pp, name, levels, group(table, per_prox, cursor + i), dtype)
    return x, z, w


def psnr(x, img):
    """PSNR of x against img, both on [0, 1] (peak 1)"""
    return float(10.0 * np.log10(1.0 / np.mean((np.asarray(x, np.float64) - img) ** 2)))


def point_problem():
    """The inputs of the issue's 'point of the feature' measurement, all seeded: -> (img [128,128] in [0,1], y [1,128,128] complex128,
    mask [128,128] uint8)."""
    img = O.phantom(1, 128, 128, seed=5)[0]
    img = img / img.max()
    rng = np.random.default_rng(3)
    mask = rng.random((128, 128)) < 0.3
    mask[:4] = True
    mask[124:] = True
    noise = 0.5 * (rng.standard_normal((128, 128)) + 1j * rng.standard_normal((128, 128)))
    y = (np.fft.fft2(img) + noise) * mask
    return img, y[None], mask.astype(np.uint8)


POINT = dict(name='haar', levels=3, iters=50, seed=99, params=dict(lambda1=0.2, reo=0.05))
