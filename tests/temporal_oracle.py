"""NumPy oracle of the temporal-sparsity prox and its loops -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the mathematics of include/pnp_mri.h ("temporal sparsity"), written from that text and not from the kernels:

    batch = S series of T consecutive slices, slice b = s T + t;  u = x + w;  U_k = T^(-1/2) sum_t u_t e^(-2 pi i k t / T)
    L1:  Z_k = csoft(U_k, thr)       CNC:  Z_k = csoft(c1 z^_k + c2 U_k + c3 cclip(z^_k, ib), thr),  z^ = F z
    keep_dc:  Z_0 = U_0 (not the CNC combination);   z+ = F^H Z;   w+ = u - z+
    real images: k = 0 .. T // 2 only, z+_t = T^(-1/2) [Z_0 + 2 sum_{0<k<T/2} Re(Z_k e^(+2 pi i k t / T)) + (T even) Z_(T/2) (-1)^t],
                 the real coefficients (0 and T / 2) take soft / clip

R = np.float64 is the oracle: the sums are products with the DFT matrix built from the twiddle table.  R = np.float32 is the float
restatement -- the same direct sums, t resp. k ascending, every product and every sum rounded to float32 -- whose distance from the
oracle ON THE SAME CASE sets the bar of a float GPU test (4 x that distance; DESIGN.md sections 13, 20).

`python tests/temporal_oracle.py` re-measures the PSNR table of DESIGN.md's temporal section and the float restatement's distances
of the loops at the presets (CPU only).
"""
import os
import sys

import numpy as np

if __name__ == '__main__':                      # run as a script: the repository root, for multicoil_oracle's `oracle` package
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import complex_oracle as CO
import multicoil_oracle as M
import wavelet_oracle as WO

PRESETS = M.O_PRESETS                          # l1: lambda1 0.1, reo 0.015;  cnc: alpha 0.45, lambda1 0.5, reo 0.05, b 64
MIN_FRAMES, MAX_FRAMES = 2, 64


def _cdt(R):
    return np.complex128 if R == np.float64 else np.complex64


def twiddles(T, R=np.float64):
    """cos, sin (2 pi j / T), j < T: computed in double, rounded once to R"""
    a = 2.0 * np.pi * np.arange(T, dtype=np.float64) / float(T)
    return np.cos(a).astype(R), np.sin(a).astype(R)


def coefs(T, cx):
    return T if cx else T // 2 + 1


def _cpx(re, im, R):
    out = np.empty(re.shape, _cdt(R))
    out.real, out.imag = re, im
    return out


def analysis(u, R=np.float64, cx=False):
    """u [S, T, ...] (real, or complex with cx) -> U [S, K, ...] complex"""
    T = u.shape[1]
    K, (c, s), scale = coefs(T, cx), twiddles(T, R), R(1.0 / np.sqrt(float(T)))
    if R == np.float64:
        j = np.outer(np.arange(K), np.arange(T)) % T
        U = scale * np.einsum('kt,st...->sk...', c[j] - 1j * s[j], u)
    else:
        re = np.zeros((u.shape[0], K) + u.shape[2:], R)
        im = np.zeros_like(re)
        for k in range(K):
            for t in range(T):
                j = (k * t) % T
                if cx:
                    re[:, k] = re[:, k] + u[:, t].real * c[j]
                    re[:, k] = re[:, k] + u[:, t].imag * s[j]
                    im[:, k] = im[:, k] + u[:, t].imag * c[j]
                    im[:, k] = im[:, k] - u[:, t].real * s[j]
                else:
                    re[:, k] = re[:, k] + u[:, t] * c[j]
                    im[:, k] = im[:, k] - u[:, t] * s[j]
        U = _cpx(re * scale, im * scale, R)
    if not cx:                                  # the real coefficients
        U[:, 0].imag = 0
        if T % 2 == 0:
            U[:, T // 2].imag = 0
    return U


def synthesis(Z, T, R=np.float64, cx=False):
    """Z [S, K, ...] -> z+ [S, T, ...]"""
    (c, s), scale = twiddles(T, R), R(1.0 / np.sqrt(float(T)))
    if cx:
        if R == np.float64:
            j = np.outer(np.arange(T), np.arange(T)) % T
            return scale * np.einsum('tk,sk...->st...', c[j] + 1j * s[j], Z)
        re = np.zeros((Z.shape[0], T) + Z.shape[2:], R)
        im = np.zeros_like(re)
        for t in range(T):
            for k in range(T):
                j = (k * t) % T
                re[:, t] = re[:, t] + Z[:, k].real * c[j]
                re[:, t] = re[:, t] - Z[:, k].imag * s[j]
                im[:, t] = im[:, t] + Z[:, k].real * s[j]
                im[:, t] = im[:, t] + Z[:, k].imag * c[j]
        return _cpx(re * scale, im * scale, R)
    out = np.zeros((Z.shape[0], T) + Z.shape[2:], R)
    for t in range(T):
        acc = np.zeros((Z.shape[0],) + Z.shape[2:], R)
        for k in range(1, (T + 1) // 2):
            j = (k * t) % T
            acc = acc + Z[:, k].real * c[j]
            acc = acc - Z[:, k].imag * s[j]
        v = R(2) * acc + Z[:, 0].real
        if T % 2 == 0:
            v = v - Z[:, T // 2].real if t & 1 else v + Z[:, T // 2].real
        out[:, t] = scale * v
    return out


def soft(a, thr):
    return np.sign(a) * np.maximum(np.abs(a) - thr, 0)


def prox(kind, x, z, w, pr, T, keep_dc=True, R=np.float64, cx=False, spectrum=False):
    """one prox step on a batch [B, ...], B a multiple of T.  kind 'l1': pr = dict(lambda1, reo); 'cnc': dict(alpha, lambda1, reo, b).
    -> (z+, w+) in R (complex of R with cx); spectrum: -> (z+, w+, Z [S, K, ...])"""
    cdt = _cdt(R)
    vt = cdt if cx else R
    x, w = np.asarray(x).astype(vt), np.asarray(w).astype(vt)
    B = x.shape[0]
    if T < MIN_FRAMES or T > MAX_FRAMES or B % T:
        raise ValueError('bad frames')
    ser = lambda a: a.reshape((B // T, T) + a.shape[1:])
    u = x + w
    U = analysis(ser(u), R, cx)
    real = [0] + ([T // 2] if T % 2 == 0 else []) if not cx else []
    if kind == 'l1':
        thr, t = R(pr['reo'] * pr['lambda1']), U
    else:
        thr, c1, c2, c3, ib = CO.cnc_scalars(pr['alpha'], pr['lambda1'], pr['reo'], pr['b'], cdt)
        zh = analysis(ser(np.asarray(z).astype(vt)), R, cx)
        t = CO._combine(zh, U, c1, c2, c3, ib, cdt)
        for k in real:
            t[:, k] = c1 * zh[:, k].real + (c2 * U[:, k].real + c3 * np.clip(zh[:, k].real, -ib, ib))
    Z = CO.csoft(t, thr, cdt)
    for k in real:
        Z[:, k] = soft(t[:, k].real, thr)
    if keep_dc:
        Z[:, 0] = U[:, 0]
    zn = synthesis(Z, T, R, cx).reshape(u.shape).astype(vt)
    return (zn, (u - zn).astype(vt), Z) if spectrum else (zn, (u - zn).astype(vt))


def structural_zeros(kind, x, z, w, pr, T, keep_dc=True, cx=False):
    """-> bool [B, ...]: where z+ is zero in ANY arithmetic -- the pixel-series whose thresholded coefficients are ALL exactly zero in the
    float64 oracle (a sum of zeros is zero whatever its order).  Not counted: a series whose surviving coefficient is an unpenalised
    mean that vanishes by cancellation alone (keep_dc: the series must then be identically zero), single frames that come out zero
    by cancellation in the synthesis, and the pixels of at_threshold_pixels -- all of these are zero or not by the last bit of a sum,
    and are held by the error bar."""
    Z = prox(kind, x, z, w, pr, T, keep_dc, cx=cx, spectrum=True)[2]
    B = np.shape(x)[0]
    dead = (Z == 0).all(axis=1)                                                       # [S, ...]
    if keep_dc:
        u = (np.asarray(x) + np.asarray(w)).reshape((B // T, T) + np.shape(x)[1:])
        dead &= (u == 0).all(axis=1)
    out = np.repeat(dead[:, None], T, axis=1).reshape(np.shape(x))
    out.reshape(B, -1)[:, list(at_threshold_pixels(T))] = False
    return out


def prox_full_spectrum(kind, x, z, w, pr, T, keep_dc=True):
    """the prox of a REAL batch through the full complex spectrum (np.fft.fft along time, unitary), float64: what the k <= T / 2 form
    above must equal"""
    x, z, w = (np.asarray(a, np.float64) for a in (x, z, w))
    B = x.shape[0]
    ser = lambda a: a.reshape((B // T, T) + a.shape[1:])
    u = x + w
    U = np.fft.fft(ser(u), axis=1, norm='ortho')
    if kind == 'l1':
        thr, t = pr['reo'] * pr['lambda1'], U
    else:
        thr, c1, c2, c3, ib = CO.cnc_scalars(pr['alpha'], pr['lambda1'], pr['reo'], pr['b'])
        zh = np.fft.fft(ser(z), axis=1, norm='ortho')
        t = c1 * zh + c2 * U + c3 * CO.cclip(zh, ib)
    Z = CO.csoft(t, thr)
    if keep_dc:
        Z[:, 0] = U[:, 0]
    zn = np.fft.ifft(Z, axis=1, norm='ortho')
    assert np.abs(zn.imag).max() <= 1e-12 * max(1.0, np.abs(zn.real).max())
    zn = zn.real.reshape(u.shape)
    return zn, u - zn


# ---- the loops -----------------------------------------------------------------------------------------------------------------------

def pixel_prox(kind, x, z, w, pr, R=np.float64):
    """the pixel-domain step of oracle/admm_oracle.py on a real batch (the baseline of the PSNR table)"""
    x, z, w = (np.asarray(a, R) for a in (x, z, w))
    u = x + w
    if kind == 'l1':
        zn = soft(u, R(pr['reo'] * pr['lambda1']))
    else:
        thr, c1, c2, c3, ib = CO.cnc_scalars(pr['alpha'], pr['lambda1'], pr['reo'], pr['b'], _cdt(R))
        zn = soft(c1 * z + (c2 * u + c3 * np.clip(z, -ib, ib)), thr)
    return zn.astype(R), (u - zn).astype(R)


def loop(y, masks, iters, kind, pr, T=None, keep_dc=True, R=np.float64, z0=None, w0=None, states=()):
    """`iters` iterations of x = dc(z, w); (z, w) = prox(x, z, w) without coils, from z0 = |ifft2(y)|, w0 = 0.  y [B, H, W], masks
    [B, H, W] (the mask of every slice).  T = None: the pixel prox.  -> (x, z, w); states: iterations k at which (x, z, z_prev, w) are
    appended to the returned list (a fourth value)"""
    y = np.asarray(y, _cdt(R))
    z = np.abs(np.fft.ifft2(y)).astype(R) if z0 is None else np.asarray(z0, R)
    w = np.zeros_like(z) if w0 is None else np.asarray(w0, R)
    x, kept = z.copy(), []
    for k in range(1, iters + 1):
        zp = z
        x = WO.dc_step(y, masks, z, w, pr['reo'], R)
        z, w = pixel_prox(kind, x, z, w, pr, R) if T is None else prox(kind, x, z, w, pr, T, keep_dc, R)
        if k in states:
            kept.append((x, z, zp, w))
    return (x, z, w, kept) if states else (x, z, w)


def coil_loop(y, S, masks, iters, kind, pr, T, keep_dc=True, R=np.float64, cx=False, cg_iters=3):
    """the same with the multi-coil x-step (tests/multicoil_oracle.py; cx: tests/complex_oracle.py), one coil set S [C, H, W] for every
    slice.  y [B, C, H, W], masks [B, H, W] -> (x, z, w)"""
    dt, O = _cdt(R), (CO if cx else M)
    B = y.shape[0]
    st = [O.init_state(y[b], S, masks[b], dt) for b in range(B)]
    aty, z, w = (np.stack([s[i] for s in st]) for i in range(3))
    x = z.copy()
    for _ in range(iters):
        x = np.stack([O.x_step(z[b], w[b], aty[b], S, masks[b], pr['reo'], cg_iters, dt) for b in range(B)])
        z, w = prox(kind, x, z, w, pr, T, keep_dc, R, cx)
    return x, z, w


# ---- the dynamic phantom of DESIGN.md's PSNR table -------------------------------------------------------------------------------------

def dynamic_phantom(T, H, W):
    """[T, H, W] float64 in [0, 1]: a static body (an ellipse with two inserts), one disc whose radius beats and one disc that moves on a
    circle, both with period T"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (yy - H / 2) / H, (xx - W / 2) / W
    body = 0.35 * ((u / 0.40) ** 2 + (v / 0.32) ** 2 <= 1.0)
    body = body + 0.20 * (((u + 0.15) / 0.10) ** 2 + ((v - 0.05) / 0.16) ** 2 <= 1.0) - 0.25 * ((u - 0.2) ** 2 + (v + 0.1) ** 2 <= 0.06 ** 2)
    out = np.empty((T, H, W))
    for t in range(T):
        ph = 2.0 * np.pi * t / T
        r = 0.07 + 0.015 * np.sin(ph)
        beat = 0.20 * ((u + 0.02) ** 2 + (v + 0.12) ** 2 <= r * r)
        cu, cv = 0.05 + 0.03 * np.cos(ph), 0.14 + 0.03 * np.sin(ph)
        move = 0.20 * ((u - cu) ** 2 + (v - cv) ** 2 <= 0.045 ** 2)
        out[t] = np.clip(body + beat + move, 0.0, 1.0)
    return out


def column_masks(T, H, W, rate=0.28, centre=13, seed=0):
    """[T, H, W] uint8: another random set of columns per frame, `rate` of them sampled, the `centre` columns around DC (un-shifted
    layout) always"""
    rng = np.random.default_rng(4100 + seed)
    out = np.zeros((T, H, W), np.uint8)
    dc = [(c - centre // 2) % W for c in range(centre)]
    for t in range(T):
        cols = np.zeros(W, bool)
        cols[dc] = True
        rest = np.flatnonzero(~cols)
        cols[rng.choice(rest, max(0, int(round(rate * W)) - centre), replace=False)] = True
        out[t][:, cols] = 1
    return out


def dynamic_problem(T, H, W, sigma=1.0, seed=0):
    """-> (img [T, H, W] float64, masks [T, H, W] uint8, y [T, H, W] complex64): y = mask . fft2(img) + mask . noise.  y holds float32
    values, so a float engine, a double engine and the oracle all start from the same numbers"""
    rng = np.random.default_rng(8800 + seed)
    img, masks = dynamic_phantom(T, H, W), column_masks(T, H, W, seed=seed)
    nz = sigma * (rng.standard_normal((T, H, W)) + 1j * rng.standard_normal((T, H, W)))
    return img, masks, ((np.fft.fft2(img) + nz) * masks).astype(np.complex64)


def psnr(x, ref):
    """of images in [0, 1], over the whole batch"""
    return float(10.0 * np.log10(1.0 / np.mean((np.asarray(x, np.float64) - ref) ** 2)))


rel = M.rel


# ---- shared inputs of tests/test_gpu_temporal.py -------------------------------------------------------------------------------------

PROX_L1 = dict(lambda1=0.5, reo=0.6)                               # thr = 0.3
PROX_CNC = dict(alpha=0.45, lambda1=0.5, reo=1.0, b=4.0)           # thr = 0.225, clip at 1 / b = 0.25: both sides of both populated


def prox_inputs(S, T, H, W, cx=False, seed=0):
    """x, z, w [S T, H, W] (complex with cx) holding float32 values: random data, every series different, and -- in the first pixels of
    every series -- a designed set: pixel 0 all zero (the oracle's z+ is exactly 0), 1 far below every threshold, 2 a temporal impulse in
    frame 1, 3 .. 3 + T - 1 a pure harmonic at each k, then harmonics k = 1 with |U_1| at thr (1 - 1e-3), thr, thr (1 + 1e-3) for both
    thresholds and z harmonics with |z^_1| at ib (1 - 1e-3), ib, ib (1 + 1e-3).  w = 0 and x = u on the designed pixels."""
    rng = np.random.default_rng(9000 + 131 * T + 7 * S + H + W + seed)
    B, N = S * T, H * W
    g = lambda sc: sc * rng.standard_normal((S, T, N)) + (1j * sc * rng.standard_normal((S, T, N)) if cx else 0)
    x, z, w = g(0.5), g(0.5), g(0.3)
    t = np.arange(T)
    wave = lambda k, ph=0.0: np.exp(2j * np.pi * k * t / T + 1j * ph) if cx else np.cos(2 * np.pi * k * t / T + ph)
    # |U_k| of a unit wave: sqrt(T) for a complex exponential and for the real coefficients 0 and T / 2, sqrt(T) / 2 for a real cosine
    gain = lambda k: np.sqrt(T) if (cx or k == 0 or 2 * k == T) else np.sqrt(T) / 2
    cols = [np.zeros(T), 1e-3 * wave(1, 0.3), 2.0 * (t == 1)]
    cols += [0.8 * wave(k, 0.2 * k) for k in range(T)]
    for thr in (PROX_L1['reo'] * PROX_L1['lambda1'], PROX_CNC['alpha'] * PROX_CNC['reo'] * PROX_CNC['lambda1']):
        cols += [thr * f / gain(1 % T) * wave(1, 0.7) for f in (1 - 1e-3, 1.0, 1 + 1e-3)]
    zcols = [(1.0 / PROX_CNC['b']) * f / gain(1 % T) * wave(1, 1.1) for f in (1 - 1e-3, 1.0, 1 + 1e-3)]
    for s_ in range(S):
        for i, c in enumerate(cols):
            x[s_, :, i], w[s_, :, i], z[s_, :, i] = (1.0 + 0.1 * s_) * c, 0, 0
        for i, c in enumerate(zcols):
            z[s_, :, len(cols) + i] = c
    dt = np.complex64 if cx else np.float32
    return tuple(a.reshape(B, H, W).astype(dt).astype(np.complex128 if cx else np.float64) for a in (x, z, w))


def at_threshold_pixels(T):
    """the pixels of prox_inputs whose designed coefficient sits EXACTLY at a threshold (|U_1| = thr for either thr, |z^_1| = ib): which
    side they fall on is decided by the last bit of a sum, so they are held by the error bar alone, never by an exact comparison"""
    first = 3 + T
    return (first + 1, first + 4, first + 7)


def series_problem(S, T, H, W, C=0, cx=False, seed=0):
    """-> (y, masks [S T, H, W] uint8, maps [C, H, W] or None): S series of the dynamic phantom (every series scaled and rolled
    differently; with cx times the phase of tests/complex_oracle.py), another column mask on every slice, complex noise of sigma 1 on
    the sampled points.  y [S T, H, W], or [S T, C, H, W] through the coil maps of tests/multicoil_oracle.py; complex128 holding float32
    values"""
    rng = np.random.default_rng(6600 + seed + 31 * T + S)
    base = dynamic_phantom(T, H, W)
    img = np.concatenate([(1.0 - 0.15 * s_) * np.roll(base, (3 * s_, -2 * s_), axis=(1, 2)) for s_ in range(S)])
    if cx:
        img = img * np.exp(1j * CO.phase(H, W))
    masks = column_masks(S * T, H, W, seed=seed + T)
    nz = lambda shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if C == 0:
        y = (np.fft.fft2(img) + nz(img.shape)) * masks
        maps = None
    else:
        maps = M.coil_maps(C, H, W, seed).astype(np.complex64).astype(np.complex128)
        y = np.stack([M.A(img[b], maps, masks[b]) + nz((C, H, W)) * masks[b] for b in range(S * T)])
    return y.astype(np.complex64).astype(np.complex128), masks, maps


def measure():
    for T, H, W in ((16, 128, 128), (5, 128, 130)):
        img, masks, y = dynamic_problem(T, H, W)
        print('%d frames of %d x %d: zero-filled %.2f dB' % (T, H, W, psnr(np.abs(np.fft.ifft2(y)), img)))
        for kind in ('l1', 'cnc'):
            pix = loop(y, masks, 50, kind, PRESETS[kind])[0]
            tmp = loop(y, masks, 50, kind, PRESETS[kind], T)[0]
            print('  %-3s 50 iterations: pixel prox %.2f dB, temporal prox %.2f dB' % (kind, psnr(pix, img), psnr(tmp, img)))
    print('float restatement of ten iterations at the presets (rel-L2 of x from the float64 oracle):')
    for T, H, W in ((5, 128, 130), (16, 128, 128)):
        img, masks, y = dynamic_problem(T, H, W, seed=1)
        for kind in ('l1', 'cnc'):
            for n in (3, 5, 10):
                a, b = loop(y, masks, n, kind, PRESETS[kind], T)[0], loop(y, masks, n, kind, PRESETS[kind], T, R=np.float32)[0]
                print('  T = %2d %dx%d %-3s %2d iterations: %.2e' % (T, H, W, kind, n, rel(b, a)))


if __name__ == '__main__':
    measure()
