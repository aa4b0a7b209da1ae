"""NumPy oracle of the coil map estimation -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the text of include/pnp_mri.h ("coil sensitivity maps from the calibration region"), written from that text and not from
the kernels: the cos^2 window on the calibration region, the low-resolution coil images, the local dominant eigenvector by matrix-free
power iteration over the wrapped (2r+1)^2 patch, the phase rule and the support.  Everything takes ONE slice: y [C,H,W] complex
(un-shifted, DC at [0, 0]), mask [H,W].  `dt` = np.complex128 (the oracle) or np.complex64: the float32 restatement -- the same lines with
every intermediate array rounded to complex64 / float32 -- whose distance from the float64 form is the yardstick of the float GPU tests
(as tests/multicoil_oracle.py does for the x-step).
"""
import numpy as np

import coilmix_oracle as CO
import multicoil_oracle as M


def _real(dt):
    return np.float32 if dt == np.complex64 else np.float64


def window(ncal, dt=np.complex128):
    """w(f) = cos^2(pi f / (ncal + 1)) at the signed frequencies of the ncal calibration lines, in line order, rounded once to dt's real"""
    i = np.arange(ncal)
    f = np.where(i < (ncal + 1) // 2, i, i - ncal)
    return (np.cos(np.pi * f / (ncal + 1.0)) ** 2).astype(_real(dt))


def first_hole(mask, ncal):
    """None, or (h, k) of the calibration point of lowest offset that the mask does not sample"""
    H, W = mask.shape
    holes = np.argwhere(CO.cal_region(ncal, H, W) & (np.asarray(mask) == 0))
    return None if len(holes) == 0 else tuple(int(v) for v in holes[0])


def lowres(y, mask, ncal, dt=np.complex128):
    """I_c = ifft2(w_H (x) w_W . y_c on the calibration region, 0 elsewhere).  ValueError when the mask has a hole in the region."""
    C, H, W = y.shape
    hole = first_hole(mask, ncal)
    if hole is not None:
        raise ValueError('calibration point (%d, %d) is not sampled' % hole)
    R = _real(dt)
    rows, cols, w = CO.cal_lines(ncal, H), CO.cal_lines(ncal, W), window(ncal, dt)
    w2 = (w[:, None] * w[None, :]).astype(R)
    K = np.zeros((C, H, W), dt)
    K[np.ix_(np.arange(C), rows, cols)] = (w2[None] * np.asarray(y).astype(dt)[np.ix_(np.arange(C), rows, cols)]).astype(dt)
    return np.fft.ifft2(K, axes=(-2, -1)).astype(dt)


def _norm(a, R):
    """sqrt(sum_c |a_c|^2), the coils in order, every partial sum rounded"""
    s = np.zeros(a.shape[1:], R)
    for c in range(a.shape[0]):
        s = (s + (a[c].real.astype(R) ** 2).astype(R)).astype(R)
        s = (s + (a[c].imag.astype(R) ** 2).astype(R)).astype(R)
    return np.sqrt(s).astype(R)


def _dotc(a, b, dt):
    """sum_c conj(a_c) b_c, the coils in order, every partial sum rounded"""
    g = np.zeros(a.shape[1:], dt)
    for c in range(a.shape[0]):
        g = (g + (np.conj(a[c]) * b[c]).astype(dt)).astype(dt)
    return g


def _div(a, s):
    with np.errstate(all='ignore'):
        return a / np.where(s > 0, s, 1)


def eigmaps(I, r, n, dt=np.complex128):
    """-> (v [C,H,W] unit vectors with v^H I >= 0, lambda [H,W]): n power steps on R(p) = sum_{q in patch(p)} I(q) I(q)^H, never formed"""
    R = _real(dt)
    I = np.asarray(I).astype(dt)
    C = I.shape[0]
    nrm = _norm(I, R)
    e0 = np.zeros_like(I)
    e0[0] = 1
    v = np.where(nrm > 0, _div(I, nrm), e0).astype(dt)
    lam = np.zeros(I.shape[1:], R)
    for _ in range(n):
        u = np.zeros_like(I)
        for dy in range(-r, r + 1):                              # row-major patch order, wrapped on both axes
            for dx in range(-r, r + 1):
                Iq = np.roll(I, (-dy, -dx), axis=(1, 2))         # Iq[p] = I[p + (dy, dx)]
                g = _dotc(Iq, v, dt)
                u = (u + (Iq * g[None]).astype(dt)).astype(dt)
        lam = _norm(u, R)
        v = np.where(lam > 0, _div(u, lam), v).astype(dt)
    g = _dotc(v, I, dt)
    m = np.abs(g).astype(R)
    v = np.where(m > 0, (v * _div(g, m)[None]).astype(dt), v).astype(dt)
    return v, lam


def support(lam, thresh):
    R = lam.dtype.type
    return lam >= R(float(thresh) * float(thresh)) * lam.max()


def estimate(y, mask, ncal=24, r=2, n=4, thresh=0.05, dt=np.complex128, full=False):
    """-> maps [C,H,W] (zero outside the support); full=True: (maps, lambda, support, unmasked vectors, low-resolution images)"""
    I = lowres(y, mask, ncal, dt)
    v, lam = eigmaps(I, r, n, dt)
    sup = support(lam, thresh)
    S = np.where(sup[None], v, 0).astype(dt)
    return (S, lam, sup, v, I) if full else S


def problem_cal(seed, C, H, W, ncal=24, std=1.0):
    """multicoil_oracle.problem with the calibration square OR-ed into the mask and y synthesised with THAT mask.
    -> (img, S, mask, noise, y)"""
    img, S, m = M.phantom(seed, H, W), M.coil_maps(C, H, W, seed), M.mask(seed, H, W)
    m = (m.astype(bool) | CO.cal_region(ncal, H, W)).astype(np.uint8)
    nz = M.noise(seed, C, m, std)
    return img, S, m, nz, M.synthesize(img, S, m, nz)


def aligned_distance(S_est, S_true, body):
    """||S_est - S_true|| / ||S_true|| over the pixels of `body`: both sets have unit norm and the estimator fixes the phase so that
    v^H I >= 0, which for a real non-negative image is the phase of the true maps"""
    return M.rel(S_est[:, body], S_true[:, body])
