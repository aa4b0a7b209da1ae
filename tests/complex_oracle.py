"""NumPy oracle of the complex-valued image mode -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the mathematics of include/pnp_mri.h ("complex-valued images on a coil context"), written from that text and not from
the kernels, on top of tests/multicoil_oracle.py (operators, CG) and tests/wavelet_oracle.py (Psi):

    state x, z, w complex;  z0 = A^H y, w0 = 0;  x-step: G x^ = A^H y + La2 (z - w) by CG warm-started at z - w, x = x^
    csoft(u, c) = u (|u| - c) / |u| where |u| > c, else 0;   cclip(z, ib) = z ib / |z| where |z| > ib, else z
    L1:  u = x + w, z+ = csoft(u, thr), w+ = u - z+          CNC:  t = c1 z + c2 u + c3 cclip(z, ib), z+ = csoft(t, thr), w+ = u - z+
    wavelet: Psi on the real and the imaginary part alike; the steps above on the detail coefficients, the approximation passes through

Everything takes ONE slice.  `dt` = np.complex128 (the oracle) or np.complex64 (the float restatement: every intermediate array rounded
to complex64 / float32), whose distance from the oracle sets the bars of the float GPU tests -- tests/multicoil_oracle.py's convention.
"""
import numpy as np

import multicoil_oracle as M
import wavelet_oracle as W

_real = M._real
O_PRESETS = M.O_PRESETS


# ---- the phase phantom ---------------------------------------------------------------------------------------------------------------

def phase(H, W_, strong=False):
    """phi = 0.9 sin(2 pi 3 u) cos(2 pi 2 v) + (pi / 2) [(u - 0.05)^2 + (v + 0.08)^2 <= 0.1^2], u = (row - H/2) / H, v = (col - W/2) / W;
    strong: sine amplitude 2.5 and a ramp 2 pi (1.5 u - v) on top"""
    yy, xx = np.mgrid[0:H, 0:W_].astype(np.float64)
    u, v = (yy - H / 2) / H, (xx - W_ / 2) / W_
    phi = (2.5 if strong else 0.9) * np.sin(2 * np.pi * 3 * u) * np.cos(2 * np.pi * 2 * v)
    phi = phi + (np.pi / 2) * (((u - 0.05) ** 2 + (v + 0.08) ** 2) <= 0.1 ** 2)
    if strong:
        phi = phi + 2 * np.pi * (1.5 * u - v)
    return phi


def truth(seed, H, W_, strong=False):
    """multicoil_oracle.phantom(seed) . e^{i phi}, complex128"""
    return M.phantom(seed, H, W_).astype(np.float64) * np.exp(1j * phase(H, W_, strong))


def problem(seed, C, H, W_, std=1.0, strong=False, real=False):
    """-> (truth complex128 [H,W], S [C,H,W], mask uint8 [H,W], y [C,H,W] complex128); real: the phantom without the phase"""
    S, m = M.coil_maps(C, H, W_, seed), M.mask(seed, H, W_)
    t = M.phantom(seed, H, W_).astype(np.complex128) if real else truth(seed, H, W_, strong)
    return t, S, m, M.A(t, S, m) + M.noise(seed, C, m, std)


# ---- the prox on complex numbers -----------------------------------------------------------------------------------------------------

def _c(re, im, dt):
    out = np.empty(np.shape(re), dt)
    out.real, out.imag = re, im
    return out


def cabs(u, dt=np.complex128):
    """two rounded products, one sum, one square root"""
    R = _real(dt)
    u = np.asarray(u).astype(dt)
    a, b = (u.real * u.real).astype(R), (u.imag * u.imag).astype(R)
    return np.sqrt((a + b).astype(R)).astype(R)


def csoft(u, c, dt=np.complex128):
    R = _real(dt)
    u, c = np.asarray(u).astype(dt), R(c)
    m = cabs(u, dt)
    big = m > c
    with np.errstate(all='ignore'):
        s = np.where(big, ((m - c).astype(R) / np.where(big, m, R(1))).astype(R), R(0)).astype(R)
    return _c((s * u.real).astype(R), (s * u.imag).astype(R), dt)


def cclip(z, ib, dt=np.complex128):
    R = _real(dt)
    z, ib = np.asarray(z).astype(dt), R(ib)
    m = cabs(z, dt)
    big = m > ib
    with np.errstate(all='ignore'):
        f = (ib / np.where(big, m, R(1))).astype(R)
    return _c(np.where(big, (z.real * f).astype(R), z.real), np.where(big, (z.imag * f).astype(R), z.imag), dt)


def cnc_scalars(alpha, lambda1, reo, b, dt=np.complex128):
    """thr, c1, c2, c3, ib: combined in double, rounded once"""
    R = _real(dt)
    return R(alpha * reo * lambda1), R(1.0 - alpha), R(alpha), R(alpha * reo * lambda1 * b), R(1.0 / b)


def _combine(z, u, c1, c2, c3, ib, dt):
    """c1 z + (c2 u + c3 cclip(z, ib)), component-wise"""
    cl = cclip(z, ib, dt)
    return (c1 * z + (c2 * u + (c3 * cl).astype(dt)).astype(dt)).astype(dt)


def l1_step(x, z, w, thr, dt=np.complex128):
    u = (np.asarray(x).astype(dt) + np.asarray(w).astype(dt)).astype(dt)
    zn = csoft(u, thr, dt)
    return zn, (u - zn).astype(dt)


def cnc_step(x, z, w, alpha, lambda1, reo, b, dt=np.complex128):
    thr, c1, c2, c3, ib = cnc_scalars(alpha, lambda1, reo, b, dt)
    z = np.asarray(z).astype(dt)
    u = (np.asarray(x).astype(dt) + np.asarray(w).astype(dt)).astype(dt)
    zn = csoft(_combine(z, u, c1, c2, c3, ib, dt), thr, dt)
    return zn, (u - zn).astype(dt)


# ---- the wavelet prox ----------------------------------------------------------------------------------------------------------------

def psi(v, name, levels, dt=np.complex128, inverse=False):
    """Psi (Psi^T) on the real and the imaginary part alike"""
    R, f = _real(dt), (W.inv if inverse else W.fwd)
    v = np.asarray(v).astype(dt)
    return _c(f(v.real, name, levels, R), f(v.imag, name, levels, R), dt)


def wl1_step(x, z, w, thr, name, levels, dt=np.complex128):
    u = (np.asarray(x).astype(dt) + np.asarray(w).astype(dt)).astype(dt)
    c = psi(u, name, levels, dt)
    c = np.where(W.detail_mask(*c.shape[-2:], levels), csoft(c, thr, dt), c)
    zn = psi(c, name, levels, dt, inverse=True)
    return zn, (u - zn).astype(dt)


def wcnc_step(x, z, w, alpha, lambda1, reo, b, name, levels, dt=np.complex128):
    thr, c1, c2, c3, ib = cnc_scalars(alpha, lambda1, reo, b, dt)
    u = (np.asarray(x).astype(dt) + np.asarray(w).astype(dt)).astype(dt)
    cz, cu = psi(z, name, levels, dt), psi(u, name, levels, dt)
    det = W.detail_mask(*cz.shape[-2:], levels)
    approx = (c1 * cz + (c2 * cu).astype(dt)).astype(dt)
    c = np.where(det, csoft(_combine(cz, cu, c1, c2, c3, ib, dt), thr, dt), approx)
    zn = psi(c, name, levels, dt, inverse=True)
    return zn, (u - zn).astype(dt)


# ---- the loops -----------------------------------------------------------------------------------------------------------------------

def init_state(y, S, m, dt=np.complex128):
    """-> (aty, z0 = A^H y, w0 = 0)"""
    aty = M.AH(np.asarray(y).astype(dt), S, m, dt)
    return aty, aty.copy(), np.zeros_like(aty)


def x_step(z, w, aty, S, m, reo, iters=3, dt=np.complex128, residual=False):
    v = (np.asarray(z).astype(dt) - np.asarray(w).astype(dt)).astype(dt)
    xh, rel = M.cg_solve(aty, v, S, m, reo, iters, dt)
    return (xh, rel) if residual else xh


def prox(kind, x, z, w, pr, dt=np.complex128, transform=None, levels=3):
    if kind == 'l1':
        thr = pr['reo'] * pr['lambda1']
        return l1_step(x, z, w, thr, dt) if transform is None else wl1_step(x, z, w, thr, transform, levels, dt)
    a = (pr['alpha'], pr['lambda1'], pr['reo'], pr['b'])
    return cnc_step(x, z, w, *a, dt) if transform is None else wcnc_step(x, z, w, *a, transform, levels, dt)


def admm(y, S, m, iter_num, kind, cg_iters=3, dt=np.complex128, transform=None, levels=3, state=False, **par):
    """ADMM_L1 (kind 'l1') / ADMM_CNC (kind 'cnc') in complex image mode at O_PRESETS (overridden by **par) -> x, or (x, z, w)"""
    pr = dict(O_PRESETS[kind], **par)
    aty, z, w = init_state(y, S, m, dt)
    x = z.copy()
    for _ in range(iter_num):
        x = x_step(z, w, aty, S, m, pr['reo'], cg_iters, dt)
        z, w = prox(kind, x, z, w, pr, dt, transform, levels)
    return (x, z, w) if state else x


rel = M.rel


def mag_err(x, t):
    """|| |x| - |truth| || / ||truth||"""
    return float(np.linalg.norm(np.abs(x) - np.abs(t)) / np.linalg.norm(t))
