"""NumPy oracle of the multi-coil (SENSE) data consistency -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the mathematics of include/pnp_mri.h ("multi-coil (SENSE) data consistency"), written from that text and not from the
kernels: fft2 unnormalised, ifft2 carries 1/N, La2 = 1/(2 reo), v = z - w real.

    (A x)_c = m . fft2(S_c . x)        A^H k = sum_c conj(S_c) . ifft2(m . k_c)        G p = A^H A p + La2 p
    x-step: G x^ = A^H y + La2 v by `iters` iterations of plain CG warm-started at x^ = v;  x = |Re x^|
    initial state: z = |A^H y|, w = 0;  z- and w-steps: oracle/admm_oracle.py's (pixels) or tests/wavelet_oracle.py's (wavelet)

Everything takes ONE slice: S [C,H,W] complex, mask [H,W], y [C,H,W].  `dt` = np.complex128 (the oracle) or np.complex64: the float32
restatement -- the same lines with every intermediate array rounded to complex64 / float32 and every scalar to float32 -- whose distance
from the float64 form is the yardstick of the float GPU tests (as tests/wavelet_oracle.py does for the wavelet prox).
"""
import numpy as np

from oracle import admm_oracle as O


def _real(dt):
    return np.float32 if dt == np.complex64 else np.float64


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------

def phantom(seed, H, W):
    """ellipse plus disc plus texture in [0, 1], float32 on the 1/255 grid (what the solvers' re-quantisation leaves unchanged)"""
    rng = np.random.default_rng(9100 + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (yy - H / 2) / H, (xx - W / 2) / W
    img = 0.55 * (((u / 0.38) ** 2 + (v / 0.30) ** 2) <= 1.0)
    cy, cx = rng.uniform(-0.12, 0.12, 2)
    img = img + 0.3 * (((u - cy) ** 2 + (v - cx) ** 2) <= 0.11 ** 2)
    fy, fx = rng.uniform(6, 14, 2)
    img = img + 0.08 * np.sin(2 * np.pi * fy * u + rng.uniform(0, 6)) * np.cos(2 * np.pi * fx * v) * (img > 0)
    return np.float32(np.round(np.clip(img, 0, 1) * 255.) / 255.)


def mask(seed, H, W, rate=0.30, border=6):
    """`rate` of the k-space points at random plus `border` full lines around DC (un-shifted layout: the first and last border / 2 rows)"""
    rng = np.random.default_rng(5200 + seed)
    m = rng.uniform(size=(H, W)) < rate
    m[:border // 2, :] = True
    m[H - border // 2:, :] = True
    return m.astype(np.uint8)


def coil_maps(C, H, W, seed=0):
    """coil c: a Gaussian magnitude (sigma 0.45 of the field of view) centred on a circle of radius 0.6 at angle 2 pi c / C + 0.3, times a
    linear phase ramp; normalised to sum_c |S_c|^2 = 1.  -> [C,H,W] complex128"""
    rng = np.random.default_rng(7300 + seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (yy - H / 2) / H, (xx - W / 2) / W
    S = np.empty((C, H, W), np.complex128)
    for c in range(C):
        a = 2 * np.pi * c / C + 0.3
        cy, cx = 0.6 * np.sin(a), 0.6 * np.cos(a)
        mag = np.exp(-((u - cy) ** 2 + (v - cx) ** 2) / (2 * 0.45 ** 2))
        ky, kx = rng.uniform(-2.0, 2.0, 2)
        S[c] = mag * np.exp(1j * (2 * np.pi * (ky * u + kx * v) + rng.uniform(0, 2 * np.pi)))
    return S / np.sqrt((np.abs(S) ** 2).sum(0, keepdims=True))


def noise(seed, C, m, std=1.0):
    """complex Gaussian noise on the sampled entries, [C,H,W] complex128"""
    rng = np.random.default_rng(3100 + seed)
    n = std * (rng.standard_normal((C,) + m.shape) + 1j * rng.standard_normal((C,) + m.shape))
    return n * (m != 0)


def noise_full(seed, shape, std=1.0):
    """complex Gaussian noise on EVERY entry of an array of `shape` ([H,W], [C,H,W] or [B,C,H,W]), complex128: what the device synthesis
    adds unmasked (y = m . fft2(S_c . img) + noise, the reference's y = fft2(img) * mask + noises)"""
    rng = np.random.default_rng(4700 + seed)
    return std * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def disc(H, W, radius=0.42):
    """1 inside the disc of `radius` * H around the centre, 0 outside: maps times this are rank-deficient there (G = La2 I)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) <= (radius * H) ** 2).astype(np.float64)


# ---- operators ---------------------------------------------------------------------------------------------------------------------

def A(x, S, m, dt=np.complex128):
    S = S.astype(dt)
    return (np.fft.fft2((S * np.asarray(x).astype(dt)).astype(dt), axes=(-2, -1)).astype(dt) * (m != 0)).astype(dt)


def AH(k, S, m, dt=np.complex128):
    S = S.astype(dt)
    img = np.fft.ifft2((np.asarray(k).astype(dt) * (m != 0)).astype(dt), axes=(-2, -1)).astype(dt)
    out = np.zeros(S.shape[1:], dt)
    for c in range(S.shape[0]):                                  # coils in order, every partial sum rounded
        out = (out + (np.conj(S[c]) * img[c]).astype(dt)).astype(dt)
    return out


def G(p, S, m, reo, dt=np.complex128):
    la2 = _real(dt)(1.0 / 2.0 / reo)
    p = np.asarray(p).astype(dt)
    return (AH(A(p, S, m, dt), S, m, dt) + (la2 * p).astype(dt)).astype(dt)


def synthesize(img, S, m, nz):
    """y_c = m . fft2(S_c . img) + noise, complex128"""
    return A(img, S, m) + nz


def _dot(a, b, dt):
    """<a, b> = sum conj(a) b, real part; rounded to the precision's real type"""
    return _real(dt)(np.sum((np.conj(a) * b).real.astype(_real(dt))))


def _ratio(num, den):
    if den == 0:
        return type(num)(0)
    with np.errstate(all='ignore'):
        q = num / den
    return q if np.isfinite(q) else type(num)(0)


def cg_solve(aty, v, S, m, reo, iters, dt=np.complex128):
    """`iters` iterations of plain CG on G x^ = aty + La2 v, warm-started at x^ = v.  -> (x^, ||r|| / ||aty + La2 v||)"""
    R = _real(dt)
    la2 = R(1.0 / 2.0 / reo)
    xh = np.asarray(v).astype(dt)
    rhs = (aty.astype(dt) + (la2 * xh).astype(dt)).astype(dt)
    r = (rhs - G(xh, S, m, reo, dt)).astype(dt)
    p = r.copy()
    rr = _dot(r, r, dt)
    for _ in range(iters):
        Gp = G(p, S, m, reo, dt)
        alpha = R(_ratio(rr, _dot(p, Gp, dt)))
        xh = (xh + (alpha * p).astype(dt)).astype(dt)
        r = (r - (alpha * Gp).astype(dt)).astype(dt)
        rn = _dot(r, r, dt)
        beta = R(_ratio(rn, rr))
        p = (r + (beta * p).astype(dt)).astype(dt)
        rr = rn
    bb = _dot(rhs, rhs, dt)
    return xh, float(np.sqrt(float(rr) / float(bb))) if bb > 0 else 0.0


def x_step(z, w, aty, S, m, reo, iters=3, dt=np.complex128, residual=False):
    R = _real(dt)
    v = (np.asarray(z).astype(R) - np.asarray(w).astype(R)).astype(R)
    xh, rel = cg_solve(aty, v, S, m, reo, iters, dt)
    x = np.abs(xh.real).astype(R)
    return (x, rel) if residual else x


def init_state(y, S, m, dt=np.complex128):
    """-> (aty, z0 = |A^H y|, w0 = 0)"""
    aty = AH(np.asarray(y).astype(dt), S, m, dt)
    z = np.abs(aty).astype(_real(dt))
    return aty, z, np.zeros_like(z)


def admm(y, S, m, iter_num, kind, cg_iters=3, dt=np.complex128, prox=None, trace=(), **par):
    """ADMM_L1 (kind 'l1': lambda1, reo) / ADMM_CNC (kind 'cnc': alpha, lambda1, reo, b) with the multi-coil x-step.  prox: None (the
    pixel steps of oracle/admm_oracle.py) or a function (x, z, w) -> (z, w).  trace: iterations at which (x, z, z_prev, w) are kept."""
    R = _real(dt)
    pr = dict(O_PRESETS[kind], **par)
    aty, z, w = init_state(y, S, m, dt)
    x = z.copy()
    rec = {}
    for i in range(iter_num):
        zp = z
        x = x_step(z, w, aty, S, m, pr['reo'], cg_iters, dt)
        if prox is not None:
            z, w = prox(x, z, w)
        elif kind == 'l1':
            z, w = O.l1_step(x, z, w, R(pr['lambda1']), R(pr['reo']))
        else:
            z, w = O.cnc_step(x, z, w, R(pr['alpha']), R(pr['lambda1']), R(pr['reo']), R(pr['b']))
        z, w = z.astype(R), w.astype(R)
        if (i + 1) in trace:
            rec[i + 1] = (x.copy(), z.copy(), zp.copy(), w.copy())
    return (x, rec) if trace else x


O_PRESETS = {'l1': dict(lambda1=0.1, reo=0.015), 'cnc': dict(alpha=0.45, lambda1=0.5, reo=0.05, b=64)}          # S1:171, S4:176


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    dt = np.complex128 if (np.iscomplexobj(a) or np.iscomplexobj(b)) else np.float64
    return float(np.linalg.norm(a.astype(dt) - b.astype(dt)) / np.linalg.norm(b.astype(dt)))


def problem(seed, C, H, W, std=1.0):
    """-> (img float32 [H,W], S [C,H,W], mask uint8 [H,W], noise [C,H,W], y [C,H,W] complex128)"""
    img, S, m = phantom(seed, H, W), coil_maps(C, H, W, seed), mask(seed, H, W)
    nz = noise(seed, C, m, std)
    return img, S, m, nz, synthesize(img, S, m, nz)
