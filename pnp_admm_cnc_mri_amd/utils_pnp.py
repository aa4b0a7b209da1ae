"""`utils_pnp` of the reference (utils/utils_pnp.py) -- same names, same arguments -- plus the
operator API the north star asks for next to it (A, AH, Df, dc_solve, prox_l1, prox_cnc), all
batched and running on the HIP engine.

The two schedule functions are host scalar code (iter_num floats); they follow
utils/utils_pnp.py:14-34 and are pinned bit-for-bit by tests/test_oracle_golden.py.
"""
import numpy as np


def get_rho_sigma(sigma=2.55 / 255, iter_num=15, modelSigma1=49.0, modelSigma2=2.55, w=1.0):
    """utils/utils_pnp.py:14-23: log/linear blend of the denoiser noise levels, and rho_k."""
    modelSigmaS = np.logspace(np.log10(modelSigma1), np.log10(modelSigma2), iter_num).astype(np.float32)
    modelSigmaS_lin = np.linspace(modelSigma1, modelSigma2, iter_num).astype(np.float32)
    sigmas = (modelSigmaS * w + modelSigmaS_lin * (1 - w)) / 255.
    rhos = list(map(lambda x: 0.23 * (sigma ** 2) / (x ** 2), sigmas))
    return rhos, sigmas


def get_rho_sigma1(sigma=2.55 / 255, iter_num=15, modelSigma1=49.0, modelSigma2=2.55, lamda=3.0):
    """utils/utils_pnp.py:26-34."""
    modelSigmaS = np.logspace(np.log10(modelSigma1), np.log10(modelSigma2), iter_num).astype(np.float32)
    sigmas = modelSigmaS / 255.
    rhos = list(map(lambda x: (sigma ** 2) / (x ** 2) / lamda, sigmas))
    return rhos, sigmas


# ----------------------------------------------------------------------------------------------
# operator API: torch CUDA tensors in, torch CUDA tensors out; an `Engine` holds y and the masks
# ----------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _prep(eng, t):
    torch = _torch()
    if not t.is_cuda:
        raise ValueError('operator API works on CUDA tensors (no CPU fallback)')
    eng.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
    return t.contiguous()


def fft2(eng, x):
    """np.fft.fft2 of a complex64 batch [B,H,W] (S4:102, 120)."""
    torch = _torch()
    x = _prep(eng, x.to(torch.complex64))
    out = torch.empty_like(x)
    eng.fft2(torch.view_as_real(x), torch.view_as_real(out), x.shape[0])
    return out


def ifft2(eng, k):
    """np.fft.ifft2 (S4:103, 123)."""
    torch = _torch()
    k = _prep(eng, k.to(torch.complex64))
    out = torch.empty_like(k)
    eng.ifft2(torch.view_as_real(k), torch.view_as_real(out), k.shape[0])
    return out


def dwt2(eng, x, shift=(0, 0)):
    """Psi x: the periodic 2-D DWT of the engine's sparsity setting (Engine.set_sparsity) of a real batch [B,H,W], Mallat layout.
    shift=(sy, sx), each in [0, 2**levels): Psi_s x = Psi roll(x, (-sy, -sx)), the transform of the shifted frame (cycle spinning).
    No counterpart in the reference."""
    torch = _torch()
    x = _prep(eng, x.to(torch.float64 if eng.f64 else torch.float32))
    out = torch.empty_like(x)
    eng.dwt2(x, out, x.shape[0], None if tuple(shift) == (0, 0) else shift)
    return out


def idwt2(eng, c, shift=(0, 0)):
    """Psi^T c, the inverse of dwt2; with shift=(sy, sx) Psi_s^T c = roll(Psi^T c, (sy, sx))."""
    torch = _torch()
    c = _prep(eng, c.to(torch.float64 if eng.f64 else torch.float32))
    out = torch.empty_like(c)
    eng.idwt2(c, out, c.shape[0], None if tuple(shift) == (0, 0) else shift)
    return out


def _coils_of(eng, coils):
    """coils=None: whatever the engine has; True / False: the caller's expectation, checked (an engine with coils returns and takes
    [B,C,H,W] k-space: a silent mismatch would only show as a shape error far away).  -> the engine's coil count, 0 without"""
    n = int(getattr(eng, 'C', 0))
    if coils is not None and bool(coils) != (n > 0):
        raise ValueError('coils=%r but the engine has %s' % (coils, '%d coils' % n if n else 'no coils (Engine.set_coils)'))
    return n


def A(eng, x, coils=None):
    """A x = fft2(x) * mask for real x [B,H,W] with the engine's uploaded masks (S4:102).  On an engine with coils (Engine.set_coils;
    coils=True insists on it): (A x)_c = fft2(S_c x) * mask, [B,C,H,W].  On an engine in complex image mode (Engine.set_image_mode) x is
    a complex batch [B,H,W]."""
    torch = _torch()
    cx = getattr(eng, 'image_mode', 'real') == 'complex'
    if x.is_complex() and not cx:
        raise ValueError("A takes a complex image only on an engine in complex image mode (Engine.set_image_mode('complex'))")
    x = _prep(eng, x.to(torch.complex64) if cx else x.float())
    n = _coils_of(eng, coils)
    k = torch.empty((x.shape[0], n) + tuple(x.shape[1:]) if n else x.shape, dtype=torch.complex64, device=x.device)
    eng.A(torch.view_as_real(x) if cx else x, torch.view_as_real(k))
    return k


def AH(eng, k, coils=None):
    """A^H k = ifft2(k * mask) (utils/utils.py:54).  On an engine with coils: k [B,C,H,W] -> sum_c conj(S_c) ifft2(k_c * mask), [B,H,W]."""
    torch = _torch()
    k = _prep(eng, k.to(torch.complex64))
    n = _coils_of(eng, coils)
    if n and (k.dim() != 4 or k.shape[1] != n):
        raise ValueError('k must be [B,%d,H,W] on this engine (got %s)' % (n, tuple(k.shape)))
    out = torch.empty((k.shape[0],) + tuple(k.shape[2:]), dtype=k.dtype, device=k.device) if n else torch.empty_like(k)
    eng.AH(torch.view_as_real(k), torch.view_as_real(out))
    return out


def estimate_coil_maps(y, mask, mask_id=None, calib=24, radius=2, power_iters=4, thresh=0.05, **kw):
    """Sensitivity maps [B,C,H,W] from the calibration region of measured k-space y [B,C,H,W], one set per slice, on device tensors or host
    arrays (coilmaps.estimate; engine=: an Engine to run on).  No counterpart in the reference."""
    from . import coilmaps
    return coilmaps.estimate(y, mask, mask_id, calib, radius, power_iters, thresh, **kw)


def coil_mix(k, M, coil_id=None):
    """out[b, j] = sum_c M[set(b), j, c] k[b, c]: prewhitening / coil compression of k-space [B,C,H,W] or of a bank of maps, on device
    tensors or host arrays (coilmix.mix; no engine: pnp_coil_mix is stateless).  No counterpart in the reference."""
    from . import coilmix
    return coilmix.mix(k, M, coil_id)


def whitening_matrix(noise_cov):
    """M_w = L^-1 of the Cholesky factor of the channels' noise covariance (coilmix.whitening_matrix)."""
    from . import coilmix
    return coilmix.whitening_matrix(noise_cov)


def compression_matrix(gram, n, whiten=None):
    """(M, eigvals): the n leading virtual coils of a calibration Gram matrix, combined with M_w (coilmix.compression_matrix)."""
    from . import coilmix
    return coilmix.compression_matrix(gram, n, whiten)


def Df(eng, x):
    """Df(x, mask, y) = A^H (A x - y) of utils/utils.py:50-55, with the engine's y and masks."""
    torch = _torch()
    x = _prep(eng, x.float())
    out = torch.empty(x.shape, dtype=torch.complex64, device=x.device)
    eng.Df(x, torch.view_as_real(out))
    return out


def dc_solve(eng, z, w, reo):
    """x-update x = |Re ifft2((La2*F(z-w) + M^T y)/(La2 + M))|, La2 = 1/(2 reo) (S4:119-124)."""
    torch = _torch()
    z = _prep(eng, z.float())
    w = _prep(eng, w.float())
    x = torch.empty_like(z)
    eng.dc_step(z, w, x, reo)
    return x


def prox_l1(eng, x, z, w, thr):
    """in place: z = soft(x + w, thr); w = w + x - z (S1:123, 126).  Returns (z, w)."""
    _prep(eng, x)
    eng.prox_l1_dual(x, z, w, thr)
    return z, w


def prox_cnc(eng, x, z, w, alpha, lambda1, reo, b):
    """in place CNC z-update + dual update (S4:127-132).  Returns (z, w)."""
    _prep(eng, x)
    eng.prox_cnc_dual(x, z, w, alpha, lambda1, reo, b)
    return z, w
