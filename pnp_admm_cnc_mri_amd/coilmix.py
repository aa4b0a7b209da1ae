"""Coil mixing ahead of the multi-coil solve: noise prewhitening and SVD coil compression (include/pnp_mri.h, "coil mixing").

NOT in the reference scripts.  Both steps are one C_out x C_in complex matrix M per coil set, applied per k-space point to the measurements
and per pixel to the maps; the forward model is linear in the coil index, so y' = M y, S' = M S is again y'_j = mask . fft2(S'_j . x) and
the solvers' coils= / y= take the mixed arrays unchanged.  This module owns no numerics: the Gram matrices and the mixing are the HIP
kernels behind pnp_coil_gram / pnp_coil_mix, the two small factorisations the library's host routines; what is done here in NumPy is
the product of C x C matrices and the sum of the per-slice Gram matrices, in slice order.

    whitening_matrix(noise_cov)                                  M_w = L^-1 (noise_cov = L L^H)
    calibration_gram(y, mask, mask_id, coil_id, Ks, ncal)        [Ks,C,C] Gram matrices of the calibration region, one per coil set
    compression_matrix(gram, n, whiten)                          (M, eigvals): M = M_c M_w, M_c from the Gram of the WHITENED data
    mix(k, M, coil_id)                                           out[b, j] = sum_c M[set(b), j, c] k[b, c]
    prepare(y, coils, mask, ...)                                 (y', coils', info): all of the above for a solver call

Device arrays are torch tensors; host arrays go through the device in chunks of slices of at most CHUNK_BYTES, so a 128-channel batch
never has to be resident whole -- and because the Gram matrices are formed per SLICE and summed on the host, the result does not depend
on the chunking, bit for bit.
"""
import ctypes as C

import numpy as np

from . import _lib

CHUNK_BYTES = 256 << 20


def _err():
    return ValueError(_lib.lib().pnp_last_error().decode('utf-8', 'replace'))


def _is_dev(a):
    return hasattr(a, 'data_ptr')


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _device(device, like=None):
    import torch
    if like is not None and _is_dev(like):
        return like.device
    from .solvers import resolve_device
    return torch.device('cuda', resolve_device(device))


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _chunks(B, slice_bytes, chunk_bytes):
    step = max(1, int(chunk_bytes) // max(1, int(slice_bytes)))
    return [(lo, min(B, lo + step)) for lo in range(0, B, step)]


def _cdt(a):
    """the complex type an array is processed in: complex128 stays, everything else is complex64"""
    if _is_dev(a):
        import torch
        if a.dtype not in (torch.complex64, torch.complex128):
            raise ValueError('device arrays must be complex64 or complex128 (got %s)' % a.dtype)
        return np.complex128 if a.dtype == torch.complex128 else np.complex64
    dt = a.dtype if hasattr(a, 'dtype') else np.asarray(a).dtype
    return np.complex128 if dt == np.complex128 else np.complex64


def _to_dev(a, dt, dev):
    """host slice -> contiguous device tensor of complex type dt; a device tensor is checked and passed on"""
    import torch
    if _is_dev(a):
        if not a.is_contiguous():
            raise ValueError('device arrays must be contiguous')
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def _ids(ids, B, n, name):
    if ids is None:
        return None
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    if ids.shape != (B,):
        raise ValueError('%s must have shape (B,) = (%d,)' % (name, B))
    if ids.size and (ids.min() < 0 or ids.max() >= n):
        raise ValueError('%s out of range [0, %d)' % (name, n))
    return ids


def check(C_in, C_out, Ks, ncal, H, W):
    """ValueError unless the sizes are valid for coil mixing (pnp_coilmix_check: the library's own rule, no device needed)."""
    if any(int(v) != v for v in (C_in, C_out, Ks, ncal)):
        raise ValueError('virtual_coils and calib must be integers')
    if _lib.lib().pnp_coilmix_check(int(C_in), int(C_out), int(Ks), int(ncal), int(H), int(W)) != 0:
        raise _err()


def whitening_matrix(noise_cov):
    """M_w [C,C] complex128 = L^-1 with noise_cov = L L^H (its lower triangle is read): the whitened channels M_w y have unit,
    uncorrelated noise.  ValueError when noise_cov is not a finite, positive-definite [C,C] matrix with C <= 128."""
    a = np.ascontiguousarray(noise_cov, dtype=np.complex128)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError('noise_cov must be a square [C,C] matrix (got shape %s)' % (a.shape,))
    out = np.empty_like(a)
    if _lib.lib().pnp_coilmix_whiten(C.c_void_p(a.ctypes.data), a.shape[0], C.c_void_p(out.ctypes.data)) != 0:
        raise _err()
    return out


def calibration_gram(y, mask, mask_id=None, coil_id=None, Ks=1, ncal=24, device=None, chunk_bytes=CHUNK_BYTES, per_slice=False):
    """Gram matrices of the calibration region (the ncal x ncal lowest frequencies, DC at [0, 0]): per slice
    R_b[i, j] = sum_p mask_b(p) y[b, i, p] conj(y[b, j, p]) on the device in double, then summed per coil set ON THE HOST IN SLICE ORDER.
    y [B,C,H,W] complex (host array or device tensor; complex128 stays double, everything else is taken as complex64), mask [H,W] or a
    bank [K,H,W] with mask_id [B], coil_id [B] into Ks sets.  -> [Ks,C,C] complex128 (per_slice=True: the [B,C,C] matrices themselves)."""
    import torch
    if np.ndim(y) != 4:
        raise ValueError('y must be [B,C,H,W] (got shape %s)' % (tuple(np.shape(y)),))
    B, Cn, H, W = (int(v) for v in np.shape(y))
    check(Cn, 1, Ks, ncal, H, W)
    mask = np.asarray(mask)
    bank = np.ascontiguousarray(mask[None] if mask.ndim == 2 else mask, dtype=np.uint8)
    if bank.shape[1:] != (H, W):
        raise ValueError('mask must be [H,W] or [K,H,W] with H x W = %d x %d' % (H, W))
    mid, cid = _ids(mask_id, B, len(bank), 'mask_id'), _ids(coil_id, B, Ks, 'coil_id')
    dt = _cdt(y)
    dev = _device(device, y)
    L = _lib.lib()
    fn = L.pnp_coil_gram_f64 if dt == np.complex128 else L.pnp_coil_gram
    grams = np.empty((B, Cn, Cn), np.complex128)
    with torch.cuda.device(dev):
        bank_t = torch.from_numpy(bank).to(dev)
        for lo, hi in ([(0, B)] if _is_dev(y) else _chunks(B, Cn * H * W * np.dtype(dt).itemsize, chunk_bytes)):
            y_t = _to_dev(y[lo:hi], dt, dev)
            mid_t = None if mid is None else torch.from_numpy(mid[lo:hi]).to(dev)
            g_t = torch.empty((hi - lo, Cn, Cn), dtype=torch.complex128, device=dev)
            _lib.check(fn(_stream(dev), _p(y_t), _p(bank_t), _p(mid_t), _p(g_t), hi - lo, Cn, H, W, int(ncal)))
            grams[lo:hi] = g_t.cpu().numpy()
    if per_slice:
        return grams
    out = np.zeros((int(Ks), Cn, Cn), np.complex128)
    for b in range(B):                                               # slice order: independent of the chunking and of the batch's cut
        out[0 if cid is None else cid[b]] += grams[b]
    return out


def compression_matrix(gram, n, whiten=None):
    """The n virtual coils that carry the most calibration energy.  gram [C,C] (or [Ks,C,C]: one result per set) Hermitian; whiten: None
    or M_w [C,C] (whitening_matrix) -- then the Gram of the whitened data, M_w gram M_w^H, is what is decomposed and the result is the
    COMBINED matrix M = M_c M_w, to be applied once to the raw data.  -> (M [n,C] complex128, eigvals [C] descending), with a leading Ks
    axis when gram had one.  The rows of M_c are the conjugated leading eigenvectors, each eigenvector's entry of largest modulus real and
    positive; eigvals[:n].sum() / eigvals.sum() is the share of the calibration energy that is kept."""
    g = np.asarray(gram, dtype=np.complex128)
    if g.ndim == 3:
        res = [compression_matrix(gk, n, whiten) for gk in g]
        return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise ValueError('gram must be [C,C] or [Ks,C,C] (got shape %s)' % (g.shape,))
    Cn = g.shape[0]
    Mw = None
    if whiten is not None:
        Mw = np.asarray(whiten, dtype=np.complex128)
        if Mw.shape != (Cn, Cn):
            raise ValueError('whiten must be [C,C] = [%d,%d]' % (Cn, Cn))
        g = Mw @ g @ Mw.conj().T
    g = np.ascontiguousarray(g)
    if int(n) != n:
        raise ValueError('the number of virtual coils must be an integer (got %r)' % (n,))
    M = np.empty((int(n) if 1 <= n <= Cn else 1, Cn), np.complex128)
    eig = np.empty(Cn, np.float64)
    if _lib.lib().pnp_coilmix_compress(C.c_void_p(g.ctypes.data), Cn, int(n), C.c_void_p(M.ctypes.data), C.c_void_p(eig.ctypes.data)) != 0:
        raise _err()
    return (M if Mw is None else M @ Mw), eig


def mix(k, M, coil_id=None, device=None, chunk_bytes=CHUNK_BYTES):
    """out[b, j, ...] = sum_c M[set(b), j, c] k[b, c, ...] on the device (pnp_coil_mix), coils accumulated in order.  k [B,C_in,...]
    complex: a contiguous device tensor (-> a new device tensor, on torch's current stream) or a host array (-> host array; chunks of
    slices of at most chunk_bytes go through the device).  M [C_out,C_in], or [Ks,C_out,C_in] with coil_id [B]; it is rounded to k's
    precision.  Measurements: k = y [B,C,H,W]; a bank of maps [Ks,C,H,W]: coil_id = arange(Ks)."""
    import torch
    if np.ndim(k) < 3:
        raise ValueError('k must be [B,C_in,...] (got shape %s)' % (tuple(np.shape(k)),))
    shape = tuple(int(v) for v in np.shape(k))
    B, Cin, N = shape[0], shape[1], int(np.prod(shape[2:]))
    M = np.asarray(M)
    Mb = M[None] if M.ndim == 2 else M
    if Mb.ndim != 3 or Mb.shape[2] != Cin:
        raise ValueError('M must be [C_out,C_in] or [Ks,C_out,C_in] with C_in = %d (got shape %s)' % (Cin, M.shape))
    Ks, Cout = int(Mb.shape[0]), int(Mb.shape[1])
    if not (1 <= Cin <= 128 and 1 <= Cout <= min(Cin, 32)) or N < 1 or B < 1:
        check(Cin, Cout, Ks, 4, 128, 128)
        raise ValueError('k must have at least one slice and one point per coil')
    cid = _ids(coil_id, B, Ks, 'coil_id')
    if cid is None and Ks != 1:
        raise ValueError('M has %d sets: coil_id is needed' % Ks)
    dt = _cdt(k)
    dev = _device(device, k)
    L = _lib.lib()
    fn = L.pnp_coil_mix_f64 if dt == np.complex128 else L.pnp_coil_mix
    tdt = torch.complex128 if dt == np.complex128 else torch.complex64
    with torch.cuda.device(dev):
        M_t = torch.from_numpy(np.ascontiguousarray(Mb, dtype=dt)).to(dev)
        on_dev = _is_dev(k)
        out = torch.empty((B, Cout) + shape[2:], dtype=tdt, device=dev) if on_dev else np.empty((B, Cout) + shape[2:], dt)
        for lo, hi in ([(0, B)] if on_dev else _chunks(B, Cin * N * np.dtype(dt).itemsize, chunk_bytes)):
            k_t = _to_dev(k[lo:hi], dt, dev)
            cid_t = None if cid is None else torch.from_numpy(cid[lo:hi]).to(dev)
            o_t = out[lo:hi] if on_dev else torch.empty((hi - lo, Cout) + shape[2:], dtype=tdt, device=dev)
            _lib.check(fn(_stream(dev), _p(k_t), _p(M_t), _p(cid_t), _p(o_t), hi - lo, Cin, Cout, N))
            if not on_dev:
                out[lo:hi] = o_t.cpu().numpy()
        if on_dev:
            torch.cuda.current_stream(dev).synchronize()             # M_t and cid_t are released on return
    return out


def plan(coils, H, W, virtual_coils=None, noise_cov=None, calib=24):
    """The sizes of a solver call with virtual_coils= / noise_cov=, checked without a device.  -> (C_in, C_out, Ks)"""
    shape = np.shape(coils)
    if len(shape) not in (3, 4) or tuple(shape[-2:]) != (int(H), int(W)):
        raise ValueError('coils must be [C,H,W] or [Ks,C,H,W] with H x W = %d x %d (got shape %s)' % (H, W, tuple(shape)))
    Cin, Ks = int(shape[-3]), (int(shape[0]) if len(shape) == 4 else 1)
    Cout = Cin if virtual_coils is None else virtual_coils
    check(Cin, Cout, Ks, calib, H, W)
    if noise_cov is not None and np.shape(noise_cov) != (Cin, Cin):
        raise ValueError('noise_cov must be [C,C] = [%d,%d] (got shape %s)' % (Cin, Cin, tuple(np.shape(noise_cov))))
    return Cin, int(Cout), Ks


def plan_y(Cin, H, W, virtual_coils=None, noise_cov=None, calib=24):
    """plan() for measurements without maps (coils='estimate': the maps are estimated from the mixed y).  -> (C_in, C_out)"""
    Cout = Cin if virtual_coils is None else virtual_coils
    check(Cin, Cout, 1, calib, H, W)
    if noise_cov is not None and np.shape(noise_cov) != (Cin, Cin):
        raise ValueError('noise_cov must be [C,C] = [%d,%d] (got shape %s)' % (Cin, Cin, tuple(np.shape(noise_cov))))
    return int(Cin), int(Cout)


def prepare(y, coils, mask, mask_id=None, coil_id=None, virtual_coils=None, noise_cov=None, calib=24, precision='f32', device=None,
            chunk_bytes=CHUNK_BYTES):
    """What the solvers do with virtual_coils= / noise_cov=: one matrix per coil set of the bank -- M_w from noise_cov, M_c from the Gram
    matrix of the calibration region (calib x calib) of the slices that use that set, M = M_c M_w -- applied once to y and to the maps.
    y [B,C,H,W] (host array or device tensor), coils [C,H,W] or [Ks,C,H,W], C <= 128; virtual_coils None: C_out = C (noise_cov alone).
    coils None: only y is mixed, by ONE matrix from the Gram matrices of the whole batch (coil_id is ignored; coils' comes back None).
    -> (y' [B,C_out,H,W], coils' of coils' rank, info = {'M', 'eigvals', 'energy', 'C_in', 'C_out', 'whitened'}) in the precision's
    complex type; M [C_out,C] ([Ks,C_out,C] for a bank) complex128 is the matrix in double, as it came from the host routines."""
    if precision not in ('f32', 'f64'):
        raise ValueError("precision must be 'f32' or 'f64'")
    if virtual_coils is None and noise_cov is None:
        raise ValueError('nothing to do: give virtual_coils=, noise_cov= or both')
    H, W = (int(v) for v in np.shape(y)[-2:])
    if coils is None:                                                # the measurements alone (the maps are estimated from y' afterwards): one set
        if np.ndim(y) != 4:
            raise ValueError('y must be [B,C,H,W] (got shape %s)' % (tuple(np.shape(y)),))
        Cin, Cout, Ks, coil_id = plan_y(np.shape(y)[1], H, W, virtual_coils, noise_cov, calib) + (1, None)
    else:
        Cin, Cout, Ks = plan(coils, H, W, virtual_coils, noise_cov, calib)
    if np.ndim(y) != 4 or np.shape(y)[1] != Cin:
        raise ValueError('y must be [B,%d,H,W] (got shape %s)' % (Cin, tuple(np.shape(y))))
    dt = np.complex128 if precision == 'f64' else np.complex64
    if _is_dev(y):
        if _cdt(y) != dt:
            raise ValueError("a device y must have the precision's complex type")
    elif np.asarray(y).dtype != dt:
        y = _Cast(np.asarray(y), dt)                                 # cast chunk by chunk, never the whole batch
    bank = None
    if coils is not None:
        bank = np.asarray(coils) if not _is_dev(coils) else coils
        if len(np.shape(coils)) == 3:
            bank = bank[None]
    Mw = None if noise_cov is None else whitening_matrix(noise_cov)
    if virtual_coils is not None:
        gram = calibration_gram(y, mask, mask_id, coil_id, Ks, calib, device, chunk_bytes)
        M, eig = compression_matrix(gram, Cout, Mw)
        energy = [float(e[:Cout].sum() / e.sum()) if e.sum() > 0 else 1.0 for e in eig]
    else:
        M, eig, energy = np.stack([Mw] * Ks), None, [1.0] * Ks
    y2 = mix(y, M, coil_id if Ks > 1 or coil_id is not None else None, device, chunk_bytes)
    S2 = None
    if bank is not None:
        if not _is_dev(bank) and bank.dtype != dt:
            bank = bank.astype(dt)
        S2 = mix(bank, M, np.arange(Ks, dtype=np.int32), device, chunk_bytes)
    single = coils is None or len(np.shape(coils)) == 3
    info = dict(M=M[0] if single else M, eigvals=None if eig is None else (eig[0] if single else eig),
                energy=energy[0] if single else energy, C_in=Cin, C_out=Cout, whitened=noise_cov is not None)
    return y2, (None if S2 is None else S2[0] if single else S2), info


class _Cast:
    """a host array whose slices come out in another complex type: y[lo:hi] is cast, the whole never is"""

    def __init__(self, a, dt):
        self.a, self.dtype, self.shape, self.ndim = a, np.dtype(dt), a.shape, a.ndim

    def __getitem__(self, s):
        return np.ascontiguousarray(self.a[s], dtype=self.dtype)

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.a, dtype=dtype or self.dtype)


def describe(info):
    """the solvers' log line"""
    e = np.atleast_1d(np.asarray(info['energy'], np.float64))
    return 'coil mixing: {:d} -> {:d} virtual coils, {:.1f} % of the calibration energy{:s} (not in the reference scripts)'.format(
        info['C_in'], info['C_out'], 100.0 * float(e.min()), ', prewhitened' if info['whitened'] else '')
