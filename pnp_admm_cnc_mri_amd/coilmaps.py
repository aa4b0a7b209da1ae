"""Coil sensitivity maps from the calibration region of k-space (include/pnp_mri.h, "coil sensitivity maps from the calibration region").

NOT in the reference scripts.  The multi-coil solvers need maps [C,H,W]; a scanner delivers k-space.  estimate() is the local
dominant-eigenvector method (Walsh's adaptive combination) in matrix-free form on low-resolution coil images: the calib x calib lowest
frequencies under a cos^2 window, the library's own inverse transform, `power_iters` power steps on the (2 radius + 1)^2 patch around
every pixel, a phase rule that leaves v^H I >= 0 (the solvers reconstruct a real non-negative image, so the maps carry all of the
phase), and a support: maps are exactly 0 where the local eigenvalue is below thresh^2 of the slice's largest, and have
sum_c |S_c|^2 = 1 everywhere else.  estimate(method='espirit') is the ESPIRiT estimator instead (include/pnp_mri.h, "ESPIRiT coil
sensitivity maps"): the Gram matrix of the kernel x kernel patches of the calibration block, its signal space above sigma of the largest
singular value, the per-pixel operator G(q) of the kernel autocorrelations, `power_iters` power steps on it from the same low-resolution
images, the same phase rule, and the support where the eigenvalue is at least crop and the low-resolution image at least thresh of its
largest.  This module owns no numerics: all of it is pnp_coil_maps / pnp_espirit_maps.

    check(C, calib, radius, power_iters, thresh, H, W)      ValueError unless the sizes are valid (no device needed); method=, kernel=,
                                                            sigma=, crop= for the ESPIRiT rules
    check_region(mask, mask_id, calib)                      ValueError unless every calibration point is sampled (host masks)
    estimate(y, mask, ...)                                  [B,C,H,W] maps, one set per slice
    describe(info)                                          the solvers' log line

Device arrays are torch tensors; host arrays go through the device in chunks of slices of at most CHUNK_BYTES.  Every slice is
estimated on its own, so the result does not depend on the chunking, bit for bit.
"""
import numpy as np

from . import _lib
from .coilmix import CHUNK_BYTES, _cdt, _chunks, _device, _err, _ids, _is_dev, _to_dev


METHODS = ('walsh', 'espirit')


def check(Cn, calib, radius, power_iters, thresh, H, W, method='walsh', kernel=4, sigma=0.02, crop=0.9):
    """ValueError unless the sizes are valid for the map estimation (pnp_coilmaps_check or, for method='espirit', pnp_espirit_check: the
    library's own rules, no device needed).  radius is not used by 'espirit', kernel / sigma / crop not by 'walsh'."""
    if method not in METHODS:
        raise ValueError("maps method must be 'walsh' or 'espirit' (got %r)" % (method,))
    if method == 'espirit':
        if any(int(v) != v for v in (Cn, calib, kernel, power_iters)):
            raise ValueError('calib, maps_kernel and maps_power_iters must be integers')
        if _lib.lib().pnp_espirit_check(int(Cn), int(calib), int(kernel), int(power_iters), float(sigma), float(crop), float(thresh), int(H),
                                        int(W)) != 0:
            raise _err()
        return
    if any(int(v) != v for v in (Cn, calib, radius, power_iters)):
        raise ValueError('calib, maps_radius and maps_power_iters must be integers')
    if _lib.lib().pnp_coilmaps_check(int(Cn), int(calib), int(radius), int(power_iters), float(thresh), int(H), int(W)) != 0:
        raise _err()


def _cal_lines(ncal, n):
    return np.array(list(range((ncal + 1) // 2)) + list(range(n - ncal // 2, n)), np.int64)


def check_region(mask, mask_id=None, calib=24):
    """ValueError unless every point of the calib x calib calibration region is sampled by every mask in use (mask [H,W] or a bank
    [K,H,W] with mask_id): the estimator does not zero-fill.  The message names the first missing point."""
    bank = np.asarray(mask)
    bank = bank[None] if bank.ndim == 2 else bank
    H, W = bank.shape[1:]
    rows, cols = _cal_lines(int(calib), H), _cal_lines(int(calib), W)
    for k in (range(len(bank)) if mask_id is None else sorted(set(int(v) for v in np.asarray(mask_id).ravel()))):
        if not 0 <= k < len(bank):
            raise ValueError('mask_id out of range [0, %d)' % len(bank))
        holes = np.argwhere(bank[k][np.ix_(rows, cols)] == 0)                 # the lines are in ascending order: the first is the lowest offset
        if len(holes):
            h, x = int(rows[holes[0][0]]), int(cols[holes[0][1]])
            raise ValueError('coil maps: mask %d does not sample calibration point (%d, %d) of the %d x %d region: every point of it must be '
                             'measured' % (k, h, x, calib, calib))


def estimate(y, mask, mask_id=None, calib=24, radius=2, power_iters=4, thresh=0.05, precision='f32', device=None, return_lambda=False,
             engine=None, chunk_bytes=CHUNK_BYTES, method='walsh', kernel=4, sigma=0.02, crop=0.9, return_rank=False):
    """Sensitivity maps of every slice from its own calibration region (pnp_coil_maps).  y [B,C,H,W] complex measurements (un-shifted, DC at
    [0, 0]): a contiguous device tensor of the precision's complex type (-> device tensors) or a host array (-> host arrays; chunks of
    slices of at most chunk_bytes go through the device).  mask [H,W] or a bank [K,H,W] with mask_id [B].  -> maps [B,C,H,W]: one coil set
    per slice, what the solvers take as coils= with coil_id=arange(B); return_lambda=True: (maps, lambda [B,H,W]), the local eigenvalue
    the support is cut from.  engine: an Engine of the same (H, W) and precision to run on (its uploaded problem and state are not
    touched); None: one is opened for the call.
    method='espirit': the ESPIRiT estimator (pnp_espirit_maps) with kernel x kernel calibration patches, the signal space above sigma of
    the largest singular value, and the support lambda >= crop and ||I|| >= thresh of the slice's largest; `radius` is IGNORED for it, and
    return_lambda returns the eigenvalue of G(q), which is about 1 where the maps are valid.  return_rank=True appends the signal-space
    rank of every slice, [B] int32 (None for 'walsh')."""
    import torch
    from .engine import Engine
    if precision not in ('f32', 'f64'):
        raise ValueError("precision must be 'f32' or 'f64'")
    if np.ndim(y) != 4:
        raise ValueError('y must be [B,C,H,W] (got shape %s)' % (tuple(np.shape(y)),))
    B, Cn, H, W = (int(v) for v in np.shape(y))
    check(Cn, calib, radius, power_iters, thresh, H, W, method, kernel, sigma, crop)
    if B < 1:
        raise ValueError('y must have at least one slice')
    mask = np.asarray(mask)
    bank = np.ascontiguousarray((mask[None] if mask.ndim == 2 else mask) != 0, dtype=np.uint8)
    if bank.shape[1:] != (H, W):
        raise ValueError('mask must be [H,W] or [K,H,W] with H x W = %d x %d' % (H, W))
    mid = _ids(mask_id, B, len(bank), 'mask_id')
    check_region(bank, mid, calib)
    dt = np.complex128 if precision == 'f64' else np.complex64
    on_dev = _is_dev(y)
    if on_dev and _cdt(y) != dt:
        raise ValueError("a device y must have the precision's complex type")
    if engine is not None and (engine.H, engine.W, engine.f64) != (H, W, precision == 'f64'):
        raise ValueError('the engine is %d x %d %s, the call %d x %d %s' % (engine.H, engine.W, 'f64' if engine.f64 else 'f32', H, W, precision))
    dev = torch.device('cuda', engine.device) if engine is not None else _device(device, y)
    tdt, rdt = (torch.complex128, torch.float64) if precision == 'f64' else (torch.complex64, torch.float32)
    pieces = [(0, B)] if on_dev else _chunks(B, Cn * H * W * np.dtype(dt).itemsize, chunk_bytes)
    own = engine is None
    with torch.cuda.device(dev):
        eng = engine if engine is not None else Engine(H, W, Bmax=min(max(hi - lo for lo, hi in pieces) * Cn, 64), device=dev.index,
                                                       precision=precision)
        try:
            bank_t = torch.from_numpy(bank).to(dev)
            maps = torch.empty((B, Cn, H, W), dtype=tdt, device=dev) if on_dev else np.empty((B, Cn, H, W), dt)
            rank = np.zeros(B, np.int32) if method == 'espirit' else None
            lam = None if not return_lambda else (torch.empty((B, H, W), dtype=rdt, device=dev) if on_dev else np.empty((B, H, W), dt(0).real.dtype))
            for lo, hi in pieces:
                y_t = _to_dev(y[lo:hi], dt, dev)
                mid_t = None if mid is None else torch.from_numpy(mid[lo:hi]).to(dev)
                m_t = maps[lo:hi] if on_dev else torch.empty((hi - lo, Cn, H, W), dtype=tdt, device=dev)
                l_t = None if lam is None else (lam[lo:hi] if on_dev else torch.empty((hi - lo, H, W), dtype=rdt, device=dev))
                torch.cuda.current_stream(dev).synchronize()         # the inputs are torch's; the call runs on the engine's stream
                if method == 'espirit':
                    rank[lo:hi] = eng.espirit_maps(y_t, bank_t, mid_t, m_t, l_t, hi - lo, Cn, calib, kernel, power_iters, sigma, crop, thresh)
                else:
                    eng.coil_maps(y_t, bank_t, mid_t, m_t, l_t, hi - lo, Cn, calib, radius, power_iters, thresh)  # synchronises at its end
                if not on_dev:
                    maps[lo:hi] = m_t.cpu().numpy()
                    if lam is not None:
                        lam[lo:hi] = l_t.cpu().numpy()
        finally:
            if own:
                eng.close()
    out = (maps, lam) if return_lambda else (maps,)
    if return_rank:
        out = out + (rank,)
    return out if len(out) > 1 else out[0]


def support_share(maps):
    """the share of pixels inside the support, per slice [B]: where any coil is not 0"""
    if _is_dev(maps):
        import torch
        return [float(v) for v in (maps != 0).any(dim=1).to(dtype=torch.float64).mean(dim=(1, 2)).cpu()]
    return [float(v) for v in (np.asarray(maps) != 0).any(axis=1).mean(axis=(1, 2))]


def describe(info):
    """the solvers' log line"""
    s = np.atleast_1d(np.asarray(info['support'], np.float64))
    if info.get('method', 'walsh') == 'espirit':
        r = np.atleast_1d(np.asarray(info['rank']))
        return ('coil maps estimated by ESPIRiT from the {:d} x {:d} calibration region: kernel {:d}, sigma {:g} (rank {:d} .. {:d}), {:d} '
                'power iterations, crop {:g}, threshold {:g}, support {:.1f} % of the pixels (not in the reference scripts)').format(
                    int(info['calib']), int(info['calib']), int(info['kernel']), float(info['sigma']), int(r.min()), int(r.max()),
                    int(info['power_iters']), float(info['crop']), float(info['thresh']), 100.0 * float(s.mean()))
    return ('coil maps estimated from the {:d} x {:d} calibration region: radius {:d}, {:d} power iterations, threshold {:g}, support '
            '{:.1f} % of the pixels (not in the reference scripts)').format(int(info['calib']), int(info['calib']), int(info['radius']),
                                                                           int(info['power_iters']), float(info['thresh']), 100.0 * float(s.mean()))
