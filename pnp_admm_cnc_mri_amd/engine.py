"""Host-side handle on one `pnp_ctx` of libpnpmri.so (include/pnp_mri.h).

`Engine` owns no numerics: every method is a thin call through the C ABI.  NumPy arrays are
passed as host pointers; objects exposing `data_ptr()` (torch CUDA tensors) as device pointers.
"""
import ctypes as C

import numpy as np

from . import _lib


def _is_dev(a):
    return hasattr(a, 'data_ptr')


def _ptr(a):
    if a is None:
        return None
    if _is_dev(a):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _is_cx(a):
    """a complex tensor or array?"""
    return bool(getattr(getattr(a, 'dtype', None), 'is_complex', False)) or (isinstance(a, np.ndarray) and np.iscomplexobj(a))


def _cx_denoise(mode):
    """the PNP_CX_DENOISE_* code of 'modulus' / 'parts'; an integer goes through as it is (the library names a bad one)"""
    if isinstance(mode, str):
        if mode not in CX_DENOISE:
            raise ValueError("cx_denoise must be 'modulus' or 'parts' (got %r)" % (mode,))
        return CX_DENOISE[mode]
    return int(mode)


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


WAVELETS = {None: 0, 'haar': 1, 'db2': 2, 'db4': 3}                                    # PNP_WAVELET_* of include/pnp_mri.h
IMAGE_MODES = {'real': 0, 'complex': 1}                                                # PNP_IMAGE_* of include/pnp_mri.h
CX_DENOISE = {'modulus': 0, 'parts': 1}                                                # PNP_CX_DENOISE_* of include/pnp_mri.h


def check_sparsity(wavelet, levels, H, W):
    """ValueError unless (wavelet, levels) is a valid sparsity setting for H x W slices (pnp_sparsity_check: the library's own rule,
    no context and no device needed).  -> the PNP_WAVELET_* code."""
    if wavelet not in WAVELETS:
        raise ValueError("transform must be one of None, 'haar', 'db2', 'db4' (got %r)" % (wavelet,))
    if wavelet is not None:
        if int(levels) != levels:
            raise ValueError('levels must be an integer (got %r)' % (levels,))
        L = _lib.lib()
        if L.pnp_sparsity_check(WAVELETS[wavelet], int(levels), int(H), int(W)) != 0:
            raise ValueError(L.pnp_last_error().decode('utf-8', 'replace'))
    return WAVELETS[wavelet]


def check_image(mode, wavelet=None, levels=3, precision='f32'):
    """ValueError unless the image mode runs with this sparsity setting and precision (pnp_image_check: the library's own rule, no
    context and no device needed -- db4 with 4 levels does not fit the LDS on complex doubles).  -> the PNP_IMAGE_* code."""
    if mode not in IMAGE_MODES:
        raise ValueError("image must be 'real' or 'complex' (got %r)" % (mode,))
    L = _lib.lib()
    if L.pnp_image_check(IMAGE_MODES[mode], WAVELETS.get(wavelet, 0), int(levels) if wavelet is not None else 0, 1 if precision == 'f64' else 0) != 0:
        raise ValueError(L.pnp_last_error().decode('utf-8', 'replace'))
    return IMAGE_MODES[mode]


def check_spin(shifts, levels, per_prox=1):
    """ValueError unless `shifts` ([n, 2] integers (sy, sx)) and `per_prox` are a valid cycle-spinning schedule for a transform of
    `levels` levels (pnp_spin_check: the library's own rule, no context and no device needed).  -> the table, [n, 2] int32."""
    a = np.asarray(shifts)
    if a.ndim != 2 or a.shape[1] != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('spin shifts must be an integer array [n, 2] of (sy, sx) (got shape %s, dtype %s)' % (a.shape, a.dtype))
    if int(per_prox) != per_prox:
        raise ValueError('per_prox must be an integer (got %r)' % (per_prox,))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError('spin: shift out of range')
    t = np.ascontiguousarray(a, dtype=np.int32)
    L = _lib.lib()
    if L.pnp_spin_check(int(levels), t.ctypes.data_as(C.POINTER(C.c_int32)), int(t.shape[0]), int(per_prox)) != 0:
        raise ValueError(L.pnp_last_error().decode('utf-8', 'replace'))
    return t


def check_temporal(frames, B=None):
    """ValueError unless `frames` is a valid series length (2..64) and -- when B is given -- a batch of B slices is a whole number of
    series (pnp_temporal_check: the library's own rule, no context and no device needed).  -> frames as an int."""
    if isinstance(frames, bool) or int(frames) != frames:
        raise ValueError('frames must be an integer (got %r)' % (frames,))
    L = _lib.lib()
    if L.pnp_temporal_check(int(frames), int(frames) if B is None else int(B)) != 0:
        raise ValueError(L.pnp_last_error().decode('utf-8', 'replace'))
    return int(frames)


LOWRANK_TABLE = 64                                                                      # entries of the 'random' shift table


def check_lowrank(frames, block, H, W, B=None, precision='f32', cnc=False):
    """ValueError unless `block` is a valid patch side for series of `frames` slices of H x W in this precision and for this step (L1, or
    CNC with cnc=True) and -- when B is given -- the batch is a whole number of series (pnp_lowrank_check: the library's own rule, no
    context and no device needed).  -> block as an int."""
    frames = check_temporal(frames)
    if isinstance(block, bool) or int(block) != block:
        raise ValueError('lowrank must be an integer (got %r)' % (block,))
    L = _lib.lib()
    if L.pnp_lowrank_check(frames, int(block), int(H), int(W), frames if B is None else int(B), 1 if precision == 'f64' else 0, 1 if cnc else 0) != 0:
        raise ValueError(L.pnp_last_error().decode('utf-8', 'replace'))
    return int(block)


def lowrank_table(shift, block, seed=0):
    """The shift table of the low-rank prox (Engine.set_lowrank), one entry per prox step, wrapping: 'random' -> 64 entries of
    np.random.default_rng(seed).integers(0, block, size=(64, 2)), made here on the host; None -> the single entry (0, 0); an array-like
    [n, 2] of (sy, sx) in [0, block) is passed through after checking.  Always int32."""
    if shift is None:
        return np.zeros((1, 2), np.int32)
    if isinstance(shift, str):
        if shift != 'random':
            raise ValueError("lowrank_shift must be 'random', None or an array [n, 2] of shifts (got %r)" % (shift,))
        return np.random.default_rng(seed).integers(0, int(block), size=(LOWRANK_TABLE, 2)).astype(np.int32)
    a = np.asarray(shift)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('lowrank_shift must be an integer array [n, 2] of (sy, sx), n >= 1 (got shape %s, dtype %s)' % (a.shape, a.dtype))
    for i, (sy, sx) in enumerate(a.tolist()):
        if not (0 <= sy < int(block) and 0 <= sx < int(block)):
            raise ValueError('lowrank_shift: entry %d = (%d, %d) out of range [0, %d)' % (i, sy, sx, int(block)))
    return np.ascontiguousarray(a, dtype=np.int32)


def spin_table(spin, levels, iters, average=1, seed=0):
    """The cycle-spinning table of a run of `iters` iterations that averages `average` shifts per prox (Engine.set_spin(table, average)):
    'random' -> np.random.default_rng(seed).integers(0, 2**levels, size=(iters * average, 2)); an array-like [n, 2] is passed through
    after checking (n a multiple of `average`, every shift in [0, 2**levels)); None -> None.  Always int32."""
    if spin is None:
        return None
    if int(average) != average or not 1 <= int(average) <= 16:
        raise ValueError('spin_average (per_prox) must be an integer in 1..16 (got %r)' % (average,))
    if isinstance(spin, str):
        if spin != 'random':
            raise ValueError("spin must be None, 'random' or an array [n, 2] of shifts (got %r)" % (spin,))
        if int(levels) != levels or not 1 <= int(levels) <= 4:
            raise ValueError('levels must be 1..4 (got %r)' % (levels,))
        if int(iters) * int(average) < 1:
            return None                                   # nothing to schedule
        spin = np.random.default_rng(seed).integers(0, 2 ** int(levels), size=(int(iters) * int(average), 2)).astype(np.int32)
    return check_spin(spin, levels, average)


def check_coils(sens, H, W, cg_iters=3):
    """ValueError unless `sens` is a valid set ([C,H,W]) or bank ([Ks,C,H,W]) of coil maps for H x W slices and cg_iters is 1..64
    (pnp_coils_check: the library's own rule, no context and no device needed).  -> (C, Ks)."""
    shape = np.shape(sens)
    if len(shape) not in (3, 4) or tuple(shape[-2:]) != (int(H), int(W)):
        raise ValueError('coils must be [C,H,W] or [Ks,C,H,W] with H x W = %d x %d (got shape %s)' % (H, W, tuple(shape)))
    Cn, Ks = int(shape[-3]), (int(shape[0]) if len(shape) == 4 else 1)
    L = _lib.lib()
    if L.pnp_coils_check(Cn, Ks, int(H), int(W)) != 0:
        raise ValueError(L.pnp_last_error().decode('utf-8', 'replace'))
    if int(cg_iters) != cg_iters or not 1 <= int(cg_iters) <= 64:
        raise ValueError('cg_iters must be an integer in 1..64 (got %r)' % (cg_iters,))
    return Cn, Ks


TRACE_FIELDS = ('r_pri', 'r_dual', 'x_norm', 'z_norm', 'w_norm', 'psnr', 're')      # PNP_TRACE_* of include/pnp_mri.h, in order


def trace_rows(sums, npix, have_gt=True):
    """Sums of squares [..., 7, B] (pnp_residuals) -> dict of the trace quantities [..., B]: square roots, and PSNR / RE by
    pnp_metrics' formulas (utils/utils_image.py:543-556, 622-636) when a ground truth went in."""
    sums = np.asarray(sums, np.float64)
    out = {name: np.sqrt(sums[..., q, :]) for q, name in enumerate(TRACE_FIELDS[:5])}
    if have_gt:
        se, sg = sums[..., 5, :], sums[..., 6, :]
        with np.errstate(divide='ignore'):
            out['psnr'] = np.where(se == 0, np.inf, 20.0 * np.log10(255.0 / np.sqrt(se / float(npix))))
        out['re'] = np.sqrt(se) / np.sqrt(sg)
    return out


def trace_meets(rows, tol):
    """The stopping rule per slice: max(r_pri, r_dual) <= tol * z_norm."""
    return np.maximum(rows['r_pri'], rows['r_dual']) <= float(tol) * rows['z_norm']


class Engine:
    """One context per (device, H, W, Bmax), H, W in [128, 1024].  Not thread-safe, not re-entrant (as the ABI says)."""

    def __init__(self, H=256, W=256, Bmax=1, device=0, precision='f32'):
        """precision='f64': the reference's own arithmetic (S4:109) -- every buffer and step in double; problem
        (upload / synthesize), state, whole loops, x, metrics and SSIM are available, the step-wise
        float32 operators of the PnP path are not (pnp_mri.h, "double-precision context")."""
        if precision not in ('f32', 'f64'):
            raise ValueError("precision must be 'f32' or 'f64'")
        self._L = _lib.lib()
        self._ctx = _lib.ctx_p()
        self.f64 = precision == 'f64'
        create = self._prec_fn('ctx_create_any')      # H, W in [128, 1024]
        _lib.check(create(int(device), int(H), int(W), int(Bmax), C.byref(self._ctx)))
        self.H, self.W, self.Bmax, self.device = int(H), int(W), int(Bmax), int(device)
        self.B = 0
        self._real = np.float64 if self.f64 else np.float32
        self._cplx = np.complex128 if self.f64 else np.complex64
        self.C = 0                                        # coils (set_coils); 0: none
        self._cx = False                                  # complex image mode (set_image_mode)

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx.value:
            self._L.pnp_ctx_destroy(self._ctx)
            self._ctx = _lib.ctx_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- plumbing -------------------------------------------------------------------------
    def set_stream(self, hip_stream):
        _lib.check(self._L.pnp_set_stream(self._ctx, C.c_void_p(int(hip_stream) if hip_stream else 0)))

    def sync(self):
        _lib.check(self._L.pnp_sync(self._ctx))

    def set_fast_path(self, enable):
        _lib.check(self._L.pnp_set_fast_path(self._ctx, 1 if enable else 0))

    def set_schedule(self, queues=2, mixed_launches=True, chunk=0):
        """Scheduling of the fused loops (bit-identical results for every setting); see pnp_set_schedule."""
        _lib.check(self._L.pnp_set_schedule(self._ctx, int(queues), 1 if mixed_launches else 0, int(chunk)))

    @property
    def schedule(self):
        q, m, ch = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self._L.pnp_get_schedule(self._ctx, C.byref(q), C.byref(m), C.byref(ch)))
        return {'queues': q.value, 'mixed': m.value, 'chunk': ch.value}

    def set_sparsity(self, wavelet=None, levels=3):
        """The penalty of admm_l1 / admm_cnc / prox_*_dual on the coefficients of the periodic 2-D DWT `wavelet` ('haar', 'db2',
        'db4') with `levels` levels instead of the pixels; None: the pixels, as ever (pnp_set_sparsity)."""
        code = check_sparsity(wavelet, levels, self.H, self.W)
        _lib.check(self._L.pnp_set_sparsity(self._ctx, code, int(levels) if wavelet is not None else 0))

    @property
    def sparsity(self):
        """(wavelet, levels) of set_sparsity; (None, 0) without one."""
        wv, lv = C.c_int(0), C.c_int(0)
        _lib.check(self._L.pnp_get_sparsity(self._ctx, C.byref(wv), C.byref(lv)))
        return {v: k for k, v in WAVELETS.items()}[wv.value], lv.value

    def set_spin(self, shifts=None, per_prox=1):
        """Cycle spinning for the wavelet prox (pnp_set_spin): `shifts` [n, 2] of (sy, sx) in [0, 2**levels), used `per_prox` per prox
        step in table order (averaged when per_prox > 1), wrapping at the end; None clears.  Needs set_sparsity first, which also
        clears it.  init_state and set_spin rewind the schedule, set_state does not (spin_cursor)."""
        if shifts is None:
            _lib.check(self._L.pnp_set_spin(self._ctx, None, 0, 1))
            return
        wavelet, levels = self.sparsity
        # without a wavelet the library refuses the call (PNP_E_STATE); with one, a bad table is a ValueError that names the rule
        t = check_spin(shifts, levels, per_prox) if wavelet is not None else np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1, 2)
        _lib.check(self._L.pnp_set_spin(self._ctx, t.ctypes.data_as(C.POINTER(C.c_int32)), int(t.shape[0]), int(per_prox)))

    @property
    def spin(self):
        """{'n', 'per_prox'} of set_spin (pnp_get_spin); n = 0 without one."""
        n, k = C.c_int(0), C.c_int(0)
        _lib.check(self._L.pnp_get_spin(self._ctx, C.byref(n), C.byref(k), None))
        return {'n': n.value, 'per_prox': k.value}

    @property
    def spin_cursor(self):
        """Prox steps since the spin schedule was last rewound: the next one uses table group spin_cursor mod (n / per_prox)."""
        p = C.c_int(0)
        _lib.check(self._L.pnp_get_spin(self._ctx, None, None, C.byref(p)))
        return p.value

    @spin_cursor.setter
    def spin_cursor(self, cursor):
        _lib.check(self._L.pnp_set_spin_cursor(self._ctx, int(cursor)))

    def set_temporal(self, frames=None, keep_dc=True):
        """Temporal sparsity (pnp_set_temporal): the batch is series of `frames` consecutive slices (2..64), and the penalty of admm_l1 /
        admm_cnc / prox_*_dual acts on the coefficients of a unitary DFT along time of every pixel's series; keep_dc: coefficient 0
        carries no penalty.  None clears.  Not together with set_sparsity / set_spin; survives set_coils and set_image_mode."""
        if frames is None:
            _lib.check(self._L.pnp_set_temporal(self._ctx, 0, 1))
            return
        _lib.check(self._L.pnp_set_temporal(self._ctx, check_temporal(frames), 1 if keep_dc else 0))

    @property
    def temporal(self):
        """(frames, keep_dc) of set_temporal (pnp_get_temporal); (None, True) without one."""
        f, k = C.c_int(0), C.c_int(0)
        _lib.check(self._L.pnp_get_temporal(self._ctx, C.byref(f), C.byref(k)))
        return (f.value or None), bool(k.value)

    def set_lowrank(self, block=None, scale=None, shifts=None):
        """Locally low-rank prox (pnp_set_lowrank), on an engine with set_temporal's series length: the prox of admm_l1 / admm_cnc /
        prox_*_dual thresholds the singular values of the block x block patches of every series across its frames, thr and ib times
        `scale` (default block / 2), on the grid anchored at `shifts` ([n, 2] of (sy, sx) in [0, block), default the single entry
        (0, 0)), one entry per prox step (lowrank_cursor).  None or 0 clears.  Real images only."""
        if not block:
            _lib.check(self._L.pnp_set_lowrank(self._ctx, 0, 0.0, None, 0))
            return
        if isinstance(block, bool) or int(block) != block:
            raise ValueError('lowrank must be an integer (got %r)' % (block,))
        t = lowrank_table(shifts, block)
        _lib.check(self._L.pnp_set_lowrank(self._ctx, int(block), float(block) / 2.0 if scale is None else float(scale),
                                           t.ctypes.data_as(C.POINTER(C.c_int32)), int(t.shape[0])))

    def _lowrank(self):
        b, s, n, p = C.c_int(0), C.c_double(0), C.c_int(0), C.c_int(0)
        _lib.check(self._L.pnp_get_lowrank(self._ctx, C.byref(b), C.byref(s), C.byref(n), C.byref(p)))
        return b.value, s.value, n.value, p.value

    @property
    def lowrank(self):
        """(block, scale, entries of the shift table) of set_lowrank (pnp_get_lowrank); None without one."""
        b, s, n, _ = self._lowrank()
        return (b, s, n) if b else None

    @property
    def lowrank_cursor(self):
        """prox steps since the cursor was last set (set_lowrank and init_state set it to 0): the next step uses entry cursor mod n"""
        return self._lowrank()[3]

    @lowrank_cursor.setter
    def lowrank_cursor(self, cursor):
        _lib.check(self._L.pnp_set_lowrank_cursor(self._ctx, int(cursor)))

    def set_coils(self, sens, cg_iters=3):
        """Multi-coil (SENSE) data consistency (pnp_set_coils): sens [C,H,W] or a bank [Ks,C,H,W] of complex sensitivity maps (host array
        or device tensor of the engine's complex type); None clears.  From then on y is [B,C,H,W], upload / synthesize take coil_id=,
        and init_state, admm_l1, admm_cnc, dc_step, A, AH follow y_c = mask . fft2(S_c . x): the x-step is `cg_iters` iterations of
        conjugate gradients (default 3: enough for maps normalised to sum_c |S_c|^2 = 1 at the presets' reo; UNNORMALISED MAPS OR A
        LARGE reo -- the in-function default 2.75 -- NEED MORE, see cg_residual).  Drops the uploaded problem."""
        if sens is None:
            _lib.check(self._prec_fn('set_coils')(self._ctx, None, 0, 0, 0))
            self.C, self.B, self._cx = 0, 0, False
            return
        Cn, Ks = check_coils(sens, self.H, self.W, cg_iters)
        dev = _is_dev(sens)
        if not dev:
            sens = _host(sens, self._cplx)
        _lib.check(self._L.pnp_set_cg(self._ctx, int(cg_iters)))
        fn = self._prec_fn('set_coils')
        _lib.check(fn(self._ctx, _ptr(sens), Cn, Ks, 1 if dev else 0))
        self.C, self.Ks, self.B, self._cx = Cn, Ks, 0, False

    def set_image_mode(self, mode='real'):
        """'complex': the loops of a coil engine keep the image phase (pnp_set_image) -- x, z, w are complex [B,H,W], z0 = A^H y,
        x = x^ of the CG x-step, the prox thresholds the modulus; init_state, admm_l1, admm_cnc, x, set_state, get_state, dc_step,
        prox_*_dual, A and the metrics follow.  Needs coils (set_coils, which also returns the engine to 'real') and no spin table; no
        trace, no residuals.  Drops the uploaded problem.  'real': as ever."""
        if mode not in IMAGE_MODES:
            raise ValueError("image must be 'real' or 'complex' (got %r)" % (mode,))
        _lib.check(self._L.pnp_set_image(self._ctx, IMAGE_MODES[mode]))
        self._cx, self.B = mode == 'complex', 0

    @property
    def image_mode(self):
        """'real' or 'complex' (pnp_get_image)"""
        m = C.c_int(0)
        _lib.check(self._L.pnp_get_image(self._ctx, C.byref(m)))
        return {v: k for k, v in IMAGE_MODES.items()}[m.value]

    def _prec_fn(self, name):
        """the entry point `name` of the engine's precision, whatever the image mode: pnp_<name>[_f64]"""
        return getattr(self._L, 'pnp_' + name + ('_f64' if self.f64 else ''))

    def _fn(self, name):
        """the entry point `name` of the engine's image mode and precision: pnp_<name>[_cx][_f64]"""
        return self._prec_fn(name + ('_cx' if self._cx else ''))

    def _step_fn(self, name):
        """the step-wise entry point `name`: in complex image mode of the engine's precision, in real mode the float32 call"""
        return self._fn(name) if self._cx else getattr(self._L, 'pnp_' + name)

    @property
    def _state_dtype(self):
        """the element type of z, w, x on the host: complex in complex image mode"""
        return self._cplx if self._cx else self._real

    @property
    def coils(self):
        """{'C', 'Ks', 'cg_iters'} (pnp_get_coils); C = 0 without coils."""
        c, k, it = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self._L.pnp_get_coils(self._ctx, C.byref(c), C.byref(k), C.byref(it)))
        return {'C': c.value, 'Ks': k.value, 'cg_iters': it.value}

    def cg_residual(self):
        """||r|| / ||A^H y + La2 (z - w)|| of the most recent x-step, per slice [B] (pnp_cg_residual; synchronises)."""
        rel = np.empty(self.B, np.float64)
        _lib.check(self._L.pnp_cg_residual(self._ctx, rel.ctypes.data_as(_lib.c_double_p)))
        return rel

    def coil_maps(self, y, mask_bank, mask_id, maps_out, lambda_out, B, Cn, calib=24, radius=2, power_iters=4, thresh=0.05):
        """Sensitivity maps from the calibration region (pnp_coil_maps; coilmaps.estimate is the array-level entry): DEVICE tensors y
        [B,C,H,W] and maps_out [B,C,H,W] of the engine's complex type, mask_bank [K,H,W] uint8, mask_id [B] int32 or None, lambda_out
        [B,H,W] real or None.  Runs on the engine's stream with its transforms and synchronises at its end; the uploaded problem, the
        state and the coils of the engine are not touched."""
        fn = self._prec_fn('coil_maps')
        _lib.check(fn(self._ctx, _ptr(y), _ptr(mask_bank), _ptr(mask_id), _ptr(maps_out), _ptr(lambda_out), int(B), int(Cn), int(calib),
                      int(radius), int(power_iters), float(thresh)))

    def espirit_maps(self, y, mask_bank, mask_id, maps_out, lambda_out, B, Cn, calib=24, kernel=4, power_iters=4, sigma=0.02, crop=0.9,
                     thresh=0.05):
        """ESPIRiT sensitivity maps (pnp_espirit_maps; coilmaps.estimate(method='espirit') is the array-level entry): the arrays of
        coil_maps.  Runs on the engine's stream with its transforms and synchronises; the uploaded problem, the state and the coils of the
        engine are not touched.  -> the signal-space rank of every slice, [B] int32."""
        fn = self._prec_fn('espirit_maps')
        _lib.check(fn(self._ctx, _ptr(y), _ptr(mask_bank), _ptr(mask_id), _ptr(maps_out), _ptr(lambda_out), int(B), int(Cn), int(calib),
                      int(kernel), int(power_iters), float(sigma), float(crop), float(thresh)))
        rank = np.empty(int(B), np.int32)
        _lib.check(self._L.pnp_espirit_ranks(self._ctx, rank.ctypes.data_as(C.c_void_p), int(B)))
        return rank

    def espirit_eigmaps(self, images, w, maps_out, lambda_out, B, Cn, kernel, power_iters):
        """The per-pixel stage of the ESPIRiT estimator alone (pnp_espirit_eigmaps): DEVICE tensors images [B,C,H,W] (low-resolution coil
        images), w [B,C,C,2k-1,2k-1] of the engine's complex type -> maps_out [B,C,H,W] (unit vectors, no support), lambda_out [B,H,W]."""
        fn = self._prec_fn('espirit_eigmaps')
        _lib.check(fn(self._ctx, _ptr(images), _ptr(w), _ptr(maps_out), _ptr(lambda_out), int(B), int(Cn), int(kernel), int(power_iters)))

    def espirit_stage_times(self, enable=True):
        """MEASUREMENT: the times (ms) of espirit_maps' three stages -- patch Gram with its read-back, host eigen-solve, per-pixel kernel
        with support -- accumulated since the previous call of this method (pnp_espirit_stage_times)."""
        ms = (C.c_float * 3)()
        _lib.check(self._L.pnp_espirit_stage_times(self._ctx, 1 if enable else 0, ms))
        return [float(v) for v in ms]

    def coil_maps_stage_times(self, enable=True):
        """MEASUREMENT: the HIP-event times (ms) of coil_maps' three stages -- window, inverse transform, eigenvectors with support --
        accumulated since the previous call of this method; enable: whether later calls are timed (pnp_coil_maps_stage_times)."""
        ms = (C.c_float * 3)()
        _lib.check(self._L.pnp_coil_maps_stage_times(self._ctx, 1 if enable else 0, ms))
        return [float(v) for v in ms]

    def _coil_id(self, coil_id, B):
        if not self.C:
            if coil_id is not None:
                raise ValueError('coil_id needs coils (set_coils)')
            return None
        cid = None if coil_id is None else _host(coil_id, np.int32)
        if cid is not None and cid.shape != (B,):
            raise ValueError('coil_id must have shape (B,)')
        return cid

    @property
    def plan(self):
        """What the next loop call does for the uploaded batch: {'queues', 'chunk', 'launches_per_iteration'} (pnp_get_plan)."""
        q, ch, n = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._L.pnp_get_plan(self._ctx, C.byref(q), C.byref(ch), C.byref(n)))
        return {'queues': q.value, 'chunk': ch.value, 'launches_per_iteration': n.value}

    @property
    def path_name(self):
        return self._L.pnp_path_name(self._ctx).decode()

    @property
    def ctx_path(self):
        """'anysize' (H, W not both in {256, 512}: the any-size FFT kernels) or, for the fixed-size kernels, path_name."""
        return self._L.pnp_ctx_path(self._ctx).decode()

    def fft_plan(self, axis):
        """The transform plan of axis 0 (rows, length W) or 1 (columns, length H) as text (pnp_fft_plan)."""
        buf = C.create_string_buffer(128)
        _lib.check(self._L.pnp_fft_plan(self._ctx, int(axis), buf, len(buf)))
        return buf.value.decode()

    @property
    def kernels_per_iteration(self):
        return self._L.pnp_kernels_per_iteration(self._ctx)

    def timer_start(self):
        _lib.check(self._L.pnp_timer_start(self._ctx))

    def timer_stop(self):
        ms = C.c_float(0)
        _lib.check(self._L.pnp_timer_stop(self._ctx, C.byref(ms)))
        return ms.value

    # -- problem --------------------------------------------------------------------------
    def _masks(self, masks, mask_id, B):
        masks = np.asarray(masks)
        if masks.ndim == 2:
            masks = masks[None]
        if masks.shape[1:] != (self.H, self.W):
            raise ValueError('mask shape %s does not match engine %dx%d' % (masks.shape[1:], self.H, self.W))
        bank = _host(masks != 0, np.uint8)
        mid = None if mask_id is None else _host(mask_id, np.int32)
        if mid is not None and mid.shape != (B,):
            raise ValueError('mask_id must have shape (B,)')
        return bank, mid

    def upload(self, y, masks, mask_id=None, coil_id=None):
        """y: [B,H,W] complex (host; cast to complex64) -- S4:102's `y`; masks [K,H,W] or [H,W].  With coils: y [B,C,H,W] (or [C,H,W]),
        coil_id [B] into the bank of maps."""
        y = np.asarray(y)
        if y.ndim == (3 if self.C else 2):
            y = y[None]
        y = _host(y, self._cplx)
        B = y.shape[0]
        want = (self.C, self.H, self.W) if self.C else (self.H, self.W)
        if y.shape[1:] != want:
            raise ValueError('y shape %s does not match engine %s' % (y.shape[1:], 'x'.join(map(str, want))))
        bank, mid = self._masks(masks, mask_id, B)
        cid = self._coil_id(coil_id, B)
        if self.C:
            up = self._prec_fn('upload_problem_mc')
            _lib.check(up(self._ctx, _ptr(y), _ptr(bank), _ptr(mid), _ptr(cid), B, bank.shape[0], 0))
            self.B = B
            return
        up = self._prec_fn('upload_problem')
        _lib.check(up(self._ctx, _ptr(y), _ptr(bank), _ptr(mid), B, bank.shape[0], 0))
        self.B = B

    def synthesize(self, img, noise, masks, mask_id=None, coil_id=None):
        """y = fft2(img)*mask + noise on the device (S4:102).  img [B,H,W] float; noise [H,W]
        (shared, the reference's noises.mat) or [B,H,W] complex.  With coils: y_c = fft2(S_c img)*mask + noise, noise [H,W],
        [C,H,W] (shared by the slices) or [B,C,H,W]; coil_id [B] into the bank of maps."""
        img = np.asarray(img)
        if img.ndim == 2:
            img = img[None]
        img = _host(img, np.float32)                      # the reference's img_L is float32 in either precision
        B = img.shape[0]
        noise = _host(noise, self._cplx)
        cid = self._coil_id(coil_id, B)
        if self.C:
            mode = {2: 0, 3: 1, 4: 2}.get(noise.ndim)
            ok = {0: (self.H, self.W), 1: (self.C, self.H, self.W), 2: (B, self.C, self.H, self.W)}
            if mode is None or noise.shape != ok[mode]:
                raise ValueError('noise shape %s is none of [H,W], [C,H,W], [B,C,H,W] of this engine' % (noise.shape,))
            bank, mid = self._masks(masks, mask_id, B)
            fn = self._prec_fn('synthesize_problem_mc')
            _lib.check(fn(self._ctx, _ptr(img), _ptr(noise), mode, _ptr(bank), _ptr(mid), _ptr(cid), B, bank.shape[0], 0))
            self.B = B
            return
        per = 1 if noise.ndim == 3 else 0
        if per and noise.shape[0] != B:
            raise ValueError('noise batch does not match images')
        if noise.shape[-2:] != (self.H, self.W):
            raise ValueError('noise shape %s does not match engine %dx%d' % (noise.shape[-2:], self.H, self.W))
        bank, mid = self._masks(masks, mask_id, B)
        fn = self._prec_fn('synthesize_problem')
        _lib.check(fn(self._ctx, _ptr(img), _ptr(noise), per, _ptr(bank), _ptr(mid), B, bank.shape[0], 0))
        self.B = B

    def download_y(self):
        y = np.empty((self.B, self.C, self.H, self.W) if self.C else (self.B, self.H, self.W), self._cplx)
        fn = self._prec_fn('download_y')
        _lib.check(fn(self._ctx, _ptr(y), 0))
        return y

    def init_state(self):
        _lib.check(self._L.pnp_init_state(self._ctx))

    def prepare_loops(self):
        """Build now the per-problem tables the whole loops will use (otherwise built by the first loop call)."""
        _lib.check(self._L.pnp_prepare_loops(self._ctx))

    def set_state(self, z=None, w=None):
        """z, w [B,H,W]: real, or complex in complex image mode (set_image_mode)"""
        dt = self._state_dtype
        zz = None if z is None else (z if _is_dev(z) else _host(z, dt))
        ww = None if w is None else (w if _is_dev(w) else _host(w, dt))
        dev = 1 if (_is_dev(z) or _is_dev(w)) else 0
        fn = self._fn('set_state')
        _lib.check(fn(self._ctx, _ptr(zz), _ptr(ww), dev))

    def get_state(self, z_out=None, w_out=None):
        """-> (z, w) as host arrays, or copied device-to-device into the given device tensors."""
        fn = self._fn('get_state')
        if z_out is not None or w_out is not None:
            if not all(o is None or _is_dev(o) for o in (z_out, w_out)):
                raise TypeError('get_state outputs must be device tensors')
            _lib.check(fn(self._ctx, _ptr(z_out), _ptr(w_out), 1))
            return z_out, w_out
        z = np.empty((self.B, self.H, self.W), self._state_dtype)
        w = np.empty_like(z)
        _lib.check(fn(self._ctx, _ptr(z), _ptr(w), 0))
        return z, w

    # -- whole loops ----------------------------------------------------------------------
    def admm_l1(self, iters, lambda1, reo, trace_every=0, tol=None, gt=None):
        """S1:111-126.  trace_every / tol / gt: the convergence trace and the stopping rule (`_traced`); both off: None, as ever."""
        if not trace_every and tol is None:
            _lib.check(self._L.pnp_admm_l1_run(self._ctx, int(iters), float(lambda1), float(reo)))
            return None
        return self._traced(self._L.pnp_admm_l1_run_traced, (int(iters), float(lambda1), float(reo)), trace_every, tol, gt)

    def admm_cnc(self, iters, alpha, lambda1, reo, b, trace_every=0, tol=None, gt=None):
        """S4:115-132.  trace_every / tol / gt as for admm_l1."""
        if not trace_every and tol is None:
            _lib.check(self._L.pnp_admm_cnc_run(self._ctx, int(iters), float(alpha), float(lambda1), float(reo), float(b)))
            return None
        return self._traced(self._L.pnp_admm_cnc_run_traced, (int(iters), float(alpha), float(lambda1), float(reo), float(b)),
                            trace_every, tol, gt)

    def _traced(self, fn, args, trace_every, tol, gt):
        """A traced run (pnp_admm_*_run_traced): a check every `trace_every` iterations and after the last one; tol: stop after the
        first check at which every slice has max(r_pri, r_dual) <= tol * z_norm (tol alone means trace_every=1); gt: uint8 [B,H,W]
        ground truth (host array or device tensor) for the psnr / re rows.  -> dict: 'iter' [C], 'r_pri', 'r_dual', 'x_norm',
        'z_norm', 'w_norm' [C, B] ('psnr', 're' with gt), 'iters_done', 'converged_at' [B] (0: never)."""
        every = 1 if (not trace_every and tol is not None) else int(trace_every)
        if every < 1:
            raise ValueError('trace_every must be >= 1 (got %r)' % (trace_every,))
        if tol is not None and not float(tol) > 0:
            raise ValueError('tol must be > 0 (got %r)' % (tol,))
        if gt is not None and not _is_dev(gt):
            gt = _host(gt, np.uint8)
            if gt.size != self.B * self.H * self.W:
                raise ValueError('gt must be [B,H,W] uint8')
        checks, done = C.c_int(0), C.c_int(0)
        _lib.check(fn(self._ctx, *args, every, float(tol) if tol is not None else 0.0, _ptr(gt), 1 if _is_dev(gt) else 0,
                      C.byref(checks), C.byref(done)))
        n = checks.value
        it = np.zeros(n, np.int32)
        vals = np.zeros((n, len(TRACE_FIELDS), self.B), np.float64)
        conv = np.zeros(self.B, np.int32)
        _lib.check(self._L.pnp_trace_read(self._ctx, _ptr(it), _ptr(vals), _ptr(conv)))
        trace = {'iter': it, 'iters_done': done.value, 'converged_at': conv}
        for q, name in enumerate(TRACE_FIELDS):
            if gt is not None or name not in ('psnr', 're'):
                trace[name] = vals[:, q, :].copy()
        return trace

    def x(self, out=None):
        """the x of the last loop, [B,H,W]: real, or complex in complex image mode"""
        fn = self._fn('download_x')
        if out is not None and _is_dev(out):
            _lib.check(fn(self._ctx, _ptr(out), 1))
            return out
        x = np.empty((self.B, self.H, self.W), self._state_dtype)
        _lib.check(fn(self._ctx, _ptr(x), 0))
        return x

    # -- step-wise operators on device tensors (PnP path) ---------------------------------
    # In complex image mode dc_step, prox_l1_dual and prox_cnc_dual take complex device tensors of the engine's precision (the _cx calls,
    # which exist in float and double); in real mode they are the float32 calls they ever were.
    def dc_step(self, z, w, x, reo):
        fn = self._step_fn('dc_step')
        _lib.check(fn(self._ctx, _ptr(z), _ptr(w), _ptr(x), float(reo)))

    def prox_l1_dual(self, x, z, w, thr):
        fn = self._step_fn('prox_l1_dual')
        _lib.check(fn(self._ctx, _ptr(x), _ptr(z), _ptr(w), float(thr)))

    def prox_cnc_dual(self, x, z, w, alpha, lambda1, reo, b):
        fn = self._step_fn('prox_cnc_dual')
        _lib.check(fn(self._ctx, _ptr(x), _ptr(z), _ptr(w), float(alpha), float(lambda1), float(reo), float(b)))

    def cnc_combine(self, z, x, w, s, t, alpha, lambda1, reo, b):
        """S6:301; complex tensors: the same expression component-wise (pnp_cnc_combine_cx)"""
        fn = self._L.pnp_cnc_combine_cx if _is_cx(z) else self._L.pnp_cnc_combine
        _lib.check(fn(self._ctx, _ptr(z), _ptr(x), _ptr(w), _ptr(s), _ptr(t), float(alpha), float(lambda1), float(reo), float(b)))

    # A real denoiser on a complex state (include/pnp_mri.h, "PnP denoisers on complex images"): complex64 device tensors [B,H,W] and the
    # float32 planes of the network -- [B,1,H,W] for mode='modulus', plane-major [2B,1,H,W] for 'parts'.  a (+ b when given) is the value
    # the network is asked about; gain: the g of 'parts'
    def cx_den_in(self, a, b, planes, mode='modulus', gain=0.5):
        _lib.check(self._L.pnp_cx_den_in(self._ctx, _ptr(a), _ptr(b), _ptr(planes), _cx_denoise(mode), float(gain)))

    def cx_den_out(self, q, a, b, z, mode='modulus', gain=0.5):
        _lib.check(self._L.pnp_cx_den_out(self._ctx, _ptr(q), _ptr(a), _ptr(b), _ptr(z), _cx_denoise(mode), float(gain)))

    def cx_den_out_dual(self, q, a, b, x, z, w, mode='modulus', gain=0.5):
        """the join of cx_den_out, then w <- w + x - z and the projection of x, z, w onto the unit disc: x, w in place, z written"""
        _lib.check(self._L.pnp_cx_den_out_dual(self._ctx, _ptr(q), _ptr(a), _ptr(b), _ptr(x), _ptr(z), _ptr(w), _cx_denoise(mode), float(gain)))

    def add(self, a, b, out):
        _lib.check(self._L.pnp_add(self._ctx, _ptr(a), _ptr(b), _ptr(out)))

    def dual_clamp(self, x, z, w):
        _lib.check(self._L.pnp_dual_clamp(self._ctx, _ptr(x), _ptr(z), _ptr(w)))

    def residuals(self, x, z, z_prev, w, gt=None, quantise=False, out=None):
        """The reduction of the traced loops on device tensors [B,H,W] in natural order (pnp_residuals): the sums of squares
        [7, B] behind a trace row (`trace_rows` forms the norms, PSNR and RE).  gt: uint8 [B,H,W], host array or device tensor;
        quantise: score round(255 x) / 255 as the PnP solvers do.  out: a float64 device tensor [7, B] -- written asynchronously on
        the engine's stream and returned -- or None: a host array, after a synchronisation."""
        if gt is not None and not _is_dev(gt):
            gt = _host(gt, np.uint8)
        fn = self._prec_fn('residuals')
        dev = out is not None
        if dev and not _is_dev(out):
            raise TypeError('residuals: out must be a device tensor (or None for a host array)')
        res = out if dev else np.empty((len(TRACE_FIELDS), self.B), np.float64)
        _lib.check(fn(self._ctx, _ptr(x), _ptr(z), _ptr(z_prev), _ptr(w), _ptr(gt), 1 if _is_dev(gt) else 0, 1 if quantise else 0,
                      _ptr(res), 1 if dev else 0))
        return res

    # -- operator API on device tensors ---------------------------------------------------
    def fft2(self, inp, out, B):
        _lib.check(self._L.pnp_fft2_fwd(self._ctx, _ptr(inp), _ptr(out), int(B)))

    def ifft2(self, inp, out, B):
        _lib.check(self._L.pnp_fft2_inv(self._ctx, _ptr(inp), _ptr(out), int(B)))

    def dwt2(self, inp, out, B, shift=None):
        """Psi of B real slices with the engine's sparsity setting (pnp_dwt2_fwd; device tensors of the engine's precision; inp may be out).
        shift=(sy, sx): Psi_s, the transform of the frame shifted by it (pnp_dwt2_shifted); None: the call as it ever was."""
        if shift is not None:
            return self._dwt2_shifted(inp, out, B, 0, shift)
        fn = self._prec_fn('dwt2_fwd')
        _lib.check(fn(self._ctx, _ptr(inp), _ptr(out), int(B)))

    def idwt2(self, inp, out, B, shift=None):
        """Psi^T (pnp_dwt2_inv); shift=(sy, sx): Psi_s^T."""
        if shift is not None:
            return self._dwt2_shifted(inp, out, B, 1, shift)
        fn = self._prec_fn('dwt2_inv')
        _lib.check(fn(self._ctx, _ptr(inp), _ptr(out), int(B)))

    def _dwt2_shifted(self, inp, out, B, inverse, shift):
        sy, sx = shift
        fn = self._prec_fn('dwt2_shifted')
        _lib.check(fn(self._ctx, _ptr(inp), _ptr(out), int(B), int(inverse), int(sy), int(sx)))

    def A(self, x, k):
        """x real [B,H,W]; in complex image mode x complex [B,H,W] (pnp_A_cx)"""
        _lib.check((self._L.pnp_A_cx if self._cx else self._L.pnp_A)(self._ctx, _ptr(x), _ptr(k)))

    def AH(self, k, out):
        _lib.check(self._L.pnp_AH(self._ctx, _ptr(k), _ptr(out)))

    def Df(self, x, out):
        _lib.check(self._L.pnp_Df(self._ctx, _ptr(x), _ptr(out)))

    def metrics(self, x_dev, gt_u8):
        """-> (psnr[B], re[B]) of img_E = x*255 against uint8 ground truth
        (utils/utils_image.py:543-556, 622-636)."""
        gt = _host(gt_u8, np.uint8)
        psnr = np.empty(self.B, np.float64)
        re = np.empty(self.B, np.float64)
        fn = self._prec_fn('metrics')
        _lib.check(fn(self._ctx, _ptr(x_dev), _ptr(gt), 0,
                      psnr.ctypes.data_as(_lib.c_double_p), re.ctypes.data_as(_lib.c_double_p)))
        return psnr, re

    def ssim(self, x_dev, gt_u8):
        """-> ssim[B] of img_E = x*255 against uint8 ground truth (utils/utils_image.py:570-615), on device."""
        gt = _host(gt_u8, np.uint8)
        out = np.empty(self.B, np.float64)
        fn = self._prec_fn('ssim')
        _lib.check(fn(self._ctx, _ptr(x_dev), _ptr(gt), 0, out.ctypes.data_as(_lib.c_double_p)))
        return out
