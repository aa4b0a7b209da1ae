"""The state and step-wise surface of a coil context, real and complex image mode alike (pnp_set_state / pnp_get_state / pnp_download_x /
pnp_dc_step / pnp_prox_l1_dual / pnp_prox_cnc_dual and their _cx / _f64 forms).

1. The loop is its steps: three iterations of pnp_admm_{l1,cnc}_run leave x, z, w bit-equal to three rounds of dc_step and prox_*_dual
   on device tensors started from get_state.  Pixel prox at 129 x 131, B = 1 (an odd element count: the float kernel's tail thread),
   db2 at 2 levels at 128 x 128, B = 2; C = 2; complex float, complex double, real float (the real step-wise calls are float only).
2. The refusal table: what each call answers to a wrong mode, a wrong precision, null pointers, bad scalars, both together, misaligned
   and overlapping arrays, and a state that is not there -- return code and message, literally.  Every input is refused by a host check
   before any launch; the misaligned and overlapping pointers lie inside a live allocation all the same."""
import ctypes

import numpy as np
import pytest

import multicoil_oracle as M

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -3
L1 = dict(lambda1=0.1, reo=0.015)
CNC = dict(alpha=0.45, lambda1=0.5, reo=0.05, b=64.0)


def problem(H, W, C, B):
    """maps [C,H,W], one mask, y [B,C,H,W] complex64: noise on the sampled points (the steps are compared with the loop, not with an oracle)"""
    rng = np.random.default_rng(H * W + B)
    m = M.mask(1, H, W)
    y = ((rng.standard_normal((B, C, H, W)) + 1j * rng.standard_normal((B, C, H, W))) * m).astype(np.complex64)
    return M.coil_maps(C, H, W, 1), m, y


def open_engine(H, W, C, B, mode, precision, wavelet=None):
    import pnp_admm_cnc_mri_amd as P
    S, m, y = problem(H, W, C, B)
    eng = P.Engine(H, W, Bmax=B, precision=precision)
    eng.set_coils(S, 3)
    eng.set_image_mode(mode)
    if wavelet:
        eng.set_sparsity(*wavelet)
    eng.upload(y, m)
    return eng


# ---- 1. the loop is its steps ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,B,wavelet', [(129, 131, 1, None), (128, 128, 2, ('db2', 2))])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('mode,precision', [('complex', 'f32'), ('complex', 'f64'), ('real', 'f32')])
def test_the_loop_is_its_steps(H, W, B, wavelet, kind, mode, precision):
    import torch
    real = torch.float64 if precision == 'f64' else torch.float32
    dt = (torch.complex128 if precision == 'f64' else torch.complex64) if mode == 'complex' else real
    with open_engine(H, W, 2, B, mode, precision, wavelet) as eng:
        eng.init_state()
        z, w, x = (torch.empty((B, H, W), dtype=dt, device='cuda') for _ in range(3))
        eng.get_state(z, w)
        if kind == 'l1':
            eng.admm_l1(3, **L1)
        else:
            eng.admm_cnc(3, **CNC)
        lx = eng.x()
        lz, lw = eng.get_state()
        for _ in range(3):
            eng.dc_step(z, w, x, (L1 if kind == 'l1' else CNC)['reo'])
            if kind == 'l1':
                eng.prox_l1_dual(x, z, w, L1['reo'] * L1['lambda1'])          # the loop's threshold: the product in double, rounded once
            else:
                eng.prox_cnc_dual(x, z, w, **CNC)
        eng.sync()
        sx, sz, sw = (t.cpu().numpy() for t in (x, z, w))
    assert np.isfinite(lx.view(lx.real.dtype)).all() and np.abs(lw).max() > 0 and np.abs(lx).max() > 0
    assert (mode == 'complex') == bool(np.iscomplexobj(lx) and np.abs(lx.imag).max() > 0)
    for name, got, ref in (('x', sx, lx), ('z', sz, lz), ('w', sw, lw)):
        assert got.dtype == ref.dtype and np.array_equal(got.view(np.uint8), ref.view(np.uint8)), name


# ---- 2. the refusal table ----------------------------------------------------------------------------------------------------------------

H = W = 128
REAL_OF_CX = 'the context is in complex image mode (pnp_set_image): use '
NEED_CX = 'needs complex image mode (pnp_set_image); in real mode use the call without _cx'
NOT_F64 = 'not available on an fp64 validation context'
NEED_F64 = 'needs a context made by pnp_ctx_create_f64'
UNDEFINED = 'z / w are undefined since the last upload / synthesize (call pnp_init_state or pnp_set_state with both z and w)'
NO_X = 'no iteration has been run since the state was set'
OVERLAP = "x, z and w must not overlap with a wavelet set (tiles read their neighbours' halo)"
CNC_OK = (0.45, 0.5, 0.05, 64.0)


def args_of(name, a, b, c):
    """the call `name` on three pointers with valid scalars"""
    if 'state' in name:
        return (a, b, 1)
    if 'download_x' in name:
        return (a, 1)
    if 'dc_step' in name:
        return (a, b, c, 0.05)
    return (a, b, c, 0.1) if 'l1' in name else (a, b, c) + CNC_OK


@pytest.mark.parametrize('mode,precision', [('real', 'f32'), ('real', 'f64'), ('complex', 'f32'), ('complex', 'f64')])
def test_refusal_table(mode, precision):
    import torch
    cx, f64 = mode == 'complex', precision == 'f64'
    sfx = ('_cx' if cx else '') + ('_f64' if f64 else '')          # this context's own forms
    with open_engine(H, W, 2, 1, mode, precision) as eng:
        lib, ctx = eng._L, eng._ctx
        buf = torch.zeros((5, H, W), dtype=torch.complex128, device='cuda')          # room for three arrays of any type, and for every offset
        plane = H * W * 16
        p, q, r = (ctypes.c_void_p(buf.data_ptr() + k * plane) for k in range(3))
        at = lambda off: ctypes.c_void_p(buf.data_ptr() + off)

        def refused(name, args, rc, msg):
            got = getattr(lib, name)(ctx, *args)
            text = lib.pnp_last_error().decode()
            print('%-28s %2d  %s' % (name, got, text))
            assert (got, text) == (rc, name + ': ' + msg), (name, args)

        # -- the state is undefined after the upload
        refused('pnp_set_state' + sfx, (p, None, 1), STATE, UNDEFINED)
        refused('pnp_set_state' + sfx, (None, q, 1), STATE, UNDEFINED)
        refused('pnp_set_state' + sfx, (None, None, 1), STATE, UNDEFINED)
        refused('pnp_get_state' + sfx, (p, q, 1), STATE, UNDEFINED)
        eng.init_state()
        # -- x before any iteration; a null x is named first
        refused('pnp_download_x' + sfx, (p, 1), STATE, NO_X)
        refused('pnp_download_x' + sfx, (None, 1), ARG, 'null')
        # -- wrong mode: every form of the other mode, in either precision (the mode is looked at first)
        for base in ('set_state', 'get_state', 'download_x', 'dc_step', 'prox_l1_dual', 'prox_cnc_dual'):
            stepwise = base in ('dc_step', 'prox_l1_dual', 'prox_cnc_dual')
            for s64 in ('', '_f64'):
                if cx and not (stepwise and s64):                              # the real step-wise calls exist in float only
                    refused('pnp_' + base + s64, args_of(base, p, q, r), STATE, REAL_OF_CX + 'pnp_' + base + '_cx' + ('' if stepwise else s64))
                if not cx:
                    refused('pnp_' + base + '_cx' + s64, args_of(base, p, q, r), STATE, NEED_CX)
            # -- wrong precision: this mode's form in the other precision
            if cx or not stepwise:
                other = 'pnp_' + base + ('_cx' if cx else '') + ('' if f64 else '_f64')
                refused(other, args_of(base, p, q, r), STATE, NOT_F64 if f64 else NEED_F64)
            elif f64:
                refused('pnp_' + base, args_of(base, p, q, r), STATE, NOT_F64)
        if not cx and f64:
            return                                                             # a real double context has no step-wise calls
        dc, l1, cnc = ('pnp_' + b + (sfx if cx else '') for b in ('dc_step', 'prox_l1_dual', 'prox_cnc_dual'))
        # -- null pointers, each position
        for k in range(3):
            ptrs = [p, q, r]
            ptrs[k] = None
            refused(dc, (*ptrs, 0.05), ARG, 'null pointer')
            refused(l1, (*ptrs, 0.1), ARG, 'null pointer')
            refused(cnc, (*ptrs, *CNC_OK), ARG, 'null pointer')
        # -- bad scalars
        nan = float('nan')
        refused(dc, (p, q, r, 0.0), ARG, 'reo must be > 0')
        refused(dc, (p, q, r, nan), ARG, 'reo must be > 0')
        refused(l1, (p, q, r, -1.0), ARG, 'thr must be >= 0')
        refused(l1, (p, q, r, nan), ARG, 'thr must be >= 0')
        refused(cnc, (p, q, r, 0.45, 0.5, 0.05, 0.0), ARG, 'b must be > 0')
        refused(cnc, (p, q, r, 0.45, -1.0, 0.05, 64.0), ARG, 'lambda1 must be >= 0 (got -1)')
        refused(cnc, (p, q, r, -0.5, 0.5, 0.05, 64.0), ARG, 'alpha must be >= 0 (got -0.5)')
        refused(cnc, (p, q, r, 0.45, 0.5, 0.0, 64.0), ARG, 'reo must be > 0 (got 0)')
        refused(cnc, (p, q, r, -0.5, -1.0, 0.0, 0.0), ARG, 'b must be > 0')                    # b, then lambda1, alpha, reo
        refused(cnc, (p, q, r, -0.5, -1.0, 0.0, 64.0), ARG, 'lambda1 must be >= 0 (got -1)')
        refused(cnc, (p, q, r, -0.5, 0.5, 0.0, 64.0), ARG, 'alpha must be >= 0 (got -0.5)')
        # -- a null pointer and a bad scalar together: the real prox calls name the pointer, the complex ones the scalar; dc_step the pointer
        refused(dc, (None, q, r, 0.0), ARG, 'null pointer')
        refused(l1, (p, None, r, -1.0), ARG, 'thr must be >= 0' if cx else 'null pointer')
        refused(cnc, (p, q, None, 0.45, 0.5, 0.05, 0.0), ARG, 'b must be > 0' if cx else 'null pointer')
        refused(cnc, (None, q, r, 0.45, -1.0, 0.05, 64.0), ARG, 'lambda1 must be >= 0 (got -1)' if cx else 'null pointer')
        if cx:
            # -- misaligned complex arrays: one complex value for the x-step, 16 bytes for the pixel prox; after null and scalars
            one = 16 if f64 else 8
            for off in (4, 8):
                if off % one:
                    refused(dc, (at(off), q, r, 0.05), ARG, 'complex arrays must be %d-byte aligned' % one)
                    refused(dc, (p, q, at(2 * plane + off), 0.05), ARG, 'complex arrays must be %d-byte aligned' % one)
                    refused(dc, (at(off), q, r, 0.0), ARG, 'reo must be > 0')
                refused(l1, (p, at(plane + off), r, 0.1), ARG, 'complex arrays must be 16-byte aligned')
                refused(cnc, (at(off), q, r, *CNC_OK), ARG, 'complex arrays must be 16-byte aligned')
                refused(l1, (None, at(plane + off), r, 0.1), ARG, 'null pointer')
        # -- with a wavelet set: overlapping arrays, after null pointers, scalars and (complex) the alignment to one complex value
        eng.set_sparsity('db2', 2)
        half = plane // 32                                       # inside the first array of either type, 16-byte aligned
        for a, b, c in ((p, p, r), (p, q, p), (p, q, q), (p, at(half), r), (at(plane + half), q, r), (p, q, at(plane - 16))):
            refused(l1, (a, b, c, 0.1), ARG, OVERLAP)
            refused(cnc, (a, b, c, *CNC_OK), ARG, OVERLAP)
        refused(l1, (p, p, None, 0.1), ARG, 'null pointer')
        refused(l1, (p, p, r, -1.0), ARG, 'thr must be >= 0')
        refused(cnc, (p, p, r, 0.45, 0.5, 0.05, -2.0), ARG, 'b must be > 0')
        if cx:
            one = 16 if f64 else 8
            off = 8 if f64 else 4
            refused(l1, (p, at(plane + off), r, 0.1), ARG, 'complex arrays must be %d-byte aligned' % one)
            refused(cnc, (p, q, at(2 * plane + off), *CNC_OK), ARG, 'complex arrays must be %d-byte aligned' % one)
            refused(l1, (p, at(off), r, 0.1), ARG, 'complex arrays must be %d-byte aligned' % one)          # misaligned and overlapping
        eng.set_sparsity(None)
