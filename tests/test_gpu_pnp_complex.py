"""The plug-and-play solvers on complex images (image='complex' on PNP_ADMM_L1_D / PNP_ADMM_CNC_D / PNP_ADMM_CNC_DnCNN) on the GPU: the
glue kernels of kernels_pnp_cx.hip bit for bit against the float32 restatement of tests/pnp_complex_oracle.py, the refusals of the four
C calls, the solvers against their loop written out on the Engine, against the complex128 / float64 oracle, phase equivariance, resume,
sharding, and the real mode before and after.

Set-up: C = 2 coils, a bank of two masks with mask_id = [1, 0, 1], contexts of Bmax = 7; maps and y rounded to complex64 once.
Shapes 128 x 128, 128 x 130, 130 x 131 and 129 x 131 with B = 1 and B = 3: B H W takes all four residues mod 4 -- the second plane of 'parts'
is 16-byte aligned for one of them only -- and is odd for some.
Bars of the oracle tests: FREEDOM (4, tests/denoiser_oracle.py) x the distance of the oracle's own complex64 / float32 CPU restatement from
it ON THE SAME CASE, computed here per case and slice and printed; relative L2 over all pixels.  On the CPU, before any kernel ran, the
10-iteration restatement distances of all sixteen cases were 4.6e-7 .. 7.9e-6: none is expansive (1e-4), so the seeded DnCNN stays.
The trained FFDNet runs B = 3 slices; the 17-layer DnCNN, whose float64 CPU forward costs ten times as much, the first slice (B = 1)."""
import ctypes
import functools

import numpy as np
import pytest

import complex_oracle as X
import multicoil_oracle as M
import pnp_complex_oracle as PO
from conftest import rel_l2, weights_trained
from denoiser_oracle import FREEDOM

pytestmark = pytest.mark.gpu

C64, C128, F32 = np.complex64, np.complex128, np.float32
BMAX, NC = 7, 2
MID = PO.MID
SHAPES = [(128, 128), (128, 130), (130, 131), (129, 131)]
GAIN = {'modulus': 0.5, 'parts': 0.3}                       # 'parts' at a gain that is not a power of two: the division rounds
CNC = dict(alpha=0.9, lambda1=1.35, reo=0.45, b=0.3)        # PRESETS['PNP_ADMM_CNC_D']['ffdnet']
PAR = {('l1', 'ffdnet_gray'): dict(reo=0.25), ('cnc', 'ffdnet_gray'): CNC,
       ('l1', 'dncnn_15'): dict(reo=0.15), ('cnc', 'dncnn_15'): dict(alpha=1.2, lambda1=4, reo=0.45, b=0.3)}


@pytest.fixture(scope='module')
def env():
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1 and torch.cuda.is_available()
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    return dict(torch=torch, P=P)


@functools.lru_cache(maxsize=None)
def case(H, W):
    S, masks, y = PO.case(H, W, NC)
    for a in (S, masks, y):
        a.setflags(write=False)
    return S, masks, y


@functools.lru_cache(maxsize=None)
def weights(name):
    if name == 'ffdnet_gray':
        return weights_trained(name)
    from pnp_admm_cnc_mri_amd import denoisers as D
    return D.seeded_state_dict(D.build(name)[0], 11)


def dev(a, dt=C64):
    import torch
    return torch.from_numpy(np.array(a, dtype=dt, order='C')).to('cuda')


def same_bits(got, want):
    """bit for bit, a NaN for a NaN (the payload and sign of a NaN are not the arithmetic's business); the sign of a zero counts"""
    g, w = np.ascontiguousarray(got).view(F32).ravel(), np.ascontiguousarray(want).view(F32).ravel()
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])


def glue_engine(P, H, W, nb):
    """a complex-mode context with nb slices uploaded: the glue calls take their size from it"""
    eng = P.Engine(H, W, Bmax=BMAX)
    eng.set_coils(M.coil_maps(NC, H, W, 1))
    eng.set_image_mode('complex')
    eng.upload(np.zeros((nb, NC, H, W), C64), M.mask(1, H, W))
    return eng


# ---- 1. the glue kernels, per element, bit for bit ---------------------------------------------------------------------------------------

DEN = F32(1e-45)
SPECIAL = np.array([0, complex(-0.0, -0.0), complex(DEN, -2 * DEN), 1, -1j, complex(np.nan, 0.25), complex(0.25, np.inf), 3e-20 - 4e-20j,
                    complex(-0.0, 0.0), 0.6 + 0.8j, 3 - 4j, complex(2e-23, 0)], C64)


def glue_inputs(n, N, seed):
    """a, b, x, w [n] complex64 and q [2 n] float32 (the network's answer: in [-0.25, 1.25], negative values among them); the special
    values of tests/host/pnp_cx_emulation.cpp stand in `a` (b = 0 there) at the first, the last and the tail elements of every slice"""
    rng = np.random.default_rng(seed)
    a, b, x, w = ((s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(C64) for s in (0.5, 0.3, 0.6, 0.4))
    q = rng.uniform(-0.25, 1.25, 2 * n).astype(F32)
    k = len(SPECIAL) // 2
    for s in range(n // N):
        for idx, val in zip(list(range(s * N, s * N + k)) + list(range((s + 1) * N - k, (s + 1) * N)), SPECIAL):
            a[idx], b[idx] = val, 0
    q[0], q[n - 1], q[n], q[2 * n - 1] = -0.5, np.nan, -0.125, 0.0
    x[1], w[1] = 3 - 4j, 0.5j                                 # outside the disc
    x[n - 2], w[n - 2] = 1, -1                                # on the circle
    return a, b, x, w, q


@pytest.mark.parametrize('mode', PO.MODES)
@pytest.mark.parametrize('nb', [1, 3])
@pytest.mark.parametrize('H,W', SHAPES)
def test_glue_kernels_bit_for_bit(env, H, W, nb, mode):
    """den_in, den_out, den_out_dual with b null and b given -- den_out_dual also with a = x, b = w, in place, as the L1 loop calls it -- and
    cnc_combine on complex tensors against the float32 NumPy restatement: the same correctly rounded +, *, /, sqrt in the same order.
    Every output is one element longer than needed and the guard element stays."""
    torch, P = env['torch'], env['P']
    N, g = H * W, GAIN[mode]
    n, npl = nb * N, 2 if mode == 'parts' else 1
    a, b, x, w, q = glue_inputs(n, N, 7 * H + W + nb)
    q = q[:npl * n]
    guard_c, guard_f = C64(7 - 7j), F32(7)

    def out_c():
        return torch.full((n + 1,), complex(guard_c), dtype=torch.complex64, device='cuda')

    with glue_engine(P, H, W, nb) as eng:
        ta, tb, tq = dev(a), dev(b), dev(q, F32)
        for bb, tbb in ((None, None), (b, tb)):
            v = a if bb is None else (a + bb).astype(C64)
            tag = '%s %dx%dx%d b %s' % (mode, nb, H, W, 'null' if bb is None else 'given')
            planes = torch.full((npl * n + 1,), float(guard_f), dtype=torch.float32, device='cuda')
            eng.cx_den_in(ta, tbb, planes, mode, g)
            z = out_c()
            eng.cx_den_out(tq, ta, tbb, z, mode, g)
            xd, wd, zd = out_c(), out_c(), out_c()
            xd[:n], wd[:n] = dev(x), dev(w)
            eng.cx_den_out_dual(tq, ta, tbb, xd, zd, wd, mode, g)
            eng.sync()
            planes, z, xd, zd, wd = (t.cpu().numpy() for t in (planes, z, xd, zd, wd))
            assert planes[-1] == guard_f and all(t[-1] == guard_c for t in (z, xd, zd, wd)), tag
            with np.errstate(all='ignore'):
                assert same_bits(planes[:-1], PO.den_in(v, mode, g, C64)), tag
                assert same_bits(z[:-1], PO.den_out(q.reshape(npl, n), v, mode, g, C64)), tag
                rx, rz, rw = PO.den_out_dual(q.reshape(npl, n), v, x, w, mode, g, C64)
            assert same_bits(xd[:-1], rx) and same_bits(zd[:-1], rz) and same_bits(wd[:-1], rw), tag
        # in place, as the L1 loop calls it: a = x, b = w
        xd, wd, zd = out_c(), out_c(), out_c()
        xd[:n], wd[:n] = dev(x), dev(w)
        eng.cx_den_out_dual(tq, xd, wd, xd, zd, wd, mode, g)
        # S6:301 on complex arrays
        t = out_c()
        eng.cnc_combine(ta, dev(x), dev(w), tb, t, **CNC)
        eng.sync()
        xd, zd, wd, t = (u.cpu().numpy() for u in (xd, zd, wd, t))
    with np.errstate(all='ignore'):
        rx, rz, rw = PO.den_out_dual(q.reshape(npl, n), (x + w).astype(C64), x, w, mode, g, C64)
        rt = PO.combine(a, x, w, b, dt=C64, **CNC)
    assert same_bits(xd[:-1], rx) and same_bits(zd[:-1], rz) and same_bits(wd[:-1], rw) and all(u[-1] == guard_c for u in (xd, zd, wd))
    assert same_bits(t[:-1], rt) and t[-1] == guard_c
    # the restatement itself did what the header says on the planted values
    if mode == 'modulus':
        z0 = PO.den_out(q.reshape(npl, n), a, mode, g, C64)
        assert z0[0] == C64(-0.5) and z0[1].real == q[1] and z0[1].imag == 0 and z0[2].real == q[2] and z0[2].imag == 0
        assert np.isnan(z0[5].real) and np.isnan(z0[n - 1].real)
    assert abs(abs(rx[1]) - 1) <= 2.0 ** -22 and rx[n - 2] == 1


# ---- 2. refusals: every return code and message ------------------------------------------------------------------------------------------

def test_refusals_of_the_four_calls(env):
    torch, P = env['torch'], env['P']
    from pnp_admm_cnc_mri_amd import _lib
    L = _lib.lib()
    H, W, nb = 128, 130, 3
    n = nb * H * W
    a, q, z, x, w = (torch.zeros(2 * n + 8, dtype=torch.float32, device='cuda') for _ in range(5))
    pa, pq, pz, px, pw = (ctypes.c_void_p(t.data_ptr()) for t in (a, q, z, x, w))
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 8)

    def calls(ctx, A=pa, Bp=None, Q=pq, Z=pz, Xp=px, Wp=pw, mode=0, gain=0.5):
        return (('pnp_cx_den_in', lambda: L.pnp_cx_den_in(ctx, A, Bp, Q, mode, gain)),
                ('pnp_cx_den_out', lambda: L.pnp_cx_den_out(ctx, Q, A, Bp, Z, mode, gain)),
                ('pnp_cx_den_out_dual', lambda: L.pnp_cx_den_out_dual(ctx, Q, A, Bp, Xp, Z, Wp, mode, gain)))

    def refused(pairs, code, text):
        for name, fn in pairs:
            assert fn() == code and L.pnp_last_error().decode() == name + ': ' + text, (name, L.pnp_last_error())

    combine = lambda ctx, Z=pz, T=pq: [('pnp_cnc_combine_cx', lambda: L.pnp_cnc_combine_cx(ctx, Z, px, pw, pa, T, 0.9, 1.35, 0.45, 0.3))]
    with glue_engine(P, H, W, nb) as eng:
        ctx = eng._ctx
        refused(calls(None) + tuple(combine(None)), -1, 'ctx is null')
        refused(calls(ctx, A=None), -1, 'null pointer')
        refused(calls(ctx, Q=None), -1, 'null pointer')
        refused(calls(ctx, Z=None)[1:], -1, 'null pointer')
        refused(calls(ctx, Xp=None)[2:] + calls(ctx, Wp=None)[2:], -1, 'null pointer')
        refused(combine(ctx, Z=None) + combine(ctx, T=None), -1, 'null pointer')
        refused(calls(ctx, mode=7), -1, 'mode must be PNP_CX_DENOISE_MODULUS (0) or PNP_CX_DENOISE_PARTS (1) (got 7)')
        refused(calls(ctx, mode=-1), -1, 'mode must be PNP_CX_DENOISE_MODULUS (0) or PNP_CX_DENOISE_PARTS (1) (got -1)')
        for gain, text in ((0.0, '0'), (-1.0, '-1'), (float('nan'), 'nan'), (float('inf'), 'inf'), (1e-60, '1e-60'), (1e60, '1e+60')):
            for mode in (0, 1):                                  # 'modulus' checks the gain it does not use
                refused(calls(ctx, mode=mode, gain=gain), -1, 'gain must be finite and > 0 (got %s)' % text)
        refused(calls(ctx, mode=7, gain=0.0), -1, 'mode must be PNP_CX_DENOISE_MODULUS (0) or PNP_CX_DENOISE_PARTS (1) (got 7)')   # the first broken rule
        align = 'the complex arrays and the plane base must be 16-byte aligned'
        refused(calls(ctx, A=off(a)) + calls(ctx, Bp=off(a)) + calls(ctx, Q=off(q)), -1, align)
        refused(calls(ctx, Z=off(z))[1:] + calls(ctx, Xp=off(x))[2:] + calls(ctx, Wp=off(w))[2:], -1, align)
        refused(combine(ctx, Z=off(z)) + combine(ctx, T=off(q)), -1, align)
        refused(calls(ctx, A=off(a), mode=7), -1, 'mode must be PNP_CX_DENOISE_MODULUS (0) or PNP_CX_DENOISE_PARTS (1) (got 7)')
        # the accepted call, and the real glue calls on a complex-mode context: what they always answered -- B H W floats of real arithmetic
        assert all(fn() == 0 for _, fn in calls(ctx) + calls(ctx, mode=1, Bp=pw) + tuple(combine(ctx)))
        rng = np.random.default_rng(2)
        hx, hz, hw = (rng.uniform(-1, 2, n).astype(F32) for _ in range(3))
        tx, tz, tw, tt = dev(hx, F32), dev(hz, F32), dev(hw, F32), torch.zeros(n, dtype=torch.float32, device='cuda')
        eng.add(tx, tw, tt)
        eng.sync()
        assert np.array_equal(tt.cpu().numpy(), hx + hw)
        assert L.pnp_cnc_combine(ctx, ctypes.c_void_p(tz.data_ptr()), ctypes.c_void_p(tx.data_ptr()), ctypes.c_void_p(tw.data_ptr()),
                                 ctypes.c_void_p(tz.data_ptr()), ctypes.c_void_p(tt.data_ptr()), 0.9, 1.35, 0.45, 0.3) == 0
        eng.dual_clamp(tx, tz, tw)
        eng.sync()
        assert np.array_equal(tt.cpu().numpy(), (F32(1 - 0.9) * hz + F32(0.9) * (hx + hw)).astype(F32) + F32(0.9 * 0.45 * 1.35 * 0.3) * (hz - hz))
        assert np.array_equal(tx.cpu().numpy(), np.clip(hx, 0, 1)) and np.array_equal(tw.cpu().numpy(), np.clip(hw + hx - hz, 0, 1))
        # no problem uploaded
        eng.set_image_mode('complex')
        refused(calls(ctx) + tuple(combine(ctx)), -3, 'no problem uploaded')
        # real image mode
        eng.set_image_mode('real')
        eng.upload(np.zeros((nb, NC, H, W), C64), M.mask(1, H, W))
        refused(calls(ctx) + tuple(combine(ctx)), -3, 'needs complex image mode (pnp_set_image)')
        refused(calls(ctx, mode=7, A=off(a)), -3, 'needs complex image mode (pnp_set_image)')
        refused(calls(ctx, A=None), -1, 'null pointer')
    with P.Engine(H, W, Bmax=BMAX, precision='f64') as e64:
        e64.set_coils(M.coil_maps(NC, H, W, 1))
        e64.set_image_mode('complex')
        e64.upload(np.zeros((nb, NC, H, W), C128), M.mask(1, H, W))
        refused(calls(e64._ctx) + tuple(combine(e64._ctx)), -3, 'not available on an fp64 validation context')
        with pytest.raises(_lib.PnpError, match='pnp_cx_den_in: not available on an fp64 validation context'):
            e64.cx_den_in(a, None, q)


# ---- 3. the solvers against their loop written out ---------------------------------------------------------------------------------------

def written_out(env, kind, names, H, W, nb, mode, gain, iters, par, cnn_batch=None, x8=False, state0=None, iter_start=0):
    """the loop of solvers_pnp.py's docstring on Engine.dc_step, the cx_den_* calls and the same Denoiser -> (x, z, w) complex64 [nb,H,W]"""
    torch, P = env['torch'], env['P']
    from pnp_admm_cnc_mri_amd import solvers_pnp as SP
    S, masks, y = case(H, W)
    d = torch.device('cuda', 0)
    dens = [SP._load_model(nm, weights(nm), 'model_zoo', iters, None, x8, cnn_batch, d, shape=(H, W)) for nm in names]
    with torch.no_grad(), P.Engine(H, W, Bmax=nb) as eng:
        eng.set_stream(torch.cuda.current_stream(d).cuda_stream)
        eng.set_coils(S, 3)
        eng.set_image_mode('complex')
        eng.upload(y[:nb], masks, MID[:nb])
        eng.init_state()
        z, w, s, t, zn = (torch.empty((nb, 1, H, W), dtype=torch.complex64, device=d) for _ in range(5))
        eng.get_state(z, w)
        if state0 is not None:
            z.copy_(dev(state0[0]).reshape(z.shape))
            w.copy_(dev(state0[1]).reshape(w.shape))
        x = z.clone()
        p = torch.empty(((2 if mode == 'parts' else 1) * nb, 1, H, W), dtype=torch.float32, device=d)
        q = torch.empty_like(p)
        for i in range(iter_start, iters):
            eng.dc_step(z, w, x, par['reo'])
            if kind == 'l1':
                eng.cx_den_in(x, w, p, mode, gain)
                dens[0](p, i, out=q)
                eng.cx_den_out_dual(q, x, w, x, z, w, mode, gain)
            else:
                eng.cx_den_in(z, None, p, mode, gain)
                dens[0](p, i, out=q)
                eng.cx_den_out(q, z, None, s, mode, gain)
                eng.cnc_combine(z, x, w, s, t, par['alpha'], par['lambda1'], par['reo'], par['b'])
                eng.cx_den_in(t, None, p, mode, gain)
                dens[-1](p, i, out=q)
                eng.cx_den_out_dual(q, t, None, x, zn, w, mode, gain)
                z, zn = zn, z
        torch.cuda.current_stream(d).synchronize()
        return tuple(u.reshape(nb, H, W).cpu().numpy() for u in (x, z, w))


def solve(env, solver, names, H, W, nb, mode, gain, iters, par, tmp_path, **kw):
    """the entry point with image='complex' -> (out, info)"""
    S, masks, y = case(H, W)
    fn = getattr(env['P'], solver)
    kw = dict(dict(y=y[:nb], mask_id=MID[:nb], coils=S, image='complex', cx_denoise=mode, cx_gain=gain, iter_num=iters, return_info=True,
                   results=str(tmp_path), model=weights(names[0])), **kw)
    res = fn(*names, masks, None, **kw, **par)
    return res[0], res[-1]


LOOPS = [('PNP_ADMM_L1_D', 'l1', ('ffdnet_gray',), 128, 130, 3, None), ('PNP_ADMM_L1_D', 'l1', ('ffdnet_gray',), 129, 131, 1, None),
         ('PNP_ADMM_CNC_D', 'cnc', ('ffdnet_gray',), 130, 131, 3, None), ('PNP_ADMM_CNC_D', 'cnc', ('ffdnet_gray',), 128, 130, 3, 2),
         ('PNP_ADMM_CNC_DnCNN', 'cnc', ('dncnn_15', 'dncnn_15'), 129, 131, 1, None), ('PNP_ADMM_L1_D', 'l1', ('ffdnet_gray',), 128, 128, 3, 2)]


@pytest.mark.parametrize('mode', PO.MODES)
@pytest.mark.parametrize('solver,kind,names,H,W,nb,cnn_batch', LOOPS)
def test_solver_is_its_loop_written_out(env, solver, kind, names, H, W, nb, cnn_batch, mode, tmp_path):
    """3 iterations, bit for bit: x (as `out`, complex128 slices), z and w.  The L1 solver builds its FFDNet in x8 mode (S3:87), which
    acts on whatever planes it is handed; cnn_batch=2 on B = 3 chunks the planes (3 + 1 of 'parts'' six).  The DnCNN pair loads the
    first network twice (faithful_model2_path)."""
    par = PAR[(kind, names[0])]
    out, info = solve(env, solver, names, H, W, nb, mode, GAIN[mode], 3, par, tmp_path, cnn_batch=cnn_batch)
    x, z, w = written_out(env, kind, names[:1] * len(names), H, W, nb, mode, GAIN[mode], 3, par, cnn_batch, x8=solver == 'PNP_ADMM_L1_D')
    assert info['image'] == 'complex' and info['cx_denoise'] == mode and len(out) == 22
    for b in range(nb):
        assert out[b].dtype == C128 and out[b].shape == (H, W) and np.array_equal(out[b], x[b].astype(C128)), b
    assert info['z'].dtype == C64 and np.array_equal(info['z'], z) and np.array_equal(info['w'], w)
    assert np.abs(x.imag).max() > 0.01 * np.abs(x).max() and np.abs(x).max() <= 1 + 2.0 ** -22 and np.isfinite(x.view(F32)).all()


def test_return_device_metrics_and_sharding(env, tmp_path):
    """return_device=True: one complex64 tensor; the metrics are those of round(255 |x|) / 255; solve_sharded (no process group: a plain
    call) gathers the same complex slices"""
    import functools as ft
    torch, P = env['torch'], env['P']
    from oracle import admm_oracle as O
    H, W, nb = 128, 130, 3
    S, masks, y = case(H, W)
    gt = np.stack([np.round(255 * np.clip(np.abs(X.truth(10 * H + b, H, W)), 0, 1)) for b in range(nb)]).astype(np.uint8)
    out, info = solve(env, 'PNP_ADMM_L1_D', ('ffdnet_gray',), H, W, nb, 'modulus', 0.5, 2, dict(reo=0.25), tmp_path, images=gt)
    xt, _ = solve(env, 'PNP_ADMM_L1_D', ('ffdnet_gray',), H, W, nb, 'modulus', 0.5, 2, dict(reo=0.25), tmp_path, return_device=True)
    assert torch.is_tensor(xt) and xt.dtype == torch.complex64 and xt.shape == (nb, H, W) and xt.is_cuda
    assert np.array_equal(xt.cpu().numpy().astype(C128), np.stack(out[:nb]))
    for b in range(nb):
        xq = np.round(255.0 * np.abs(out[b].astype(C64)).astype(F32)).astype(np.float64)
        assert abs(info['psnr'][b] - O.calculate_psnr(xq, gt[b])) <= 1e-3, (b, info['psnr'][b])
    got = P.sharding.solve_sharded(ft.partial(P.PNP_ADMM_L1_D, 'ffdnet_gray', model=weights('ffdnet_gray'), results=str(tmp_path)), masks, None,
                                   y=y[:nb], mask_id=MID[:nb], coils=S, image='complex', iter_num=2, reo=0.25)
    assert got.dtype == C64 and np.array_equal(got.astype(C128), np.stack(out[:nb]))


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle(kind, name, H, W, nb, mode):
    """{iterations: x [nb,H,W]} of the complex128 / float64 oracle and of its complex64 / float32 restatement, 3 and 10 iterations of one run"""
    S, masks, y = case(H, W)
    ref, low = {3: [], 10: []}, {3: [], 10: []}
    for dt, store in ((C128, ref), (C64, low)):
        net = PO.cpu_net(name, weights(name), dt)
        for b in range(nb):
            kept = PO.pnp(y[b], S, masks[MID[b]], 10, kind, (net,), mode, GAIN[mode], dt=dt, keep=(3, 10), **PAR[(kind, name)])[3]
            for k in (3, 10):
                store[k].append(kept[k][0])
    return ref, low


@pytest.mark.parametrize('iters', [3, 10])
@pytest.mark.parametrize('mode', PO.MODES)
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
@pytest.mark.parametrize('name', ['ffdnet_gray', 'dncnn_15'])
@pytest.mark.parametrize('H,W', [(128, 130), (129, 131)])
def test_against_the_oracle(env, H, W, name, kind, mode, iters, tmp_path):
    nb = 3 if name == 'ffdnet_gray' else 1
    solver, names = {('l1', 'ffdnet_gray'): ('PNP_ADMM_L1_D', (name,)), ('l1', 'dncnn_15'): ('PNP_ADMM_L1_D', (name,)),
                     ('cnc', 'ffdnet_gray'): ('PNP_ADMM_CNC_D', (name,)), ('cnc', 'dncnn_15'): ('PNP_ADMM_CNC_DnCNN', (name, name))}[(kind, name)]
    ref, low = oracle(kind, name, H, W, nb, mode)
    out, _ = solve(env, solver, names, H, W, nb, mode, GAIN[mode], iters, PAR[(kind, name)], tmp_path)
    for b in range(nb):
        d32 = rel_l2(low[iters][b], ref[iters][b])
        err, bar = rel_l2(out[b], ref[iters][b]), FREEDOM * d32
        print('%s %s %s %dx%d it %d slice %d: %.2e (restatement %.2e, bar %.2e)' % (name, kind, mode, H, W, iters, b, err, d32, bar))
        assert d32 <= 1e-4, 'an expansive case: replace the fixture'
        assert err <= bar, (b, err, bar)


# ---- 5. phase equivariance on the card -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('solver,kind', [('PNP_ADMM_L1_D', 'l1'), ('PNP_ADMM_CNC_D', 'cnc')])
def test_phase_equivariance_of_the_modulus_mode(env, solver, kind, tmp_path):
    """y e^{0.7 i} against x e^{0.7 i}, 3 iterations.  The turned y is rounded to complex64 again, so the two runs differ by roundings of the
    data and of every step: the bar is 4 x the same figure of the oracle's float32 restatement, per slice."""
    H, W, nb, name = 128, 130, 3, 'ffdnet_gray'
    S, masks, y = case(H, W)
    th = np.exp(0.7j)
    yt = (y * th).astype(C64).astype(C128)
    par = PAR[(kind, name)]
    a, _ = solve(env, solver, (name,), H, W, nb, 'modulus', 0.5, 3, par, tmp_path)
    b, _ = solve(env, solver, (name,), H, W, nb, 'modulus', 0.5, 3, par, tmp_path, y=yt[:nb])
    net = PO.cpu_net(name, weights(name), C64)
    for k in range(nb):
        m = masks[MID[k]]
        ra, rb = (PO.pnp(v[k], S, m, 3, kind, (net,), 'modulus', dt=C64, **par)[0] for v in (y, yt))
        fig = rel_l2(rb, ra.astype(C128) * th)
        err = rel_l2(b[k], a[k] * th)
        print('equivariance %s slice %d: %.2e (restatement %.2e, bar %.2e)' % (kind, k, err, fig, 4 * fig))
        assert err <= 4 * fig and fig < 1e-5, (k, err, fig)


# ---- 6. resume ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('solver,kind,mode', [('PNP_ADMM_L1_D', 'l1', 'modulus'), ('PNP_ADMM_L1_D', 'l1', 'parts'), ('PNP_ADMM_CNC_D', 'cnc', 'parts'),
                                              ('PNP_ADMM_CNC_D', 'cnc', 'modulus')])
def test_resume_is_bit_equal_to_the_uncut_run(env, solver, kind, mode, tmp_path):
    """state0 = the complex (z, w) after 2 iterations, iter_start = 2 of 4: the uncut run's bits"""
    H, W, nb, names = 129, 131, 3, ('ffdnet_gray',)
    par = PAR[(kind, names[0])]
    full, fi = solve(env, solver, names, H, W, nb, mode, GAIN[mode], 4, par, tmp_path)
    _, half = solve(env, solver, names, H, W, nb, mode, GAIN[mode], 2, par, tmp_path)
    assert np.iscomplexobj(half['z']) and np.iscomplexobj(half['w']) and np.abs(half['w']).max() > 0
    rest, ri = solve(env, solver, names, H, W, nb, mode, GAIN[mode], 4, par, tmp_path, state0=(half['z'], half['w']), iter_start=2)
    assert all(np.array_equal(rest[b], full[b]) for b in range(nb)) and np.array_equal(ri['z'], fi['z']) and np.array_equal(ri['w'], fi['w'])
    assert not np.array_equal(half['z'], fi['z'])


# ---- 7. the real mode is untouched ---------------------------------------------------------------------------------------------------------

def test_real_mode_before_and_after_a_complex_solve(env, tmp_path, monkeypatch):
    """a real coil PNP_ADMM_L1_D solve gives the same bits, on the same path, before and after complex PnP solves in the same process"""
    P = env['P']
    from pnp_admm_cnc_mri_amd import solvers
    H, W, nb = 128, 130, 3
    S, masks, y = case(H, W)
    paths = []

    class Recording(solvers.Engine):
        def close(self):
            if getattr(self, '_ctx', None) is not None and self._ctx.value:
                paths.append((self.image_mode, self.path_name))
            super().close()

    monkeypatch.setattr(solvers, 'Engine', Recording)

    def real():
        out, info = P.PNP_ADMM_L1_D('ffdnet_gray', masks, None, y=y[:nb], mask_id=MID[:nb], coils=S, iter_num=3, reo=0.25, return_info=True,
                                    results=str(tmp_path), model=weights('ffdnet_gray'))
        return np.stack(out[:nb]), info

    before, bi = real()
    for mode in PO.MODES:
        solve(env, 'PNP_ADMM_CNC_D', ('ffdnet_gray',), H, W, nb, mode, GAIN[mode], 2, CNC, tmp_path)
    after, ai = real()
    assert before.dtype == np.float64 and 'image' not in bi and 'cx_denoise' not in bi
    assert np.array_equal(before, after) and np.array_equal(bi['z'], ai['z']) and np.array_equal(bi['w'], ai['w'])
    assert [p[0] for p in paths] == ['real', 'complex', 'complex', 'real'] and paths[0] == paths[-1]
