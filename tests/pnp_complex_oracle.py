"""NumPy oracle of the plug-and-play loops on complex images -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Not a test module; CPU only.

A restatement of include/pnp_mri.h ("PnP denoisers on complex images") and of the solvers' docstring (solvers_pnp.py, image='complex'),
written from that text, on tests/complex_oracle.py's init_state / x_step / cclip:

    modulus:  m = |v|, d = D(m);  D(v) = (d / m) v where m != 0, (d, 0) where m == 0
    parts:    P = (0.5 + g Re v, 0.5 + g Im v), Q = D(P) in one call on the two planes;  D(v) = ((Q0 - 0.5) / g, (Q1 - 0.5) / g)
    L1:   x = x_step(z, w);  z+ = D(x + w);  w+ = (w + x) - z+;  x, z+, w+ <- cclip(., 1)
    CNC:  x = x_step(z, w);  s = D(z);  t = c1 z + c2 (x + w) + c3 (z - s) component-wise, left to right;  z+ = D(t);  w+ = (w + x) - z+;
          x, z+, w+ <- cclip(., 1)           (c1, c2, c3 = 1 - alpha, alpha, alpha reo lambda1 b: combined in double, rounded once)
    z0 = A^H y, w0 = 0.  x is clipped AFTER w is formed, and the clipped x is what the loop returns.

Everything takes ONE slice [H,W] (the glue functions any shape).  `dt` = np.complex128 (the oracle) or np.complex64: the float32
restatement -- every +, *, /, sqrt rounded to float32 in the kernels' order, no fused multiply-add -- which the glue kernels must equal bit
for bit, and whose distance from the oracle, with the same network in float32 on the CPU, sets the bars of the loops' GPU tests.
The network is `net(planes [n,H,W] real of the dtype's precision, i) -> [n,H,W]`; `cpu_net` builds one from a CPU `Denoiser` (the pattern
of tests/denoiser_oracle.py::cpu_denoiser)."""
import copy

import numpy as np

import complex_oracle as X

_real = X._real
_c = X._c
MODES = ('modulus', 'parts')


# ---- the glue, element by element ----------------------------------------------------------------------------------------------------

def den_in(v, mode, g=0.5, dt=np.complex128):
    """v [...] -> planes [1, ...] (modulus) or [2, ...] (parts)"""
    R = _real(dt)
    v = np.asarray(v).astype(dt)
    if mode == 'modulus':
        return X.cabs(v, dt)[None]
    g = R(g)
    return np.stack([(R(0.5) + (g * v.real).astype(R)).astype(R), (R(0.5) + (g * v.imag).astype(R)).astype(R)])


def den_out(q, v, mode, g=0.5, dt=np.complex128):
    """the network's planes q ([1, ...] or [2, ...]) and the value v it was asked about -> the denoised complex value"""
    R = _real(dt)
    q = np.asarray(q).astype(R)
    if mode == 'parts':
        g = R(g)
        return _c(((q[0] - R(0.5)).astype(R) / g).astype(R), ((q[1] - R(0.5)).astype(R) / g).astype(R), dt)
    v = np.asarray(v).astype(dt)
    m = X.cabs(v, dt)
    zero = m == 0
    with np.errstate(all='ignore'):
        f = (q[0] / np.where(zero, R(1), m)).astype(R)
        re, im = (f * v.real).astype(R), (f * v.imag).astype(R)
    return _c(np.where(zero, q[0], re), np.where(zero, R(0), im), dt)


def dual(x, z, w, dt=np.complex128):
    """-> (x, z, w): w+ = (w + x) - z from the unclipped values, then the three projections onto the unit disc"""
    x, z, w = (np.asarray(a).astype(dt) for a in (x, z, w))
    with np.errstate(all='ignore'):
        wn = ((w + x).astype(dt) - z).astype(dt)
        return X.cclip(x, 1, dt), X.cclip(z, 1, dt), X.cclip(wn, 1, dt)


def den_out_dual(q, v, x, w, mode, g=0.5, dt=np.complex128):
    return dual(x, den_out(q, v, mode, g, dt), w, dt)


def combine(z, x, w, s, alpha, lambda1, reo, b, dt=np.complex128):
    """S6:301 component-wise: ((c1 z) + (c2 (x + w))) + (c3 (z - s))"""
    R = _real(dt)
    c1, c2, c3 = R(1.0 - alpha), R(alpha), R(alpha * reo * lambda1 * b)
    z, x, w, s = (np.asarray(a).astype(dt) for a in (z, x, w, s))

    def part(zr, xr, wr, sr):
        with np.errstate(all='ignore'):
            a = (c1 * zr).astype(R)
            bb = (c2 * (xr + wr).astype(R)).astype(R)
            cc = (c3 * (zr - sr).astype(R)).astype(R)
            return ((a + bb).astype(R) + cc).astype(R)
    return _c(part(z.real, x.real, w.real, s.real), part(z.imag, x.imag, w.imag, s.imag), dt)


# ---- the network ---------------------------------------------------------------------------------------------------------------------

def cpu_net(name, state_dict, dt=np.complex128):
    """-> net(planes [n,H,W], i) -> [n,H,W]: `name` (denoisers.build) with `state_dict` on the CPU in float64 (dt complex128) or float32,
    every layer in PyTorch, through the project's own Denoiser"""
    import torch
    from pnp_admm_cnc_mri_amd import denoisers as D
    tdt = torch.float64 if dt == np.complex128 else torch.float32
    net, nlm, scheduled = D.build(name)
    assert not scheduled and D.family(name) in ('ffdnet', 'dncnn')
    net.load_state_dict(state_dict, strict=True)
    net = copy.deepcopy(net).eval().to(tdt)
    for m in [net] + list(net.modules()):
        if hasattr(m, 'backend'):
            m.backend = 'torch'
    den = D.Denoiser(name, net, nlm, backend='torch', channels_last=False, miopen_find=False)

    def call(planes, i):
        with torch.no_grad():
            x = torch.from_numpy(np.ascontiguousarray(planes, dtype=_real(dt)))[:, None]
            return np.stack([den(x[k:k + 1], i)[0, 0].numpy() for k in range(len(x))])      # plane by plane: PyTorch's float64 CPU convolution
                                                                                            # is several times slower per image on a batch
    return call


def denoise(v, net, i, mode, g=0.5, dt=np.complex128):
    """the complex denoiser step on one slice v [H,W]"""
    return den_out(net(den_in(v, mode, g, dt), i), v, mode, g, dt)


# ---- the loops -----------------------------------------------------------------------------------------------------------------------

def pnp(y, S, m, iter_num, kind, nets, mode='modulus', g=0.5, cg_iters=3, dt=np.complex128, state0=None, iter_start=0, keep=(), **par):
    """PNP_ADMM_L1_D (kind 'l1': par reo; nets (D,)) / PNP_ADMM_CNC_D and _DnCNN (kind 'cnc': par alpha, lambda1, reo, b; nets (D1, D2) or
    (D,)) with image='complex' on one slice.  -> (x, z, w) after iter_num iterations; keep: iteration counts k whose (x, z, w) are wanted
    too -> {k: (x, z, w)} as a fourth value"""
    aty, z, w = X.init_state(y, S, m, dt)
    if state0 is not None:
        z, w = np.asarray(state0[0]).astype(dt), np.asarray(state0[1]).astype(dt)
    x = z.copy()
    kept = {}
    for i in range(iter_start, iter_num):
        x = X.x_step(z, w, aty, S, m, par['reo'], cg_iters, dt)
        if kind == 'l1':
            v = (x + w).astype(dt)
            zn = denoise(v, nets[0], i, mode, g, dt)
        else:
            s = denoise(z, nets[0], i, mode, g, dt)
            t = combine(z, x, w, s, par['alpha'], par['lambda1'], par['reo'], par['b'], dt)
            zn = denoise(t, nets[-1], i, mode, g, dt)
        x, z, w = dual(x, zn, w, dt)
        if i + 1 in keep:
            kept[i + 1] = (x, z, w)
    return (x, z, w, kept) if keep else (x, z, w)


# ---- the problem of the tests --------------------------------------------------------------------------------------------------------

B, MID = 3, np.array([1, 0, 1], np.int32)


def case(H, W, C=2):
    """-> S [C,H,W], masks [2,H,W], y [B,C,H,W]: B = 3 slices of the phase phantom through the true maps, a bank of two masks with mask_id =
    [1, 0, 1]; maps and y rounded to complex64 once (complex128 holding complex64 values), as tests/test_gpu_complex.py does"""
    import multicoil_oracle as M
    C64, C128 = np.complex64, np.complex128
    S = M.coil_maps(C, H, W, H + C).astype(C64).astype(C128)
    masks = np.stack([M.mask(H + k, H, W) for k in range(2)])
    t = [X.truth(10 * H + b, H, W) for b in range(B)]
    y = np.stack([M.A(t[b], S, masks[MID[b]]) + M.noise(b, C, masks[MID[b]]) for b in range(B)]).astype(C64).astype(C128)
    return S, masks, y
