"""NumPy oracle of the ESPIRiT coil map estimation -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the text of include/pnp_mri.h ("ESPIRiT coil sensitivity maps"), written from that text and not from the kernels: the
calibration block in ascending frequency, the Gram matrix of its k x k patches, the signal space by numpy.linalg.eigh, the kernel
autocorrelations w, the per-pixel operator G(q), the power iteration from the windowed low-resolution images, the phase rule and the
support.  Everything takes ONE slice: y [C,H,W] complex (un-shifted, DC at [0, 0]), mask [H,W].  `dt` = np.complex128 (the oracle) or
np.complex64: the float32 restatement -- the Gram matrix and the host stage stay in double, as in the library; w, the phasors and every
intermediate of the per-pixel stage are rounded to complex64 / float32 -- whose distance from the float64 form is the yardstick of the
float GPU tests (as tests/coilmaps_oracle.py does).
"""
import numpy as np

import coilmaps_oracle as CM
import coilmix_oracle as CO


def block(y, ncal):
    """K [C,ncal,ncal]: the calibration region in ascending signed frequency on both axes (a roll by ncal // 2)"""
    C, H, W = y.shape
    K = np.asarray(y)[np.ix_(np.arange(C), CO.cal_lines(ncal, H), CO.cal_lines(ncal, W))]
    return np.roll(K, (ncal // 2, ncal // 2), axis=(1, 2))


def calib_rows(K, k):
    """A as [P,P,n]: row (i, j) holds K[c, i + a, j + b] at column (c k + a) k + b"""
    C, ncal, _ = K.shape
    P = ncal - k + 1
    win = np.lib.stride_tricks.sliding_window_view(K, (k, k), axis=(1, 2))          # [C,P,P,k,k]
    return np.ascontiguousarray(win.transpose(1, 2, 0, 3, 4)).reshape(P, P, C * k * k)


def gram(y, mask, ncal, k, reverse=False):
    """A^H A [n,n] in double, the position rows accumulated in ascending (or, reverse, descending) order.  ValueError on a hole."""
    hole = CM.first_hole(mask, ncal)
    if hole is not None:
        raise ValueError('calibration point (%d, %d) is not sampled' % hole)
    A = calib_rows(block(np.asarray(y).astype(np.complex128), ncal), k)
    G = np.zeros((A.shape[2],) * 2, np.complex128)
    for i in (range(A.shape[0] - 1, -1, -1) if reverse else range(A.shape[0])):
        Ai = A[i, ::-1] if reverse else A[i]
        G = G + Ai.conj().T @ Ai
    return G


def signal_space(G, sigma):
    """-> (P = V V^H over the eigenvectors with s_j >= sigma s_max, symmetrised; rank; s descending)"""
    e, V = np.linalg.eigh(0.5 * (G + G.conj().T))
    s = np.sqrt(np.maximum(e, 0.0))
    keep = s >= sigma * s.max()
    Vk = V[:, keep]
    P = Vk @ Vk.conj().T
    return 0.5 * (P + P.conj().T), int(keep.sum()), s[::-1].copy()


def kernels(P, C, k):
    """w [C,C,2k-1,2k-1]: w_cc'(d) = (1 / k^2) sum_{a - a' = d} conj(P)[(c, a), (c', a')], entry (dy + k - 1, dx + k - 1); the upper
    triangle from the sum, the lower as w_c'c(-d) = conj(w_cc'(d))"""
    Pc = np.conj(P).reshape(C, k, k, C, k, k)
    D = 2 * k - 1
    w = np.zeros((C, C, D, D), np.complex128)
    for ay in range(k):
        for ax in range(k):
            for by in range(k):
                for bx in range(k):
                    w[:, :, ay - by + k - 1, ax - bx + k - 1] += Pc[:, ay, ax, :, by, bx]
    w /= k * k
    for c in range(C):
        for c2 in range(c + 1, C):
            w[c2, c] = np.conj(w[c, c2][::-1, ::-1])
    return w


def phasors(n, k, dt=np.complex128):
    """E_n(q, d) = exp(+2 pi i ((q d) mod n) / n), [n,2k-1] for d = -(k-1) .. k-1, formed in double and rounded once"""
    t = (np.arange(n)[:, None] * np.arange(-(k - 1), k)[None, :]) % n
    return np.exp(2j * np.pi * t / n).astype(dt)


def operator(w, H, W, dt=np.complex128):
    """G [C,C,H,W]: G_cc'(q) = sum_dy E_H(q_y, dy) [sum_dx w_cc'(dy, dx) E_W(q_x, dx)], dx then dy ascending, every partial sum rounded; the
    upper triangle computed, the lower its conjugate, the diagonal real"""
    C, _, D, _ = w.shape
    k = (D + 1) // 2
    w = np.asarray(w).astype(dt)
    EH, EW = phasors(H, k, dt), phasors(W, k, dt)
    if dt == np.complex128:                                      # the oracle itself: the order of the sums is not its business
        G = np.matmul(EH[None, None], np.matmul(w, EW.T[None, None]))
    else:
        G = np.zeros((C, C, H, W), dt)
        for dy in range(D):
            inner = np.zeros((C, C, W), dt)
            for dx in range(D):
                inner = (inner + (w[:, :, dy, dx, None] * EW[None, None, :, dx]).astype(dt)).astype(dt)
            G = (G + (EH[None, None, :, dy, None] * inner[:, :, None, :]).astype(dt)).astype(dt)
    for c in range(C):
        G[c, c] = G[c, c].real
        for c2 in range(c):
            G[c, c2] = np.conj(G[c2, c])
    return G


def eigmaps(I, w, n, dt=np.complex128, G=None):
    """-> (v [C,H,W] unit vectors with v^H I >= 0, lambda [H,W]): n power steps on G(q) from v = I / ||I||"""
    R = CM._real(dt)
    I = np.asarray(I).astype(dt)
    C, H, W = I.shape
    if G is None:
        G = operator(w, H, W, dt)
    nrm = CM._norm(I, R)
    e0 = np.zeros_like(I)
    e0[0] = 1
    v = np.where(nrm > 0, CM._div(I, nrm), e0).astype(dt)
    lam = np.zeros((H, W), R)
    for _ in range(n):
        u = np.zeros_like(I)
        for c2 in range(C):
            u = (u + (G[:, c2] * v[c2][None]).astype(dt)).astype(dt)
        lam = CM._norm(u, R)
        v = np.where(lam > 0, CM._div(u, lam), v).astype(dt)
    g = CM._dotc(v, I, dt)
    m = np.abs(g).astype(R)
    v = np.where(m > 0, (v * CM._div(g, m)[None]).astype(dt), v).astype(dt)
    return v, lam


def support(lam, inorm, crop, thresh):
    R = lam.dtype.type
    return (lam >= R(crop)) & (inorm >= R(thresh) * inorm.max())


def estimate(y, mask, ncal=24, k=4, n=4, sigma=0.02, crop=0.9, thresh=0.05, dt=np.complex128, full=False, reverse=False):
    """-> maps [C,H,W] (zero outside the support); full=True: a dict with maps, lam, sup, v, I, inorm, w, rank, sing, gram"""
    C = y.shape[0]
    Gm = gram(y, mask, ncal, k, reverse)
    P, rank, sing = signal_space(Gm, sigma)
    w = kernels(P, C, k)
    I = CM.lowres(y, mask, ncal, dt)
    v, lam = eigmaps(I, w, n, dt)
    inorm = CM._norm(I, CM._real(dt))
    sup = support(lam, inorm, crop, thresh)
    S = np.where(sup[None], v, 0).astype(dt)
    return dict(maps=S, lam=lam, sup=sup, v=v, I=I, inorm=inorm, w=w, rank=rank, sing=sing, gram=Gm) if full else S
