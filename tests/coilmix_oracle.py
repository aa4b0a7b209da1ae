"""NumPy oracle of the coil mixing (prewhitening, coil compression) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A restatement of the text of include/pnp_mri.h ("coil mixing"), written from that text and not from the kernels: the calibration region,
the Gram matrix, out = M in with the coils accumulated in order, M_w = L^-1, M_c = the conjugated leading eigenvectors with the phase
rule.  `dt` = np.complex128 (the oracle) or np.complex64 (the float32 restatement: every partial sum rounded; its distance from the
float64 form is the yardstick of the float GPU tests, as in tests/multicoil_oracle.py).
"""
import numpy as np

import multicoil_oracle as M


def cal_lines(ncal, n):
    """the ncal lines of the calibration region along an axis of length n, in order: 0 .. ceil(ncal/2) - 1, then n - floor(ncal/2) .. n - 1"""
    return np.array(list(range((ncal + 1) // 2)) + list(range(n - ncal // 2, n)), np.int64)


def cal_region(ncal, H, W):
    """boolean [H,W]: the calibration region"""
    r = np.zeros((H, W), bool)
    r[np.ix_(cal_lines(ncal, H), cal_lines(ncal, W))] = True
    return r


def gram(y, mask, ncal):
    """R[i,j] = sum_{p in calibration} mask(p) y[i,p] conj(y[j,p]), y [C,H,W], float64.  -> (R [C,C], sum |y_i| |y_j| over the same points)"""
    rows, cols = cal_lines(ncal, y.shape[1]), cal_lines(ncal, y.shape[2])
    v = (np.asarray(y, np.complex128)[:, rows][:, :, cols] * (np.asarray(mask)[rows][:, cols] != 0)).reshape(y.shape[0], -1)
    return v @ v.conj().T, np.abs(v) @ np.abs(v).T


def mix(k, Mx, dt=np.complex128):
    """out[j] = sum_c Mx[j,c] k[c], k [C_in,...], the coils in order and every partial sum rounded to dt"""
    k, Mx = np.asarray(k).astype(dt), np.asarray(Mx).astype(dt)
    out = np.zeros((Mx.shape[0],) + k.shape[1:], dt)
    for c in range(k.shape[0]):
        out = (out + (Mx[:, c].reshape((-1,) + (1,) * (k.ndim - 1)) * k[c]).astype(dt)).astype(dt)
    return out


def mix_abs(k, Mx):
    """sum_c |Mx[j,c]| |k[c]|: the scale of the element-wise rounding bound"""
    return np.tensordot(np.abs(np.asarray(Mx, np.complex128)), np.abs(np.asarray(k, np.complex128)), axes=(1, 0))


def whitening_matrix(psi):
    return np.linalg.inv(np.linalg.cholesky(np.asarray(psi, np.complex128)))


def compression(R, n):
    """-> (M_c [n,C], eigenvalues descending [C]) by numpy.linalg.eigh, with the phase rule: each eigenvector's entry of largest modulus
    (the first on a tie) real and positive"""
    w, v = np.linalg.eigh(np.asarray(R, np.complex128))
    w, v = w[::-1], v[:, ::-1]
    for j in range(v.shape[1]):
        at = int(np.argmax(np.abs(v[:, j])))
        v[:, j] *= np.conj(v[at, j]) / abs(v[at, j])
    return v[:, :n].conj().T.copy(), w


def projector(Mc):
    return Mc.conj().T @ Mc


def unitary(C, seed):
    rng = np.random.default_rng(6400 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C)))
    return q


def hpd(C, seed, floor=0.5):
    """a seeded Hermitian positive-definite matrix of order C (a noise covariance with correlated channels)"""
    rng = np.random.default_rng(8800 + seed)
    b = rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C))
    a = b @ b.conj().T / C + floor * np.eye(C)
    return (a + a.conj().T) / 2


def rank4_maps(Cn, H, W, seed=0):
    """Cn channels that span the 4-dimensional space of the oracle's 4 smooth maps: S = A S4 with a seeded Cn x 4 matrix A whose columns
    have norms 1, 0.8, 0.75, 0.5 (so that the four Gram eigenvalues are well apart), normalised to sum_c |S_c|^2 = 1"""
    rng = np.random.default_rng(2900 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((Cn, 4)) + 1j * rng.standard_normal((Cn, 4)))
    S = np.tensordot(q * np.array([1.0, 0.8, 0.75, 0.5]), M.coil_maps(4, H, W, seed), axes=(1, 0))
    return S / np.sqrt((np.abs(S) ** 2).sum(0, keepdims=True))


def correlated_noise(seed, psi, m, std=1.0):
    """complex Gaussian noise on the sampled entries with channel covariance 2 std^2 psi, [C,H,W]"""
    L = np.linalg.cholesky(np.asarray(psi, np.complex128))
    return np.tensordot(L, M.noise(seed, len(L), m, std), axes=(1, 0))
