"""Shared by the any-size FFT sweeps (test_anysize_host.py on the CPU, test_gpu_anysize_sweep.py on the GPU): the lengths, the
pairing of column and row lengths, the host rules of csrc/anysize_plan.h and kernels_anysize.hip restated (kind, m, lines per
workgroup), the two error measures and the recorded 2-D figures of the emulation (tests/golden/anysize_sweep_bounds.json)."""
import json
import os

import numpy as np

MIN_N, MAX_N = 128, 1024
LENGTHS = range(MIN_N, MAX_N + 1)                    # 897 lengths
BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'anysize_sweep_bounds.json')


def pair(H):
    """W of the one shape in which H is the column length: a bijection of [128, 1024] (389 is coprime to 897 = 3 * 13 * 23), so
    every length is a column length once and a row length once.  256 -> 796 and 512 -> 813: no shape takes the fixed-size kernels."""
    return MIN_N + ((H - MIN_N) * 389 + 211) % 897


def shape_seed(H, W):
    return H * 4096 + W


def primes(n):
    out, q = [], 2
    while n > 1:
        while n % q == 0:
            out.append(q)
            n //= q
        q += 1
    return out


def smooth7(n):
    return all(q <= 7 for q in primes(n))


def stockham_length(n):
    """m of anysize_plan.h: n itself if 7-smooth, else the power of two >= 2n - 1 of Bluestein."""
    if smooth7(n):
        return n
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def radices(m):
    """factor() of anysize_plan.h: 4s, at most one 2, then 3s, 5s, 7s."""
    out = []
    while m % 4 == 0:
        out.append(4)
        m //= 4
    if m % 2 == 0:
        out.append(2)
        m //= 2
    for p in (3, 5, 7):
        while m % p == 0:
            out.append(p)
            m //= p
    assert m == 1
    return out


def lines_per_wg(n, f64, across=1 << 30):
    """lines_per_wg of kernels_anysize.hip: about 40 KiB of LDS per workgroup, two buffers of pitch m + 1, 1 .. 16 lines."""
    per_line = 2 * (16 if f64 else 8) * (stockham_length(n) + 1)
    return max(1, min(16, 40 * 1024 // per_line, across))


def combo(n, f64, across=1 << 30):
    """What shapes a kernel along one axis: (kind, m, G)."""
    return ('stockham' if smooth7(n) else 'bluestein', stockham_length(n), lines_per_wg(n, f64, across))


def coil_lines_per_wg(n, f64):
    """coil_axis of kernels_anysize.hip: the coil rows hold a third LDS array of n values per line beside the two buffers of pitch m + 1,
    counted against the same 40 KiB; never more lines than the plain rows take."""
    per_line = (16 if f64 else 8) * (2 * (stockham_length(n) + 1) + n)
    return max(1, min(40 * 1024 // per_line, lines_per_wg(n, f64)))


def coil_lds_bytes(n, f64):
    """coil_lds of kernels_anysize.hip: the dynamic LDS of one coil-row workgroup."""
    return (16 if f64 else 8) * coil_lines_per_wg(n, f64) * (2 * (stockham_length(n) + 1) + n)


def coil_row_combo(n, f64):
    """What shapes a coil row kernel along W: (kind, m if Bluestein else None, G)."""
    kind = 'stockham' if smooth7(n) else 'bluestein'
    return kind, stockham_length(n) if kind == 'bluestein' else None, coil_lines_per_wg(n, f64)


# the first row length of every (kind, m, G) of the coil rows, worked out from coil_axis()'s rule; test_multicoil_host.py holds the
# restatement above to it, test_gpu_multicoil_edges.py runs each length once
COIL_ROW_FIRSTS = {False: (128, 129, 135, 144, 160, 175, 189, 216, 245, 255, 257, 288, 343, 432, 511, 513, 576, 864),
                   True: (128, 129, 144, 175, 216, 255, 257, 288, 432, 513)}


def shape_combos(H, W, f64):
    """(rows' combination, columns' combination) of a context, as anysize_create sets them."""
    return combo(W, f64), combo(H, f64, W)


# the column lengths of the 2-D emulation (test_anysize_host.py): the whole sweep in two dimensions costs minutes of CPU, this
# fixed subset a few seconds -- every ninth length, and the lengths at which the 1-D sweep measured its worst values or whose plan
# is a single radix
GRID_LENGTHS = tuple(sorted(set(range(MIN_N, MAX_N + 1, 9)) | {243, 343, 625, 729, 877, 896, 945, 1022, 1024}))


def errors(got, ref):
    """(relative L2, max |err| / rms(ref), index of the worst bin) of one line or slice, in complex128."""
    e = np.asarray(got, np.complex128) - np.asarray(ref, np.complex128)
    e2 = e.real ** 2 + e.imag ** 2
    r2 = float(np.sum(ref.real.astype(np.float64) ** 2 + ref.imag.astype(np.float64) ** 2))
    worst = np.unravel_index(int(np.argmax(e2)), e2.shape)
    return float(np.sqrt(np.sum(e2) / r2)), float(np.sqrt(e2[worst] / (r2 / e2.size))), tuple(int(i) for i in worst)


def load_bounds():
    with open(BOUNDS) as f:
        return json.load(f)
