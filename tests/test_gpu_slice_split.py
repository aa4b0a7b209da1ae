"""GPU checks of the slice-resident CNC kernel (kernels_slice256.hip, k_slice<2>) with its transient LDS halved: the transform groups
exchange in two planes, the transpositions cross in eight halves, and 16 units of w stay on the compute unit (csrc/slice_layout.h).
Against the float64 oracle's trace (x, z and w, every iteration count that takes another path: 1 = prologue, last iteration and flush in
one; 2; 5), a batch larger than the chip (a compute unit's second workgroup fills the LDS the first one left), and a launch cut in two."""
import ctypes as C

import numpy as np
import pytest

from oracle import admm_oracle as O

pytestmark = pytest.mark.gpu

CNC = (0.45, 0.5, 0.05, 64)
# values in [0, 1]; float32 kernel against the float64 oracle, per pixel: the bar of test_gpu_slice_resident_w.py
BAR = 2e-5


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


@pytest.fixture(scope='module')
def bank(golden_inputs):
    """the three reference masks and the 24 (phantom, mask) problems every batch below is made of"""
    masks = np.stack([golden_inputs['masks'][k] for k in ('Q_Random30', 'Q_Radial30', 'Q_Cartesian30')]).astype(np.uint8)
    ys = {(p, m): O.synthetic_problem(p, masks[m])[1].astype(np.complex64) for p in range(8) for m in range(3)}
    return masks, ys


def _batch(bank, slices):
    masks, ys = bank
    mid = (np.asarray(slices) % 3).astype(np.int32)
    return masks, mid, np.stack([ys[(int(b) % 8, int(b) % 3)] for b in slices])


@pytest.fixture(scope='module')
def oracle_trace(bank):
    masks, mid, ys = _batch(bank, range(3))
    return [O.admm_cnc(ys[b].astype(np.complex128), masks[mid[b]], 5, *CNC, trace=(1, 2, 5))[1] for b in range(3)]


@pytest.mark.parametrize('K', [1, 2, 5])
def test_three_masks_against_the_oracle_trace(P, bank, oracle_trace, monkeypatch, K):
    """covers the last iteration's x store in two halves, the packed column in wave 0's borrowed region and every unit of w"""
    masks, mid, ys = _batch(bank, range(3))
    monkeypatch.setenv('PNP_SLICE', '1')
    with P.Engine(256, 256, Bmax=3) as eng:
        eng.upload(ys, masks, mid)
        assert eng.path_name == 'slice'
        eng.init_state()
        eng.admm_cnc(K, *CNC)
        got = (eng.x(), *eng.get_state())
    for b in range(3):
        ref = oracle_trace[b][K]
        errs = [float(np.abs(got[i][b].astype(np.float64) - ref[i]).max()) for i in range(3)]
        print('K', K, 'slice', b, 'max |x, z, w - oracle|:', errs)
        assert max(errs) <= BAR, (b, errs)


def test_second_workgroup_of_a_compute_unit_equals_a_small_batch(P, bank, monkeypatch):
    """B = compute units + 2: the last workgroups start on a compute unit whose LDS another slice just left (flush, then the next
    prologue over the same words).  Slice 0 and the last three slices, bit for bit, against the same slices solved three at a time."""
    from pnp_admm_cnc_mri_amd import _lib
    cus = C.c_int(0)
    _lib.check(_lib.lib().pnp_device_info(0, None, C.byref(cus), None, 0, None, 0))
    B = cus.value + 2
    monkeypatch.setenv('PNP_SLICE', '1')

    def solve(slices):
        masks, mid, ys = _batch(bank, slices)
        with P.Engine(256, 256, Bmax=len(slices)) as eng:
            eng.upload(ys, masks, mid)
            assert eng.path_name == 'slice'
            eng.init_state()
            eng.admm_cnc(2, *CNC)
            return (eng.x(), *eng.get_state())

    big = solve(range(B))
    for slices in ([0, 1, 2], [B - 3, B - 2, B - 1]):
        small = solve(slices)
        for i, b in enumerate(slices):
            if b in (1, 2):
                continue
            for name, a, s in zip('xzw', big, small):
                assert np.array_equal(a[b], s[i]), (b, name, float(np.abs(a[b] - s[i]).max()))


def test_a_launch_of_five_equals_launches_of_two_and_three(P, bank, monkeypatch):
    masks, mid, ys = _batch(bank, range(3))
    monkeypatch.setenv('PNP_SLICE', '1')
    with P.Engine(256, 256, Bmax=3) as eng:
        eng.upload(ys, masks, mid)
        assert eng.path_name == 'slice'
        eng.init_state()
        eng.admm_cnc(5, *CNC)
        one = (eng.x(), *eng.get_state())
        eng.init_state()
        eng.admm_cnc(2, *CNC)
        eng.admm_cnc(3, *CNC)
        two = (eng.x(), *eng.get_state())
    assert one[2].any()
    for name, a, b in zip('xzw', one, two):
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
