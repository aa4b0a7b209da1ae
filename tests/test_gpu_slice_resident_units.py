"""GPU checks of the resident UNITS of w in the slice-resident CNC kernel (kernels_slice256.hip, k_slice<2>; table: csrc/slice_layout.h,
sl_units_lds / sl_units_reg).  A unit (s, q) is the q-th 16-byte access of register set s: image rows 64 s .. 64 s + 63, columns
32 q .. 32 q + 31 of a slice.  Within a launch a resident unit's w is read from HBM once, lives in LDS or in registers for the launch's
iterations and returns to HBM when they are over.  A launch of ONE iteration makes no use of that (its prologue fills the units and its
end empties them), so K single-iteration launches are the reference for one launch of K: x, z and w must be equal bit for bit."""
import numpy as np
import pytest

from oracle import admm_oracle as O

pytestmark = pytest.mark.gpu

CNC = (0.45, 0.5, 0.05, 64)


@pytest.fixture(scope='module')
def P():
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib
    assert _lib.device_count() >= 1
    return P


def _problem(golden_inputs, B):
    masks = np.stack([golden_inputs['masks'][k] for k in ('Q_Random30', 'Q_Radial30', 'Q_Cartesian30')]).astype(np.uint8)
    mid = (np.arange(B) % 3).astype(np.int32)
    ys = np.stack([O.synthetic_problem(b % 8, masks[mid[b]])[1] for b in range(B)]).astype(np.complex64)
    return masks, mid, ys


@pytest.mark.parametrize('B,K', [(5, 7), (70, 4), (3, 1), (3, 2)])
def test_one_launch_of_k_iterations_equals_k_single_iteration_launches_in_every_unit(P, golden_inputs, monkeypatch, B, K):
    masks, mid, ys = _problem(golden_inputs, B)
    monkeypatch.setenv('PNP_SLICE', '1')
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.upload(ys, masks, mid)
        assert eng.path_name == 'slice'
        eng.init_state()
        eng.admm_cnc(K, *CNC)
        one = (eng.x(), *eng.get_state())
        eng.init_state()
        for _ in range(K):
            eng.admm_cnc(1, *CNC)
        many = (eng.x(), *eng.get_state())
    for name, a, b in zip('xzw', one, many):
        print(name, 'max |one - many| =', float(np.abs(a - b).max()))
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
    # w moved in each of the 32 units of every slice -- the resident ones (whichever the table names) and the ones that travel
    w = one[2].reshape(B, 4, 64, 8, 32)                     # [slice][set s][row in set][access q][column in access]
    moved = np.abs(w).max(axis=(2, 4))
    print('smallest max |w| of a unit:', float(moved.min()))
    assert (moved > 0).all(), np.argwhere(moved == 0)[:4]
