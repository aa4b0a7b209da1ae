"""GPU checks of what the four-pass transposition and the LDS-resident share of w add to the slice-resident CNC kernel
(kernels_slice256.hip, k_slice<2>): within a launch, set 0 of w is read from HBM once, lives in LDS for the launch's
iterations and returns to HBM when they are over.  A launch of ONE iteration makes no use of that (its prologue fills LDS
and its end empties it), so K single-iteration launches are the reference for one launch of K."""
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


@pytest.mark.parametrize('B,K', [(5, 7), (70, 4)])
def test_one_launch_of_k_iterations_equals_k_single_iteration_launches(P, golden_inputs, monkeypatch, B, K):
    """x, z and w, bit for bit: the resident rows of w (row pairs 0..31 of every slice) and the rows that travel through HBM
    every iteration see the same arithmetic in the same order."""
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
    assert one[2].any()                                   # w is not trivially zero
    for name, a, b in zip('xzw', one, many):
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
    # the resident rows are image rows 0..63: they moved like all others
    assert np.abs(one[2][:, :64]).max() > 0 and np.abs(one[2][:, 64:]).max() > 0


def test_l1_single_state_hand_over_after_a_cnc_run_agrees_with_the_two_launch_path(P, golden_inputs, monkeypatch):
    """CNC iterations (four-pass kernel, resident w) followed by ADMM_L1 in its single-state form (two-pass kernel) on the same
    state, against the two-launch fused path running the same calls: both paths share the arithmetic cores, not the data flow
    (values in [0, 1]; the flows differ by ~3e-7 per pixel and iteration: the 2e-5 of test_slice_path_at_every_batch_shape)."""
    B = 6
    masks, mid, ys = _problem(golden_inputs, B)
    res = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('PNP_SLICE', mode)
        with P.Engine(256, 256, Bmax=B) as eng:
            eng.upload(ys, masks, mid)
            assert eng.path_name == ('slice' if mode == '1' else 'fused')
            eng.init_state()
            eng.admm_cnc(4, *CNC)
            eng.admm_l1(3, 0.1, 0.015)
            xl = eng.x()
            zl, wl = eng.get_state()
            eng.admm_cnc(2, *CNC)                          # and back: the L1 launch's state feeds the resident form again
            res[mode] = (xl, zl, wl, eng.x(), *eng.get_state())
    for i, (a, b) in enumerate(zip(res['1'], res['0'])):
        d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
        assert d <= 2e-5, (i, d)
