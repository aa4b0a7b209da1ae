"""tests/denoiser_oracle.py itself, on a machine without a GPU: the bars it hands tests/test_gpu_denoiser_shapes.py are sane, its reference is
not a restatement of the code under test, and its inputs drive the networks through both sides of their ReLUs.

Measured on the CPU (seed 11; shape C of FFDNet / FDnCNN: seeds 19 / 17): the float32 forward is 3.5e-6 of the slice's peak from the float64
one for FDnCNN at 3 x 41 x 58, the worst; FFDNet 2.4e-6, DRUNet 1.2e-6 (7 x 5), DnCNN 4.4e-7 and 6.0e-7, IRCNN 3.0e-7; the smallest is
IRCNN's 5.4e-8 at 7 x 5.  Outputs peak between 0.068 (FFDNet at 3 x 7 x 5) and 8.9 (DRUNet at 264 x 250)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import denoiser_oracle as O
from pnp_admm_cnc_mri_amd import denoisers as D

CASES = O.cases()
_ID = lambda c: '%s-%dx%dx%d-i%d%s' % (c[0], *c[1], c[2], '-x8' if c[3] else '')


@pytest.mark.parametrize('case', CASES, ids=_ID)
def test_the_bars_are_sane(case):
    """every slice of every case: the output peaks at 0.05 or more and the float32 CPU forward lies in (0, 5e-6] of that peak from the float64
    one -- so no bar exceeds 2e-5 of a slice's peak.  A case outside these limits is a mis-designed input (denoiser_oracle.SEEDS), not a
    reason for a wider bar."""
    name, shape, i, x8 = case
    ref = O.reference(name, shape, i, x8)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (shape[0], 1, shape[1], shape[2]) and bool(torch.isfinite(ref).all())
    peak = ref.abs().reshape(shape[0], -1).amax(1).numpy()
    d = O.d32(name, shape, i, x8)
    print('BAR %s: peak %s  d32 %s' % (_ID(case), np.array2string(peak, precision=3), np.array2string(d, precision=3)))
    assert (peak >= 0.05).all(), peak
    assert ((d > 0) & (d <= 5e-6)).all(), d
    assert np.array_equal(O.bar(name, shape, i, x8), 4.0 * d) and O.FREEDOM == 4.0
    assert (O.bar(name, shape, i, x8) <= 2e-5).all()


def test_the_cases_are_the_ones_the_gpu_tests_name():
    assert O.NETS == ('ffdnet_gray', 'dncnn_15', 'dncnn_gray_blind', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray')
    assert (O.A, O.B, O.C, O.E) == ((3, 41, 58), (3, 58, 41), (1, 7, 5), (1, 264, 250))
    assert O.shape_d('ffdnet_gray') == (12, 136, 152) and all(O.shape_d(n) == (3, 136, 152) for n in O.NETS[1:])
    assert [n for n in O.NETS if 'E' in O.shapes(n)] == ['drunet_gray']
    assert len(CASES) == 6 * 4 + 1 + 8 + 4 + 1 and len(set(CASES)) == len(CASES)
    assert O.SCHEDULE[:3] == (30 / 255, 20 / 255, 10 / 255) and all(O.SCHEDULE[i] == O.SCHEDULE[i % 3] for i in range(8))
    # what the shapes are chosen to reach
    assert O.body_size('ffdnet_gray', O.A) == (21, 29) and O.body_size('ffdnet_gray', O.C) == (4, 3)
    assert O.body_size('drunet_gray', O.A) == (48, 64) and O.body_size('drunet_gray', O.C) == (16, 16)
    assert O.E[1] * O.E[2] > 256 ** 2 and (D._corner_span(264, 32), D._corner_span(250, 32)) == (160, 128)


def test_dist_is_per_slice_and_per_element():
    ref = torch.zeros(2, 1, 4, 5, dtype=torch.float64)
    ref[0, 0, 1, 2], ref[1, 0, 3, 4] = 2.0, -4.0
    got = ref.clone().float()
    got[1, 0, 0, 0] += 1e-3                                        # ONE wrong pixel
    assert np.allclose(O.dist(got, ref), [0.0, 2.5e-4], rtol=1e-6, atol=0)
    assert O.where_worst(got, ref) == (1, 0, 0)


def test_the_input_is_keyed_by_name_and_shape():
    _, _, xa, _ = O.case('dncnn_15', O.A)
    _, _, xa2, _ = O.case('dncnn_15', O.A)
    _, _, xb, _ = O.case('dncnn_15', O.B)
    _, _, xi, _ = O.case('ircnn_gray', O.A)
    assert torch.equal(xa, xa2) and xa.dtype == torch.float32 and float(xa.min()) >= 0 and float(xa.max()) < 1
    assert not torch.equal(xa, xb.transpose(2, 3)) and not torch.equal(xa, xi)
    assert O.reference('dncnn_15', O.A) is O.reference('dncnn_15', list(O.A), 0, False)          # cached per process


# ----------------------------------------------------------------------------------------------
# The reference is not a restatement of the code under test: the same forwards from bare torch.nn.functional calls in float64 -- conv2d,
# relu, pixel_unshuffle / pixel_shuffle, replicate pad, crop -- with nothing of denoisers.py but the seeded weights.  The U-Net's 2 x 2
# stride-2 convolution is written as pixel_unshuffle + 1 x 1 convolution and its transposed one as 1 x 1 convolution + pixel_shuffle.
# ----------------------------------------------------------------------------------------------
def _weights64(name, shape):
    net, _, _ = D.build(name)
    return {k: v.double() for k, v in D.seeded_state_dict(net, O.seed_of(name, shape)).items()}


def _stack64(sd, h, nb, dilations=None):
    for k in range(nb):
        d = 1 if dilations is None else dilations[k]
        h = F.conv2d(h, sd['model.%d.weight' % (2 * k)], sd['model.%d.bias' % (2 * k)], padding=d, dilation=d)
        if k != nb - 1:
            h = F.relu(h)
    return h


@pytest.mark.parametrize('name,nb,dil', [('dncnn_15', 17, None), ('dncnn_gray_blind', 20, None), ('ircnn_gray', 7, [1, 2, 3, 4, 3, 2, 1])])
def test_reference_equals_a_bare_rebuild_of_a_residual_stack(name, nb, dil):
    sd = _weights64(name, O.A)
    x = O.case(name, O.A)[2].double()
    want = x - _stack64(sd, x, nb, dil)
    assert float(O.dist(O.reference(name, O.A), want).max()) <= 1e-12


@pytest.mark.parametrize('shape', [O.A, O.C])
def test_reference_equals_a_bare_rebuild_of_ffdnet(shape):
    """odd H (and, at 7 x 5, odd W): replicate pad to even, unshuffle, the constant noise-level map 15 / 255, 15 layers, shuffle, crop"""
    sd = _weights64('ffdnet_gray', shape)
    x = O.case('ffdnet_gray', shape)[2].double()
    _, H, W = shape
    h = F.pad(x, (0, W % 2, 0, H % 2), mode='replicate')
    h = F.pixel_unshuffle(h, 2)
    h = torch.cat((h, torch.full_like(h[:, :1], 15.0 / 255)), 1)
    want = F.pixel_shuffle(_stack64(sd, h, 15), 2)[..., :H, :W]
    assert float(O.dist(O.reference('ffdnet_gray', shape), want).max()) <= 1e-12


def test_reference_equals_a_bare_rebuild_of_fdncnn():
    sd = _weights64('fdncnn_gray', O.B)
    x = O.case('fdncnn_gray', O.B)[2].double()
    nm = torch.from_numpy(np.abs(O.noises(58, 41)).astype(np.float32) / np.float32(255.0)).double()      # S6:26-29: a float32 map
    want = _stack64(sd, torch.cat((x, nm.expand(3, 1, 58, 41)), 1), 20)
    assert float(O.dist(O.reference('fdncnn_gray', O.B), want).max()) <= 1e-12


def _unet64(sd, x0):
    def blocks(h, pre, first):
        for k in range(first, first + 4):
            h = h + F.conv2d(F.relu(F.conv2d(h, sd['%s.%d.res.0.weight' % (pre, k)], padding=1)), sd['%s.%d.res.2.weight' % (pre, k)], padding=1)
        return h

    def down(h, pre):
        w = sd[pre + '.4.weight']                                   # [2C][C][2][2] -> 1 x 1 over the unshuffled channels c * 4 + i * 2 + j
        return F.conv2d(F.pixel_unshuffle(h, 2), w.reshape(w.shape[0], w.shape[1] * 4, 1, 1))

    def up(h, pre):
        w = sd[pre + '.0.weight']                                   # [C][C / 2][2][2] -> 1 x 1 to the channels o * 4 + i * 2 + j, then shuffle
        return F.pixel_shuffle(F.conv2d(h, w.permute(1, 2, 3, 0).reshape(w.shape[1] * 4, w.shape[0], 1, 1)), 2)
    x1 = F.conv2d(x0, sd['m_head.weight'], padding=1)
    x2 = down(blocks(x1, 'm_down1', 0), 'm_down1')
    x3 = down(blocks(x2, 'm_down2', 0), 'm_down2')
    x4 = down(blocks(x3, 'm_down3', 0), 'm_down3')
    h = blocks(x4, 'm_body', 0)
    h = blocks(up(h + x4, 'm_up3'), 'm_up3', 1)
    h = blocks(up(h + x3, 'm_up2'), 'm_up2', 1)
    h = blocks(up(h + x2, 'm_up1'), 'm_up1', 1)
    return F.conv2d(h + x1, sd['m_tail.weight'], padding=1)


@pytest.mark.parametrize('i', [0, 1])
def test_reference_equals_a_bare_rebuild_of_drunet_at_41_by_58(i):
    """the noise-level map of iteration i, the replicate pad to 48 x 64, the U-Net, the crop"""
    sd = _weights64('drunet_gray', O.A)
    x = O.case('drunet_gray', O.A)[2].double()
    sigma = float(np.float32(O.SIGMAS[i]))                          # the schedule is a float32 tensor
    h = torch.cat((x, torch.full_like(x, sigma)), 1)
    h = F.pad(h, (0, 64 - 58, 0, 48 - 41), mode='replicate')
    want = _unet64(sd, h)[..., :41, :58]
    assert float(O.dist(O.reference('drunet_gray', O.A, i), want).max()) <= 1e-12


def test_x8_reference_is_the_plain_forward_of_the_transformed_input():
    """mode 1 of the x8 cycle is a transposition ... of a network that is not symmetric: the view's forward differs from the plain one,
    and equals the bare rebuild on the transformed input, transformed back"""
    sd = _weights64('ircnn_gray', O.A)
    x = O.case('ircnn_gray', O.A)[2].double()
    dil = [1, 2, 3, 4, 3, 2, 1]
    f = lambda t: t - _stack64(sd, t, 7, dil)
    want = {1: f(x.rot90(1, (2, 3)).flip(2)).flip(2).rot90(-1, (2, 3)), 2: f(x.flip(2)).flip(2),
            3: f(x.rot90(3, (2, 3))).rot90(-3, (2, 3)), 5: f(x.rot90(1, (2, 3))).rot90(-1, (2, 3))}
    for i, w in want.items():
        assert float(O.dist(O.reference('ircnn_gray', O.A, i, True), w).max()) <= 1e-12, i
        assert float(O.dist(O.reference('ircnn_gray', O.A, i, True), O.reference('ircnn_gray', O.A)).max()) > 1e-3, i


# ----------------------------------------------------------------------------------------------
# The inputs are non-degenerate: a network whose ReLUs are all open (or all shut) is a linear map (or a constant), and a kernel that
# dropped its ReLU would pass.
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['A', 'C', 'D'])
@pytest.mark.parametrize('name', O.NETS)
def test_the_inputs_are_non_degenerate(name, tag):
    """after the first and the last body layer -- the first and last 64 -> 64 convolution in front of a ReLU; DRUNet: the first
    convolution of its first and last residual block -- the share of positive pre-activations lies in (0.1, 0.9)"""
    shape = O.shapes(name)[tag]
    den, x = O.cpu_denoiser(name, shape, torch.float64)
    net = den.model
    if isinstance(net, D.UNetRes):
        first, last = net.m_down1[0].res[0], net.m_up1[4].res[0]
    else:
        convs = [m for m in net.model if isinstance(m, torch.nn.Conv2d)]
        first, last = convs[1], convs[-2]
    assert first.in_channels == first.out_channels == 64 and last.in_channels == last.out_channels == 64 and first is not last
    share = {}
    hooks = [m.register_forward_hook(lambda mod, inp, out, k=k: share.__setitem__(k, float((out > 0).double().mean())))
             for k, m in (('first', first), ('last', last))]
    try:
        den(x, 0)
    finally:
        for h in hooks:
            h.remove()
    assert sorted(share) == ['first', 'last']
    assert all(0.1 < s < 0.9 for s in share.values()), share
