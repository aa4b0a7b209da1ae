"""hip_layers' classification of the denoisers' layers (stack_plan / unet_plan) without a GPU and without loading the library: for every
family and every HIP backend the sequence of entry points, with dilation and fmt where a call has them, written down here from the
architectures and the rules (not printed from the function) -- and the coverage answers, which are read from the same plans."""
import pytest
import torch
import torch.nn as nn

from pnp_admm_cnc_mri_amd import denoisers as D
from pnp_admm_cnc_mri_amd import hip_layers as HL

P = 'pnp_conv3x3_'
HEAD, HEAD_H = P + 'head_nhwc', P + 'head_nhwc_f16'
C64, C64_X3, WIDE_X3, FMT, HALF = P + 'c64_nhwc', P + 'c64_nhwc_f16x3', P + 'nhwc_f16x3', P + 'nhwc_f16x3_fmt', P + 'nhwc_f16'
TAIL, TAIL_X3, TAIL_ADD_X3, TAIL_H = P + 'tail_nchw', P + 'tail_nchw_f16x3', P + 'tail_add_nchw_f16x3', P + 'tail_nchw_f16'


def calls(plan):
    """a plan as the library calls it makes, in order: (entry, dilation, fmt) for a C -> C conv3x3 (two per residual block), (entry, skip) for
    a layer that may add a kept result, (entry,) otherwise; ('torch', where) for a PyTorch step"""
    out = []
    for kind, where, m, *a in plan:
        if kind == 'torch':
            out.append(('torch', where))
        elif kind == 'body':
            out.append((a[0], a[2], a[3]))
        elif kind == 'block':
            out += [(a[0], 1, a[1]), (a[2], 1, a[3])]
        elif kind in ('up', 'tail'):
            out.append((a[0], a[1]))
        else:
            out.append((a[0],))
    return out


def _stack(name, backend):
    return calls(D.hip_plan(D.build(name)[0], backend))


@pytest.mark.parametrize('name,nbody', [('dncnn_15', 15), ('dncnn_gray_blind', 18), ('fdncnn_gray', 18)])
def test_plain_stacks(name, nbody):
    assert _stack(name, 'hip') == [(HEAD,)] + [(C64, 1, 0)] * nbody + [(TAIL, None)]
    # split-half: a body layer followed by a body layer stores split (4), reads split if its predecessor stored it (1)
    assert _stack(name, 'hip_f16x3') == [(HEAD,), (FMT, 1, 4)] + [(FMT, 1, 5)] * (nbody - 2) + [(FMT, 1, 1), (TAIL_X3, None)]
    assert _stack(name, 'hip_f16') == [(HEAD_H,)] + [(HALF, 1, 0)] * nbody + [(TAIL_H, None)]


def test_ircnn_dilations():
    dil = [2, 3, 4, 3, 2]
    assert _stack('ircnn_gray', 'hip') == [(HEAD,)] + [(C64, d, 0) for d in dil] + [(TAIL, None)]
    assert _stack('ircnn_gray', 'hip_f16x3') == [(HEAD,)] + [(FMT, d, f) for d, f in zip(dil, (4, 5, 5, 5, 1))] + [(TAIL_X3, None)]
    assert _stack('ircnn_gray', 'hip_f16') == [(HEAD_H,)] + [(HALF, d, 0) for d in dil] + [(TAIL_H, None)]


def test_ffdnet_fused_ends():
    assert _stack('ffdnet_gray', 'hip') == [(HEAD,)] + [(C64, 1, 0)] * 13 + [(TAIL, None)]          # the float32 kernels have no fused ends
    assert _stack('ffdnet_gray', 'hip_f16x3') == ([('pnp_ffdnet_head_nhwc',), (FMT, 1, 4)] + [(FMT, 1, 5)] * 11
                                                  + [(FMT, 1, 1), ('pnp_ffdnet_tail_f16x3',)])
    assert _stack('ffdnet_gray', 'hip_f16') == [('pnp_ffdnet_head_nhwc_f16',)] + [(HALF, 1, 0)] * 13 + [('pnp_ffdnet_tail_f16',)]
    colour = D.FFDNet(in_nc=3, out_nc=3)                                                            # 13 -> 64: not a first layer of the library
    assert calls(D.hip_plan(colour, 'hip_f16x3'))[:3] == [('torch', 0), ('torch', 1), ('pnp_relayout_c64',)]


def _unet(blocks, down, up, head, tail):
    """head, (4 blocks, down) x 3, 4 blocks, (up with skip, 4 blocks) x 3, tail with skip"""
    out = [(head,)]
    for k in (1, 2, 3):
        out += blocks + [(down,)]
    out += blocks
    for k in (3, 2, 1):
        out += [(up, 'm_down%d.4' % k)] + blocks
    return out + [(tail, 'm_head')]


def test_drunet():
    # a run of blocks: f0 = Y | (X if the block's input is split), f2 = X | (SKIP if it is) | (Y if the next block takes it split)
    run = [(FMT, 1, 4), (FMT, 1, 5)] + [(FMT, 1, 5), (FMT, 1, 7)] * 2 + [(FMT, 1, 5), (FMT, 1, 3)]
    assert _stack('drunet_gray', 'hip_f16x3') == _unet(run, 'pnp_conv2x2s2_nhwc_f16x3', 'pnp_convT2x2s2_nhwc_f16x3', HEAD, TAIL_ADD_X3)
    assert _stack('drunet_gray', 'hip_f16') == _unet([(HALF, 1, 0)] * 8, 'pnp_conv2x2s2_nhwc_f16', 'pnp_convT2x2s2_nhwc_f16', HEAD_H, TAIL_H)
    # float32 matrix cores: the ends and the 8 blocks of 64 channels, each on its own between PyTorch's layers
    torch_ = lambda name, ks: [('torch', '%s.%d' % (name, k)) for k in ks]
    assert _stack('drunet_gray', 'hip') == ([(HEAD,)] + [(C64, 1, 0)] * 8 + torch_('m_down1', [4]) + torch_('m_down2', range(5)) + torch_('m_down3', range(5))
                                            + torch_('m_body', range(4)) + torch_('m_up3', range(5)) + torch_('m_up2', range(5)) + torch_('m_up1', [0])
                                            + [(C64, 1, 0)] * 8 + [(TAIL, None)])
    # at a size that does not survive three halvings the 2 x 2 layers are PyTorch's and every block stands alone, in float32 format
    net = D.build('drunet_gray')[0]
    odd = calls(HL.unet_plan(net, 'hip_f16x3', 36, 40))
    assert odd[:3] == [(HEAD,), (FMT, 1, 4), (FMT, 1, 1)] and odd[9] == ('torch', 'm_down1.4') and odd[-1] == (TAIL_X3, None)
    assert odd[10:12] == [(FMT, 1, 4), (FMT, 1, 1)] and sum(1 for c in odd if c[0] == 'torch') == 6
    assert net.hip_covers(32, 40, 'hip_f16x3') and not net.hip_covers(36, 40, 'hip_f16x3') and not net.hip_covers(32, 40, 'hip')


def _mutants():
    """the five families, the networks test_a_network_with_a_layer_the_library_does_not_take_raises_at_construction builds, a stack with a
    ReLU behind its last convolution and one with a 128-channel middle layer"""
    for name in ('ffdnet_gray', 'dncnn_15', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray'):
        yield name, name, D.build(name)[0]
    net = D.DnCNN(nb=5)
    net.model[4] = nn.Conv2d(64, 64, 5, 1, 2)
    yield '5x5', 'dncnn_15', net
    net = D.DnCNN(nb=5)
    net.model[3] = nn.Tanh()
    yield 'tanh', 'dncnn_15', net
    yield 'colour', 'ffdnet_color', D.FFDNet(in_nc=3, out_nc=3)
    net = D.IRCNN()
    net.model[4] = nn.Conv2d(64, 64, 3, 1, 5, dilation=5)
    yield 'dilation 5', 'ircnn_gray', net
    yield '500 channels', 'drunet_gray', D.UNetRes(nc=(64, 128, 256, 500))
    net = D.UNetRes()
    net.m_body[1].res[0] = nn.Conv2d(512, 512, 3, 1, 1, bias=False, groups=2)
    yield 'groups', 'drunet_gray', net
    net = D.DnCNN(nb=5)
    net.model.append(nn.ReLU())
    yield 'relu last', 'dncnn_15', net
    net = D.DnCNN(nb=5)
    net.model[4] = nn.Conv2d(128, 128, 3, 1, 1)
    yield '128 middle', 'dncnn_15', net


def test_coverage_answers_agree_with_the_plan():
    """covered <=> the plan has no PyTorch step, under every backend; the 'hip_f16' constructor raises <=> not covered"""
    seen = {}
    for label, name, net in _mutants():
        for backend in HL.HIP_BACKENDS:
            plan = D.hip_plan(net, backend)
            no_torch = all(step[0] != 'torch' for step in plan)
            covered = net.hip_covers(backend=backend) if isinstance(net, D.UNetRes) else HL.hip_covers_stack(net.model, backend)
            assert covered == no_torch == (HL.uncovered(plan) is None), (label, backend)
            seen[label, backend] = covered
        kw = dict(sigmas=torch.tensor([0.1]), noises=torch.zeros(16, 16).numpy() if D.family(name) == 'fdncnn' else None)
        if seen[label, 'hip_f16']:
            assert D.Denoiser(name, net, 15, backend='hip_f16', **kw).backend == 'hip_f16'
        else:
            with pytest.raises(ValueError, match='hip_f16'):
                D.Denoiser(name, net, 15, backend='hip_f16', **kw)
        D.Denoiser(name, net, 15, backend='hip_f16x3', **kw)                    # the mixing backends take every network
    for name in ('ffdnet_gray', 'dncnn_15', 'fdncnn_gray', 'ircnn_gray'):
        assert all(seen[name, b] for b in HL.HIP_BACKENDS)
    assert (seen['drunet_gray', 'hip'], seen['drunet_gray', 'hip_f16x3'], seen['drunet_gray', 'hip_f16']) == (False, True, True)
    assert not any(seen[label, b] for label in ('5x5', 'tanh', 'colour', 'dilation 5', '500 channels', 'groups', 'relu last', '128 middle')
                   for b in HL.HIP_BACKENDS)
    # the descriptions name the layer
    relu_last, wide = [net for label, _, net in _mutants() if label in ('relu last', '128 middle')]
    assert HL.f16_uncovered_stack(relu_last.model).startswith('layer 8: Conv2d(64, 1,')         # a last layer WITH a ReLU is PyTorch's, as the walk has it
    assert HL.f16_uncovered_stack(wide.model).startswith('layer 4: Conv2d(128, 128,')           # a plain stack's body is 64 -> 64 under every backend
