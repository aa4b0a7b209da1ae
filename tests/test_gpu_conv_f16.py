"""The half-precision kernels behind `Denoiser(backend='hip_f16')` (csrc/kernels_conv_f16.hip, csrc/kernels_pix2x2_f16.hip),
one layer at a time and one forward at a time.

The arithmetic the kernels are held to: half operands (weights rounded to half at pack time), exact products on v_mfma_f32_16x16x32_f16,
float32 accumulation, bias / skip / ReLU in float32, ONE rounding to half on store.  So:

  * a layer asked for float32 output, fed values that ARE halves, is an exact-product float32 accumulation: the suite's one-layer bar,
    rel-L2 <= 2e-6 against float64 of the same half values (one-hot inputs: <= 1e-6);
  * the half output is `.half()` of that float32 result BIT FOR BIT, a float32 x gives the bits of the pre-rounded half x;
  * the 2 x 2 layers take the same flag for a float32 y and are held to the same bars (2e-6; one-hot exact), their half output to bit-equality
    with `.half()` of it;
  * one forward: || hip_f16 - F || <= 1.25 * || E - F || with F the exact float64 forward and E the float64 emulation of the arithmetic
    above, both computed here (the kernels' float32 accumulation adds in quadrature to the format's own error: + 0.5 % measured on
    the CPU; the 25 % covers summation order and DRUNet's depth).
"""
import copy
import ctypes as C

import numpy as np
import pytest

from f16_emulation import emulation

pytestmark = pytest.mark.gpu

X32, K32, Y32 = 1, 2, 4


@pytest.fixture(scope='module')
def env():
    import torch
    import torch.nn.functional as F
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import _lib, denoisers
    assert torch.cuda.is_available() and _lib.device_count() >= 1
    return dict(torch=torch, F=F, P=P, L=_lib.lib(), lib=_lib, D=denoisers)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _s(env):
    return C.c_void_p(env['torch'].cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pack(env, w_oihw):
    torch, L, lib = env['torch'], env['L'], env['lib']
    ch = w_oihw.shape[0]
    w9 = torch.empty(9 * ch * ch, dtype=torch.float16, device='cuda')
    lib.check(L.pnp_conv3x3_pack_f16(_s(env), _p(w_oihw.contiguous()), _p(w9), ch))
    return w9


def _resident(env, wps):
    cus = C.c_int()
    env['lib'].check(env['L'].pnp_device_info(0, None, C.byref(cus), None, 0, None, 0))
    return wps * cus.value


def _assert_grid_is_rounded(env, items, wps, blocks):
    """The precondition of the cases that exercise the persistent grid's rounding (csrc/conv_plan.h: cp_grid): the `wps` workgroups per
    compute unit of THIS card are no multiple of the blocks of 64 channels, and there are more items than those workgroups.  Asserted, not
    skipped on."""
    assert _resident(env, wps) % blocks != 0 and items > _resident(env, wps), (_resident(env, wps), blocks, items)


def _conv(env, x_nhwc, w_oihw, bias, skip, relu, dilation=1, fmt=0):
    """x / skip: NHWC, float32 tensors when fmt says so, halves otherwise -> y NHWC (float32 with Y32, else half)"""
    torch, L, lib = env['torch'], env['L'], env['lib']
    n, H, W, ch = x_nhwc.shape
    assert x_nhwc.dtype == (torch.float32 if fmt & X32 else torch.float16) and x_nhwc.is_contiguous()
    assert skip is None or (skip.dtype == (torch.float32 if fmt & K32 else torch.float16) and skip.is_contiguous())
    y = torch.full((n, H, W, ch), float('nan'), dtype=torch.float32 if fmt & Y32 else torch.float16, device='cuda')
    lib.check(L.pnp_conv3x3_nhwc_f16(_s(env), _p(x_nhwc), _p(_pack(env, w_oihw)), _p(bias), _p(skip), _p(y), n, ch, H, W, 1 if relu else 0, dilation, fmt))
    return y


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------
# one layer
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,H,W', [(3, 136, 136), (2, 16, 16), (1, 8, 16), (2, 5, 23), (1, 1, 1), (5, 128, 128), (7, 136, 136)])
@pytest.mark.parametrize('variant', ['bias_relu', 'plain', 'skip_relu'])
def test_conv3x3_c64_against_float64(env, n, H, W, variant):
    """the shapes and variants of test_gpu_conv.py::test_conv3x3_c64_against_pytorch (tiles that overhang the image, one tile, one pixel)
    and 7 x 136 x 136 = 1071 items on the 768 persistent workgroups of a 256-unit card (three per unit at dilation 1: the loop's second
    trip): x, w, skip drawn, rounded to half; float32 output against float64 of those halves"""
    torch, F = env['torch'], env['F']
    g = torch.Generator(device='cuda').manual_seed(1000 * n + 10 * H + W)
    x = torch.randn(n, 64, H, W, device='cuda', generator=g).half()
    w = (torch.randn(64, 64, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5).half().float()
    b = torch.randn(64, device='cuda', generator=g) * 0.1 if variant != 'plain' else None
    sk = torch.randn(n, 64, H, W, device='cuda', generator=g).half() if variant == 'skip_relu' else None
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=1)
    if sk is not None:
        ref = ref + sk.double()
    if variant != 'plain':
        ref = F.relu(ref)
    xn, skn = _nhwc(x), None if sk is None else _nhwc(sk)
    y = _conv(env, xn, w, b, skn, variant != 'plain', fmt=Y32)
    err = _rel(y.permute(0, 3, 1, 2), ref)
    print('conv3x3 f16 %s %s: rel-L2 vs float64 %.3g' % ((n, H, W), variant, err))
    assert err <= 2e-6
    # formats: the half output is .half() of the float32-format result bit for bit; a float32 x gives the bits of the pre-rounded x; so does
    # a float32 skip that holds half values
    yh = _conv(env, xn, w, b, skn, variant != 'plain', fmt=0)
    assert torch.equal(yh, y.half())
    g2 = torch.Generator(device='cuda').manual_seed(7)
    xf = torch.randn(n, H, W, 64, device='cuda', generator=g2)       # float32 values that are NOT halves
    assert torch.equal(_conv(env, xf, w, b, skn, variant != 'plain', fmt=X32 | Y32), _conv(env, xf.half(), w, b, skn, variant != 'plain', fmt=Y32))
    assert torch.equal(_conv(env, xf, w, b, skn, variant != 'plain', fmt=X32), _conv(env, xf.half(), w, b, skn, variant != 'plain', fmt=0))
    if skn is not None:
        assert torch.equal(_conv(env, xn, w, b, skn.float(), True, fmt=K32 | Y32), y)
    # asymmetric weights + a one-hot input catch a transposed tap or channel map
    x1 = torch.zeros(1, 64, H, W, device='cuda')
    x1[0, 7, H // 2, W // 2] = 1.0
    y1 = _conv(env, _nhwc(x1.half()), w, None, None, False, fmt=Y32)
    assert _rel(y1.permute(0, 3, 1, 2), F.conv2d(x1.double(), w.double(), padding=1)) <= 1e-6


@pytest.mark.parametrize('dilation', [2, 3, 4])
@pytest.mark.parametrize('n,H,W', [(3, 136, 136), (2, 5, 23), (1, 1, 1), (5, 128, 128)])
def test_dilated_conv3x3_c64_against_float64(env, n, H, W, dilation):
    """IRCNN's layers: a halo of d pixels, taps d apart; images smaller than the halo, overhanging tiles, more items than workgroups"""
    torch, F = env['torch'], env['F']
    g = torch.Generator(device='cuda').manual_seed(100 * dilation + n + H)
    x = torch.randn(n, 64, H, W, device='cuda', generator=g).half()
    w = (torch.randn(64, 64, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5).half().float()
    b = torch.randn(64, device='cuda', generator=g) * 0.1
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=dilation, dilation=dilation))
    y = _conv(env, _nhwc(x), w, b, None, True, dilation, Y32)
    assert _rel(y.permute(0, 3, 1, 2), ref) <= 2e-6
    assert torch.equal(_conv(env, _nhwc(x), w, b, None, True, dilation, 0), y.half())
    assert torch.equal(_conv(env, _nhwc(x).float(), w, b, None, True, dilation, X32 | Y32), y)
    x1 = torch.zeros(1, 64, H, W, device='cuda')
    x1[0, 5, H // 2, W // 2] = 1.0
    y1 = _conv(env, _nhwc(x1.half()), w, None, None, False, dilation, Y32)
    assert _rel(y1.permute(0, 3, 1, 2), F.conv2d(x1.double(), w.double(), padding=dilation, dilation=dilation)) <= 1e-6


@pytest.mark.parametrize('ch,n,H,W', [(128, 3, 40, 56), (256, 2, 24, 24), (512, 2, 32, 32), (192, 1, 5, 23), (128, 40, 64, 64), (1024, 1, 9, 9),
                                      (192, 2, 96, 128), (320, 2, 96, 128)])
@pytest.mark.parametrize('variant', ['bias_relu', 'skip'])
def test_wide_layers_against_float64(env, ch, n, H, W, variant):
    """C -> C for C = 128 .. 1024 (DRUNet's other scales): the K loop over chunks of 64 input channels, a workgroup per block of 64 output channels.
    The last two are the shape at which the f16x3 kernels' persistent grid is rounded down to a multiple of the blocks.  This kernel runs THREE
    workgroups per compute unit at dilation 1, always a multiple of the 3 blocks of C = 192 (576 items on 768 workgroups of 256 units: one
    trip, nothing to round) -- the rounding needs a block count that does not divide 3 x units: C = 320, 960 items in 5 blocks on 765 of 768."""
    torch, F = env['torch'], env['F']
    if ch == 320:
        _assert_grid_is_rounded(env, n * ((H + 7) // 8) * ((W + 15) // 16) * (ch // 64), 3, ch // 64)
    g = torch.Generator(device='cuda').manual_seed(ch + n + H)
    x = torch.randn(n, ch, H, W, device='cuda', generator=g).half()
    w = (torch.randn(ch, ch, 3, 3, device='cuda', generator=g) * (2.0 / (9 * ch)) ** 0.5).half().float()
    b = torch.randn(ch, device='cuda', generator=g) * 0.1 if variant == 'bias_relu' else None
    sk = torch.randn(n, ch, H, W, device='cuda', generator=g).half() if variant == 'skip' else None
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=1)
    ref = F.relu(ref) if variant == 'bias_relu' else ref + sk.double()
    skn = None if sk is None else _nhwc(sk)
    y = _conv(env, _nhwc(x), w, b, skn, variant == 'bias_relu', fmt=Y32)
    assert _rel(y.permute(0, 3, 1, 2), ref) <= 2e-6
    assert torch.equal(_conv(env, _nhwc(x), w, b, skn, variant == 'bias_relu', fmt=0), y.half())
    assert torch.equal(_conv(env, _nhwc(x).float(), w, b, skn, variant == 'bias_relu', fmt=X32 | Y32), y)
    x1 = torch.zeros(1, ch, H, W, device='cuda')
    x1[0, ch - 3, H // 2, W // 2] = 1.0
    y1 = _conv(env, _nhwc(x1.half()), w, None, None, False, fmt=Y32)
    assert _rel(y1.permute(0, 3, 1, 2), F.conv2d(x1.double(), w.double(), padding=1)) <= 1e-6


def test_pack_rounds_to_nearest_even(env):
    """the packed weights are the torch `.half()` of the float32 weights (round to nearest even), a permutation of them"""
    torch = env['torch']
    g = torch.Generator(device='cuda').manual_seed(11)
    w = torch.randn(128, 128, 3, 3, device='cuda', generator=g)
    w[0, 0, 0, 0] = 1.0 + 2.0 ** -11                                # a tie: rounds to the even neighbour 1.0
    w[0, 0, 0, 1] = 1.0 + 3 * 2.0 ** -11                            # a tie: rounds up to 1 + 2^-9
    p = _pack(env, w)
    assert torch.equal(p.sort().values, w.half().flatten().sort().values)


@pytest.mark.parametrize('n,H,W', [(3, 136, 136), (2, 16, 16), (2, 5, 23), (1, 1, 1), (4, 128, 128)])
def test_head_layers_store_the_half_of_the_float32_heads(env, n, H, W):
    """first layers keep the float32 direct arithmetic of pnp_conv3x3_head_nhwc / pnp_ffdnet_head_nhwc (held to 2e-6 against float64 here
    too) and store halves: bit-equal to `.half()` of those kernels' results"""
    torch, F, L, lib = env['torch'], env['F'], env['L'], env['lib']
    g = torch.Generator(device='cuda').manual_seed(7 * n + H + W)
    for cin in (1, 2, 5, 8):
        x = torch.randn(n, cin, H, W, device='cuda', generator=g)
        w = torch.randn(64, cin, 3, 3, device='cuda', generator=g) * (2.0 / (9 * cin)) ** 0.5
        b = torch.randn(64, device='cuda', generator=g) * 0.1
        for relu, bias in ((1, b), (0, None)):
            y32 = torch.empty(n, H, W, 64, device='cuda')
            lib.check(L.pnp_conv3x3_head_nhwc(_s(env), _p(x), _p(w), _p(bias), _p(y32), n, cin, H, W, relu))
            ref = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=1)
            assert _rel(y32.permute(0, 3, 1, 2), F.relu(ref) if relu else ref) <= 2e-6
            y16 = torch.full((n, H, W, 64), float('nan'), dtype=torch.float16, device='cuda')
            lib.check(L.pnp_conv3x3_head_nhwc_f16(_s(env), _p(x), _p(w), _p(bias), _p(y16), n, cin, H, W, relu))
            assert torch.equal(y16, y32.half()), (cin, relu)
    # FFDNet's fused head at the full-resolution size (H, W): odd sizes are replicate-padded
    x = torch.rand(n, 1, H, W, device='cuda', generator=g)
    sg = torch.rand(n, device='cuda', generator=g) * 0.2
    w = torch.randn(64, 5, 3, 3, device='cuda', generator=g) * (2.0 / 45) ** 0.5
    b = torch.randn(64, device='cuda', generator=g) * 0.1
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    for per_image in (1, 0):
        y32 = torch.empty(n, h2, w2, 64, device='cuda')
        lib.check(L.pnp_ffdnet_head_nhwc(_s(env), _p(x), _p(sg), per_image, _p(w), _p(b), _p(y32), n, H, W, 1))
        y16 = torch.full((n, h2, w2, 64), float('nan'), dtype=torch.float16, device='cuda')
        lib.check(L.pnp_ffdnet_head_nhwc_f16(_s(env), _p(x), _p(sg), per_image, _p(w), _p(b), _p(y16), n, H, W, 1))
        assert torch.equal(y16, y32.half())


@pytest.mark.parametrize('n,H,W', [(3, 136, 136), (2, 16, 16), (2, 5, 23), (1, 1, 1), (4, 128, 128), (9, 256, 256)])
def test_the_three_tails_against_float64(env, n, H, W):
    """64 -> cout <= 4 reading halves, storing float32: plain, with the second input added while staging (the sum rounded to half once, as
    the operand), and FFDNet's pixel-shuffled, cropped form.  (9 x 256 x 256: 4608 tiles on 512 persistent workgroups.)"""
    torch, F, L, lib = env['torch'], env['F'], env['L'], env['lib']
    g = torch.Generator(device='cuda').manual_seed(13 * n + H + W)
    xn = torch.randn(n, H, W, 64, device='cuda', generator=g).half()
    x2n = torch.randn(n, H, W, 64, device='cuda', generator=g).half()
    for cout in (1, 2, 3, 4):
        w = torch.randn(cout, 64, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5
        b = torch.randn(cout, device='cuda', generator=g) * 0.1
        for bias in (b, None):
            for second in (None, x2n):
                op = xn if second is None else (xn.float() + second.float()).half()
                ref = F.conv2d(op.permute(0, 3, 1, 2).double(), w.half().double(), None if bias is None else bias.double(), padding=1)
                y = torch.full((n, cout, H, W), float('nan'), device='cuda')
                lib.check(L.pnp_conv3x3_tail_nchw_f16(_s(env), _p(xn), _p(second), _p(w), _p(bias), _p(y), n, cout, H, W))
                assert _rel(y, ref) <= 2e-6, (cout, bias is None, second is None)
    # FFDNet: full-resolution size (H, W), the layer runs at ceil / 2
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    xq = torch.randn(n, h2, w2, 64, device='cuda', generator=g).half()
    w = torch.randn(4, 64, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(4, device='cuda', generator=g) * 0.1
    ref = F.pixel_shuffle(F.conv2d(xq.permute(0, 3, 1, 2).double(), w.half().double(), b.double(), padding=1), 2)[..., :H, :W]
    y = torch.full((n, 1, H, W), float('nan'), device='cuda')
    lib.check(L.pnp_ffdnet_tail_f16(_s(env), _p(xq), _p(w), _p(b), _p(y), n, H, W))
    assert _rel(y, ref) <= 2e-6
    x1 = torch.zeros(1, H, W, 64, dtype=torch.float16, device='cuda')
    x1[0, H // 2, W // 2, 9] = 1.0
    w1 = torch.randn(3, 64, 3, 3, device='cuda', generator=g)
    y1 = torch.empty(1, 3, H, W, device='cuda')
    lib.check(L.pnp_conv3x3_tail_nchw_f16(_s(env), _p(x1), None, _p(w1), None, _p(y1), 1, 3, H, W))
    assert _rel(y1, F.conv2d(x1.permute(0, 3, 1, 2).double(), w1.half().double(), padding=1)) <= 1e-6


@pytest.mark.parametrize('up,ch,n,H,W', [(0, 64, 3, 40, 56), (0, 128, 2, 24, 24), (0, 256, 2, 16, 32), (0, 64, 1, 2, 2), (0, 192, 1, 6, 34),
                                        (1, 128, 3, 20, 28), (1, 256, 2, 12, 12), (1, 512, 2, 8, 16), (1, 128, 1, 1, 1), (1, 384, 1, 3, 17),
                                        (0, 64, 12, 128, 128), (1, 128, 8, 64, 64), (0, 192, 4, 96, 128), (1, 384, 2, 48, 64)])
@pytest.mark.parametrize('with_x2', [False, True])
def test_pix2x2_layers_against_float64(env, up, ch, n, H, W, with_x2):
    """DRUNet's Conv2d(C, 2C, 2, 2) and ConvTranspose2d(C, C/2, 2, 2) on halves, with and without the second input (added in float32,
    rounded to half once, as the operand): float32 output against float64 at the one-layer bar, the half output = its `.half()` bit for bit.
    (12 x 128 x 128 down: 768 items, 8 x 64 x 64 up: 1024, on 512 persistent workgroups -- the loop's second trip.  The last two: 576 items in
    6 / 12 blocks of matrix columns -- the grid is rounded down to a multiple of the blocks, 510 / 504 of 512.)"""
    torch, F, L, lib = env['torch'], env['F'], env['L'], env['lib']
    if (ch, n) in ((192, 4), (384, 2)):
        gh, gw = (H, W) if up else (H // 2, W // 2)
        _assert_grid_is_rounded(env, n * ((gh + 7) // 8) * ((gw + 15) // 16) * (2 * ch // 64), 2, 2 * ch // 64)
    g = torch.Generator(device='cuda').manual_seed(up * 1000 + ch + H)
    x = torch.randn(n, H, W, ch, device='cuda', generator=g).half()
    x2 = torch.randn(n, H, W, ch, device='cuda', generator=g).half() if with_x2 else None
    wshape = (ch, ch // 2, 2, 2) if up else (2 * ch, ch, 2, 2)
    w = torch.randn(wshape, device='cuda', generator=g) * (1.0 / (ch if up else 4 * ch)) ** 0.5
    wp = torch.empty(w.numel(), dtype=torch.float16, device='cuda')
    lib.check(L.pnp_conv2x2_pack_f16(_s(env), _p(w), _p(wp), ch, up))
    op = (x if x2 is None else (x.float() + x2.float()).half()).permute(0, 3, 1, 2).double()
    ref = F.conv_transpose2d(op, w.half().double(), stride=2) if up else F.conv2d(op, w.half().double(), stride=2)
    shape = (n, 2 * H, 2 * W, ch // 2) if up else (n, H // 2, W // 2, 2 * ch)
    fn = L.pnp_convT2x2s2_nhwc_f16 if up else L.pnp_conv2x2s2_nhwc_f16
    y32 = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    lib.check(fn(_s(env), _p(x), _p(x2), _p(wp), _p(y32), n, ch, H, W, 1))
    err = _rel(y32.permute(0, 3, 1, 2), ref)
    print('pix2x2 up=%d C=%d %s x2=%s: rel-L2 vs float64 %.3g' % (up, ch, (n, H, W), with_x2, err))
    assert err <= 2e-6
    y = torch.full(shape, float('nan'), dtype=torch.float16, device='cuda')
    lib.check(fn(_s(env), _p(x), _p(x2), _p(wp), _p(y), n, ch, H, W, 0))
    assert torch.equal(y, y32.half())
    # one-hot input: every output is ONE weight, already a half -- exact
    x1 = torch.zeros(1, H, W, ch, dtype=torch.float16, device='cuda')
    x1[0, H // 2, W // 2, ch - 5] = 1.0
    y1 = torch.empty((1,) + tuple(y.shape[1:]), dtype=torch.float16, device='cuda')
    lib.check(fn(_s(env), _p(x1), None, _p(wp), _p(y1), 1, ch, H, W, 0))
    o1 = x1.permute(0, 3, 1, 2).double()
    r1 = F.conv_transpose2d(o1, w.half().double(), stride=2) if up else F.conv2d(o1, w.half().double(), stride=2)
    assert torch.equal(y1.permute(0, 3, 1, 2).double(), r1)


def test_a_slice_does_not_depend_on_its_batch(env):
    """bit for bit: every kernel, a slice alone against the same slice inside a batch of five"""
    torch, L, lib = env['torch'], env['L'], env['lib']
    g = torch.Generator(device='cuda').manual_seed(21)
    n, H, W = 5, 72, 88
    x = torch.randn(n, H, W, 64, device='cuda', generator=g).half()
    sk = torch.randn(n, H, W, 64, device='cuda', generator=g).half()
    w = torch.randn(64, 64, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(64, device='cuda', generator=g) * 0.1
    for dil in (1, 3):
        full = _conv(env, x, w, b, sk, True, dil, 0)
        for k in (0, 3, 4):
            assert torch.equal(_conv(env, x[k:k + 1].contiguous(), w, b, sk[k:k + 1].contiguous(), True, dil, 0), full[k:k + 1])
    w128 = torch.randn(128, 128, 3, 3, device='cuda', generator=g) * (2.0 / 1152) ** 0.5
    x128 = torch.randn(n, 24, 40, 128, device='cuda', generator=g).half()
    full = _conv(env, x128, w128, None, None, True, 1, 0)
    assert torch.equal(_conv(env, x128[2:3].contiguous(), w128, None, None, True, 1, 0), full[2:3])
    wt = torch.randn(1, 64, 3, 3, device='cuda', generator=g) * 0.05
    yt = torch.empty(n, 1, H, W, device='cuda')
    lib.check(L.pnp_conv3x3_tail_nchw_f16(_s(env), _p(x), _p(sk), _p(wt), None, _p(yt), n, 1, H, W))
    y1 = torch.empty(1, 1, H, W, device='cuda')
    lib.check(L.pnp_conv3x3_tail_nchw_f16(_s(env), _p(x[3:4].contiguous()), _p(sk[3:4].contiguous()), _p(wt), None, _p(y1), 1, 1, H, W))
    assert torch.equal(y1, yt[3:4])
    for up in (0, 1):
        ch = 128
        xx = torch.randn(n, 16, 24, ch, device='cuda', generator=g).half()
        ww = torch.randn((ch, ch // 2, 2, 2) if up else (2 * ch, ch, 2, 2), device='cuda', generator=g) * 0.05
        wp = torch.empty(ww.numel(), dtype=torch.float16, device='cuda')
        lib.check(L.pnp_conv2x2_pack_f16(_s(env), _p(ww), _p(wp), ch, up))
        fn = L.pnp_convT2x2s2_nhwc_f16 if up else L.pnp_conv2x2s2_nhwc_f16
        shp = (32, 48, ch // 2) if up else (8, 12, 2 * ch)
        yy = torch.empty((n,) + shp, dtype=torch.float16, device='cuda')
        lib.check(fn(_s(env), _p(xx), None, _p(wp), _p(yy), n, ch, 16, 24, 0))
        y1 = torch.empty((1,) + shp, dtype=torch.float16, device='cuda')
        lib.check(fn(_s(env), _p(xx[1:2].contiguous()), None, _p(wp), _p(y1), 1, ch, 16, 24, 0))
        assert torch.equal(y1, yy[1:2])


def test_range_inf_nan_and_subnormal_operands(env, monkeypatch):
    """a result beyond 65504 is inf in the stored half and finite in the float32 format (loud, not clamped); NaN in gives NaN out through
    the ReLU; operands that are SUBNORMAL halves are multiplied as they are (the matrix cores do not flush them): the 2e-6 bar holds"""
    torch, F, D = env['torch'], env['F'], env['D']
    g = torch.Generator(device='cuda').manual_seed(31)
    x = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device='cuda')
    x[0, 8, 8, 3] = 6e4
    w = torch.zeros(64, 64, 3, 3, device='cuda')
    w[5, 3, 1, 1] = 2.0                                            # y[.., 5] at (8, 8) = 120 000
    w[6, 3, 1, 1] = -2.0
    w += torch.randn(64, 64, 3, 3, device='cuda', generator=g) * 1e-3
    yh, yf = _conv(env, x, w, None, None, False, fmt=0), _conv(env, x, w, None, None, False, fmt=Y32)
    assert torch.isfinite(yf).all() and abs(float(yf[0, 8, 8, 5]) - 1.2e5) < 600
    assert float(yh[0, 8, 8, 5]) == float('inf') and float(yh[0, 8, 8, 6]) == float('-inf')
    assert torch.isfinite(yh[0, :4]).all()
    assert float(_conv(env, x, w, None, None, True, fmt=0)[0, 8, 8, 5]) == float('inf')
    xn = torch.randn(1, 16, 16, 64, device='cuda', generator=g).half()
    xn[0, 4, 4, 9] = float('nan')
    yn = _conv(env, xn, torch.randn(64, 64, 3, 3, device='cuda', generator=g) * 0.05, None, None, True, fmt=0)
    assert torch.isnan(yn[0, 3:6, 3:6]).all() and torch.isfinite(yn[0, 8:]).all()
    # subnormal halves: integers k * 2^-24, |k| < 1024
    xs = (torch.randint(-1023, 1024, (2, 64, 40, 48), device='cuda', generator=g).double() * 2.0 ** -24)
    assert float(xs.abs().max()) < 2.0 ** -14 and torch.equal(xs.half().double(), xs)
    ws = (torch.randn(64, 64, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5).half().float()
    ref = F.conv2d(xs, ws.double(), padding=1)
    ys = _conv(env, _nhwc(xs.half()), ws, None, None, False, fmt=Y32)
    err = _rel(ys.permute(0, 3, 1, 2), ref)
    print('subnormal half operands: rel-L2 vs float64 %.3g' % err)
    assert err <= 2e-6
    # weights outside the half range are refused when they are packed; PNP_CONV_CHECK_RANGE=1 names an activation that left it
    net = D.DnCNN(nb=4)
    net.load_state_dict(D.seeded_state_dict(net, 1))
    with torch.no_grad():
        net.model[2].weight[0, 0, 0, 0] = 1e5
    net.backend = 'hip_f16'
    with pytest.raises(ValueError):
        net.cuda()(torch.rand(1, 1, 16, 16, device='cuda'))
    net = D.DnCNN(nb=4)
    net.load_state_dict(D.seeded_state_dict(net, 1))
    with torch.no_grad():
        net.model[0].weight.mul_(3e5)                              # a float32 first layer: fine as a weight, its result leaves the half range
    net.backend = 'hip_f16'
    net = net.cuda()
    out = net(torch.rand(1, 1, 16, 16, device='cuda'))
    assert not torch.isfinite(out).all()                           # loud at the output
    monkeypatch.setenv('PNP_CONV_CHECK_RANGE', '1')
    with pytest.raises(FloatingPointError):
        net(torch.rand(1, 1, 16, 16, device='cuda'))


# ----------------------------------------------------------------------------------------------
# one forward
# ----------------------------------------------------------------------------------------------
def _family_case(env, name):
    from conftest import weights50, weights_trained
    torch, D = env['torch'], env['D']
    net, nlm, sched = D.build(name)
    if name == 'ffdnet_gray':
        sd = weights_trained('ffdnet_gray')
    elif name == 'dncnn_25':
        sd = weights_trained('dncnn_25')
    elif name == 'ircnn_gray':
        sd = weights50(name)['10']
    else:
        sd = weights50(name)
    net.load_state_dict(sd, strict=True)
    return net.eval(), nlm, sched


@pytest.mark.parametrize('size', [(256, 256), (203, 178)])
@pytest.mark.parametrize('name', ['ffdnet_gray', 'dncnn_25', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray'])
def test_one_forward_against_the_float64_emulation(env, golden_inputs, name, size):
    torch, D = env['torch'], env['D']
    H, W = size
    net, nlm, sched = _family_case(env, name)
    sig = torch.tensor([20.0 / 255]) if sched else None
    noises = golden_inputs['noises'][:H, :W] if D.family(name) == 'fdncnn' else None
    gray = torch.from_numpy(golden_inputs['gray'][:H, :W].astype(np.float32) / 255.0)
    g = torch.Generator().manual_seed(5)
    x = torch.stack([gray, gray.flip(0), gray.flip(1)])[:, None] + torch.randn(3, 1, H, W, generator=g) * (20.0 / 255)
    x = x.float().cuda()
    den = D.Denoiser(name, net, nlm, sigmas=sig, noises=noises, backend='hip_f16').to('cuda')
    net64 = copy.deepcopy(net).double()
    for m in [net64] + list(net64.modules()):
        if hasattr(m, 'backend'):
            m.backend = 'torch'
    mk = lambda n_: D.Denoiser(name, n_, nlm, sigmas=sig, noises=noises, backend='torch', channels_last=False, miopen_find=False).to('cuda')
    F_ = mk(net64)(x.double(), 0).clone()
    E_ = mk(emulation(D, torch, net64).cuda())(x.double(), 0).clone()
    assert F_.dtype == torch.float64 and E_.dtype == torch.float64
    # the forward itself, with every PyTorch convolution made to raise: no MIOpen call
    orig, orig_t, seen = torch.nn.Conv2d.forward, torch.nn.ConvTranspose2d.forward, []

    def boom(self, inp, *a):
        seen.append(1)
        raise AssertionError('a PyTorch convolution was called')
    torch.nn.Conv2d.forward = torch.nn.ConvTranspose2d.forward = boom
    before = torch.backends.cudnn.benchmark
    try:
        Y = den(x, 0).clone()
    finally:
        torch.nn.Conv2d.forward, torch.nn.ConvTranspose2d.forward = orig, orig_t
    assert not seen and torch.backends.cudnn.benchmark == before
    assert Y.dtype == torch.float32 and torch.isfinite(Y).all()
    dY, dE = float((Y.double() - F_).norm()), float((E_ - F_).norm())
    nF = float(F_.norm())
    print('FORWARD %s %dx%d: ||hip_f16 - F|| / ||F|| = %.4g   ||E - F|| / ||F|| = %.4g   ratio %.3f   ||hip_f16 - E|| / ||F|| = %.4g'
          % (name, H, W, dY / nF, dE / nF, dY / dE, float((Y.double() - E_).norm()) / nF))
    assert dE > 0 and dY <= 1.25 * dE
    # graph replay equals the eager forward bit for bit -- for the four families Denoiser captures; an IRCNN forward is never captured
    # (its bank switches between iterations), under any backend
    deng = D.Denoiser(name, net, nlm, sigmas=sig, noises=noises, backend='hip_f16', graph=True).to('cuda')
    assert deng._graph_ok(x) == (D.family(name) != 'ircnn')
    if deng._graph_ok(x):
        for _ in range(2):
            assert torch.equal(deng(x, 0), Y)
        assert deng._graphs


def test_ircnn_bank_switch_repacks(env):
    """the packed half weights are cached per parameter version: loading another model of IRCNN's bank repacks them"""
    from conftest import weights50
    torch, D = env['torch'], env['D']
    bank = weights50('ircnn_gray')
    net, nlm, _ = D.build('ircnn_gray')
    net.load_state_dict(bank['0'])
    den = D.Denoiser('ircnn_gray', net.eval(), nlm, sigmas=torch.tensor([49.0 / 255, 3.0 / 255]), bank=bank, backend='hip_f16').to('cuda')
    x = torch.rand(2, 1, 64, 64, device='cuda')
    outs = []
    for i in (0, 1, 0):
        den.select_bank(i)
        outs.append(den(x, i).clone())
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    fresh, _, _ = D.build('ircnn_gray')
    fresh.load_state_dict(bank[str(int(np.ceil(3.0 / 2.) - 1))])
    ref = D.Denoiser('ircnn_gray', fresh.eval(), nlm, sigmas=torch.tensor([3.0 / 255]), backend='hip_f16').to('cuda')(x, 0)
    assert torch.equal(outs[1], ref)


def test_a_residual_block_called_on_its_own_takes_and_returns_float32(env):
    """`_ResBlock.forward` under 'hip_f16' outside a U-Net: float32 in and out through the format mask -- the input rounded to half as the
    first convolution's operand and added UNROUNDED as the skip, the result not rounded: the same bits as the two layer calls"""
    torch, D = env['torch'], env['D']
    g = torch.Generator(device='cuda').manual_seed(41)
    blk = D._ResBlock(128).cuda().eval()
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn(p_.shape, device='cuda', generator=g) * (2.0 / 1152) ** 0.5)
    blk.backend = 'hip_f16'
    x = torch.randn(2, 128, 24, 40, device='cuda', generator=g)
    with torch.no_grad():
        y = blk(x)
    xn = _nhwc(x)
    h = _conv(env, xn, blk.res[0].weight.detach(), None, None, True, fmt=X32)
    ref = _conv(env, h, blk.res[2].weight.detach(), None, xn, False, fmt=K32 | Y32)
    assert y.dtype == torch.float32 and torch.equal(y, ref.permute(0, 3, 1, 2))
