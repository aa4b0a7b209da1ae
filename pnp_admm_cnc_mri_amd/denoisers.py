"""Denoiser networks of the PnP solvers as plain PyTorch-ROCm modules (the north star keeps the
CNN forward pass in PyTorch/MIOpen: MFMA work lives only inside these conv layers).

Own declarations of the five architectures the reference instantiates, with KAIR's state_dict
key names so real `model_zoo/*.pth` files load with `strict=True`:

    DnCNN   models/network_dncnn.py:36-67    model.{0,2,..,32}.{weight,bias}   17 conv, x - n
    FDnCNN  models/network_dncnn.py:120-141  model.{0,2,..,38}                 20 conv, 2-ch in
    IRCNN   models/network_dncnn.py:70-109   model.{0,2,..,12}                 7 dilated conv, x - n
    FFDNet  models/network_ffdnet.py:31-73   model.{0,2,..,28}                 unshuffle/15 conv/shuffle
    UNetRes models/network_unet.py:76-136    m_head, m_down{1,2,3}, m_body, m_up{3,2,1}, m_tail (DRUNet)

plus the dispatch `denoising_step` (S6:18-67 == S3:19-68), the inference wrapper `test_mode`
(utils/utils_model.py:12-109; modes 0 and 2 are the ones the solvers reach), `augment_img_tensor4`
(utils/utils_image.py:333-349) and a deterministic weight generator for parity tests (the
reference ships no weights: model_zoo/README.md).
"""
import hashlib
import logging
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_layers as HL
from .hip_layers import HIP_BACKENDS, split_activations, unsplit_activations  # noqa: F401 -- the last two: read from here by tests/test_gpu_conv.py


def _conv_stack(in_nc, out_nc, nc, nb, dilations=None):
    """[Conv3x3, ReLU] * (nb-1) + Conv3x3 as one nn.Sequential (conv at the even indices)."""
    L = []
    for i in range(nb):
        ci = in_nc if i == 0 else nc
        co = out_nc if i == nb - 1 else nc
        d = 1 if dilations is None else dilations[i]
        L.append(nn.Conv2d(ci, co, 3, 1, d, dilation=d, bias=True))
        if i != nb - 1:
            L.append(nn.ReLU(inplace=True))
    return nn.Sequential(*L)


class _PlainStack(nn.Module):
    """shared by DnCNN / FDnCNN / FFDNet / IRCNN: `self.model` is the conv stack, `backend` selects who runs it (hip_layers.stack_forward)"""
    backend = 'torch'

    def _stack(self, x):
        return HL.stack_forward(self.model, x, self.backend) if self.backend in HIP_BACKENDS else self.model(x)


class DnCNN(_PlainStack):
    def __init__(self, in_nc=1, out_nc=1, nc=64, nb=17):
        super().__init__()
        self.model = _conv_stack(in_nc, out_nc, nc, nb)

    def forward(self, x):
        return x - self._stack(x)


class FDnCNN(_PlainStack):
    def __init__(self, in_nc=2, out_nc=1, nc=64, nb=20):
        super().__init__()
        self.model = _conv_stack(in_nc, out_nc, nc, nb)

    def forward(self, x):
        return self._stack(x)


class IRCNN(_PlainStack):
    def __init__(self, in_nc=1, out_nc=1, nc=64):
        super().__init__()
        self.model = _conv_stack(in_nc, out_nc, nc, 7, dilations=[1, 2, 3, 4, 3, 2, 1])

    def forward(self, x):
        return x - self._stack(x)


class FFDNet(_PlainStack):
    def __init__(self, in_nc=1, out_nc=1, nc=64, nb=15):
        super().__init__()
        self.model = _conv_stack(in_nc * 4 + 1, out_nc * 4, nc, nb)

    def _fused_ok(self, x, sigma):
        """backends 'hip_f16x3' / 'hip_f16', gray in and out, every layer on libpnpmri.so: the pad / pixel-unshuffle / concatenation in front
        of the stack and the pixel-shuffle / crop behind it are folded into the first and last layer's kernels (hip_layers.stack_plan)"""
        return (self.backend in HIP_BACKENDS and x.is_cuda and x.dtype == torch.float32 and x.shape[1] == 1 and sigma.numel() in (1, x.shape[0])
                and HL.stack_plan(self.model, self.backend, ffdnet=True)[0][0] == 'ffdnet_head')

    def _forward_fused(self, x, sigma, out=None):
        xc = x.contiguous()
        sg = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
        if out is None:
            out = torch.empty_like(xc)
        elif not (out.is_contiguous() and out.shape == xc.shape and out.dtype == torch.float32 and out.device == x.device):
            raise ValueError('FFDNet: `out` must be a contiguous float32 tensor of the input\'s shape on its device')
        return HL.stack_forward(self.model, xc, self.backend, sg, out)

    def forward(self, x, sigma, out=None):
        """sigma: [B,1,1,1] (or [1,1,1,1], broadcast over the batch -- the reference's
        `sigma.repeat(1, 1, H/2, W/2)` only works for B = 1, models/network_ffdnet.py:67).  out: optional result tensor."""
        if self._fused_ok(x, sigma):
            return self._forward_fused(x, sigma, out)
        h, w = x.shape[-2:]
        x = F.pad(x, (0, int(math.ceil(w / 2) * 2 - w), 0, int(math.ceil(h / 2) * 2 - h)), mode='replicate')
        x = F.pixel_unshuffle(x, 2)
        m = sigma.to(x.dtype).expand(x.shape[0], 1, x.shape[-2], x.shape[-1])
        x = self._stack(torch.cat((x, m), 1))
        x = F.pixel_shuffle(x, 2)
        x = x[..., :h, :w]
        return x if out is None else out.copy_(x)


class _ResBlock(nn.Module):
    """x + conv(relu(conv(x))), bias-free (models/basicblock.py:213-225, mode 'CRC').  With a HIP backend the blocks its kernels take
    (64 channels: DRUNet's full-resolution scale, 28 % of its arithmetic, where MIOpen's fp32 kernels are at their slowest; every
    scale under 'hip_f16x3' / 'hip_f16') run on libpnpmri.so, the residual add fused into the second convolution's epilogue."""
    backend = 'torch'

    def __init__(self, nc):
        super().__init__()
        self.res = nn.Sequential(nn.Conv2d(nc, nc, 3, 1, 1, bias=False), nn.ReLU(inplace=True),
                                 nn.Conv2d(nc, nc, 3, 1, 1, bias=False))

    def hip_ok(self, backend=None):
        return HL.block_ok(self, backend or self.backend)             # backend=: "would it, under that backend?"

    def forward_nhwc(self, ctx, xn, entry0, fmt0, entry2, fmt2):
        """the block on a contiguous [n][H][W][C] tensor, on libpnpmri.so; entry points and formats: hip_layers.block_calls"""
        be = HL.BACKENDS[self.backend]
        h = HL.conv3x3(ctx, be, entry0, xn, self.res[0], None, True, fmt0)
        return HL.conv3x3(ctx, be, entry2, h, self.res[2], xn, False, fmt2)

    def forward(self, x):
        if self.hip_ok():
            ctx = HL.lib_ctx(x, boundary=True)
            xn = x.permute(0, 2, 3, 1)
            if not xn.is_contiguous():
                xn = xn.contiguous()                           # NCHW-contiguous input: one copy; channels_last tensors pass as they are
            return self.forward_nhwc(ctx, xn, *HL.block_calls(HL.BACKENDS[self.backend], self)).permute(0, 3, 1, 2)   # a channels_last NCHW view
        if self.backend == 'hip_f16':
            raise ValueError("backend='hip_f16': libpnpmri.so does not take %r" % self.res)
        return x + self.res(x)


class UNetRes(nn.Module):
    """DRUNet: 4 scales, 4 residual blocks each, stride-2 conv down, 2x2 transposed conv up, no bias.  With a HIP backend the
    first (2 -> 64) and last (64 -> 1) convolution run on libpnpmri.so's direct kernels as well; under 'hip_f16x3' / 'hip_f16' so do
    the 2 x 2 strided / transposed convolutions between the scales (csrc/kernels_pix2x2_*.hip) and the skip sums: no MIOpen call is
    left (hip_covers); under 'hip' (float32 matrix cores: 64-channel blocks only) the other layers stay with PyTorch."""
    backend = 'torch'

    def __init__(self, in_nc=2, out_nc=1, nc=(64, 128, 256, 512), nb=4):
        super().__init__()
        rb = lambda c: [_ResBlock(c) for _ in range(nb)]
        self.m_head = nn.Conv2d(in_nc, nc[0], 3, 1, 1, bias=False)
        self.m_down1 = nn.Sequential(*rb(nc[0]), nn.Conv2d(nc[0], nc[1], 2, 2, 0, bias=False))
        self.m_down2 = nn.Sequential(*rb(nc[1]), nn.Conv2d(nc[1], nc[2], 2, 2, 0, bias=False))
        self.m_down3 = nn.Sequential(*rb(nc[2]), nn.Conv2d(nc[2], nc[3], 2, 2, 0, bias=False))
        self.m_body = nn.Sequential(*rb(nc[3]))
        self.m_up3 = nn.Sequential(nn.ConvTranspose2d(nc[3], nc[2], 2, 2, 0, bias=False), *rb(nc[2]))
        self.m_up2 = nn.Sequential(nn.ConvTranspose2d(nc[2], nc[1], 2, 2, 0, bias=False), *rb(nc[1]))
        self.m_up1 = nn.Sequential(nn.ConvTranspose2d(nc[1], nc[0], 2, 2, 0, bias=False), *rb(nc[0]))
        self.m_tail = nn.Conv2d(nc[0], out_nc, 3, 1, 1, bias=False)

    def hip_covers(self, H=None, W=None, backend=None):
        """True when EVERY layer of the U-Net runs on libpnpmri.so (hip_layers.unet_plan has no PyTorch step): such a forward makes no
        MIOpen call at all.  H, W (if given) must survive three halvings.  backend=: "would it, under that backend?" """
        be = backend or self.backend
        return be in HIP_BACKENDS and HL.uncovered(HL.unet_plan(self, be, H, W)) is None

    def _forward_nhwc(self, x0, plan):
        """models/network_unet.py:123-136 by a plan without a PyTorch step: every tensor NHWC (halves under 'hip_f16'), the four skip
        sums formed inside the kernel that consumes them (transposed convolution / last layer), never in memory"""
        ctx, be = HL.lib_ctx(x0, boundary=True), HL.BACKENDS[self.backend]
        kept = {}                                              # results a later layer adds as its skip, by the step that made them
        for kind, where, m, *a in plan:
            if kind == 'block':
                t = m.forward_nhwc(ctx, t, *a)
            elif kind == 'down':
                t = kept[where] = HL.conv2x2(ctx, be, a[0], t, None, m, False)
            elif kind == 'up':
                t = HL.conv2x2(ctx, be, a[0], t, kept[a[1]], m, True)      # m_up(x + x_skip)
            elif kind == 'head':
                t = kept[where] = HL.head(ctx, be, a[0], x0, m, a[1])
            else:
                return HL.tail(ctx, be, a[0], t, kept[a[1]], m)

    def forward(self, x0):
        plan = None
        if self.backend in HIP_BACKENDS and x0.is_cuda and x0.dtype == torch.float32:
            plan = HL.unet_plan(self, self.backend, x0.shape[-2], x0.shape[-1])
            if HL.uncovered(plan) is None:
                return self._forward_nhwc(x0, plan)
        if self.backend == 'hip_f16':                          # all of it on libpnpmri.so, or an error: no mixing with PyTorch layers
            if plan is None:
                raise RuntimeError("Denoiser(backend='hip_f16') needs float32 CUDA tensors")
            raise ValueError("backend='hip_f16': libpnpmri.so does not take %s of this U-Net at %d x %d (every layer must be one it takes, "
                             "H and W multiples of 8)" % (HL.uncovered(plan), x0.shape[-2], x0.shape[-1]))
        # the mixed forward: the ends by the plan, the blocks each on their own (_ResBlock.forward), the rest PyTorch
        head, tail = (plan[0], plan[-1]) if plan else (('torch',), ('torch',))
        if plan:
            ctx, be = HL.lib_ctx(x0, boundary=True), HL.BACKENDS[self.backend]
        x1 = HL.head(ctx, be, head[3], x0, self.m_head, False).permute(0, 3, 1, 2) if head[0] == 'head' else self.m_head(x0)     # a channels_last NCHW view
        x2 = self.m_down1(x1)
        x3 = self.m_down2(x2)
        x4 = self.m_down3(x3)
        x = self.m_body(x4)
        x = self.m_up3(x + x4)
        x = self.m_up2(x + x3)
        x = self.m_up1(x + x2)
        x = x + x1
        if tail[0] != 'tail':
            return self.m_tail(x)
        xn = x.permute(0, 2, 3, 1)
        return HL.tail(ctx, be, tail[3], xn if xn.is_contiguous() else xn.contiguous(), None, self.m_tail)


def hip_plan(model, backend, H=None, W=None):
    """hip_layers' classification of `model`'s layers under a HIP backend (H, W: of the tensor a U-Net is called with)"""
    if isinstance(model, UNetRes):
        return HL.unet_plan(model, backend, H, W)
    if isinstance(model, _PlainStack):
        return HL.stack_plan(model.model, backend, ffdnet=isinstance(model, FFDNet))
    return [('torch', 'a %s' % type(model).__name__, None)]


# ----------------------------------------------------------------------------------------------
# model construction by name, as the substring switch of S6:129-217 / S3:122-215 does it
# ----------------------------------------------------------------------------------------------
def family(model_name):
    if 'dncnn' in model_name and 'fdncnn' not in model_name:
        return 'dncnn'
    for f in ('fdncnn', 'drunet', 'ircnn', 'ffdnet'):
        if f in model_name:
            return f
    raise ValueError('unknown denoiser %r' % model_name)


def build(model_name):
    """-> (module, noise_level_model, uses_sigma_schedule).  Constants: S6:131,150,167,186,201."""
    fam = family(model_name)
    if fam == 'dncnn':
        nb = 20 if model_name in ['dncnn_gray_blind', 'dncnn_color_blind', 'dncnn3'] else 17      # S6:133-136
        return DnCNN(1, 1, 64, nb), 15, False
    if fam == 'fdncnn':
        return FDnCNN(2, 1, 64, 20), 15, False
    if fam == 'drunet':
        return UNetRes(2, 1, (64, 128, 256, 512), 4), 15 / 255.0, True
    if fam == 'ircnn':
        return IRCNN(1, 1, 64), 15 / 255.0, True
    return FFDNet(1, 1, 64, 15), 15, False


def seeded_state_dict(module, seed=0, gain=1.0):
    """Deterministic synthetic weights, generated per tensor from a NumPy RNG keyed by
    (seed, state_dict key) -- identical wherever it is run, independent of torch's RNG.
    He-scaled normal weights (x gain), small biases, last layer damped so outputs stay O(input)."""
    sd = module.state_dict()
    keys = list(sd.keys())
    last_w = [k for k in keys if k.endswith('weight')][-1]
    out = {}
    for k in keys:
        v = sd[k]
        h = int.from_bytes(hashlib.sha256(('%d:%s' % (seed, k)).encode()).digest()[:8], 'little')
        rng = np.random.default_rng(h)
        if k.endswith('weight'):
            fan_in = int(np.prod(v.shape[1:])) if v.dim() > 1 else int(v.shape[0])
            std = gain * math.sqrt(2.0 / fan_in) * (0.3 if k == last_w else 1.0)
            if '.res.2.' in k:
                std *= 0.1            # residual branches near identity: keeps deep random nets well conditioned
            a = rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(std)
        else:
            a = rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(0.01)
        out[k] = torch.from_numpy(a)
    return out


# Contractive synthetic weights (parity fixtures at the reference's own 50 iterations, tests/golden/pnp50_*).  He-scaled random nets
# are expansive: two float32 implementations of the same PnP loop drift 1e-2 apart in 50 iterations, which says nothing about
# either.  Here every convolution is  W = a P + (eps / sigma) R:  P the centre-tap identity on the channels both sides share
# (image channels -> the same-numbered feature channels in the first layer, all C channels in a C -> C layer, the first out_nc
# channels in the last), R standard normal from the seeded per-key generator, sigma = the operator norm of conv(R) (power
# iteration, measured ONCE by oracle/make_golden_pnp.py and committed in tests/golden/pnp_known.json so that every machine builds
# bit-identical weights).  Each layer is then (a + eps)-Lipschitz, every feature channel carries O(1) activations through the
# whole depth, and the map of the network is  a_last x + (a few per cent of seeded features):  a denoiser-like contraction.
_CONTRACTIVE = {          # role -> (a, eps); 'tail' a is per family below
    'head': (1.0, 0.5), 'body': (1.0, 0.01), 'res0': (0.0, 1.0), 'res2': (0.0, 0.02), 'down': (0.0, 0.5), 'up': (0.0, 0.5), 'tail': (None, 0.01)}
# x - n(x) families: n ~ 0.15 x (IRCNN) / 0.3 x (DnCNN: with 0.15 the DnCNN-pair preset, alpha 1.2 and lambda 4 (S6:571), amplifies a
# 1e-6 difference between two float32 convolution implementations ~15 x in 50 iterations; with 0.3, 3 x).  Direct maps: 0.6 .. 0.7 -- with 0.85 the reference's own PNP_ADMM_L1_D loop (clamps on x, z AND w,
# S3:293-296) grows a pixel-local oscillation in dark regions from iteration ~35 on (profiles/experiments/contractive_sens.py): a property
# of that loop, not of an implementation, but a fixture must not sit on it
_CONTRACTIVE_TAIL = {'dncnn': 0.3, 'ircnn': 0.15, 'fdncnn': 0.7, 'ffdnet': 0.6, 'drunet': 0.6}


def contractive_roles(module):
    """{state_dict weight key: role} for the five architectures (see _CONTRACTIVE)."""
    keys = [k for k in module.state_dict() if k.endswith('weight')]
    roles = {}
    if isinstance(module, UNetRes):
        for k in keys:
            if k == 'm_head.weight':
                roles[k] = 'head'
            elif k == 'm_tail.weight':
                roles[k] = 'tail'
            elif '.res.0.' in k:
                roles[k] = 'res0'
            elif '.res.2.' in k:
                roles[k] = 'res2'
            elif k.startswith('m_down'):
                roles[k] = 'down'
            elif k.startswith('m_up'):
                roles[k] = 'up'
            else:
                raise ValueError(k)
    else:
        for n, k in enumerate(keys):
            roles[k] = 'head' if n == 0 else 'tail' if n == len(keys) - 1 else 'body'
    return roles


def contractive_state_dict(module, fam, seed, gains):
    """Deterministic CONTRACTIVE weights (comment above).  `gains`: {weight key: operator norm of the conv with the seeded standard-
    normal kernel R} as committed in tests/golden/pnp_known.json ('gains50'); a pure function of (architecture, family, seed, gains)."""
    sd = module.state_dict()
    roles = contractive_roles(module)
    n_img = 4 if fam == 'ffdnet' else 1
    out = {}
    for k, v in sd.items():
        h = int.from_bytes(hashlib.sha256(('%d:%s' % (seed, k)).encode()).digest()[:8], 'little')
        rng = np.random.default_rng(h)
        if not k.endswith('weight'):
            out[k] = torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32) * np.float32(0.01))
            continue
        role = roles[k]
        a, eps = _CONTRACTIVE[role]
        if role == 'tail':
            a = _CONTRACTIVE_TAIL[fam]
        r = rng.standard_normal(tuple(v.shape))                     # float64
        wgt = r * (eps / float(gains[k]))
        if a:
            co, ci = v.shape[0], v.shape[1]
            n = n_img if role == 'head' else co if role == 'tail' else min(co, ci)
            ctr = (v.shape[2] // 2, v.shape[3] // 2)
            for c in range(min(n, co, ci)):
                wgt[c, c, ctr[0], ctr[1]] += a
        out[k] = torch.from_numpy(wgt.astype(np.float32))
    return out


# ----------------------------------------------------------------------------------------------
# inference helpers
# ----------------------------------------------------------------------------------------------
# The eight symmetries of the square as (quarter turns counter-clockwise in the (H, W) plane, then
# an up-down flip), numbered the way utils/utils_image.py:333-349 numbers its x8 self-ensemble modes.
_D4 = ((0, False), (1, True), (0, True), (3, False), (2, True), (1, False), (2, False), (3, True))


def augment_img_tensor4(img, mode=0):
    """x8 self-ensemble view `mode` of a [B,C,H,W] tensor (same numbering as the reference's
    `augment_img_tensor4`; modes 3 and 5 are each other's inverse, every other mode is its own)."""
    turns, flip = _D4[mode]
    out = torch.rot90(img, turns, (2, 3)) if turns else img
    return out.flip(2) if flip else out


def _corner_span(n, refield):
    """Length of the two overlapping windows [0, q) and [n - q, n) a side of length n is cut into:
    half the side rounded up to the next multiple of the receptive field (utils_model.py:91-94)."""
    return (n // 2 // refield + 1) * refield


def test_split_fn(model, L, refield=32, min_size=256, sf=1, modulo=1):
    """Quadrant inference with the arithmetic of utils/utils_model.py:76-109, batched: an image of
    at most min_size^2 pixels goes through the model whole (replicate-padded to a multiple of
    `modulo`); a larger one is cut into its four overlapping corner windows, which are stacked into
    ONE [4B, C, qh, qw] batch and sent through the model in one call (again split when a window is
    itself larger than min_size^2), and each window contributes the quarter of the output it covers
    without overlap.  One larger MIOpen launch per layer instead of four."""
    B = L.shape[0]
    h, w = L.shape[-2:]
    if h * w <= min_size ** 2:
        ph, pw = -h % modulo, -w % modulo
        if ph or pw:
            L = F.pad(L, (0, pw, 0, ph), mode='replicate')
        return model(L)[..., :h * sf, :w * sf]
    qh, qw = _corner_span(h, refield), _corner_span(w, refield)
    corners = [(r0, c0) for r0 in (0, h - qh) for c0 in (0, w - qw)]        # TL, TR, BL, BR
    tiles = torch.cat([L[..., r0:r0 + qh, c0:c0 + qw] for r0, c0 in corners], dim=0).contiguous()
    if h * w <= 4 * min_size ** 2:
        E = model(tiles)
    else:
        E = test_split_fn(model, tiles, refield, min_size, sf, modulo)
    out = torch.empty((B, E.shape[1], h * sf, w * sf), dtype=E.dtype, device=E.device)
    hm, wm = (h // 2) * sf, (w // 2) * sf                                   # where the quarters meet
    for k, (r0, c0) in enumerate(corners):
        rows = slice(0, hm) if r0 == 0 else slice(hm, h * sf)               # output rows of this quarter
        cols = slice(0, wm) if c0 == 0 else slice(wm, w * sf)
        e = E[k * B:(k + 1) * B]
        out[..., rows, cols] = e[..., rows.start - r0 * sf:rows.stop - r0 * sf, cols.start - c0 * sf:cols.stop - c0 * sf]
    return out


def test_mode(model, L, mode=0, refield=32, min_size=256, sf=1, modulo=1):
    """utils/utils_model.py:12-37, the modes the solvers use: 0 (plain) and 2 (split)."""
    if mode == 0:
        return model(L)
    if mode == 2:
        return test_split_fn(model, L, refield, min_size, sf, modulo)
    raise NotImplementedError('test_mode %d is not reached by the PnP solvers' % mode)


def forward_flops(den, H, W, device, detail=False):
    """Floating-point operations of ONE denoiser call on one H x W slice: 2 x the multiply-accumulates of every
    Conv2d / ConvTranspose2d the call really executes (counted by forward hooks on a one-slice probe, so the quadrant split of
    DRUNet above 256 x 256 and the 1/4-resolution FFDNet body are what they are, not what a formula assumes).
    detail=True -> (total, part): `part` = the flops of the C -> C conv3x3 layers and <= 4-channel last layers that backend
    'hip_f16x3' runs as THREE half-precision matrix products per float32 product (bench_pnp.py prices those at 3 x)."""
    macs = [0, 0]

    def hook(m, inp, out):
        kh, kw = m.kernel_size
        if isinstance(m, torch.nn.ConvTranspose2d):
            n = inp[0].numel() * (m.out_channels // m.groups) * kh * kw
        else:
            n = out.numel() * (m.in_channels // m.groups) * kh * kw
        macs[0] += n
        if HL._hip_body_ok(m, 'f16x3') or HL._hip_tail_ok(m):
            macs[1] += n

    hs = [m.register_forward_hook(hook) for m in den.model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    swapped = [(m, m.backend) for m in den.model.modules() if getattr(m, 'backend', None) in HIP_BACKENDS]
    graph, den.graph = den.graph, False          # nothing of the probe may end up in a captured graph
    for m, _ in swapped:
        m.backend = 'torch'                  # the probe counts module calls; the HIP backend does the same arithmetic outside them
    try:
        den(torch.rand((1, 1, H, W), dtype=torch.float32, device=device), 0)
    finally:
        for h in hs:
            h.remove()
        for m, b in swapped:
            m.backend = b
        den.graph = graph
    return (2 * macs[0], 2 * macs[1]) if detail else 2 * macs[0]


def auto_backend(model, device=None, bank=None, cnn_dtype=None, shape=None):
    """What `cnn_backend='auto'` (the entry points' default since round 6) resolves to: ('hip_f16x3' | 'torch', reason).
    'hip_f16x3' -- the split-half matrix-core kernels of libpnpmri.so, held to the same goldens and bars as the PyTorch / MIOpen backend at
    every run length (tests/test_gpu_pnp.py) -- when (a) the device is a gfx950 part, (b) EVERY convolution of the network is one the
    library takes (hip_plan has no PyTorch step: otherwise part of the forward would still be MIOpen's), (c) every weight -- of
    every model of an IRCNN bank -- is finite and inside the half range, (d) float32 arithmetic is asked for, (e) the slices' shape (H, W),
    if given, is a multiple of 8 on both sides (the shapes the split-half kernels are held to).  'torch' otherwise."""
    if cnn_dtype not in (None, 'fp32'):
        return 'torch', 'cnn_dtype=%s is a PyTorch autocast mode' % cnn_dtype
    if shape is not None and (int(shape[0]) % 8 or int(shape[1]) % 8):
        return 'torch', 'slices of %d x %d: H, W not multiples of 8' % (int(shape[0]), int(shape[1]))
    dev = torch.device(device if device is not None else 'cuda')
    if dev.type != 'cuda' or not torch.cuda.is_available():
        return 'torch', 'no HIP device'
    arch = getattr(torch.cuda.get_device_properties(dev), 'gcnArchName', '')
    if not arch.startswith('gfx950'):
        return 'torch', 'device is %s, the kernels are built for gfx950' % (arch or 'unknown')
    if HL.uncovered(hip_plan(model, 'hip_f16x3')):
        return 'torch', 'the network has layers libpnpmri.so does not take'
    sds = [model.state_dict()] + ([bank[k] for k in bank] if bank else [])
    for sd in sds:
        for k, v in sd.items():
            if torch.is_floating_point(v) and not HL.in_half_range(v):
                return 'torch', 'weight %s lies outside the half range' % k
    return 'hip_f16x3', 'every convolution on libpnpmri.so (split-half f16 matrix-core kernels), weights inside the half range'


class Denoiser:
    """`denoising_step2` (S6:18-67) == `denoising_step1` (S3:19-68) bound to one model: maps a
    [B,1,H,W] float32 CUDA tensor to the denoised tensor for iteration i."""

    def __init__(self, model_name, model, noise_level_model, sigmas=None, noises=None, x8=False, bank=None,
                 cnn_batch=None, channels_last=True, cnn_dtype=None, miopen_find='auto', backend='torch', graph=False, shape=None):
        """backend: 'torch' (default: the whole forward in PyTorch-ROCm / MIOpen, as the north star keeps it) or 'hip' (the
        64 -> 64 conv3x3 (+ ReLU) layers of DnCNN / FDnCNN / FFDNet / IRCNN (dilations 1..4) and DRUNet's 64-channel residual
        blocks on libpnpmri.so's fp32-MFMA kernel, the plain stacks' first and last layers on its direct kernels; float32 only)
        or 'hip_f16' (opt-in throughput mode, never chosen by 'auto': halves between the layers, one matrix instruction per product,
        float32 accumulation -- NOT at the 1e-5 parity bar; every layer must be one libpnpmri.so takes, or the constructor raises)
        or 'hip_f16x3' (the same as 'hip', with the 64 -> 64 layers in split-half arithmetic on the f16 matrix cores: float32 operands
        carried as two halves, three exact-product matrix instructions per product, float32 accumulation -- float32-level
        results at several times the float32 matrix rate; operands must lie within the half range).  shape: the slices' (H, W),
        for backend='auto' (auto_backend)."""
        # graph=True: a forward of at most `cnn_batch` slices is captured once per input shape into a HIP graph (torch.cuda.CUDAGraph)
        # and replayed -- for the reference's own usage, ONE slice per call (S6:231), where a forward is a train of 17 .. 70 launches
        # of a few microseconds each.  Same kernels, same results; re-captured when a parameter changes (load_state_dict).
        self.graph = bool(graph)
        self._graphs = {}
        self._sig_static = None
        self._in_graph = False
        if backend == 'auto':
            backend, why = auto_backend(model, None, bank, cnn_dtype, shape)
            logging.getLogger('pnp_admm_cnc_mri_amd').info('cnn_backend=auto -> %s (%s)', backend, why)
        if backend not in ('torch',) + HIP_BACKENDS:
            raise ValueError("backend must be 'auto', 'torch', 'hip', 'hip_f16x3' or 'hip_f16'")
        if backend in HIP_BACKENDS and cnn_dtype not in (None, 'fp32'):
            raise ValueError("backend='%s' takes and returns float32 only" % backend)
        if backend == 'hip_f16':                               # full coverage or nothing: no PyTorch layer in a half-precision forward
            bad = HL.uncovered(hip_plan(model, backend))
            if bad:
                raise ValueError("backend='hip_f16' needs every layer on libpnpmri.so; it does not take %s" % bad)
        self.name, self.fam = model_name, family(model_name)
        self.model = model
        self.backend = backend
        if isinstance(model, (_PlainStack, UNetRes)):
            model.backend = backend
        for m in model.modules():
            if isinstance(m, _ResBlock):
                m.backend = backend
        self.noise_level_model = noise_level_model
        self.sigmas = sigmas              # torch tensor [iter_num] (drunet / ircnn)
        self.x8 = x8
        self.bank = bank                  # ircnn: {str(idx): state_dict}
        self.former_idx = 0
        # slices per CNN call.  None (default): 64 -- except for the plain stacks (FFDNet, DnCNN, FDnCNN, IRCNN) on the HIP backends, where a call
        # takes up to 256 slices of 256 x 256 (fewer for larger slices: the same pixel count): their 64-channel layers are short launches at
        # 64 slices (16 items per workgroup of the wide kernel), and 256 per call measured +5 % on config 3 (profiles/experiments/
        # ab_cnn_batch_r06.txt; DRUNet: +-0, its tensors are four times larger).  Results do not depend on it (bit-equal per slice on the HIP
        # backends, tests/test_gpu_round2.py) wherever libpnpmri.so runs every layer; DRUNet under 'hip' leaves its wider layers to MIOpen,
        # whose default kernels do not even repeat bit for bit: float32 round-off apart there, bit-equal only with
        # torch.backends.cudnn.deterministic set (100 x slower: the caller's choice; tests/test_gpu_denoiser_shapes.py).
        self._cnn_batch_auto = cnn_batch is None
        if cnn_batch is None:
            cnn_batch = 256 if (backend in HIP_BACKENDS and isinstance(model, _PlainStack)) else 64
        self.cnn_batch = cnn_batch
        self.channels_last = channels_last        # NHWC weights/activations: MIOpen's faster fp32 conv path (+9 %)
        # MIOpen "find" mode (torch.backends.cudnn.benchmark) for the forward passes.  Without a find-db entry MIOpen's
        # immediate mode can fall back to a kernel that is two orders of magnitude slower: on a fresh MI355X box the
        # FFDNet stack at 64 x 1 x 256 x 256 per call ran 25.7 s per PnP iteration (512 slices) against 0.172 s once a
        # find had run.  'auto' = find for conv batches of at least 16 images (throughput runs; one-off search of a few
        # seconds per new shape, cached by MIOpen), immediate mode for the single-image calls of the reference-sized runs.
        self.miopen_find = miopen_find
        # None = float32 (parity with the reference).  'bf16' / 'fp16' run the conv stack under
        # torch.autocast on the MFMA low-precision path: a throughput mode that does NOT meet the
        # 1e-5 parity bar and is never used by tests of record.
        self.cnn_dtype = {None: None, 'fp32': None, 'bf16': torch.bfloat16, 'fp16': torch.float16}[cnn_dtype]
        self.noise_map = None
        if self.fam == 'fdncnn':
            if noises is None:
                raise ValueError('fdncnn needs `noises` for its noise-level map (S6:26-29)')
            nm = np.absolute(np.asarray(noises)).astype(np.float32) / np.float32(255.)
            self.noise_map = torch.from_numpy(nm)[None, None]          # [1,1,H,W]

    def to(self, device):
        self.model = self.model.to(device)
        if self.channels_last and torch.device(device).type == 'cuda':
            self.model = self.model.to(memory_format=torch.channels_last)
        if self.sigmas is not None:
            self.sigmas = self.sigmas.to(device)
        if self.noise_map is not None:
            self.noise_map = self.noise_map.to(device)
        return self

    def select_bank(self, i):
        """IRCNN's 25-model bank: index from sigma_i, reload on change (S6:289-298)."""
        if self.fam != 'ircnn' or self.bank is None:
            return
        current_idx = int(np.ceil(float(self.sigmas[i]) * 255. / 2.) - 1)
        if current_idx != self.former_idx:
            self.model.load_state_dict(self.bank[str(current_idx)], strict=True)
            self.model.eval()
        self.former_idx = current_idx

    def _one(self, x, i, out=None):
        """the model on one batch of at most cnn_batch slices; `out` (FFDNet): the result goes straight into this tensor"""
        fam = self.fam
        if fam == 'dncnn':
            return self.model(x)
        if fam == 'fdncnn':
            return self.model(torch.cat((x, self.noise_map.expand(x.shape[0], -1, -1, -1)), dim=1))
        if fam == 'drunet':
            if self.x8:
                x = augment_img_tensor4(x, i % 8)
            # inside _graph_forward (warm-up, capture, replay) the noise level is a device scalar refreshed per call; every other
            # path -- batches beyond cnn_batch, graph switched off, the flop probe -- reads iteration i's own value
            sig = self._sig_static if self._in_graph else self.sigmas[i]
            s = sig.float().reshape(1, 1, 1, 1).expand(x.shape[0], 1, x.shape[2], x.shape[3])
            x = test_mode(self.model, torch.cat((x, s), dim=1), mode=2, refield=32, min_size=256, modulo=16)
            if self.x8:
                x = augment_img_tensor4(x, 8 - i % 8 if i % 8 in (3, 5) else i % 8)
            return x
        if fam == 'ircnn':
            if self.x8:
                x = augment_img_tensor4(x, i % 8)
            x = self.model(x)
            if self.x8:
                x = augment_img_tensor4(x, 8 - i % 8 if i % 8 in (3, 5) else i % 8)
            return x
        sigma = torch.full((1, 1, 1, 1), self.noise_level_model / 255., dtype=x.dtype, device=x.device)
        return self.model(x, sigma) if out is None else self.model(x, sigma, out=out)

    def _graph_ok(self, x):
        return (self.graph and x.is_cuda and x.shape[0] <= self.cnn_batch and self.cnn_dtype is None and not self.x8
                and self.bank is None and self.fam in ('dncnn', 'fdncnn', 'ffdnet', 'drunet'))

    def _graph_forward(self, x, i):
        """replay (capturing first) the HIP graph of `_one` for this input shape"""
        params = (tuple((p.data_ptr(), p._version) for p in self.model.parameters()),
                  tuple(getattr(m, 'backend', None) for m in self.model.modules()))      # what the captured launches depend on
        key = (tuple(x.shape), x.device.index)
        ent = self._graphs.get(key)
        if self.fam == 'drunet':
            if self._sig_static is None:
                self._sig_static = torch.zeros((), dtype=torch.float32, device=x.device)
            self._sig_static.copy_(self.sigmas[i])
        if ent is None or ent[0] != params:
            static_in = x.clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
            self._in_graph = True
            try:
                with torch.cuda.stream(side):                     # warm-up off the capture: weight packing, MIOpen's choices, the allocator
                    for _ in range(2):
                        self._one(static_in, i)
                torch.cuda.current_stream(x.device).wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    static_out = self._one(static_in, i)
            finally:
                self._in_graph = False
            ent = self._graphs[key] = (params, g, static_in, static_out)
        _, g, static_in, static_out = ent
        static_in.copy_(x)
        g.replay()
        return static_out

    @torch.no_grad()
    def __call__(self, x, i, out=None):
        B = x.shape[0]
        if out is None:
            out = torch.empty_like(x)
        if self._graph_ok(x):
            out.copy_(self._graph_forward(x, i))
            return out
        find = (min(B, self.cnn_batch) >= 16 and x.is_cuda) if self.miopen_find == 'auto' else bool(self.miopen_find)
        if find and self.backend in HIP_BACKENDS and not HL.uncovered(hip_plan(self.model, self.backend, *(-(-d // 16) * 16 for d in x.shape[-2:]))):
            find = False                      # no MIOpen call in this forward: the process-global flag is left alone.  DRUNet: every layer on
                                              # libpnpmri.so at the size the model is CALLED with -- test_mode pads to multiples of 16 (_one,
                                              # utils/utils_model.py:60-68), so three halvings always survive
        cd = torch.backends.cudnn
        before = cd.benchmark
        cd.benchmark = bool(find or before)
        try:
            cb = self.cnn_batch
            if self._cnn_batch_auto and cb > 64:          # the automatic 256 is for 256 x 256 slices: the same pixel count per call for larger ones
                cb = max(64, cb * 65536 // max(65536, x.shape[-2] * x.shape[-1]))
            for b0 in range(0, B, cb):
                if (self.cnn_dtype is None and self.backend in ('hip_f16x3', 'hip_f16') and isinstance(self.model, FFDNet) and x.is_cuda and out.is_contiguous()
                        and out.dtype == torch.float32 and out.device == x.device):
                    self._one(x[b0:b0 + cb], i, out=out[b0:b0 + cb])     # no copy: the last layer writes the slice itself
                elif self.cnn_dtype is None:
                    out[b0:b0 + cb] = self._one(x[b0:b0 + cb], i)
                else:
                    with torch.autocast('cuda', dtype=self.cnn_dtype):
                        out[b0:b0 + cb] = self._one(x[b0:b0 + cb], i).float()
        finally:
            cd.benchmark = before
        return out
