"""The denoisers' layers on libpnpmri.so (`Denoiser(backend='hip' | 'hip_f16x3' | 'hip_f16')`): which
layer of a network the library takes under which backend (ONE classification: `stack_plan`, `unet_plan`), the calls themselves, the
walk of a plain stack, and the weight caches.  The architectures, `Denoiser` and the U-Net's walk are in denoisers.py.

The plain stacks' 64 -> 64 conv3x3 (+ ReLU) layers -- 97 % of FFDNet's and DnCNN's arithmetic, IRCNN's dilated ones included -- and
DRUNet's residual blocks run on the library with activations in NHWC; the stacks' first (<= 8 -> 64) and last (64 -> <= 4) layers on
its direct kernels, so that DnCNN / FDnCNN / FFDNet / IRCNN make no MIOpen call at all.
  'hip'        float32 matrix cores (csrc/kernels_conv.hip: 0.77-0.79 of the fp32 matrix peak where MIOpen reaches 0.56-0.59)
  'hip_f16x3'  float32 operands as pairs of halves, three exact-product f16 matrix instructions per product, float32 accumulation
               (csrc/kernels_conv_f16x3.hip: float32-level error, 1.9-2.6 x the fp32 matrix peak; also DRUNet's 128 / 256 / 512-
               channel blocks and its 2 x 2 layers)
  'hip_f16'    HALF precision between the layers (csrc/kernels_conv_f16.hip, kernels_pix2x2_f16.hip): activations stored as halves,
               weights rounded to half at pack time, ONE matrix instruction per product, float32 accumulation, one rounding per layer
               on store; the network's input, output and first layer stay float32.  A throughput mode: it does NOT meet the 1e-5
               parity bar, is opt-in, is never chosen by 'auto', and needs EVERY layer on the library (no mixing with PyTorch layers).
Same weights, same state_dict; the default backend is PyTorch-ROCm / MIOpen (the north star's split).  Nothing here computes on
another device or falls back: a missing library or a CPU tensor raises.
"""
import collections
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib

# What differs between the backends, as data: the arithmetic's name, the dtype of activations between layers and of packed weights, the
# entry points, the trailing arguments of the 2 x 2 calls (the half kernels' y_f32 = 0), where PNP_CONV_CHECK_RANGE=1 looks, and
# whether layers the library does not take may run in PyTorch inside the same forward.
_Backend = collections.namedtuple('_Backend', 'math act wdtype pack pack2x2 conv head tail tail_skip down up extra2x2 ffdnet_head ffdnet_tail '
                                              'relayout checks mixes')
_f32, _f16 = torch.float32, torch.float16
BACKENDS = {
    'hip': _Backend('f32', _f32, _f32, 'pnp_conv3x3_c64_pack', None, 'pnp_conv3x3_c64_nhwc', 'pnp_conv3x3_head_nhwc', 'pnp_conv3x3_tail_nchw', None,
                    None, None, (), None, None, 'pnp_relayout_c64', (), True),
    'hip_f16x3': _Backend('f16x3', _f32, _f32, 'pnp_conv3x3_pack_f16x3', 'pnp_conv2x2_pack_f16x3', 'pnp_conv3x3_c64_nhwc_f16x3', 'pnp_conv3x3_head_nhwc',
                          'pnp_conv3x3_tail_nchw_f16x3', 'pnp_conv3x3_tail_add_nchw_f16x3', 'pnp_conv2x2s2_nhwc_f16x3', 'pnp_convT2x2s2_nhwc_f16x3', (),
                          'pnp_ffdnet_head_nhwc', 'pnp_ffdnet_tail_f16x3', 'pnp_relayout_c64', ('conv',), True),
    'hip_f16': _Backend('f16', _f16, _f16, 'pnp_conv3x3_pack_f16', 'pnp_conv2x2_pack_f16', 'pnp_conv3x3_nhwc_f16', 'pnp_conv3x3_head_nhwc_f16',
                        'pnp_conv3x3_tail_nchw_f16', 'pnp_conv3x3_tail_nchw_f16', 'pnp_conv2x2s2_nhwc_f16', 'pnp_convT2x2s2_nhwc_f16', (0,),
                        'pnp_ffdnet_head_nhwc_f16', 'pnp_ffdnet_tail_f16', None, ('conv', '2x2', 'tail'), False),
}
HIP_BACKENDS = tuple(BACKENDS)


def _hip_math(backend):
    return BACKENDS[backend].math if backend in BACKENDS else 'f32'


# pnp_conv3x3_nhwc_f16's format mask: which tensors are float32 INSTEAD of half (include/pnp_mri.h)
F16_X_F32, F16_SKIP_F32, F16_Y_F32 = 1, 2, 4

# The SPLIT activation format the f16x3 layers hand to each other (include/pnp_mri.h, pnp_conv3x3_nhwc_f16x3_fmt): same shape and bytes
# as the float32 NHWC tensor, every block of 64 channels stored as [64 hi halves][64 lo halves], value = hi + lo / 2048.
FMT_X, FMT_SKIP, FMT_Y = 1, 2, 4

HALF_MAX = 65504                                                   # the half range: operands of the f16 matrix instructions


def split_activations(x_nhwc):
    """float32 [n][H][W][C] -> the same-shaped float32-typed tensor holding the split format (tests, debugging; the kernels do this
    in their epilogues)"""
    n, H, W, Cc = x_nhwc.shape
    hi = x_nhwc.to(torch.float16)
    lo = ((x_nhwc - hi.float()) * 2048.0).to(torch.float16)
    blk = torch.stack((hi.reshape(n, H, W, Cc // 64, 64), lo.reshape(n, H, W, Cc // 64, 64)), dim=4)       # [n][H][W][C/64][2][64] halves
    return blk.contiguous().view(torch.float32).reshape(n, H, W, Cc)


def unsplit_activations(s_nhwc):
    """the inverse: split format -> float32 values hi + lo / 2048"""
    n, H, W, Cc = s_nhwc.shape
    blk = s_nhwc.contiguous().view(torch.float16).reshape(n, H, W, Cc // 64, 2, 64).float()
    return (blk[..., 0, :] + blk[..., 1, :] / 2048.0).reshape(n, H, W, Cc)


def in_half_range(v):
    """every value finite and within the half range (synchronises)"""
    return bool(torch.isfinite(v).all()) and float(v.abs().max()) <= HALF_MAX


def _check_range(be, site, t_nhwc, where, split=False):
    """PNP_CONV_CHECK_RANGE=1 (bring-up with real KAIR weights): every activation handed to an f16x3 or f16 layer must be finite and
    within the half range -- beyond it the layer's operands turn into inf / NaN (loudly, but only at the output).  Off by default: it
    synchronises the stream at every layer.  site: 'conv' | '2x2' | 'tail', looked at where the backend's table says."""
    if site not in be.checks or os.environ.get('PNP_CONV_CHECK_RANGE') != '1':
        return
    v = unsplit_activations(t_nhwc) if split else t_nhwc
    if in_half_range(v):
        return
    if v.dtype == torch.float16:                                   # backend 'hip_f16': a value that left the half range was STORED as inf
        raise FloatingPointError("backend='hip_f16': an activation entering %s is not finite: a layer's result left the half range "
                                 "(|x| <= %d) or NaN came in" % (where, HALF_MAX))
    raise FloatingPointError("backend='hip_f16x3': an activation entering %s is not finite or lies outside the half range "
                             "(|x| <= %d): max |x| = %r" % (where, HALF_MAX, float(torch.nan_to_num(v.abs(), nan=float('inf')).max())))


# ----------------------------------------------------------------------------------------------
# which layers the library takes: each predicate once
# ----------------------------------------------------------------------------------------------
def _plain3x3(conv):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros')


def _hip_head_ok(conv):
    """a first layer of the direct kernels: few image channels -> 64"""
    return _plain3x3(conv) and conv.in_channels <= 8 and conv.out_channels == 64


def _hip_tail_ok(conv):
    """a last layer of the direct kernels: 64 -> few image channels"""
    return _plain3x3(conv) and conv.in_channels == 64 and conv.out_channels <= 4


def _hip_body_ok(conv, math='f32'):
    """a 64 -> 64 conv3x3, stride 1, dilation d in 1..4 with zero padding d: the layers libpnpmri.so's matrix-core kernels take
    (d = 1: DnCNN / FDnCNN / FFDNet bodies, DRUNet's 64-channel blocks; d = 2..4: IRCNN, models/network_dncnn.py:87-101); the
    f16x3 and f16 kernels also take C -> C channels for C = 128 .. 1024 in steps of 64 at d = 1 (DRUNet's other scales)"""
    if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.groups == 1
            and conv.padding_mode == 'zeros' and conv.dilation[0] == conv.dilation[1] and conv.padding == conv.dilation
            and conv.in_channels == conv.out_channels):
        return False
    if conv.in_channels == 64:
        return 1 <= conv.dilation[0] <= 4
    return math in ('f16x3', 'f16') and conv.in_channels % 64 == 0 and 64 < conv.in_channels <= 1024 and conv.dilation[0] == 1


def block_ok(block, backend):
    """a residual block x + conv(relu(conv(x))) (`block.res`) whose two convolutions are body layers under `backend`"""
    res = getattr(block, 'res', None)
    return (backend in BACKENDS and isinstance(res, nn.Sequential) and len(res) == 3
            and _hip_body_ok(res[0], BACKENDS[backend].math) and _hip_body_ok(res[2], BACKENDS[backend].math))


def _hip_2x2_ok(m, up):
    """DRUNet's scale changes: a bias-free Conv2d(C, 2C, 2, 2) (up: ConvTranspose2d(C, C / 2, 2, 2)), csrc/kernels_pix2x2_*.hip"""
    if not (isinstance(m, nn.ConvTranspose2d if up else nn.Conv2d) and m.kernel_size == (2, 2) and m.stride == (2, 2) and m.padding == (0, 0)
            and m.bias is None and m.groups == 1 and m.dilation == (1, 1) and m.in_channels <= 1024):
        return False
    if up:
        return m.output_padding == (0, 0) and 2 * m.out_channels == m.in_channels and m.in_channels % 128 == 0
    return m.out_channels == 2 * m.in_channels and m.in_channels % 64 == 0


# ----------------------------------------------------------------------------------------------
# ONE classification per layer.  A plan is a list of steps (kind, where, module, ...) in execution order; the walks execute it, and
# "is the network covered", "which layer is not", "does the forward call MIOpen" are read from it (uncovered).  No tensor, no GPU.
#   ('head', where, conv, entry, relu)            ('ffdnet_head', where, conv, entry, relu)
#   ('body', where, conv, entry, relu, dilation, fmt)
#   ('tail', where, conv, entry, skip)            ('ffdnet_tail', where, conv, entry)           skip: `where` of the step whose result is added, or None
#   ('block', where, block, entry0, fmt0, entry2, fmt2)                                        a residual block's two body layers
#   ('down', where, conv, entry)                  ('up', where, conv, entry, skip)             the U-Net's 2 x 2 layers
#   ('relayout', where, conv, entry)              NCHW -> NHWC in front of a body layer (no call for a channels_last tensor)
#   ('torch', where, module)                      PyTorch runs it: allowed under 'hip' and 'hip_f16x3', an error under 'hip_f16'
# ----------------------------------------------------------------------------------------------
def conv_entry(be, ch, fmt):
    """the entry point of a C -> C conv3x3: the split-half family has one for 64 channels in float32 format, one for more channels,
    and one for tensors in the split activation format"""
    if be.math == 'f16x3' and (fmt or ch != 64):
        return 'pnp_conv3x3_nhwc_f16x3_fmt' if fmt else 'pnp_conv3x3_nhwc_f16x3'
    return be.conv


def block_calls(be, block, first=True, last=True, f32_io=True):
    """(entry0, fmt0, entry2, fmt2) of a residual block's two convolutions.  f16x3: the tensor between them is in the split activation
    format (the first convolution splits its outputs once, the second copies halves into its operand tile), and so is the tensor
    between two blocks of a run -- first / last: the block's place in its run.  f16: halves, unless the block takes and returns float32
    (f32_io: called on its own; its input is rounded to half as the first convolution's operand and added unrounded as the skip)."""
    f0 = f2 = 0
    if be.math == 'f16x3':
        f0 = FMT_Y | (0 if first else FMT_X)
        f2 = FMT_X | (0 if first else FMT_SKIP) | (0 if last else FMT_Y)
    elif be.math == 'f16' and f32_io:
        f0, f2 = F16_X_F32, F16_SKIP_F32 | F16_Y_F32
    ch = block.res[0].in_channels
    return conv_entry(be, ch, f0), f0, conv_entry(be, ch, f2), f2


def stack_plan(seq, backend, ffdnet=False):
    """the plan of a [Conv3x3, ReLU] * (nb - 1) + Conv3x3 stack: a first layer with <= 8 input channels and a last layer with <= 4 output
    channels on the direct kernels, 64 -> 64 layers (the float32 kernel's rule under every backend: no wider layers in a plain stack) on
    the matrix cores, a ReLU with the convolution in front of it.  f16x3: a body layer followed by a body layer stores the split
    activation format (FMT_Y), and reads it (FMT_X) if the one before it stored it.  ffdnet: gray FFDNet (5 -> 64 ... 64 -> 4) with every
    layer on the library has its un/shuffle stages folded into the first and last layer's kernels."""
    be = BACKENDS[backend]
    mods = list(seq)
    steps, nhwc, split, k = [], False, False, 0                    # nhwc: the tensor is [n][H][W][64] between library layers; split: in the split format
    while k < len(mods):
        m = mods[k]
        relu = k + 1 < len(mods) and isinstance(mods[k + 1], nn.ReLU)
        kn = k + (2 if relu else 1)
        if not nhwc and _hip_head_ok(m):
            steps.append(('head', k, m, be.head, relu))
            nhwc = True
        elif _hip_body_ok(m) and (nhwc or be.relayout):
            if not nhwc:
                steps.append(('relayout', k, m, be.relayout))
            fmt = 0
            if be.math == 'f16x3':
                out_split = kn < len(mods) and _hip_body_ok(mods[kn])          # the next layer is then a body layer too: nhwc holds
                fmt, split = (FMT_X if split else 0) | (FMT_Y if out_split else 0), out_split
            steps.append(('body', k, m, conv_entry(be, 64, fmt), relu, m.dilation[0], fmt))
            nhwc = True
        elif nhwc and _hip_tail_ok(m) and not relu:
            steps.append(('tail', k, m, be.tail, None))
            nhwc = False
        else:
            steps.append(('torch', k, m))
            nhwc, kn = False, k + 1                                # a ReLU behind it is a PyTorch step of its own
        k = kn
    if nhwc:
        steps.append(('torch', 'the end of the stack (its last layer is no 64 -> <= 4 convolution): a channels_last view for PyTorch', None))
    if (ffdnet and be.ffdnet_head and uncovered(steps) is None and steps[0][0] == 'head' and steps[0][2].in_channels == 5
            and steps[-1][0] == 'tail' and steps[-1][2].out_channels == 4):
        steps[0] = ('ffdnet_head',) + steps[0][1:3] + (be.ffdnet_head, steps[0][4])
        steps[-1] = ('ffdnet_tail',) + steps[-1][1:3] + (be.ffdnet_tail,)
    return steps


def unet_plan(net, backend, H=None, W=None):
    """the plan of a UNetRes (m_head, m_down1..3 = blocks + 2 x 2 down, m_body, m_up3..1 = 2 x 2 up + blocks, m_tail).  When the library
    takes EVERY layer (f16x3 / f16; H, W, if given, survive three halvings) the whole forward is NHWC: runs of blocks hand split
    tensors on (block_calls), each up layer adds its skip while it stages its operand and the last layer adds the first one's result.
    Otherwise each layer stands alone between PyTorch's: the ends and the blocks the library takes, in float32 format, no fused skips."""
    be = BACKENDS[backend]
    halves = H is None or not (H % 8 or W % 8)
    layers = [('head' if _hip_head_ok(net.m_head) else 'torch', 'm_head', net.m_head)]
    for name in ('m_down1', 'm_down2', 'm_down3', 'm_body', 'm_up3', 'm_up2', 'm_up1'):
        seq = getattr(net, name)
        for k, m in enumerate(seq):
            if name.startswith('m_down') and k == len(seq) - 1:
                kind, ok = 'down', be.down and halves and _hip_2x2_ok(m, False)
            elif name.startswith('m_up') and k == 0:
                kind, ok = 'up', be.up and halves and _hip_2x2_ok(m, True)
            else:
                kind, ok = 'block', block_ok(m, backend)
            layers.append((kind if ok else 'torch', '%s.%d' % (name, k), m))
    layers.append(('tail' if _hip_tail_ok(net.m_tail) else 'torch', 'm_tail', net.m_tail))
    full = all(kind != 'torch' for kind, _, _ in layers)
    steps, skips = [], []
    for i, (kind, where, m) in enumerate(layers):
        if kind == 'block':
            steps.append((kind, where, m) + block_calls(be, m, not (full and layers[i - 1][0] == 'block'), not (full and layers[i + 1][0] == 'block'),
                                                        f32_io=not full))
        elif kind == 'head':
            steps.append((kind, where, m, be.head, False))
            skips.append(where)
        elif kind == 'down':
            steps.append((kind, where, m, be.down))
            skips.append(where)
        elif kind == 'up':
            steps.append((kind, where, m, be.up, skips.pop() if full else None))
        elif kind == 'tail':
            steps.append((kind, where, m, be.tail_skip if full else be.tail, skips.pop() if full else None))
        else:
            steps.append((kind, where, m))
    return steps


def uncovered(plan):
    """None when the library takes every layer of the plan -- such a forward makes no MIOpen call at all --, else a description of the
    first step that is PyTorch's"""
    for step in plan:
        if step[0] == 'torch':
            where = step[1] if isinstance(step[1], str) else 'layer %d' % step[1]          # a stack's steps carry the layer's index
            return where if step[2] is None else '%s: %r' % (where, step[2])
    return None


def hip_covers_stack(seq, backend='hip'):
    return uncovered(stack_plan(seq, backend)) is None


def f16_uncovered_stack(seq):
    return uncovered(stack_plan(seq, 'hip_f16'))


# ----------------------------------------------------------------------------------------------
# plumbing: the library, the stream, pointers; the weight caches
# ----------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lib_ctx(t, boundary=False):
    """(library, the current stream of the tensor's device, pointer-of) for a call on `t`; boundary: `t` enters a network from outside"""
    if not t.is_cuda or (boundary and t.dtype != torch.float32):
        raise RuntimeError("Denoiser's HIP backends need CUDA tensors, float32 at the network's boundary")
    return _lib.lib(), C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream), _ptr


def _cached(conv, slot, build, *args):
    """build(conv.weight as a contiguous [out][in][kh][kw] tensor, *args), kept in the layer's own __dict__ -- outside the state_dict, not
    moved by .to() -- and rebuilt when the parameter changes (load_state_dict, IRCNN's bank switches; a captured graph's warm-up fills it)"""
    w = conv.weight
    key = (w.data_ptr(), w._version, str(w.device))
    cache = conv.__dict__.setdefault('_pnp_hip_w', {})
    hit = cache.get(slot)
    if hit is None or hit[0] != key:
        cache[slot] = hit = (key, build(w.detach().contiguous(memory_format=torch.contiguous_format), *args))
    return hit[1]


def _oihw(conv):
    """conv.weight as an [out][in][3][3]-contiguous tensor (the parameter may be in channels_last format)"""
    return _cached(conv, 'oihw', torch.clone)


def _pack(src, conv, be, L, stream, transposed):
    if be.math != 'f32' and not in_half_range(src):
        raise ValueError("backend='hip_%s': a convolution weight lies outside the half range (|w| <= %d)" % (be.math, HALF_MAX))
    packed = torch.empty(src.numel(), dtype=be.wdtype, device=src.device)
    if transposed is None:
        _lib.check(getattr(L, be.pack)(stream, _ptr(src), _ptr(packed), *(() if be.math == 'f32' else (conv.in_channels,))))
    else:
        _lib.check(getattr(L, be.pack2x2)(stream, _ptr(src), _ptr(packed), conv.in_channels, int(transposed)))
    return packed


def _packed(conv, be, L, stream, transposed=None):
    """conv.weight in the fragment order of the backend's matrix-core kernels (halves under 'hip_f16', rounded to nearest even once,
    at pack time).  transposed: None for a conv3x3, False / True for a 2 x 2 stride-2 (transposed) convolution."""
    return _cached(conv, be.math, _pack, conv, be, L, stream, transposed)


# ----------------------------------------------------------------------------------------------
# the calls
# ----------------------------------------------------------------------------------------------
def head(ctx, be, entry, x, conv, relu):
    """a network's first layer: float32 NCHW in, [n][H][W][64] in the backend's activation dtype out"""
    L, stream, ptr = ctx
    xc = x.contiguous()
    n, _, H, W = xc.shape
    y = torch.empty((n, H, W, 64), dtype=be.act, device=x.device)
    _lib.check(getattr(L, entry)(stream, ptr(xc), ptr(_oihw(conv)), ptr(conv.bias), ptr(y), n, conv.in_channels, H, W, int(relu)))
    return y


def ffdnet_head(ctx, be, entry, x, sigma, conv, relu):
    """FFDNet's first layer straight from the network's own gray input: replicate pad to even size, pixel-unshuffle and the noise-level
    map (one level for the batch or one per image) inside the kernel"""
    L, stream, ptr = ctx
    n, _, h, w = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, 64), dtype=be.act, device=x.device)
    _lib.check(getattr(L, entry)(stream, ptr(x), ptr(sigma), 1 if sigma.numel() > 1 else 0, ptr(_oihw(conv)), ptr(conv.bias), ptr(y), n, h, w, int(relu)))
    return y


def conv3x3(ctx, be, entry, x_nhwc, conv, skip_nhwc, relu, fmt=0):
    """one C -> C conv3x3 (+ bias, + skip, ReLU) on a contiguous [n][H][W][C] tensor; fmt: FMT_* (f16x3) or F16_* (f16) bits"""
    L, stream, ptr = ctx
    n, H, W, ch = x_nhwc.shape
    f32 = 0 if be.math == 'f16' else -1                            # the F16_* bits say which tensors are float32; every one under the other backends
    if x_nhwc.dtype != (_f32 if (fmt | f32) & F16_X_F32 else _f16) or (
            skip_nhwc is not None and skip_nhwc.dtype != (_f32 if (fmt | f32) & F16_SKIP_F32 else _f16)):
        raise TypeError('%s: a tensor\'s dtype does not match fmt=%d' % (entry, fmt))
    if be.checks:
        _check_range(be, 'conv', x_nhwc, 'a %d-channel conv3x3' % ch, split=be.math == 'f16x3' and bool(fmt & FMT_X))
    out = torch.empty(x_nhwc.shape, dtype=_f32 if (fmt | f32) & F16_Y_F32 else _f16, device=x_nhwc.device)
    d = conv.dilation[0]
    if entry == 'pnp_conv3x3_nhwc_f16x3':                          # more than 64 channels, float32 format: dilation 1, no mask
        dims = (n, ch, H, W, int(relu))
    elif entry == be.conv and be.math != 'f16':                    # the 64-channel entry points
        dims = (n, H, W, int(relu), d)
    else:
        dims = (n, ch, H, W, int(relu), d, fmt)
    _lib.check(getattr(L, entry)(stream, ptr(x_nhwc), ptr(_packed(conv, be, L, stream)), ptr(conv.bias), ptr(skip_nhwc), ptr(out), *dims))
    return out


def conv2x2(ctx, be, entry, t_nhwc, skip_nhwc, conv, up):
    """DRUNet's Conv2d(C, 2C, 2, 2) / ConvTranspose2d(C, C / 2, 2, 2) of t + skip (the sum is formed while the operand is staged)"""
    L, stream, ptr = ctx
    _check_range(be, '2x2', t_nhwc, 'a 2 x 2 convolution')
    c = conv.in_channels
    n, h, w, _ = t_nhwc.shape
    out = torch.empty((n, 2 * h, 2 * w, c // 2) if up else (n, h // 2, w // 2, 2 * c), dtype=be.act, device=t_nhwc.device)
    wp = _packed(conv, be, L, stream, up)
    _lib.check(getattr(L, entry)(stream, ptr(t_nhwc), ptr(skip_nhwc), ptr(wp), ptr(out), n, c, h, w, *be.extra2x2))
    return out


def tail(ctx, be, entry, x_nhwc, skip_nhwc, conv):
    """a network's last layer: [n][H][W][64] (+ skip, where the entry point takes one) in, float32 NCHW out"""
    L, stream, ptr = ctx
    _check_range(be, 'tail', x_nhwc, 'the last layer')
    n, H, W, _ = x_nhwc.shape
    out = torch.empty((n, conv.out_channels, H, W), dtype=torch.float32, device=x_nhwc.device)
    x2 = (ptr(skip_nhwc),) if entry == be.tail_skip else ()
    _lib.check(getattr(L, entry)(stream, ptr(x_nhwc), *x2, ptr(_oihw(conv)), ptr(conv.bias), ptr(out), n, conv.out_channels, H, W))
    return out


def ffdnet_tail(ctx, be, entry, x_nhwc, conv, out):
    """FFDNet's last layer straight into the network's own [n][1][h][w] output: pixel-shuffle and crop inside the kernel"""
    L, stream, ptr = ctx
    _check_range(be, 'tail', x_nhwc, 'the last layer')
    n, _, h, w = out.shape
    _lib.check(getattr(L, entry)(stream, ptr(x_nhwc), ptr(_oihw(conv)), ptr(conv.bias), ptr(out), n, h, w))
    return out


def to_nhwc(ctx, entry, h):
    """a float32 NCHW tensor of 64 channels as [n][H][W][64]: a channels_last tensor already is, in memory"""
    hp = h.permute(0, 2, 3, 1)
    if hp.is_contiguous():
        return hp
    L, stream, ptr = ctx
    nhwc = torch.empty(hp.shape, dtype=h.dtype, device=h.device)
    _lib.check(getattr(L, entry)(stream, ptr(h.contiguous()), ptr(nhwc), h.shape[0], h.shape[2], h.shape[3], 1))
    return nhwc


def stack_forward(seq, x, backend, sigma=None, out=None):
    """`seq(x)` for a plain stack by its plan (stack_plan): DnCNN / FDnCNN / FFDNet / IRCNN run without a MIOpen call; layers the
    library does not take run in PyTorch inside the same call under 'hip' and 'hip_f16x3' and raise under 'hip_f16'.  Raises if the
    library or a GPU tensor is missing: no silent fallback to another device.  sigma, out (FFDNet with fused ends): `x` is the
    network's own input, the last layer writes the network's own output `out`."""
    be = BACKENDS[backend]
    ctx = lib_ctx(x, boundary=True)
    plan = stack_plan(seq, backend, ffdnet=sigma is not None)
    if not be.mixes and uncovered(plan):
        raise ValueError("backend='%s': libpnpmri.so does not take %s" % (backend, uncovered(plan)))
    h, nhwc = x, None                                              # h: NCHW tensor, or nhwc: [n][H][W][64] between library layers
    for kind, _, m, *a in plan:
        if kind == 'body':
            nhwc = conv3x3(ctx, be, a[0], nhwc, m, None, a[1], a[3])
        elif kind == 'head':
            nhwc = head(ctx, be, a[0], h, m, a[1])
        elif kind == 'tail':
            h, nhwc = tail(ctx, be, a[0], nhwc, None, m), None
        elif kind == 'ffdnet_head':
            nhwc = ffdnet_head(ctx, be, a[0], h, sigma, m, a[1])
        elif kind == 'ffdnet_tail':
            h, nhwc = ffdnet_tail(ctx, be, a[0], nhwc, m, out), None
        elif kind == 'relayout':
            nhwc = to_nhwc(ctx, a[0], h)
        else:
            if nhwc is not None:
                h, nhwc = nhwc.permute(0, 3, 1, 2), None           # a channels_last NCHW view: PyTorch takes it as it is
            if m is not None:
                h = m(h)
    return h
