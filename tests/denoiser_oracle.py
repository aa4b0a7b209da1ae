"""The float64 oracle of a WHOLE denoiser forward, per element (tests/test_denoiser_oracle_cpu.py, tests/test_gpu_denoiser_shapes.py).  Not a
test module; CPU only: nothing here touches a GPU.

  case(name, shape, seed)        the seeded network, the input and the side inputs of one case
  reference(name, shape, i, x8)  the forward in float64 on the CPU, through the project's own host path (Denoiser: DRUNet's pad to 16
                                 and quadrant split, the x8 views, FDnCNN's noise map) with every layer in PyTorch
  d32(name, shape, i, x8)        per slice, the distance of the SAME forward in float32 on the CPU from that reference
  dist(got, ref)[b]              max |got[b] - ref[b]| / max |ref[b]|: one number per slice, no averaging over pixels
  bar[b]                         FREEDOM x d32[b]: a float32 implementation that sums in another order may be FREEDOM times as far from
                                 the float64 result as PyTorch's float32 CPU kernels are (tests/test_gpu_wavelet.py, tests/param_space_oracle.py);
                                 the reference is double precision, so no floor is needed

Shapes are (n, H, W); the tags are those of tests/test_gpu_denoiser_shapes.py."""
import copy
import functools
import hashlib

import numpy as np
import torch

from pnp_admm_cnc_mri_amd import denoisers as D

FREEDOM = 4.0            # another order of the sums (tests/test_gpu_wavelet.py FREEDOM, tests/param_space_oracle.py FREEDOM)
SEED = 11
NETS = ('ffdnet_gray', 'dncnn_15', 'dncnn_gray_blind', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray')
SIGMAS = (30.0 / 255, 20.0 / 255, 10.0 / 255)
# the schedule handed to Denoiser: SIGMAS, repeated so that the x8 cases' iterations 3 .. 7 have an entry too (sigmas[i] = SIGMAS[i % 3])
SCHEDULE = SIGMAS * 3

A, B, C = (3, 41, 58), (3, 58, 41), (1, 7, 5)
E = (1, 264, 250)
# The weights' seed per case.  With seed 11 the 35 output pixels of shape C peak at 0.039 (FFDNet) and 0.046 (FDnCNN): below the 0.05 that
# tests/test_denoiser_oracle_cpu.py asks of every case, so that a bar relative to the peak means something.  Seeds 19 and 17 give peaks of
# 0.108 and 0.141, and 0.068 .. 0.085 for the three slices of C3 (chosen from the float64 reference alone, before any kernel ran).
SEEDS = {('ffdnet_gray', 7, 5): 19, ('fdncnn_gray', 7, 5): 17}
C3 = (3, 7, 5)           # FFDNet only: three slices of shape C's size, for the test of writes through `out=` with cnn_batch=2


def seed_of(name, shape):
    return SEEDS.get((name, shape[1], shape[2]), SEED)


def shape_d(name):
    """shape D: 136 x 152; 3 slices where the body runs at full size, 12 for FFDNet, whose body runs at 68 x 76"""
    return (12 if D.family(name) == 'ffdnet' else 3, 136, 152)


def shapes(name):
    """{tag: (n, H, W)} of the shapes `name` runs at"""
    s = {'A': A, 'B': B, 'C': C, 'D': shape_d(name)}
    if D.family(name) == 'drunet':
        s['E'] = E
    return s


# the x8 cases, at shape A: IRCNN walks all eight views; DRUNet a rotation (1), the two modes that are each other's inverse (3, 5) and a flip (6)
X8 = {'ircnn_gray': (0, 1, 2, 3, 4, 5, 6, 7), 'drunet_gray': (1, 3, 5, 6)}


def cases():
    """every (name, shape, i, x8) the GPU tests hold to a bar of this module"""
    out = [(name, shp, 0, False) for name in NETS for shp in shapes(name).values()]
    return out + [(name, A, i, True) for name, its in X8.items() for i in its] + [('ffdnet_gray', C3, 0, False)]


def body_size(name, shape):
    """(H, W) of the tensors the network's full-resolution 64-channel layers see for one window: FFDNet's half size after its replicate
    pad, DRUNet's pad to 16 (no quadrant split below 256 x 256 pixels), the slice's own size otherwise"""
    _, H, W = shape
    fam = D.family(name)
    if fam == 'ffdnet':
        return (H + 1) // 2, (W + 1) // 2
    if fam == 'drunet':
        assert H * W <= 256 ** 2
        return -(-H // 16) * 16, -(-W // 16) * 16
    return H, W


def _key(*parts):
    return int.from_bytes(hashlib.sha256(':'.join(str(p) for p in parts).encode()).digest()[:8], 'little') >> 1


def noises(H, W):
    """FDnCNN's H x W complex noise, as test_hip_backend_matches_the_pytorch_forward builds it"""
    return (np.random.default_rng(3).standard_normal((H, W)) + 1j * np.random.default_rng(4).standard_normal((H, W))) * 5


def case(name, shape, seed=None):
    """-> (net, noise_level_model, x, side): D.build(name) with D.seeded_state_dict(net, seed) in eval mode; x = torch.rand [n, 1, H, W]
    float32 from a CPU generator keyed by (name, shape); side = the keywords Denoiser takes besides: `sigmas` for the families with a
    sigma schedule, `noises` for FDnCNN.  A fresh network per call: callers may move or retype it."""
    n, H, W = shape
    net, nlm, scheduled = D.build(name)
    net.load_state_dict(D.seeded_state_dict(net, seed_of(name, shape) if seed is None else seed))
    g = torch.Generator().manual_seed(_key(name, n, H, W))
    x = torch.rand((n, 1, H, W), generator=g, dtype=torch.float32)
    side = {}
    if scheduled:
        side['sigmas'] = torch.tensor(SCHEDULE)
    if D.family(name) == 'fdncnn':
        side['noises'] = noises(H, W)
    return net.eval(), nlm, x, side


def cpu_denoiser(name, shape, dtype, x8=False, seed=None):
    """-> (Denoiser on the CPU with a deep copy of the case's network in `dtype` and every layer in PyTorch, the input in `dtype`)"""
    net, nlm, x, side = case(name, shape, seed)
    net = copy.deepcopy(net).to(dtype)
    for m in [net] + list(net.modules()):
        if hasattr(m, 'backend'):
            m.backend = 'torch'
    return D.Denoiser(name, net, nlm, x8=x8, backend='torch', channels_last=False, miopen_find=False, **side), x.to(dtype)


def _cpu_forward(name, shape, i, x8, seed, dtype):
    den, x = cpu_denoiser(name, shape, dtype, x8, seed)
    out = den(x, i)
    assert out.dtype == dtype and out.shape == x.shape
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, shape, i, x8, seed):
    with torch.no_grad():
        return _cpu_forward(name, shape, i, x8, seed, torch.float64)


def reference(name, shape, i=0, x8=False, seed=None):
    """the float64 forward on the CPU, [n, 1, H, W]; cached per process: do not write to it"""
    return _reference(name, tuple(shape), int(i), bool(x8), seed_of(name, shape) if seed is None else seed)


def dist(got, ref):
    """[n] float64: max |got[b] - ref[b]| / max |ref[b]|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape
    nb = ref.shape[0]
    return ((got - ref).abs().reshape(nb, -1).amax(1) / ref.abs().reshape(nb, -1).amax(1)).numpy()


@functools.lru_cache(maxsize=None)
def _d32(name, shape, i, x8, seed):
    with torch.no_grad():
        return dist(_cpu_forward(name, shape, i, x8, seed, torch.float32), reference(name, shape, i, x8, seed))


def d32(name, shape, i=0, x8=False, seed=None):
    """[n] float64: the distance of the float32 CPU forward from `reference`, per slice; cached per process"""
    return _d32(name, tuple(shape), int(i), bool(x8), seed_of(name, shape) if seed is None else seed).copy()


def bar(name, shape, i=0, x8=False, seed=None):
    """[n]: FREEDOM x d32, as a multiple of max |ref[b]|"""
    return FREEDOM * d32(name, shape, i, x8, seed)


def where_worst(got, ref):
    """(slice, row, column) of the largest |got - ref|: for the message of a failing comparison"""
    e = (got.detach().cpu().double() - ref.detach().cpu().double()).abs()[:, 0]
    k = int(e.reshape(-1).argmax())
    H, W = e.shape[-2:]
    return k // (H * W), (k // W) % H, k % W
