"""Whole denoiser forwards on the HIP backends at odd, rectangular and tiny sizes, PER ELEMENT against the float64 oracle of
tests/denoiser_oracle.py: dist[b] = max |got[b] - ref[b]| / max |ref[b]| <= FREEDOM x the float32 CPU forward's own distance, per slice.

Shapes (n, H, W), each the smallest that reaches the edge named:
  A  3 x 41 x 58     odd H, no side a multiple of 8 or 16: ragged last narrow (16 x 8) and wide (16 x 16) tile on both axes; FFDNet's body at
                     21 x 29 after its replicate pad; DRUNet padded to 48 x 64, 6 x 8 -- less than one tile -- at its coarsest scale
  B  3 x 58 x 41     the transpose of A: a swapped H and W shows
  C  1 x 7 x 5       smaller than one tile and than IRCNN's dilation-4 halo; DRUNet reaches 2 x 2, FFDNet runs at 4 x 3
  D  n x 136 x 152   the by-size rule (csrc/conv_plan.h: cp_use_wide) picks the wide f16x3 kernel, its tiles ragged (136 = 8 * 16 + 8); n = 3,
                     for FFDNet (body at 68 x 76) 12; also run with the narrow and the wide kernel forced: bit-equal
  E  1 x 264 x 250   DRUNet: more than 256^2 pixels, so test_split_fn cuts four 160 x 128 windows -- the quadrant path on a rectangle

  (a) every network x {'hip', 'hip_f16x3'} x {A, B, C, D} (DRUNet: E too) against float64; 'hip_f16' at A and B by its own criterion
      (tests/test_gpu_conv_f16.py: norm distance <= 1.25 x that of the float64 emulation of tests/f16_emulation.py)
  (b) the x8 views of IRCNN and DRUNet at A                 (c) FFDNet's `out=` writes stay inside the caller's tensor
  (d) bit-exact invariants at A: slice b alone, cnn_batch, graph replay
  (e) PNP_ADMM_CNC_D / PNP_ADMM_CNC_DnCNN at 218 x 170 with the HIP backends named explicitly

Where a plan has no PyTorch step the forward runs with torch.nn.Conv2d.forward / ConvTranspose2d.forward made to raise.  `pytest -s`
prints the ratio dist / bar of every case and, at the end, the worst per network and backend.  Measured on an MI355X, worst dist / bar
over (a), (b) and (c) (1.0 = at the bar; the PyTorch / MIOpen forward of the same cases: 0.13 .. 0.58):

    network            'hip'    'hip_f16x3'
    ffdnet_gray        0.510    0.389
    dncnn_15           0.701    0.285
    dncnn_gray_blind   0.520    0.306
    fdncnn_gray        0.486    0.310
    ircnn_gray         0.457    0.298
    drunet_gray        0.316    0.275

No case needed the north star's margin; every size that is no multiple of 8 -- A, B, C, E and (e)'s 218 x 170 (relative L2 3e-7 .. 5e-7 from
the oracle loop) -- is inside its bar on both parity backends.  'hip_f16' lies at 0.99 .. 1.02 of its emulation's distance (bar 1.25)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import denoiser_oracle as O
from f16_emulation import emulation
from oracle import admm_oracle as AO
from conftest import rel_l2, weights50

pytestmark = pytest.mark.gpu

PARITY = ('hip', 'hip_f16x3')
ALL = PARITY + ('hip_f16',)
WORST = {}               # (network, backend) -> the largest dist / bar seen


@pytest.fixture(scope='module')
def env():
    import torch
    from pnp_admm_cnc_mri_amd import _lib, denoisers, hip_layers, solvers_pnp
    assert torch.cuda.is_available() and _lib.device_count() >= 1
    yield dict(torch=torch, D=denoisers, HL=hip_layers, S=solvers_pnp, lib=_lib, L=_lib.lib())
    for (name, backend), r in sorted(WORST.items()):
        print('WORST %-17s %-9s dist / bar = %.3f' % (name, backend, r))


def _den(env, name, shape, backend, **kw):
    """the case's network under `backend` on the GPU, and its input there"""
    net, nlm, x, side = O.case(name, shape)
    den = env['D'].Denoiser(name, net, nlm, backend=backend, miopen_find=False, **side, **kw).to('cuda')
    return den, x.cuda()


def _called_size(D, name, H, W):
    """the size DRUNet's module is called with: padded to 16, or the quadrant windows (denoisers.test_split_fn)"""
    if D.family(name) != 'drunet':
        return H, W
    if H * W <= 256 ** 2:
        return -(-H // 16) * 16, -(-W // 16) * 16
    return D._corner_span(H, 32), D._corner_span(W, 32)


def _covered(env, den, x):
    D, HL = env['D'], env['HL']
    return HL.uncovered(D.hip_plan(den.model, den.backend, *_called_size(D, den.name, *x.shape[-2:]))) is None


@contextlib.contextmanager
def _no_pytorch_convolution(torch):
    orig, orig_t = torch.nn.Conv2d.forward, torch.nn.ConvTranspose2d.forward

    def boom(self, inp, *a):
        raise AssertionError('a PyTorch convolution was called')
    torch.nn.Conv2d.forward = torch.nn.ConvTranspose2d.forward = boom
    try:
        yield
    finally:
        torch.nn.Conv2d.forward, torch.nn.ConvTranspose2d.forward = orig, orig_t


@contextlib.contextmanager
def _miopen_deterministic(torch):
    """MIOpen's reproducible mode for the duration of a test (a process-wide flag: restored)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before


def _run(env, den, x, i=0, **kw):
    """den(x, i) -- with every PyTorch convolution made to raise where the plan has no PyTorch step"""
    with _no_pytorch_convolution(env['torch']) if _covered(env, den, x) else contextlib.nullcontext():
        return den(x, i, **kw).clone()


def _north_star(env, name, shape, i, x8):
    """the PyTorch / MIOpen float32 forward of the same case: its dist / bar, for the message of a case above its bar"""
    den, x = _den(env, name, shape, 'torch', x8=x8)
    return O.dist(den(x, i), O.reference(name, shape, i, x8)) / O.bar(name, shape, i, x8)


def _check(env, got, name, shape, backend, i=0, x8=False):
    """(a)'s criterion: every value finite, dist <= FREEDOM x d32 for every slice"""
    ref, bar = O.reference(name, shape, i, x8), O.bar(name, shape, i, x8)
    assert got.dtype == env['torch'].float32 and got.shape == ref.shape and bool(env['torch'].isfinite(got).all())
    ratio = O.dist(got, ref) / bar
    WORST[(name, backend)] = max(WORST.get((name, backend), 0.0), float(ratio.max()))
    print('RATIO %s %s %s i=%d x8=%d: dist / bar = %s' % (name, backend, 'x'.join(map(str, shape)), i, x8, np.array2string(ratio, precision=3)))
    if not (ratio <= 1.0).all():
        b, r, c = O.where_worst(got, ref)
        raise AssertionError('%s %s %s: dist / bar = %s (the PyTorch / MIOpen forward: %s); worst at slice %d, row %d, column %d of %d x %d'
                             % (name, backend, shape, ratio, _north_star(env, name, shape, i, x8), b, r, c, shape[1], shape[2]))


@functools.lru_cache(maxsize=None)
def _emulated(name, shape):
    """the float64 emulation of backend 'hip_f16' (tests/f16_emulation.py) on the CPU, through the same host path as the reference"""
    import torch
    from pnp_admm_cnc_mri_amd import denoisers as D
    den, x = O.cpu_denoiser(name, shape, torch.float64)
    den.model = emulation(D, torch, den.model)
    with torch.no_grad():
        return den(x, 0)


def _check_f16(env, got, name, shape):
    """'hip_f16' is no parity backend; its criterion is the one of test_one_forward_against_the_float64_emulation: as far from the
    float64 forward as the emulation that rounds to half where the backend rounds, within 1.25"""
    ref, emu = O.reference(name, shape), _emulated(name, shape)
    assert got.dtype == env['torch'].float32 and got.shape == ref.shape and bool(env['torch'].isfinite(got).all())
    dY, dE = float((got.cpu().double() - ref).norm()), float((emu - ref).norm())
    print('F16 %s %s: ||hip_f16 - F|| / ||E - F|| = %.3f' % (name, 'x'.join(map(str, shape)), dY / dE))
    assert dE > 0 and dY <= 1.25 * dE, (name, shape, dY, dE)


def _assert_the_wide_kernel_is_chosen(env, name, shape):
    """shape D's precondition, asserted and not skipped on: the wide tiling of the body's tensors has at least as many items as this
    card has compute units (csrc/conv_plan.h: cp_use_wide)"""
    cus = C.c_int()
    env['lib'].check(env['L'].pnp_device_info(0, None, C.byref(cus), None, 0, None, 0))
    H, W = O.body_size(name, shape)
    assert shape[0] * -(-H // 16) * -(-W // 16) >= cus.value > 0, (shape, H, W, cus.value)


# ----------------------------------------------------------------------------------------------
# (a) per element against float64
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', PARITY)
@pytest.mark.parametrize('name,tag', [(n, t) for n in O.NETS for t in O.shapes(n)])
def test_whole_forward_per_element_against_float64(env, name, tag, backend):
    torch, L = env['torch'], env['L']
    shape = O.shapes(name)[tag]
    den, x = _den(env, name, shape, backend)
    if tag != 'D':
        _check(env, _run(env, den, x), name, shape, backend)
        return
    _assert_the_wide_kernel_is_chosen(env, name, shape)
    prev = L.pnp_conv3x3_f16x3_set_variant(-1)                     # by size
    try:
        got = _run(env, den, x)
        _check(env, got, name, shape, backend)
        if _covered(env, den, x):                                  # (MIOpen, in DRUNet under 'hip', promises no bit-equal repeat)
            for variant in (0, 1):                                 # the narrow, then the wide kernel for every dilation-1 layer
                L.pnp_conv3x3_f16x3_set_variant(variant)
                assert torch.equal(_run(env, den, x), got), variant
    finally:
        L.pnp_conv3x3_f16x3_set_variant(prev)


@pytest.mark.parametrize('tag', ['A', 'B'])
@pytest.mark.parametrize('name', O.NETS)
def test_half_precision_backend_keeps_its_own_criterion(env, name, tag):
    shape = O.shapes(name)[tag]
    den, x = _den(env, name, shape, 'hip_f16')
    assert _covered(env, den, x)
    _check_f16(env, _run(env, den, x), name, shape)


# ----------------------------------------------------------------------------------------------
# (b) the x8 views on a rectangle: the kernels see 58 x 41 tensors for the odd modes
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,i', [(n, i) for n, its in O.X8.items() for i in its])
def test_x8_views_on_a_rectangle(env, name, i):
    den, x = _den(env, name, O.A, 'hip_f16x3', x8=True)
    _check(env, _run(env, den, x, i), name, O.A, 'hip_f16x3', i, True)


# ----------------------------------------------------------------------------------------------
# (c) writes stay inside the caller's tensor: FFDNet's last layer does the pixel-shuffle and the crop to odd h, w itself
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [O.A, O.C3], ids=['A', 'C'])
@pytest.mark.parametrize('backend', ['hip_f16x3', 'hip_f16'])
def test_ffdnet_writes_stay_inside_the_callers_tensor(env, backend, shape):
    torch = env['torch']
    name, G = 'ffdnet_gray', 4096
    den, x = _den(env, name, shape, backend, cnn_batch=2)
    assert x.shape[0] == 3
    numel = x.numel()
    buf = torch.full((G + numel + G,), -12345.678, dtype=torch.float32, device='cuda')
    before = buf.clone()
    out = buf[G:G + numel].view(x.shape)
    assert out.is_contiguous() and out.data_ptr() == buf.data_ptr() + 4 * G
    with _no_pytorch_convolution(torch):
        ret = den(x, 0, out=out)
    torch.cuda.synchronize()
    assert ret is out
    for guard in (slice(0, G), slice(G + numel, None)):
        assert torch.equal(buf[guard].view(torch.int32), before[guard].view(torch.int32))
    if backend == 'hip_f16':
        _check_f16(env, out.clone(), name, shape)
    else:
        _check(env, out.clone(), name, shape, backend)


# ----------------------------------------------------------------------------------------------
# (d) bit-exact invariants at shape A
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', ALL)
@pytest.mark.parametrize('name', O.NETS)
def test_a_slice_does_not_depend_on_its_batch(env, name, backend):
    """slice b of the batched forward equals the forward of x[b:b+1]; cnn_batch=2 on three slices equals cnn_batch=3 (denoisers.py: "bit-equal
    per slice on the HIP backends").

    The test runs with torch.backends.cudnn.deterministic set, as tests/test_gpu_pnp.py does: it matters for the one case where MIOpen takes
    part, DRUNet under 'hip' (only its 64-channel blocks and its ends run on libpnpmri.so there; the 128 / 256 / 512-channel blocks and the
    2 x 2 layers are MIOpen's).  MIOpen's default float32 kernels for those layers do not repeat bit for bit -- at 3 x 41 x 58 the SAME call
    twice differs by 5e-7 of the peak, under the plain 'torch' backend as well, and every one of the seven layer shapes does so on its own --
    so no bit-exact statement about such a forward can be tested without its deterministic mode; with it each layer, and the forward, is
    repeatable and independent of the batch (measured on an MI355X: difference 0, a forward of 220 ms instead of 2 ms, which is why the
    product does not set the flag itself).  Where libpnpmri.so runs every layer the flag is read by nothing."""
    torch = env['torch']
    with _miopen_deterministic(torch):
        den, x = _den(env, name, O.A, backend, cnn_batch=3)
        whole = _run(env, den, x)
        for b in range(3):
            assert torch.equal(_run(env, den, x[b:b + 1]), whole[b:b + 1]), b
        den2, _ = _den(env, name, O.A, backend, cnn_batch=2)
        assert torch.equal(_run(env, den2, x), whole)


@pytest.mark.parametrize('backend', ALL)
@pytest.mark.parametrize('name', ['dncnn_15', 'dncnn_gray_blind', 'fdncnn_gray', 'ffdnet_gray', 'drunet_gray'])
def test_graph_replay_equals_the_eager_forward(env, name, backend):
    """graph=True: two replays of the captured forward equal the eager forward -- bit for bit where no MIOpen call is left; DRUNet under
    'hip', where MIOpen runs the layers the float32 kernels do not take, keeps the 1e-5 of test_graph_replay_of_a_forward_equals_the_eager_forward"""
    torch = env['torch']
    den, x = _den(env, name, O.A, backend)
    eager = _run(env, den, x)
    deng, _ = _den(env, name, O.A, backend, graph=True)
    assert deng._graph_ok(x)
    for _ in range(2):
        got = _run(env, deng, x)
        if _covered(env, den, x):
            assert torch.equal(got, eager)
        else:
            assert name == 'drunet_gray' and backend == 'hip'
            assert rel_l2(got.cpu().numpy(), eager.cpu().numpy()) <= 1e-5
    assert deng._graphs


# ----------------------------------------------------------------------------------------------
# (e) the solver entry points off the multiples of 8: 218 x 170, where 'auto' resolves to PyTorch (tests/test_gpu_anysize.py)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', ['hip_f16x3', 'hip'])
@pytest.mark.parametrize('entry', ['cnc_d_ffdnet', 'cnc_dncnn_pair'])
def test_solver_entry_points_at_218_by_170(env, entry, backend, tmp_path):
    """3 iterations on 2 slices with two seeded masks and the contractive fixture weights, against the oracle's per-slice loop driven by
    the same GPU denoiser: relative L2 <= 1e-5, the bar of test_pnp_admm_cnc_d_ffdnet_against_oracle_loop"""
    torch, D, S = env['torch'], env['D'], env['S']
    H, W, B, iters = 218, 170, 2, 3
    masks = np.stack([AO.synthetic_mask(k, H, W) for k in ('random', 'radial')]).astype(np.uint8)
    mid = np.arange(B, dtype=np.int32)
    ys = np.stack([AO.synthetic_problem(b, masks[mid[b]], H, W)[1] for b in range(B)]).astype(np.complex64)
    name = 'ffdnet_gray' if entry == 'cnc_d_ffdnet' else 'dncnn_25'
    sd = weights50(name)
    net, nlm, _ = D.build(name)
    net.load_state_dict(sd)
    den = D.Denoiser(name, net.eval(), nlm, backend=backend).to(torch.device('cuda'))

    def denoise(a, i):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None].cuda()
        return den(t, i)[0, 0].cpu().numpy()
    kw = dict(y=ys, mask_id=mid, model=sd, results=str(tmp_path), cnn_backend=backend, iter_num=iters)
    if entry == 'cnc_d_ffdnet':
        opts = dict(alpha=0.9, lambda1=1.35, reo=0.45, b=0.3)
        out, _ = S.PNP_ADMM_CNC_D(name, masks, None, **kw, **opts)
    else:
        opts = dict(alpha=1.2, lambda1=4, reo=0.45, b=0.3)          # S6:571; the reference loads the first net's file into both (S6:435)
        out, _ = S.PNP_ADMM_CNC_DnCNN('dncnn_25', 'dncnn_15', masks, None, **kw, **opts)
    for b in range(B):
        assert out[b].shape == (H, W) and np.isfinite(out[b]).all()
        ref = AO.pnp_admm_cnc(ys[b].astype(np.complex128), masks[mid[b]], denoise, iters, opts['alpha'], opts['lambda1'], opts['reo'], opts['b'])
        err = rel_l2(out[b], ref)
        print('SOLVER %s %s slice %d: rel-L2 %.3g' % (entry, backend, b, err))
        assert err <= 1e-5, (b, err)
