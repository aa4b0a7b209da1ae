"""`Denoiser(backend='hip_f16')` without a GPU: the C ABI of the half-precision layers (header, binding, exported symbols, argument errors
as codes before any HIP call), the Python contract (construction, what it refuses, `auto_backend` untouched), and the compiled gfx950 ISA
of the new translation units (registers, LDS, scratch, matrix instructions, the weight DMA's order) -- hipcc cross-compiles without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT
from pnp_admm_cnc_mri_amd import _lib
from pnp_admm_cnc_mri_amd import denoisers as D
from pnp_admm_cnc_mri_amd import hip_layers as HL

HEADER = os.path.join(ROOT, 'include', 'pnp_mri.h')
NEW = ['pnp_conv3x3_nhwc_f16', 'pnp_conv3x3_pack_f16', 'pnp_conv3x3_head_nhwc_f16', 'pnp_ffdnet_head_nhwc_f16', 'pnp_conv3x3_tail_nchw_f16',
       'pnp_ffdnet_tail_f16', 'pnp_conv2x2s2_nhwc_f16', 'pnp_convT2x2s2_nhwc_f16', 'pnp_conv2x2_pack_f16']
E_ARG = -1


def test_header_binding_and_exports_agree_on_the_new_entry_points():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(pnp_[A-Za-z0-9_]+)\s*\(', src))
    L = _lib.lib()
    for n in NEW:
        assert n in declared and n in _lib.SIGNATURES and hasattr(L, n), n
    # additive: the ABI number the existing tests pin is unchanged, half tensors travel as void*, the header stays C99 (test_abi_cpu builds it)
    assert L.pnp_abi_version() == 13 and int(re.search(r'#define PNP_ABI_VERSION\s+(\d+)', src).group(1)) == 13
    assert 'added after abi 13, additive' in open(HEADER).read().lower().replace('\n', ' ').replace(' * ', ' ')
    proto = re.search(r'int pnp_conv3x3_nhwc_f16\((.*?)\);', src, flags=re.S).group(1)
    assert 'const void* x_dev' in proto and 'void* y_dev' in proto and '_Float16' not in src and '__half' not in src
    for m, v in (('PNP_F16_X_F32', 1), ('PNP_F16_SKIP_F32', 2), ('PNP_F16_Y_F32', 4)):
        assert int(re.search(r'#define %s\s+(\d+)' % m, src).group(1)) == v
        assert (HL.F16_X_F32, HL.F16_SKIP_F32, HL.F16_Y_F32) == (1, 2, 4)


def test_argument_errors_come_back_as_codes_without_a_device():
    """validated before any HIP call: this passes on a machine with no GPU.  The pointers are never dereferenced."""
    L = _lib.lib()
    p = C.c_void_p(0x1000)
    q = C.c_void_p(0x2000)
    r = C.c_void_p(0x3000)
    msg = lambda: L.pnp_last_error().decode()
    conv = L.pnp_conv3x3_nhwc_f16
    assert conv(None, None, q, None, None, r, 1, 64, 8, 8, 0, 1, 0) == E_ARG and 'null' in msg()
    assert conv(None, p, None, None, None, r, 1, 64, 8, 8, 0, 1, 0) == E_ARG and 'null' in msg()
    assert conv(None, p, q, None, None, None, 1, 64, 8, 8, 0, 1, 0) == E_ARG and 'null' in msg()
    for ch in (0, 32, 96, 100, 1088):
        assert conv(None, p, q, None, None, r, 1, ch, 8, 8, 0, 1, 0) == E_ARG and 'multiple of 64' in msg(), ch
    assert conv(None, p, q, None, None, r, 1, 128, 8, 8, 0, 2, 0) == E_ARG and 'dilation' in msg()       # a dilation above 1 at C > 64
    assert conv(None, p, q, None, None, r, 1, 64, 8, 8, 0, 5, 0) == E_ARG and 'dilation' in msg()
    assert conv(None, p, q, None, None, r, 1, 64, 8, 8, 0, 0, 0) == E_ARG
    assert conv(None, p, q, None, None, r, 1, 64, 8, 8, 0, 1, 8) == E_ARG and 'fmt' in msg()
    assert conv(None, p, q, None, None, r, 0, 64, 8, 8, 0, 1, 0) == E_ARG
    assert conv(None, p, q, None, None, p, 1, 64, 8, 8, 0, 1, 0) == E_ARG and 'alias' in msg()
    assert conv(None, p, q, None, r, r, 1, 64, 8, 8, 0, 1, 0) == E_ARG and 'alias' in msg()
    # the 2^31 byte bound on one image as a float32 tensor: 2897 x 2897 x 64 x 4 bytes exceeds it (2896 x 2896 would pass and go on to a launch,
    # which a test without a device cannot make); at C = 1024, 725 x 725 exceeds it
    assert conv(None, p, q, None, None, r, 1, 64, 2897, 2897, 0, 1, 0) == E_ARG and '2 GiB' in msg()
    assert conv(None, p, q, None, None, r, 1, 1024, 725, 725, 0, 1, 0) == E_ARG and '2 GiB' in msg()
    assert L.pnp_conv3x3_pack_f16(None, None, q, 64) == E_ARG and L.pnp_conv3x3_pack_f16(None, p, p, 64) == E_ARG
    assert L.pnp_conv3x3_pack_f16(None, p, q, 96) == E_ARG and 'multiple of 64' in msg()
    assert L.pnp_conv3x3_head_nhwc_f16(None, None, q, None, r, 1, 1, 8, 8, 1) == E_ARG and 'null' in msg()
    assert L.pnp_conv3x3_head_nhwc_f16(None, p, q, None, r, 1, 9, 8, 8, 1) == E_ARG and 'cin' in msg()
    assert L.pnp_conv3x3_head_nhwc_f16(None, p, q, None, r, 1, 1, 2897, 2897, 1) == E_ARG and '2 GiB' in msg()
    assert L.pnp_ffdnet_head_nhwc_f16(None, p, None, 0, q, None, r, 1, 8, 8, 1) == E_ARG and 'null' in msg()
    assert L.pnp_ffdnet_head_nhwc_f16(None, p, q, 0, q, None, r, 1, 0, 8, 1) == E_ARG
    assert L.pnp_ffdnet_head_nhwc_f16(None, p, q, 0, q, None, r, 1, 5794, 5794, 1) == E_ARG and '2 GiB' in msg()
    assert L.pnp_conv3x3_tail_nchw_f16(None, p, None, None, None, r, 1, 1, 8, 8) == E_ARG and 'null' in msg()
    assert L.pnp_conv3x3_tail_nchw_f16(None, p, None, q, None, r, 1, 5, 8, 8) == E_ARG and 'cout' in msg()
    assert L.pnp_conv3x3_tail_nchw_f16(None, p, None, q, None, r, 1, 1, 2897, 2897) == E_ARG and '2 GiB' in msg()
    assert L.pnp_conv3x3_tail_nchw_f16(None, p, r, q, None, r, 1, 1, 8, 8) == E_ARG and 'alias' in msg()
    assert L.pnp_ffdnet_tail_f16(None, None, q, None, r, 1, 8, 8) == E_ARG and L.pnp_ffdnet_tail_f16(None, p, q, None, r, 1, 8, 0) == E_ARG
    assert L.pnp_ffdnet_tail_f16(None, p, q, None, r, 1, 5794, 5794) == E_ARG and '2 GiB' in msg()
    for fn, up in ((L.pnp_conv2x2s2_nhwc_f16, 0), (L.pnp_convT2x2s2_nhwc_f16, 1)):
        for y_f32 in (0, 1):
            assert fn(None, None, None, q, r, 1, 128, 8, 8, y_f32) == E_ARG and 'null' in msg()
            assert fn(None, p, None, q, r, 1, 96, 8, 8, y_f32) == E_ARG and 'multiple of' in msg()
            assert fn(None, p, None, q, r, 1, 1088, 8, 8, y_f32) == E_ARG
            assert fn(None, p, None, q, p, 1, 128, 8, 8, y_f32) == E_ARG and 'alias' in msg()
            assert fn(None, p, None, q, r, 1, 128, 2048, 2048, y_f32) == E_ARG and '2 GiB' in msg()
    assert L.pnp_convT2x2s2_nhwc_f16(None, p, None, q, r, 1, 64, 8, 8, 0) == E_ARG and '128' in msg()
    assert L.pnp_conv2x2s2_nhwc_f16(None, p, None, q, r, 1, 64, 7, 8, 0) == E_ARG and 'even' in msg()
    # the bound keeps 16 rows to spare, so that the byte offset of a halo or overhang row cannot wrap around 2^32 back into the buffer: an
    # image of 8 rows whose float32 size alone is below 2 GiB (8 x 1 040 000 x 64 x 4 = 2.13e9) is refused, 24 rows of it are 6.4e9
    assert conv(None, p, q, None, None, r, 1, 64, 8, 1040000, 0, 1, 0) == E_ARG and '16 rows' in msg()
    assert L.pnp_conv3x3_tail_nchw_f16(None, p, None, q, None, r, 1, 1, 8, 1040000) == E_ARG and '16 rows' in msg()
    assert L.pnp_conv2x2_pack_f16(None, None, q, 64, 0) == E_ARG and L.pnp_conv2x2_pack_f16(None, p, q, 64, 1) == E_ARG
    with pytest.raises(_lib.PnpError):
        _lib.check(conv(None, p, q, None, None, r, 1, 100, 8, 8, 0, 1, 0))


def _den(name, backend, **kw):
    net, nlm, sched = D.build(name)
    net.load_state_dict(D.seeded_state_dict(net, 3))
    sig = torch.tensor([20.0 / 255]) if sched else None
    noises = torch.zeros(16, 16).numpy() if D.family(name) == 'fdncnn' else None
    return D.Denoiser(name, net.eval(), nlm, sigmas=sig, noises=noises, backend=backend, **kw)


@pytest.mark.parametrize('name', ['ffdnet_gray', 'dncnn_25', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray', 'dncnn_gray_blind'])
def test_the_backend_constructs_for_every_family_and_refuses_what_the_others_refuse(name):
    den = _den(name, 'hip_f16')
    assert den.backend == 'hip_f16' and den.model.backend == 'hip_f16'
    assert den.cnn_batch == _den(name, 'hip_f16x3').cnn_batch          # the same defaults as f16x3
    for dt in ('fp16', 'bf16'):
        with pytest.raises(ValueError, match='float32 only'):
            _den(name, 'hip_f16', cnn_dtype=dt)
    assert _den(name, 'hip_f16', cnn_dtype='fp32').backend == 'hip_f16'
    with pytest.raises(RuntimeError, match='CUDA'):                    # a CPU tensor: no fallback to PyTorch layers
        den(torch.rand(1, 1, 16, 16), 0)
    assert 'hip_f16' in D.HIP_BACKENDS and _den(name, 'hip_f16', graph=True).graph


def test_auto_backend_answers_as_before_and_never_picks_the_half_backend():
    for name in ('ffdnet_gray', 'dncnn_25', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray'):
        net, _, _ = D.build(name)
        be, why = D.auto_backend(net)
        assert be in ('torch', 'hip_f16x3'), (name, be)
        if not torch.cuda.is_available():
            assert (be, why) == ('torch', 'no HIP device')
        assert D.auto_backend(net, cnn_dtype='fp16') == ('torch', 'cnn_dtype=fp16 is a PyTorch autocast mode')
        assert D.auto_backend(net, shape=(250, 256))[0] == 'torch'
    with pytest.raises(ValueError, match="'hip_f16'"):
        _den('ffdnet_gray', 'hip_f17')


def test_a_network_with_a_layer_the_library_does_not_take_raises_at_construction():
    """no mixing with PyTorch layers, no silent fallback: the constructor names the layer"""
    net = D.DnCNN(nb=5)
    net.model[4] = torch.nn.Conv2d(64, 64, 5, 1, 2)
    with pytest.raises(ValueError, match=r'layer 4: Conv2d\(64, 64, kernel_size=\(5, 5\)'):
        D.Denoiser('dncnn_15', net, 15, backend='hip_f16')
    D.Denoiser('dncnn_15', net, 15, backend='hip_f16x3')               # the other HIP backends mix: unchanged
    net = D.DnCNN(nb=5)
    net.model[3] = torch.nn.Tanh()
    with pytest.raises(ValueError, match='layer 3: Tanh'):
        D.Denoiser('dncnn_15', net, 15, backend='hip_f16')
    net = D.FFDNet(in_nc=3, out_nc=3)                                  # colour FFDNet: 13 input channels
    with pytest.raises(ValueError, match=r'layer 0: Conv2d\(13, 64'):
        D.Denoiser('ffdnet_color', net, 15, backend='hip_f16')
    net = D.IRCNN()
    net.model[4] = torch.nn.Conv2d(64, 64, 3, 1, 5, dilation=5)
    with pytest.raises(ValueError, match='dilation=\\(5, 5\\)'):
        D.Denoiser('ircnn_gray', net, 15 / 255., sigmas=torch.tensor([0.1]), backend='hip_f16')
    net = D.UNetRes(nc=(64, 128, 256, 500))
    with pytest.raises(ValueError, match='hip_f16'):
        D.Denoiser('drunet_gray', net, 15 / 255., sigmas=torch.tensor([0.1]), backend='hip_f16')
    net = D.UNetRes()
    net.m_body[1].res[0] = torch.nn.Conv2d(512, 512, 3, 1, 1, bias=False, groups=2)
    with pytest.raises(ValueError, match=r'm_body\.1'):
        D.Denoiser('drunet_gray', net, 15 / 255., sigmas=torch.tensor([0.1]), backend='hip_f16')
    assert HL.f16_uncovered_stack(D.build('ffdnet_gray')[0].model) is None and D.UNetRes().hip_covers(backend='hip_f16')
    assert not D.UNetRes().hip_covers(backend='hip') and D.UNetRes().hip_covers(backend='hip_f16x3')


# ----------------------------------------------------------------------------------------------
# the compiled ISA of the new translation units
# ----------------------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, 'pnp_admm_cnc_mri_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=off', '-fno-slp-vectorize']     # = csrc/Makefile for these units

import importlib.util
_spec = importlib.util.spec_from_file_location('isa_scan', os.path.join(CSRC, 'tools', 'isa_scan.py'))
isa_scan = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_scan)


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    d = tmp_path_factory.mktemp('gfx950_asm_f16')
    out = {}
    for src in ('kernels_conv_f16.hip', 'kernels_pix2x2_f16.hip', 'kernels_pix2x2_f16x3.hip'):
        o = str(d / (src[:-4] + '.s'))
        r = subprocess.run([HIPCC] + FLAGS + ['--cuda-device-only', '-S', os.path.join(CSRC, src), '-o', o], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=CSRC)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        out[src] = open(o).read()
    return out


def _is_dma(x):
    return x.startswith('buffer_load') and x.split(';')[0].rstrip().endswith(' lds')


def test_the_makefile_builds_and_scans_the_new_units():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    rule = [l for l in mk.splitlines() if l.rstrip().endswith('CXXFLAGS += -fno-slp-vectorize')]
    assert len(rule) == 1
    for u in ('kernels_conv_f16', 'kernels_pix2x2_f16'):
        assert u + '.hip' in srcs and u + '.o' in rule[0].split(':')[0].split() and u + '.s' in rule[0].split(':')[0].split()
    assert 'f16_common.h' in mk


def test_conv_f16_kernel_resources(asm):
    """k_conv3x3_f16<dilation, float32 x>: no scratch; THREE workgroups per compute unit at dilation 1 (3 x 51 200 bytes of LDS, at most 168
    registers), TWO at dilations 2, 3, 4 (54 784 / 65 664 / 77 824 bytes, at most 256 registers: the f16x3 kernel's tile alone is 98 .. 137 KiB
    there, one workgroup per unit); the occupancy the compiler reports is 3 waves per SIMD at dilation 1 and 2 at dilations 2 .. 4.
    Every matrix instruction is the half form with float32 accumulation, 16 per tap (2 K steps x 2 M tiles x 4 N tiles, one product each --
    the f16x3 kernel has 48), nine unrolled taps, two instances of the chunk code whose first starts its 8 accumulators from a constant 0;
    two LDS-DMAs per thread and tap (8 KiB per tap) + the first tap's."""
    ks = {n: k for n, k in isa_scan.kernels_of(asm['kernels_conv_f16.hip']).items() if 'k_conv3x3_f16' in n}
    assert len(ks) == 8, sorted(ks)
    lds = {1: 51200, 2: 54784, 3: 65664, 4: 77824}
    for n, k in ks.items():
        i = k['info']
        dil = int(n.split('k_conv3x3_f16ILi')[1][0])
        assert i['ScratchSize'] == 0, (n, i)
        wps = 3 if dil == 1 else 2
        assert i['LDSByteSize'] == lds[dil] and wps * i['LDSByteSize'] <= 160 * 1024, (n, i)
        assert i['NumVgprs'] + i['NumAgprs'] <= (168 if wps == 3 else 256) and i['Occupancy'] == wps, (n, i)
        mf = [x for x in k['body'] if x.startswith('v_mfma')]
        assert len(mf) == 2 * 9 * 16 and all(x.startswith('v_mfma_f32_16x16x32_f16') for x in mf), (n, len(mf))
        assert sum(1 for x in mf if x.split(';')[0].rstrip().endswith(', 0')) == 8, n
        assert sum(1 for x in k['body'] if _is_dma(x)) == 2 + 2 * 18, n
        assert not any(x.startswith('scratch_') for x in k['body']), n
    assert not isa_scan.scan_text(asm['kernels_conv_f16.hip'])[0]                # the build's own scan: no store hazard


def test_conv_f16_weight_dma_is_older_than_the_loads_counted_behind_it(asm):
    """the per-tap `s_waitcnt vmcnt(k)` leaves the k loads of an input-prefetch piece in flight and is right only while the tap's two LDS-DMAs
    were issued BEFORE them; the walk of tools/isa_scan.py (groups of two, back edges followed) proves it on the compiled ISA of every
    instance, and that no wave ends with a DMA in flight.  The walk does tell a wrong order apart:"""
    dv = isa_scan.dma_order_violations
    Dm, Ld = 'buffer_load_dwordx4 v1, s[0:3], s5 offen lds', 'buffer_load_dwordx4 v[2:5], v1, s[0:3], 0 offen'
    tail = [Dm] * 2 + ['s_waitcnt vmcnt(0)', 's_barrier', 's_endpgm']
    assert not dv([Dm] * 2 + [Ld, 's_waitcnt vmcnt(1)', 's_barrier'] + tail, group=2)
    assert dv([Dm, Ld, Dm, 's_waitcnt vmcnt(1)', 's_barrier'] + tail, group=2)
    ks = {n: k for n, k in isa_scan.kernels_of(asm['kernels_conv_f16.hip']).items() if 'k_conv3x3_f16' in n}
    assert len(ks) == 8
    for n, k in ks.items():
        v = dv(k['body'], group=2, labels=k['labels'])
        assert not v, (n, v[:3])


def test_no_lds_access_is_outstanding_at_any_barrier_of_the_new_kernels(asm):
    """The kernels' barriers inside the tap / chunk loops are raw `s_barrier`s (a __syncthreads() would drain the weight DMA), and a raw barrier
    waits for no counter: a `ds_read` of the operand tile still in flight when its wave passes the barrier races with the other waves' writes
    of the next tile behind it.  The source puts `s_waitcnt lgkmcnt(0)` in front of every such barrier and a sched_barrier behind each block
    of matrix instructions (hipcc otherwise moves a chunk's reads and MFMAs behind the next chunk's barrier); this walk over the compiled
    ISA (tools/isa_scan.py, also part of `make`) proves it for every barrier of every new kernel, back edges included -- and of k_pix2x2_h3
    (kernels_pix2x2_f16x3.hip), which is the same body (pix2x2_body.h) as k_pix2x2_f16."""
    f = isa_scan.lds_pending_at_barriers
    rd = 'ds_read_b128 v[1:4], v0'
    assert f([rd, 's_waitcnt lgkmcnt(1)', rd, 's_waitcnt vmcnt(4)', 's_barrier'])                   # the shape the 2 x 2 kernel first compiled to
    assert f(['ds_write_b128 v0, v[1:4]', 's_barrier'])
    assert not f([rd, rd, 's_waitcnt vmcnt(4) lgkmcnt(0)', 's_barrier', rd, 's_waitcnt lgkmcnt(0)', 's_barrier'])
    assert not f([rd, 's_waitcnt lgkmcnt(0)', 's_load_dwordx2 s[0:1], s[2:3], 0x0', 's_barrier'])   # scalar loads touch no LDS
    assert f(['s_load_dwordx2 s[0:1], s[2:3], 0x0', rd, 's_waitcnt lgkmcnt(1)', 's_barrier'])       # out-of-order scalar return: only 0 counts
    loop = ['s_waitcnt lgkmcnt(0)', 's_barrier', rd, 's_cbranch_scc1 .LBB0_1']
    assert not f(loop + ['s_endpgm'], {'.LBB0_1': 0}) and f(loop[1:] + ['s_endpgm'], {'.LBB0_1': 0})
    n_barriers = 0
    for src in ('kernels_conv_f16.hip', 'kernels_pix2x2_f16.hip', 'kernels_pix2x2_f16x3.hip'):
        for n, k in isa_scan.kernels_of(asm[src]).items():
            n_barriers += sum(1 for x in k['body'] if x.startswith('s_barrier'))
            bad = f(k['body'], k['labels'])
            assert not bad, (n, bad[:3])
    assert n_barriers >= 8 * 22 + 4 * 5 + 4 + 4 * 5                     # 3 x 3 instances, 2 x 2 instances, the last-layer kernel, the split-half 2 x 2 instances: really walked


def test_the_recorded_l1_outputs_of_the_trained_ffdnet_are_the_oracle_loops():
    """tests/golden/pnp_l1_ffdnet_trained_it.npz (PNP_ADMM_L1_D of the unmodified reference script, trained FFDNet, 2 / 5 / 10 iterations at the
    S3 preset; recorded by profiles/experiments/record_l1_ffdnet_trained_it.py) is anchored here: the oracle's loop driven by the float32
    network on the CPU reproduces all three arrays BIT FOR BIT -- as it does the reference's CNC outputs at those run lengths."""
    import json
    import numpy as np
    from conftest import GOLD, weights_trained
    from oracle import admm_oracle as O
    d = np.load(os.path.join(GOLD, 'inputs_set1_05.npz'))
    mask = np.unpackbits(d['Q_Random30_packbits'])[:65536].reshape(256, 256).astype(np.float64)
    y = O.synthesize(O.requantise(d['gray_u8']), mask, d['noises_c128'] * 3.0)
    net, nlm, _ = D.build('ffdnet_gray')
    net.load_state_dict(weights_trained('ffdnet_gray'), strict=True)
    den = D.Denoiser('ffdnet_gray', net.eval(), nlm, backend='torch', channels_last=False, miopen_find=False)
    denoise = lambda a, i: den(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None], i)[0, 0].numpy()
    gold = np.load(os.path.join(GOLD, 'pnp_l1_ffdnet_trained_it.npz'))
    reo = json.load(open(os.path.join(GOLD, 'pnp_known.json')))['known50']['trained_l1_d_ffdnet_gray_opts']['reo']
    assert sorted(gold.files) == ['trained_l1_d_ffdnet_gray_it%d' % n for n in (10, 2, 5)]
    for n_it in (2, 5, 10):
        x = O.pnp_admm_l1(y, mask, denoise, n_it, reo)
        assert np.array_equal(np.asarray(x, np.float32), gold['trained_l1_d_ffdnet_gray_it%d' % n_it]), n_it


def test_pix2x2_and_end_layer_kernel_resources(asm):
    """k_pix2x2_f16 (four instances): two workgroups per compute unit (51 200 bytes of LDS, <= 256 registers, no scratch), 16 half-precision
    matrix instructions per chunk in two unrolled chunks, two DMAs per thread and chunk in an order the counted wait relies on; the first /
    last layer kernels and the two packing kernels: no scratch, two workgroups per unit for the persistent tail."""
    ks = {n: k for n, k in isa_scan.kernels_of(asm['kernels_pix2x2_f16.hip']).items() if 'k_pix2x2_f16' in n}
    assert len(ks) == 4, sorted(ks)
    for n, k in ks.items():
        i = k['info']
        assert i['ScratchSize'] == 0 and i['NumVgprs'] + i['NumAgprs'] <= 256 and i['LDSByteSize'] == 51200 and i['Occupancy'] >= 2, (n, i)
        mf = [x for x in k['body'] if x.startswith('v_mfma')]
        assert len(mf) == 32 and all(x.startswith('v_mfma_f32_16x16x32_f16') for x in mf), (n, len(mf))
        assert sum(1 for x in k['body'] if _is_dma(x)) == 6, n
        v = isa_scan.dma_order_violations(k['body'], group=2, labels=k['labels'])
        assert not v, (n, v[:3])
    assert not isa_scan.scan_text(asm['kernels_pix2x2_f16.hip'])[0]
    allk = dict(isa_scan.kernels_of(asm['kernels_conv_f16.hip']), **isa_scan.kernels_of(asm['kernels_pix2x2_f16.hip']))
    assert len(allk) == 8 + 4 + 4, sorted(allk)                        # + head, tail and pack in one unit, the pack of the other
    for n, k in allk.items():
        assert k['info']['ScratchSize'] == 0, (n, k['info'])
    tail = [k for n, k in allk.items() if 'k_conv3x3_tail_f16' in n]
    assert len(tail) == 1 and tail[0]['info']['NumVgprs'] <= 256 and 2 * tail[0]['info']['LDSByteSize'] <= 160 * 1024
    assert sum(1 for x in tail[0]['body'] if x.startswith('v_mfma_f32_16x16x32_f16')) == 36
