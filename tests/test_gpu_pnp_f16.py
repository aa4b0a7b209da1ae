"""The PnP entry points with `cnn_backend='hip_f16'` (half precision between the denoiser's layers).

This backend is a throughput mode: it does not meet the float32 backends' 1e-5 bar and is not asked to.  What it is asked:

  * trained denoisers, 2 / 5 / 10 iterations, against the UNMODIFIED reference's outputs (tests/golden/pnp50_set1_05.npz; PNP_ADMM_L1_D with
    the trained FFDNet at those run lengths: tests/golden/pnp_l1_ffdnet_trained_it.npz, recorded from the same unmodified script at its
    S3 preset): rel-L2 <= 2 x the distance of the ORACLE's loop driven by the float64 emulation E of the backend's arithmetic
    (tests/f16_emulation.py) from the same golden, computed here on the CPU.  Two realisations of half rounding (float32 / float64
    accumulation) differed by at most a factor 1.17 up to 10 iterations on the CPU: hence 2.  PSNR within 0.01 dB of the golden's;
  * the contractive fixtures at the presets' own 50 iterations, all five families: PSNR within 0.01 dB of the golden's;
  * a slice's result does not depend on how the batch is cut (B = 9 against 4 + 5, bit for bit).
"""
import copy
import json
import os

import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import rel_l2, GOLD
from f16_emulation import emulation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env():
    import torch
    from pnp_admm_cnc_mri_amd import solvers_pnp, denoisers, _lib
    assert _lib.device_count() >= 1 and torch.cuda.is_available()
    known = json.load(open(os.path.join(GOLD, 'pnp_known.json')))['known50']
    gold = dict(np.load(os.path.join(GOLD, 'pnp50_set1_05.npz')))
    gold.update(np.load(os.path.join(GOLD, 'pnp_l1_ffdnet_trained_it.npz')))
    return dict(torch=torch, S=solvers_pnp, D=denoisers, known50=known, gold50=gold)


def _psnr(x, gt):
    return O.calculate_psnr(np.round(x.astype(np.float64) * 255), gt)


def _emulated_denoiser(env, name, sd):
    """denoise(a, i) of the oracle's loops: the float64 emulation E of backend 'hip_f16' on the CPU, float32 in and out"""
    torch, D = env['torch'], env['D']
    net, nlm, _ = D.build(name)
    net.load_state_dict(sd, strict=True)
    net64 = net.eval().double()
    den = D.Denoiser(name, emulation(D, torch, net64), nlm, backend='torch', channels_last=False, miopen_find=False)

    def denoise(a, i):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None].double()
        return den(t, i)[0, 0].numpy().astype(np.float32)
    return denoise


def _problem(golden_inputs):
    mask = golden_inputs['masks']['Q_Random30'].astype(np.float64)
    y = O.synthesize(O.requantise(golden_inputs['gray']), mask, golden_inputs['noises'])
    return mask, y


def _check(tag, out, ref, bound_from, gray):
    err, e_err = rel_l2(out, ref), rel_l2(bound_from, ref)
    dp = abs(_psnr(out, gray) - _psnr(ref, gray))
    print('LOOP %s: hip_f16 vs golden rel-L2 %.4g   oracle loop driven by E vs golden %.4g   ratio %.3f   PSNR %.3f dB (golden %.3f, diff %.4f)'
          % (tag, err, e_err, err / e_err, _psnr(out, gray), _psnr(ref, gray), dp))
    assert err <= 2 * e_err, (tag, err, e_err)
    assert dp <= 0.01, (tag, dp)


@pytest.mark.parametrize('n_it', [2, 5, 10])
def test_trained_ffdnet_loops_against_the_reference(env, golden_inputs, n_it, tmp_path, monkeypatch):
    from conftest import weights_trained
    S = env['S']
    sd = weights_trained('ffdnet_gray')
    mask, y = _problem(golden_inputs)
    den_e = _emulated_denoiser(env, 'ffdnet_gray', sd)
    if n_it == 5:
        monkeypatch.setenv('PNP_CONV_CHECK_RANGE', '1')             # every activation of the trained network stays inside the half range
    kw = dict(images=golden_inputs['gray'][None], model=sd, results=str(tmp_path), cnn_backend='hip_f16')
    tag = 'trained_cnc_d_ffdnet_gray_it%d' % n_it
    opts = dict(env['known50'][tag + '_opts'])
    opts['iter_num'] = int(opts['iter_num'])
    assert opts['iter_num'] == n_it
    out, _ = S.PNP_ADMM_CNC_D('ffdnet_gray', mask, golden_inputs['noises'], **kw, **opts)
    e_loop = O.pnp_admm_cnc(y, mask, den_e, n_it, opts['alpha'], opts['lambda1'], opts['reo'], opts['b'])
    _check(tag, out[0], env['gold50'][tag], e_loop, golden_inputs['gray'])
    tag = 'trained_l1_d_ffdnet_gray_it%d' % n_it
    reo = env['known50']['trained_l1_d_ffdnet_gray_opts']['reo']   # the S3 preset the fixture was recorded at
    out = S.PNP_ADMM_L1_D('ffdnet_gray', mask, golden_inputs['noises'], iter_num=n_it, reo=reo, **kw)
    e_loop = O.pnp_admm_l1(y, mask, den_e, n_it, reo)
    _check(tag, out[0], env['gold50'][tag], e_loop, golden_inputs['gray'])


@pytest.mark.parametrize('n_it', [2, 5])
def test_trained_dncnn_pair_against_the_reference(env, golden_inputs, n_it, tmp_path):
    from conftest import weights_trained
    S = env['S']
    sd = weights_trained('dncnn_25')
    mask, y = _problem(golden_inputs)
    den_e = _emulated_denoiser(env, 'dncnn_25', sd)                 # the reference loads model 1's file into both networks (S6:435)
    kw = dict(images=golden_inputs['gray'][None], results=str(tmp_path), cnn_backend='hip_f16')
    tag = 'trained_cnc_dncnn_pair_it%d' % n_it
    opts = dict(env['known50'][tag + '_opts'])
    opts['iter_num'] = int(opts['iter_num'])
    assert opts['iter_num'] == n_it
    out, _ = S.PNP_ADMM_CNC_DnCNN('dncnn_25', 'dncnn_15', mask, golden_inputs['noises'], model=sd, **kw, **opts)
    e_loop = O.pnp_admm_cnc(y, mask, den_e, n_it, opts['alpha'], opts['lambda1'], opts['reo'], opts['b'], denoise2=den_e)
    _check(tag, out[0], env['gold50'][tag], e_loop, golden_inputs['gray'])
    tag = 'trained_l1_d_dncnn_15_it%d' % n_it
    opts = dict(env['known50'][tag + '_opts'])
    opts['iter_num'] = int(opts['iter_num'])
    out = S.PNP_ADMM_L1_D('dncnn_15', mask, golden_inputs['noises'], model=sd, **kw, **opts)
    e_loop = O.pnp_admm_l1(y, mask, den_e, n_it, opts['reo'])
    _check(tag, out[0], env['gold50'][tag], e_loop, golden_inputs['gray'])


@pytest.mark.parametrize('tag', ['cnc_d_ffdnet_gray', 'cnc_d_fdncnn_gray', 'cnc_d_drunet_gray', 'cnc_d_ircnn_gray', 'cnc_dncnn_pair'])
def test_contractive_fixtures_at_fifty_iterations_hold_the_psnr(env, golden_inputs, tag, tmp_path):
    """all five families at the presets' own run length: PSNR within 0.01 dB of the unmodified reference's golden"""
    from conftest import weights50
    S = env['S']
    mask = golden_inputs['masks']['Q_Random30'].astype(np.float64)
    opts = dict(env['known50'][tag + '_opts'])
    opts['iter_num'] = int(opts['iter_num'])
    assert opts['iter_num'] == 50
    kw = dict(images=golden_inputs['gray'][None], results=str(tmp_path), cnn_backend='hip_f16')
    if tag == 'cnc_dncnn_pair':
        out, _ = S.PNP_ADMM_CNC_DnCNN('dncnn_25', 'dncnn_15', mask, golden_inputs['noises'], model=weights50('dncnn_25'), **kw, **opts)
    else:
        name = '_'.join(tag[len('cnc_d_'):].split('_')[:2])
        out, _ = S.PNP_ADMM_CNC_D(name, mask, golden_inputs['noises'], model=weights50(name), **kw, **opts)
    ref = env['gold50'][tag]
    assert np.isfinite(out[0]).all()
    p, pr = _psnr(out[0], golden_inputs['gray']), _psnr(ref, golden_inputs['gray'])
    print('FIFTY %s: rel-L2 vs golden %.4g   PSNR %.4f dB (golden %.4f)' % (tag, rel_l2(out[0], ref), p, pr))
    assert abs(p - pr) <= 0.01, (tag, p, pr)


def test_sub_batches_are_bit_equal(env, golden_inputs, tmp_path):
    """B = 9 in one call against 4 + 5: the same bits per slice (FFDNet through its fused first / last layers, and DRUNet)"""
    S = env['S']
    gray = golden_inputs['gray']
    imgs = np.stack([np.roll(gray, 17 * k, axis=k % 2) for k in range(9)])
    mask = golden_inputs['masks']['Q_Radial30'].astype(np.float64)
    for name, seed in (('ffdnet_gray', 7), ('drunet_gray', 3)):
        net, _, _ = env['D'].build(name)
        sd = env['D'].seeded_state_dict(net, seed)
        kw = dict(model=sd, results=str(tmp_path), cnn_backend='hip_f16', alpha=0.9, iter_num=3, lambda1=1.35, reo=0.45, b=0.3)
        full, _ = S.PNP_ADMM_CNC_D(name, mask, golden_inputs['noises'], images=imgs, **kw)
        a, _ = S.PNP_ADMM_CNC_D(name, mask, golden_inputs['noises'], images=imgs[:4], **kw)
        b, _ = S.PNP_ADMM_CNC_D(name, mask, golden_inputs['noises'], images=imgs[4:], **kw)
        for k in range(9):
            assert np.array_equal(full[k], (a[k] if k < 4 else b[k - 4])), (name, k)
        # cnn_graph=True: the captured forward gives the same bits
        g, _ = S.PNP_ADMM_CNC_D(name, mask, golden_inputs['noises'], images=imgs[:4], cnn_graph=True, **kw)
        for k in range(4):
            assert np.array_equal(g[k], a[k]), (name, 'graph', k)
