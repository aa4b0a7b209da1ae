#!/usr/bin/env python3
"""Rates of backend 'hip_f16' beside 'hip_f16x3' (output: profiles/conv_f16_r07.txt), one card, one process, HIP events:

  layer    the 64 -> 64 conv3x3 + bias + ReLU body layer at [256, 64, 128, 128] (config 3's shape per CNN call): the f16x3 layer as the
           library dispatches it inside a stack (split activation format in and out, the wide kernel) and the hip_f16 layer (halves in
           and out); blocks of launches alternate between the two, >= 2 s each in total.  THE CONDITION: t(hip_f16) <= t(f16x3) / 1.5.
  config 3 512 slices of 256 x 256, trained FFDNet, Q_Radial30, PNP_ADMM_CNC_D's S6:573 preset, sustained >= 5 s, both backends
  config 4 DRUNet's shard of 512 slices, Q_Cartesian30, both backends (reported, not gated)

usage: python profiles/experiments/conv_f16_rate.py [--layer-only] [--sustain-s 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def layer_rates(torch, L, lib, seconds=2.0):
    n, H, W, ch = 256, 128, 128, 64
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    g = torch.Generator(device='cuda').manual_seed(1)
    x32 = torch.relu(torch.randn(n, H, W, ch, device='cuda', generator=g)) * 0.5          # a body layer's input: ReLU'd, O(1)
    w = torch.randn(ch, ch, 3, 3, device='cuda', generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(ch, device='cuda', generator=g) * 0.1
    from pnp_admm_cnc_mri_amd import denoisers as D, hip_layers as HL
    xs = HL.split_activations(x32)
    ys = torch.empty_like(xs)
    w3 = torch.empty(9 * ch * ch, device='cuda')
    lib.check(L.pnp_conv3x3_pack_f16x3(s, p(w), p(w3), ch))
    xh = x32.half()
    yh = torch.empty_like(xh)
    wh = torch.empty(9 * ch * ch, dtype=torch.float16, device='cuda')
    lib.check(L.pnp_conv3x3_pack_f16(s, p(w), p(wh), ch))
    f3 = lambda: lib.check(L.pnp_conv3x3_nhwc_f16x3_fmt(s, p(xs), p(w3), p(b), None, p(ys), n, ch, H, W, 1, 1, 7))
    fh = lambda: lib.check(L.pnp_conv3x3_nhwc_f16(s, p(xh), p(wh), p(b), None, p(yh), n, ch, H, W, 1, 1, 0))
    # same inputs, so the two results agree to half precision (a wrong kernel is not a fast kernel)
    f3(); fh()
    torch.cuda.synchronize()
    dev = float((yh.float() - HL.unsplit_activations(ys)).norm() / HL.unsplit_activations(ys).norm())
    assert dev < 2e-3, dev
    for _ in range(30):
        f3(); fh()
    torch.cuda.synchronize()
    tot = {'f16x3': [0.0, 0], 'f16': [0.0, 0]}
    blocks = []
    t_end = time.perf_counter() + 2 * seconds
    while time.perf_counter() < t_end or min(v[0] for v in tot.values()) < seconds * 1e3:
        for name, f in (('f16x3', f3), ('f16', fh)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                f()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            tot[name][0] += ms
            tot[name][1] += 100
            blocks.append((name, ms / 100))
    flop = 2.0 * n * H * W * ch * ch * 9
    res = {}
    for name in tot:
        per = sorted(v for k, v in blocks if k == name)
        t_ms = tot[name][0] / tot[name][1]
        bytes_ = n * H * W * ch * (8 if name == 'f16x3' else 4)                         # activations read + written once
        res[name] = dict(ms=t_ms, ms_min_block=per[0], ms_max_block=per[-1], launches=tot[name][1], tflops_products=flop / t_ms / 1e9,
                         gb_per_s=bytes_ / t_ms / 1e6)
    res['speedup'] = res['f16x3']['ms'] / res['f16']['ms']
    res['agreement_rel_l2'] = dev
    return res


def pnp_rate(torch, model, backend, sustain_s, B=512):
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import denoisers as D, solvers_pnp as SP, synthetic as S, utils_pnp
    import bench_pnp
    fam = D.family(model)
    H = W = 256
    mname = {'ffdnet': 'Q_Radial30', 'drunet': 'Q_Cartesian30'}[fam]
    masks = S.reference_masks()[mname].astype(np.uint8)[None]
    img, noise = S.batch(0, B, H, W)
    opts = SP.PRESETS['PNP_ADMM_CNC_D'][fam]
    dev = torch.device('cuda', 0)
    net, nlm, sched = D.build(model)
    sd, _ = bench_pnp.fixture_weights(model, net, 'trained' if fam == 'ffdnet' else 'contractive')
    net.load_state_dict(sd)
    sig = torch.tensor(utils_pnp.get_rho_sigma(max(0.255 / 255., nlm), 50, 49, nlm * 255., 1.0)[1]) if sched else None
    den = D.Denoiser(model, net.eval(), nlm, sigmas=sig, backend=backend).to(dev)
    eng = P.Engine(H, W, Bmax=B, device=0)
    eng.synthesize(img, noise, masks, np.zeros(B, np.int32))
    eng.init_state()
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    z = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    w = torch.empty_like(z)
    eng.get_state(z, w)
    x, s, t, zn = (torch.empty_like(z) for _ in range(4))

    def it(i):
        nonlocal z, zn
        eng.dc_step(z, w, x, opts['reo'])
        den(z, i % 50, out=s)
        eng.cnc_combine(z, x, w, s, t, opts['alpha'], opts['lambda1'], opts['reo'], opts['b'])
        den(t, i % 50, out=zn)
        eng.dual_clamp(x, zn, w)
        z, zn = zn, z
    with torch.no_grad():
        for i in range(3):
            it(i)
        torch.cuda.synchronize()
        n_it, t0 = 0, time.perf_counter()
        while True:
            for _ in range(5):
                it(3 + n_it)
                n_it += 1
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if wall >= sustain_s:
                break
    finite = bool(torch.isfinite(x).all())
    del eng
    return dict(model=model, backend=backend, slices=B, iterations=n_it, seconds=wall, it_per_s=n_it / wall, slice_it_per_s=B * n_it / wall, finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layer-only', action='store_true')
    ap.add_argument('--sustain-s', type=float, default=5.0)
    args = ap.parse_args()
    import torch
    from pnp_admm_cnc_mri_amd import _lib
    assert torch.cuda.is_available(), 'needs the GPU: there is no CPU path to time'
    L = _lib.lib()
    prop = torch.cuda.get_device_properties(0)
    clk, cus, pci, arch = C.c_int(0), C.c_int(0), C.create_string_buffer(32), C.create_string_buffer(64)
    _lib.check(L.pnp_device_info(0, C.byref(clk), C.byref(cus), pci, 32, arch, 64))
    print('card: %s, PCI %s (%s), %d compute units, %d MHz; torch %s; command: %s' % (prop.name, pci.value.decode(), arch.value.decode(), cus.value, clk.value,
                                                                                       torch.__version__, ' '.join(sys.argv)))
    r = layer_rates(torch, L, _lib)
    print('LAYER [256, 64, 128, 128] conv3x3 + bias + ReLU, HIP events, blocks of 100 launches alternating:')
    for k in ('f16x3', 'f16'):
        v = r[k]
        print('  %-6s %.4f ms per layer (blocks %.4f .. %.4f, %d launches)   %.1f TFLOP/s of products   %.0f GB/s of activations'
              % (k, v['ms'], v['ms_min_block'], v['ms_max_block'], v['launches'], v['tflops_products'], v['gb_per_s']))
    print('  hip_f16 / f16x3 speed-up: %.3f x   (condition: >= 1.5)   agreement of the two results: rel-L2 %.3g' % (r['speedup'], r['agreement_rel_l2']))
    out = {'layer': r}
    if not args.layer_only:
        out['pnp'] = []
        for model in ('ffdnet_gray', 'drunet_gray'):
            for backend in ('hip_f16x3', 'hip_f16', 'hip_f16x3', 'hip_f16'):       # twice, alternating: the spread
                e = pnp_rate(torch, model, backend, args.sustain_s)
                out['pnp'].append(e)
                print('PNP_ADMM_CNC_D %-12s %-10s 512 slices: %.3f it/s (%d iterations in %.2f s, finite=%s)'
                      % (model, backend, e['it_per_s'], e['iterations'], e['seconds'], e['finite']))
    print('JSON ' + json.dumps(out))
    return 0 if r['speedup'] >= 1.5 else 3


if __name__ == '__main__':
    sys.exit(main())
