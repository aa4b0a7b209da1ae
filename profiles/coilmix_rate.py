"""Coil mixing ahead of the multi-coil solve: what the two kernels reach on the card and what compression buys.

    python profiles/coilmix_rate.py [--admm-batch 128] [--iters 10]      -> one JSON line per case

HIP events, warm, best of three after a warm-up.  Measured, not asserted: no threshold hangs on any of these.
  mix     pnp_coil_mix on B slices of 256 x 256, C_in -> C_out, float: ms, gbs = (C_in + C_out) 8 B N bytes / ms (the stream by design; M
          is not counted), tflops = 8 C_in C_out flops per point; gbs_stream: pnp_calibrate_stream on the same card
  gram    pnp_coil_gram at ncal = 24 on the same arrays: ms (it reads 576 points per coil and slice: latency, not bandwidth)
  admm    one ADMM_CNC iteration (preset, cg_iters = 3) on B slices of 256 x 256 with 32 physical coils, and with the 8 virtual coils that
          coilmix.prepare makes of the same data; ms_prepare: the whole setup (Gram, Jacobi, mixing y and the maps) from device arrays
  recon   relative L2 distance of the reconstruction from compressed data against the one from all coils (3 slices of 128 x 130, ten
          ADMM_CNC iterations, the oracle's smooth maps with random phase ramps)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import torch                                          # noqa: E402
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib, coilmix as CM  # noqa: E402
import multicoil_oracle as M                          # noqa: E402

H = W = 256


def best_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def p(t):
    return C.c_void_p(t.data_ptr())


def kernels(B, Cin, Cout, gbs_stream):
    L = _lib.lib()
    N = H * W
    k = torch.randn((B, Cin, H, W), dtype=torch.complex64, device='cuda')
    m = torch.randn((1, Cout, Cin), dtype=torch.complex64, device='cuda')
    out = torch.empty((B, Cout, H, W), dtype=torch.complex64, device='cuda')
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = best_ms(lambda: _lib.check(L.pnp_coil_mix(s, p(k), p(m), None, p(out), B, Cin, Cout, N)))
    r = dict(case='mix', B=B, C_in=Cin, C_out=Cout, H=H, W=W, ms=round(ms, 4), gbs=round((Cin + Cout) * 8 * B * N / 1e6 / ms, 1),
             tflops=round(8.0 * Cin * Cout * B * N / 1e9 / ms, 2), gbs_stream=round(gbs_stream, 1))
    print(json.dumps(r), flush=True)
    mask = torch.ones((1, H, W), dtype=torch.uint8, device='cuda')
    g = torch.empty((B, Cin, Cin), dtype=torch.complex128, device='cuda')
    ms = best_ms(lambda: _lib.check(L.pnp_coil_gram(s, p(k), p(mask), None, p(g), B, Cin, H, W, 24)))
    print(json.dumps(dict(case='gram', B=B, C=Cin, ncal=24, H=H, W=W, ms=round(ms, 4))), flush=True)


def admm_it(y, S, m, iters):
    B = y.shape[0]
    with P.Engine(H, W, Bmax=B) as eng:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.set_coils(S, 3)
        eng.upload(y, m)
        eng.init_state()
        eng.admm_cnc(iters, 0.45, 0.5, 0.05, 64)
        eng.sync()
        best = None
        for _ in range(3):
            eng.timer_start()
            eng.admm_cnc(iters, 0.45, 0.5, 0.05, 64)
            ms = eng.timer_stop() / iters
            best = ms if best is None else min(best, ms)
        return best, eng.x()


def admm(B, iters):
    S = M.coil_maps(32, H, W, 32).astype(np.complex64)
    m = M.mask(0, H, W)
    imgs = np.stack([M.phantom(b % 8, H, W) for b in range(B)])
    with P.Engine(H, W, Bmax=B) as eng:
        eng.set_coils(S, 3)
        eng.synthesize(imgs, np.zeros((H, W), np.complex64), m)
        y = eng.download_y()
    ms32, x32 = admm_it(y, S, m, iters)
    y_t, S_t = torch.from_numpy(y).cuda(), torch.from_numpy(S).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y8, S8, info = CM.prepare(y_t, S_t, m, virtual_coils=8)
    torch.cuda.synchronize()
    prep = (time.perf_counter() - t0) * 1e3
    ms8, x8 = admm_it(y8.cpu().numpy(), S8.cpu().numpy(), m, iters)
    print(json.dumps(dict(case='admm', B=B, H=H, W=W, cg_iters=3, ms_per_it_32_physical=round(ms32, 4), ms_per_it_8_virtual=round(ms8, 4),
                          ratio=round(ms32 / ms8, 2), ms_prepare=round(prep, 1), energy=round(info['energy'], 5),
                          rel_l2_8_vs_32=float(np.linalg.norm(x8 - x32) / np.linalg.norm(x32)))), flush=True)


def recon():
    Hn, Wn, B = 128, 130, 3
    m = M.mask(1, Hn, Wn)
    imgs = np.stack([M.phantom(b, Hn, Wn) for b in range(B)])
    for Cin, Cout in ((16, 8), (32, 8), (32, 12)):
        S = M.coil_maps(Cin, Hn, Wn, Cin)
        y = np.stack([M.synthesize(imgs[b], S, m, M.noise(b, Cin, m)) for b in range(B)])
        kw = dict(y=y, coils=S, iter_num=10, **M.O_PRESETS['cnc'])
        full = np.stack(P.ADMM_CNC(m, None, **kw)[:B])
        comp, info = P.ADMM_CNC(m, None, virtual_coils=Cout, return_info=True, **kw)
        d = [float(np.linalg.norm(comp[b] - full[b]) / np.linalg.norm(full[b])) for b in range(B)]
        print(json.dumps(dict(case='recon', H=Hn, W=Wn, C_in=Cin, C_out=Cout, rel_l2_compressed_vs_full=[round(v, 5) for v in d],
                              energy=round(info['coil_mix']['energy'], 5))), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--admm-batch', type=int, default=128)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    gbs = C.c_double(0)
    _lib.check(_lib.lib().pnp_calibrate_stream(0, 512, 1.0, C.byref(gbs)))
    kernels(512, 32, 8, gbs.value)
    kernels(64, 128, 32, gbs.value)
    admm(a.admm_batch, a.iters)
    recon()
