"""Complex-valued images on a coil context: what the complex mode costs over the real one on the card.

    python profiles/complex_rate.py [--batch 512] [--coils 8] [--iters 10] [--calls 30]      -> one JSON line

B slices of 256 x 256, C coils, ADMM_CNC preset, cg_iters = 3, float; HIP events (the library's timer), warm, best of three.  Two engines
in one process, one in real and one in complex mode, on the same measurements; every figure is taken real / complex / real / complex ...
  ms_admm_it        one ADMM iteration (x-step + prox) of pnp_admm_cnc_run: pixel prox, and db2 with 3 levels
  ms_xstep          pnp_dc_step / pnp_dc_step_cx on device tensors
  ms_prox           pnp_prox_cnc_dual / pnp_prox_cnc_dual_cx alone, pixel and db2 (best of three windows of `calls` calls, per call)
  gbs_prox_design   the complex prox's bytes by design over its time: pixel CNC five complex arrays (x, z, w read; z, w written: 40 B per
                    pixel), wavelet CNC 11 (analysis: z -> c, x, w and c -> c; synthesis: c, x, w -> z, w: 88 B per pixel)
  gbs_stream        pnp_calibrate_stream on the same card
--real-only: the real-mode iteration and prox alone, through calls the parent commit has too: copied into a built checkout of the parent
and run there, it times the real prox of the parent, which the complex prox is set against (one process per tree, alternating)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                          # noqa: E402
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib                 # noqa: E402

H = W = 256
CNC = (0.45, 0.5, 0.05, 64)


def scene(B, Cn):
    """-> maps [C,H,W] complex64 (Gaussian magnitudes on a circle, linear phases, sum_c |S_c|^2 = 1), mask [H,W] uint8 (30 % random
    plus six full lines around DC), images [B,H,W] float32 (eight different discs on an ellipse)"""
    rng = np.random.default_rng(20)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (yy - H / 2) / H, (xx - W / 2) / W
    S = np.empty((Cn, H, W), np.complex128)
    for c in range(Cn):
        a = 2 * np.pi * c / Cn + 0.3
        mag = np.exp(-((u - 0.6 * np.sin(a)) ** 2 + (v - 0.6 * np.cos(a)) ** 2) / (2 * 0.45 ** 2))
        ky, kx = rng.uniform(-2.0, 2.0, 2)
        S[c] = mag * np.exp(2j * np.pi * (ky * u + kx * v))
    S /= np.sqrt((np.abs(S) ** 2).sum(0, keepdims=True))
    m = rng.uniform(size=(H, W)) < 0.30
    m[:3] = m[-3:] = True
    base = 0.55 * (((u / 0.38) ** 2 + (v / 0.30) ** 2) <= 1.0)
    eight = [np.clip(base + 0.3 * (((u - 0.1 * np.sin(k)) ** 2 + (v - 0.1 * np.cos(k)) ** 2) <= 0.11 ** 2), 0, 1) for k in range(8)]
    return S.astype(np.complex64), m.astype(np.uint8), np.stack([eight[b % 8] for b in range(B)]).astype(np.float32)


def timed(eng, fn):
    eng.timer_start()
    fn()
    return eng.timer_stop()


def alternate(pairs, reps=3):
    """pairs: {name: (engine, fn)}; a warm-up of each, then `reps` rounds over all of them in order -> best ms per name"""
    for eng, fn in pairs.values():
        fn()
        eng.sync()
    best = {}
    for _ in range(reps):
        for name, (eng, fn) in pairs.items():
            ms = timed(eng, fn)
            best[name] = ms if name not in best else min(best[name], ms)
    return best


def real_only(B, Cn, iters, calls):
    """the real-mode figures alone, through calls that the parent commit has too: run from a built checkout of the parent, this is the
    real prox of the parent on the same card"""
    S, m, imgs = scene(B, Cn)
    out = dict(H=H, W=W, B=B, C=Cn, cg_iters=3, tree=os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    with P.Engine(H, W, Bmax=B) as e:
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.set_coils(S, 3)
        e.synthesize(imgs, np.zeros((H, W), np.complex64), m)
        e.init_state()
        z, w, x = (torch.empty((B, H, W), dtype=torch.float32, device='cuda') for _ in range(3))
        e.get_state(z, w)
        e.dc_step(z, w, x, CNC[2])
        prox = lambda: [e.prox_cnc_dual(x, z, w, *CNC) for _ in range(calls)]
        out['ms_admm_it_pixel_real'] = round(alternate({'r': (e, lambda: e.admm_cnc(iters, *CNC))})['r'] / iters, 4)
        out['ms_prox_pixel_real'] = round(alternate({'r': (e, prox)})['r'] / calls, 4)
        e.set_sparsity('db2', 3)
        e.init_state()
        out['ms_admm_it_db2_real'] = round(alternate({'r': (e, lambda: e.admm_cnc(iters, *CNC))})['r'] / iters, 4)
        out['ms_prox_db2_real'] = round(alternate({'r': (e, prox)})['r'] / calls, 4)
    return out


def main(B, Cn, iters, calls):
    S, m, imgs = scene(B, Cn)
    out = dict(H=H, W=W, B=B, C=Cn, cg_iters=3)
    stream = torch.cuda.current_stream().cuda_stream
    with P.Engine(H, W, Bmax=B) as er, P.Engine(H, W, Bmax=B) as ec:
        for e in (er, ec):
            e.set_stream(stream)
            e.set_coils(S, 3)
        er.synthesize(imgs, np.zeros((H, W), np.complex64), m)
        y = er.download_y()
        ec.set_image_mode('complex')
        ec.upload(y, m)
        del y
        engines = {'real': er, 'complex': ec}
        st = {}
        for k, e in engines.items():
            e.init_state()
            dt = torch.complex64 if k == 'complex' else torch.float32
            z, w, x = (torch.empty((B, H, W), dtype=dt, device='cuda') for _ in range(3))
            e.get_state(z, w)
            st[k] = (z, w, x)
        out['launches_per_iteration'] = {k: e.kernels_per_iteration for k, e in engines.items()}
        loop = lambda e: (lambda: e.admm_cnc(iters, *CNC))
        step = lambda k: (lambda: engines[k].dc_step(st[k][0], st[k][1], st[k][2], CNC[2]))

        def prox(k):
            z, w, x = st[k]
            return lambda: [engines[k].prox_cnc_dual(x, z, w, *CNC) for _ in range(calls)]

        r = alternate({k: (e, loop(e)) for k, e in engines.items()})
        out['ms_admm_it_pixel'] = {k: round(v / iters, 4) for k, v in r.items()}
        r = alternate({k: (engines[k], step(k)) for k in engines})
        out['ms_xstep'] = {k: round(v, 4) for k, v in r.items()}
        r = alternate({k: (engines[k], prox(k)) for k in engines})
        out['ms_prox_pixel'] = {k: round(v / calls, 4) for k, v in r.items()}
        for e in engines.values():
            e.set_sparsity('db2', 3)
            e.init_state()
        out['launches_per_iteration_db2'] = {k: e.kernels_per_iteration for k, e in engines.items()}
        r = alternate({k: (e, loop(e)) for k, e in engines.items()})
        out['ms_admm_it_db2'] = {k: round(v / iters, 4) for k, v in r.items()}
        r = alternate({k: (engines[k], prox(k)) for k in engines})
        out['ms_prox_db2'] = {k: round(v / calls, 4) for k, v in r.items()}
    px = B * H * W
    out['gbs_prox_design'] = {'pixel': round(40 * px / 1e9 / (out['ms_prox_pixel']['complex'] * 1e-3), 1),
                              'db2': round(88 * px / 1e9 / (out['ms_prox_db2']['complex'] * 1e-3), 1)}
    out['ratio_complex_over_real'] = {k[3:]: round(out[k]['complex'] / out[k]['real'], 3)
                                      for k in ('ms_admm_it_pixel', 'ms_admm_it_db2', 'ms_xstep', 'ms_prox_pixel', 'ms_prox_db2')}
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--coils', type=int, default=8)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--real-only', action='store_true', help='the real-mode figures alone (also runs from a checkout of the parent commit)')
    a = ap.parse_args()
    if a.real_only:
        print(json.dumps(real_only(a.batch, a.coils, a.iters, a.calls)), flush=True)
        sys.exit(0)
    gbs = C.c_double(0)
    _lib.check(_lib.lib().pnp_calibrate_stream(0, 512, 1.0, C.byref(gbs)))
    res = main(a.batch, a.coils, a.iters, a.calls)
    res['gbs_stream'] = round(gbs.value, 1)
    print(json.dumps(res), flush=True)
