"""Rate of the temporal prox (pnp_set_temporal; DESIGN.md, temporal section): 512 slices of 256 x 256, float, HIP events, warm, best of
three rounds with the arms ALTERNATING in one process.

  prox launch      the temporal prox (L1 and CNC) at T = 2 .. 64 beside the pixel prox -- through the parent commit's libpnpmri.so with
                   --parent-lib (raw ctypes), else this library's, which is the same kernel.  The two move the same bytes: x and w read,
                   z and w written (16 B per pixel-frame), CNC reads z too (20 B).  tbs = those designed bytes over the launch time.
  iteration        a whole loop iteration with frames set (T = 16, 64; four launches) beside an iteration of the wavelet loop (db2, three
                   levels; five launches) -- the parent's with --parent-lib -- and of the pixel loop (slice-resident at this batch).
  double           the iteration with frames set on a double-precision context, 128 slices.
  gbs_stream       pnp_calibrate_stream on the same card.

    python profiles/temporal_rate.py [--parent-lib PATH] [--rounds 3] > profiles/temporal_rate.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib, synthetic as S   # noqa: E402

L1 = (0.1, 0.015)
CNC = (0.45, 0.5, 0.05, 64.0)
B, H, W = 512, 256, 256
REPS, ITERS = 20, 10
FRAMES = (2, 4, 8, 16, 32, 64)


def problem(n):
    m = S.reference_masks()
    masks = np.stack([m[k] for k in ('Q_Random30', 'Q_Radial30', 'Q_Cartesian30')]).astype(np.uint8)
    img, noise = S.batch(0, 8)
    reps = (n + 7) // 8
    return np.tile(img, (reps, 1, 1))[:n], np.tile(noise, (reps, 1, 1))[:n], masks, (np.arange(n) % 3).astype(np.int32)


class Parent:
    """the pixel prox and the wavelet loop through another build of the library (calls the parent commit has)"""

    def __init__(self, path, img, noise, masks, mid):
        L = self.L = C.CDLL(path)
        self.ctx = C.c_void_p()
        vp = C.c_void_p
        L.pnp_ctx_create.argtypes = [C.c_int] * 4 + [C.POINTER(vp)]
        L.pnp_synthesize_problem.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int]
        L.pnp_admm_l1_run.argtypes = [vp, C.c_int] + [C.c_double] * 2
        L.pnp_admm_cnc_run.argtypes = [vp, C.c_int] + [C.c_double] * 4
        L.pnp_prox_l1_dual.argtypes = [vp] * 4 + [C.c_double]
        L.pnp_prox_cnc_dual.argtypes = [vp] * 4 + [C.c_double] * 4
        L.pnp_set_sparsity.argtypes = [vp, C.c_int, C.c_int]
        L.pnp_set_fast_path.argtypes = [vp, C.c_int]
        L.pnp_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
        for f in (L.pnp_init_state, L.pnp_timer_start, L.pnp_ctx_destroy, L.pnp_sync):
            f.argtypes = [vp]
        assert L.pnp_ctx_create(0, H, W, len(img), C.byref(self.ctx)) == 0
        assert L.pnp_synthesize_problem(self.ctx, img.ctypes.data, noise.ctypes.data, 1, masks.ctypes.data, mid.ctypes.data, len(img), len(masks), 0) == 0
        assert L.pnp_init_state(self.ctx) == 0
        self.abi = L.pnp_abi_version()

    def timed(self, fn):
        ms = C.c_float()
        assert self.L.pnp_timer_start(self.ctx) == 0
        fn()
        assert self.L.pnp_timer_stop(self.ctx, C.byref(ms)) == 0
        return ms.value

    def prox(self, cnc, t):
        p = [C.c_void_p(a.data_ptr()) for a in t]
        if cnc:
            return self.timed(lambda: [self.L.pnp_prox_cnc_dual(self.ctx, *p, *CNC) for _ in range(REPS)]) / REPS
        return self.timed(lambda: [self.L.pnp_prox_l1_dual(self.ctx, *p, L1[0] * L1[1]) for _ in range(REPS)]) / REPS

    def wavelet_iteration(self, cnc):
        L = self.L
        assert L.pnp_set_sparsity(self.ctx, 2, 3) == 0 and L.pnp_init_state(self.ctx) == 0
        run = (lambda: L.pnp_admm_cnc_run(self.ctx, ITERS, *CNC)) if cnc else (lambda: L.pnp_admm_l1_run(self.ctx, ITERS, *L1))
        t = self.timed(run) / ITERS
        assert L.pnp_set_sparsity(self.ctx, 0, 0) == 0
        return t


def prox(eng, cnc, t):
    eng.timer_start()
    for _ in range(REPS):
        if cnc:
            eng.prox_cnc_dual(*t, *CNC)
        else:
            eng.prox_l1_dual(*t, L1[0] * L1[1])
    return eng.timer_stop() / REPS


def iteration(eng, cnc):
    eng.init_state()
    eng.timer_start()
    if cnc:
        eng.admm_cnc(ITERS, *CNC)
    else:
        eng.admm_l1(ITERS, *L1)
    return eng.timer_stop() / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import torch
    if _lib.device_count() < 1:
        raise SystemExit('temporal_rate: no HIP device')
    img, noise, masks, mid = problem(B)
    parent = Parent(a.parent_lib, img, noise, masks, mid) if a.parent_lib else None
    dev = torch.device('cuda', 0)
    t = [torch.rand((B, H, W), device=dev) for _ in range(3)]
    n = B * H * W
    with P.Engine(H, W, Bmax=B) as eng:
        eng.synthesize(img, noise, masks, mid)
        eng.init_state()
        print('%d slices of %d x %d, float; %d launches (%d iterations) per window, best of %d alternating rounds' % (B, H, W, REPS, ITERS, a.rounds))
        if parent:
            print('pixel prox and wavelet loop: the parent library (ABI %d)' % parent.abi)
        ms = {}
        for r in range(a.rounds + 1):                                      # round 0 warms every arm up
            for cnc in (False, True):
                kind = 'cnc' if cnc else 'l1'
                eng.set_temporal(None)
                v = parent.prox(cnc, t) if parent else prox(eng, cnc, t)
                ms.setdefault(('prox', kind, 'pixel'), []).append(v)
                for T in FRAMES:
                    eng.set_temporal(T)
                    ms.setdefault(('prox', kind, T), []).append(prox(eng, cnc, t))
                eng.set_temporal(None)
                ms.setdefault(('iter', kind, 'pixel, slice-resident'), []).append(iteration(eng, cnc))
                if parent:
                    ms.setdefault(('iter', kind, 'wavelet db2 L3 (parent)'), []).append(parent.wavelet_iteration(cnc))
                else:
                    eng.set_sparsity('db2', 3)
                    ms.setdefault(('iter', kind, 'wavelet db2 L3'), []).append(iteration(eng, cnc))
                    eng.set_sparsity(None)
                for T in (16, 64):
                    eng.set_temporal(T)
                    ms.setdefault(('iter', kind, 'temporal T=%d' % T), []).append(iteration(eng, cnc))
                eng.set_temporal(None)
        for (what, kind, arm), v in ms.items():
            best, med = min(v[1:]), float(np.median(v[1:]))
            if what == 'prox':
                per = 20 if kind == 'cnc' else 16
                print('prox %-3s %-8s best %8.4f ms  median %8.4f ms  %5.1f MB by design -> %6.3f TB/s' % (
                    kind, arm if arm == 'pixel' else 'T=%d' % arm, best, med, per * n / 1e6, per * n / best / 1e9))
            else:
                print('iteration %-3s %-26s best %8.4f ms  median %8.4f ms' % (kind, arm, best, med))
    # double: a whole iteration with frames set on 128 slices (the real step-wise prox call is float only)
    BD = 128
    with P.Engine(H, W, Bmax=BD, precision='f64') as eng:
        eng.synthesize(img[:BD], noise[:BD], masks, mid[:BD])
        ms = {}
        for r in range(a.rounds + 1):
            for cnc in (False, True):
                for T in (16, 64):
                    eng.set_temporal(T)
                    ms.setdefault(('cnc' if cnc else 'l1', T), []).append(iteration(eng, cnc))
        for (kind, T), v in ms.items():
            print('iteration %-3s double, %d slices, temporal T=%-2d   best %8.4f ms  median %8.4f ms' % (kind, BD, T, min(v[1:]), float(np.median(v[1:]))))
    gbs = C.c_double()
    _lib.check(_lib.lib().pnp_calibrate_stream(0, B, 1.0, C.byref(gbs)))
    print('pnp_calibrate_stream, %d slices: %.0f GB/s' % (B, gbs.value))


if __name__ == '__main__':
    main()
