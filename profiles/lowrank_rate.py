"""Rate of the locally low-rank prox (pnp_set_lowrank): 512 slices of 256 x 256, float, HIP events, warm, best of
three rounds with the arms ALTERNATING in one process.

  prox launch      the low-rank prox (L1 and CNC) at b = 8, T = 4 .. 64, and b = 16, T = 16, beside the temporal prox at the same T and
                   the pixel prox -- both through the parent commit's libpnpmri.so with --parent-lib (raw ctypes), else this library's,
                   which has the same kernels.  All move the same bytes by design: x and w read, z and w written (16 B per pixel-frame),
                   CNC reads z too (20 B; the low-rank CNC launch re-reads x and w twice more, from L2 at these sizes).
                   tbs = those designed bytes over the launch time.
  iteration        a whole loop iteration with the block set (b = 8, T = 16; four launches) beside the pixel loop.
  gbs_stream       pnp_calibrate_stream on the same card.

    python profiles/lowrank_rate.py [--parent-lib PATH] [--rounds 3] > profiles/lowrank_rate.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib, engine as E, synthetic as S   # noqa: E402

L1 = (0.1, 0.015)
CNC = (0.45, 0.5, 0.05, 64.0)
B, H, W = 512, 256, 256
REPS, LR_REPS, ITERS = 20, 3, 5
ARMS = ((8, 4), (8, 8), (8, 16), (8, 32), (8, 64), (16, 16))       # (b, T)


def problem(n):
    m = S.reference_masks()
    masks = np.stack([m[k] for k in ('Q_Random30', 'Q_Radial30', 'Q_Cartesian30')]).astype(np.uint8)
    img, noise = S.batch(0, 8)
    reps = (n + 7) // 8
    return np.tile(img, (reps, 1, 1))[:n], np.tile(noise, (reps, 1, 1))[:n], masks, (np.arange(n) % 3).astype(np.int32)


class Parent:
    """the pixel prox and the temporal prox through another build of the library (calls the parent commit has)"""

    def __init__(self, path, img, noise, masks, mid):
        L = self.L = C.CDLL(path)
        self.ctx = C.c_void_p()
        vp = C.c_void_p
        L.pnp_ctx_create.argtypes = [C.c_int] * 4 + [C.POINTER(vp)]
        L.pnp_synthesize_problem.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int]
        L.pnp_prox_l1_dual.argtypes = [vp] * 4 + [C.c_double]
        L.pnp_prox_cnc_dual.argtypes = [vp] * 4 + [C.c_double] * 4
        L.pnp_set_temporal.argtypes = [vp, C.c_int, C.c_int]
        L.pnp_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
        for f in (L.pnp_init_state, L.pnp_timer_start, L.pnp_ctx_destroy, L.pnp_sync):
            f.argtypes = [vp]
        assert L.pnp_ctx_create(0, H, W, len(img), C.byref(self.ctx)) == 0
        assert L.pnp_synthesize_problem(self.ctx, img.ctypes.data, noise.ctypes.data, 1, masks.ctypes.data, mid.ctypes.data, len(img), len(masks), 0) == 0
        assert L.pnp_init_state(self.ctx) == 0
        self.abi = L.pnp_abi_version()
        self.has_lowrank = hasattr(L, 'pnp_set_lowrank')

    def prox(self, cnc, t, frames):
        L = self.L
        assert L.pnp_set_temporal(self.ctx, frames or 0, 1) == 0
        p = [C.c_void_p(a.data_ptr()) for a in t]
        ms = C.c_float()
        assert L.pnp_timer_start(self.ctx) == 0
        for _ in range(REPS):
            if cnc:
                L.pnp_prox_cnc_dual(self.ctx, *p, *CNC)
            else:
                L.pnp_prox_l1_dual(self.ctx, *p, L1[0] * L1[1])
        assert L.pnp_timer_stop(self.ctx, C.byref(ms)) == 0
        return ms.value / REPS


def prox(eng, cnc, t, reps):
    eng.timer_start()
    for _ in range(reps):
        if cnc:
            eng.prox_cnc_dual(*t, *CNC)
        else:
            eng.prox_l1_dual(*t, L1[0] * L1[1])
    return eng.timer_stop() / reps


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
        raise SystemExit('lowrank_rate: no HIP device')
    img, noise, masks, mid = problem(B)
    parent = Parent(a.parent_lib, img, noise, masks, mid) if a.parent_lib else None
    dev = torch.device('cuda', 0)
    t0 = [torch.rand((B, H, W), device=dev) for _ in range(3)]
    n = B * H * W
    with P.Engine(H, W, Bmax=B) as eng:
        eng.synthesize(img, noise, masks, mid)
        eng.init_state()
        print('%d slices of %d x %d, float; %d launches per window (%d of the low-rank prox, %d iterations), best of %d alternating rounds'
              % (B, H, W, REPS, LR_REPS, ITERS, a.rounds))
        if parent:
            print('pixel prox and temporal prox: the parent library (ABI %d, pnp_set_lowrank %s)' % (parent.abi, 'present' if parent.has_lowrank else 'absent'))
        ms = {}
        for r in range(a.rounds + 1):                                      # round 0 warms every arm up
            for cnc in (False, True):
                kind = 'cnc' if cnc else 'l1'
                t = [x.clone() for x in t0]                                  # the same data for every arm: the sweeps depend on it
                eng.set_temporal(None)
                ms.setdefault((kind, 'pixel', 0, 0), []).append(parent.prox(cnc, t, None) if parent else prox(eng, cnc, t, REPS))
                for b, T in ARMS:
                    t = [x.clone() for x in t0]
                    if parent:
                        v = parent.prox(cnc, t, T)
                    else:
                        eng.set_temporal(T)
                        v = prox(eng, cnc, t, REPS)
                    ms.setdefault((kind, 'temporal', 0, T), []).append(v)
                    t = [x.clone() for x in t0]
                    eng.set_temporal(T)
                    eng.set_lowrank(b, None, E.lowrank_table('random', b))
                    ms.setdefault((kind, 'lowrank', b, T), []).append(prox(eng, cnc, t, LR_REPS))
                    eng.set_lowrank(0)
                eng.set_temporal(None)
                ms.setdefault((kind, 'iter pixel', 0, 0), []).append(iteration(eng, cnc))
                eng.set_temporal(16)
                eng.set_lowrank(8, None, E.lowrank_table('random', 8))
                ms.setdefault((kind, 'iter lowrank', 8, 16), []).append(iteration(eng, cnc))
                eng.set_temporal(None)
        best = {k: min(v[1:]) for k, v in ms.items()}
        for (kind, arm, b, T), v in ms.items():
            per = 20 if kind == 'cnc' else 16
            med = float(np.median(v[1:]))
            if arm == 'pixel':
                print('prox %-3s pixel              best %9.4f ms  median %9.4f ms  %5.1f MB by design -> %6.3f TB/s' % (kind, best[kind, arm, b, T], med, per * n / 1e6, per * n / best[kind, arm, b, T] / 1e9))
            elif arm == 'temporal':
                print('prox %-3s temporal T=%-2d      best %9.4f ms  median %9.4f ms  %6.3f TB/s' % (kind, T, best[kind, arm, b, T], med, per * n / best[kind, arm, b, T] / 1e9))
            elif arm == 'lowrank':
                x = best[kind, arm, b, T]
                print('prox %-3s lowrank b=%-2d T=%-2d best %9.4f ms  median %9.4f ms  %6.3f TB/s   %6.1f x temporal, %6.1f x pixel' % (
                    kind, b, T, x, med, per * n / x / 1e9, x / best[kind, 'temporal', 0, T], x / best[kind, 'pixel', 0, 0]))
            else:
                print('iteration %-3s %-22s best %9.4f ms  median %9.4f ms' % (kind, arm[5:] + (' b=%d T=%d' % (b, T) if b else ', slice-resident'), best[kind, arm, b, T], med))
    gbs = C.c_double()
    _lib.check(_lib.lib().pnp_calibrate_stream(0, B, 1.0, C.byref(gbs)))
    print('pnp_calibrate_stream, %d slices: %.0f GB/s' % (B, gbs.value))


if __name__ == '__main__':
    main()
