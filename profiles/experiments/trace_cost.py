"""What the convergence trace costs: 512 slices x 100 iterations of ADMM_CNC (S4:176 presets), HIP events, the arms
ALTERNATING in one process -- untraced; every=10 and every=1, each with and without a ground truth -- and, with --parent-lib, the
untraced run through the parent commit's libpnpmri.so in the same alternation (raw ctypes: the evidence that the headline path did not
move).  Then the reduction kernel alone (pnp_residuals on 512 slices in natural order) in GB/s beside pnp_calibrate_stream of the same
card, and one slice x 50 iterations with every=1 beside the `latency` record of bench.py.

    python profiles/experiments/trace_cost.py [--parent-lib PATH] [--rounds 5] > profiles/experiments/trace_cost.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib, synthetic as S   # noqa: E402

CNC = (0.45, 0.5, 0.05, 64.0)
B, ITERS = 512, 100


def problem(n):
    m = S.reference_masks()
    masks = np.stack([m[k] for k in ('Q_Random30', 'Q_Radial30', 'Q_Cartesian30')]).astype(np.uint8)
    img, noise = S.batch(0, 8)
    reps = (n + 7) // 8
    return np.tile(img, (reps, 1, 1))[:n], np.tile(noise, (reps, 1, 1))[:n], masks, (np.arange(n) % 3).astype(np.int32)


class Parent:
    """the untraced loop through another build of the library (functions of ABI 12 only)"""

    def __init__(self, path, img, noise, masks, mid):
        L = self.L = C.CDLL(path)
        self.ctx = C.c_void_p()
        vp = C.c_void_p
        L.pnp_ctx_create.argtypes = [C.c_int] * 4 + [C.POINTER(vp)]
        L.pnp_synthesize_problem.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int]
        L.pnp_admm_cnc_run.argtypes = [vp, C.c_int] + [C.c_double] * 4
        L.pnp_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
        for f in (L.pnp_init_state, L.pnp_timer_start, L.pnp_prepare_loops, L.pnp_ctx_destroy):
            f.argtypes = [vp]
        assert L.pnp_ctx_create(0, 256, 256, len(img), C.byref(self.ctx)) == 0
        assert L.pnp_synthesize_problem(self.ctx, img.ctypes.data, noise.ctypes.data, 1, masks.ctypes.data, mid.ctypes.data, len(img), len(masks), 0) == 0
        assert L.pnp_init_state(self.ctx) == 0 and L.pnp_prepare_loops(self.ctx) == 0
        self.abi = L.pnp_abi_version()

    def run(self):
        L, ms = self.L, C.c_float()
        assert L.pnp_init_state(self.ctx) == 0 and L.pnp_timer_start(self.ctx) == 0
        assert L.pnp_admm_cnc_run(self.ctx, ITERS, *CNC) == 0 and L.pnp_timer_stop(self.ctx, C.byref(ms)) == 0
        return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import torch
    img, noise, masks, mid = problem(B)
    gt = torch.from_numpy(np.round(img * 255).astype(np.uint8)).cuda()
    parent = Parent(a.parent_lib, img, noise, masks, mid) if a.parent_lib else None
    arms = [('untraced', {}), ('every=10', dict(trace_every=10)), ('every=10 + gt', dict(trace_every=10, gt=gt)),
            ('every=1', dict(trace_every=1)), ('every=1 + gt', dict(trace_every=1, gt=gt))]
    ms = {name: [] for name, _ in arms}
    ms['parent untraced'] = []
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, masks, mid)
        eng.init_state()
        eng.prepare_loops()
        print('path %s, %d slices x %d iterations of ADMM_CNC, %d alternating rounds; ms per run (HIP events), best / median' % (eng.path_name, B, ITERS, a.rounds))
        for r in range(a.rounds + 1):                                      # round 0 warms every arm up
            for name, kw in arms:
                eng.init_state()
                eng.timer_start()
                eng.admm_cnc(ITERS, *CNC, **kw)
                t = eng.timer_stop()
                if r:
                    ms[name].append(t)
            if parent and r:
                ms['parent untraced'].append(parent.run())
            elif parent:
                parent.run()
        base = np.median(ms['untraced'])
        for name, v in ms.items():
            if v:
                print('  %-16s best %8.3f  median %8.3f  (%+6.2f %% of untraced, %.0f it/s)' % (name, min(v), np.median(v), 100 * (np.median(v) / base - 1),
                                                                                              ITERS / np.median(v) * 1e3))
        if parent:
            print('  parent library: ABI %d' % parent.abi)
        # the reduction alone, natural order, on caller tensors
        dev = torch.device('cuda', 0)
        t4 = [torch.rand((B, 256, 256), device=dev) for _ in range(4)]
        out = torch.zeros((7, B), dtype=torch.float64, device=dev)
        n = 256 * 256
        for label, g, per in (('without gt', None, 16), ('with gt', gt, 17)):
            for rep in range(3):
                eng.residuals(*t4, gt=g, out=out)
            eng.timer_start()
            for rep in range(50):
                eng.residuals(*t4, gt=g, out=out)
            t = eng.timer_stop() / 50
            print('pnp_residuals %s, %d slices: %.4f ms per launch, %d N bytes by design = %.1f MB -> %.0f GB/s' % (
                label, B, t, per, per * n * B / 1e6, per * n * B / t / 1e6))
    gbs = C.c_double()
    _lib.check(_lib.lib().pnp_calibrate_stream(0, B, 1.0, C.byref(gbs)))
    print('pnp_calibrate_stream, %d slices: %.0f GB/s' % (B, gbs.value))
    img1, noise1, masks1, mid1 = problem(1)
    with P.Engine(256, 256, Bmax=1) as eng:
        eng.synthesize(img1, noise1, masks1, mid1)
        eng.init_state()
        res = {}
        for name, kw in (('untraced', {}), ('every=1', dict(trace_every=1)), ('every=1, tol=1e-9', dict(trace_every=1, tol=1e-9))):
            v = []
            for rep in range(12):
                eng.init_state()
                eng.timer_start()
                eng.admm_cnc(50, *CNC, **kw)
                v.append(eng.timer_stop())
            res[name] = np.median(v[2:])
        print('one slice, 50 iterations of ADMM_CNC (%s path), ms per solve, median of 10: %s' % (
            eng.path_name, ', '.join('%s %.3f' % kv for kv in res.items())))


if __name__ == '__main__':
    main()
