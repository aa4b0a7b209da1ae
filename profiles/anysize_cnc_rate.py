"""ADMM_CNC batched iterations per second on the generic three-launch iteration, any-size kernels against the fixed-size
generic kernels at 256 x 256 (fast path off), with a bytes-per-iteration estimate of that iteration.

    python profiles/anysize_cnc_rate.py [--batch 64] [--iters 50] [--shape 320x320 ...]      -> one JSON line per shape

Bytes per pixel and iteration of the generic iteration (float): rows forward reads z, w (8) and writes the spectrum (8); the
column pass reads it (8), y (8) and the mask (1) and writes it back (8); rows inverse reads it (8) and z, w (8), writes z, w (8):
65 B.  The estimate counts each array once per pass (the caches neither help nor hurt)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from oracle import admm_oracle as O                   # noqa: E402

BYTES_PER_PX = 65


def rate(H, W, B, iters):
    masks = np.stack([O.synthetic_mask(k, H, W) for k in ('random', 'radial', 'cartesian')]).astype(np.uint8)
    mid = (np.arange(B) % 3).astype(np.int32)
    img = np.stack([O.phantom(b % 8, H, W) for b in range(B)])
    noise = O.kspace_noise(0, H, W).astype(np.complex64)
    with P.Engine(H, W, Bmax=B) as eng:
        eng.set_fast_path(False)
        eng.synthesize(img, noise, masks, mid)
        eng.init_state()
        eng.admm_cnc(5, 0.45, 0.5, 0.05, 64)              # warm-up
        eng.sync()
        best = None
        for _ in range(3):
            eng.init_state()
            eng.timer_start()
            eng.admm_cnc(iters, 0.45, 0.5, 0.05, 64)
            ms = eng.timer_stop()
            best = ms if best is None else min(best, ms)
        x = eng.x()
        its = iters / (best * 1e-3)
        gb = BYTES_PER_PX * H * W * B / 1e9
        return dict(H=H, W=W, B=B, iters=iters, ctx_path=eng.ctx_path, plan_rows=eng.fft_plan(0), plan_cols=eng.fft_plan(1),
                    it_s=round(its, 1), ms_per_it=round(best / iters, 4), gb_per_it_est=round(gb, 4), tb_s_est=round(its * gb / 1e3, 3),
                    x_finite=bool(np.isfinite(x).all()))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--shape', action='append', default=None, help='HxW (repeatable); default: 256x256 320x320 384x384 218x170')
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shape] if a.shape else [(256, 256), (320, 320), (384, 384), (218, 170)]
    for H, W in shapes:
        print(json.dumps(rate(H, W, a.batch, a.iters)), flush=True)
