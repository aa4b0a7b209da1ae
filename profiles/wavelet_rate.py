"""Batched iterations per second of ADMM_L1 / ADMM_CNC with the sparsity penalty on wavelet coefficients (transform=), beside the
pixel-domain loop of the same context on its two-launch path (PNP_SLICE=0), with the bytes the two prox launches move by design.

    PNP_SLICE=0 python profiles/wavelet_rate.py [--batch 512] [--iters 20] [--transform none haar db4] [--levels 3]   -> one JSON line per run

A library without the wavelet entry points (the parent commit) runs `--transform none` alone: the script then touches nothing new.
Under `rocprofv3 --kernel-trace --stats -- python profiles/wavelet_rate.py --iters 5 --repeats 1` the kernel table splits an
iteration into its data-consistency launches and the two prox launches (k_wv_fwd, k_wv_inv).

Bytes per pixel of one prox by design (float): analysis reads x, w (8; CNC also z: 12) and writes c (4; CNC writes and re-reads the raw
coefficients of z first: + 8); synthesis reads c, x, w (12) and writes z, w (8): 32 for L1, 44 for CNC.  The halo re-reads come from L2."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import synthetic as S      # noqa: E402

PROX_BYTES_PER_PX = {'l1': 32, 'cnc': 44}


def rate(B, iters, repeats, kind, transform, levels):
    img, noise = S.batch(0, 8)
    img, noise = np.tile(img, (B // 8 + 1, 1, 1))[:B], np.tile(noise, (B // 8 + 1, 1, 1))[:B]
    mask = S.reference_masks()['Q_Random30'].astype(np.uint8)
    run = (lambda e, n: e.admm_l1(n, 0.1, 0.015)) if kind == 'l1' else (lambda e, n: e.admm_cnc(n, 0.45, 0.5, 0.05, 64))
    with P.Engine(256, 256, Bmax=B) as eng:
        eng.synthesize(img, noise, mask)
        if transform != 'none':
            eng.set_sparsity(transform, levels)
        eng.init_state()
        run(eng, 3)                                       # warm-up, tables
        eng.sync()
        best = None
        for _ in range(repeats):
            eng.init_state()
            eng.timer_start()
            run(eng, iters)
            ms = eng.timer_stop()
            best = ms if best is None else min(best, ms)
        x = eng.x()
        out = dict(kind=kind, transform=transform, levels=levels if transform != 'none' else 0, B=B, iters=iters, path=eng.path_name,
                   launches_per_iteration=eng.plan['launches_per_iteration'], it_s=round(iters / (best * 1e-3), 1),
                   ms_per_it=round(best / iters, 4), x_finite=bool(np.isfinite(x).all()))
        if transform != 'none':
            out['prox_gb_by_design'] = round(PROX_BYTES_PER_PX[kind] * 65536 * B / 1e9, 4)
        return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--levels', type=int, default=3)
    ap.add_argument('--transform', nargs='+', default=['none', 'haar', 'db4'])
    ap.add_argument('--kind', nargs='+', default=['l1', 'cnc'])
    a = ap.parse_args()
    for kind in a.kind:
        for tr in a.transform:
            print(json.dumps(rate(a.batch, a.iters, a.repeats, kind, tr, a.levels)), flush=True)
