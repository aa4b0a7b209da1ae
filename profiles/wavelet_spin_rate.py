"""Cost of cycle spinning for the wavelet prox: the prox launches alone (pnp_prox_l1_dual / pnp_prox_cnc_dual on device tensors, HIP
events of the library's timer) and the whole iteration, alternating in one process between
    none   no spin setting            s00   a table of (0, 0)            s11   a table of (1, 1): the worst alignment of the row reads
    K4     four averaged shifts per prox: (0, 0), (1, 1), (3, 5), (7, 7)

    python profiles/wavelet_spin_rate.py [--batch 512] [--transform haar db4] [--levels 3] [--tree DIR] [--variants none]   -> one JSON line per case

Warm, best of three, the variants interleaved inside every repeat.  --tree DIR imports the package from another checkout (a build of the
parent commit): a library without pnp_set_spin runs `none` alone, which is the parent's unshifted prox for the ratios of DESIGN.md 18.

Bytes per pixel by design (float): a shifted prox moves what the unshifted one does, 32 (L1) / 44 (CNC) -- profiles/wavelet_rate.py; of K
averaged shifts the first K - 1 syntheses read c and write (j > 0: also read) the accumulator instead of reading x, w and writing z, w,
the last one reads the accumulator on top: K full analyses, and 8 B per pixel of accumulator traffic per extra shift."""
import argparse
import json
import os
import sys

import numpy as np


def prox_bytes_per_px(kind, K):
    fwd = 12 if kind == 'l1' else 24                      # wavelet_rate.py: analysis 8 + 4 (CNC 12 + 4 + 8)
    if K == 1:
        return fwd + 20
    # synthesis: first c -> acc (8), middle c + acc -> acc (12), last c + acc + x + w -> z, w (24)
    return K * fwd + 8 + 12 * (K - 2) + 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--levels', type=int, default=3)
    ap.add_argument('--calls', type=int, default=10, help='prox calls / iterations per timed region')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--transform', nargs='+', default=['haar', 'db4'])
    ap.add_argument('--kind', nargs='+', default=['l1', 'cnc'])
    ap.add_argument('--variants', nargs='+', default=['none', 's00', 's11', 'K4'],
                    help='`--variants none` times this tree the way a tree without pnp_set_spin is timed: alone')
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import synthetic as S

    B, H, W = a.batch, 256, 256
    img, noise = S.batch(0, 8)
    img, noise = np.tile(img, (B // 8 + 1, 1, 1))[:B], np.tile(noise, (B // 8 + 1, 1, 1))[:B]
    mask = S.reference_masks()['Q_Random30'].astype(np.uint8)
    spun = hasattr(P.Engine, 'set_spin')
    variants = [('none', None, 1)]
    if spun:
        variants += [('s00', [(0, 0)], 1), ('s11', [(1, 1)], 1), ('K4', [(0, 0), (1, 1), (3, 5), (7, 7)], 4)]
    variants = [v for v in variants if v[0] == 'none' or v[0] in a.variants]
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(1)
    x0, z0, w0 = (torch.rand((B, H, W), generator=g).to(dev) * s for s in (1.0, 1.0, 0.3))
    for kind in a.kind:
        prox = ((lambda e, x, z, w: e.prox_l1_dual(x, z, w, 0.0015)) if kind == 'l1'
                else (lambda e, x, z, w: e.prox_cnc_dual(x, z, w, 0.45, 0.5, 0.05, 64)))
        loop = (lambda e, n: e.admm_l1(n, 0.1, 0.015)) if kind == 'l1' else (lambda e, n: e.admm_cnc(n, 0.45, 0.5, 0.05, 64))
        for tr in a.transform:
            with P.Engine(H, W, Bmax=B) as eng:
                eng.synthesize(img, noise, mask)
                eng.set_sparsity(tr, a.levels)
                best = {v[0]: [None, None] for v in variants}

                def setting(table, K):
                    if spun:
                        eng.set_spin(table, K)

                for name, table, K in variants:                       # warm-up: every kernel variant once, the accumulator allocated
                    setting(table, K)
                    z, w = z0.clone(), w0.clone()
                    prox(eng, x0, z, w)
                    eng.init_state()
                    loop(eng, 2)
                    eng.sync()
                for _ in range(a.repeats):
                    for name, table, K in variants:
                        setting(table, K)
                        z, w = z0.clone(), w0.clone()
                        torch.cuda.synchronize()
                        eng.timer_start()
                        for _c in range(a.calls):
                            prox(eng, x0, z, w)
                        ms = eng.timer_stop() / a.calls
                        best[name][0] = ms if best[name][0] is None else min(best[name][0], ms)
                        eng.init_state()
                        eng.timer_start()
                        loop(eng, a.calls)
                        ms = eng.timer_stop() / a.calls
                        best[name][1] = ms if best[name][1] is None else min(best[name][1], ms)
                for name, table, K in variants:
                    gb = prox_bytes_per_px(kind, K) * H * W * B / 1e9
                    print(json.dumps(dict(kind=kind, transform=tr, levels=a.levels, B=B, variant=name, per_prox=K,
                                          launches_per_iteration=eng_plan(eng, spun, table, K),
                                          prox_ms=round(best[name][0], 4), iteration_ms=round(best[name][1], 4),
                                          prox_vs_none=round(best[name][0] / best['none'][0], 3),
                                          iteration_vs_none=round(best[name][1] / best['none'][1], 3),
                                          prox_gb_by_design=round(gb, 4), prox_gb_s_by_design=round(gb / (best[name][0] * 1e-3), 1))),
                          flush=True)


def eng_plan(eng, spun, table, K):
    if spun:
        eng.set_spin(table, K)
    return eng.plan['launches_per_iteration']


if __name__ == '__main__':
    main()
