"""Is a run split into launches bit-identical to one launch, per path and solver?  Untraced calls only (pnp_admm_*_run), 15 iterations as
one launch, again as one launch, as 15 launches and as 6 + 1 + 8; the cases of tests/test_gpu_trace.py.  Output: trace_split_vs_single.txt
(the two-launch 256 x 256 path is not split-invariant for the last slice of an odd batch)."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np
import pnp_admm_cnc_mri_amd as P
import test_gpu_trace as T
K = 15
for path, H, W, B, prec in T.CASES:
    img, noise, masks, mid = T._batch(P, H, W, B)
    with P.Engine(H, W, Bmax=B, precision=prec) as eng:
        eng.synthesize(img, noise, masks, mid)
        for solver in ('l1', 'cnc'):
            res = {}
            for name, cuts in (('one', [K]), ('one_again', [K]), ('singles', [1] * K), ('6+1+8', [6, 1, 8])):
                eng.init_state()
                for n in cuts:
                    T._run(eng, solver, n)
                res[name] = (eng.x(), *eng.get_state())
            for name in ('one_again', 'singles', '6+1+8'):
                d = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(res[name], res['one'])]
                print('%-7s %dx%d B=%-3d %s %-3s %-9s vs one launch: max|dx|, |dz|, |dw| = %.3e %.3e %.3e' % (path, H, W, B, prec, solver, name, *d), flush=True)
