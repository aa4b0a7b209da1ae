"""Time of the three stages of the coil map estimation (pnp_coil_maps), beside pnp_calibrate_stream on the same card.

    python profiles/coilmaps_rate.py [--batch 512] [--size 256]      -> one JSON line per case, recorded in profiles/coilmaps_rate.txt

Measured, not asserted: B slices of size x size, C = 8 and C = 32, radius 2, 4 power iterations, calibration 24 x 24, float; random
complex data on the device, a full mask.  Warm (one untimed call first), HIP events around each stage inside the library
(pnp_coil_maps_stage_times), best of three calls per stage.  The estimation runs once per problem.

  ms_window / ms_ifft / ms_eig   the stages: window kernel; the context's inverse transform over B C pseudo-slices; eigenvector kernel and
                                 the two support kernels
  gbs_window, gbs_ifft           bytes each stage must move at least (window: one store of B C N complex values, the region's loads are
                                 0.9 % of that; transform: two passes, each reading and writing the array) over its time
  tflops_eig                     16 (2r + 1)^2 C n flops per pixel over ms_eig
  gbs_stream                     pnp_calibrate_stream on the same card (512 slices of 256 KiB, the slice-resident loop's access shape)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib                 # noqa: E402


def case(B, Cn, n, r, iters, gbs_stream):
    import torch
    y = torch.view_as_complex(torch.randn((B, Cn, n, n, 2), dtype=torch.float32, device='cuda'))
    bank = torch.ones((1, n, n), dtype=torch.uint8, device='cuda')
    out = torch.empty_like(y)
    lam = torch.empty((B, n, n), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    with P.Engine(n, n, Bmax=B) as eng:
        eng.coil_maps(y, bank, None, out, lam, B, Cn, 24, r, iters, 0.05)          # warm-up
        eng.coil_maps_stage_times(True)
        best = None
        for _ in range(3):
            eng.coil_maps(y, bank, None, out, lam, B, Cn, 24, r, iters, 0.05)
            ms = eng.coil_maps_stage_times(True)
            best = ms if best is None else [min(a, b) for a, b in zip(best, ms)]
        eng.coil_maps_stage_times(False)
    px = B * n * n
    arr = px * Cn * 8
    flops = 16.0 * (2 * r + 1) ** 2 * Cn * iters * px
    ok = bool(torch.isfinite(torch.view_as_real(out)).all()) and bool(torch.isfinite(lam).all())
    return dict(B=B, C=Cn, H=n, W=n, radius=r, power_iters=iters, ms_window=round(best[0], 3), ms_ifft=round(best[1], 3), ms_eig=round(best[2], 3),
                ms_total=round(sum(best), 3), gbs_window=round(arr / best[0] / 1e6, 1), gbs_ifft=round(4 * arr / best[1] / 1e6, 1),
                tflops_eig=round(flops / best[2] / 1e9, 2), gbs_stream=round(gbs_stream, 1), finite=ok)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--size', type=int, default=256)
    a = ap.parse_args()
    gbs = C.c_double(0)
    _lib.check(_lib.lib().pnp_calibrate_stream(0, 512, 1.0, C.byref(gbs)))
    info = (C.c_int(0), C.c_int(0), C.create_string_buffer(32), C.create_string_buffer(32))
    _lib.check(_lib.lib().pnp_device_info(0, C.byref(info[0]), C.byref(info[1]), info[2], 32, info[3], 32))
    print(json.dumps(dict(card=info[3].value.decode(), compute_units=info[1].value, clock_mhz=info[0].value,
                          command=' '.join(['python'] + sys.argv))), flush=True)
    for Cn in (8, 32):
        print(json.dumps(case(a.batch, Cn, a.size, 2, 4, gbs.value)), flush=True)
