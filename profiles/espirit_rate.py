"""Time of the stages of the ESPIRiT coil map estimation (pnp_espirit_maps), beside pnp_coil_maps and pnp_calibrate_stream on the same card.

    python profiles/espirit_rate.py [--batch 512] [--size 256]      -> one JSON line per case, recorded in profiles/espirit_rate.txt

Measured, not asserted: B slices of size x size at (C, kernel) = (8, 4) and (4, 5) -- 128 and 100 columns of the calibration matrix -- 4
power iterations, calibration 24 x 24, sigma 0.02, float; random complex data on the device, a full mask (a random block has full rank:
the Jacobi sweeps see no structure to profit from).  Warm (one untimed call first), the times taken inside the library
(pnp_espirit_stage_times), best of two calls per stage.  The estimation runs once per problem.

  ms_gram    k_calib_patch_gram over the slices of every pass and the read-back of the Gram matrices (HIP events)
  ms_host    signal space and kernel autocorrelations: cyclic Jacobi on C k^2 columns, in double, at most 16 host threads (host clock)
  ms_pixel   k_espirit_maps and the two support kernels (HIP events); tflops_pixel counts 8 flops per complex multiply-add, C^2 ((2k-1)^2 +
             2k-1 + 1) of them per pixel and power step
  ms_call    the whole call by the host clock: the three stages, the window, the inverse transform and the copies of w
  ms_walsh   pnp_coil_maps (radius 2, the same power iterations) on the same data and engine: its three stages summed
  gbs_stream pnp_calibrate_stream on the same card (512 slices of 256 KiB, the slice-resident loop's access shape)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib                 # noqa: E402


def case(B, Cn, k, n, iters, gbs_stream):
    import torch
    y = torch.view_as_complex(torch.randn((B, Cn, n, n, 2), dtype=torch.float32, device='cuda'))
    bank = torch.ones((1, n, n), dtype=torch.uint8, device='cuda')
    out = torch.empty_like(y)
    lam = torch.empty((B, n, n), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    with P.Engine(n, n, Bmax=B) as eng:
        eng.espirit_maps(y, bank, None, out, lam, B, Cn, 24, k, iters, 0.02, 0.9, 0.05)          # warm-up
        eng.espirit_stage_times(True)
        best, call = None, None
        for _ in range(2):
            t0 = time.perf_counter()
            rank = eng.espirit_maps(y, bank, None, out, lam, B, Cn, 24, k, iters, 0.02, 0.9, 0.05)
            dt = 1e3 * (time.perf_counter() - t0)
            ms = eng.espirit_stage_times(True)
            best = ms if best is None else [min(a, b) for a, b in zip(best, ms)]
            call = dt if call is None else min(call, dt)
        eng.espirit_stage_times(False)
        ok = bool(torch.isfinite(torch.view_as_real(out)).all()) and bool(torch.isfinite(lam).all())
        eng.coil_maps(y, bank, None, out, lam, B, Cn, 24, 2, iters, 0.05)
        eng.coil_maps_stage_times(True)
        eng.coil_maps(y, bank, None, out, lam, B, Cn, 24, 2, iters, 0.05)
        walsh = sum(eng.coil_maps_stage_times(False))
    D = 2 * k - 1
    flops = 8.0 * Cn * Cn * (D * D + D + 1) * iters * B * n * n
    return dict(B=B, C=Cn, kernel=k, columns=Cn * k * k, H=n, W=n, power_iters=iters, ms_gram=round(best[0], 3), ms_host=round(best[1], 1),
                ms_pixel=round(best[2], 3), ms_call=round(call, 1), tflops_pixel=round(flops / best[2] / 1e9, 2), ms_walsh=round(walsh, 3),
                rank_min=int(rank.min()), rank_max=int(rank.max()), gbs_stream=round(gbs_stream, 1), finite=ok)


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
    for Cn, k in ((8, 4), (4, 5)):
        print(json.dumps(case(a.batch, Cn, k, a.size, 4, gbs.value)), flush=True)
