"""Multi-coil (SENSE) data consistency: what the batched CG x-step reaches on the card.

    python profiles/coils_rate.py [--batch 512] [--coils 4 8] [--iters 10]      -> one JSON line per case

Per case (B slices of 256 x 256, C coils, ADMM_CNC preset, cg_iters = 3; HIP events, warm, best of three after a warm-up):
  ms_per_admm_it   one ADMM iteration (x-step + pixel prox) of pnp_admm_cnc_run
  ms_xstep[k]      pnp_dc_step with cg_iters = k, k = 1, 2, 3;  ms_cg_it = (ms_xstep[3] - ms_xstep[1]) / 2: one more CG iteration = one
                   application of G (three launches) plus the two update kernels.  G ALONE has no entry point and is not timed alone
  ms_A_AH          pnp_A followed by pnp_AH: G's transforms with other ends (four launches; the work array moves five times, not four)
  gbs_design       the bytes by design of the x-step -- (1 + cg_iters) applications of G, each moving the [B][C][H][W] complex work
                   array four times; maps, p, Gp and the update kernels' traffic NOT counted -- over ms_xstep[3]
  gbs_stream       pnp_calibrate_stream on the same card (512 slices of 256 KiB, the slice-resident loop's access shape)
  ms_xstep_torch   the same x-step composed from the calls a user had before: pnp_fft2_fwd / pnp_fft2_inv on B * C slices plus torch
                   elementwise multiplies and sums, scalars kept on the device;  ratio = ms_xstep_torch / ms_xstep[3]
The last case is ONE slice with 8 coils: the latency figure."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import torch                                          # noqa: E402
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib, utils_pnp as U  # noqa: E402
import multicoil_oracle as M                          # noqa: E402

H = W = 256
REO = 0.05


def best_of(eng, fn, reps=3):
    fn()
    eng.sync()
    best = None
    for _ in range(reps):
        eng.timer_start()
        fn()
        ms = eng.timer_stop()
        best = ms if best is None else min(best, ms)
    return best


def torch_xstep(eng2, S, m, aty, z, w, la2, iters, B, Cn):
    """the x-step from pnp_fft2_fwd / pnp_fft2_inv on B * C slices and torch elementwise operations"""
    buf = torch.empty((B, Cn, H, W), dtype=torch.complex64, device='cuda')

    def G(p):
        torch.mul(S[None], p[:, None], out=buf)
        eng2.fft2(torch.view_as_real(buf), torch.view_as_real(buf), B * Cn)
        buf.mul_(m)
        eng2.ifft2(torch.view_as_real(buf), torch.view_as_real(buf), B * Cn)
        return (S.conj()[None] * buf).sum(1) + la2 * p

    dot = lambda a, b: (a.conj() * b).real.sum((1, 2), keepdim=True)
    xh = (z - w).to(torch.complex64)
    r = aty + la2 * xh - G(xh)
    p = r.clone()
    rr = dot(r, r)
    for _ in range(iters):
        Gp = G(p)
        alpha = rr / dot(p, Gp)
        xh = xh + alpha * p
        r = r - alpha * Gp
        rn = dot(r, r)
        p = r + (rn / rr) * p
        rr = rn
    return xh.real.abs()


def run(B, Cn, iters):
    S = M.coil_maps(Cn, H, W, Cn)
    m = M.mask(0, H, W)
    imgs = np.stack([M.phantom(b % 8, H, W) for b in range(B)])
    out = dict(H=H, W=W, B=B, C=Cn, cg_iters=3)
    with P.Engine(H, W, Bmax=B) as eng:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.set_coils(S, 3)
        eng.synthesize(imgs, np.zeros((H, W), np.complex64), m)
        eng.init_state()
        out['path'], out['launches_per_iteration'] = eng.path_name, eng.kernels_per_iteration
        out['ms_per_admm_it'] = round(best_of(eng, lambda: eng.admm_cnc(iters, 0.45, 0.5, REO, 64)) / iters, 4)
        eng.init_state()
        z = torch.empty((B, H, W), dtype=torch.float32, device='cuda')
        w = torch.empty_like(z)
        x = torch.empty_like(z)
        eng.get_state(z, w)
        xs = {}
        for k in (1, 2, 3):
            _lib.check(eng._L.pnp_set_cg(eng._ctx, k))
            xs[k] = best_of(eng, lambda: eng.dc_step(z, w, x, REO))
        out['ms_xstep'] = {k: round(v, 4) for k, v in xs.items()}
        out['ms_cg_it'] = round((xs[3] - xs[1]) / 2, 4)
        kk = torch.empty((B, Cn, H, W), dtype=torch.complex64, device='cuda')
        img_d = torch.empty((B, H, W), dtype=torch.complex64, device='cuda')
        out['ms_A_AH'] = round(best_of(eng, lambda: (eng.A(z, torch.view_as_real(kk)), eng.AH(torch.view_as_real(kk), torch.view_as_real(img_d)))), 4)
        work_bytes = B * Cn * H * W * 8
        out['gb_design_xstep'] = round(4 * 4 * work_bytes / 1e9, 3)
        out['gbs_design'] = round(4 * 4 * work_bytes / 1e9 / (xs[3] * 1e-3), 1)
        x_ref = x.clone()
        aty = U.AH(eng, torch.from_numpy(eng.download_y()).cuda())
        del kk
    with P.Engine(H, W, Bmax=B * Cn) as eng2:
        eng2.set_stream(torch.cuda.current_stream().cuda_stream)
        Sd, md = torch.from_numpy(S.astype(np.complex64)).cuda(), torch.from_numpy(m.astype(np.float32)).cuda()
        la2 = 1.0 / 2.0 / REO
        res = {}
        ms = best_of(eng2, lambda: res.__setitem__('x', torch_xstep(eng2, Sd, md, aty, z, w, la2, 3, B, Cn)))
        out['ms_xstep_torch'] = round(ms, 4)
        out['ratio_torch_over_hip'] = round(ms / xs[3], 2)
        out['torch_vs_hip_rel_l2'] = float((res['x'] - x_ref).norm() / x_ref.norm())
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--coils', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    gbs = C.c_double(0)
    _lib.check(_lib.lib().pnp_calibrate_stream(0, 512, 1.0, C.byref(gbs)))
    cases = [(a.batch, c) for c in a.coils] + [(1, 8)]
    for B, Cn in cases:
        r = run(B, Cn, a.iters)
        r['gbs_stream'] = round(gbs.value, 1)
        print(json.dumps(r), flush=True)
