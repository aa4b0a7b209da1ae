"""PnP denoisers on complex images: what the complex plug-and-play loop costs over the real coil loop on the card.

    python profiles/pnp_complex_rate.py [--batch 64] [--coils 8] [--iters 5] [--calls 30] [--out profiles/pnp_complex_rate.txt]

B slices of 256 x 256, C coils, cg_iters = 3, float; FFDNet (seeded weights: the time does not depend on them) on cnn_backend='hip_f16x3';
the iteration of PNP_ADMM_L1_D at its FFDNet preset (reo = 0.25).  HIP events (the library's timer on torch's stream), warm, best of
three, every figure taken alternately in one process: real / modulus / parts / real / ...
  ms_it             one PnP iteration: x-step + the denoiser step + the dual update, per mode
  ms_xstep, ms_cnn  its parts alone: pnp_dc_step[_cx]; the network on B slices (real, 'modulus') and on 2 B ('parts')
  ms_glue           each glue kernel alone (best of three windows of `calls` calls, per call), with its bytes per pixel by design and the
                    rate that gives, against pnp_calibrate_stream on the same card.  The windows call one kernel back to back on the same
                    arrays (32 MiB per complex array at the defaults): what the last-level cache keeps between calls is in these rates
One JSON line, printed and written to --out.
--real-only: the real coil iteration alone, through calls the parent commit has too: copied into a built checkout of the parent and run
there, it times the parent's loop (one process per tree, in the order parent / this / parent / this)."""
import argparse
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                          # noqa: E402
import pnp_admm_cnc_mri_amd as P                      # noqa: E402
from pnp_admm_cnc_mri_amd import _lib, denoisers as D # noqa: E402
from complex_rate import alternate, scene             # noqa: E402

H = W = 256
REO = 0.25
# bytes per pixel by design, b null / b given (kernels_pnp_cx.hip); the join of 'parts' does not read a, b
BYTES = {'den_in': {'modulus': (12, 20), 'parts': (16, 24)}, 'den_out': {'modulus': (20, 28), 'parts': (16, 16)},
         'den_out_dual': {'modulus': (52, 60), 'parts': (48, 48)}, 'combine_cx': 40}


def denoiser(dev):
    net = D.build('ffdnet_gray')[0]
    net.load_state_dict(D.seeded_state_dict(net, 11))
    net.eval()
    return D.Denoiser('ffdnet_gray', net, 15, backend='hip_f16x3', shape=(H, W)).to(dev)


def engine(B, S, m, y, cx):
    e = P.Engine(H, W, Bmax=B)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.set_coils(S, 3)
    if cx:
        e.set_image_mode('complex')
    e.upload(y, m)
    e.init_state()
    st = SimpleNamespace()
    dt = torch.complex64 if cx else torch.float32
    st.z, st.w, st.t = (torch.empty((B, 1, H, W), dtype=dt, device='cuda') for _ in range(3))
    e.get_state(st.z, st.w)
    st.x = st.z.clone()
    return e, st


def measurements(B, Cn):
    S, m, imgs = scene(B, Cn)
    with P.Engine(H, W, Bmax=B) as e:
        e.set_coils(S, 3)
        e.synthesize(imgs, np.zeros((H, W), np.complex64), m)
        return S, m, e.download_y()


def real_iteration(e, den, st, i):
    e.dc_step(st.z, st.w, st.x, REO)
    e.add(st.x, st.w, st.t)
    den(st.t, i, out=st.z)
    e.dual_clamp(st.x, st.z, st.w)


def real_only(B, Cn, iters):
    S, m, y = measurements(B, Cn)
    den = denoiser('cuda')
    with torch.no_grad():
        e, st = engine(B, S, m, y, False)
        with e:
            ms = alternate({'real': (e, lambda: [real_iteration(e, den, st, i) for i in range(iters)])})['real']
    tree = os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return dict(H=H, W=W, B=B, C=Cn, cg_iters=3, tree=tree, ms_it_real=round(ms / iters, 4))


def main(B, Cn, iters, calls):
    from pnp_admm_cnc_mri_amd import solvers_pnp as SP
    S, m, y = measurements(B, Cn)
    den = denoiser('cuda')
    out = dict(H=H, W=W, B=B, C=Cn, cg_iters=3, cnn='ffdnet_gray on hip_f16x3', gain=0.5)
    px = B * H * W
    with torch.no_grad():
        er, sr = engine(B, S, m, y, False)
        ec, sc = engine(B, S, m, y, True)
        with er, ec:
            glue = {mode: SP._Complex(torch, ec, sc, mode, 0.5) for mode in ('modulus', 'parts')}

            def cx_iteration(mode):
                def run():
                    for i in range(iters):
                        ec.dc_step(sc.z, sc.w, sc.x, REO)
                        glue[mode].denoise_dual(den, i, sc.x, sc.w, sc.x, sc.z, sc.w)
                return run

            r = alternate(dict({'real': (er, lambda: [real_iteration(er, den, sr, i) for i in range(iters)])},
                               **{mode: (ec, cx_iteration(mode)) for mode in glue}))
            out['ms_it'] = {k: round(v / iters, 4) for k, v in r.items()}
            r = alternate({'real': (er, lambda: er.dc_step(sr.z, sr.w, sr.x, REO)), 'complex': (ec, lambda: ec.dc_step(sc.z, sc.w, sc.x, REO))})
            out['ms_xstep'] = {k: round(v, 4) for k, v in r.items()}
            r = alternate({'B': (ec, lambda: den(glue['modulus'].p, 0, out=glue['modulus'].q)), '2B': (ec, lambda: den(glue['parts'].p, 0, out=glue['parts'].q))})
            out['ms_cnn'] = {k: round(v, 4) for k, v in r.items()}
            a, b, s = sc.x, sc.w, sc.t
            pairs = {}
            for mode, g in glue.items():
                for tag, bb in (('', None), ('+b', b)):
                    pairs['den_in %s%s' % (mode, tag)] = (ec, lambda g=g, bb=bb, mode=mode: [ec.cx_den_in(a, bb, g.p, mode, 0.5) for _ in range(calls)])
                    pairs['den_out %s%s' % (mode, tag)] = (ec, lambda g=g, bb=bb, mode=mode: [ec.cx_den_out(g.q, a, bb, s, mode, 0.5) for _ in range(calls)])
                    pairs['den_out_dual %s%s' % (mode, tag)] = (ec, lambda g=g, bb=bb, mode=mode: [ec.cx_den_out_dual(g.q, a, bb, sc.x, sc.z, sc.w, mode, 0.5)
                                                                                                  for _ in range(calls)])
            pairs['combine_cx'] = (ec, lambda: [ec.cnc_combine(sc.z, sc.x, sc.w, s, sc.t, 0.9, 1.35, 0.45, 0.3) for _ in range(calls)])
            pairs['dual_clamp (real)'] = (er, lambda: [er.dual_clamp(sr.x, sr.z, sr.w) for _ in range(calls)])
            r = alternate(pairs)
            out['ms_glue'] = {}
            for name, ms in r.items():
                kern, _, rest = name.partition(' ')
                nbytes = 24 if kern == 'dual_clamp' else BYTES[kern] if kern == 'combine_cx' else BYTES[kern][rest.split('+')[0]][rest.endswith('+b')]
                out['ms_glue'][name] = dict(ms=round(ms / calls, 4), bytes_per_pixel=nbytes, gbs=round(nbytes * px / 1e9 / (ms / calls * 1e-3), 1))
    out['ratio_over_real'] = {k: round(out['ms_it'][k] / out['ms_it']['real'], 3) for k in ('modulus', 'parts')}
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--coils', type=int, default=8)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'pnp_complex_rate.txt'))
    ap.add_argument('--real-only', action='store_true', help='the real coil iteration alone (also runs from a checkout of the parent commit)')
    a = ap.parse_args()
    if a.real_only:
        print(json.dumps(real_only(a.batch, a.coils, a.iters)), flush=True)
        sys.exit(0)
    gbs = C.c_double(0)
    _lib.check(_lib.lib().pnp_calibrate_stream(0, 512, 1.0, C.byref(gbs)))
    res = main(a.batch, a.coils, a.iters, a.calls)
    res['gbs_stream'] = round(gbs.value, 1)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
