#!/usr/bin/env python3
"""How tests/golden/pnp_l1_ffdnet_trained_it.npz was recorded: PNP_ADMM_L1_D of the UNMODIFIED reference script (S3) with the trained FFDNet
fixture (tests/golden/ffdnet_gray_trained.npz) on 05.png, Q_Random30, at the script's own preset, cut short at 2 / 5 / 10 iterations -- the
L1 twins of the `trained_cnc_d_ffdnet_gray_it{n}` goldens that oracle/make_golden_pnp.py --trained records (that script records the L1 run
at 50 iterations only).  Same harness: oracle/make_golden.py runs the reference's main with --iter_num 1 to obtain its solver function,
masks and options; the calls of record pass iter_num themselves.  CPU only; needs the reference checkout oracle/make_golden.py points to.

usage: python profiles/experiments/record_l1_ffdnet_trained_it.py          (writes the .npz; tests/test_conv_f16_cpu.py pins its content)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import make_golden as MG                # noqa: E402
import make_golden_pnp as MP            # noqa: E402
from pnp_admm_cnc_mri_amd import denoisers as D   # noqa: E402


def main():
    MG.install_shims()
    if not hasattr(np, 'int'):
        np.int = int                    # what the reference was written against (S6:290); the script itself is not touched
    os.chdir(MG.scratch_dir())
    os.makedirs('model_zoo')
    torch.set_num_threads(8)
    meta = json.load(open(os.path.join(MG.GOLD, 'pnp_known.json')))
    for n in ('drunet_gray', 'dncnn_25', 'dncnn_15'):               # what the script's main loads
        net, _, _ = D.build(n)
        torch.save(D.contractive_state_dict(net, D.family(n), meta['known50']['seeds'][n], meta['gains50'][n]), os.path.join('model_zoo', n + '.pth'))
    w = np.load(os.path.join(MG.GOLD, 'ffdnet_gray_trained.npz'))
    net, _, _ = D.build('ffdnet_gray')
    torch.save({k: torch.from_numpy(w[k]) for k in net.state_dict()}, os.path.join('model_zoo', 'ffdnet_gray.pth'))
    g, _, _ = MG.run_script(MP.S3, ['--iter_num', '1'], 'Set1_dn_drunet_gray')
    arrays = {}
    for n_it in (2, 5, 10):
        opts = dict(g['PNP_ADMM_L1_D_opts3'], iter_num=n_it)
        with contextlib.redirect_stdout(io.StringIO()):
            o = g['PNP_ADMM_L1_D']('ffdnet_gray', g['mask'][0], g['noises'], **opts)
        arrays['trained_l1_d_ffdnet_gray_it%d' % n_it] = np.asarray(o[0], np.float32)
        print(n_it, opts, float(arrays['trained_l1_d_ffdnet_gray_it%d' % n_it].astype(np.float64).sum()), flush=True)
    np.savez_compressed(os.path.join(MG.GOLD, 'pnp_l1_ffdnet_trained_it.npz'), **arrays)


if __name__ == '__main__':
    main()
