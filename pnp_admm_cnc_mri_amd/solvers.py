"""Solver entry points with the reference's signatures, running on the HIP engine.

    ADMM_L1(mask, noises, **opts)  -> out          ("【1】ADMM_L1.py":29-169)
    ADMM_CNC(mask, noises, **opts) -> out          ("【4】ADMM_CNC .py":31-174)

Same option names, same in-function fallback defaults (S1:35-37, S4:37-41 -- which differ from
the CLI presets S1:171 / S4:176, kept in `PRESETS`), same return value (a list pre-sized 22 whose
first entries are the x iterates, S4:50/138), same log lines (S4:155, S4:168).  What is new is
batching: all images are reconstructed at once by one fused device loop, and synthetic inputs can
bypass the file system through the extra keyword arguments

    images=   [B,H,W] uint8 (or float in [0,1]) ground-truth slices instead of testsets/<Set>
    y=        [B,H,W] complex measurements (skips the synthesis  y = fft2(img)*mask + noises)
    mask_id=  [B] index into `mask` when `mask` is a bank [K,H,W]            (build extension)
    testsets=, testset_name=, results=, save_E=, return_info=
    device=None  HIP device index; None = LOCAL_RANK when a torch.distributed process group is initialised (one process per
              GPU), else 0
    return_device=False   True: `out` is ONE torch tensor [B,H,W] on the device (float32; float64 with precision='f64') instead of the
              22-slot list of host arrays -- no device-to-host copy of the reconstructions; what sharding.solve_sharded hands
              to the final RCCL gather
    precision= 'f32' (default: float32 / complex64 device arithmetic, the throughput path) or 'f64' (the reference's own
               float64 arithmetic, S4:109: every buffer and step in double -- the setting that meets 1e-5 relative L2 on the
               committed 50-iteration CNC presets and beyond)
    trace_every=0, tol=None   convergence trace and residual-based stopping (all five solvers; needs return_info=True, the trace is
              info['trace']): every `trace_every` iterations and after the last one the residuals r_pri = ||x - z||, r_dual =
              ||z_k - z_{k-1}||, the norms of x, z, w and -- with a ground truth -- PSNR / RE of that iteration are recorded per slice
              (Engine._traced has the fields); tol: the run stops after the first check at which every slice has
              max(r_pri, r_dual) <= tol * ||z|| (tol alone: a check every iteration) -- out, metrics, PNGs and log lines are then
              those of iteration trace['iters_done'], and one more log line says so.  Both off: nothing changes
    transform=None, levels=3   (ADMM_L1 and ADMM_CNC only) 'haar', 'db2' or 'db4': the sparsity penalty acts on the coefficients of that
              periodic 2-D DWT with `levels` levels (1..4; H and W divisible by 2^levels) instead of the pixels -- the prox becomes
              Psi^T soft(Psi v), the CNC pair of thresholds is applied coefficient-wise, the coarsest approximation band is never
              thresholded (include/pnp_mri.h, "wavelet-domain sparsity").  NOT in the reference scripts, whose prox acts on the pixels;
              None (the default) is bit for bit what it was.  One extra log line names the transform
    spin=None, spin_average=1, spin_seed=0   (ADMM_L1 and ADMM_CNC only, with transform=) cycle spinning: the prox of every iteration acts
              in a circularly shifted frame, which takes the artefacts of the decimated transform off the 2^levels grid (include/pnp_mri.h,
              "cycle spinning").  spin='random': iter_num * spin_average shifts (sy, sx) drawn from [0, 2^levels) by
              np.random.default_rng(spin_seed) (engine.spin_table); or an array [n, 2] of shifts, used in order and wrapping.
              spin_average = K (1..16): every prox averages K consecutive shifts of the table, at 2 K launches instead of 2.  NOT in
              the reference scripts; None (the default) calls nothing new.  One extra log line names the table and K
    frames=None, temporal_keep_dc=True   (ADMM_L1 and ADMM_CNC only; taken by name from the options: not in the signatures, which are
              pinned as they were) temporal sparsity for a dynamic series: the batch is series of `frames` consecutive slices (2..64, B a
              multiple of it) and the penalty acts on the coefficients of a unitary DFT along time of every pixel's series, coefficient 0
              unpenalised unless temporal_keep_dc=False (include/pnp_mri.h, "temporal sparsity").  One prox launch per iteration; with
              coils= and image='complex' as well; not with transform= / spin=.  NOT in the reference scripts; None (the default) calls
              nothing new.  One extra log line names the series length; info['frames'] is set
    lowrank=None, lowrank_scale=None, lowrank_shift='random', lowrank_seed=0   (ADMM_L1 and ADMM_CNC only, with frames=; taken by name
              from the options like frames=) the LOCALLY LOW-RANK prox for a dynamic series whose contrast changes without a period:
              lowrank = b (2..32, at most min(H, W)) cuts every frame into b x b patches, a patch across the `frames` slices of its series
              is a b^2 x frames matrix, and the prox thresholds its singular values instead of the temporal DFT's coefficients
              (include/pnp_mri.h, "low-rank"): L1 soft-thresholds them, CNC clips those of z and soft-thresholds those of the
              combination.  lowrank_scale (default b / 2) multiplies the threshold and the clip level.  lowrank_shift moves the patch
              grid from one prox step to the next so that no pixel stays at a patch border: 'random' (the default) is a table of 64
              shifts np.random.default_rng(lowrank_seed).integers(0, b, size=(64, 2)), made on the host (engine.lowrank_table); None
              keeps the grid at (0, 0); an array [n, 2] of (sy, sx) in [0, b) is used in order, wrapping.  One prox launch per
              iteration; with coils= as well; real images only (not with image='complex'), not with transform= / spin=, and
              temporal_keep_dc=False does not apply.  A (frames, b, precision, solver) whose patch does not fit the LDS is a
              ValueError.  NOT in the reference scripts; None (the default) calls nothing new.  One extra log line;
              info['lowrank'] = {block, scale, shifts}

    coils=None, coil_id=None, cg_iters=3   (all five solvers) multi-coil (SENSE) data consistency: coils [C,H,W] complex sensitivity maps,
              or a bank [Ks,C,H,W] with coil_id [B] picking each slice's set.  The forward model becomes y_c = mask . fft2(S_c . x):
              y= is [B,C,H,W], or images= are synthesised through the maps (noises [H,W], [C,H,W] or [B,C,H,W]); the x-update is
              `cg_iters` iterations of conjugate gradients warm-started at z - w, the initial state |A^H y|; the z- and w-steps are
              untouched.  3 iterations are enough for maps normalised to sum_c |S_c|^2 = 1 at the presets' reo (1e-7 from the converged
              solve); UNNORMALISED MAPS OR A LARGE reo (the in-function default of ADMM_CNC, 2.75: condition number about 6.5) NEED
              MORE -- info['cg_residual'] has ||r|| / ||rhs|| of the last x-step per slice.  NOT in the reference scripts; None (the
              default) is bit for bit what it was.  One extra log line names C and cg_iters
    virtual_coils=None, noise_cov=None, calib=24   (all five solvers) coil mixing ahead of the solve (coilmix.py; include/pnp_mri.h, "coil
              mixing"): noise_cov [C,C], the channels' noise covariance, prewhitens the data (M_w = L^-1 of its Cholesky factor);
              virtual_coils = n keeps the n virtual coils that carry the most energy of the calib x calib lowest frequencies (SVD coil
              compression: M_c from the Gram matrix of the slices that use a coil set, one matrix per set of the bank).  Both are one
              matrix M = M_c M_w applied once to y and to the maps, after which the solve runs on n coils: `coils` may then have up to
              128 channels, the limit of 32 and check_coils apply to the MIXED count, and the x-step costs n / C of what it did.  They need
              coils= and measured y= (images= may still be given as the ground truth); noise_cov alone means n = C <= 32.  NOT in the
              reference scripts; with all three at their defaults nothing is called and nothing changes.  One extra log line ("coil
              mixing: 64 -> 8 virtual coils, 97.1 % of the calibration energy, prewhitened"); info['coil_mix'] = {M, eigvals, energy}.
              Under sharding.solve_sharded every rank forms its matrices from the slices of its own shard

    coils='estimate', maps_radius=2, maps_power_iters=4, maps_thresh=0.05   (all five solvers) the maps are ESTIMATED from the calib x calib
              calibration region of the measured y= (coilmaps.py; include/pnp_mri.h, "coil sensitivity maps from the calibration
              region"): local dominant eigenvectors of low-resolution coil images over (2 maps_radius + 1)^2 patches by maps_power_iters
              power steps, zero where the local eigenvalue is below maps_thresh^2 of the slice's largest.  One coil set per slice
              (coil_id = arange(B); giving coil_id= is a ValueError); every point of the region must be sampled (ValueError naming the
              first missing one); needs y=, images= may still be the ground truth.  With virtual_coils= / noise_cov= y is mixed first, by
              ONE matrix from the Gram matrices of the whole batch, and the maps are estimated from the MIXED y: up to 128 physical
              channels.  NOT in the reference scripts.  One extra log line; info['coil_maps'] = {calib, radius, power_iters, thresh,
              support: the share of pixels kept per slice}
    maps_method='walsh', maps_kernel=4, maps_sigma=0.02, maps_crop=0.9   (all five solvers, with coils='estimate') maps_method='espirit'
              estimates the maps by ESPIRiT instead (include/pnp_mri.h, "ESPIRiT coil sensitivity maps"): maps_kernel x maps_kernel
              calibration patches, the signal space above maps_sigma of the largest singular value, maps_power_iters power steps on
              the per-pixel operator, kept where its eigenvalue is >= maps_crop and the low-resolution image >= maps_thresh of its
              largest; maps_radius is not used.  C maps_kernel^2 <= 128 (of the MIXED channels: virtual_coils= first).  info['coil_maps']
              gains method, kernel, sigma, crop and rank (per slice).  The default, 'walsh', is bit for bit what it was

    image='real'   (all five solvers) 'complex': the reconstruction keeps the image phase (include/pnp_mri.h, "complex-valued
              images"): x, z, w are complex, z0 = A^H y without the modulus, the x-step returns x^ itself instead of |Re x^|, and the prox
              thresholds the MODULUS of a pixel (or, with transform=, of a wavelet coefficient of the complex image).  Needs coils= (an
              array or 'estimate', with or without virtual_coils= / noise_cov=) and measured y=; spin=, trace_every= and tol= are refused
              with it (ValueError before an engine is opened).  `out` then holds complex128 [H,W] arrays (return_device=True: one complex
              tensor), PSNR / SSIM / RE are taken on |x| when images= is given, info['image'] = 'complex'.  NOT in the reference scripts,
              which reconstruct a real PNG; 'real' (the default) calls nothing new and is bit for bit what it was.  One extra log line.
              The three PnP entry points put their real denoiser on the complex image by cx_denoise= / cx_gain= (solvers_pnp.py)

The PnP entry points (PNP_ADMM_L1_D, PNP_ADMM_CNC_D, PNP_ADMM_CNC_DnCNN) live in solvers_pnp.py.
"""
import logging
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np

from . import coilmaps, coilmix, imageio
from ._lib import PnpError
from .engine import Engine, check_coils, check_image, check_lowrank, check_sparsity, check_temporal, lowrank_table, spin_table

# CLI presets of the reference scripts (positional order differs per script!)
PRESETS = {
    'ADMM_L1': dict(iter_num=50, lambda1=0.1, reo=0.015),                         # S1:171
    'ADMM_CNC': dict(alpha=0.45, iter_num=50, lambda1=0.5, reo=0.05, b=64),       # S4:176
}

# The coil keywords of all five entry points (the docstring above has what they mean).  An entry point takes its keywords ONCE, as
# `call = SimpleNamespace(**locals())`; its driver (_solve here, solvers_pnp._solve_pnp) hands _Job these thirteen as one namespace.
COIL_KEYS = ('coils', 'coil_id', 'cg_iters', 'virtual_coils', 'noise_cov', 'calib', 'maps_radius', 'maps_power_iters', 'maps_thresh',
             'maps_method', 'maps_kernel', 'maps_sigma', 'maps_crop')


def coil_options(call):
    """the COIL_KEYS of an entry point's keywords `call`, as the namespace _Job takes"""
    return SimpleNamespace(**{k: getattr(call, k) for k in COIL_KEYS})


def logger_info(logger_name, log_path):
    """File + stream logger with the reference's format (utils/utils_logger.py:25-44).  Like the
    reference, one logger per name for the whole process; unlike it, a later call with another
    `log_path` moves the file handler there instead of silently logging into the first file."""
    log = logging.getLogger(logger_name)
    formatter = logging.Formatter('%(asctime)s.%(msecs)03d : %(message)s', datefmt='%y-%m-%d %H:%M:%S')
    want = os.path.abspath(log_path)
    files = [h for h in log.handlers if isinstance(h, logging.FileHandler)]
    if not any(h.baseFilename == want for h in files):
        for h in files:
            log.removeHandler(h)
            h.close()
        fh = logging.FileHandler(log_path, mode='a')
        fh.setFormatter(formatter)
        log.addHandler(fh)
    if not any(type(h) is logging.StreamHandler for h in log.handlers):
        sh = logging.StreamHandler()
        sh.setFormatter(formatter)
        log.addHandler(sh)
    log.setLevel(logging.INFO)
    return log


def resolve_device(device=None):
    """The HIP device index an entry point runs on.  An explicit `device=` wins; the default (None) is this process's
    LOCAL_RANK when a `torch.distributed` process group is initialised -- one process per GPU: rank r of an
    8-rank job must not land on the root's card -- and 0 otherwise (the reference's single-process usage, S4:83)."""
    if isinstance(device, (int, np.integer)):
        return int(device)
    if device is not None and getattr(device, 'index', None) is not None:      # torch.device('cuda', 3)
        return int(device.index)
    if device is not None and not hasattr(device, 'index'):
        return int(device)
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return int(os.environ.get('LOCAL_RANK', 0))
    except ImportError:                                               # no torch: the plain solvers need none
        pass
    return 0


class _Job:
    """Everything around the hot loop that ADMM_L1 / ADMM_CNC / the PnP solvers share:
    inputs (S4:83-109), outputs and metrics (S4:138-172)."""

    def __init__(self, mask, noises, tag, suffix, coil, images=None, y=None, mask_id=None, testsets='testsets',
                 testset_name='Set1', results='results', save_E=None, device=None, log=None, ssim=None,
                 psnr_fmt='{:.4f}', precision='f32', image='real'):
        """coil: the COIL_KEYS of the call (coil_options)"""
        # psnr_fmt: S1:150 and S3:320 print the per-image PSNR with two decimals, S4:155 / S6:332 / S6:548 with four
        self.tag, self.suffix, self.psnr_fmt = tag, suffix, psnr_fmt
        if precision not in ('f32', 'f64'):
            raise ValueError("precision must be 'f32' or 'f64'")
        self.precision, self.image, self.testset_name = precision, image, testset_name
        self._check_options(coil, image, mask, mask_id, y)
        name, L_path = testset_name + '_dn_' + tag, os.path.join(testsets, testset_name)
        self._load(images, y, L_path, os.path.join(results, name), save_E)
        self.noises = None if noises is None else np.asarray(noises)
        self.device = resolve_device(device)
        self.ssim = True if ssim is None else ssim
        self._open_log(log, name, L_path)

    def _check_options(self, c, image, mask, mask_id, y):
        """The coil and image rules that need the mask's size (image_request has the rest of image=): every one a ValueError before an
        engine is opened.  Leaves the mask bank, the coil options and what they ask for (mixing, estimate, maps_opts) on the job."""
        if image == 'complex':
            if c.coils is None:
                raise ValueError("image='complex' runs on the multi-coil path: it needs coils= (an array of maps or 'estimate')")
            if y is None:
                raise ValueError("image='complex' reconstructs MEASURED data: it needs y= [B,C,H,W] (the synthesis from images= is "
                                 'real-input; images= may still be given as the ground truth of |x|)')
        mask = np.asarray(mask)
        self.mask_bank = mask[None] if mask.ndim == 2 else mask
        self.H, self.W = self.mask_bank.shape[1:]
        self.mask_id = None if mask_id is None else np.asarray(mask_id, np.int32)
        self.coils, self.cg_iters = c.coils, c.cg_iters
        self.coil_id = None if c.coil_id is None else np.asarray(c.coil_id, np.int32)
        self.virtual_coils, self.noise_cov, self.calib, self.coil_mix = c.virtual_coils, c.noise_cov, c.calib, None
        self.mixing = c.virtual_coils is not None or c.noise_cov is not None
        self.estimate, self.coil_maps = isinstance(c.coils, str), None
        if self.estimate:
            if c.coils != 'estimate':
                raise ValueError("coils must be an array of sensitivity maps or 'estimate' (got %r)" % (c.coils,))
            if y is None:
                raise ValueError("coils='estimate' estimates the maps from MEASURED data: it needs y= [B,C,H,W] (images= may still be given "
                                 'as the ground truth)')
            if c.coil_id is not None:
                raise ValueError("coils='estimate' builds one coil set per slice (coil_id = arange(B)): coil_id= cannot be given with it")
            ys = tuple(np.shape(y))
            if len(ys) not in (3, 4) or ys[-2:] != (self.H, self.W):
                raise ValueError('y must be [B,C,H,W] (or [C,H,W]) with H x W = %d x %d (got shape %s)' % (self.H, self.W, ys))
            c_out = coilmix.plan_y(ys[-3], self.H, self.W, c.virtual_coils, c.noise_cov, c.calib)[1] if self.mixing else int(ys[-3])
            coilmaps.check(c_out, c.calib, c.maps_radius, c.maps_power_iters, c.maps_thresh, self.H, self.W, c.maps_method, c.maps_kernel,
                           c.maps_sigma, c.maps_crop)
            check_coils(np.broadcast_to(np.int8(0), (1, c_out, self.H, self.W)), self.H, self.W, c.cg_iters)
            coilmaps.check_region(self.mask_bank, self.mask_id, c.calib)
            self.maps_opts = dict(calib=int(c.calib), radius=int(c.maps_radius), power_iters=int(c.maps_power_iters),
                                  thresh=float(c.maps_thresh))
            if c.maps_method == 'espirit':                           # 'walsh', the default: the call and the info are what they were
                self.maps_opts.update(method='espirit', kernel=int(c.maps_kernel), sigma=float(c.maps_sigma), crop=float(c.maps_crop))
        elif self.mixing:
            if c.coils is None or y is None:
                raise ValueError('virtual_coils= / noise_cov= mix MEASURED data: they need coils= and y= (the device synthesis from images= '
                                 'is limited to 32 physical coils; images= may still be given as the ground truth)')
            _, c_out, ks = coilmix.plan(c.coils, self.H, self.W, c.virtual_coils, c.noise_cov, c.calib)
            check_coils(np.broadcast_to(np.int8(0), (ks, c_out, self.H, self.W)), self.H, self.W, c.cg_iters)   # the MIXED count
        elif c.coils is not None:
            check_coils(c.coils, self.H, self.W, c.cg_iters)
        elif c.coil_id is not None:
            raise ValueError('coil_id= needs coils=')

    def _load(self, images, y, L_path, E_path, save_E):
        """The ground truth (images=, or the files of testsets/<Set>: S4:62-94) and the measurements y=; where the results go."""
        self.names = None
        self.from_files = images is None and y is None
        self.E_path = E_path
        self.save_E = (True if save_E is None else save_E) if self.from_files else bool(save_E)
        if self.from_files:
            # S4:62-94: list testsets/<Set>, gray decode, modcrop(8), re-quantise
            paths = imageio.get_image_paths(L_path)
            self.names = [os.path.basename(p) for p in paths]
            imgs = [imageio.modcrop(imageio.imread_gray(p), 8) for p in paths]
            for p, im in zip(paths, imgs):
                if im.shape != (self.H, self.W):
                    raise ValueError('%s is %s, mask is %dx%d' % (p, im.shape, self.H, self.W))
            images = np.stack(imgs)
        self.gt_u8 = None
        self.img_L = None
        if images is not None:
            images = np.asarray(images)
            if images.ndim == 2:
                images = images[None]
            if images.dtype != np.uint8:
                images = imageio.single2uint(np.asarray(images, np.float32))
            self.gt_u8 = np.ascontiguousarray(images)
            self.img_L = imageio.requantise(self.gt_u8)                          # S4:91-94
        self.y = None if y is None else np.asarray(y)
        if self.y is not None and self.y.ndim == (2 if self.coils is None else 3):
            self.y = self.y[None]
        self.B = len(self.gt_u8) if self.gt_u8 is not None else len(self.y)

    def _open_log(self, log, name, L_path):
        """the caller's logger, or -- when there are files to read or to write -- the reference's, in the results directory"""
        self.log = log
        if self.log is None and (self.from_files or self.save_E):
            os.makedirs(self.E_path, exist_ok=True)
            self.log = logger_info(name, os.path.join(self.E_path, name + '.log'))
            self.log.info(L_path)

    def say(self, line, *args):
        """one log line (line.format(*args)) where there is a logger"""
        if self.log is not None:
            self.log.info(line.format(*args) if args else line)

    def _mix_coils(self):
        """Coil mixing, once and before an engine exists: y' = M y and, for given maps, S' = M S -- from here on the virtual coils are
        the coils.  With coils='estimate' ONE matrix for the batch; the maps come from y' in _set_coils."""
        if not self.mixing or self.coil_mix is not None:
            return
        self.y, coils, self.coil_mix = coilmix.prepare(self.y, None if self.estimate else self.coils, self.mask_bank, self.mask_id,
                                                       self.coil_id, self.virtual_coils, self.noise_cov, self.calib, self.precision,
                                                       self.device)
        if not self.estimate:
            self.coils = coils
        self.say(coilmix.describe(self.coil_mix))

    def _set_coils(self, eng):
        """The coil side of an open engine, in the order the library needs: estimate the maps (one coil set per slice, from the slice's
        own calibration region), set_coils, then set_image_mode -- set_coils returns the engine to real mode."""
        if self.estimate and self.coil_maps is None:
            self.coils, rank = coilmaps.estimate(self.y, self.mask_bank, self.mask_id, precision=self.precision, engine=eng, return_rank=True,
                                                 **self.maps_opts)
            self.coil_id = np.arange(self.B, dtype=np.int32)
            self.coil_maps = dict(self.maps_opts, support=coilmaps.support_share(self.coils))
            if rank is not None:
                self.coil_maps['rank'] = [int(v) for v in rank]
            self.say(coilmaps.describe(self.coil_maps))
        if self.coils is not None:
            eng.set_coils(self.coils, self.cg_iters)
            self.say('multi-coil data consistency: {:d} coils, {:d} CG iterations per x-step (not in the reference scripts)',
                     eng.C, int(self.cg_iters))
        if self.image == 'complex':
            eng.set_image_mode('complex')
            self.say('complex-valued image: the phase is kept, the prox thresholds the modulus (not in the reference scripts)')

    def open_engine(self, stream=None, transform=None, levels=3, spin=None, spin_average=1, frames=None, keep_dc=True, lowrank=None):
        """stream: HIP stream handle every engine call is ordered on (PnP: torch's current stream),
        set BEFORE the first kernel so upload / synthesis / init and the loop share one queue.
        transform / levels: Engine.set_sparsity (ADMM_L1 / ADMM_CNC); spin / spin_average: the table of spin_request and its group
        size, Engine.set_spin; frames / keep_dc: Engine.set_temporal; lowrank: the dict of lowrank_request, Engine.set_lowrank."""
        self._mix_coils()
        eng = Engine(self.H, self.W, Bmax=self.B, device=self.device, precision=self.precision)
        if transform is not None:
            eng.set_sparsity(transform, levels)
            self.say('sparsity transform: {:s}, {:d} levels (periodic 2-D DWT; not in the reference scripts)', transform, int(levels))
        if spin is not None:
            eng.set_spin(spin, spin_average)
            self.say('cycle spinning: {:d} shifts, {:d} averaged per prox (not in the reference scripts)', len(spin), int(spin_average))
        if frames is not None:
            eng.set_temporal(frames, keep_dc)
            self.say('temporal sparsity: series of {:d} frames, DFT along time{:s} (not in the reference scripts)', int(frames),
                     ', coefficient 0 unpenalised' if keep_dc else '')
        if lowrank is not None:
            eng.set_lowrank(lowrank['block'], lowrank['scale'], lowrank['shifts'])
            self.say('locally low-rank prox: {:d} x {:d} patches across the frames, thresholds x {:g}, {:d} grid shifts (not in the '
                     'reference scripts)', lowrank['block'], lowrank['block'], lowrank['scale'], len(lowrank['shifts']))
        if stream is not None:
            eng.set_stream(stream)
        self._set_coils(eng)
        coil = {} if self.coils is None else {'coil_id': self.coil_id}
        if self.y is not None:
            eng.upload(self.y, self.mask_bank, self.mask_id, **coil)
        else:
            eng.synthesize(self.img_L, self.noises, self.mask_bank, self.mask_id, **coil)        # S4:102
        eng.init_state()                                                                  # S4:103-109
        return eng

    def finish(self, eng, x, x_dev=None, extra=''):
        """S4:138-172: out list, optional PNGs, PSNR/SSIM/RE log lines, averages.  Metrics are
        device reductions on x_dev (None = the ctx's x; PnP passes the uint8-quantised x, S6:314)."""
        A = np.zeros((self.H, self.W), dtype='uint8')
        psnr1 = [0] * max(22, self.B)
        if isinstance(x, np.ndarray):
            out = [A] * max(22, self.B)
            for n in range(self.B):
                out[n] = x[n].astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        else:
            out = x                                                  # return_device=True: the device tensor [B,H,W] itself
            if self.save_E:
                x = x.reshape(self.B, self.H, self.W).cpu().numpy()
        info = OrderedDict(psnr=[], ssim=[], re=[])
        if self.image == 'complex':
            info['image'] = 'complex'
        if self.coils is not None:
            try:
                info['cg_residual'] = list(map(float, eng.cg_residual()))
            except PnpError as e:                                                # iter_num = 0: no x-step has run
                if e.code != -3:
                    raise
                info['cg_residual'] = []
        if self.coil_mix is not None:
            info['coil_mix'] = {k: self.coil_mix[k] for k in ('M', 'eigvals', 'energy')}
        if self.coil_maps is not None:
            info['coil_maps'] = dict(self.coil_maps)
        if self.gt_u8 is not None:
            psnr, re = eng.metrics(x_dev, self.gt_u8)                                     # device reductions
            info['psnr'], info['re'] = list(map(float, psnr)), list(map(float, re))
            if self.ssim:
                info['ssim'] = list(map(float, eng.ssim(x_dev, self.gt_u8)))                  # device, double
            for n in range(self.B):
                psnr1[n] = info['psnr'][n]
                if self.names is not None:
                    self.say('{:s} - PSNR: ' + self.psnr_fmt + ' dB; SSIM: {:.4f} ; RE: {:.4f}.',
                             self.names[n], info['psnr'][n], info['ssim'][n] if self.ssim else float('nan'), info['re'][n])
            ave = lambda v: sum(v) / len(v) if v else float('nan')
            self.say('------> testset_name: ({}), {}Average PSNR:({:.3f})dB, Average ssim : ({:.3f}), Average re : ({:.3f}) )',
                     self.testset_name, extra, ave(info['psnr']), ave(info['ssim']), ave(info['re']))
        if self.save_E:
            os.makedirs(self.E_path, exist_ok=True)
            for n in range(self.B):
                stem = os.path.splitext(self.names[n])[0] if self.names else '%04d' % n
                imageio.imsave_gray(np.abs(x[n]) * 255, os.path.join(self.E_path, stem + self.suffix + '.png'))
        return out, psnr1, info


def trace_request(trace_every, tol, return_info):
    """-> whether the call asks for a trace / a stopping rule; it comes back in `info`, so it needs return_info=True."""
    on = bool(trace_every) or tol is not None
    if on and not return_info:
        raise ValueError('trace_every= / tol= return the trace as info[\'trace\']: pass return_info=True')
    if on and trace_every is not None and int(trace_every) < 0:
        raise ValueError('trace_every must be >= 1 (got %r)' % (trace_every,))
    if tol is not None and not float(tol) > 0:
        raise ValueError('tol must be > 0 (got %r)' % (tol,))
    return on


def image_request(image, spin, trace_every, tol, transform=None, levels=3, precision='f32'):
    """the rules of image= that need no _Job; every one is a ValueError here, before an engine is opened"""
    if image not in ('real', 'complex'):
        raise ValueError("image must be 'real' or 'complex' (got %r)" % (image,))
    if image == 'complex':
        if spin is not None:
            raise ValueError("image='complex' does not run with spin= (cycle spinning is not built for complex images)")
        if trace_every or tol is not None:
            raise ValueError("image='complex' does not run with trace_every= / tol= (the trace is not built for complex images)")
        check_image('complex', transform, levels, precision)


def spin_request(spin, spin_average, spin_seed, transform, levels, iter_num):
    """-> the table [n, 2] int32 of spin= / spin_average= / spin_seed= (engine.spin_table), or None; every rule is a ValueError here,
    before an engine is opened."""
    if spin is None:
        return None
    if transform is None:
        raise ValueError('spin= shifts the frame of the wavelet prox: it needs transform=')
    return spin_table(spin, levels, iter_num, spin_average, spin_seed)


def temporal_keywords(call, opts):
    """frames= / temporal_keep_dc= of ADMM_L1 / ADMM_CNC: read BY NAME from the entry point's options and put beside its other keywords on
    `call` (the signatures are pinned as they were, tests/test_solver_surface_cpu.py, so the two are not parameters)"""
    call.frames = opts.get('frames')
    call.temporal_keep_dc = opts.get('temporal_keep_dc', True)


def temporal_request(frames, transform, spin, B=None):
    """the rules of frames=; every one is a ValueError here, before an engine is opened.  B: the batch, once it is known"""
    if frames is None:
        return
    if transform is not None or spin is not None:
        raise ValueError('frames= (temporal sparsity) does not run with transform= / spin= (a spatial wavelet together with the temporal '
                         'transform is not built)')
    check_temporal(frames, B)


def lowrank_keywords(call, opts):
    """lowrank= / lowrank_scale= / lowrank_shift= / lowrank_seed= of ADMM_L1 / ADMM_CNC: read BY NAME from the entry point's options, as
    temporal_keywords does"""
    call.lowrank = opts.get('lowrank')
    call.lowrank_scale = opts.get('lowrank_scale')
    call.lowrank_shift = opts.get('lowrank_shift', 'random')
    call.lowrank_seed = opts.get('lowrank_seed', 0)


def lowrank_request(c, cnc):
    """-> dict(block, scale, shifts [n, 2] int32) of lowrank= and its companions, or None; every rule is a ValueError here, before an
    engine is opened"""
    if c.lowrank is None:
        return None
    if c.frames is None:
        raise ValueError('lowrank= (locally low-rank prox) needs frames= (the series length)')
    temporal_request(c.frames, c.transform, c.spin)
    if c.image != 'real':
        raise ValueError("lowrank= does not run with image='complex' (real images only)")
    if not c.temporal_keep_dc:
        raise ValueError('lowrank= has no unpenalised coefficient: temporal_keep_dc=False does not apply')
    H, W = np.asarray(c.mask).shape[-2:]
    block = check_lowrank(c.frames, c.lowrank, H, W, None, c.precision, cnc)
    scale = block / 2.0 if c.lowrank_scale is None else c.lowrank_scale
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not 0 < scale < float('inf'):
        raise ValueError('lowrank_scale must be a positive number (got %r)' % (c.lowrank_scale,))
    return dict(block=block, scale=float(scale), shifts=lowrank_table(c.lowrank_shift, block, c.lowrank_seed))


def log_early_stop(job, trace, iter_num, tol):
    """the one extra log line of a run that the stopping rule ended before iter_num"""
    if trace is not None and tol is not None and trace['iters_done'] < iter_num:
        job.say('stopped after iteration {:d} of {:d}: max(r_pri, r_dual) <= {:g} * ||z|| for every slice',
                int(trace['iters_done']), int(iter_num), float(tol))


def _device_x(eng, job):
    """the ctx's x copied device-to-device into a torch tensor that outlives the engine"""
    import torch
    f64 = job.precision == 'f64'
    dt = (torch.complex128 if f64 else torch.complex64) if job.image == 'complex' else (torch.float64 if f64 else torch.float32)
    xt = torch.empty((job.B, job.H, job.W), dtype=dt, device=torch.device('cuda', job.device))
    eng.x(out=xt)
    eng.sync()
    return xt


def _solve(c, tag, suffix, psnr_fmt, iter_num, run):
    """ADMM_L1 / ADMM_CNC around the one call they differ in.  c: the entry point's keywords; run(eng, *trace_args): its whole loop on
    the engine, with trace_args = (trace_every, tol, ground truth) for a traced call and none otherwise."""
    traced = trace_request(c.trace_every, c.tol, c.return_info)
    lowrank = lowrank_request(c, tag == 'ADMM_CNC')
    check_sparsity(c.transform, c.levels, *np.asarray(c.mask).shape[-2:])          # before an engine is opened
    image_request(c.image, c.spin, c.trace_every, c.tol, c.transform, c.levels, c.precision)
    shifts = spin_request(c.spin, c.spin_average, c.spin_seed, c.transform, c.levels, iter_num)
    temporal_request(c.frames, c.transform, c.spin)
    job = _Job(c.mask, c.noises, tag, suffix, coil_options(c), c.images, c.y, c.mask_id, c.testsets, c.testset_name, c.results, c.save_E,
               c.device, psnr_fmt=psnr_fmt, precision=c.precision, image=c.image)
    temporal_request(c.frames, c.transform, c.spin, job.B)
    with job.open_engine(transform=c.transform, levels=c.levels, spin=shifts, spin_average=c.spin_average, frames=c.frames,
                         keep_dc=c.temporal_keep_dc, lowrank=lowrank) as eng:
        trace = run(eng, c.trace_every, c.tol, job.gt_u8) if traced else run(eng)
        log_early_stop(job, trace, iter_num, c.tol)
        x = _device_x(eng, job) if c.return_device else eng.x()      # iter_num = 0: the initial x = |ifft2(y)| (S4:103, 138)
        out, _, info = job.finish(eng, x)
        if traced:
            info['trace'] = trace
        if c.frames is not None:
            info['frames'] = int(c.frames)
        if lowrank is not None:
            info['lowrank'] = lowrank
    return (out, info) if c.return_info else out


def ADMM_L1(mask, noises, images=None, y=None, mask_id=None, testsets='testsets', testset_name='Set1',
            results='results', save_E=None, device=None, return_info=False, precision='f32', return_device=False, trace_every=0, tol=None,
            transform=None, levels=3, coils=None, coil_id=None, cg_iters=3, virtual_coils=None, noise_cov=None, calib=24,
            maps_radius=2, maps_power_iters=4, maps_thresh=0.05, maps_method='walsh', maps_kernel=4, maps_sigma=0.02,
            maps_crop=0.9, spin=None, spin_average=1, spin_seed=0, image='real', **ADMM_L1_opts):
    """ADMM with L1 prox on the MI355X engine.  Reference: "【1】ADMM_L1.py":29-169."""
    call = SimpleNamespace(**locals())                   # the keywords above, by name: the first statement
    temporal_keywords(call, ADMM_L1_opts)
    lowrank_keywords(call, ADMM_L1_opts)
    iter_num = ADMM_L1_opts.get('iter_num', 20)          # S1:35
    lambda1 = ADMM_L1_opts.get('lambda1', 0.04)          # S1:36
    reo = ADMM_L1_opts.get('reo', 0.04)                  # S1:37
    return _solve(call, 'ADMM_L1', '_PDG L1', '{:.2f}', iter_num,                                       # PSNR format S1:150
                  lambda eng, *trace: eng.admm_l1(iter_num, lambda1, reo, *trace))                      # S1:111-126, all slices, on device


def ADMM_CNC(mask, noises, images=None, y=None, mask_id=None, testsets='testsets', testset_name='Set1',
             results='results', save_E=None, device=None, return_info=False, precision='f32', return_device=False, trace_every=0, tol=None,
             transform=None, levels=3, coils=None, coil_id=None, cg_iters=3, virtual_coils=None, noise_cov=None, calib=24,
             maps_radius=2, maps_power_iters=4, maps_thresh=0.05, maps_method='walsh', maps_kernel=4, maps_sigma=0.02,
             maps_crop=0.9, spin=None, spin_average=1, spin_seed=0, image='real', **ADMM_CNC_opts):
    """ADMM with the convex-non-convex z-step.  Reference: "【4】ADMM_CNC .py":31-174."""
    call = SimpleNamespace(**locals())                   # the keywords above, by name: the first statement
    temporal_keywords(call, ADMM_CNC_opts)
    lowrank_keywords(call, ADMM_CNC_opts)
    iter_num = ADMM_CNC_opts.get('iter_num', 4)          # S4:37
    alpha = ADMM_CNC_opts.get('alpha', 0.4)              # S4:38
    lambda1 = ADMM_CNC_opts.get('lambda1', 0.04)         # S4:39
    reo = ADMM_CNC_opts.get('reo', 2.75)                 # S4:40  (reo is 1/beta of the paper)
    b = ADMM_CNC_opts.get('b', 1)                        # S4:41  (b is b^2 of the paper)
    return _solve(call, 'ADMM_CNC', '_ADMM CNC', '{:.4f}', iter_num,
                  lambda eng, *trace: eng.admm_cnc(iter_num, alpha, lambda1, reo, b, *trace))           # S4:115-132
