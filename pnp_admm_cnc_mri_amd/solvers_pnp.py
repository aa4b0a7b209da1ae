"""Plug-and-play solver entry points with the reference's signatures:

    PNP_ADMM_L1_D(model_name, mask, noises, **opts)                 -> out            (S3:77-337)
    PNP_ADMM_CNC_D(model_name, mask, noises, **opts)                -> (out, psnr1)   (S6:79-351)
    PNP_ADMM_CNC_DnCNN(model_name1, model_name2, mask, noises, **o) -> (out, psnr1)   (S6:372-567)

(S3 = "【3】PNP_ADMM_L1_D  .py", S6 = "【6】PNP_ADMM_CNC_D .py".)  The x-update runs in the HIP
engine (pnp_dc_step on torch's current stream), the denoiser is a PyTorch-ROCm module, the
pointwise glue (S6:301, 305-308) runs in HIP kernels on the tensors' device pointers.  State never
leaves the device; what the reference's host<->device marshalling does to the numbers is kept:
float32 state, |z| and |w| (no-ops once clamped), clamp(0,1) of x, z and w after every iteration.

Extra keyword arguments (all optional): images=, y=, mask_id=, testsets=, testset_name=, results=,
save_E=, device=, return_info=  as in solvers.py, plus
    model_zoo='model_zoo'   directory of KAIR .pth files (S6:107-109)
    model= / model2=        an nn.Module (or state_dict) instead of a file
    cnn_batch=None          slices per CNN forward (activation memory).  None: 64 -- 256 (of 256 x 256; the same pixel count for larger slices) for
                            the plain stacks on the HIP backends, whose layers are short launches at 64 (denoisers.Denoiser)
    cnn_dtype=None          None = float32 (parity); 'bf16'/'fp16' = autocast throughput mode, off parity
    miopen_find='auto'      'auto': torch.backends.cudnn.benchmark is switched on around the CNN forward passes of conv batches
                            of >= 16 images and restored afterwards (a process-global flag: INTEGRATION.md section 4);
                            False / True: leave the caller's setting alone / force a find for every forward
    cnn_backend='auto'      'auto' (default since round 6): 'hip_f16x3' when the device is gfx950, every convolution of the network is one
                            libpnpmri.so takes and the weights lie inside the half range, else 'torch' -- one log line says which and why
                            (denoisers.auto_backend); 'torch': the whole CNN forward in PyTorch-ROCm / MIOpen (north star); 'hip': the 64 -> 64 conv3x3 + ReLU
                            body layers of DnCNN / FDnCNN / FFDNet on libpnpmri.so's fp32 matrix-core kernel (exact f32
                            arithmetic, ~1e-6 from MIOpen's results; first and last layer on its direct kernels);
                            'hip_f16x3': the same with the 64 -> 64 layers in split-half arithmetic on the f16 matrix cores
                            (float32 operands as two halves, exact products, float32 accumulation: float32-level results,
                            2.3 x the float32 kernel's rate; operands must lie within the half range);
                            'hip_f16': opt-in throughput mode, never what 'auto' picks -- halves between the layers, one matrix
                            instruction per product, float32 accumulation: off the 1e-5 parity bar (rel-L2 ~2e-4 from
                            the float32 loop at 10 iterations, PSNR within 0.01 dB); every layer must be one libpnpmri.so takes
    return_device=False     True: `out` is one torch tensor [B,H,W] on the device instead of the 22-slot list of host arrays (solvers.py)
    state0=None, iter_start=0   (PNP_ADMM_CNC_D, PNP_ADMM_L1_D) resume the loop: state0 = (z, w) arrays [B,H,W] as they stand AFTER iteration
                            iter_start, the loop then runs iterations iter_start .. iter_num - 1 (sigma schedule, bank switch and x8 mode of
                            those indices).  With return_info=True the final (z, w) come back as info['z'], info['w'].  What the
                            teacher-forced parity tests use: one iteration from the reference's own state (tests/test_gpu_pnp.py)
    trace_every=0, tol=None convergence trace and residual-based stopping as in solvers.py (info['trace']; needs return_info=True): the rows are
                            reduced on the device from the loop's own tensors after the clamp (S6:306-308) -- Engine.residuals, one launch per
                            check, PSNR / RE on round(255 x) / 255 as the final metric -- and read once after the loop, or once per check with
                            tol.  With state0= / iter_start= the iteration numbers continue from iter_start
    cnn_graph=False         True: a denoiser forward of at most cnn_batch slices is captured once per shape into a HIP graph and replayed
                            (the reference's one-slice calls: a forward is a train of short launches; FFDNet 0.50 -> see DESIGN.md 4.8)
    image='real', cx_denoise='modulus', cx_gain=0.5   (taken by name from the options: not in the signatures, which are pinned as they were)
                            image='complex': the loop keeps the image phase (solvers.py has the rules of the
                            keyword: it needs coils= and measured y=; trace_every= / tol= are refused).  x, z, w are complex, z0 = A^H y,
                            the x-step is the complex CG step, and the REAL network D acts on a complex v through one of two maps
                            (include/pnp_mri.h, "PnP denoisers on complex images"):
                              cx_denoise='modulus'  D(v) = (D(|v|) / |v|) v, (D(0), 0) where |v| = 0: one network pass on B slices, as the
                                                    real loop; phase-equivariant (y e^{i theta} gives x e^{i theta})
                              cx_denoise='parts'    the planes 0.5 + g Re v and 0.5 + g Im v go through D in ONE call on 2 B slices (plane-major,
                                                    so cnn_batch chunks them as ever) and come back as ((Q - 0.5) / g); g = cx_gain, finite and
                                                    > 0.  The network's noise level acts on the planes, i.e. it is scaled by 1 / g on the image;
                                                    twice the network cost; NOT phase-equivariant
                            x, z and w are projected onto the unit disc after every iteration (the complex counterpart of the clamp(0, 1));
                            w is formed from the unclipped x and z.  `out` then holds complex128 [H,W] arrays (return_device=True: one complex64
                            tensor), the metrics and the saved PNGs are on round(255 |x|) / 255, info['image'] = 'complex', info['cx_denoise'],
                            and info['z'], info['w'] -- like state0= -- are complex.  NOT in the reference scripts; 'real' (the default) calls
                            nothing new and is bit for bit what it was; cx_denoise= / cx_gain= other than their defaults are refused with it
"""
import os
from types import SimpleNamespace

import numpy as np

from . import denoisers as D
from . import utils_pnp as pnp
from .engine import CX_DENOISE, TRACE_FIELDS, trace_meets, trace_rows
from .solvers import _Job, coil_options, image_request, log_early_stop, resolve_device, trace_request

PRESETS = {
    # PNP_ADMM_CNC_D(alpha, iter, lambda1, reo, b), S6:569-577
    'PNP_ADMM_CNC_D': {
        'fdncnn': dict(alpha=0.9, iter_num=50, lambda1=0.2, reo=0.45, b=0.3),
        'ffdnet': dict(alpha=0.9, iter_num=50, lambda1=1.35, reo=0.45, b=0.3),
        'ircnn': dict(alpha=0.5, iter_num=50, lambda1=1.3, reo=0.45, b=2),
        'drunet': dict(alpha=1, iter_num=50, lambda1=0.8, reo=0.8, b=0.45),
    },
    'PNP_ADMM_CNC_DnCNN': dict(alpha=1.2, iter_num=50, lambda1=4, reo=0.45, b=0.3),     # S6:571
    # PNP_ADMM_L1_D(iter, reo), S3:339-347
    'PNP_ADMM_L1_D': {
        'fdncnn': dict(iter_num=50, reo=0.25), 'dncnn': dict(iter_num=50, reo=0.15),
        'ffdnet': dict(iter_num=50, reo=0.25), 'ircnn': dict(iter_num=50, reo=0.145),
        'drunet': dict(iter_num=50, reo=0.26),
    },
}


def _load_model(model_name, model, model_zoo, iter_num, noises, x8, cnn_batch, device, cnn_dtype=None, miopen_find='auto',
                cnn_backend='auto', cnn_graph=False, shape=None):
    """The model-zoo switch of S6:129-217: build by name, load weights, eval, no grad, to device.  shape: the slices' (H, W), for
    cnn_backend='auto'."""
    import torch
    net, nlm, scheduled = D.build(model_name)
    bank = None
    if model is None:
        path = os.path.join(model_zoo, model_name + '.pth')
        if not os.path.exists(path):
            raise FileNotFoundError('%s not found (the reference ships no weights, model_zoo/README.md); pass model= '
                                    'or put KAIR weights there' % path)
        model = torch.load(path, map_location='cpu')
    if isinstance(model, torch.nn.Module):
        net = model
    elif D.family(model_name) == 'ircnn' and all(k.isdigit() for k in model.keys()):
        bank = model                                   # dict of 25 state_dicts keyed by str(index), S6:196
        net.load_state_dict(bank['0'] if '0' in bank else next(iter(bank.values())), strict=True)
    else:
        net.load_state_dict(model, strict=True)
    net.eval()
    for _, v in net.named_parameters():
        v.requires_grad = False
    sigmas = None
    if scheduled:                                      # S6:172-174, 191-193
        _, s = pnp.get_rho_sigma(sigma=max(0.255 / 255., nlm), iter_num=iter_num, modelSigma1=49,
                                 modelSigma2=nlm * 255., w=1.0)
        sigmas = torch.tensor(s)
    return D.Denoiser(model_name, net, nlm, sigmas=sigmas, noises=noises, x8=x8, bank=bank, cnn_batch=cnn_batch,
                      cnn_dtype=cnn_dtype, miopen_find=miopen_find, backend=cnn_backend, graph=cnn_graph, shape=shape).to(device)


CX_KEYS = {'image': 'real', 'cx_denoise': 'modulus', 'cx_gain': 0.5}


def cx_keywords(call, opts):
    """image= / cx_denoise= / cx_gain= of a PnP entry point: taken BY NAME out of its options and put beside its other keywords on `call`
    (the signatures of the entry points are pinned as they were, tests/test_solver_surface_cpu.py, so the three are not parameters; they
    are never left in the dict for the loop to ignore: cx_request judges every value)"""
    for k, default in CX_KEYS.items():
        setattr(call, k, opts.pop(k, default))


def cx_request(image, cx_denoise, cx_gain, trace_every, tol):
    """the rules of image= / cx_denoise= / cx_gain= on the PnP entry points that need no _Job: every one a ValueError here, before an engine
    is opened.  -> whether the loop is complex"""
    image_request(image, None, trace_every, tol)
    if cx_denoise not in CX_DENOISE:
        raise ValueError("cx_denoise must be 'modulus' or 'parts' (got %r)" % (cx_denoise,))
    try:
        with np.errstate(over='ignore'):                   # the kernels take the gain as a float: finite and > 0 there too
            gain_ok = bool(np.isfinite(np.float32(cx_gain))) and float(np.float32(cx_gain)) > 0
    except (TypeError, ValueError):
        gain_ok = False
    if not gain_ok:
        raise ValueError('cx_gain must be finite and > 0 (got %r)' % (cx_gain,))
    if image == 'real' and (cx_denoise != 'modulus' or cx_gain != 0.5):
        raise ValueError("cx_denoise= / cx_gain= say how a real denoiser acts on a COMPLEX image: they need image='complex'")
    return image == 'complex'


class _Real:
    """The denoiser step of a real loop: the network on the tensor itself (S6:300-308)."""

    def __init__(self, torch, eng, st):
        self.eng, self.st = eng, st

    def denoise(self, den, i, a, out):
        den(a, i, out=out)

    def denoise_dual(self, den, i, a, b, x, z, w):
        """z = D(a + b) (b None: D(a)), then the dual update and the clamps"""
        if b is not None:
            self.eng.add(a, b, self.st.t)                                         # x + w
            a = self.st.t
        den(a, i, out=z)
        self.eng.dual_clamp(x, z, w)


class _Complex:
    """The denoiser step of a complex loop: the real network between Engine.cx_den_in and cx_den_out[_dual] -- on the modulus, or on the
    two planes of the parts in one call on 2 B slices.  Owns the planes p (in) and q (out)."""

    def __init__(self, torch, eng, st, mode, gain):
        self.eng, self.mode, self.gain = eng, mode, float(gain)
        B, _, H, W = st.z.shape
        self.p = torch.empty(((2 if mode == 'parts' else 1) * B, 1, H, W), dtype=torch.float32, device=st.z.device)
        self.q = torch.empty_like(self.p)

    def denoise(self, den, i, a, out):
        self.eng.cx_den_in(a, None, self.p, self.mode, self.gain)
        den(self.p, i, out=self.q)
        self.eng.cx_den_out(self.q, a, None, out, self.mode, self.gain)

    def denoise_dual(self, den, i, a, b, x, z, w):
        self.eng.cx_den_in(a, b, self.p, self.mode, self.gain)
        den(self.p, i, out=self.q)
        self.eng.cx_den_out_dual(self.q, a, b, x, z, w, self.mode, self.gain)


def _device_state(torch, eng, B, H, W, dev, cx=False):
    """z0 = |ifft2(y)|, w0 = 0 (S6:253-256) copied device-to-device into torch tensors; x starts as
    z0 too (S6:252-253), which is what a zero-iteration call returns.  cx: complex tensors, z0 = A^H y (Engine.get_state in complex mode)."""
    z = torch.empty((B, 1, H, W), dtype=torch.complex64 if cx else torch.float32, device=dev)
    w = torch.empty_like(z)
    eng.get_state(z, w)
    x = z.clone()
    return x, z, w


def _resume(torch, z, w, state0, dev):
    """state0 = (z, w) [B,H,W] host arrays -> the loop's device tensors (float32, as S6:277-285 hands them to the network; complex64 in a
    complex loop)"""
    if state0 is None:
        return
    z0, w0 = state0
    dt = np.complex64 if z.is_complex() else np.float32
    z.copy_(torch.from_numpy(np.ascontiguousarray(z0, dtype=dt)).reshape(z.shape).to(dev))
    w.copy_(torch.from_numpy(np.ascontiguousarray(w0, dtype=dt)).reshape(w.shape).to(dev))


def _finish_pnp(torch, job, eng, x, extra, return_device=False):
    """S6:314-351: img_E = uint8(round(x*255)); metrics on the quantised image.  return_device: `out` is the device tensor [B,H,W]
    (solvers.py), no host copy of the reconstructions.  A complex x: the metrics are on round(255 |x|) / 255."""
    xq = torch.round((x.abs() if x.is_complex() else x) * 255.0) / 255.0
    xs = x.reshape(job.B, job.H, job.W)
    out, psnr1, info = job.finish(eng, xs.clone() if return_device else xs.cpu().numpy(), x_dev=xq.contiguous(), extra=extra)
    return out, psnr1, info


class _Tracer:
    """The convergence trace of a PnP loop: check(k, x, z, z_prev, w) after iteration k (1-based, counted from the very first iteration
    also when the loop resumes at iter_start) reduces the tensors on the device when k is a checked iteration and says whether the
    stopping rule ends the loop there; result() is the trace of Engine._traced.  Off (`on` False): check() does nothing."""

    def __init__(self, torch, eng, job, dev, on, trace_every, tol, iter_start, iter_num):
        """on: what trace_request made of the call"""
        self.on = on
        self.tol, self.iter_num, self.done = tol, iter_num, iter_num if iter_num > iter_start else iter_start
        if not self.on:
            return
        every = 1 if (not trace_every and tol is not None) else int(trace_every)
        self.torch, self.eng, self.job = torch, eng, job
        self.iters = [k for k in range(iter_start + 1, iter_num + 1) if k % every == 0 or k == iter_num]
        self.gt = None if job.gt_u8 is None else torch.from_numpy(job.gt_u8).to(dev)
        self.sums = torch.zeros((max(len(self.iters), 1), len(TRACE_FIELDS), job.B), dtype=torch.float64, device=dev)
        self.rows = 0
        self.converged_at = np.zeros(job.B, np.int32)

    def wants(self, k):
        return self.on and self.rows < len(self.iters) and self.iters[self.rows] == k

    def check(self, k, x, z, z_prev, w):
        """-> True when the loop is to stop after iteration k"""
        if not self.wants(k):
            return False
        row = self.sums[self.rows]
        self.eng.residuals(x, z, z_prev, w, gt=self.gt, quantise=True, out=row)
        self.rows += 1
        if self.tol is None:
            return False
        self.torch.cuda.current_stream(row.device).synchronize()
        met = trace_meets(trace_rows(row.cpu().numpy(), self.job.H * self.job.W, self.gt is not None), self.tol)
        self.converged_at[met & (self.converged_at == 0)] = k
        if met.all():
            self.done = k
        return bool(met.all())

    def result(self):
        trace = trace_rows(self.sums[:self.rows].cpu().numpy(), self.job.H * self.job.W, self.gt is not None)
        trace.update(iter=np.asarray(self.iters[:self.rows], np.int32), iters_done=int(self.done), converged_at=self.converged_at)
        log_early_stop(self.job, trace, self.iter_num, self.tol)
        return trace


def _solve_pnp(c, nets, tag, suffix, psnr_fmt, iter_num, body, scratch, extra='', x8_for=(), keep_z=False):
    """The three PnP solvers around their iteration.  c: the entry point's keywords; nets: [(model_name, model)], one per denoiser to
    load; body(i, eng, dens, st, tracer) -> True to stop: iteration i on the loop's tensors st.x, st.z, st.w and the `scratch` ones
    (names; each like z), with the loaded denoisers `dens` and the denoiser step st.D of the image mode (_Real, or _Complex for
    image='complex': decided here, once).  x8_for: the families that run in x8 mode; keep_z: the body updates z in
    place, so a traced run gets st.z_prev for the z before a checked iteration (None otherwise).  extra: the front of the averages'
    log line.  -> (out, psnr1, info)"""
    import torch
    traced = trace_request(c.trace_every, c.tol, c.return_info)
    cx = cx_request(c.image, c.cx_denoise, c.cx_gain, c.trace_every, c.tol)
    device = resolve_device(c.device)                                  # None: LOCAL_RANK under a process group, else 0
    dev = torch.device('cuda', device)
    x8 = bool(x8_for) and D.family(nets[0][0]) in x8_for
    job = _Job(c.mask, c.noises, tag, suffix, coil_options(c), c.images, c.y, c.mask_id, c.testsets, c.testset_name, c.results, c.save_E,
               device, psnr_fmt=psnr_fmt, image=c.image)
    dens = [_load_model(name, model, c.model_zoo, iter_num, c.noises, x8, c.cnn_batch, dev, c.cnn_dtype, c.miopen_find, c.cnn_backend,
                        c.cnn_graph, (job.H, job.W)) for name, model in nets]
    iter_start = getattr(c, 'iter_start', 0)                           # PNP_ADMM_CNC_DnCNN has neither keyword
    with torch.cuda.device(dev), torch.no_grad(), job.open_engine(torch.cuda.current_stream(dev).cuda_stream) as eng:
        B, H, W = job.B, job.H, job.W
        st = SimpleNamespace()
        st.x, st.z, st.w = _device_state(torch, eng, B, H, W, dev, cx)
        _resume(torch, st.z, st.w, getattr(c, 'state0', None), dev)
        for name in scratch:
            setattr(st, name, torch.empty_like(st.z))
        st.D = _Complex(torch, eng, st, c.cx_denoise, c.cx_gain) if cx else _Real(torch, eng, st)
        tracer = _Tracer(torch, eng, job, dev, traced, c.trace_every, c.tol, iter_start, iter_num)
        st.z_prev = torch.empty_like(st.z) if keep_z and tracer.on else None
        for i in range(iter_start, iter_num):                                 # S6:262, S6:491, S3:255
            if body(i, eng, dens, st, tracer):
                break
        torch.cuda.current_stream(dev).synchronize()
        trace = tracer.result() if tracer.on else None
        out, psnr1, info = _finish_pnp(torch, job, eng, st.x, extra, c.return_device)
        if cx:
            info['cx_denoise'] = c.cx_denoise
        if c.return_info:
            info['z'], info['w'] = st.z.reshape(B, H, W).cpu().numpy(), st.w.reshape(B, H, W).cpu().numpy()
        if tracer.on:
            info['trace'] = trace
    return out, psnr1, info


def _cnc_body(alpha, lambda1, reo, b, bank):
    """-> the iteration PNP_ADMM_CNC_D (S6:262-308) and PNP_ADMM_CNC_DnCNN (S6:491-525) share: s = D1(z), t = their combination,
    z = D2(t), with z and z_new swapped instead of copied.  One loaded denoiser is both D1 and D2; bank: switch its bank first (S6:289-298)."""
    def body(i, eng, dens, st, tracer):
        den1, den2 = dens[0], dens[-1]
        eng.dc_step(st.z, st.w, st.x, reo)                                    # S6:266-271, S6:495-500
        if bank:
            den1.select_bank(i)                                               # S6:289-298
        st.D.denoise(den1, i, st.z, st.s)                                     # S6:300, S6:517
        eng.cnc_combine(st.z, st.x, st.w, st.s, st.t, alpha, lambda1, reo, b)    # S6:301, S6:518
        st.D.denoise_dual(den2, i, st.t, None, st.x, st.z_new, st.w)          # S6:302, S6:519; S6:305-308, S6:522-525
        st.z, st.z_new = st.z_new, st.z
        return tracer.check(i + 1, st.x, st.z, st.z_new, st.w)                # z_new now holds z of the iteration before
    return body


def PNP_ADMM_CNC_D(model_name, mask, noises, images=None, y=None, mask_id=None, testsets='testsets',
                   testset_name='Set1', results='results', save_E=None, device=None, return_info=False,
                   model_zoo='model_zoo', model=None, cnn_batch=None, cnn_dtype=None, miopen_find='auto', cnn_backend='auto', cnn_graph=False, return_device=False,
                   state0=None, iter_start=0, trace_every=0, tol=None, coils=None, coil_id=None, cg_iters=3, virtual_coils=None, noise_cov=None, calib=24, maps_radius=2, maps_power_iters=4, maps_thresh=0.05, maps_method='walsh', maps_kernel=4, maps_sigma=0.02, maps_crop=0.9, **PNP_ADMM_CNC_D_opts):
    """CNC ADMM with a CNN denoiser in place of both soft-thresholds.  Reference: S6:79-351."""
    call = SimpleNamespace(**locals())                     # the keywords above, by name: the first statement
    cx_keywords(call, PNP_ADMM_CNC_D_opts)
    alpha = PNP_ADMM_CNC_D_opts.get('alpha', 0.4)          # S6:85-89
    iter_num = PNP_ADMM_CNC_D_opts.get('iter_num', 46)
    lambda1 = PNP_ADMM_CNC_D_opts.get('lambda1', 2.75)
    reo = PNP_ADMM_CNC_D_opts.get('reo', 1)
    b = PNP_ADMM_CNC_D_opts.get('b', 1)
    out, psnr1, info = _solve_pnp(call, [(model_name, model)], model_name, 'PNP_ADMM_CNC_D', '{:.4f}', iter_num,      # x8 = False, S6:93
                                  _cnc_body(alpha, lambda1, reo, b, bank=True), ('s', 't', 'z_new'), 'alpha: ({:.3f}), '.format(alpha))
    return (out, psnr1, info) if return_info else (out, psnr1)


def PNP_ADMM_CNC_DnCNN(model_name1, model_name2, mask, noises, images=None, y=None, mask_id=None,
                       testsets='testsets', testset_name='Set1', results='results', save_E=None, device=None,
                       return_info=False, model_zoo='model_zoo', model=None, model2=None, cnn_batch=None,
                       cnn_dtype=None, faithful_model2_path=True, miopen_find='auto', cnn_backend='auto', cnn_graph=False, return_device=False,
                       trace_every=0, tol=None, coils=None, coil_id=None, cg_iters=3, virtual_coils=None, noise_cov=None, calib=24, maps_radius=2, maps_power_iters=4, maps_thresh=0.05, maps_method='walsh', maps_kernel=4, maps_sigma=0.02, maps_crop=0.9, **opts):
    """Two DnCNN-17 nets: s = D1(z), z = D2(t).  Reference: S6:372-567.
    `faithful_model2_path`: the reference loads model_path1 into BOTH nets (S6:435) although it logs
    path 2; True reproduces that, False loads model_name2's own weights."""
    call = SimpleNamespace(**locals())                     # the keywords above, by name: the first statement
    cx_keywords(call, opts)
    alpha = opts.get('alpha', 0.4)
    iter_num = opts.get('iter_num', 46)
    lambda1 = opts.get('lambda1', 2.75)
    reo = opts.get('reo', 1)
    b = opts.get('b', 1)
    second = (model_name1, model) if faithful_model2_path and model2 is None else (model_name2, model2)
    out, psnr1, info = _solve_pnp(call, [(model_name1, model), second], model_name1 + '_' + model_name2, 'PNP_ADMM_CNC_DnCNN', '{:.4f}',
                                  iter_num, _cnc_body(alpha, lambda1, reo, b, bank=False), ('s', 't', 'z_new'),
                                  'alpha: ({:.3f}), '.format(alpha))
    return (out, psnr1, info) if return_info else (out, psnr1)


def PNP_ADMM_L1_D(model_name, mask, noises, images=None, y=None, mask_id=None, testsets='testsets',
                  testset_name='Set1', results='results', save_E=None, device=None, return_info=False,
                  model_zoo='model_zoo', model=None, cnn_batch=None, cnn_dtype=None, miopen_find='auto', cnn_backend='auto', cnn_graph=False, return_device=False,
                  state0=None, iter_start=0, trace_every=0, tol=None, coils=None, coil_id=None, cg_iters=3, virtual_coils=None, noise_cov=None, calib=24, maps_radius=2, maps_power_iters=4, maps_thresh=0.05, maps_method='walsh', maps_kernel=4, maps_sigma=0.02, maps_crop=0.9, **PNP_ADMM_L1_D_opts):
    """L1-ADMM with the CNN as the prox: z = D(x + w).  Reference: S3:77-337."""
    call = SimpleNamespace(**locals())                     # the keywords above, by name: the first statement
    cx_keywords(call, PNP_ADMM_L1_D_opts)
    iter_num = PNP_ADMM_L1_D_opts.get('iter_num', 20)      # S3:83-84
    reo = PNP_ADMM_L1_D_opts.get('reo', 0.04)

    def body(i, eng, dens, st, tracer):
        den, = dens
        eng.dc_step(st.z, st.w, st.x, reo)                                    # S3:259-264
        den.select_bank(i)
        if tracer.wants(i + 1):                                               # z is updated in place: a checked iteration keeps the z before it
            st.z_prev.copy_(st.z)
        st.D.denoise_dual(den, i, st.x, st.w, st.x, st.z, st.w)               # z = D(x + w), S3:290; S3:293-296
        return tracer.check(i + 1, st.x, st.z, st.z_prev, st.w)
    out, _, info = _solve_pnp(call, [(model_name, model)], model_name, '_' + model_name + '_PNP_ADMM_L1_D', '{:.2f}',     # file name S3:308, PSNR format S3:320
                              iter_num, body, ('t',) if call.image == 'real' else (), x8_for=('drunet', 'ffdnet'),      # x8 = True (S3:87) survives only there (S3:130,142,181)
                              keep_z=True)
    return (out, info) if return_info else out
