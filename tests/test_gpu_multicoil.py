"""Multi-coil (SENSE) data consistency on the GPU (pnp_set_coils) against tests/multicoil_oracle.py.

Shapes: the smallest that reach every transform kind and path -- 128 x 128 (radix-2), 140 x 160 (mixed radix on both axes), 131 x 128
(Bluestein on one axis), 256 x 256 (the shape whose fast engines must be bypassed); batches of B = 3 with C = 3, 2 and 1 coils.
Float bars of the operators and of one x-step: 4 x the distance of the oracle's own float32 restatement from its float64 form ON THE SAME
INPUTS (computed here, per case); double: 1e-12.  Loops: 1e-5 in float (the project's bar), 1e-8 in double (tests/test_gpu_f64.py's)."""
import functools
import os

import numpy as np
import pytest

import multicoil_oracle as M
import wavelet_oracle as WO
from conftest import rel_l2, weights_trained

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128, 3), (140, 160, 2), (131, 128, 3), (256, 256, 3)]          # H, W, C
B = 3
MID = np.array([0, 1, 0], np.int32)
C64, C128 = np.complex64, np.complex128


@functools.lru_cache(maxsize=None)
def case(H, W, C):
    """B seeded slices with one set of maps and a bank of two masks; y in float64"""
    S = M.coil_maps(C, H, W, H + C)
    masks = np.stack([M.mask(H, H, W), M.mask(H + 1, H, W)])
    imgs = np.stack([M.phantom(10 * H + b, H, W) for b in range(B)])
    y = np.stack([M.synthesize(imgs[b], S, masks[MID[b]], M.noise(b, C, masks[MID[b]])) for b in range(B)])
    for a in (S, masks, imgs, y):
        a.setflags(write=False)
    return S, masks, imgs, y


@functools.lru_cache(maxsize=None)
def loop_ref(H, W, C, kind, iters=10):
    S, masks, imgs, y = case(H, W, C)
    return np.stack([M.admm(y[b], S, masks[MID[b]], iters, kind) for b in range(B)])


def open_engine(H, W, C, precision='f32', cg_iters=3, upload=True):
    import pnp_admm_cnc_mri_amd as P
    S, masks, imgs, y = case(H, W, C)
    eng = P.Engine(H, W, Bmax=B, precision=precision)
    eng.set_coils(S, cg_iters)
    if upload:
        eng.upload(y, masks, MID)
    return eng


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda', dtype=dtype)          # a copy: the cached inputs are read-only


# ---- 1. operators -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,C', SHAPES)
def test_A_AH_G_against_the_oracle_float(H, W, C):
    """A, A^H and G = A^H A + La2 (composed of the two, as a caller would) on the device against the oracle, each within 4 x the float32
    restatement's own distance; <A x, k> = N <x, A^H k> within the two bars (Cauchy-Schwarz).  The fused G of the x-step (expanding rows,
    masked columns, combining rows with La2 p and the row sums) is what test_one_x_step checks: the ABI has no entry point for G alone."""
    import torch
    from pnp_admm_cnc_mri_amd import utils_pnp as U
    S, masks, imgs, y = case(H, W, C)
    rng = np.random.default_rng(H * W + C)
    k = (rng.standard_normal((B, C, H, W)) + 1j * rng.standard_normal((B, C, H, W))).astype(C64)
    with open_engine(H, W, C) as eng:
        assert eng.path_name == 'coils' and eng.coils == {'C': C, 'Ks': 1, 'cg_iters': 3}
        got_A = U.A(eng, dev(imgs), coils=True)
        got_AH = U.AH(eng, dev(k))
        got_G = U.AH(eng, got_A).cpu().numpy() + np.float32(10.0) * imgs
        torch.cuda.synchronize()
        got_A, got_AH = got_A.cpu().numpy(), got_AH.cpu().numpy()
        with pytest.raises(Exception, match='pnp_Df'):
            U.Df(eng, dev(imgs))
    assert got_A.shape == (B, C, H, W) and got_AH.shape == (B, H, W)
    for b in range(B):
        m = masks[MID[b]]
        ref_A, ref_AH, ref_G = M.A(imgs[b], S, m), M.AH(k[b], S, m), M.G(imgs[b], S, m, 0.05)
        bar_A, bar_AH, bar_G = (4 * M.rel(f32, ref) for f32, ref in ((M.A(imgs[b], S, m, C64), ref_A), (M.AH(k[b], S, m, C64), ref_AH),
                                                                       (M.G(imgs[b], S, m, 0.05, C64), ref_G)))
        eA, eAH, eG = rel_l2(got_A[b], ref_A), rel_l2(got_AH[b], ref_AH), rel_l2(got_G[b], ref_G)
        print('A %.2e (bar %.2e)  AH %.2e (bar %.2e)  G %.2e (bar %.2e)' % (eA, bar_A, eAH, bar_AH, eG, bar_G))
        assert eA <= bar_A and eAH <= bar_AH and eG <= bar_G, (b, eA, bar_A, eAH, bar_AH, eG, bar_G)
        lhs = np.vdot(got_A[b].astype(C128), k[b].astype(C128))
        rhs = H * W * np.vdot(imgs[b].astype(C128), got_AH[b].astype(C128))
        assert abs(lhs - rhs) <= (bar_A + bar_AH) * np.linalg.norm(got_A[b]) * np.linalg.norm(k[b]), (b, lhs, rhs)


@pytest.mark.parametrize('H,W,C', SHAPES)
def test_A_AH_against_the_oracle_double(H, W, C):
    """In double the operators are reached through the problem: synthesis without noise is A (download_y), the initial state is |A^H y|;
    1e-12.  (One x-step in double, hence G: test_one_x_step.)"""
    import pnp_admm_cnc_mri_amd as P
    S, masks, imgs, y = case(H, W, C)
    with P.Engine(H, W, Bmax=B, precision='f64') as eng:
        eng.set_coils(S)
        eng.synthesize(imgs, np.zeros((H, W), C128), masks, MID)
        got_A = eng.download_y()
        eng.upload(y, masks, MID)
        eng.init_state()
        z0, w0 = eng.get_state()
    assert got_A.shape == (B, C, H, W) and not w0.any()
    for b in range(B):
        m = masks[MID[b]]
        assert rel_l2(got_A[b], M.A(imgs[b], S, m)) <= 1e-12
        assert rel_l2(z0[b], np.abs(M.AH(y[b], S, m))) <= 1e-12


# ---- 2. one x-step -------------------------------------------------------------------------------------------------------------------

def _state(H, W, C):
    """a state with a non-trivial dual: z = |A^H y| rounded to float32, w a smooth seeded field a tenth of its size"""
    S, masks, imgs, y = case(H, W, C)
    z = np.stack([M.init_state(y[b], S, masks[MID[b]])[1] for b in range(B)]).astype(np.float32)
    w = (0.1 * z * np.cos(np.arange(W) / 9.0)[None, None, :]).astype(np.float32)
    return z, w


@pytest.mark.parametrize('H,W,C', SHAPES)
@pytest.mark.parametrize('precision', ['f32', 'f64'])
def test_one_x_step(H, W, C, precision):
    """dc_step with cg_iters = 3 against the oracle's x-step (float: Engine.dc_step on device tensors; double, which has no step-wise
    entry points: one loop iteration from the same state); cg_residual() within a factor of 2 of the oracle's, and strictly falling from
    cg_iters = 1 to 3."""
    import torch
    S, masks, imgs, y = case(H, W, C)
    z, w = _state(H, W, C)
    reo = 0.05
    res = {}
    for it in (1, 2, 3):
        with open_engine(H, W, C, precision, it) as eng:
            if precision == 'f32':
                x = torch.empty((B, H, W), dtype=torch.float32, device='cuda')
                eng.dc_step(dev(z), dev(w), x, reo)
                torch.cuda.synchronize()
                got = x.cpu().numpy()
            else:
                eng.set_state(z, w)
                eng.admm_l1(1, 0.1, reo)
                got = eng.x()
            res[it] = eng.cg_residual()
    assert (res[1] > res[2]).all() and (res[2] > res[3]).all(), res
    for b in range(B):
        m = masks[MID[b]]
        aty = M.AH(y[b], S, m)
        ref, rel = M.x_step(z[b], w[b], aty, S, m, reo, 3, residual=True)
        if precision == 'f32':
            y32 = y[b].astype(C64)
            bar = 4 * M.rel(M.x_step(z[b], w[b], M.AH(y32, S, m, C64), S, m, reo, 3, C64), ref)
        else:
            bar = 1e-12
        err = rel_l2(got[b], ref)
        print('%s x-step %.2e (bar %.2e)  residual %.2e (oracle %.2e)' % (precision, err, bar, res[3][b], rel))
        assert err <= bar, (b, err, bar)
        assert rel / 2 <= res[3][b] <= rel * 2, (b, res[3][b], rel)


# ---- 3. ten iterations at the presets --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H,W,C,precision', [s + ('f32',) for s in SHAPES] + [SHAPES[0] + ('f64',), SHAPES[3] + ('f64',)])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_ten_iterations_at_the_presets(H, W, C, precision, kind):
    import pnp_admm_cnc_mri_amd as P
    S, masks, imgs, y = case(H, W, C)
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    out, info = solver(masks, None, y=y, mask_id=MID, coils=S, precision=precision, return_info=True, iter_num=10, **M.O_PRESETS[kind])
    ref = loop_ref(H, W, C, kind)
    bar = 1e-5 if precision == 'f32' else 1e-8
    assert len(info['cg_residual']) == B and all(0 < r < 1e-6 for r in info['cg_residual']), info['cg_residual']
    for b in range(B):
        err = rel_l2(out[b], ref[b])
        print('%s %s %dx%d slice %d: %.2e' % (kind, precision, H, W, b, err))
        assert err <= bar, (b, err)


# ---- 4. one uniform coil is the single-coil solver; coils=None is what it was -------------------------------------------------------

@pytest.mark.parametrize('H,W', [(256, 256), (140, 160)])
@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_one_uniform_coil_equals_the_call_without_coils(H, W, kind):
    """C = 1, S = 1, cg_iters = 1 through coils= is within 1e-5 of the same call without coils after 10 iterations."""
    import pnp_admm_cnc_mri_amd as P
    S, masks, imgs, y = case(H, W, 2)
    y1 = np.stack([(np.fft.fft2(imgs[b]) + M.noise(b, 1, masks[MID[b]])[0]) * masks[MID[b]] for b in range(B)])
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    kw = dict(mask_id=MID, iter_num=10, **M.O_PRESETS[kind])
    plain = solver(masks, None, y=y1, **kw)
    coil = solver(masks, None, y=y1[:, None], coils=np.ones((1, H, W), C64), cg_iters=1, **kw)
    for b in range(B):
        assert rel_l2(coil[b], plain[b]) <= 1e-5, (b, rel_l2(coil[b], plain[b]))


@pytest.mark.parametrize('slice_mode,path', [('1', 'slice'), ('0', 'fused')])
def test_clearing_the_coils_restores_the_fast_paths_bit_for_bit(slice_mode, path, monkeypatch):
    """A 256 x 256 context with coils never enters the slice-resident or two-launch engines ('coils'); set_coils(None) brings back the
    path, the launch plan and every bit of the result of a context that never had coils."""
    import pnp_admm_cnc_mri_amd as P
    monkeypatch.setenv('PNP_SLICE', slice_mode)
    S, masks, imgs, y = case(256, 256, 3)
    y1 = np.stack([np.fft.fft2(imgs[b]) * masks[MID[b]] for b in range(B)])
    runs = []
    for with_coils in (False, True):
        with P.Engine(256, 256, Bmax=B) as eng:
            if with_coils:
                eng.set_coils(S)
                eng.upload(y, masks, MID)
                assert eng.path_name == 'coils' and eng.kernels_per_iteration == 21 and eng.plan['launches_per_iteration'] == 21
                with pytest.raises(Exception, match='pnp_upload_problem_mc'):
                    eng.C = 0
                    eng.upload(y1, masks, MID)                      # the single-coil entry point on a coil context
                eng.set_coils(None)
                with pytest.raises(Exception, match='no problem'):
                    eng.init_state()                                # clearing dropped the problem
                with pytest.raises(Exception, match='pnp_set_coils'):
                    eng.C = 3
                    eng.upload(y, masks, MID)                       # and the _mc entry point needs coils
                eng.C = 0
            eng.upload(y1, masks, MID)
            eng.init_state()
            assert eng.path_name == path
            eng.admm_cnc(10, 0.45, 0.5, 0.05, 64)
            runs.append((eng.x(), eng.kernels_per_iteration))
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][0], runs[1][0])


# ---- 5. / 6. banks, determinism, independence -----------------------------------------------------------------------------------------

def test_banks_determinism_and_independence():
    """Ks = 2 with coil_id = [1, 0, 1] and a mask bank of 2 with mask_id = [0, 1, 1]: the batch equals the three slices solved one by one,
    BIT FOR BIT (no sum depends on the batch or on a slice's place in it), and a second run of the batch equals the first."""
    import pnp_admm_cnc_mri_amd as P
    H, W, C = 131, 128, 3
    bank = np.stack([M.coil_maps(C, H, W, 1), M.coil_maps(C, H, W, 2)])
    cid, mid = np.array([1, 0, 1], np.int32), np.array([0, 1, 1], np.int32)
    _, masks, imgs, _ = case(H, W, C)
    y = np.stack([M.synthesize(imgs[b], bank[cid[b]], masks[mid[b]], M.noise(b, C, masks[mid[b]])) for b in range(B)])
    kw = dict(coils=bank, iter_num=4, **M.O_PRESETS['cnc'])
    first = np.stack(P.ADMM_CNC(masks, None, y=y, mask_id=mid, coil_id=cid, **kw)[:B])
    again = np.stack(P.ADMM_CNC(masks, None, y=y, mask_id=mid, coil_id=cid, **kw)[:B])
    assert np.array_equal(first, again)
    for b in range(B):
        alone = P.ADMM_CNC(masks, None, y=y[b:b + 1], mask_id=mid[b:b + 1], coil_id=cid[b:b + 1], **kw)[0]
        assert np.array_equal(alone, first[b]), b
        ref = M.admm(y[b], bank[cid[b]], masks[mid[b]], 4, 'cnc')
        assert rel_l2(first[b], ref) <= 1e-5, (b, rel_l2(first[b], ref))
    with pytest.raises(Exception, match='coil_id'):
        P.ADMM_CNC(masks, None, y=y, mask_id=mid, coil_id=[0, 2, 1], **kw)


# ---- 7. / 8. composition with the wavelet prox and with the trace -----------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['l1', 'cnc'])
def test_composition_with_the_wavelet_prox(kind):
    import pnp_admm_cnc_mri_amd as P
    H, W, C = SHAPES[0]
    S, masks, imgs, y = case(H, W, C)
    pr = M.O_PRESETS[kind]
    if kind == 'l1':
        prox = lambda x, z, w: WO.prox_l1(x, z, w, pr['reo'] * pr['lambda1'], 'haar', 2)
    else:
        prox = lambda x, z, w: WO.prox_cnc(x, z, w, pr['alpha'], pr['lambda1'], pr['reo'], pr['b'], 'haar', 2)
    solver = P.ADMM_L1 if kind == 'l1' else P.ADMM_CNC
    out = solver(masks, None, y=y, mask_id=MID, coils=S, transform='haar', levels=2, iter_num=5, **pr)
    for b in range(B):
        ref = M.admm(y[b], S, masks[MID[b]], 5, kind, prox=prox)
        assert rel_l2(out[b], ref) <= 1e-5, (b, rel_l2(out[b], ref))


def test_composition_with_the_trace():
    import pnp_admm_cnc_mri_amd as P
    H, W, C = SHAPES[0]
    S, masks, imgs, y = case(H, W, C)
    out, info = P.ADMM_CNC(masks, None, y=y, mask_id=MID, coils=S, iter_num=5, trace_every=2, return_info=True, **M.O_PRESETS['cnc'])
    tr = info['trace']
    assert list(tr['iter']) == [2, 4, 5] and tr['iters_done'] == 5
    for b in range(B):
        _, rec = M.admm(y[b], S, masks[MID[b]], 5, 'cnc', trace=(2, 4, 5))
        for c, it in enumerate((2, 4, 5)):
            x, z, zp, w = rec[it]
            for name, want in (('r_pri', np.linalg.norm(x - z)), ('r_dual', np.linalg.norm(z - zp))):
                assert abs(tr[name][c, b] - want) <= 1e-4 * want, (b, it, name, tr[name][c, b], want)


# ---- 9. PnP -------------------------------------------------------------------------------------------------------------------------------

def test_pnp_takes_the_coils_and_runs_the_loop_written_out():
    """PNP_ADMM_L1_D with coils= equals, bit for bit, its loop written out here with Engine.dc_step and the same Denoiser; and it is NOT
    what the call without coils makes of the coil-combined data (the options dict swallows unknown keywords: `coils` must not be one)."""
    import torch
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import solvers_pnp as SP
    H, W, C = 128, 128, 2
    S = M.coil_maps(C, H, W, 5)
    _, masks, imgs, _ = case(H, W, 3)
    m = masks[0]
    y = np.stack([M.synthesize(imgs[b], S, m, M.noise(b, C, m)) for b in range(B)])
    reo = 0.25
    got = P.PNP_ADMM_L1_D('ffdnet_gray', m, None, y=y, coils=S, model=weights_trained(), iter_num=3, reo=reo)
    d = torch.device('cuda', 0)
    den = SP._load_model('ffdnet_gray', weights_trained(), 'model_zoo', 3, None, True, None, d, shape=(H, W))
    with torch.cuda.device(d), torch.no_grad(), P.Engine(H, W, Bmax=B) as eng:
        eng.set_stream(torch.cuda.current_stream(d).cuda_stream)
        eng.set_coils(S)
        eng.upload(y, m)
        eng.init_state()
        x, z, w = SP._device_state(torch, eng, B, H, W, d)
        t = torch.empty_like(z)
        for i in range(3):
            eng.dc_step(z, w, x, reo)
            den.select_bank(i)
            eng.add(x, w, t)
            den(t, i, out=z)
            eng.dual_clamp(x, z, w)
        torch.cuda.current_stream(d).synchronize()
        mine = x.reshape(B, H, W).cpu().numpy()
    for b in range(B):
        assert np.array_equal(np.asarray(got[b], np.float32), mine[b]), b
    combined = np.stack([np.fft.fft2(M.AH(y[b], S, m)) * m for b in range(B)])
    plain = P.PNP_ADMM_L1_D('ffdnet_gray', m, None, y=combined, model=weights_trained(), iter_num=3, reo=reo)
    for b in range(B):
        assert rel_l2(got[b], plain[b]) > 1e-3, b
