"""The signatures of the five solver entry points and of sharding.solve_sharded, as literals taken from the commit before the entry points
were put on their shared drivers: names, order, kinds and defaults.  No GPU, no library call."""
import inspect

import pytest

COILS = ("coils=None, coil_id=None, cg_iters=3, virtual_coils=None, noise_cov=None, calib=24, maps_radius=2, maps_power_iters=4, "
         "maps_thresh=0.05, maps_method='walsh', maps_kernel=4, maps_sigma=0.02, maps_crop=0.9")
FILES = "images=None, y=None, mask_id=None, testsets='testsets', testset_name='Set1', results='results', save_E=None, device=None, return_info=False"
PLAIN = ("(mask, noises, " + FILES + ", precision='f32', return_device=False, trace_every=0, tol=None, transform=None, levels=3, " + COILS
         + ", spin=None, spin_average=1, spin_seed=0, image='real', **%s)")
CNN = "cnn_dtype=None, miopen_find='auto', cnn_backend='auto', cnn_graph=False, return_device=False"
PNP = ("(model_name, mask, noises, " + FILES + ", model_zoo='model_zoo', model=None, cnn_batch=None, " + CNN
       + ", state0=None, iter_start=0, trace_every=0, tol=None, " + COILS + ", **%s)")
SIGNATURES = {
    'ADMM_L1': PLAIN % 'ADMM_L1_opts',
    'ADMM_CNC': PLAIN % 'ADMM_CNC_opts',
    'PNP_ADMM_L1_D': PNP % 'PNP_ADMM_L1_D_opts',
    'PNP_ADMM_CNC_D': PNP % 'PNP_ADMM_CNC_D_opts',
    'PNP_ADMM_CNC_DnCNN': ("(model_name1, model_name2, mask, noises, " + FILES + ", model_zoo='model_zoo', model=None, model2=None, "
                           "cnn_batch=None, cnn_dtype=None, faithful_model2_path=True, miopen_find='auto', cnn_backend='auto', "
                           "cnn_graph=False, return_device=False, trace_every=0, tol=None, " + COILS + ", **opts)"),
    'solve_sharded': '(solver, mask, noises, images=None, y=None, mask_id=None, dst=0, group=None, gather_device=None, coil_id=None, '
                     '**solver_kwargs)',
}


def entry(name):
    import pnp_admm_cnc_mri_amd as P
    from pnp_admm_cnc_mri_amd import sharding
    return sharding.solve_sharded if name == 'solve_sharded' else getattr(P, name)


@pytest.mark.parametrize('name', list(SIGNATURES))
def test_signature_is_what_it_was(name):
    assert str(inspect.signature(entry(name))) == SIGNATURES[name]


@pytest.mark.parametrize('name', [n for n in SIGNATURES if n != 'solve_sharded'])
def test_sharding_sees_return_device(name):
    from pnp_admm_cnc_mri_amd import sharding
    assert sharding._accepts(entry(name), 'return_device')


def test_the_coil_keywords_are_named_once():
    """the tuple the entry points collect their coil keywords by is the thirteen of the signatures, in their order"""
    from pnp_admm_cnc_mri_amd import solvers
    assert ', '.join(solvers.COIL_KEYS) == ', '.join(p.split('=')[0] for p in COILS.split(', '))
    for name in SIGNATURES:
        if name != 'solve_sharded':
            assert set(solvers.COIL_KEYS) <= set(inspect.signature(entry(name)).parameters), name
