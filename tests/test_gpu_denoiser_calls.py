"""The forwards make the calls the classification says: one forward per (family, HIP backend) with every conv / FFDNet / relayout
entry point of libpnpmri.so recorded by name, against hip_layers' plan of the same network (tests/test_denoiser_plan_cpu.py holds the
plans themselves to the architectures)."""
import pytest

from test_denoiser_plan_cpu import calls

pytestmark = pytest.mark.gpu


class _Recorder:
    """the object _lib.lib() returns, noting the name of each layer call (weight packing happens once per weight: left out)"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(('pnp_conv', 'pnp_ffdnet', 'pnp_relayout')) or '_pack' in name:
            return fn

        def recorded(*args):
            self.names.append(name)
            return fn(*args)
        return recorded


@pytest.mark.parametrize('backend', ['hip', 'hip_f16x3', 'hip_f16'])
@pytest.mark.parametrize('name', ['ffdnet_gray', 'dncnn_15', 'dncnn_gray_blind', 'fdncnn_gray', 'ircnn_gray', 'drunet_gray'])
def test_a_forward_makes_the_calls_of_its_plan(name, backend, monkeypatch):
    import torch
    from pnp_admm_cnc_mri_amd import _lib, denoisers as D
    side = 64 if name == 'drunet_gray' else 32
    net, nlm, sched = D.build(name)
    net.load_state_dict(D.seeded_state_dict(net, 5))
    noises = torch.zeros(side, side).numpy() if D.family(name) == 'fdncnn' else None
    den = D.Denoiser(name, net.eval(), nlm, sigmas=torch.tensor([20.0 / 255]) if sched else None, noises=noises, backend=backend,
                     miopen_find=False).to('cuda')
    x = torch.rand(1, 1, side, side, device='cuda', generator=torch.Generator(device='cuda').manual_seed(11))
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', rec)
    y = den(x, 0)
    torch.cuda.synchronize()
    want = [c[0] for c in calls(D.hip_plan(den.model, backend, side, side)) if c[0] != 'torch']
    assert rec.names == want
    assert len(want) == {'ffdnet_gray': 15, 'dncnn_15': 17, 'dncnn_gray_blind': 20, 'fdncnn_gray': 20, 'ircnn_gray': 7,
                         'drunet_gray': 18 if backend == 'hip' else 64}[name]
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
