"""Range limits of pnp_ctx_create_any[_f64] (no compute: these run without a GPU).  128 <= H, W <= 1024 are accepted for
their size; outside, PNP_E_ARG with the message naming the accepted shapes.  pnp_ctx_create[_f64] keep H, W in {256, 512}."""
import ctypes as C

import pytest

from pnp_admm_cnc_mri_amd import _lib


@pytest.mark.parametrize('H, W', [(127, 256), (256, 127), (1025, 1025), (320, 1025), (127, 127)])
@pytest.mark.parametrize('create', ['pnp_ctx_create_any', 'pnp_ctx_create_any_f64'])
def test_out_of_range_is_an_argument_error(H, W, create):
    L = _lib.lib()
    ctx = _lib.ctx_p()
    assert getattr(L, create)(0, H, W, 1, C.byref(ctx)) == -1            # PNP_E_ARG
    msg = L.pnp_last_error()
    assert b'256 or 512' in msg and b'[128, 1024]' in msg
    assert not ctx.value


@pytest.mark.parametrize('H, W', [(320, 218), (128, 128), (1024, 1024), (218, 170), (640, 368), (256, 320)])
@pytest.mark.parametrize('create', ['pnp_ctx_create_any', 'pnp_ctx_create_any_f64'])
def test_in_range_is_not_refused_for_its_size(H, W, create):
    """Without a device the creation may still fail -- at the HIP call, never at the size check."""
    L = _lib.lib()
    ctx = _lib.ctx_p()
    rc = getattr(L, create)(0, H, W, 1, C.byref(ctx))
    if rc == 0:
        L.pnp_ctx_destroy(ctx)
        return
    assert rc != -1, L.pnp_last_error()
    assert b'must be' not in L.pnp_last_error()


def test_introspection_argument_errors():
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    assert L.pnp_fft_plan(None, 0, buf, 64) == -1
    assert L.pnp_ctx_path(None) == b'generic'


@pytest.mark.parametrize('create', ['pnp_ctx_create', 'pnp_ctx_create_f64'])
def test_fixed_size_creation_keeps_its_contract(create):
    """pnp_ctx_create[_f64] keep the published contract H, W in {256, 512}: the plain-C consumer of the ABI
    (tests/host/abi_consumer.c) relies on 300 x 256 being refused by pnp_ctx_create; the any-size shapes are reached through
    pnp_ctx_create_any[_f64], which the tests above cover."""
    L = _lib.lib()
    ctx = _lib.ctx_p()
    for H, W in ((320, 218), (300, 256), (100, 256)):
        assert getattr(L, create)(0, H, W, 1, C.byref(ctx)) == -1
        assert b'256 or 512' in L.pnp_last_error() and not ctx.value
