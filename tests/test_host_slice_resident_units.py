"""CPU test of the resident UNITS of w in the slice-resident CNC kernel (kernels_slice256.hip, k_slice<2>): the table and index maps of
csrc/slice_layout.h (sl_units_lds / sl_units_reg / w_home, sl_res_index, sl_res1_index, sl_reg_slot) emulated thread by thread with
g++ (tests/host/slice_resident_units_emulation.cpp) -- built with the sanitizer flags of test_host_cores.py, so an out-of-range
address is an error, not a wrong number.  The program exits non-zero when a resident address is written by more than one lane or by
none, when a lane would read back what another lane wrote, when LDS units, register units and set 0 together cover a w element twice,
when the flush does not restore the complete state, and on a collision or hole in any transposition pass; its x, z, w are compared
with the oracle to the tolerance of test_four_pass_resident_pipeline_matches_oracle.  Two tables: the kernel's own, and one that
spreads LDS and register units over other accesses and all four register sets."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import rel_l2, ROOT

SRC = os.path.join(ROOT, 'tests', 'host', 'slice_resident_units_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
TABLES = {'kernel': [], 'spread': ['-DSLICE_UNITS_LDS1=0x90', '-DSLICE_UNITS_REG=0x8104FF21']}     # (0, q) bits are masked: set 0 is in LDS


@pytest.fixture(scope='module', params=sorted(TABLES))
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp('emu_units_' + request.param) / 'slice_resident_units_emulation')
    subprocess.check_call(['g++'] + SAN + TABLES[request.param] + ['-o', out, SRC])
    return out


def _problem(golden_inputs):
    masks = np.stack([golden_inputs['masks']['Q_Random30'], golden_inputs['masks']['Q_Cartesian30']]).astype(np.uint8)
    ys = np.stack([O.synthetic_problem(b, masks[b])[1] for b in range(2)]).astype(np.complex64)
    rng = np.random.default_rng(11)
    z = rng.uniform(0, 1, (2, 256, 256)).astype(np.float32)
    w = rng.uniform(-0.1, 0.1, (2, 256, 256)).astype(np.float32)
    return z, w, ys, masks


@pytest.mark.parametrize('cnc', [0, 1])
def test_resident_units_pipeline_matches_oracle(exe, golden_inputs, cnc, tmp_path):
    z, w, ys, masks = _problem(golden_inputs)
    reo = 0.05
    cdc = 1.0 / (1.0 + 1.0 / 2.0 / reo)
    if cnc:
        alpha, lam, b = 0.45, 0.5, 64
        prox = (alpha * reo * lam, 1 - alpha, alpha, alpha * reo * lam * b, 1.0 / b)
    else:
        lam = 0.1
        prox = (reo * lam, 0, 0, 0, 0)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    for s in range(2):                                  # the program reconstructs slice 0 of its input file
        order = [s, 1 - s]
        inp, out = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
        with open(inp, 'wb') as f:
            f.write(struct.pack('<iif5f', 1, cnc, cdc, *prox))
            for a, dt in ((z[order], np.float32), (w[order], np.float32), (ys[order], np.complex64), (masks[order], np.uint8)):
                f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        r = subprocess.run([exe, inp, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
        raw = np.fromfile(out, dtype=np.float64).reshape(3, 256, 256)
        y128 = ys[s].astype(np.complex128)
        xr = O.dc_step(z[s].astype(np.float64), w[s].astype(np.float64), y128, masks[s], reo)
        if cnc:
            zr, wr = O.cnc_step(xr, z[s].astype(np.float64), w[s].astype(np.float64), alpha, lam, reo, b)
        else:
            zr, wr = O.l1_step(xr, z[s].astype(np.float64), w[s].astype(np.float64), lam, reo)
        assert rel_l2(raw[0], xr) <= 2e-6, rel_l2(raw[0], xr)
        assert rel_l2(raw[1], zr) <= 2e-6
        assert np.abs(raw[2] - wr).max() <= 2e-6
