"""CPU test of the halved transient LDS of the slice-resident CNC kernel (kernels_slice256.hip, k_slice<2>): the transform groups'
exchange in two planes, the transpositions' four passes in eight halves and the 16-unit table of resident w, emulated lane by lane
with g++ on one array of LDS words laid out by the map of csrc/slice_layout.h (tests/host/slice_split_emulation.cpp) -- built with
the sanitizer flags of test_host_cores.py, so an out-of-range address is an error, not a wrong number.  The program exits non-zero
when a transient word is read in a phase in which no lane wrote it (the words are poisoned between phases) or is written twice in one
phase, when a resident float has two owners or none, when two LDS areas overlap or the map leaves the compute unit's 163 840 bytes.
Its x, z, w after a launch of one and of three iterations must be bit-equal to slice_resident_units_emulation's (one iteration per
run, chained) on the same input, and within test_host_slice_resident_units.py's tolerance of the oracle.  Two tables: the kernel's
own, and one that spreads LDS and register units over other accesses and all four register sets."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import admm_oracle as O
from conftest import rel_l2, ROOT

SRC = os.path.join(ROOT, 'tests', 'host', 'slice_split_emulation.cpp')
REF = os.path.join(ROOT, 'tests', 'host', 'slice_resident_units_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
TABLES = {'kernel': [], 'spread': ['-DSLICE_UNITS_LDS1=0xB5', '-DSLICE_UNITS_REG=0x8104FF21']}     # (0, q) bits are masked: set 0 is in LDS
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
REO, ALPHA, LAM, BB = 0.05, 0.45, 0.5, 64


@pytest.fixture(scope='module', params=sorted(TABLES))
def exes(request, tmp_path_factory):
    d = tmp_path_factory.mktemp('emu_split_' + request.param)
    out = []
    for src in (SRC, REF):
        out.append(str(d / os.path.basename(src)[:-4]))
        subprocess.check_call(['g++'] + SAN + TABLES[request.param] + ['-o', out[-1], src])
    return out


def _run(exe, tmp_path, z, w, ys, masks, extra=()):
    cdc = 1.0 / (1.0 + 1.0 / 2.0 / REO)
    prox = (ALPHA * REO * LAM, 1 - ALPHA, ALPHA, ALPHA * REO * LAM * BB, 1.0 / BB)
    inp, out = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    with open(inp, 'wb') as f:
        f.write(struct.pack('<iif5f', 1, 1, cdc, *prox))
        for a, dt in ((z, np.float32), (w, np.float32), (ys, np.complex64), (masks, np.uint8)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    r = subprocess.run([exe, inp, out] + list(extra), env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
    return np.fromfile(out, dtype=np.float64).reshape(3, 256, 256)


def test_split_pipeline_equals_unit_emulation_and_oracle(exes, golden_inputs, tmp_path):
    split, ref = exes
    masks = np.stack([golden_inputs['masks']['Q_Random30'], golden_inputs['masks']['Q_Cartesian30']]).astype(np.uint8)
    ys = np.stack([O.synthetic_problem(b, masks[b])[1] for b in range(2)]).astype(np.complex64)
    rng = np.random.default_rng(11)
    z = rng.uniform(0, 1, (2, 256, 256)).astype(np.float32)             # the programs reconstruct slice 0 of their input
    w = rng.uniform(-0.1, 0.1, (2, 256, 256)).astype(np.float32)
    y128 = ys[0].astype(np.complex128)
    zc, wc = z.copy(), w.copy()                                           # the unit emulation: one iteration per run, chained
    zo, wo = z[0].astype(np.float64), w[0].astype(np.float64)             # the oracle
    for it in range(1, 4):
        chained = _run(ref, tmp_path, zc, wc, ys, masks)
        zc[0], wc[0] = chained[1].astype(np.float32), chained[2].astype(np.float32)
        assert np.array_equal(zc[0].astype(np.float64), chained[1]) and np.array_equal(wc[0].astype(np.float64), chained[2])
        xo = O.dc_step(zo, wo, y128, masks[0], REO)
        zo, wo = O.cnc_step(xo, zo, wo, ALPHA, LAM, REO, BB)
        if it not in (1, 3):
            continue
        got = _run(split, tmp_path, z, w, ys, masks, [str(it)])
        for name, a, b in zip('xzw', got, chained):
            assert np.array_equal(a, b), (it, name, float(np.abs(a - b).max()))
        assert rel_l2(got[0], xo) <= 2e-6, (it, rel_l2(got[0], xo))
        assert rel_l2(got[1], zo) <= 2e-6, (it, rel_l2(got[1], zo))
        assert np.abs(got[2] - wo).max() <= 2e-6, (it, float(np.abs(got[2] - wo).max()))
