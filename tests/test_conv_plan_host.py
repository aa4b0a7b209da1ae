"""CPU tests of csrc/conv_plan.h, the host-side plan of the denoisers' conv layers: tiles / items / persistent grid and the wide-or-narrow
choice against an independent restatement of the launchers' arithmetic, the one size bound of the three arithmetic families against a
brute-force walk of the rows every kernel geometry addresses (tests/host/conv_plan_emulation.cpp under g++ and the sanitizers), and the
accept / reject behaviour of the real library's entry points without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pnp_admm_cnc_mri_amd import _lib

SRC = os.path.join(ROOT, 'tests', 'host', 'conv_plan_emulation.cpp')
SAN = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
LIMIT = 2 ** 31 - 1
E_ARG = -1
OK, DIMS, CHANNELS, CHANNELS_UP, DILATION, FMT, CIN, COUT, ODD, SIZE, ITEMS, SHUFFLE = range(12)        # ConvWhy


@pytest.fixture(scope='module')
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('emu_conv_plan') / 'conv_plan_emulation')
    subprocess.check_call(['g++'] + SAN + ['-o', exe, SRC])

    def run(lines):
        r = subprocess.run([exe], input='\n'.join(lines).encode() + b'\n', env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and b'runtime error' not in r.stderr and b'AddressSanitizer' not in r.stderr, (r.returncode, r.stderr.decode()[-1500:])
        out = r.stdout.decode().split('\n')[:-1]
        assert not any(l.startswith('error') for l in out), out
        return out
    return run


def test_the_constants_the_kernels_take_from_the_plan(ask):
    assert [int(v) for v in ask(['constants'])[0].split()] == [16, 8, 16, 16, 16, 8, 64, 64, 1024, 8, 4, 16, 4]


# ---- 3a: tiles, items, grid, wide / narrow: restated from the launchers this header replaced ------------------------------------------

def _grid(items, wps, cus, nc):
    g = wps * cus
    g -= g % nc
    if g < nc:
        g = nc
    return items if items < g else g


def _expect(kind, n, ch, H, W, up, wps, cus, mode, dil):
    nc = 1
    if kind == 'narrow':
        tx, ty, nc = (W + 15) // 16, (H + 7) // 8, ch >> 6
    elif kind == 'wide':
        tx, ty, nc = (W + 15) // 16, (H + 15) // 16, ch >> 6
    elif kind == 'direct':
        tx, ty = (W + 15) // 16, (H + 7) // 8
    elif kind == 'ffdnet':
        tx, ty = ((W + 1) // 2 + 15) // 16, ((H + 1) // 2 + 7) // 8
    else:
        gh, gw = (H, W) if up else (H // 2, W // 2)
        tx, ty, nc = (gw + 15) // 16, (gh + 7) // 8, (2 * ch) >> 6
    items = n * tx * ty * nc
    items16 = n * ((W + 15) // 16) * ((H + 15) // 16) * (ch >> 6)
    wide = int(dil == 1 and (mode >= 1 or (mode < 0 and items16 >= cus)))
    return tx, ty, items, _grid(items, wps, cus, nc), wide, nc


def _cases():
    out = []
    shapes = [(1, 8, 16), (2, 96, 128), (1, 37, 21), (3, 250, 256), (5, 24, 40)]
    for cus in (1, 7, 256, 304):
        for nc in (1, 2, 3, 6, 12, 16):
            ch = 64 * nc
            for kind, wpss in (('narrow', (1, 2, 3)), ('wide', (1,)), ('direct', (2,)), ('ffdnet', (2,))):
                for wps in wpss:
                    if kind in ('direct', 'ffdnet') and nc > 1:
                        continue
                    base = max(nc, wps * cus - (wps * cus) % nc) // nc             # images of one tile each: items = grid exactly, then the next
                    for n, H, W in shapes + [(base, 8, 16), (base + 1, 8, 16)]:
                        for mode, dil in ((-1, 1), (0, 1), (1, 1), (-1, 2)) if kind == 'narrow' and wps == 2 else ((-1, 1),):
                            out.append((kind, n, ch, H, W, 0, wps, cus, mode, dil))
            for up in (0, 1):
                if up and ch % 128:
                    continue
                nb = 2 * nc
                base = max(nb, 2 * cus - (2 * cus) % nb) // nb
                for n, H, W in [(2, 96, 128), (1, 6, 6), (4, 48, 64), (base, 8 if up else 16, 16 if up else 32), (base + 1, 8 if up else 16, 16 if up else 32)]:
                    out.append(('pix2', n, ch, H, W, up, 2, cus, -1, 1))
    return out


def test_tiles_items_and_grid_match_the_launchers_arithmetic(ask):
    cases = _cases()
    got = ask(['tiling ' + ' '.join(str(v) for v in c) for c in cases])
    assert len(got) == len(cases) > 500
    seen = set()
    for c, line in zip(cases, got):
        tx, ty, items, grid, wide, nc = _expect(*c)
        assert [int(v) for v in line.split()] == [tx, ty, items, grid, wide], (c, line)
        # the properties themselves: a positive multiple of the blocks, at most the items, and a grid-stride loop from every workgroup
        # covers every item exactly once while a workgroup keeps its block
        assert grid >= 1 and grid % nc == 0 and grid <= items, (c, grid)
        idx = np.concatenate([np.arange(b, items, grid) for b in range(grid)])
        blk = np.concatenate([np.full(len(range(b, items, grid)), b % nc) for b in range(grid)])
        assert len(idx) == items and np.array_equal(np.sort(idx), np.arange(items)) and np.array_equal(idx % nc, blk), c
        wps, cus = c[6], c[7]
        seen.add(('few', items < nc * 2)); seen.add(('eq', items == grid)); seen.add(('next', items > grid and items - grid <= nc))
        seen.add(('starved', wps * cus < nc)); seen.add(('round', (wps * cus) % nc != 0 and items > wps * cus)); seen.add(('wide', wide))
    assert seen == {(k, v) for k in ('few', 'eq', 'next', 'starved', 'round') for v in (False, True)} | {('wide', 0), ('wide', 1)}


# ---- 3b: the size bound ------------------------------------------------------------------------------------------------------------

def _fits(H, W, ch):
    return (H + 16) * W * ch * 4 <= LIMIT


def _square_limit(ch):
    s = 1
    while _fits(s + 1, s + 1, ch):
        s += 1
    return s


def _widest(H, ch):
    return LIMIT // ((H + 16) * ch * 4)


def _rows(ask, H, W, pix):
    out = {}
    for line in ask(['rows %d %d %d' % (H, W, pix)]):
        name, max_inside, min_outside, size, lowest = line.split()
        out[name] = (int(max_inside), int(min_outside), int(size), int(lowest))
    assert sorted(out) == ['narrow_d1', 'narrow_d2', 'narrow_d3', 'narrow_d4', 'pix2', 'wide']
    return out


def test_the_largest_accepted_shapes_keep_every_row_offset_out_of_the_wrap(ask):
    """At the largest shape the check accepts -- square at C = 64 (2888: the float32-size bound alone gave 2896) and at C = 1024, one row, seven
    rows -- every offset of a row inside the image is the row's own (below 2^31), and every offset of a halo or overhang row, taken in 32 bits
    as the kernels take it, is at least the buffer's size: out of the descriptor's range.  No geometry reaches below row H + 15."""
    assert _square_limit(64) == 2888 and _square_limit(1024) == 716
    shapes = [(_square_limit(64),) * 2 + (64,), (_square_limit(1024),) * 2 + (1024,), (1, _widest(1, 64), 64), (7, _widest(7, 64), 64), (1, _widest(1, 1024), 1024)]
    for H, W, ch in shapes:
        assert _fits(H, W, ch) and not _fits(H, W + 1, ch)
        assert ask(['check body 1 %d %d %d 1 0' % (ch, H, W), 'check body 1 %d %d %d 1 0' % (ch, H, W + 1)]) == [str(OK), str(SIZE)]
        for pix in (4 * ch, 2 * ch):                                               # float32 and half tensors
            for name, (max_inside, min_outside, size, lowest) in _rows(ask, H, W, pix).items():
                assert size == H * W * pix and max_inside == size - 16 and max_inside < 2 ** 31, (H, W, ch, name)
                assert lowest <= H + 15 and (lowest == H + 15 or name != 'wide' or H % 16 != 1), (H, W, ch, name, lowest)
                if name != 'pix2':
                    assert size <= min_outside < 2 ** 32, (H, W, ch, pix, name, min_outside, size)
    assert ask(['check body 1 64 2889 2889 1 0', 'check body 1 1024 717 717 1 0']) == [str(SIZE)] * 2


def test_the_short_wide_image_that_wrapped_is_refused(ask):
    """H = 7, W = 2^20, C = 64: 1.9e9 bytes, below the float32-size bound the float32 and f16x3 families used to apply -- and the offset of the
    wide kernel's halo row 16 (one tile: rows -1 .. 16) is exactly 2^32, which wraps to the image's first byte.  The walk shows the wrap, the
    check refuses the shape."""
    H, W, ch = 7, 1 << 20, 64
    assert H * W * ch * 4 <= LIMIT < (H + 16) * W * ch * 4
    r = _rows(ask, H, W, 4 * ch)
    assert r['wide'][3] == 16 and r['wide'][1] == 0 < r['wide'][2]                  # an outside row's offset lands inside the buffer
    assert ask(['check body 1 64 %d %d 1 0' % (H, W), 'check tail 1 1 %d %d 0 0' % (H, W), 'check head 1 1 %d %d' % (H, W)]) == [str(SIZE)] * 3


def test_ffdnet_and_2x2_forms_apply_the_bound_to_the_tensors_the_kernels_address(ask):
    s = _square_limit(64)
    # FFDNet runs at ceil(h / 2) x ceil(w / 2): odd sizes round up
    assert ask(['check ffdnet 1 %d %d' % (2 * s - 1, 2 * s - 1), 'check ffdnet 1 %d %d' % (2 * s, 2 * s), 'check ffdnet 1 %d %d' % (2 * s + 1, 2 * s + 1),
                'check ffdnet 1 0 8', 'check tail 1 4 %d %d %d %d' % (s, s, 2 * s - 1, 2 * s), 'check tail 1 4 %d %d %d %d' % (s, s, 2 * s + 1, 2 * s),
                'check tail 1 3 8 8 15 16']) == [str(v) for v in (OK, OK, SIZE, DIMS, OK, SHUFFLE, SHUFFLE)]
    # 2 x 2: input and result both; down at C: the input is the larger tensor, up at C: the result (4 H W C / 2 values)
    down = next(v for v in range(2, 9000, 2) if not _fits(v, v, 128))
    up = next(v for v in range(1, 9000) if not _fits(2 * v, 2 * v, 64))
    assert ask(['check pix2 1 128 %d %d 0' % (down - 2, down - 2), 'check pix2 1 128 %d %d 0' % (down, down),
                'check pix2 1 128 %d %d 1' % (up - 1, up - 1), 'check pix2 1 128 %d %d 1' % (up, up),
                'check pix2 1 64 8 8 1', 'check pix2 1 64 7 8 0', 'check pix2 1 96 8 8 0', 'check pix2 1 192 8 8 1',
                'check pack3 1088', 'check pack3 1024', 'check pack2 64 1', 'check pack2 64 0',
                'check relayout 1 46341 46341', 'check relayout 2 46340 46340', 'check relayout 1 0 3']) == \
        [str(v) for v in (OK, SIZE, OK, SIZE, CHANNELS_UP, ODD, CHANNELS, CHANNELS_UP, CHANNELS, OK, CHANNELS_UP, OK, ITEMS, OK, DIMS)]
    # the other rules, and the item bound: 2^31 tiles of 8 x 16
    assert ask(['check body 1 64 8 8 5 0', 'check body 1 128 8 8 2 0', 'check body 1 64 8 8 4 7', 'check body 1 64 8 8 1 8', 'check body 0 64 8 8 1 0',
                'check head 1 9 8 8', 'check head 1 8 8 8', 'check tail 1 5 8 8 0 0', 'check body 2147483647 64 8 16 1 0', 'check body 2147483647 128 8 16 1 0',
                'check body 1 64 2147483647 2147483647 1 0']) == [str(v) for v in (DILATION, DILATION, OK, FMT, DIMS, CIN, OK, COUT, OK, ITEMS, SIZE)]


# ---- 3c: the three families accept and refuse alike (the real library, no device) ---------------------------------------------------------

def test_every_family_refuses_oversize_images_as_argument_errors():
    """8 x 1 040 000 x 64 floats are 2.13e9 bytes -- inside 2 GiB, but 24 rows of it are not: refused with the 16 rows named, by the float32 and
    f16x3 entry points as by their half-precision twins (tests/test_conv_f16_cpu.py).  4096 x 4096 is refused as beyond 2 GiB.  All of them
    PNP_E_ARG before any HIP call -- five of these entry points used to pass such shapes on to the launcher.  Pointers are never dereferenced."""
    L = _lib.lib()
    p, q, r = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    msg = lambda: L.pnp_last_error().decode()
    for (H, W), word in (((8, 1040000), '16 rows'), ((4096, 4096), '2 GiB')):
        calls = [
            ('pnp_conv3x3_c64_nhwc', (None, p, q, None, None, r, 1, H, W, 0, 1)),
            ('pnp_conv3x3_c64_nhwc_f16x3', (None, p, q, None, None, r, 1, H, W, 0, 1)),
            ('pnp_conv3x3_nhwc_f16x3', (None, p, q, None, None, r, 1, 64, H, W, 0)),
            ('pnp_conv3x3_nhwc_f16x3_fmt', (None, p, q, None, None, r, 1, 64, H, W, 0, 1, 0)),
            ('pnp_conv3x3_head_nhwc', (None, p, q, None, r, 1, 1, H, W, 1)),
            ('pnp_conv3x3_tail_nchw', (None, p, q, None, r, 1, 1, H, W)),
            ('pnp_conv3x3_tail_nchw_f16x3', (None, p, q, None, r, 1, 1, H, W)),
            ('pnp_conv2x2s2_nhwc_f16x3', (None, p, None, q, r, 1, 64, H, W)),
            ('pnp_convT2x2s2_nhwc_f16x3', (None, p, None, q, r, 1, 64, H, W)),
            # the half-precision twins answer the same
            ('pnp_conv3x3_nhwc_f16', (None, p, q, None, None, r, 1, 64, H, W, 0, 1, 0)),
            ('pnp_conv3x3_head_nhwc_f16', (None, p, q, None, r, 1, 1, H, W, 1)),
            ('pnp_conv3x3_tail_nchw_f16', (None, p, None, q, None, r, 1, 1, H, W)),
            ('pnp_conv2x2s2_nhwc_f16', (None, p, None, q, r, 1, 64, H, W, 0)),
        ]
        for name, args in calls:
            assert getattr(L, name)(*args) == E_ARG, (name, H, W)
            assert word in msg() and name + ':' in msg(), (name, msg())
    # the largest square at C = 64 went from 2896 to 2888: the first refused one, every family
    for name, args in (('pnp_conv3x3_c64_nhwc', (None, p, q, None, None, r, 1, 2889, 2889, 0, 1)),
                       ('pnp_conv3x3_nhwc_f16x3', (None, p, q, None, None, r, 1, 64, 2889, 2889, 0)),
                       ('pnp_conv3x3_nhwc_f16', (None, p, q, None, None, r, 1, 64, 2889, 2889, 0, 1, 0))):
        assert getattr(L, name)(*args) == E_ARG and '16 rows' in msg() and '2 GiB' in msg(), name
    # the remaining rules of the float32 / f16x3 entry points come back under their own names
    assert L.pnp_conv3x3_c64_nhwc(None, p, q, None, None, r, 1, 8, 8, 0, 5) == E_ARG and 'dilation' in msg()
    assert L.pnp_conv3x3_nhwc_f16x3_fmt(None, p, q, None, None, r, 1, 64, 8, 8, 0, 1, 8) == E_ARG and 'fmt' in msg()
    assert L.pnp_conv3x3_nhwc_f16x3(None, p, q, None, None, r, 1, 96, 8, 8, 0) == E_ARG and 'multiple of 64' in msg()
    assert L.pnp_conv3x3_nhwc_f16x3(None, p, q, None, None, p, 1, 64, 8, 8, 0) == E_ARG and 'alias' in msg()
    assert L.pnp_conv3x3_head_nhwc(None, p, q, None, r, 1, 9, 8, 8, 1) == E_ARG and 'cin' in msg()
    assert L.pnp_conv3x3_tail_nchw_f16x3(None, p, q, None, r, 1, 5, 8, 8) == E_ARG and 'cout' in msg()
    assert L.pnp_convT2x2s2_nhwc_f16x3(None, p, None, q, r, 1, 64, 8, 8) == E_ARG and '128' in msg()
    assert L.pnp_conv2x2s2_nhwc_f16x3(None, p, None, q, r, 1, 64, 7, 8) == E_ARG and 'even' in msg()
    assert L.pnp_relayout_c64(None, p, p, 1, 8, 8, 1) == E_ARG and 'alias' in msg()
    assert L.pnp_conv3x3_c64_pack_f16x3(None, None, q) == E_ARG and 'null' in msg() and 'pnp_conv3x3_c64_pack_f16x3' in msg()
