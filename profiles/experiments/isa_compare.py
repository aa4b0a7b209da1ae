#!/usr/bin/env python3
"""Per-kernel comparison of two builds' gfx950 assembly (`make` leaves csrc/*.s): which kernels are instruction-identical, and for those
that are not, what a refactor must keep -- LDS bytes, occupancy, scratch, registers, the counts of matrix / LDS / buffer / barrier
instructions and the order of the memory and barrier instructions among themselves -- plus the two ISA walks of tools/isa_scan.py.

usage: isa_compare.py PARENT_DIR BRANCH_DIR > shared_conv_bodies_isa.txt      (directories holding the *.s files of the two builds)"""
import glob
import importlib.util
import os
import re
import sys

_spec = importlib.util.spec_from_file_location('isa_scan', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'pnp_admm_cnc_mri_amd', 'csrc', 'tools', 'isa_scan.py'))
isa_scan = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_scan)

CLASSES = (('mfma', 'v_mfma'), ('ds_read', 'ds_read'), ('ds_write', 'ds_write'), ('buf_load', 'buffer_load'), ('buf_store', 'buffer_store'), ('barrier', 's_barrier'))
INFO = ('LDSByteSize', 'Occupancy', 'ScratchSize')


def is_dma(x):
    return x.startswith('buffer_load') and x.rstrip().endswith(' lds')


def mem_order(body):
    """the memory and barrier instructions in program order, by mnemonic (an LDS-DMA marked)"""
    out = []
    for x in body:
        op = x.split()[0]
        if op.startswith(tuple(p for _, p in CLASSES[1:])) or op.startswith(('global_', 'flat_', 'scratch_')):
            out.append(op + ('.lds' if is_dma(x) else ''))
    return out


def mem_blocks(k):
    """the same per straight-line run (cut at every label and behind every branch), sorted: what a different block LAYOUT leaves unchanged"""
    body, cuts = k['body'], set(k['labels'].values())
    runs, cur = [], []
    for idx, x in enumerate(body):
        if idx in cuts and cur:
            runs.append(cur)
            cur = []
        cur.append(x)
        if x.startswith(('s_branch', 's_cbranch')):
            runs.append(cur)
            cur = []
    runs.append(cur)
    return sorted(tuple(m) for m in map(mem_order, runs) if m)


def describe(k):
    i, b = k['info'], k['body']
    c = {n: sum(1 for x in b if x.startswith(p)) for n, p in CLASSES}
    c['dma'] = sum(1 for x in b if is_dma(x))
    return i, c


def unit_of(path):
    return os.path.basename(path)[:-2]


def main(parent, branch):
    rows, same, changed = [], 0, []
    for pb in sorted(glob.glob(os.path.join(branch, '*.s'))):
        pp = os.path.join(parent, os.path.basename(pb))
        # a kernel is its name and template arguments: the name of its argument struct may differ between the builds
        key = lambda ks: {re.sub(r'NS_\d+[A-Za-z0-9]*ArgsE', 'NS_ArgsE', n): k for n, k in ks.items()}
        kb, kp = key(isa_scan.kernels_of(open(pb).read())), key(isa_scan.kernels_of(open(pp).read()))
        if set(kb) != set(kp):
            print('%s: kernel symbols differ: only parent %s, only branch %s' % (unit_of(pb), sorted(set(kp) - set(kb)), sorted(set(kb) - set(kp))))
        for n in sorted(set(kb) & set(kp)):
            if kb[n]['body'] == kp[n]['body'] and kb[n]['info'] == kp[n]['info']:
                same += 1
            else:
                changed.append((unit_of(pb), n, kp[n], kb[n]))
    print('%d kernels instruction-identical to the parent (same instruction stream with comments stripped, same resources), %d differ:' % (same, len(changed)))
    ok = True
    for unit, n, p, b in changed:
        (ip, cp), (ib, cb) = describe(p), describe(b)
        regs_p, regs_b = ip['NumVgprs'] + ip['NumAgprs'], ib['NumVgprs'] + ib['NumAgprs']
        order = 'SAME' if mem_order(p['body']) == mem_order(b['body']) else 'SAME IN EVERY BLOCK, the blocks laid out in another order' if mem_blocks(p) == mem_blocks(b) else 'DIFFERS'
        keep = all(ip[k] == ib[k] for k in INFO) and regs_b <= regs_p and cp == cb and order != 'DIFFERS'
        ok &= keep
        print('\n%s  %s' % (unit, n))
        print('    %-8s LDS %6d  occupancy %d  scratch %d  VGPR+AGPR %3d  instructions %5d  s_waitcnt %3d   %s'
              % ('parent', ip['LDSByteSize'], ip['Occupancy'], ip['ScratchSize'], regs_p, len(p['body']), sum(1 for x in p['body'] if x.startswith('s_waitcnt')),
                 '  '.join('%s %d' % kv for kv in cp.items())))
        print('    %-8s LDS %6d  occupancy %d  scratch %d  VGPR+AGPR %3d  instructions %5d  s_waitcnt %3d   %s'
              % ('branch', ib['LDSByteSize'], ib['Occupancy'], ib['ScratchSize'], regs_b, len(b['body']), sum(1 for x in b['body'] if x.startswith('s_waitcnt')),
                 '  '.join('%s %d' % kv for kv in cb.items())))
        print('    memory / barrier order %s; resources and counts %s' % (order, 'KEPT' if keep else 'NOT KEPT'))
        if any(is_dma(x) for x in b['body']) or 'k_conv3x3_tail' in n:
            group = 2 if '_f16' in n and '_f16x3' not in n else 4
            walk = lambda k: (len(isa_scan.lds_pending_at_barriers(k['body'], k['labels'])),
                              len(isa_scan.dma_order_violations(k['body'], group=group, labels=k['labels'])) if any(is_dma(x) for x in k['body']) else 0)
            print('    lds_pending_at_barriers / dma_order_violations: parent %d / %d, branch %d / %d' % (walk(p) + walk(b)))
    print('\n' + ('every differing kernel keeps its parent\'s resources, counts and memory order' if ok else 'SOME KERNEL DOES NOT KEEP ITS PARENT\'S RESOURCES'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
