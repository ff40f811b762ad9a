"""Static and dynamic instruction census of a kernel's ISA per solver phase.

Usage: python tools/isa_phases.py file.s kernel_substring [--trips LABEL=N,LABEL=N,...]
                                  [--trips-file FILE] [--default-trips N] [--show LABEL]
Compile with -DEHM2_ISA_MARKS: csrc/ehm_ipm2.h then leaves a comment "@@PHASE k" where phase k of
ipm_solve ENDS (the phase numbers of tools/solver_phases.py), e.g.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DEHM_NP=16 -DEHM_SLOTS=3 -DEHM_PERSIST_MIDFIRST=1 \
          -DEHM2_ISA_MARKS --cuda-device-only -S explicit_hybrid_mpc_amd/csrc/ehm_k2.hip -o /tmp/k2.s  For every phase: instruction counts by class, and the
loops found inside it (label, body length, classes).

With --trips (or --trips-file: one "LABEL=N" per line, "#" comments) a second table gives DYNAMIC
counts: an instruction counts once for every trip of every loop around it (the product over the
nest; a loop = the span from a label to the last backward branch to it).  A loop that is not
listed runs --default-trips times (1): leave the iteration loop and the kernel's outer loops
unlisted and the table reads "per IPM iteration".  N = 0 takes a body out (a tail that does not
run at the given sizes).  --show LABEL prints a loop's body, to tell which source loop it is.
"""
import argparse
import re
import sys
from collections import Counter, OrderedDict


def classify(op):
    if op.startswith('v_mfma'):
        return 'MFMA'
    if op.startswith(('ds_', )):
        return 'LDS'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'VMEM'
    if op.startswith('v_'):
        if 'f64' in op and not op.startswith('v_cmp'):
            return 'VALU_F64'
        if 'readlane' in op or 'readfirstlane' in op:
            return 'VALU_RDLANE'
        if 'writelane' in op:
            return 'VALU_WRLANE'
        if op.startswith(('v_mov', 'v_accvgpr')):
            return 'VALU_MOV'
        return 'VALU_OTHER'
    if op.startswith('s_waitcnt'):
        return 'WAIT'
    if op.startswith('s_nop'):
        return 'NOP'
    if op.startswith(('s_cbranch', 's_branch')):
        return 'BRANCH'
    if op.startswith('s_'):
        return 'SALU'
    return 'OTHER'


def parse_trips(args):
    trips = {}
    items = []
    if args.trips_file:
        for l in open(args.trips_file):
            l = l.split('#')[0].strip()
            if l:
                items.append(l)
    if args.trips:
        items += [x for x in args.trips.split(',') if x]
    for it in items:
        k, v = it.split('=')
        trips[k.strip()] = int(v)
    return trips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('path')
    ap.add_argument('kernel')
    ap.add_argument('--trips', default='')
    ap.add_argument('--trips-file', default=None)
    ap.add_argument('--default-trips', type=int, default=1)
    ap.add_argument('--show', default=None)
    args = ap.parse_args()
    path, kname = args.path, args.kernel
    trips = parse_trips(args)
    lines = open(path).read().split('\n')
    start = None
    for i, l in enumerate(lines):
        if l.startswith('_Z') and kname in l.split(':')[0] and ':' in l:
            start = i
            break
    if start is None:
        raise SystemExit('kernel not found')
    end = start
    while not lines[end].strip().startswith('.Lfunc_end'):
        end += 1
    body = lines[start:end]
    phases = OrderedDict()
    cur = 'prologue'
    seen = Counter()
    labels = {}
    insts = []      # (idx, phase, op, text)
    for l in body:
        t = l.strip()
        if '@@PHASE' in t:
            name = t.split('@@PHASE')[1].strip()
            seen[name] += 1
            cur = '%s#%d' % (name, seen[name])
            continue
        if re.match(r'^[.\w$]+:', t):
            labels[t.split(':')[0]] = len(insts)
            continue
        if not t or t.startswith(';') or t.startswith('.'):
            continue
        op = t.split()[0]
        insts.append((len(insts), cur, op, t))
    for idx, ph, op, t in insts:
        phases.setdefault(ph, Counter())[classify(op)] += 1
    # loops: backward branches
    loops = []
    for idx, ph, op, t in insts:
        if op.startswith(('s_cbranch', 's_branch')):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] <= idx:
                b = insts[labels[tgt]:idx + 1]
                c = Counter(classify(x[2]) for x in b)
                loops.append((insts[labels[tgt]][1], ph, tgt, len(b), c))
    order = ['VALU_F64', 'VALU_OTHER', 'VALU_MOV', 'VALU_RDLANE', 'VALU_WRLANE', 'MFMA', 'LDS', 'VMEM',
             'SALU', 'WAIT', 'NOP', 'BRANCH', 'OTHER']
    print('%-26s' % 'phase' + ''.join('%8s' % o[-7:] for o in order) + '   total')
    for ph, c in phases.items():
        print('%-26s' % ph + ''.join('%8d' % c.get(o, 0) for o in order) + '%8d' % sum(c.values()))
    print('\nloops (phase of head -> phase of branch, label, body length):')
    for hp, bp, tgt, n, c in loops:
        valu = sum(v for k, v in c.items() if k.startswith('VALU'))
        print('  %-22s %-22s %-12s %5d  valu %4d f64 %4d lds %4d mfma %3d' %
              (hp, bp, tgt, n, valu, c.get('VALU_F64', 0), c.get('LDS', 0), c.get('MFMA', 0)))
    # loop spans: label -> (first instruction, last backward branch to it)
    spans = {}
    for idx, ph, op, t in insts:
        if op.startswith(('s_cbranch', 's_branch')):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] <= idx:
                lo, hi = spans.get(tgt, (labels[tgt], idx))
                spans[tgt] = (lo, max(hi, idx))
    if args.show:
        lo, hi = spans[args.show]
        print('\n%s: instructions %d..%d' % (args.show, lo, hi))
        for x in insts[lo:hi + 1]:
            print('    [%s] %s' % (x[1], x[3]))
    if trips or args.default_trips != 1:
        unknown = [k for k in trips if k not in spans]
        if unknown:
            raise SystemExit('no such loop: %s' % ', '.join(unknown))
        weight = [1] * len(insts)
        for tgt, (lo, hi) in spans.items():
            n = trips.get(tgt, args.default_trips)
            if n != 1:
                for i in range(lo, hi + 1):
                    weight[i] *= n
        dyn = OrderedDict()
        for idx, ph, op, t in insts:
            dyn.setdefault(ph, Counter())[classify(op)] += weight[idx]
        print('\ndynamic counts (trips: %s; other loops x%d):' %
              (', '.join('%s=%d' % kv for kv in sorted(trips.items())) or 'none', args.default_trips))
        print('%-26s' % 'phase' + ''.join('%8s' % o[-7:] for o in order) + '   total')
        for ph, c in dyn.items():
            print('%-26s' % ph + ''.join('%8d' % c.get(o, 0) for o in order) + '%8d' % sum(c.values()))


if __name__ == '__main__':
    main()
