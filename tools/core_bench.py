#!/usr/bin/env python
"""
The invariant core of the compiled laws people hold (CompiledLaw.invariant_core, csrc/ehm_core.hip,
DESIGN.md 3.8i; needs a GPU, except --registers).

    python tools/core_bench.py [--trees headline,config3,cwh_z_job1] [--trajectories 100000]
                               [--steps 200] [--out PATH]
    python tools/core_bench.py --registers [--registers-source ehm_invariance.hip]
                               [--registers-out PATH]

Trees: the headline partition, the depth-18 config-3 tree and cwh_z job 1, as tools/audit_bench.py
builds them, each as a double law and as ``to_single(flush=True)``.  The plant is ``Plant.from_mpc``
of the law's own model.  Per law the nominal successor (no box), and for a law whose model has box
process terms (cwh_z) also their box (tools/invariance_bench.process_box):
  core leaves and ``core_volume_fraction``, sweeps, edges and mean fan-out of the rows built, the
  ``unresolved`` count; device seconds of the relation, wall seconds of the sweeps, of
  ``invariant_core()`` as a whole, of ``successors()`` and of ``cells()`` on the same law in the same
  process (one call each after a warm-up of the kernels' code);
  a rollout check: --trajectories states uniform in the core (a core leaf drawn by volume, a point
  uniform in its cell), --steps steps under a fresh disturbance uniform in the box each step; the
  number that stop.  It must be 0: anything else is a bug in the argument or in the code.
A ``max_edges`` failure at the defaults is written down as such, and the law measured once more
with the cap at 2^31 - 1.  Nothing is promised about these
numbers in advance.  One JSON line per measurement to stdout and, as they come, to
profiles/core/core_bench.txt.

--registers compiles csrc/ehm_core.hip for gfx950 with -Rpass-analysis=kernel-resource-usage and
writes the figures of every kernel to profiles/core/registers.txt (no GPU needed);
--registers-source ehm_invariance.hip does the same for the kernels of ``successors``, which step a
leaf's vertices with the same device code, into profiles/invariance/registers.txt.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# per source of --registers: where the figures go, and what its kernels keep in dynamic LDS
REGISTERS = {
    'ehm_core.hip': ('core', 'the static part; the plant, the box and the edge count of k_reach '
                     'are dynamic, a few KiB'),
    'ehm_invariance.hip': ('invariance', 'the static part, none; the plant, the box and the '
                           'counters are dynamic, at most 40 852 bytes'),
    'ehm_robust.hip': ('robust', 'the static part, none; the plant, the generators of every mode, '
                       'the boxes, the region rows and the counters are dynamic, at most 39 316 '
                       'bytes'),
}


def registers(source, path):
    from explicit_hybrid_mpc_amd import build
    src = os.path.join(build.SRC_DIR, source)
    path = path or os.path.join(ROOT, 'profiles', REGISTERS[source][0], 'registers.txt')
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                '-o', os.path.join(tmp, 'registers.o')]
        text = subprocess.run(cmd, check=True, stderr=subprocess.PIPE, text=True).stderr
    demangle = subprocess.run(['c++filt'], input=text, stdout=subprocess.PIPE, text=True).stdout
    rows, cur = [], None
    for line in demangle.splitlines():
        m = re.search(r'remark: (.*)$', line)
        if not m:
            continue
        body = re.sub(r'\s*\[-Rpass-analysis[^\]]*\]$', '', m.group(1).strip())
        name = re.match(r'Function Name: (.*)$', body)
        if name:
            cur = {'name': re.sub(r'\(anonymous namespace\)::|^void |\(.*$', '', name.group(1))}
            rows.append(cur)
        elif cur is not None and ':' in body:
            k, v = body.split(':', 1)
            cur[k.strip()] = v.strip()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as out:
        out.write('# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on '
                  'csrc/%s\n# (LDS: %s)\n' % (source, REGISTERS[source][1]))
        for r in rows:
            out.write('%-26s SGPRs %3s  VGPRs %3s  AGPRs %3s  scratch %s bytes/lane  waves/SIMD %s'
                      '  LDS %s bytes/block\n' % (
                          r['name'], r.get('TotalSGPRs', r.get('SGPRs', '?')),
                          r.get('VGPRs', '?'), r.get('AGPRs', '?'),
                          r.get('ScratchSize [bytes/lane]', '?'),
                          r.get('Occupancy [waves/SIMD]', '?'),
                          r.get('LDS Size [bytes/block]', '?')))
    print(open(path).read())


def sample_core(rng, vertices, core, n):
    """n states uniform in the union of the core cells."""
    V = vertices[core]
    p = V.shape[2]
    vol = np.abs(np.linalg.det(V[:, 1:] - V[:, :1]))
    pick = rng.choice(V.shape[0], n, p=vol / vol.sum())
    w = rng.dirichlet(np.ones(p + 1), n)
    return np.einsum('nv,nvc->nc', w, V[pick])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='headline,config3,cwh_z_job1')
    ap.add_argument('--trajectories', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'core', 'core_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--registers', action='store_true')
    ap.add_argument('--registers-source', default='ehm_core.hip', choices=sorted(REGISTERS))
    ap.add_argument('--registers-out', default=None)
    args = ap.parse_args()
    if args.registers:
        return registers(args.registers_source, args.registers_out)
    from explicit_hybrid_mpc_amd import _capi, explicit, invariance, simulate
    from tools.audit_bench import config3, cwh_job1, headline
    from tools.invariance_bench import process_box
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/core_bench.py --trees %s --trajectories %d --steps %d\n' % (
        args.trees, args.trajectories, args.steps))

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return res, time.perf_counter() - t0

    makers = {'headline': headline, 'cwh_z_job1': cwh_job1, 'config3': config3}
    rng = np.random.default_rng(20261020)
    for name in args.trees.split(','):
        orc, V, flat = makers[name]()
        src = explicit.ExplicitMPC(flat, orc)
        double = src.compile()
        src.close()
        try:
            plant = simulate.Plant.from_mpc(orc.mpc)
        except ValueError as e:
            emit(tree=name, not_measured=str(e))
            double.close()
            orc.close()
            continue
        laws = [(double, 'double')]
        try:
            laws.append((double.to_single(flush=True), 'single, flush'))
        except _capi.EhmError as e:
            emit(tree=name, law='single, flush', not_measured=str(e))
        boxes = [('nominal', None)]
        box = process_box(orc.mpc, plant.n_d)
        if box is not None:
            boxes.append(('process terms', box))
        for law, precision in laws:
            some = np.arange(min(64, law.stats['n_leaf']))
            law.cells(some)                                         # warm-up: roots, kernels' code
            law.successors(plant=plant, leaves=some)
            cells, t_cells = timed(law.cells)
            for label, d_box in boxes:
                row = dict(tree=name, law=precision, p=law.p, n_u=law.n_u,
                           leaves=law.stats['n_leaf'], roots=law.stats['n_roots'],
                           plant=dict(n_modes=int(plant.n_modes), n_d=int(plant.n_d)), box=label,
                           d_box=None if d_box is None else [list(d_box[0]), list(d_box[1])])
                _, t_succ = timed(lambda: law.successors(plant=plant, d_box=d_box))
                try:
                    res, t_core = timed(lambda: law.invariant_core(plant=plant, d_box=d_box,
                                                                   return_edges=True))
                except _capi.EhmError as e:
                    # written down as it is; then once more with the largest cap there is
                    emit(failed=str(e), max_edges=invariance.MAX_EDGES, successors_wall_s=t_succ,
                         cells_wall_s=t_cells, **row)
                    if e.code != _capi.EHM_E_CAPACITY:
                        continue
                    row.update(max_edges=2 ** 31 - 1)
                    try:
                        res, t_core = timed(lambda: law.invariant_core(
                            plant=plant, d_box=d_box, return_edges=True, max_edges=2 ** 31 - 1))
                    except _capi.EhmError as e2:
                        emit(failed=str(e2), **row)
                        continue
                built = int((np.diff(res.indptr) > 0).sum())
                row.update(counts=res.counts, core_leaves=res.counts['core'],
                           core_volume_fraction=res.core_volume_fraction, n_sweeps=res.n_sweeps,
                           n_edges=res.n_edges, rows_built=built,
                           mean_fan_out=res.n_edges / max(built, 1),
                           widest_row=int(np.diff(res.indptr).max()),
                           unresolved=res.counts['unresolved'], set_convex=res.set_convex,
                           holds=res.holds, reach_s=res.seconds_reach,
                           sweeps_s=res.seconds_sweeps, invariant_core_wall_s=t_core,
                           successors_wall_s=t_succ, cells_wall_s=t_cells)
                if res.core.any():
                    X0 = sample_core(rng, cells.vertices, res.core, args.trajectories)
                    status = []
                    for at in range(0, X0.shape[0], 25000):         # the disturbances of a batch
                        Xb, d = X0[at:at + 25000], None
                        if d_box is not None:
                            d = rng.uniform(d_box[0], d_box[1],
                                            (args.steps, Xb.shape[0], plant.n_d))
                        status.append(law.rollout(Xb, args.steps, d=d, plant=plant,
                                                  record=False).status)
                    status = np.concatenate(status)
                    row.update(rollout=dict(trajectories=int(X0.shape[0]), steps=args.steps,
                                            stopped=int((status != 0).sum()),
                                            by_status={int(s): int((status == s).sum())
                                                       for s in np.unique(status)}))
                else:
                    row.update(rollout='not run: the core is empty')
                emit(**row)
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
