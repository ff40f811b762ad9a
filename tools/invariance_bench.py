#!/usr/bin/env python
"""
Where the compiled laws people hold send their own leaves (CompiledLaw.successors,
csrc/ehm_invariance.hip; needs a GPU).

    python tools/invariance_bench.py [--trees headline,cwh_z_job1,config3] [--repeats 5]
                                     [--out PATH]

Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py), cwh_z job 1
and the depth-18 config-3 tree, as tools/audit_bench.py builds them, each as a double law and as
``to_single(flush=True)``.  The plant is ``Plant.from_mpc`` of the law's own model.  Per law the
nominal successor (no box), and for cwh_z also the box of the process terms of
``NoiseModel.from_mpc`` (box terms through their maps, summed; a law whose model has none is
reported as not measured):
  counts by status, ``invariant_volume_fraction``, ``set_convex``, ``worst_margin``;
  kernel seconds (what the library reports) and wall seconds of ``successors()`` beside the wall
  seconds of ``cells()`` on the same law in the same process, each the median of --repeats after a
  warm-up call.
Nothing is promised about these numbers in advance: they are written down whatever they are.  One
JSON line per measurement to stdout and, as they come, to profiles/invariance/invariance_bench.txt.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_hybrid_mpc_amd import _capi, explicit, simulate      # noqa: E402
from explicit_hybrid_mpc_amd.noise import NoiseModel               # noqa: E402
from tools.audit_bench import config3, cwh_job1, headline          # noqa: E402


def process_box(mpc, n_d):
    """(lo, hi) [n_d] of the model's process terms if they are all boxes, else None."""
    model = NoiseModel.from_mpc(mpc)
    if model is None or n_d == 0:
        return None
    terms = [t for t in model.terms if t.kind == 'process']
    if not terms or any(t.shape != 'box' for t in terms):
        return None
    lo, hi = np.zeros(n_d), np.zeros(n_d)
    for t in terms:
        reach = np.abs(t.map) @ t.h
        lo += t.map @ t.c - reach
        hi += t.map @ t.c + reach
    return lo, hi


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='headline,cwh_z_job1,config3')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'invariance',
                                                  'invariance_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/invariance_bench.py --trees %s --repeats %d\n' % (args.trees, args.repeats))

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    makers = {'headline': headline, 'cwh_z_job1': cwh_job1, 'config3': config3}
    med = lambda a: float(np.median(a))
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
        if box is None:
            emit(tree=name, box='process', not_measured='the model gives no process box')
        else:
            boxes.append(('process terms', box))
        for law, precision in laws:
            law.cells(np.arange(min(64, law.stats['n_leaf'])))      # warm-up: roots, kernels' code
            t_cells = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                law.cells()
                t_cells.append(time.perf_counter() - t0)
            for label, d_box in boxes:
                law.successors(plant=plant, d_box=d_box)            # warm-up; the convexity test
                wall, kernel = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    res = law.successors(plant=plant, d_box=d_box)
                    wall.append(time.perf_counter() - t0)
                    kernel.append(res.seconds)
                emit(tree=name, law=precision, p=law.p, n_u=law.n_u, leaves=law.stats['n_leaf'],
                     roots=law.stats['n_roots'], has_nbr=law.stats['nbr_bytes'] > 0,
                     plant=dict(n_modes=int(plant.n_modes), n_d=int(plant.n_d),
                                n_g=int(plant.gx.size)),
                     box=label, d_box=None if d_box is None else [list(d_box[0]), list(d_box[1])],
                     corners=res.n_corners, counts=res.counts,
                     invariant_volume_fraction=res.invariant_volume_fraction,
                     cell_volume_fraction=res.cell_volume_fraction, set_convex=res.set_convex,
                     holds_on_set=res.holds_on_set, worst_margin=res.worst_margin,
                     worst_leaf=res.worst_leaf,
                     max_violation=float(np.fmax.reduce(res.max_violation, initial=-np.inf)),
                     kernel_s=med(kernel), kernel_s_all=kernel, successors_wall_s=med(wall),
                     successors_wall_s_all=wall, cells_wall_s=med(t_cells),
                     cells_wall_s_all=t_cells)
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
