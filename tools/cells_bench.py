#!/usr/bin/env python
"""
Leaf cells of the compiled laws people hold (CompiledLaw.cells, csrc/ehm_certify.hip, DESIGN.md
3.8f): throughput and what the cells are next to the partitions they came from (needs a GPU).

    python tools/cells_bench.py [--repeats 5] [--out PATH]

Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py) and cwh_z
job 1, as tools/audit_bench.py builds them.  Per tree the double compiled law and its single form
(``to_single()``, or ``to_single(flush=True)`` where the plain form is refused):
  leaves/s over the wall time of ``cells()`` -- the parent table, the cell kernel and the copy of
  [n, p+1, p] vertices and [n, p+1, n_u] inputs to the host -- median of --repeats;
  leaves by status; the largest |cell - source vertex| and the same over the recovery bound
  p kappa_2(E_root) 2^-52 max|v_root|; the cells' volume (``ehm_volume_batch``) over the roots';
  for the single law the leaves whose cell differs from the double law's (none where both have
  one) and the largest difference of the vertex inputs.
There is no earlier number to compare with: recorded, not gated.  Writes one JSON line per law to
stdout and the lot to profiles/certify/cells_bench.txt.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_hybrid_mpc_amd import _capi, applied, engine, explicit     # noqa: E402
from tools.audit_bench import cwh_job1, headline               # noqa: E402


def root_above(flat):
    n = flat.vertices.shape[0]
    parent = np.full(n, -1, dtype=np.int64)
    for ch in (np.asarray(flat.left), np.asarray(flat.right)):
        k = np.nonzero(ch >= 0)[0]
        parent[ch[k]] = k
    top = np.arange(n)
    while (parent[top] >= 0).any():
        top = np.where(parent[top] >= 0, parent[top], top)
    return top


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'certify', 'cells_bench.txt'))
    args = ap.parse_args()
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for name, make in (('headline', headline), ('cwh_z_job1', cwh_job1)):
        orc, V, flat = make()
        src = explicit.ExplicitMPC(flat, orc)
        double = src.compile()
        src.close()
        try:
            single, form = double.to_single(), 'single'
        except _capi.EhmError:
            single, form = double.to_single(flush=True), 'single, flush'
        p = double.p
        top = root_above(flat)
        first = None
        for law, precision in ((double, 'double'), (single, form)):
            law.cells(np.arange(min(64, law.stats['n_leaf'])))      # warm-up: roots, kernels' code
            wall = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                got = law.cells()
                wall.append(time.perf_counter() - t0)
            live = got.status == 0
            source = flat.vertices[got.leaf_node]
            R = flat.vertices[top[got.leaf_node]]
            kappa = np.linalg.cond(np.transpose(R[:, 1:] - R[:, :1], (0, 2, 1)))
            scale = p * kappa * 2. ** -52 * np.abs(R).max(axis=(1, 2))
            err = np.abs(got.vertices - source).max(axis=(1, 2))
            usrc = flat.vertex_inputs[got.leaf_node]
            vol = engine.volume_batch(got.vertices[live], device=law.device)
            roots = applied.root_cells(law)
            row = dict(tree=name, law=precision, p=p, n_u=law.n_u, nodes=int(flat.n_nodes),
                       leaves=len(got), roots=int(law.stats['n_roots']), repeats=args.repeats,
                       wall_s=float(np.median(wall)), wall_s_all=wall,
                       leaves_per_s=len(got) / float(np.median(wall)), counts=got.counts,
                       max_vertex_error=float(err[live].max()),
                       max_vertex_error_over_bound=float((err / scale)[live].max()),
                       max_input_error_against_source=float(
                           np.abs(got.inputs - usrc)[live].max()),
                       volume_over_roots=float(vol.sum() / roots['volume'].sum()))
            if first is None:
                first = got
            else:
                both = live & (first.status == 0)
                row['cells_that_differ_from_double'] = int(
                    (got.vertices[both] != first.vertices[both]).any(axis=(1, 2)).sum())
                row['max_input_difference_from_double'] = float(
                    np.abs(got.inputs - first.inputs)[both].max())
                row['no_cell_where_double_has_one'] = int((~live & (first.status == 0)).sum())
            emit(**row)
        for law in (single, double):
            law.close()
        orc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# tools/cells_bench.py --repeats %d\n' % args.repeats)
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
