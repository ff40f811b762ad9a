#!/usr/bin/env python
"""
What merging the leaves that apply one affine map saves on the compiled laws people hold
(CompiledLaw.reduce, csrc/ehm_reduce.hip; needs a GPU).

    python tools/reduce_bench.py [--trees headline,cwh_z_job1,config3] [--n 200000] [--repeats 3]
                                 [--out PATH]

Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py) as a double
law and as ``to_single(flush=True)``, cwh_z job 1 and the depth-18 config-3 tree as double laws, as
tools/audit_bench.py builds them.  Per law, at tol = the default (``applied.default_input_tol`` of
its u_0), 1e2 x and 1e4 x the default:
  leaves, internal records and bytes before / after, the largest accepted deviation;
  ``reduce()`` seconds (wall, median of --repeats, and what the library reports) beside ``cells()``
  seconds on the same law -- the same walk plus one more climb per input; reported, not gated;
  ``evaluate`` on 2^21 states uniform in the parameter box, kernel seconds and mean depth before /
  after, and the largest difference of the two laws' inputs on them;
  ``audit(oracle, n)`` of the reduced law (and once of the law itself): counts, max_ratio, passed.
Nothing fixes a reduction ratio in advance: the figures are written down whatever they are.  One
JSON line per measurement to stdout and, as they come, to profiles/reduce/reduce_bench.txt.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_hybrid_mpc_amd import explicit                   # noqa: E402
from tools.audit_bench import config3, cwh_job1, headline      # noqa: E402

FACTORS = (1., 1e2, 1e4)


def audit_row(res):
    return dict(counts=res.counts, max_ratio=res.max_ratio, passed=res.passed,
                violations=int(res.counts.get('violation', 0)), n_relaxed=res.n_relaxed)


def evaluate_row(law, X):
    law.evaluate(X[:4096])
    u, _, depth, secs = law.evaluate(X, return_info=True)
    return u, dict(kernel_s=secs, mean_depth=float(depth.mean()), max_depth=int(depth.max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='headline,cwh_z_job1,config3')
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--states', type=int, default=1 << 21)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reduce', 'reduce_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/reduce_bench.py --trees %s --n %d --repeats %d --states %d\n' % (
        args.trees, args.n, args.repeats, args.states))

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
        laws = [(double, 'double')]
        if name == 'headline':
            laws.append((double.to_single(flush=True), 'single, flush'))
        rng = np.random.default_rng(0)
        X = rng.uniform(V.min(axis=0), V.max(axis=0), (args.states, V.shape[1]))
        for law, precision in laws:
            law.cells(np.arange(min(64, law.stats['n_leaf'])))      # warm-up: roots, kernels' code
            t_cells = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                law.cells()
                t_cells.append(time.perf_counter() - t0)
            u0, ev0 = evaluate_row(law, X)
            base = law.reduce(0.)                                   # warm-up; the default tolerance
            base.close()
            default = float(law.reduce().reduction['tol'][0])
            emit(tree=name, law=precision, p=law.p, n_u=law.n_u, nodes=int(flat.n_nodes),
                 leaves=law.stats['n_leaf'], n_int=law.stats['n_plane'], roots=law.stats['n_roots'],
                 bytes=law.stats['bytes'], default_tol=default, cells_wall_s=med(t_cells),
                 cells_wall_s_all=t_cells, evaluate=ev0, states=args.states,
                 audit=audit_row(law.audit(orc, n=args.n, seed=1)))
            for factor in FACTORS:
                tol = factor * default
                wall, lib = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    red = law.reduce(tol)
                    wall.append(time.perf_counter() - t0)
                    lib.append(red.reduction['seconds'])
                    r = red.reduction
                    if _ + 1 < args.repeats:
                        red.close()
                u1, ev1 = evaluate_row(red, X)
                both = np.isfinite(u0).all(axis=1) & np.isfinite(u1).all(axis=1)
                emit(tree=name, law=precision, tol=tol, tol_over_default=factor,
                     leaves_before=r['n_leaf_before'], leaves_after=r['n_leaf_after'],
                     n_int_before=r['n_int_before'], n_int_after=r['n_int_after'],
                     bytes_before=r['bytes_before'], bytes_after=r['bytes_after'],
                     bytes_ratio=r['bytes_after'] / r['bytes_before'],
                     max_deviation=r['max_deviation'], reduce_wall_s=med(wall),
                     reduce_wall_s_all=wall, reduce_library_s=med(lib),
                     cells_wall_s=med(t_cells), reduce_over_cells=med(wall) / med(t_cells),
                     evaluate_before=ev0, evaluate_after=ev1,
                     max_input_difference_on_states=float(np.abs(u1 - u0)[both].max()),
                     audit=audit_row(red.audit(orc, n=args.n, seed=1)))
                red.close()
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
