#!/usr/bin/env python
"""
The certificate of the compiled laws people hold, leaf by leaf (CompiledLaw.certify,
csrc/ehm_certify.hip): throughput, seconds by stage and findings (needs a GPU).

    python tools/certify_bench.py [--repeats 3] [--max-tries 3] [--out PATH]

Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py) and cwh_z
job 1, as tools/audit_bench.py builds them.  Per tree the double compiled law and its single form
(``to_single()``, or ``to_single(flush=True)`` where the plain form is refused), certified against
the oracle the partition was made with:
  leaves/s over the wall time of ``certify()``, median of --repeats, and the split the library
  reports -- the cell, pack and judge kernels (device time), the feasibility batches, the cost
  batches, the tests (``ehm_bar_e_batch``), the volumes and the rest (host wall time);
  leaves by status, the certified volume fraction, ``n_relaxed``, the worst uncertified leaf, the
  tries made; for the single law the leaves the double law certifies and it does not.
About (p + 1) n_delta feasibility LPs, (p + 1) point LPs per candidate and one slack LP per
commutation and try are expected per leaf; the new kernels should be a few per cent at most.
There is no earlier number to compare with: recorded, not gated.  Writes one JSON line per law to
stdout and the lot to profiles/certify/certify_bench.txt.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_hybrid_mpc_amd import _capi, explicit     # noqa: E402
from tools.audit_bench import cwh_job1, headline               # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--max-tries', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'certify',
                                                  'certify_bench.txt'))
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
        first = None
        for law, precision in ((double, 'double'), (single, form)):
            law.certify(orc, leaves=np.arange(min(64, law.stats['n_leaf'])),
                        max_tries=args.max_tries)       # warm-up: problems, roots, kernels' code
            wall, split = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                res = law.certify(orc, max_tries=args.max_tries, return_leaves=True)
                wall.append(time.perf_counter() - t0)
                split.append(res.seconds)
            med = float(np.median(wall))
            row = dict(tree=name, law=precision, p=law.p, n_u=law.n_u,
                       n_delta=int(orc.gpu.can.n_delta), leaves=res.n, repeats=args.repeats,
                       max_tries=args.max_tries, wall_s=med, wall_s_all=wall,
                       leaves_per_s=res.n / med,
                       seconds={k: float(np.median([s[k] for s in split])) for k in split[0]},
                       counts=res.counts, passed=res.passed,
                       certified_volume_fraction=res.certified_volume_fraction,
                       cell_volume_fraction=res.cell_volume_fraction, n_relaxed=res.n_relaxed,
                       input_tol=res.input_tol, worst=res.worst,
                       tries_histogram=np.bincount(res.tries).tolist(),
                       candidates_histogram=np.bincount(res.n_candidates).tolist(),
                       largest_tbest_of_a_certified_leaf=float(
                           np.max(res.tbest[res.status == 0])) if (res.status == 0).any() else None)
            row['new_kernels_share_of_wall'] = row['seconds']['kernels'] / med
            if first is None:
                first = res
            else:
                lost = (first.status == 0) & (res.status != 0)
                row['certified_by_double_not_by_this'] = int(lost.sum())
                row['their_statuses'] = np.bincount(res.status[lost], minlength=6).tolist()
                row['certified_by_this_not_by_double'] = int(
                    ((first.status != 0) & (res.status == 0)).sum())
            emit(**row)
        for law in (single, double):
            law.close()
        orc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# tools/certify_bench.py --repeats %d --max-tries %d\n' % (args.repeats,
                                                                           args.max_tries))
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
