#!/usr/bin/env python
"""
Throughput of the sampled audit (ExplicitMPC.audit, csrc/ehm_audit.hip) against the same audit made
the way tests/test_gpu_explicit.py makes it on the host (needs a GPU).

    python tools/audit_bench.py [--n 200000] [--repeats 5] [--skip-config3] [--out PATH]

Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py) and cwh_z
job 1.  Per tree, in one process and in alternating runs, medians of --repeats:
  (a) device  law.audit(n): samples/s over wall time, and the split the library reports -- the
              sampling kernel, the locate / cost / reduce kernels (device time), the P_theta
              batches (host wall time);
  (b) host    the same n the way the existing guarantee test does it: numpy draw from the bounding
              box, law.evaluate for the leaf, np.linalg.solve for Vbar, oracle.gpu.solve_pt, the
              comparisons in numpy (for cwh_z the bounding box is the set).
No ratio is fixed in advance: the LP solves are expected to dominate both, and a device path that
is no faster is recorded as that.  Also recorded: max_ratio, the histogram and the open volume
fraction of each tree, and -- unless --skip-config3 -- of the depth-18 config-3 tree (pwa_mpc(0),
abs_frac 0.1, eps_r 1e-2, bench.py's CONFIG3), whose leaves at the depth limit are open.
Writes one JSON line per measurement to stdout and the lot to profiles/audit/audit_bench.txt.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_hybrid_mpc_amd import examples, explicit, partition          # noqa: E402
from explicit_hybrid_mpc_amd import tools as ehm_tools                    # noqa: E402
from oracle import geometry                                               # noqa: E402


def headline():
    mpc = examples.linear_mpc(seed=0)
    V = examples.box_vertices(examples.theta_box(mpc))
    orc = examples.create_oracle(mpc, V, abs_frac=0.02, abs_err=None, rel_err=1e-2)
    roots, _ = ehm_tools.delaunay_roots(V)
    return orc, V, partition.run_engine(orc, roots, action='ecc', max_nodes=1 << 23)


def cwh_job1():
    known = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'known_answers.json')))['runs']
    V, _, orc = examples.example('cwh_z', abs_frac=0.5, rel_err=float(known[0]['rel_err']))
    roots, _ = geometry.delaunay_simplices(V)
    return orc, V, orc.gpu.partition(np.array(roots), action='ecc', max_nodes=1 << 24)


def config3(max_depth=18):
    mpc = examples.pwa_mpc(seed=0)
    V = examples.box_vertices(examples.theta_box(mpc))
    orc = examples.create_oracle(mpc, V, abs_frac=0.1, abs_err=None, rel_err=1e-2)
    roots, _ = ehm_tools.delaunay_roots(V)
    return orc, V, partition.run_engine(orc, roots, action='ecc', max_nodes=1 << 24,
                                        max_depth=max_depth)


def host_audit(law, flat, orc, V, n, seed, rtol=1e-7):
    """The audit of test_partition_delivers_the_epsilon_suboptimality_guarantee: (counts by status
    value, max ratio).  Box-shaped sets only."""
    rng = np.random.default_rng(seed)
    half = np.abs(V).max(axis=0)
    X = rng.uniform(-1, 1, (n, half.size)) * half * (1 - 1e-9)
    _, leaf, _, _ = law.evaluate(X, return_info=True)
    R = flat.vertices[leaf]
    E = np.transpose(R[:, 1:] - R[:, :1], (0, 2, 1))
    beta = np.linalg.solve(E, (X - R[:, 0])[:, :, None])[:, :, 0]
    alpha = np.concatenate([1. - beta.sum(axis=1, keepdims=True), beta], axis=1)
    vbar = np.sum(alpha * flat.vertex_costs[leaf], axis=1)
    vstar, _, didx = orc.gpu.solve_pt(X)
    with np.errstate(invalid='ignore'):
        gap = vbar - vstar
        bound = np.maximum(orc.eps_a, orc.eps_r * vstar)
        tol = rtol * (1 + np.abs(vstar))
        st = np.zeros(n, dtype=np.int64)
        st[gap > bound + tol] = 1
        st[~(gap >= -tol)] = 2
        st[(flat.flags[leaf] & 1) == 0] = 3
        st[didx < 0] = 4
        judged = st <= 2
        ratio = float(np.max((gap / bound)[judged])) if judged.any() else -np.inf
    return np.bincount(st, minlength=5).tolist(), ratio


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--skip-config3', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'audit', 'audit_bench.txt'))
    args = ap.parse_args()
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for name, make in (('headline', headline), ('cwh_z_job1', cwh_job1)):
        orc, V, flat = make()
        law = explicit.ExplicitMPC(flat, orc)
        law.audit(n=2048, seed=0)                       # warm-up: cells, costs, kernels' code
        host_audit(law, flat, orc, V, 2048, 0)
        dev, host, split = [], [], []
        res = None
        for r in range(args.repeats):                   # alternating runs, one process
            t0 = time.perf_counter()
            res = law.audit(n=args.n, seed=1 + r)
            dev.append(time.perf_counter() - t0)
            split.append(res.seconds)
            t0 = time.perf_counter()
            hcounts, hratio = host_audit(law, flat, orc, V, args.n, 1 + r)
            host.append(time.perf_counter() - t0)
        med = lambda a: float(np.median(a))
        emit(tree=name, nodes=int(flat.n_nodes), leaves=int(law.cells()['node'].size), n=args.n,
             repeats=args.repeats, device_samples_per_s=args.n / med(dev),
             device_wall_s=med(dev), device_wall_s_all=dev,
             sample_kernel_s=med([s[0] for s in split]),
             locate_cost_reduce_kernels_s=med([s[1] for s in split]),
             p_theta_wall_s=med([s[2] for s in split]),
             host_samples_per_s=args.n / med(host), host_wall_s=med(host), host_wall_s_all=host,
             device_over_host=med(host) / med(dev),
             counts=res.counts, relocated=res.relocated, max_ratio=res.max_ratio,
             histogram=res.histogram.tolist(), open_volume_fraction=res.open_volume_fraction,
             host_counts_last=hcounts, host_max_ratio_last=hratio, passed=res.passed)
        law.close()
        orc.close()
    if not args.skip_config3:
        orc, V, flat = config3()
        law = explicit.ExplicitMPC(flat, orc)
        res = law.audit(n=args.n, seed=1)
        emit(tree='config3_depth18', nodes=int(flat.n_nodes),
             leaves=int(law.cells()['node'].size), n=args.n, counts=res.counts,
             relocated=res.relocated, max_ratio=res.max_ratio, histogram=res.histogram.tolist(),
             open_volume_fraction=res.open_volume_fraction, worst=None if res.worst is None else
             {k: (v.tolist() if hasattr(v, 'tolist') else v) for k, v in res.worst.items()},
             passed=res.passed, passed_allowing_open=res.counts['violation'] +
             res.counts['negative'] + res.counts['infeasible'] == 0, seconds=res.seconds)
        law.close()
        orc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# tools/audit_bench.py --n %d --repeats %d\n' % (args.n, args.repeats))
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
