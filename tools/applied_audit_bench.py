#!/usr/bin/env python
"""
Throughput and findings of the audit by the cost of the applied input (CompiledLaw.audit,
csrc/ehm_applied.hip) next to the existing audit of the source law (needs a GPU).

    python tools/applied_audit_bench.py [--n 200000] [--repeats 5] [--out PATH]

Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py) and cwh_z
job 1, as tools/audit_bench.py builds them.  Per tree the double compiled law and its single form
(``to_single()``, or ``to_single(flush=True)`` where the plain form is refused), each in one process
in runs alternating with ``ExplicitMPC.audit`` on the same seed, medians of --repeats:
  samples/s over wall time of both audits, and the split the library reports for the new one --
  sampling kernel, evaluation kernel, pack + reduce kernels (device time), the P_theta batches
  of the oracle and of the applied-input problem (host wall time).
About two P_theta batches where ``audit`` has one are expected; that is recorded, not gated.
Findings per law, at the default input_tol and at input_tol = 0 (the exact substitution): counts,
max_ratio, n_relaxed, and of the samples whose input is saturated -- it sits on a bound of the
oracle's input set: a row of the canonical form on u_0 alone, G_u u_0 <= w, with
w - G_u ubar <= 1e-6 max(1, |w|) -- how many are inadmissible.  Also recorded, because the audit's
choice to price an admissible input by the exact substitution rests on it: what the same samples
give with V_u taken from the relaxed problem at EVERY sample (``relaxed_throughout``: negative
samples and the smallest (V_u - V*) / slack), computed here from ``GpuProblem.solve_pt`` on
``applied_input_problem(can, input_tol)``.
Writes one JSON line per measurement to stdout and the lot to
profiles/applied_audit/applied_audit_bench.txt.
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


def input_bound_rows(can):
    """(G_u [r, n_u], w [r]) of the rows of commutation 0 that hold u_0 alone: its bounds."""
    G, S, n_u = can.G[0], can.S[0], can.n_u
    alone = (G[:, :n_u] != 0.).any(axis=1) & ~(G[:, n_u:] != 0.).any(axis=1) & \
        ~(S != 0.).any(axis=1)
    return G[alone][:, :n_u], can.w[0][alone]


def findings(law, orc, n, seed, input_tol):
    res = law.audit(orc, n=n, seed=seed, input_tol=input_tol, return_samples=True)
    Gu, w = input_bound_rows(orc.gpu.can)
    finite = np.isfinite(res.u).all(axis=1)
    room = w[None, :] - np.where(finite[:, None], res.u, 0.) @ Gu.T
    saturated = finite & (room <= 1e-6 * np.maximum(1., np.abs(w))[None, :]).any(axis=1)
    judged = res.status <= 2
    slack = res.rtol * (1. + np.abs(res.vstar))
    out = dict(input_tol=res.input_tol, counts=res.counts, max_ratio=res.max_ratio,
               passed=res.passed, n_relaxed=res.n_relaxed, input_bound_rows=int(w.size),
               saturated=int(saturated.sum()),
               saturated_inadmissible=int((saturated & (res.status == 3)).sum()),
               saturated_relaxed=int((saturated & (res.relaxed == 1)).sum()),
               smallest_gap_over_slack=float(np.min(((res.vu - res.vstar) / slack)[judged]))
               if judged.any() else None, histogram=res.histogram.tolist())
    if res.input_tol > 0.:
        out['relaxed_throughout'] = relaxed_throughout(orc, res)
    return out


def relaxed_throughout(orc, res):
    """The samples of ``res`` with V_u taken from the relaxed problem at every one of them."""
    red = applied.applied_input_problem(orc.gpu.can, res.input_tol)
    gp = engine.GpuProblem(red, orc.eps_a, orc.eps_r, device=orc.gpu.device)
    U = np.where(np.isfinite(res.u), res.u, 0.)
    J, _, didx = gp.solve_pt(np.concatenate([res.x, U], axis=1))
    gp.close()
    ok = (res.delta_idx >= 0) & np.isfinite(res.u).all(axis=1) & (didx >= 0)
    gap = (J + U @ red.cost_u - res.vstar)[ok]
    slack = (res.rtol * (1. + np.abs(res.vstar)))[ok]
    return dict(judged=int(ok.sum()), negative=int((~(gap >= -slack)).sum()),
                smallest_gap_over_slack=float(np.min(gap / slack)) if ok.any() else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'applied_audit',
                                                  'applied_audit_bench.txt'))
    args = ap.parse_args()
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    med = lambda a: float(np.median(a))
    for name, make in (('headline', headline), ('cwh_z_job1', cwh_job1)):
        orc, V, flat = make()
        src = explicit.ExplicitMPC(flat, orc)
        double = src.compile()
        try:
            single, form = double.to_single(), 'single'
        except _capi.EhmError:
            single, form = double.to_single(flush=True), 'single, flush'
        src.audit(n=2048, seed=0)                       # warm-up: cells, costs, kernels' code
        for law, precision in ((double, 'double'), (single, form)):
            law.audit(orc, n=2048, seed=0)
            new, old, split = [], [], []
            for r in range(args.repeats):               # alternating runs, one process
                t0 = time.perf_counter()
                res = law.audit(orc, n=args.n, seed=1 + r)
                new.append(time.perf_counter() - t0)
                split.append(res.seconds)
                t0 = time.perf_counter()
                src.audit(n=args.n, seed=1 + r)
                old.append(time.perf_counter() - t0)
            emit(tree=name, law=precision, nodes=int(flat.n_nodes),
                 leaves=int(law.stats['n_leaf']), roots=int(law.stats['n_roots']), n=args.n,
                 repeats=args.repeats, samples_per_s=args.n / med(new), wall_s=med(new),
                 wall_s_all=new, sample_kernel_s=med([s[0] for s in split]),
                 eval_kernel_s=med([s[1] for s in split]),
                 pack_reduce_kernels_s=med([s[2] for s in split]),
                 p_theta_wall_s=med([s[3] for s in split]),
                 applied_wall_s=med([s[4] for s in split]),
                 audit_samples_per_s=args.n / med(old), audit_wall_s=med(old),
                 audit_wall_s_all=old, applied_over_audit_wall=med(new) / med(old),
                 default=findings(law, orc, args.n, 1, None),
                 exact=findings(law, orc, args.n, 1, 0.))
        for law in (single, double, src):
            law.close()
        orc.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# tools/applied_audit_bench.py --n %d --repeats %d\n' % (args.n, args.repeats))
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
