#!/usr/bin/env python
"""
Certified fuel bounds of the compiled laws people hold (CoreResult.cost, csrc/ehm_cost.hip,
DESIGN.md 3.8m; needs a GPU, except --registers).

    python tools/cost_bench.py [--trees cwh_z_job1,headline,config3] [--trajectories 100000]
                               [--steps 1115] [--repeats 3] [--sweeps 16] [--out PATH]
    python tools/cost_bench.py --registers [--registers-out PATH]

Trees as tools/core_bench.py builds them, each as a double law and as ``to_single(flush=True)``; the
plant is ``Plant.from_mpc`` of the law's own model.

cwh_z job 1, nominally and under the box of its process terms: the core and the limit set of
``reach()``, then ``cost`` over each for --steps steps (20 orbits at the step count of
tools/dv_experiment.py): ``best_rate_hi``, ``best_rate_lo`` with their K, ``start_hi`` and
``start_lo`` at the horizon, the cycle the worst path ends in, and the leaves with the largest
``w_hi``.  Beside the nominal double law's bounds the mean and the 5-95 % band of ``u_norm_sum`` of
--trajectories nominal rollouts of the same length from states uniform in the core; every one of them
must lie between ``start_lo`` and ``start_hi``: the tool fails otherwise.

The headline law and config 3, for timing only (both cores are empty, so nothing is claimed): the
relation of ``rows='invariant'`` with ``level`` forced to 1 and every leaf that has a cell in the
domain (edges into leaves without one dropped), --sweeps sweeps, one warm-up call and --repeats
calls each with and without args: the device time per sweep (sweep and bookkeeping), the weights
kernel, the wall time of checking and uploading the relation; beside them ``k_reach_post`` on the
same relation (``reach_relation`` with no leaf a seed: clear, post and bookkeeping per step) and the
numpy mirror of the recurrence on the host (tests/cost_cpu.py, 2 sweeps).

Nothing is promised about these numbers in advance.  One JSON line per measurement to stdout and, as
they come, to profiles/cost/cost_bench.txt.  --registers compiles csrc/ehm_cost.hip for gfx950 with
-Rpass-analysis=kernel-resource-usage into profiles/cost/registers.txt (no GPU needed).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def registers(path):
    from tools import core_bench
    core_bench.REGISTERS['ehm_cost.hip'] = (
        'cost', 'all static: the wavefronts\' partial maxima and minima of k_cost_book')
    core_bench.registers('ehm_cost.hip', path)


def cycle_of(path):
    """The leaves of the last cycle a path closes (from the last leaf it has visited before back to
    that visit), or None where it never returns to a leaf."""
    path = [int(l) for l in path if l >= 0]
    for end in range(len(path) - 1, 0, -1):
        if path[end] in path[:end]:
            back = end - 1 - path[end - 1::-1].index(path[end])
            return path[back:end]
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='cwh_z_job1,headline,config3')
    ap.add_argument('--trajectories', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=1115)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cost', 'cost_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--registers', action='store_true')
    ap.add_argument('--registers-out', default=None)
    args = ap.parse_args()
    if args.registers:
        return registers(args.registers_out)
    from explicit_hybrid_mpc_amd import _capi, explicit, invariance, simulate
    from tests import cost_cpu
    from tools.audit_bench import config3, cwh_job1, headline
    from tools.core_bench import sample_core
    from tools.invariance_bench import process_box
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/cost_bench.py --trees %s --trajectories %d --steps %d --repeats %d '
              '--sweeps %d\n' % (args.trees, args.trajectories, args.steps, args.repeats,
                                 args.sweeps))

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def core_of(law, plant, d_box, row):
        try:
            return law.invariant_core(plant=plant, d_box=d_box, return_edges=True)
        except _capi.EhmError as e:
            if e.code != _capi.EHM_E_CAPACITY:
                raise
            row.update(max_edges=2 ** 31 - 1)
            return law.invariant_core(plant=plant, d_box=d_box, return_edges=True,
                                      max_edges=2 ** 31 - 1)

    def summary(res):
        worst = np.argsort(-np.nan_to_num(res.w_hi, nan=-1.))[:5]
        return dict(
            n_domain=res.n_domain, holds=res.holds, best_rate_hi=res.best_rate_hi,
            best_k_hi=res.best_k_hi, best_rate_lo=res.best_rate_lo, best_k_lo=res.best_k_lo,
            start_hi=float(res.start_hi[-1]), start_lo=float(res.start_lo[-1]),
            rate_hi_at_horizon=float(res.rate_hi[-1]), rate_lo_at_horizon=float(res.rate_lo[-1]),
            worst_cycle=cycle_of(res.path_hi), best_cycle=cycle_of(res.path_lo),
            heaviest_leaves=[dict(leaf=int(l), w_hi=float(res.w_hi[l]), w_lo=float(res.w_lo[l]),
                                  pad=float(res.pad[l])) for l in worst],
            w_hi_max=float(np.nanmax(res.w_hi)), w_hi_median=float(np.nanmedian(res.w_hi)),
            w_lo_zero_leaves=int((res.w_lo == 0.).sum()), pad_max=float(np.nanmax(res.pad)),
            weights_s=res.seconds_weights, sweeps_s=res.seconds_sweeps,
            upload_wall_s=res.seconds_upload)

    def fuel(law, plant, d_box, row, rng, rollouts):
        core = core_of(law, plant, d_box, row)
        reach = core.reach()
        row.update(core_leaves=core.counts['core'], n_edges=core.n_edges,
                   set_convex=core.set_convex, horizon=args.steps,
                   limit_leaves=None if reach.limit is None else int(reach.limit.sum()))
        over_core = core.cost(horizon=args.steps, return_paths=True)
        row.update(core=summary(over_core))
        if reach.limit is not None and reach.limit.any():
            row.update(limit=summary(reach.cost(core, horizon=args.steps, return_paths=True)))
        if rollouts:
            X0 = sample_core(rng, law.cells().vertices, core.core, args.trajectories)
            spent, stopped = [], 0
            for at in range(0, X0.shape[0], 25000):
                run = law.rollout(X0[at:at + 25000], args.steps, plant=plant, record=False)
                stopped += int((run.status != 0).sum())
                spent.append(run.u_norm_sum)
            spent = np.concatenate(spent)
            inside = bool((spent <= over_core.start_hi[-1] * (1. + 1e-12)).all() and
                          (spent >= over_core.start_lo[-1] * (1. - 1e-12)).all())
            row.update(rollout=dict(
                trajectories=int(spent.size), steps=args.steps, stopped=stopped,
                u_norm_sum_mean=float(spent.mean()), u_norm_sum_p05=float(np.quantile(spent, 0.05)),
                u_norm_sum_p95=float(np.quantile(spent, 0.95)), u_norm_sum_max=float(spent.max()),
                u_norm_sum_min=float(spent.min()), inside_bounds=inside,
                start_hi_over_max=float(over_core.start_hi[-1] / spent.max())))
            emit(**row)
            if not inside or stopped:
                raise SystemExit('a rollout spends outside the bounds: a bug in the argument or '
                                 'the code')
            return
        emit(**row)

    def timing(law, plant, row):
        core = core_of(law, plant, None, row)
        n = core.level.size
        level = np.ones(n, dtype=np.int32)
        D = law.cells().status == 0
        indptr, indices = core.indptr, core.indices
        if not D.all():
            keep = D[indices]
            src = np.repeat(np.arange(n), np.diff(indptr))[keep]
            indptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
            indices = indices[keep]
        row.update(core_leaves=core.counts['core'], n_edges=int(indices.size),
                   n_domain=int(D.sum()), rows_with_edges=int((np.diff(indptr) > 0).sum()),
                   longest_row=int(np.diff(indptr).max()), sweeps=args.sweeps,
                   relation_bytes=int(indices.nbytes + indptr.nbytes))
        H = args.sweeps
        for paths, key in ((False, 'values'), (True, 'values_and_args')):
            runs = []
            for rep in range(args.repeats + 1):
                t0 = time.perf_counter()
                res = invariance.cost_relation(law, indptr, indices, level, D, horizon=H,
                                               return_paths=paths)
                wall = time.perf_counter() - t0
                if rep:                                     # the first call warms up
                    runs.append(dict(wall_s=wall, upload_wall_s=res.seconds_upload,
                                     weights_s=res.seconds_weights, sweeps_s=res.seconds_sweeps,
                                     s_per_sweep=res.seconds_sweeps / H))
            per = [r['s_per_sweep'] for r in runs]
            row[key] = dict(runs=runs, s_per_sweep_min=min(per), s_per_sweep_max=max(per))
        row.update(max_hi=float(res.max_hi[-1]), min_lo=float(res.min_lo[-1]))
        # k_reach_post on the same relation: clear, post and bookkeeping per step
        no_seed = np.full(n, -1, dtype=np.int32)
        runs = []
        for rep in range(args.repeats + 1):
            free = invariance.reach_relation(law, indptr, indices, no_seed, np.nonzero(D)[0],
                                             horizon=H, max_sweeps=H, row_map='wave')
            if rep:
                runs.append(free.seconds_steps / H)
        row.update(reach_post_s_per_step=dict(min=min(runs), max=max(runs)))
        # the numpy mirror of the recurrence on the host
        t0 = time.perf_counter()
        mir = cost_cpu.bounds(indptr, indices, D, res.w_hi, res.w_lo, 2)
        row.update(host_mirror_s_per_sweep=(time.perf_counter() - t0) / 2)
        two = invariance.cost_relation(law, indptr, indices, level, D, horizon=2)
        row.update(mirror_agrees=bool(np.array_equal(mir.hi, two.hi, equal_nan=True) and
                                      np.array_equal(mir.lo, two.lo, equal_nan=True)))
        emit(**row)

    makers = {'headline': headline, 'cwh_z_job1': cwh_job1, 'config3': config3}
    rng = np.random.default_rng(20261021)
    for name in args.trees.split(','):
        orc, V, flat = makers[name]()
        src = explicit.ExplicitMPC(flat, orc)
        double = src.compile()
        src.close()
        plant = simulate.Plant.from_mpc(orc.mpc)
        laws = [(double, 'double'), (double.to_single(flush=True), 'single, flush')]
        for law, precision in laws:
            base = dict(tree=name, law=precision, p=law.p, n_u=law.n_u,
                        leaves=law.stats['n_leaf'])
            if name == 'cwh_z_job1':
                boxes = [('nominal', None)]
                box = process_box(orc.mpc, plant.n_d)
                if box is not None:
                    boxes.append(('process terms', box))
                for label, d_box in boxes:
                    fuel(law, plant, d_box, dict(
                        base, box=label,
                        d_box=None if d_box is None else [list(d_box[0]), list(d_box[1])]), rng,
                        rollouts=label == 'nominal' and precision == 'double')
            else:
                timing(law, plant, dict(base, box='nominal'))
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
