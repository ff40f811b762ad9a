#!/usr/bin/env python
"""
The reach tube and the limit set of the compiled laws people hold (CoreResult.reach,
csrc/ehm_reach.hip; needs a GPU, except --registers).

    python tools/reach_bench.py [--trees cwh_z_job1,config3,headline] [--trajectories 100000]
                                [--steps 200] [--repeats 3] [--out PATH]
    python tools/reach_bench.py --registers [--registers-out PATH]

Trees as tools/core_bench.py builds them, each as a double law and as ``to_single(flush=True)``; the
plant is ``Plant.from_mpc`` of the law's own model.

cwh_z job 1, nominally and under the box of its process terms: the core (all of its set), then
``reach()`` from all core leaves: the limit set's size, ``settle``, ``limit_box`` and
``limit_volume_fraction``; beside them the extremes of the states of --trajectories rollouts of
--steps steps (states uniform in the core, a fresh disturbance of the box each step) from step
``settle`` on.  The extremes must lie inside ``limit_box``: the tool fails otherwise.

The headline law and config 3, ``rows='invariant'`` (``max_edges`` raised to 2^31 - 1 where the
default refuses): ``reach(X0=..., horizon=10)`` from the leaves of 2 000 states uniform in a small
box around the origin (--origin-box of the roots' largest vertex modulus, per coordinate):
``leak_step``, the tube's boxes and sizes, and for both row mappings, --repeats calls each, the device
time per sweep of phase A (push, bookkeeping and box reduction) and per step of phase C (clear,
post, bookkeeping and box reduction), and the wall time of checking and uploading the relation; the
time of the core's own sweeps on the same relation beside them.  Both laws' cores are empty and a box
around the origin holds seeds, so that call leaks at step 0 and makes no step of phases B and C: the
same relation and start are run once more with no leaf called a seed (``no_seeds_*``: 16 sweeps at
most per phase, 10 steps), for the time per sweep of all three phases in both mappings.

Nothing is promised about these numbers in advance.  One JSON line per measurement to stdout and, as
they come, to profiles/reach/reach_bench.txt.  --registers compiles csrc/ehm_reach.hip for gfx950
with -Rpass-analysis=kernel-resource-usage into profiles/reach/registers.txt (no GPU needed).
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
    core_bench.REGISTERS['ehm_reach.hip'] = (
        'reach', 'all static: the counters and the wavefronts\' partial boxes of k_reach_book, the '
        'tree of k_reach_final')
    core_bench.registers('ehm_reach.hip', path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='cwh_z_job1,config3,headline')
    ap.add_argument('--trajectories', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--origin-box', type=float, default=0.02)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reach', 'reach_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--registers', action='store_true')
    ap.add_argument('--registers-out', default=None)
    args = ap.parse_args()
    if args.registers:
        return registers(args.registers_out)
    from explicit_hybrid_mpc_amd import _capi, explicit, invariance, simulate
    from tools.audit_bench import config3, cwh_job1, headline
    from tools.core_bench import sample_core
    from tools.invariance_bench import process_box
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/reach_bench.py --trees %s --trajectories %d --steps %d --repeats %d '
              '--origin-box %g\n' % (args.trees, args.trajectories, args.steps, args.repeats,
                                     args.origin_box))

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return res, time.perf_counter() - t0

    def core_of(law, plant, d_box, row):
        """The core with its edges; the cap raised once where the default refuses."""
        try:
            return timed(lambda: law.invariant_core(plant=plant, d_box=d_box, return_edges=True))
        except _capi.EhmError as e:
            if e.code != _capi.EHM_E_CAPACITY:
                raise
            row.update(max_edges=2 ** 31 - 1)
            return timed(lambda: law.invariant_core(plant=plant, d_box=d_box, return_edges=True,
                                                    max_edges=2 ** 31 - 1))

    def limit_set(law, plant, d_box, row, rng):
        core, t_core = core_of(law, plant, d_box, row)
        res, t_reach = timed(lambda: core.reach())
        row.update(core_leaves=core.counts['core'], n_edges=core.n_edges,
                   set_convex=core.set_convex, closure=int(res.closure.sum()),
                   n_arrival=res.n_arrival, leak_step=res.leak_step, converged=res.converged,
                   holds=res.holds, invariant_core_wall_s=t_core, reach_wall_s=t_reach,
                   boxes_s=res.seconds_boxes, arrival_s=res.seconds_arrival,
                   settle_s=res.seconds_settle, upload_wall_s=res.seconds_upload)
        if res.limit is None:
            row.update(limit='none: the start set leaks or a phase did not finish')
            return emit(**row)
        row.update(limit_leaves=int(res.limit.sum()), settle=res.settle,
                   settle_count=res.settle_count.tolist(), limit_box=res.limit_box.tolist(),
                   closure_box=res.tube_box[-1].tolist(),
                   limit_volume_fraction=res.limit_volume_fraction,
                   closure_volume_fraction=res.closure_volume_fraction)
        # the rollouts: where the states are from step `settle` on
        X0 = sample_core(rng, law.cells().vertices, core.core, args.trajectories)
        lo, hi, stopped, outside = np.full(law.p, np.inf), np.full(law.p, -np.inf), 0, 0
        for at in range(0, X0.shape[0], 25000):
            Xb, d = X0[at:at + 25000], None
            if d_box is not None:
                d = rng.uniform(d_box[0], d_box[1], (args.steps, Xb.shape[0], plant.n_d))
            run = law.rollout(Xb, args.steps, d=d, plant=plant)
            stopped += int((run.status != 0).sum())
            late = run.x[res.settle:args.steps].reshape(-1, law.p)
            late = late[np.isfinite(late).all(axis=1)]
            lo, hi = np.minimum(lo, late.min(axis=0)), np.maximum(hi, late.max(axis=0))
            rows = np.searchsorted(law.leaf_node, run.leaf[res.settle:])
            outside += int((~res.limit[rows[run.leaf[res.settle:] >= 0]]).sum())
        inside = bool((lo >= res.limit_box[0]).all() and (hi <= res.limit_box[1]).all())
        row.update(rollout=dict(trajectories=int(X0.shape[0]), steps=args.steps, stopped=stopped,
                                from_step=res.settle, state_min=lo.tolist(),
                                state_max=hi.tolist(), inside_limit_box=inside,
                                leaves_outside_limit=outside))
        emit(**row)
        if not inside or outside or stopped:
            raise SystemExit('the rollouts leave the limit set: a bug in the argument or the code')

    def tube(law, plant, row, rng, roots_abs):
        core, t_core = core_of(law, plant, None, row)
        half = args.origin_box * roots_abs
        X0 = rng.uniform(-half, half, (2000, law.p))
        row.update(core_leaves=core.counts['core'], n_edges=core.n_edges,
                   relation_bytes=int(core.indices.nbytes + core.indptr.nbytes),
                   invariant_core_wall_s=t_core, core_sweeps=core.n_sweeps,
                   core_sweeps_wall_s=core.seconds_sweeps, origin_half_width=half.tolist())
        for row_map in ('thread', 'wave'):
            runs = []
            for _ in range(args.repeats):
                res, wall = timed(lambda: core.reach(X0=X0, horizon=10, row_map=row_map))
                runs.append(dict(
                    wall_s=wall, upload_wall_s=res.seconds_upload, boxes_s=res.seconds_boxes,
                    arrival_s=res.seconds_arrival, sweeps_arrival=res.sweeps_arrival,
                    arrival_s_per_sweep=res.seconds_arrival / max(res.sweeps_arrival, 1),
                    steps_s=res.seconds_steps, n_steps=len(res.step_count),
                    steps_s_per_step=res.seconds_steps / max(len(res.step_count) - 1, 1)))
            row[row_map] = runs
        # the kernels alone: the same relation and start with no leaf a seed, so that nothing leaks
        # and all three phases run (16 sweeps at most each, 10 steps)
        u, leaf, _, _ = law.evaluate(X0, return_info=True)
        rows = np.unique(np.searchsorted(law.leaf_node, leaf[np.isfinite(u).all(axis=1)]))
        no_seed = np.full(core.level.size, -1, dtype=np.int32)
        for row_map in ('thread', 'wave'):
            runs = []
            for _ in range(args.repeats):
                free = invariance.reach_relation(law, core.indptr, core.indices, no_seed, rows,
                                                 horizon=10, max_sweeps=16, row_map=row_map)
                runs.append(dict(
                    sweeps_arrival=free.sweeps_arrival, sweeps_settle=free.sweeps_settle,
                    arrival_s_per_sweep=free.seconds_arrival / max(free.sweeps_arrival, 1),
                    settle_s_per_sweep=free.seconds_settle / max(free.sweeps_settle, 1),
                    steps_s_per_step=free.seconds_steps / 10, converged=free.converged,
                    closure=int(free.closure.sum()), step_count=free.step_count.tolist()))
            row['no_seeds_' + row_map] = runs
        row.update(start_leaves=int(res.tube_count[0]), n_outside=res.n_outside,
                   leak_step=res.leak_step, n_arrival=res.n_arrival, converged=res.converged,
                   closure=int(res.closure.sum()), tube_count=res.tube_count.tolist(),
                   tube_box=res.tube_box.tolist(), step_count=res.step_count.tolist(),
                   step_box=res.step_box.tolist())
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
        from explicit_hybrid_mpc_amd import applied
        roots_abs = np.abs(applied.root_cells(double)['vertices']).max(axis=(0, 1))
        for law, precision in laws:
            base = dict(tree=name, law=precision, p=law.p, leaves=law.stats['n_leaf'],
                        default_row_map=invariance.ROW_MAP)
            if name == 'cwh_z_job1':
                boxes = [('nominal', None)]
                box = process_box(orc.mpc, plant.n_d)
                if box is not None:
                    boxes.append(('process terms', box))
                for label, d_box in boxes:
                    limit_set(law, plant, d_box, dict(
                        base, box=label,
                        d_box=None if d_box is None else [list(d_box[0]), list(d_box[1])]), rng)
            else:
                tube(law, plant, dict(base, box='nominal'), rng, roots_abs)
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
