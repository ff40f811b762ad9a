#!/usr/bin/env python
"""
What splitting the leaves of a compiled law does to the closed-loop certificates of the laws people
hold (CompiledLaw.refine, csrc/ehm_refine.hip; needs a GPU, except --registers).

    python tools/refine_bench.py [--trees cwh_z_job1,config3,headline] [--repeats 3]
                                 [--states 1048576] [--trajectories 20000] [--steps 1115] [--out PATH]
    python tools/refine_bench.py --registers [--registers-out PATH]

Trees as tools/audit_bench.py builds them, each as a double law and as ``to_single(flush=True)``; the
plant is ``Plant.from_mpc`` of the law's own model.  Per law:
  ``refine(levels=1)`` wall seconds (median of --repeats) and the device seconds of its plan kernels
  beside ``cells()`` and ``reduce(0.)`` on the same law; bytes before / after, ``max_plane_residual``
  and the stop codes; ``evaluate`` on --states states uniform in the parameter box, kernel seconds
  and mean depth before / after, and whether the inputs are bit-equal.
cwh_z job 1 (every leaf, levels 1 .. 4, and ``max_spread`` at 1/2, 1/4 and 1/8 of the coarse law's
largest spread per input with up to 8 levels): the core, ``settle``, ``limit_box``, the leaves of the
limit set, and ``start_hi``, ``start_lo``, ``best_rate_hi`` of ``cost`` over --steps steps beside the
coarse law's figures and the band of ``u_norm_sum`` of --trajectories nominal rollouts of the coarse
law from states uniform in its core (the refined law is the same function).
The headline law and config 3: the leaves that fail the one-step test (level 0 of the coarse core)
refined 1, 2 and 3 levels -- does a core appear?
The two single laws: ``certify`` after refining only their stalled and uncertified leaves, 1 and 2
levels.
Nothing is promised about these numbers in advance; the tool records what it finds, the figures that
show no gain included.  One JSON line per measurement to stdout and, as they come, to
profiles/refine/refine_bench.txt.  --registers compiles csrc/ehm_refine.hip for gfx950 with
-Rpass-analysis=kernel-resource-usage into profiles/refine/registers.txt (no GPU needed).
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
    core_bench.REGISTERS['ehm_refine.hip'] = (
        'refine', 'all static: the workgroup\'s residuals, and from P = 6 on the cell of every '
        'thread while its solve runs')
    core_bench.registers('ehm_refine.hip', path)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='cwh_z_job1,config3,headline')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--states', type=int, default=1 << 20)
    ap.add_argument('--trajectories', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=1115)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refine', 'refine_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--registers', action='store_true')
    ap.add_argument('--registers-out', default=None)
    args = ap.parse_args()
    if args.registers:
        return registers(args.registers_out)
    from explicit_hybrid_mpc_amd import _capi, certify, explicit, simulate
    from tools.audit_bench import config3, cwh_job1, headline
    from tools.core_bench import sample_core
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/refine_bench.py --trees %s --repeats %d --states %d --trajectories %d '
              '--steps %d\n' % (args.trees, args.repeats, args.states, args.trajectories,
                                args.steps))

    def emit(**row):
        line = json.dumps(row, default=lambda o: o.item() if hasattr(o, 'item') else str(o))
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    med = lambda a: float(np.median(a))

    def timed(fn):
        wall, last = [], None
        for _ in range(args.repeats):
            if last is not None and hasattr(last, 'close'):
                last.close()
            t0 = time.perf_counter()
            last = fn()
            wall.append(time.perf_counter() - t0)
        return med(wall), last

    def evaluate_row(law, X):
        law.evaluate(X[:4096])
        u, _, depth, secs = law.evaluate(X, return_info=True)
        return u, dict(kernel_s=secs, mean_depth=float(depth.mean()), max_depth=int(depth.max()))

    def core_of(law, plant):
        try:
            return law.invariant_core(plant=plant, return_edges=True)
        except _capi.EhmError as e:
            if e.code != _capi.EHM_E_CAPACITY:
                raise
            return law.invariant_core(plant=plant, return_edges=True, max_edges=2 ** 31 - 1)

    def closed_loop(law, plant):
        """The figures of 3.8i, 3.8l and 3.8m on one law."""
        t0 = time.perf_counter()
        core = core_of(law, plant)
        row = dict(leaves=law.stats['n_leaf'], core_leaves=core.counts['core'],
                   core_volume_fraction=core.core_volume_fraction, counts=core.counts,
                   n_edges=core.n_edges, n_sweeps=core.n_sweeps)
        if core.core.any():
            reach = core.reach()
            row.update(settle=reach.settle, converged=reach.converged,
                       limit_leaves=None if reach.limit is None else int(reach.limit.sum()),
                       limit_box=None if reach.limit_box is None else reach.limit_box.tolist())
            if reach.limit is not None and reach.limit.any():
                V = law.cells().vertices[reach.limit]
                whole = [V.min(axis=(0, 1)).tolist(), V.max(axis=(0, 1)).tolist()]
                row.update(limit_cells_box=whole)
            cost = core.cost(horizon=args.steps)
            row.update(start_hi=float(cost.start_hi[-1]), start_lo=float(cost.start_lo[-1]),
                       best_rate_hi=cost.best_rate_hi, best_k_hi=cost.best_k_hi,
                       best_rate_lo=cost.best_rate_lo, cost_holds=cost.holds)
        row.update(wall_s=time.perf_counter() - t0)
        return core, row

    makers = {'headline': headline, 'cwh_z_job1': cwh_job1, 'config3': config3}
    rng = np.random.default_rng(20261021)
    for name in args.trees.split(','):
        orc, V, flat = makers[name]()
        src = explicit.ExplicitMPC(flat, orc)
        double = src.compile()
        src.close()
        plant = simulate.Plant.from_mpc(orc.mpc)
        laws = [(double, 'double'), (double.to_single(flush=True), 'single, flush')]
        X = rng.uniform(V.min(axis=0), V.max(axis=0), (args.states, V.shape[1]))
        for law, precision in laws:
            base = dict(tree=name, law=precision, p=law.p, n_u=law.n_u)
            # -- what a pass costs and what it does to the law -------------------------------------
            law.cells(np.arange(min(64, law.stats['n_leaf'])))
            law.refine(levels=1, leaves=[0]).close()
            law.reduce(0.).close()
            t_cells, _ = timed(law.cells)
            t_reduce, red = timed(lambda: law.reduce(0.))
            red.close()
            t_refine, fine = timed(lambda: law.refine(levels=1))
            r = fine.refinement
            u0, ev0 = evaluate_row(law, X)
            u1, ev1 = evaluate_row(fine, X)
            emit(**base, what='one level', leaves_before=r['n_leaf_before'],
                 leaves_after=r['n_leaf_after'], bytes_before=r['bytes_before'],
                 bytes_after=r['bytes_after'], stops=r['stops'],
                 max_plane_residual=r['max_plane_residual'], refine_wall_s=t_refine,
                 refine_library_s=r['seconds'], refine_plan_kernel_s=r['plan_seconds'],
                 cells_wall_s=t_cells, reduce_wall_s=t_reduce, evaluate_before=ev0,
                 evaluate_after=ev1, states=args.states,
                 inputs_bit_equal=bool(u0.tobytes() == u1.tobytes()))
            fine.close()
            # -- the closed loop -------------------------------------------------------------------
            core, row = closed_loop(law, plant)
            emit(**base, what='closed loop', refinement='none', **row)
            if name == 'cwh_z_job1':
                if precision == 'double' and core.core.any():
                    X0 = sample_core(rng, law.cells().vertices, core.core, args.trajectories)
                    run = law.rollout(X0, args.steps, plant=plant, record=False)
                    spent = run.u_norm_sum
                    emit(**base, what='simulated band', trajectories=int(spent.size),
                         steps=args.steps, stopped=int((run.status != 0).sum()),
                         u_norm_sum_mean=float(spent.mean()), u_norm_sum_min=float(spent.min()),
                         u_norm_sum_p05=float(np.quantile(spent, 0.05)),
                         u_norm_sum_p95=float(np.quantile(spent, 0.95)),
                         u_norm_sum_max=float(spent.max()))
                U = law.cells().inputs
                spread = np.nanmax(U.max(axis=1) - U.min(axis=1), axis=0)
                runs = [('levels=%d' % k, dict(levels=k)) for k in (1, 2, 3, 4)]
                runs += [('max_spread=spread/%d, levels<=8' % k, dict(levels=8, max_spread=spread / k))
                         for k in (2, 4, 8)]
                for label, kw in runs:
                    fine = law.refine(**kw)
                    _, row = closed_loop(fine, plant)
                    emit(**base, what='closed loop', refinement=label,
                         refine=dict(passes=fine.refinement['passes'],
                                     stops=fine.refinement['stops'],
                                     max_plane_residual=fine.refinement['max_plane_residual'],
                                     seconds=fine.refinement['seconds']), **row)
                    fine.close()
            else:
                for levels in (1, 2, 3):
                    fine = law.refine(levels=levels, leaves=core.level == 0)
                    _, row = closed_loop(fine, plant)
                    emit(**base, what='closed loop', refinement='the level-0 leaves, levels=%d' % levels,
                         refine=dict(passes=fine.refinement['passes'],
                                     stops=fine.refinement['stops'],
                                     max_plane_residual=fine.refinement['max_plane_residual'],
                                     seconds=fine.refinement['seconds']), **row)
                    fine.close()
            # -- the certificate of a single law ---------------------------------------------------
            if precision != 'double' and name in ('headline', 'cwh_z_job1'):
                res = law.certify(orc, return_leaves=True)
                open_ = np.isin(res.status, [certify.STATUS_NAMES.index('stalled'),
                                             certify.STATUS_NAMES.index('uncertified')])
                emit(**base, what='certify', refinement='none', counts=res.counts,
                     certified_volume_fraction=res.certified_volume_fraction)
                for levels in (1, 2):
                    if not open_.any():
                        break
                    fine = law.refine(levels=levels, leaves=open_)
                    again = fine.certify(orc)
                    emit(**base, what='certify',
                         refinement='the stalled and uncertified leaves, levels=%d' % levels,
                         leaves_refined=int(open_.sum()), stops=fine.refinement['stops'],
                         counts=again.counts,
                         certified_volume_fraction=again.certified_volume_fraction)
                    fine.close()
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
