#!/usr/bin/env python
"""
What per-leaf error boxes do to the certificate of the noisy closed loop
(CompiledLaw.robust_successors / robust_core with radii='leaf', csrc/ehm_radii_dev.h, DESIGN.md 3.8k;
needs a GPU).

    python tools/robust_radii_bench.py [--trees cwh_z_job1,headline] [--trajectories 100000]
                                       [--steps 200] [--radius-iters 3] [--out PATH] [--append]

Trees and laws as tools/robust_bench.py.  cwh_z job 1 runs under its own model
(``NoiseModel.from_mpc``); a law whose model has none (the headline law) runs under
``noise.state_input_model`` of its set, for the kernels' time only.  Per law, as a double law and as
``to_single(flush=True)``, the global-box call (``radii='global'``, the path of 3.8j) and the per-leaf
call run next to each other in one process.  Per call: one-step counts, worst margin, core leaves and
volume fraction, sweeps, edges; device seconds of the table kernel (slack / nG), of k_leaf_radii, of the
one-step kernel and of the relation (the per-leaf relation's time holds its own pass of
k_leaf_radii), wall seconds of both calls.  For the per-leaf call the median and the largest half-width
of every box over the live leaves against the global box's, coordinate by coordinate, and of a_L, a'_L
and ubar_L against x_abs and u_abs.  For a non-empty core --trajectories noisy rollouts of --steps steps
under the model itself from states uniform in the core; the number that stop must be 0.  Nothing is
promised about the numbers in advance.  One JSON line per measurement to stdout and to
profiles/robust/robust_radii_bench.txt.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='cwh_z_job1,headline')
    ap.add_argument('--trajectories', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--radius-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'robust',
                                                  'robust_radii_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    args = ap.parse_args()
    from explicit_hybrid_mpc_amd import _capi, explicit, simulate
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    from tools import core_bench
    from tools.audit_bench import config3, cwh_job1, headline
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/robust_radii_bench.py --trees %s --trajectories %d --steps %d '
              '--radius-iters %d\n' % (args.trees, args.trajectories, args.steps, args.radius_iters))

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return res, time.perf_counter() - t0

    def floats(a):
        return None if a is None else [float(v) for v in np.asarray(a).ravel()]

    def widths(one):
        """Per kind: the global half-width, and the median and largest per-leaf one over it."""
        live = one.status < 3
        kinds = dict(process='process', state='state', input='input', state_next='state')
        rows = {}
        for key, kind in kinds.items():
            box = one.leaf_boxes[key]
            if box is None or one.boxes[kind] is None:
                rows[key] = None
                continue
            glob = np.maximum(np.abs(one.boxes[kind][0]), np.abs(one.boxes[kind][1]))
            leaf = np.maximum(np.abs(box[live, 0]), np.abs(box[live, 1]))
            with np.errstate(invalid='ignore', divide='ignore'):
                ratio = leaf / glob
            rows[key] = dict(global_half=floats(glob), median_half=floats(np.median(leaf, axis=0)),
                             largest_half=floats(leaf.max(axis=0)),
                             median_ratio=floats(np.median(ratio, axis=0)),
                             largest_ratio=floats(ratio.max(axis=0)))
        for key, glob in (('x_abs_leaf', one.x_abs), ('x_next_abs', one.x_abs),
                          ('u_abs_leaf', one.u_abs)):
            a = getattr(one, key)[live]
            rows[key] = dict(global_bound=floats(glob), median=floats(np.median(a, axis=0)),
                             largest=floats(a.max(axis=0)))
        return rows

    def noisy_stops(law, plant, cells, core, model, rng):
        X0 = core_bench.sample_core(rng, cells.vertices, core, args.trajectories)
        status = np.concatenate([
            law.rollout(X0[at:at + 25000], args.steps, plant=plant, record=False, noise=model,
                        seed=20261021, traj0=at).status
            for at in range(0, X0.shape[0], 25000)])
        return dict(trajectories=int(X0.shape[0]), steps=args.steps,
                    stopped=int((status != 0).sum()),
                    by_status={int(s): int((status == s).sum()) for s in np.unique(status)})

    makers = {'headline': headline, 'cwh_z_job1': cwh_job1, 'config3': config3}
    rng = np.random.default_rng(20261021)
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
        model = NoiseModel.from_mpc(orc.mpc)
        own = model is not None
        if not own:
            half = np.abs(np.asarray(V)).max(axis=0)
            base = state_input_model(half, double.n_u)
            model = NoiseModel(double.p, double.n_u, plant.n_d)
            model.terms = list(base.terms)
        for law, precision in laws:
            some = np.arange(min(64, law.stats['n_leaf']))
            law.cells(some)                                         # warm-up: roots, kernels' code
            law.robust_successors(plant=plant, leaves=some, noise=model)
            law.robust_successors(plant=plant, leaves=some, noise=model, radii='leaf')
            cells = law.cells()
            for radii in ('global', 'leaf'):
                kw = dict(plant=plant, noise=model, radii=radii, radius_iters=args.radius_iters)
                row = dict(tree=name, law=precision, p=law.p, n_u=law.n_u,
                           leaves=law.stats['n_leaf'], roots=law.stats['n_roots'],
                           plant=dict(n_modes=int(plant.n_modes), n_d=int(plant.n_d)),
                           model='from_mpc' if own else 'state_input_model (kernel time only)',
                           radii=radii)
                one, t_one = timed(lambda: law.robust_successors(**kw))
                try:
                    res, t_core = timed(lambda: law.robust_core(**kw))
                except _capi.EhmError as e:
                    if e.code != _capi.EHM_E_CAPACITY:
                        raise
                    row.update(max_edges=2 ** 31 - 1)
                    res, t_core = timed(lambda: law.robust_core(max_edges=2 ** 31 - 1, **kw))
                row.update(
                    n_facets=one.n_facets, n_generators=one.n_generators,
                    x_abs=floats(one.x_abs), u_abs=floats(one.u_abs),
                    one_step_counts=one.counts, worst_margin=one.worst_margin,
                    invariant_volume_fraction=one.invariant_volume_fraction, counts=res.counts,
                    core_leaves=res.counts['core'], core_volume_fraction=res.core_volume_fraction,
                    levels=int(res.level.max()), n_sweeps=res.n_sweeps, n_edges=res.n_edges,
                    set_convex=res.set_convex, holds=res.holds, table_s=one.seconds_slack,
                    radii_s=one.seconds_radii, step_s=one.seconds, reach_s=res.seconds_reach,
                    sweeps_s=res.seconds_sweeps, robust_successors_wall_s=t_one,
                    robust_core_wall_s=t_core)
                if radii == 'leaf':
                    row.update(radius_iters=args.radius_iters, boxes=widths(one))
                if own and res.core.any():
                    row.update(rollout_model=noisy_stops(law, plant, cells, res.core, model, rng))
                elif own:
                    row.update(rollout_model='not run: the core is empty')
                emit(**row)
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
