#!/usr/bin/env python
"""
Invariance of the compiled laws people hold under measurement and input error
(CompiledLaw.robust_successors / robust_core, csrc/ehm_robust.hip; needs a GPU, except
--registers).

    python tools/robust_bench.py [--trees headline,config3,cwh_z_job1] [--trajectories 100000]
                                 [--steps 200] [--out PATH] [--append]
    python tools/robust_bench.py --registers

Trees and laws as tools/core_bench.py: the headline partition, the depth-18 config-3 tree and cwh_z
job 1, each as a double law and as ``to_single(flush=True)``, the plant ``Plant.from_mpc`` of the law's
own model.  Per law:
  'as invariant_core': the robust calls under explicit boxes equal to the box of the 3.8i run (the
  model's box process terms, tools/invariance_bench.process_box; none for a law without them), next
  to ``invariant_core`` under that box in the same process -- the closed-form facet test against the
  located corners, the same relation; the two cores are compared leaf by leaf;
  'noise model': for a law whose model has one (``NoiseModel.from_mpc``: cwh_z), the boxes
  ``bounding_boxes`` makes of it, with ``x_abs`` and ``u_abs``.
Per run: facets, generators, the boxes, counts, core leaves and volume fraction, sweeps, edges, the
worst one-step margin; device seconds of the slack table, of the one-step kernel and of the relation,
wall seconds of ``robust_successors()`` and ``robust_core()`` (one call each after a warm-up of the
kernels' code).  For every non-empty core a rollout check: --trajectories states uniform in the core,
--steps steps of the NOISY rollout under a model that draws from exactly the boxes certified (and,
for the 'noise model' run, under the model itself); the number that stop.  It must be 0: anything
else is a bug in the argument or in the code.  Nothing is promised about the numbers in advance; an
empty core is a finding.  One JSON line per measurement to stdout and, as they come, to
profiles/robust/robust_bench.txt.

--registers writes the figures of the kernels of csrc/ehm_robust.hip to
profiles/robust/registers.txt and those of csrc/ehm_core.hip, which holds the PER_MODE instances of
k_reach next to the shared-E ones, to profiles/core/registers.txt (tools/core_bench.registers; no
GPU).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box_model(p, n_u, n_d, boxes):
    """A NoiseModel that draws uniformly from exactly the boxes (dict by kind of (lo, hi) or None)."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    m = NoiseModel(p, n_u, n_d)
    for kind, box in boxes.items():
        if box is not None:
            m.addIndependentTerm(kind, box[0], box[1])
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--trees', default='headline,config3,cwh_z_job1')
    ap.add_argument('--trajectories', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'robust', 'robust_bench.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--registers', action='store_true')
    args = ap.parse_args()
    from tools import core_bench
    if args.registers:
        core_bench.registers('ehm_robust.hip', None)
        return core_bench.registers('ehm_core.hip', None)
    from explicit_hybrid_mpc_amd import _capi, explicit, simulate
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    from tools.audit_bench import config3, cwh_job1, headline
    from tools.invariance_bench import process_box
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, 'a' if args.append else 'w')
    out.write('# tools/robust_bench.py --trees %s --trajectories %d --steps %d\n' % (
        args.trees, args.trajectories, args.steps))

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return res, time.perf_counter() - t0

    def lists(boxes):
        return {k: None if b is None else [list(map(float, b[0])), list(map(float, b[1]))]
                for k, b in boxes.items()}

    def noisy_stops(law, plant, cells, core, model, rng):
        X0 = core_bench.sample_core(rng, cells.vertices, core, args.trajectories)
        kw = dict(noise=model, seed=20261020) if model.terms else {}    # no box at all: nominal
        status = np.concatenate([
            law.rollout(X0[at:at + 25000], args.steps, plant=plant, record=False,
                        **dict(kw, traj0=at) if kw else {}).status
            for at in range(0, X0.shape[0], 25000)])
        return dict(trajectories=int(X0.shape[0]), steps=args.steps,
                    stopped=int((status != 0).sum()),
                    by_status={int(s): int((status == s).sum()) for s in np.unique(status)})

    makers = {'headline': headline, 'cwh_z_job1': cwh_job1, 'config3': config3}
    rng = np.random.default_rng(20261020)
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
        d_box = process_box(orc.mpc, plant.n_d)
        runs = [('as invariant_core', dict(d_box=d_box))]
        model = NoiseModel.from_mpc(orc.mpc)
        if model is not None:
            runs.append(('noise model', dict(noise=model)))
        for law, precision in laws:
            some = np.arange(min(64, law.stats['n_leaf']))
            law.cells(some)                                         # warm-up: roots, kernels' code
            law.successors(plant=plant, leaves=some)
            law.robust_successors(plant=plant, leaves=some)
            cells = law.cells()
            cap = {}
            try:
                old, t_old = timed(lambda: law.invariant_core(plant=plant, d_box=d_box))
            except _capi.EhmError as e:
                if e.code != _capi.EHM_E_CAPACITY:
                    raise
                cap = dict(max_edges=2 ** 31 - 1)
                old, t_old = timed(lambda: law.invariant_core(plant=plant, d_box=d_box, **cap))
            _, t_old_succ = timed(lambda: law.successors(plant=plant, d_box=d_box))
            for label, kw in runs:
                row = dict(tree=name, law=precision, p=law.p, n_u=law.n_u,
                           leaves=law.stats['n_leaf'], roots=law.stats['n_roots'],
                           plant=dict(n_modes=int(plant.n_modes), n_d=int(plant.n_d)), run=label,
                           **cap)
                one, t_one = timed(lambda: law.robust_successors(plant=plant, **kw))
                res, t_core = timed(lambda: law.robust_core(plant=plant, **dict(kw, **cap)))
                row.update(
                    n_facets=one.n_facets, n_generators=one.n_generators, boxes=lists(one.boxes),
                    x_abs=None if one.x_abs is None else list(map(float, one.x_abs)),
                    u_abs=None if one.u_abs is None else list(map(float, one.u_abs)),
                    one_step_counts=one.counts, worst_margin=one.worst_margin,
                    invariant_volume_fraction=one.invariant_volume_fraction, counts=res.counts,
                    core_leaves=res.counts['core'], core_volume_fraction=res.core_volume_fraction,
                    n_sweeps=res.n_sweeps, n_edges=res.n_edges, set_convex=res.set_convex,
                    holds=res.holds, slack_s=one.seconds_slack, step_s=one.seconds,
                    reach_s=res.seconds_reach, sweeps_s=res.seconds_sweeps,
                    robust_successors_wall_s=t_one, robust_core_wall_s=t_core)
                if label == 'as invariant_core':
                    row.update(invariant_core=dict(
                        counts=old.counts, core_leaves=old.counts['core'],
                        core_volume_fraction=old.core_volume_fraction, n_edges=old.n_edges,
                        reach_s=old.seconds_reach, step_s=old.seeds.seconds,
                        invariant_core_wall_s=t_old, successors_wall_s=t_old_succ,
                        same_core=bool(np.array_equal(old.core, res.core)),
                        same_one_step_status=bool(np.array_equal(old.seeds.status, one.status))))
                if res.core.any():
                    certified = box_model(law.p, law.n_u, plant.n_d, one.boxes)
                    row.update(rollout=noisy_stops(law, plant, cells, res.core, certified, rng))
                    if 'noise' in kw:
                        row.update(rollout_model=noisy_stops(law, plant, cells, res.core,
                                                             kw['noise'], rng))
                else:
                    row.update(rollout='not run: the core is empty')
                emit(**row)
        for law, _ in laws:
            law.close()
        orc.close()
    out.close()


if __name__ == '__main__':
    main()
