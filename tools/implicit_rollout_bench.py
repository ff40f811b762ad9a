#!/usr/bin/env python
"""
Throughput of the implicit law in closed loop: the host loop (rollout_implicit, on_device=False)
against the device loop (on_device=True) (needs a GPU).

    python tools/implicit_rollout_bench.py [--repeats 3] [--host-repeats N] [--scale 1.0]
                                           [--paths host,device]

Workloads: cwh_z job 1, 10 000 trajectories x 1 115 steps from x0 = 0 under NoiseModel.from_mpc;
the headline single-commutation law (linear_mpc(0)), 100 000 trajectories x 100 steps from uniform
states in the box.  --scale shrinks the trajectory counts (a quick run).  Per workload and path: one
warm-up on a small batch, then --repeats timed runs; one JSON line each with trajectory-steps/s
(applied steps) by device time (events around the loop's launches; the device loop only) and by
wall time, launches per step and LPs per step, then the median and the spread (max - min) / median
of the repeats.  The baseline to judge the device loop against is the host path run from a checkout
of the parent commit: copy this file into that checkout's tools/ and run it there with
--paths host (the host path needs nothing of the new code), then --paths device here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_hybrid_mpc_amd import examples, explicit, simulate        # noqa: E402
from explicit_hybrid_mpc_amd.noise import NoiseModel                    # noqa: E402
from explicit_hybrid_mpc_amd.oracle import Oracle                       # noqa: E402


def run(name, im, oracle, X0, T, repeats, on_device, **kw):
    nd = oracle.canonical.n_delta
    if on_device:
        kw = dict(kw, on_device=True)      # (a parent checkout's rollout has no such keyword)
    im.rollout(X0[:256], min(T, 8), record=False, **kw)       # warm-up
    rates = []
    for r in range(repeats):
        c0 = oracle.gpu.stats()
        t0 = time.perf_counter()
        res = im.rollout(X0, T, record=False, **kw)
        wall = time.perf_counter() - t0
        c1 = oracle.gpu.stats()
        applied = int(res.steps.sum())
        row = dict(workload=name, path='device loop' if on_device else 'host loop', repeat=r,
                   trajectories=X0.shape[0], T=T, commutations=nd, applied_steps=applied,
                   stopped=int((res.status != 0).sum()), wall_s=wall,
                   steps_per_s_wall=applied / wall)
        if on_device:
            row.update(device_s=res.seconds, steps_per_s_device=applied / res.seconds,
                       launches_per_step=res.launches / max(T, 1),
                       lps_per_step=sum(res.lp_solves) / max(T, 1),
                       phase_one_lps=res.lp_solves[0], point_lps=res.lp_solves[1],
                       stalled_pairs=res.n_stalled_pairs,
                       stalled_phase_one=res.n_stalled_phase_one,
                       stalled_trajectories=int(res.stalled.sum()))
        else:
            row.update(launches_per_step=(c1['kernel_launches'] - c0['kernel_launches']) / max(T, 1),
                       lps_per_step=(c1['lp_solves'] - c0['lp_solves']) / max(T, 1))
        rates.append(row['steps_per_s_wall'])
        print(json.dumps(row), flush=True)
    med = float(np.median(rates))
    print(json.dumps(dict(workload=name, path=row['path'], median_steps_per_s_wall=med,
                          spread=(max(rates) - min(rates)) / med, repeats=repeats)), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--host-repeats', type=int, default=None,
                    help='repeats of the host loop (default: --repeats)')
    ap.add_argument('--paths', default='host,device')
    args = ap.parse_args()
    paths = [dict(host=False, device=True)[k] for k in args.paths.split(',') if k]
    reps = lambda dev: args.repeats if dev or args.host_repeats is None else args.host_repeats
    out = {}
    # cwh_z job 1 under the reference's noise model
    _, _, oracle = examples.example('cwh_z', abs_frac=0.5, rel_err=2.0)
    mpc = oracle.mpc
    T_f = 20 * 2 * np.pi / mpc.pars['wo']
    T = len(np.linspace(0, T_f, int(T_f / mpc.T_s + 1)))
    n = max(1, int(10000 * args.scale))
    im = explicit.ImplicitMPC(oracle)
    kw = dict(noise=NoiseModel.from_mpc(mpc), seed=0)
    for dev in paths:
        out[('cwh_z job 1', dev)] = run('cwh_z job 1', im, oracle, np.zeros((n, 2)), T,
                                        reps(dev), dev, **kw)
    oracle.close()
    # the headline single-commutation law
    mpc = examples.linear_mpc(seed=0)
    oracle = Oracle(mpc, 1., 1.)
    half = examples.theta_box(mpc)
    n = max(1, int(100000 * args.scale))
    X0 = np.random.default_rng(0).uniform(-1, 1, (n, half.size)) * half
    im = explicit.ImplicitMPC(oracle)
    for dev in paths:
        out[('headline', dev)] = run('headline (linear_mpc(0))', im, oracle, X0, 100, reps(dev),
                                     dev)
    oracle.close()
    if len(paths) == 2:
        for name in ('cwh_z job 1', 'headline'):
            print('%s: device loop / host loop = %.2f x (wall, medians)' % (
                name, out[(name, True)] / out[(name, False)]))


if __name__ == '__main__':
    main()
