#!/usr/bin/env python
"""
The reference's closed-loop experiment under its noise model (needs a GPU):

    python tools/dv_experiment.py [--n 10000] [--n-implicit 256] [--jobs 1,2,3,4,5] [--seed 0]
                                  [--implicit-on-device [--implicit-trajectories N]] [--compiled]

lib/post_process.py:553-568: both laws of cwh_z from x0 = 0 for 20 orbits at T_s = 100 s (1 115
steps, Simulator's time grid), here with NoiseModel.from_mpc (the six terms of
lib/mpc_library.py:236-255) drawn inside the rollout.  Explicit law: --n noisy trajectories;
implicit law: the first --n-implicit of them, with common random numbers (same seed, same
trajectory ids).  Per job the delta-v of total_delta_v_usage (sum_t ||u_t||_2, in mm/s): mean,
median, 5 % and 95 % for both laws, the overconsumption on the common trajectories, and the
paper's single-run numbers (lib/post_process.py:414-417) beside them.  --implicit-on-device runs the
implicit law's loop on the device (rollout(..., on_device=True)), which makes --implicit-trajectories
as large as --n affordable (it overrides --n-implicit); the row then also reports the stalled pairs.
--compiled rolls out the compiled law (ExplicitMPC.compile(), the artefact a user ships) in place of
the partitioner's tree, in the experiment and in the throughput runs, and beside it its
single-precision form (CompiledLaw.to_single()) on the same seed and trajectory ids: per job the
mean and the 5-95 % band of the delta-v under both laws and the largest difference on one
trajectory go to --single-out (default profiles/compiled/dv_single.txt), a line per job as it
finishes.

Then the throughput of the noisy against the nominal rollout, measured in the same call (1e6
trajectories x 100 steps from uniform states, applied trajectory-steps per second of kernel time)
on the cwh_z job-1 tree (the reference model) and on the headline tree (a hand-built
state / input model).
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from explicit_hybrid_mpc_amd import examples, explicit                  # noqa: E402
from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model  # noqa: E402
from rollout_bench import PAPER_EXPLICIT, PAPER_IMPLICIT, cwh_tree, headline_tree  # noqa: E402


def reference_steps(mpc):
    T_f = 20 * 2 * np.pi / mpc.pars['wo']
    return len(np.linspace(0, T_f, int(T_f / mpc.T_s + 1)))


def stats(dv):
    return dict(mean=float(dv.mean()), median=float(np.median(dv)),
                p5=float(np.percentile(dv, 5)), p95=float(np.percentile(dv, 95)))


def law_of(flat, oracle, use_compiled):
    """The explicit law of a partition, or its compiled form (the source closed)."""
    ex = explicit.ExplicitMPC(flat, oracle)
    if not use_compiled:
        return ex
    cl = ex.compile()
    ex.close()
    return cl


def single_law_row(cl, a, n, T, model, seed):
    """The single-precision form of the compiled law ``cl`` on the trajectories of its rollout
    ``a``: the same figures, and how far the two laws part; the refusal if it has no single form."""
    from explicit_hybrid_mpc_amd import _capi
    try:
        single = cl.to_single()
    except _capi.EhmError as err:
        return dict(refused=str(err))
    t0 = time.perf_counter()
    c = single.rollout(np.zeros((n, 2)), T, noise=model, seed=seed, record=False)
    wall = time.perf_counter() - t0
    both = (a.status == 0) & (c.status == 0)
    diff = 1e3 * np.abs(c.u_norm_sum - a.u_norm_sum)[both]
    row = dict(trajectories=n, stopped=int((c.status != 0).sum()),
               max_violation=float(c.max_violation.max()), kernel_s=c.seconds, wall_s=wall,
               dv_mm_s=stats(1e3 * c.u_norm_sum), bytes=single.stats['bytes'],
               double_bytes=cl.stats['bytes'], same_status=int((a.status == c.status).sum()),
               same_steps=int((a.steps == c.steps).sum()),
               dv_diff_max_mm_s=float(diff.max()) if diff.size else None,
               dv_diff_mean_mm_s=float(diff.mean()) if diff.size else None)
    single.close()
    return row


def single_line(r):
    """One job's line of --single-out."""
    e, s = r['explicit'], r['single']
    head = 'job %d  %6d leaves  double: mean %.4f  5%% %.4f  95%% %.4f  stopped %d' % (
        r['job'], r['leaves'], e['dv_mm_s']['mean'], e['dv_mm_s']['p5'], e['dv_mm_s']['p95'],
        e['stopped'])
    if 'refused' in s:
        return head + '  |  single: ' + s['refused']
    d = s['dv_mm_s']
    return head + ('  |  single: mean %.4f  5%% %.4f  95%% %.4f  stopped %d  |  same status %d / %d, '
                   'per trajectory |dv32 - dv64| max %.3g mean %.3g  |  bytes %d -> %d' % (
                       d['mean'], d['p5'], d['p95'], s['stopped'], s['same_status'],
                       s['trajectories'], s['dv_diff_max_mm_s'], s['dv_diff_mean_mm_s'],
                       s['double_bytes'], s['bytes']))


def experiment(job, n, n_im, seed, on_device=False, use_compiled=False):
    oracle, flat = cwh_tree(job)
    mpc = oracle.mpc
    T = reference_steps(mpc)
    model = NoiseModel.from_mpc(mpc)
    ex = law_of(flat, oracle, use_compiled)
    im = explicit.ImplicitMPC(oracle)
    t0 = time.perf_counter()
    a = ex.rollout(np.zeros((n, 2)), T, noise=model, seed=seed, record=False)
    t_ex = time.perf_counter() - t0
    t0 = time.perf_counter()
    b = im.rollout(np.zeros((n_im, 2)), T, noise=model, seed=seed, record=False,
                   **(dict(on_device=True) if on_device else {}))
    t_im = time.perf_counter() - t0
    single = single_law_row(ex, a, n, T, model, seed) if use_compiled else None
    dv_ex, dv_im = 1e3 * a.u_norm_sum, 1e3 * b.u_norm_sum
    ok = (a.status[:n_im] == 0) & (b.status == 0)
    row = dict(job=job, leaves=int(np.sum(flat.left < 0)), T=T, seed=seed,
               law='compiled' if use_compiled else 'explicit',
               explicit=dict(trajectories=n, stopped=int((a.status != 0).sum()),
                             max_violation=float(a.max_violation.max()),
                             kernel_s=a.seconds, wall_s=t_ex, dv_mm_s=stats(dv_ex)),
               implicit=dict(trajectories=n_im, stopped=int((b.status != 0).sum()),
                             max_violation=float(b.max_violation.max()), wall_s=t_im,
                             on_device=bool(on_device),
                             stalled_pairs=getattr(b, 'n_stalled_pairs', None),
                             stalled_trajectories=(int(b.stalled.sum()) if on_device else None),
                             dv_mm_s=stats(dv_im)),
               common=int(ok.sum()),
               overconsumption_pct=100. * (dv_ex[:n_im][ok].sum() - dv_im[ok].sum())
               / dv_im[ok].sum(),
               overconsumption_median_pct=100. * float(np.median(
                   (dv_ex[:n_im][ok] - dv_im[ok]) / dv_im[ok])),
               paper_implicit=PAPER_IMPLICIT[job - 1], paper_explicit=PAPER_EXPLICIT[job - 1],
               paper_overconsumption_pct=100. * (PAPER_EXPLICIT[job - 1] - PAPER_IMPLICIT[job - 1])
               / PAPER_IMPLICIT[job - 1])
    if single is not None:
        row['single'] = single
    print(json.dumps(row), flush=True)
    ex.close()
    oracle.close()
    return row


def throughput(name, mpc, flat, model, n, T, rng, use_compiled=False):
    ex = law_of(flat, types.SimpleNamespace(mpc=mpc), use_compiled)
    half = examples.theta_box(mpc)
    X0 = rng.uniform(-1, 1, (n, half.size)) * half
    ex.rollout(X0[:1024], T, record=False)
    ex.rollout(X0[:1024], T, record=False, noise=model)
    row = dict(tree=name, law='compiled' if use_compiled else 'explicit',
               nodes=int(flat.n_nodes), trajectories=n, T=T, terms=len(model.terms))
    for label, kw in (('nominal', {}), ('noisy', dict(noise=model, seed=1))):
        res = ex.rollout(X0, T, record=False, **kw)
        applied = int(res.steps.sum())
        row[label] = dict(applied_steps=applied, stopped=int((res.status != 0).sum()),
                          kernel_s=res.seconds, steps_per_s=applied / res.seconds)
    row['noisy_over_nominal'] = row['noisy']['steps_per_s'] / row['nominal']['steps_per_s']
    print(json.dumps(row), flush=True)
    ex.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--n-implicit', type=int, default=256)
    ap.add_argument('--implicit-on-device', action='store_true')
    ap.add_argument('--implicit-trajectories', type=int, default=None)
    ap.add_argument('--jobs', default='1,2,3,4,5')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--rate-n', type=int, default=1000000)
    ap.add_argument('--rate-T', type=int, default=100)
    ap.add_argument('--skip-rates', action='store_true')
    ap.add_argument('--compiled', action='store_true')
    ap.add_argument('--single-out', default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'compiled',
        'dv_single.txt'))
    args = ap.parse_args()
    if args.implicit_trajectories is not None:
        if not args.implicit_on_device:
            ap.error('--implicit-trajectories goes with --implicit-on-device')
        args.n_implicit = min(args.implicit_trajectories, args.n)
    rows = []
    for j in (int(j) for j in args.jobs.split(',') if j):
        rows.append(experiment(j, args.n, args.n_implicit, args.seed, args.implicit_on_device,
                               args.compiled))
        if args.compiled:
            os.makedirs(os.path.dirname(os.path.abspath(args.single_out)), exist_ok=True)
            with open(args.single_out, 'w' if len(rows) == 1 else 'a') as f:
                if len(rows) == 1:
                    f.write('delta-v [mm/s] over 20 orbits from x0 = 0 under NoiseModel.from_mpc: '
                            'the compiled law and its single-precision form, %d trajectories each, '
                            'seed %d, the same trajectory ids\n' % (args.n, args.seed))
                f.write(single_line(rows[-1]) + '\n')
    if rows:
        print('\ndelta-v [mm/s] over 20 orbits from x0 = 0 (explicit: %d trajectories, implicit: '
              'the first %d, common random numbers)' % (args.n, args.n_implicit))
        print('job  leaves   implicit mean  med   5%%    95%%  |  explicit mean  med   5%%    95%%'
              '  | over. %%  | paper imp  exp   over. %%')
        for r in rows:
            i, e = r['implicit']['dv_mm_s'], r['explicit']['dv_mm_s']
            print('%3d  %6d   %6.2f %6.2f %6.2f %6.2f | %6.2f %6.2f %6.2f %6.2f | %7.1f | %5.2f %6.2f %7.1f'
                  % (r['job'], r['leaves'], i['mean'], i['median'], i['p5'], i['p95'],
                     e['mean'], e['median'], e['p5'], e['p95'], r['overconsumption_pct'],
                     r['paper_implicit'], r['paper_explicit'], r['paper_overconsumption_pct']))
    if not args.skip_rates:
        rng = np.random.default_rng(0)
        oracle, flat = cwh_tree(1)
        throughput('cwh_z job 1', oracle.mpc, flat, NoiseModel.from_mpc(oracle.mpc), args.rate_n,
                   args.rate_T, rng, args.compiled)
        oracle.close()
        mpc, flat = headline_tree()
        half = examples.theta_box(mpc)
        throughput('headline (configs[2])', mpc, flat, state_input_model(half, mpc.B[0].shape[1]),
                   args.rate_n, args.rate_T, rng, args.compiled)


if __name__ == '__main__':
    main()
