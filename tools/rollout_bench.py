#!/usr/bin/env python
"""
Closed-loop simulation throughput and the cwh_z delta-v overconsumption table (needs a GPU).

    python tools/rollout_bench.py [--n 1000000] [--T 100] [--jobs 1,2,3,4,5] [--n-compare 10000]
                                  [--laws [--repeats 3] [--flush]]

Trajectory-steps/s, one JSON line per tree and path:
  (a) fused    ExplicitMPC.rollout: one launch of ehm_explicit_rollout (device time of the kernel,
               and wall time including the host copies); steps counted are the ones applied;
  (b) host     T calls of ExplicitMPC.evaluate plus a numpy plant step, what a caller writes
               without the rollout (wall time; every trajectory runs all T steps, no exit test);
  (c) cpu      the CPU restatement (oracle.explicit_cpu.ExplicitFlatCPU + the numpy plant step),
               one process, a few trajectories, for scale.
--laws runs, instead of all that, the explicit law, the compiled law (ExplicitMPC.compile()) and its
single-precision form (CompiledLaw.to_single()) in one process with the calls interleaved:
--repeats rollouts of each after a warm-up, nominal and under a noise model, kernel time; one JSON
line per tree and case with the applied trajectory-steps/s of each (median, min .. max), the ratios
compiled / explicit and single / compiled, and whether the rollouts ended alike.  A law without a
single form is reported (``single`` holds the refusal) and the other two run; with --flush such a
law is narrowed with ``to_single(flush=True)`` instead and the line carries ``flushed``, the counts
of the values set to zero.
Trees: the headline partition (linear_mpc(0), abs_frac 0.02, eps_r 1e-2, as bench.py) and cwh_z
job 1.  Then simulate.compare on cwh_z jobs 1..5 (lib/post_process.py:484-526 / make_jobs.sh) from
uniform initial states in the box, nominal and with a box-bounded process disturbance; the
paper's overconsumption (lib/post_process.py:414-415, single noisy trajectories) is printed beside
it for context only.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_hybrid_mpc_amd import engine, examples, explicit, simulate   # noqa: E402
from explicit_hybrid_mpc_amd import tools as ehm_tools                   # noqa: E402
from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model  # noqa: E402
from oracle import geometry                                              # noqa: E402
from oracle.explicit_cpu import ExplicitFlatCPU                          # noqa: E402

CWH_FRACS = [0.5, 0.25, 0.1, 0.03, 0.01]
PAPER_IMPLICIT = [4.02, 3.78, 3.74, 3.72, 3.88]       # lib/post_process.py:414-415 [mm/s]
PAPER_EXPLICIT = [40.24, 37.29, 4.79, 2.2, 3.94]


def headline_tree():
    mpc = examples.linear_mpc(seed=0)
    gp = engine.GpuProblem(mpc.compile(), 1., 1.)
    V = examples.box_vertices(examples.theta_box(mpc))
    roots, _ = ehm_tools.delaunay_roots(V)
    gp.set_eps(float(np.max(gp.solve_pt(0.02 * V)[0])), 1e-2)
    flat = gp.partition(roots, action='ecc', max_nodes=1 << 23)
    gp.close()
    return mpc, flat


def cwh_tree(job):
    known = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                        'tests', 'golden', 'known_answers.json')))['runs']
    full_set, _, oracle = examples.example('cwh_z', abs_frac=CWH_FRACS[job - 1],
                                           rel_err=float(known[job - 1]['rel_err']))
    roots, _ = geometry.delaunay_simplices(full_set)
    flat = oracle.gpu.partition(np.array(roots), action='ecc', max_nodes=1 << 24)
    return oracle, flat


def rates(name, mpc, flat, n, T, rng):
    ex = explicit.ExplicitMPC(flat, types.SimpleNamespace(mpc=mpc))
    pl = simulate.Plant.from_mpc(mpc)
    half = examples.theta_box(mpc)
    X0 = rng.uniform(-1, 1, (n, half.size)) * half
    ex.rollout(X0[:1024], T, record=False)                 # warm-up (set-up of the plant, code)
    t0 = time.perf_counter()
    res = ex.rollout(X0, T, record=False)
    wall = time.perf_counter() - t0
    applied = int(res.steps.sum())
    print(json.dumps(dict(tree=name, path='(a) fused rollout', nodes=int(flat.n_nodes),
                          trajectories=n, T=T, applied_steps=applied,
                          stopped=int((res.status != 0).sum()),
                          kernel_s=res.seconds, wall_s=wall,
                          steps_per_s_kernel=applied / res.seconds,
                          steps_per_s_wall=applied / wall)), flush=True)
    m = ex._node_mode
    ex.evaluate(X0[:1024])
    t0 = time.perf_counter()
    x = X0.copy()
    for t in range(T):
        u, leaf, _, _ = ex.evaluate(x, return_info=True)
        x = pl.step(x, u, m[leaf])
    wall = time.perf_counter() - t0
    print(json.dumps(dict(tree=name, path='(b) host loop of evaluate + numpy plant',
                          trajectories=n, T=T, wall_s=wall, steps_per_s_wall=n * T / wall)),
          flush=True)
    cpu = ExplicitFlatCPU(flat.vertices, flat.vertex_inputs, flat.left, flat.right,
                          flat.info['n_roots'])
    nc, Tc = 20, min(T, 10)
    t0 = time.perf_counter()
    for i in range(nc):
        x = X0[i].copy()
        for t in range(Tc):
            u, k = cpu(x)
            x = pl.step(x[None], u[None], m[[k]])[0]
    wall = time.perf_counter() - t0
    print(json.dumps(dict(tree=name, path='(c) CPU restatement, one process',
                          trajectories=nc, T=Tc, wall_s=wall, steps_per_s_wall=nc * Tc / wall)),
          flush=True)
    ex.close()


def both_laws(name, mpc, flat, model, n, T, repeats, rng, flush=False):
    """The explicit law, the compiled law and its single-precision form on the same states in one
    process, calls interleaved."""
    from explicit_hybrid_mpc_amd import _capi
    ex = explicit.ExplicitMPC(flat, types.SimpleNamespace(mpc=mpc))
    cl = ex.compile()
    laws = [('explicit', ex), ('compiled', cl)]
    refusal = None
    try:
        laws.append(('single', cl.to_single()))
    except _capi.EhmError as err:
        refusal = str(err)
        if flush:
            laws.append(('single', cl.to_single(flush=True)))
    flushed = laws[-1][1].flushed if laws[-1][0] == 'single' else None
    half = examples.theta_box(mpc)
    X0 = rng.uniform(-1, 1, (n, half.size)) * half
    for label, kw in (('nominal', {}), ('noisy', dict(noise=model, seed=1))):
        for _, law in laws:
            law.rollout(X0[:1024], T, record=False, **kw)              # warm-up
        secs = {key: [] for key, _ in laws}
        last = {}
        for _ in range(repeats):
            for key, law in laws:
                last[key] = law.rollout(X0, T, record=False, **kw)
                secs[key].append(last[key].seconds)
        a, res = last['explicit'], last['compiled']
        row = dict(tree=name, case=label, nodes=int(flat.n_nodes), trajectories=n, T=T,
                   repeats=repeats, same_steps=int((a.steps == res.steps).sum()),
                   same_status=int((a.status == res.status).sum()))
        for key, r in last.items():
            applied = int(r.steps.sum())
            t = np.array(secs[key])
            row[key] = dict(applied_steps=applied, stopped=int((r.status != 0).sum()),
                            kernel_s=[float(v) for v in t],
                            steps_per_s_median=applied / float(np.median(t)),
                            steps_per_s_min=applied / float(t.max()),
                            steps_per_s_max=applied / float(t.min()))
        row['compiled_over_explicit'] = (row['compiled']['steps_per_s_median']
                                         / row['explicit']['steps_per_s_median'])
        if 'single' in last:
            s = last['single']
            row['single_over_compiled'] = (row['single']['steps_per_s_median']
                                           / row['compiled']['steps_per_s_median'])
            row['single_same_steps'] = int((s.steps == res.steps).sum())
            row['single_same_status'] = int((s.status == res.status).sum())
            both = (s.status == 0) & (res.status == 0)
            row['single_u_norm_rel_max'] = float(np.max(
                np.abs(s.u_norm_sum - res.u_norm_sum)[both]
                / np.maximum(res.u_norm_sum[both], 1e-300))) if both.any() else None
        else:
            row['single'] = refusal
        if flushed is not None:
            row['flushed'] = flushed
            row['refusal_without_flush'] = refusal
        print(json.dumps(row), flush=True)
    for _, law in laws:
        law.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--jobs', default='1,2,3,4,5')
    ap.add_argument('--n-compare', type=int, default=10000)
    ap.add_argument('--skip-rates', action='store_true')
    ap.add_argument('--laws', action='store_true')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--flush', action='store_true',
                    help='--laws: narrow with flush=True where the plain narrowing refuses')
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    if args.laws:
        mpc, flat = headline_tree()
        both_laws('headline (configs[2])', mpc, flat,
                  state_input_model(examples.theta_box(mpc), mpc.B[0].shape[1]), args.n, args.T,
                  args.repeats, rng, args.flush)
        del flat
        oracle, flat = cwh_tree(1)
        both_laws('cwh_z job 1', oracle.mpc, flat, NoiseModel.from_mpc(oracle.mpc), args.n, args.T,
                  args.repeats, rng, args.flush)
        oracle.close()
        return
    if not args.skip_rates:
        mpc, flat = headline_tree()
        rates('headline (configs[2])', mpc, flat, args.n, args.T, rng)
        del flat
        oracle, flat = cwh_tree(1)
        rates('cwh_z job 1', oracle.mpc, flat, args.n, args.T, rng)
        oracle.close()
    table = []
    for job in [int(j) for j in args.jobs.split(',') if j]:
        oracle, flat = cwh_tree(job)
        mpc = oracle.mpc
        ex = explicit.ExplicitMPC(flat, oracle)
        im = explicit.ImplicitMPC(oracle)
        X0 = rng.uniform(-1, 1, (args.n_compare, 2)) * examples.theta_box(mpc)
        d = rng.uniform(-1, 1, (args.T, args.n_compare, 1)) * mpc.pars['w_max']
        for label, dist in (('nominal', None), ('d in +-w_max', d)):
            t0 = time.perf_counter()
            fig = simulate.compare(ex, im, X0, args.T, d=dist)
            row = dict(job=job, leaves=int(np.sum(flat.left < 0)), case=label,
                       trajectories=args.n_compare, T=args.T, both_ok=fig['both_ok'],
                       overconsumption_pct=100 * fig['overconsumption_total'],
                       overconsumption_median_pct=100 * float(np.nanmedian(fig['overconsumption'])),
                       cost_ratio=fig['cost_ratio_total'], exits_explicit=fig['exits_explicit'],
                       stopped_implicit=fig['stopped_implicit'],
                       max_violation_explicit=float(fig['explicit'].max_violation.max()),
                       paper_overconsumption_pct=100 * (PAPER_EXPLICIT[job - 1] - PAPER_IMPLICIT[job - 1])
                       / PAPER_IMPLICIT[job - 1],
                       wall_s=time.perf_counter() - t0)
            table.append(row)
            print(json.dumps(row), flush=True)
        ex.close()
        oracle.close()
    if table:
        print('\njob  leaves  case            over. %   median %   cost ratio  exits  paper %')
        for r in table:
            print('%3d  %6d  %-14s  %7.2f   %8.2f   %10.4f  %5d  %7.1f' % (
                r['job'], r['leaves'], r['case'], r['overconsumption_pct'],
                r['overconsumption_median_pct'], r['cost_ratio'], r['exits_explicit'],
                r['paper_overconsumption_pct']))


if __name__ == '__main__':
    main()
