#!/usr/bin/env python
"""
The inverted-pendulum law on the device (needs a GPU):

    python tools/pendulum_bench.py [--max-nodes 2000000] [--n 1000000] [--T 50] [--n-compare 300]

(1) P_theta at the 16 vertices of the box D_x and at the abs_frac-scaled ones: which are feasible,
    and what create_oracle's eps_a rule (lib/examples.py:42-46) gives;
(2) the full partition of example('pendulum', abs_frac, rel_err) from the three sections' Delaunay
    roots, capped at --max-nodes nodes: seconds, leaves, closed volume fraction, depth; if it
    fails, every root on its own, and the roots that finish grown together (parts 3-4 use that);
(3) guarded-rollout throughput (applied plant steps per second of kernel time) against the
    nominal kernel on the same tree (one mode, sliding right, at T_s -- the nominal kernel takes
    at most 4 modes -- one plant step per controller step);
(4) explicit against implicit input usage (sum_t |u_t|) from --n-compare initial states.
One JSON line per part.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_hybrid_mpc_amd import examples, explicit, simulate          # noqa: E402
from explicit_hybrid_mpc_amd.oracle import Oracle                         # noqa: E402


def depth_of(flat):
    depth = np.zeros(flat.n_nodes, dtype=np.int64)
    for k in range(flat.n_nodes):
        if flat.left[k] >= 0:
            depth[flat.left[k]] = depth[flat.right[k]] = depth[k] + 1
    return depth


def emit(d):
    print(json.dumps(d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--abs-frac', type=float, default=0.5)
    ap.add_argument('--rel-err', type=float, default=2.0)
    ap.add_argument('--max-nodes', type=int, default=2000000)
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--T', type=int, default=50)
    ap.add_argument('--n-compare', type=int, default=300)
    ap.add_argument('--T-compare', type=int, default=20)
    a = ap.parse_args()
    law = examples.pendulum(4)
    oracle = Oracle(law, 1., 1.)
    # (1) feasibility at the vertices and the eps_a rule
    V = law.box_vertices()
    J1, _, d1 = oracle.gpu.solve_pt(V)
    Js, _, ds = oracle.gpu.solve_pt(a.abs_frac * V)
    rule_ok = bool((ds >= 0).all())
    eps_a = float(np.max(Js[ds >= 0])) if (ds >= 0).any() else float('nan')
    emit(dict(part='vertices', n_vertices=len(V), feasible_full=int((d1 >= 0).sum()),
              infeasible_full=[V[i].tolist() for i in np.flatnonzero(d1 < 0)],
              feasible_scaled=int((ds >= 0).sum()), abs_frac=a.abs_frac,
              create_oracle_raises=not rule_ok, eps_a_over_feasible_scaled=eps_a,
              J_scaled=[float(x) if d >= 0 else None for x, d in zip(Js, ds)]))
    oracle.eps_a, oracle.eps_r = eps_a, a.rel_err
    oracle.gpu.set_eps(eps_a, a.rel_err)
    # (2) the full partition, capped
    roots, owner = examples.pendulum_roots(law)
    _, _, dv = oracle.gpu.solve_pt(roots.reshape(-1, 4))
    root_ok = (dv.reshape(len(roots), 5) >= 0).all(axis=1)
    tic = time.time()
    try:
        flat = oracle.gpu.partition(np.array(roots), action='ecc', max_nodes=a.max_nodes)
        err = None
    except Exception as e:                     # reported, not hidden
        flat, err = None, '%s: %s' % (type(e).__name__, e)
    secs = time.time() - tic
    total = float(np.prod(2 * np.diag(law.D_x)))
    out = dict(part='partition', abs_frac=a.abs_frac, rel_err=a.rel_err, eps_a=eps_a,
               n_roots=len(roots), roots_per_section=np.bincount(owner).tolist(),
               roots_all_vertices_feasible=int(root_ok.sum()), max_nodes=a.max_nodes,
               seconds=secs, error=err)
    if flat is None:
        # how far it gets: every root on its own, then the roots that finish, together
        fails = []
        for r in range(len(roots)):
            try:
                oracle.gpu.partition(roots[r:r + 1], action='ecc', max_nodes=a.max_nodes,
                                     export=False)
            except Exception as e:
                fails.append(dict(root=r, section=int(owner[r]), error=str(e)))
        good = np.array([r for r in range(len(roots)) if r not in {f['root'] for f in fails}])
        out.update(roots_failing=len(fails), failures=fails[:8],
                   roots_failing_per_section=np.bincount([f['section'] for f in fails],
                                                         minlength=3).tolist())
        if good.size:
            tic = time.time()
            try:
                flat = oracle.gpu.partition(roots[good], action='ecc', max_nodes=a.max_nodes)
            except Exception as e:
                out['good_roots_error'] = str(e)
            out['good_roots_seconds'] = time.time() - tic
            out['good_roots'] = int(good.size)
            out['good_roots_volume_fraction'] = float(
                sum(abs(np.linalg.det(R[1:] - R[0])) / 24. for R in roots[good])) / total
    if flat is not None:
        leaves = flat.left < 0
        closed = leaves & ((flat.flags & 1) != 0)
        dep = depth_of(flat)
        out.update(n_nodes=int(flat.n_nodes), leaves=int(leaves.sum()), closed=int(closed.sum()),
                   depth=int(dep[leaves].max()),
                   volume_closed_fraction=float(flat.info.get('volume_closed', np.nan)) / total)
    emit(out)
    if flat is None or not closed.any():
        return
    # (3) guarded against nominal rollout throughput on the tree
    ex = explicit.ExplicitMPC(flat, types.SimpleNamespace(mpc=law))
    rng = np.random.default_rng(0)
    ks = rng.choice(np.flatnonzero(closed), size=a.n)
    X0 = np.einsum('nj,njc->nc', rng.dirichlet(np.ones(5), size=a.n), flat.vertices[ks])
    guarded = simulate.Plant.from_mpc(law)
    # the nominal kernel takes at most 4 modes: one mode (sliding right) at T_s
    nominal = simulate.Plant(law.A[:1], law.B[:1], law.w[:1], None, [None], np.zeros((0, 4)),
                             np.zeros(0), law.Q, law.R, 'quadratic', T_s=law.T_s)
    rows = {}
    for name, plant, S in (('nominal', nominal, 1), ('guarded', guarded, guarded.substeps)):
        ex.rollout(X0[:1024], 2, record=False, plant=plant)          # warm-up
        res = ex.rollout(X0, a.T, record=False, plant=plant)
        ctrl = int(res.steps.sum())
        rows[name] = dict(controller_steps=ctrl, plant_steps=ctrl * S, kernel_seconds=res.seconds,
                          plant_steps_per_s=ctrl * S / res.seconds,
                          controller_steps_per_s=ctrl / res.seconds,
                          status_counts=np.bincount(res.status, minlength=4).tolist())
    emit(dict(part='rollout', n=a.n, T=a.T, **rows,
              guarded_over_nominal_controller_steps=rows['guarded']['controller_steps_per_s'] /
              rows['nominal']['controller_steps_per_s']))
    ex.close()
    # (4) explicit against implicit input usage
    exo = explicit.ExplicitMPC(flat, oracle)
    im = explicit.ImplicitMPC(oracle)
    Xc = X0[:a.n_compare]
    cmp_ = simulate.compare(exo, im, Xc, a.T_compare)
    emit(dict(part='compare', n=len(Xc), T=a.T_compare,
              overconsumption_total=cmp_['overconsumption_total'],
              cost_ratio_total=cmp_['cost_ratio_total'], u_norm_explicit=cmp_['u_norm_explicit'],
              u_norm_implicit=cmp_['u_norm_implicit'], both_ok=cmp_['both_ok'],
              exits_explicit=cmp_['exits_explicit'], stopped_explicit=cmp_['stopped_explicit'],
              stopped_implicit=cmp_['stopped_implicit'],
              overconsumption_median=float(np.nanmedian(cmp_['overconsumption']))))
    exo.close()
    oracle.close()


if __name__ == '__main__':
    main()
