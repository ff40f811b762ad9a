#!/usr/bin/env python
"""
ExplicitMPC.evaluate against CompiledLaw.evaluate on one GPU: the same 2^21
uniform states through the headline tree (the partition of configs[1], 1.6 M nodes) and through the
p = 8 spine case of ``bench.py --workload explicit``, in kernel time (the ``secs`` both calls
return) after a warm-up, median and spread of three repeats -- one repeat is the summed kernel time
of ``--calls`` back-to-back calls, the two laws interleaved call by call, so that a sample spans
tens of milliseconds and not one 2 ms launch --, plus the compile time and the device bytes of both forms next to the reference's own estimate of a storage-optimised law
(lib/post_process.py:99-142, get_opt_memreq).

    python tools/compiled_bench.py [--queries N] [--repeats R] [--out FILE]

``--single`` (default output profiles/compiled/single_bench.txt): instead, the double compiled law
against its single-precision form (``CompiledLaw.to_single``) on the same two trees and the same
states in one process, the calls interleaved in the same way: kernel times, their ratio and spread
(a ratio below 1 is reported as such), the device bytes of both laws against the stride formulas,
and how far the two laws agree.  A tree whose law has no single form is reported with the values
that refuse it.  ``--single --flush`` (profiles/compiled/single_flush_bench.txt): the headline tree
alone, narrowed with ``to_single(flush=True)``; the counts of the values set to zero are reported.

``--nested`` (profiles/compiled/nested_bench.txt): the p = 8 spine in the reference's nested layout
(a right spine of data-less nodes, built without recursion), ``compile()`` -- a walk of test nodes --
against ``compile(spine='roots')`` -- the root table and its locator -- on the same states.  The
serial walk makes thousands of containment tests per state, so this case runs ``--nested-queries``
states (default 2^14) and at most 5 calls per repeat.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                            # noqa: E402
from explicit_hybrid_mpc_amd import engine, examples, explicit          # noqa: E402
from explicit_hybrid_mpc_amd import tools as ehm_tools                  # noqa: E402


def reference_opt_memreq(flat, p, n_u, word=8):
    """Bytes of the reference's 'optimized storage ... in which the mixing matrix is stored
    directly' (get_opt_memreq, lib/post_process.py:118-128) for this tree: per leaf a containment
    record p (p + 1) and the inputs n_u (p + 1), per internal node whose left child is no leaf that
    child's containment record."""
    left = np.asarray(flat.left)
    internal = np.nonzero(left >= 0)[0]
    n_leaf = int((left < 0).sum())
    n_rec = int((left[left[internal]] >= 0).sum())
    return word * (n_leaf * (p * (p + 1) + n_u * (p + 1)) + n_rec * p * (p + 1))


def run_case(name, flat, half, n_q, repeats, calls, rng, out):
    ex = explicit.ExplicitMPC(flat)
    t0 = time.perf_counter()
    cl = ex.compile()
    wall = time.perf_counter() - t0
    st = cl.stats
    X = rng.uniform(-1, 1, (n_q, half.size)) * half
    times = {'evaluate': [], 'compiled': []}
    for _ in range(3):                                      # warm-up: buffers, clocks, caches
        for law in (ex, cl):
            law.evaluate(X)
    depth = {}
    for _ in range(repeats):
        total = {'evaluate': 0., 'compiled': 0.}
        for _ in range(calls):                              # interleaved: drift hits both alike
            for law, key in ((ex, 'evaluate'), (cl, 'compiled')):
                u, leaf, vis, secs = law.evaluate(X, return_info=True)
                total[key] += secs
                depth[key] = float(vis.mean())
                if key == 'evaluate':
                    u_e, leaf_e = u, leaf
        for key in total:
            times[key].append(total[key] / calls)
    same = float((leaf == leaf_e).mean())
    du = float(np.abs(u - u_e)[leaf == leaf_e].max()) if same > 0 else float('nan')
    out('case %s: %d nodes, %d roots, p = %d, n_u = %d, %d states; %d repeats, each the mean kernel '
        'time of %d calls' % (name, flat.n_nodes, flat.info['n_roots'], ex.p, ex.n_u, n_q, repeats,
                              calls))
    for key in ('evaluate', 'compiled'):
        t = np.array(times[key])
        out('  %-9s kernel ms: median %.3f  min %.3f  max %.3f  (%.3g states/s, %.1f decisions '
            'per state)' % (key, 1e3 * np.median(t), 1e3 * t.min(), 1e3 * t.max(),
                            n_q / np.median(t), depth[key]))
    te, tc = np.median(times['evaluate']), np.median(times['compiled'])
    spread = max(np.ptp(times['evaluate']), np.ptp(times['compiled']))
    out('  speed-up of the medians: %.2fx  (difference %.3f ms, largest spread %.3f ms)' % (
        te / tc, 1e3 * (te - tc), 1e3 * spread))
    out('  same leaf for %.4f %% of the states; max |u - u_evaluate| there %.3g' % (100 * same, du))
    out('  compile: %.1f ms in the library, %.1f ms with the host copies' % (
        1e3 * cl.compile_seconds, 1e3 * wall))
    out('  nodes: %d plane, %d test, %d leaves; device bytes: compiled %d, evaluator %d (%.2fx); '
        'the reference\'s get_opt_memreq formula on this tree: %d' % (
            st['n_plane'], st['n_test'], st['n_leaf'], st['bytes'], st['source_bytes'],
            st['source_bytes'] / st['bytes'],
            reference_opt_memreq(flat, ex.p, ex.n_u)))
    ex.close()
    cl.close()


def single_bytes(st, p, n_u):
    """``stats['bytes']`` of a single law from the stride formulas (CompiledLaw.stats)."""
    node = 32 if p <= 5 else 64
    leaf = 16 * ((4 * (p + n_u + n_u * p) + 15) // 16)
    return st['n_plane'] * node + st['n_leaf'] * (leaf + 4) + st['n_roots'] * (st['side_stride'] + 4) \
        + st['nbr_bytes']


def run_single_case(name, flat, half, n_q, repeats, calls, rng, out, flush=False):
    from explicit_hybrid_mpc_amd import _capi
    ex = explicit.ExplicitMPC(flat)
    cl = ex.compile()
    ex.close()
    p, n_u, st = cl.p, cl.n_u, cl.stats
    out('case %s: %d nodes, %d roots, p = %d, n_u = %d, %d states; %d repeats, each the mean kernel '
        'time of %d calls' % (name, flat.n_nodes, flat.info['n_roots'], p, n_u, n_q, repeats, calls))
    try:
        t0 = time.perf_counter()
        single = cl.to_single(flush=flush)
        wall = time.perf_counter() - t0
    except _capi.EhmError as err:
        a = cl.arrays()
        tiny = float(np.finfo(np.float32).tiny)
        used = {'node': p + 1, 'leaf_rec': p + n_u + n_u * p}
        out('  no single form: %s' % err)
        for key, cols in used.items():
            v = np.abs(a[key][:, :cols])
            low = (v > 0) & (v < tiny)
            out('  %s: %d of %d values nonzero and below FLT_MIN (in %d of %d records), %d above '
                'FLT_MAX' % (key, int(low.sum()), v.size, int(low.any(axis=1).sum()), v.shape[0],
                             int((v > np.finfo(np.float32).max).sum())))
        cl.close()
        return
    s32 = single.stats
    if flush:
        out('  flushed to zero: %d plane coefficients, %d plane offsets, %d leaf values' % (
            single.flushed['a'], single.flushed['b'], single.flushed['leaf']))
    X = rng.uniform(-1, 1, (n_q, half.size)) * half
    laws = ((cl, 'double'), (single, 'single'))
    for _ in range(3):                                      # warm-up: buffers, clocks, caches
        for law, _ in laws:
            law.evaluate(X)
    times = {'double': [], 'single': []}
    res = {}
    for _ in range(repeats):
        total = {'double': 0., 'single': 0.}
        for _ in range(calls):                              # interleaved: drift hits both alike
            for law, key in laws:
                u, leaf, vis, secs = law.evaluate(X, return_info=True)
                total[key] += secs
                res[key] = (u, leaf, float(vis.mean()))
        for key in total:
            times[key].append(total[key] / calls)
    for key in ('double', 'single'):
        t = np.array(times[key])
        out('  %-6s kernel ms: median %.3f  min %.3f  max %.3f  (%.3g states/s, %.1f decisions per '
            'state)' % (key, 1e3 * np.median(t), 1e3 * t.min(), 1e3 * t.max(), n_q / np.median(t),
                        res[key][2]))
    td, ts = np.median(times['double']), np.median(times['single'])
    spread = max(np.ptp(times['double']), np.ptp(times['single']))
    out('  double / single of the medians: %.3fx  (difference %.3f ms, largest spread %.3f ms)%s' % (
        td / ts, 1e3 * (td - ts), 1e3 * spread, '' if td >= ts else '  -- the single law is SLOWER'))
    same = res['double'][1] == res['single'][1]
    du = float(np.abs(res['double'][0] - res['single'][0])[same].max()) if same.any() else float('nan')
    out('  same leaf for %.4f %% of the states; max |u_single - u_double| there %.3g' % (
        100 * same.mean(), du))
    out('  narrowing: %.1f ms with the allocations' % (1e3 * wall))
    out('  device bytes: double %d (node %d B, leaf %d B), single %d (node %d B, leaf %d B): '
        '%.3fx; the stride formula gives %d for the single law (%s)' % (
            st['bytes'], st['node_stride'], st['leaf_stride'], s32['bytes'], s32['node_stride'],
            s32['leaf_stride'], st['bytes'] / s32['bytes'], single_bytes(s32, p, n_u),
            'matches' if single_bytes(s32, p, n_u) == s32['bytes'] else 'DOES NOT MATCH'))
    cl.close()
    single.close()


def nested_spine(roots, n_u):
    """The roots (leaves with zero inputs) hung off a right spine of data-less nodes, as the
    reference nests its Delaunay pre-partition; iterative: the spine is as deep as it is long."""
    from explicit_hybrid_mpc_amd.tree import NodeData, Tree
    p1 = roots.shape[1]
    leaf = lambda r: Tree(NodeData(roots[r], vertex_inputs=np.zeros((p1, n_u))), top=False)
    R = roots.shape[0]
    root = at = Tree(None)
    for r in range(R - 1):
        at.left = leaf(r)
        at.right = leaf(r + 1) if r == R - 2 else Tree(None, top=False)
        at = at.right
    return root


def run_nested_case(name, roots, n_u, half, n_q, repeats, calls, rng, out):
    t0 = time.perf_counter()
    tree = nested_spine(roots, n_u)
    ex = explicit.ExplicitMPC(tree)
    built = time.perf_counter() - t0
    laws = []
    for key, spine in (('tests', 'tests'), ('roots', 'roots')):
        t0 = time.perf_counter()
        laws.append((ex.compile(spine=spine), key, time.perf_counter() - t0))
    ex.close()
    X = rng.uniform(-1, 1, (n_q, half.size)) * half
    out('case %s: nested layout, %d roots on a spine of %d data-less nodes (built and set up in '
        '%.1f s), p = %d, n_u = %d, %d states; %d repeats, each the mean kernel time of %d calls' % (
            name, roots.shape[0], roots.shape[0] - 1, built, roots.shape[2], n_u, n_q, repeats,
            calls))
    for law, _, _ in laws:                                  # warm-up: buffers, clocks, caches
        law.evaluate(X)
    times = {key: [] for _, key, _ in laws}
    res = {}
    for _ in range(repeats):
        total = dict.fromkeys(times, 0.)
        for _ in range(calls):                              # interleaved: drift hits both alike
            for law, key, _ in laws:
                u, leaf, vis, secs = law.evaluate(X, return_info=True)
                total[key] += secs
                res[key] = (u, leaf, float(vis.mean()))
        for key in total:
            times[key].append(total[key] / calls)
    for law, key, wall in laws:
        t, st = np.array(times[key]), law.stats
        out("  spine='%s' kernel ms: median %.3f  min %.3f  max %.3f  (%.3g states/s, %.1f decisions "
            'per state); %d test nodes, %d roots, %d device bytes, compile %.1f ms' % (
                key, 1e3 * np.median(t), 1e3 * t.min(), 1e3 * t.max(), n_q / np.median(t),
                res[key][2], st['n_test'], st['n_roots'], st['bytes'], 1e3 * wall))
    tt, tr = np.median(times['tests']), np.median(times['roots'])
    out('  tests / roots of the medians: %.1fx  (largest spread %.3f ms)' % (
        tt / tr, 1e3 * max(np.ptp(times['tests']), np.ptp(times['roots']))))
    same = res['tests'][1] == res['roots'][1]
    out('  same leaf for %.4f %% of the states; inputs bit-equal there: %s' % (
        100 * same.mean(), bool(np.array_equal(res['tests'][0][same], res['roots'][0][same]))))
    for law, _, _ in laws:
        law.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--queries', type=int, default=1 << 21)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--single', action='store_true',
                    help='the double compiled law against its single-precision form')
    ap.add_argument('--flush', action='store_true',
                    help='--single: the headline tree narrowed with flush=True')
    ap.add_argument('--nested', action='store_true',
                    help="the nested p = 8 spine: compile() against compile(spine='roots')")
    ap.add_argument('--nested-queries', type=int, default=1 << 14)
    args = ap.parse_args()
    if args.flush and not args.single:
        ap.error('--flush goes with --single')
    case = run_single_case if args.single else run_case
    if args.out is None and (args.single or args.nested):
        args.out = os.path.join(ROOT, 'profiles', 'compiled',
                                'nested_bench.txt' if args.nested else
                                'single_flush_bench.txt' if args.flush else 'single_bench.txt')
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    rng = np.random.default_rng(args.seed)
    if args.nested:
        mpc8 = examples.pwa4_mpc(N=bench.CONFIG5['N'], seed=args.seed)
        half8 = examples.theta_box(mpc8)
        roots8 = np.asarray(ehm_tools.delaunay_roots(examples.box_vertices(half8))[0],
                            dtype=np.float64)
        run_nested_case('p8_spine', roots8, int(mpc8.n_u), half8, args.nested_queries, args.repeats,
                        min(args.calls, 5), rng, out)
        return save()
    mpc = bench.make_mpc('config2', args.seed)
    gp = engine.GpuProblem(mpc.compile(), 1., 1.)
    half = examples.theta_box(mpc)
    V = examples.box_vertices(half)
    J_abs, _, _ = gp.solve_pt(0.02 * V)
    gp.set_eps(float(np.max(J_abs)), 1e-2)
    roots, _ = ehm_tools.delaunay_roots(V)
    flat = gp.partition(roots, action='ecc', export=True, with_volume=False)
    gp.close()
    if args.flush:
        run_single_case('headline_tree', flat, half, args.queries, args.repeats, args.calls, rng, out,
                        flush=True)
        return save()
    case('headline_tree', flat, half, args.queries, args.repeats, args.calls, rng, out)
    mpc8 = examples.pwa4_mpc(N=bench.CONFIG5['N'], seed=args.seed)
    half8 = examples.theta_box(mpc8)
    roots8 = np.asarray(ehm_tools.delaunay_roots(examples.box_vertices(half8))[0], dtype=np.float64)
    K, p8 = roots8.shape[0], roots8.shape[2]
    n_u8 = int(mpc8.n_u)
    leafs = -np.ones(K, dtype=np.int32)
    flat8 = engine.FlatTree(roots8, leafs, leafs.copy(), np.zeros(K, dtype=np.int32),
                            np.zeros((K, p8 + 1)), np.zeros((K, p8 + 1, n_u8)),
                            np.zeros(K, dtype=np.uint8), np.zeros(K), {'n_roots': K}, None)
    case('p8_spine', flat8, half8, args.queries, args.repeats, args.calls, rng, out)
    save()


if __name__ == '__main__':
    main()
