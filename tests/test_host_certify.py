"""
The leaf cells of a compiled law on the host (tests/certify_cpu.py, the numpy mirror of
csrc/ehm_certify.hip) against the vertices of the trees the laws were compiled
from, and the device code's host-side bookkeeping under the sanitizers.  No GPU.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

from explicit_hybrid_mpc_amd.engine import FlatTree
from oracle.geometry import split_along_longest_edge
from tests import certify_cpu as zc
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import explicit_synth as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2. ** -52
# |cell - source| <= C_ROOT p kappa_2(E_root) 2^-52 max|v_root|: all of it is the recovery of the
# root's vertices through inv(inv(E)), the midpoints below add none.  The largest ratio the mirror
# measures on the trees of this file is 0.114; C_ROOT is that with a margin of 4,
# rounded up.
C_ROOT = 0.5


def split_tree(p, n_u, seed, n_roots=3, n_split=400, sliver=30):
    """A forest over ``n_roots`` random simplices: ``n_split`` longest-edge bisections of random
    leaves (``oracle.geometry``), then one edge of one leaf bisected ``sliver`` times over.
    Returns (FlatTree, ids of the sliver chain's leaves)."""
    rng = np.random.default_rng([77, p, seed])
    V = [rng.normal(size=(p + 1, p)) * rng.uniform(0.5, 4.) + rng.normal(size=p)
         for _ in range(n_roots)]
    left, right = [-1] * n_roots, [-1] * n_roots

    def bisect(k, edge=None):
        if edge is None:
            S1, S2, (i, j) = split_along_longest_edge(V[k])
        else:
            i, j = edge
            S1, S2 = V[k].copy(), V[k].copy()
            S1[i] = S2[j] = (V[k][i] + V[k][j]) / 2.
        left[k], right[k] = len(V), len(V) + 1
        V.extend([np.array(S1), np.array(S2)])
        left.extend([-1, -1])
        right.extend([-1, -1])
        return left[k], right[k], (int(i), int(j))

    for _ in range(n_split):
        open_ = [k for k in range(len(V)) if left[k] < 0]
        bisect(open_[rng.integers(len(open_))])
    chain = []
    if sliver:
        open_ = [k for k in range(len(V)) if left[k] < 0]
        a, b, edge = bisect(open_[rng.integers(len(open_))])
        for _ in range(sliver - 1):
            k = (a, b)[rng.integers(2)]
            chain.append(a + b - k)
            a, b, _ = bisect(k, edge)
        chain += [a, b]
    K = len(V)
    V = np.array(V)
    U = rng.normal(size=(K, p + 1, n_u))
    flat = FlatTree(V, np.array(left, np.int32), np.array(right, np.int32), np.zeros(K, np.int32),
                    np.zeros((K, p + 1)), U, np.zeros(K, np.uint8), np.zeros(K),
                    {'n_roots': n_roots}, [0])
    return flat, np.array(chain)


def synth_tree(p):
    """A ``SynthLaw`` over the first roots of the Kuhn forest: subtrees of depth 8..20 and sliver
    chains of 26."""
    rng = np.random.default_rng([78, p])
    law = es.SynthLaw(es.kuhn_forest(p, 60), p % 3 + 1, 2, rng, n_sub=9)
    return law.flat, np.array(law.sliver_leaves)


def root_of(flat):
    """The root above every node."""
    n = flat.vertices.shape[0]
    parent = np.full(n, -1, dtype=np.int64)
    for ch in (np.asarray(flat.left), np.asarray(flat.right)):
        k = np.nonzero(ch >= 0)[0]
        parent[ch[k]] = k
    top = np.arange(n)
    while (parent[top] >= 0).any():
        top = np.where(parent[top] >= 0, parent[top], top)
    return top


def recovery_ratio(flat, arrays, V, leaves):
    """max over the leaves of |cell - source| / (p kappa_2(E_root) 2^-52 max|v_root|)."""
    p = V.shape[2]
    src = flat.vertices[arrays['leaf_node'][leaves]]
    top = root_of(flat)[arrays['leaf_node'][leaves]]
    R = flat.vertices[top]
    kappa = np.linalg.cond(np.transpose(R[:, 1:] - R[:, :1], (0, 2, 1)))
    scale = p * kappa * EPS * np.abs(R).max(axis=(1, 2))
    return float((np.abs(V - src).max(axis=(1, 2)) / scale).max())


CASES = [('split', 2), ('split', 3), ('split', 6), ('split', 7), ('synth', 2), ('synth', 3),
         ('synth', 6), ('synth', 7)]


@pytest.fixture(scope='module', params=CASES, ids=['%s-p%d' % c for c in CASES])
def tree(request):
    kind, p = request.param
    flat, chain = split_tree(p, 1 + p % 2, 0) if kind == 'split' else synth_tree(p)
    arrays, _ = cc.compile_flat(flat)
    assert arrays['header'][cc.HEADER.index('n_test')] == 0
    assert arrays['header'][cc.HEADER.index('node_stride')] == (8 if p <= 6 else 16)
    return flat, chain, arrays


def test_cells_from_exact_roots_are_the_source_bit_for_bit(tree):
    flat, chain, arrays = tree
    n_roots = flat.info['n_roots']
    trace = []
    V, status = zc.cells(arrays, roots=flat.vertices[:n_roots], trace=trace)
    assert (status == zc.CELL).all()
    assert np.array_equal(V, flat.vertices[arrays['leaf_node']])
    # at a plane node one vertex is at +1, one at -1 and the others at 0, to the rounding of the
    # inverse the plane was taken from: kappa 2^-52 with kappa up to 2^30 at the end of a sliver
    # chain, far from the 0.5 that separates the two kinds
    s = np.array(trace)
    far = np.abs(np.abs(s) - 1.)
    print('double planes: |s| <= %.3g or | |s| - 1 | <= %.3g' % (
        np.abs(s)[np.abs(s) < 0.5].max(), far[np.abs(s) >= 0.5].max()))
    assert ((np.abs(s) < 1e-4) | (far < 1e-4)).all()
    # the sliver chain's leaves are among them
    assert np.isin(chain, arrays['leaf_node']).all() and chain.size >= 2


def test_cells_from_recovered_roots_are_within_the_recovery_bound(tree):
    flat, _, arrays = tree
    V, status = zc.cells(arrays)
    assert (status == zc.CELL).all()
    ratio = recovery_ratio(flat, arrays, V, np.arange(status.size))
    print('recovery ratio %.3g' % ratio)
    assert ratio <= C_ROOT


def test_float_planes_give_the_same_cells(tree):
    """The planes only choose the two vertices.  Rounding their coefficients to float moves a plane
    value by at most 2^-24 (sum |a_c v_c| + |b|); where that stays below 0.4 the float planes choose
    the vertices the double planes choose (whose values are within 1e-4 of 0 and +-1), so the cell
    is the source's bit for bit.  Beyond it -- deep in a chain that bisects one edge over and over,
    where the single law's own turns are no longer certain either -- a leaf may
    get no cell; it never gets a wrong one."""
    flat, _, arrays = tree
    arrays32 = zc.narrow_flushed(arrays)
    n_roots = flat.info['n_roots']
    mag = np.zeros(zc.header(arrays)['n_leaf'])
    zc.cells(arrays, roots=flat.vertices[:n_roots], magnitude=mag)
    trace = []
    V, status = zc.cells(arrays32, roots=flat.vertices[:n_roots], trace=trace)
    sure = 2. ** -24 * mag < 0.4
    assert (status[sure] == zc.CELL).all() and sure.sum() >= 0.8 * sure.size
    got = status == zc.CELL
    assert np.array_equal(V[got], flat.vertices[arrays32['leaf_node']][got])
    assert np.isnan(V[~got]).all()
    print('float planes: %d of %d leaves without a cell, %d of them unsure' % (
        (~got).sum(), got.size, (~got & ~sure).sum()))
    W, status64 = zc.cells(arrays32)
    assert np.array_equal(status64, status)
    assert np.array_equal(W[got], zc.cells(arrays)[0][got])


def test_vertex_inputs_interpolate_the_source_inputs(tree):
    """The leaf's map at its own vertices gives back the vertex inputs it was made from, to the
    conditioning of the leaf; the single law's to float rounding of the same."""
    flat, chain, arrays = tree
    n_roots = flat.info['n_roots']
    keep = ~np.isin(arrays['leaf_node'], chain)          # slivers: kappa ~ 2^26 and beyond
    leaves = np.nonzero(keep)[0]
    V, status = zc.cells(arrays, leaves, roots=flat.vertices[:n_roots])
    U = zc.vertex_inputs(arrays, leaves, V, status)
    src = flat.vertex_inputs[arrays['leaf_node'][leaves]]
    S = flat.vertices[arrays['leaf_node'][leaves]]
    kappa = np.linalg.cond(np.transpose(S[:, 1:] - S[:, :1], (0, 2, 1)))
    p = V.shape[2]
    tol = 32. * p * kappa * EPS * np.abs(src).max()
    assert (np.abs(U - src).max(axis=(1, 2)) <= tol).all()
    # row 0 is u_0 + K 0
    assert np.array_equal(U[:, 0], src[:, 0])
    assert np.array_equal(U[status == zc.NO_CELL], np.full_like(U[status == zc.NO_CELL], np.nan),
                          equal_nan=True)


def test_a_node_that_is_no_bisection_and_a_deep_chain_give_no_cell():
    flat, chain = split_tree(3, 1, 1, n_split=60, sliver=30)
    arrays, _ = cc.compile_flat(flat)
    h = zc.header(arrays)
    p = h['p']
    ch = zc.children(arrays)
    # the subtree under internal record `bad`: its plane scaled so that no vertex is beyond 0.5
    below = [None] * h['n_int']
    for k in range(h['n_int'] - 1, -1, -1):
        leaves = []
        for c in ch[k]:
            leaves += below[c] if c >= 0 else [~c]
        below[k] = leaves
    bad = next(k for k in range(h['n_int']) if 3 <= len(below[k]) <= 12)
    broken = {k: np.array(v, copy=True) for k, v in arrays.items()}
    broken['node'][bad, :p + 1] *= 0.25
    V, status = zc.cells(broken)
    want = np.zeros(h['n_leaf'], dtype=np.int32)
    want[below[bad]] = zc.NO_CELL
    assert np.array_equal(status, want)
    good, _ = zc.cells(arrays)
    assert np.array_equal(V[want == 0], good[want == 0])
    assert np.isnan(V[want == 1]).all()
    # a bound of 12 levels: exactly the leaves deeper than that have no cell
    par = zc.parents(arrays)
    depth = np.array([len(zc.walk_up(par, l, 1 << 30)[1]) for l in range(h['n_leaf'])])
    assert depth.max() > 30
    V, status = zc.cells(arrays, max_depth=12)
    assert np.array_equal(status == zc.NO_CELL, depth > 12)
    assert np.array_equal(V[depth <= 12], good[depth <= 12])
    # the device's bound on a chain that reaches past it
    deep, _ = cc.compile_flat(zc.chain_tree(2, 300))
    _, status = zc.cells(deep, roots=zc.chain_tree(2, 300).vertices[:1])
    depth = np.array([len(zc.walk_up(zc.parents(deep), l, 1 << 30)[1]) for l in range(301)])
    assert np.array_equal(status == zc.NO_CELL, depth > zc.MAX_DEPTH) and (depth > 256).sum() == 45


def test_parents_and_unreached_records():
    flat, _ = split_tree(2, 1, 2, n_split=20, sliver=0)
    arrays, _ = cc.compile_flat(flat)
    pn, sn, pl, sl = zc.parents(arrays)
    ch = zc.children(arrays)
    entry = arrays['root_entry']
    for r, e in enumerate(entry):
        assert (pn[e] if e >= 0 else pl[~e]) == ~r
    for k in range(ch.shape[0]):
        for side, c in enumerate(ch[k]):
            assert ((pn[c], sn[c]) if c >= 0 else (pl[~c], sl[~c])) == (k, side)
    # a root table that leaves a root out: everything below it is unreached, and has no cell
    cut = {k: np.array(v, copy=True) for k, v in arrays.items()}
    cut['root_entry'][2] = cut['root_entry'][1]
    top = root_of(flat)[arrays['leaf_node']]
    _, status = zc.cells(cut, roots=flat.vertices[[0, 1, 1]])
    assert np.array_equal(status == zc.NO_CELL, top == 2)


class _FakeOracles:
    """Batched oracles of a made-up problem with three commutations over cells in one dimension:
    commutation d is feasible at theta' = (v, u) iff |u| <= LIMIT[d] (the relaxed problem adds 0.5),
    costs J = d + v^2 and stalls where asked; the cell closes iff max Vbar < CLOSE."""
    LIMIT = (1., 2., 3.)
    CLOSE = 2.5

    def __init__(self, widen=0., stall=()):
        self.widen, self.stall, self.calls = widen, set(stall), []

    def point(self, rows, slots, feas):
        self.calls.append(('feas' if feas else 'cost', len(slots)))
        lim = np.array(self.LIMIT)[slots] + self.widen
        if feas:
            return np.abs(rows[:, 1]) - lim, None, np.zeros(len(slots), np.int32)
        st = np.array([1 if (int(d), float(r[0])) in self.stall else 0
                       for d, r in zip(slots, rows)], dtype=np.int32)
        return slots + rows[:, 0] ** 2, None, st

    def bar_e(self, R, Vbar):
        self.calls.append(('test', len(R)))
        tb = Vbar.max(axis=1) - self.CLOSE
        return tb < 0., tb


def test_candidate_rule_order_and_statuses_of_the_mirror():
    V = np.array([[[0.], [1.]], [[1.], [2.]], [[2.], [3.]], [[3.], [4.]], [[4.], [5.]],
                  [[np.nan], [np.nan]]])
    U = np.array([[[0.5], [0.5]],       # all three commutations, the first closes
                  [[1.5], [0.5]],       # commutations 1 and 2 only; costs 2, 5 and 3, 6: none closes
                  [[3.2], [0.]],        # none on the exact problem, commutation 2 on the relaxed one
                  [[9.], [9.]],         # none at all
                  [[np.inf], [0.]],     # no law
                  [[np.nan], [np.nan]]])
    cell = np.array([0, 0, 0, 0, 0, 1], dtype=np.int32)
    exact, relaxed = _FakeOracles(), _FakeOracles(widen=0.5)
    volume = lambda R: np.abs(R[:, 1, 0] - R[:, 0, 0])
    out = zc.certify(V, U, cell, np.array([0.25]), 3, exact.point, relaxed.point, exact.bar_e,
                     volume, 0)
    assert out['status'].tolist() == [zc.CERTIFIED, zc.UNCERTIFIED, zc.UNCERTIFIED,
                                      zc.INADMISSIBLE, zc.NO_LAW, zc.CERT_NO_CELL]
    assert out['n_candidates'].tolist() == [3, 2, 1, 0, 0, 0]
    assert out['tries'].tolist() == [1, 2, 1, 0, 0, 0]
    assert out['relaxed'].tolist() == [0, 0, 1, 0, 0, 0]
    assert out['delta_idx'].tolist() == [0, -1, -1, -1, -1, -1]
    # W = J + cost_u . ubar, of the last candidate tried
    assert np.array_equal(out['W'][0], [0.125, 1.125])
    assert np.array_equal(out['W'][1], [2. + 1. + 0.375, 2. + 4. + 0.125])
    assert np.array_equal(out['W'][2], [2. + 4. + 0.8, 2. + 9.])
    assert np.isnan(out['W'][3:]).all() and np.isnan(out['tbest'][3:]).all()
    assert np.array_equal(out['volume'], [1., 1., 1., 1., 1., np.nan], equal_nan=True)
    assert out['certified_volume'] == 1. and out['worst'] == (2, 11. - 2.5)
    # feasibility for the 4 live leaves x 2 vertices x 3 commutations, then only the candidates
    assert exact.calls[:2] == [('feas', 24), ('cost', 10)]
    assert relaxed.calls == [('feas', 12), ('cost', 2)]
    assert exact.calls[2:] == [('test', 3), ('test', 1)]
    # one try only; a stalled solve sets the cheaper candidate of leaf 1 aside
    once = zc.certify(V, U, cell, np.array([0.25]), 3, exact.point, relaxed.point, exact.bar_e,
                      volume, 1)
    assert once['tries'].tolist() == [1, 1, 1, 0, 0, 0]
    assert np.array_equal(once['W'][1], [1. + 1. + 0.375, 1. + 4. + 0.125])
    stalled = _FakeOracles(stall=[(1, 2.)])
    out = zc.certify(V, U, cell, np.array([0.25]), 3, stalled.point, None, stalled.bar_e, volume,
                     0)
    assert out['status'].tolist() == [zc.CERTIFIED, zc.STALLED, zc.INADMISSIBLE, zc.INADMISSIBLE,
                                      zc.NO_LAW, zc.CERT_NO_CELL]
    assert out['tries'][1] == 1 and out['n_candidates'][1] == 2
    # the order: by the sum of W, the lower commutation on ties, whatever the order of arrival
    cands = [(0, np.array([2., 2.]), False), (1, np.array([1., 3.]), False),
             (2, np.array([0., 1.]), False), (3, np.array([0., 0.]), True)]
    assert zc.candidate_order(cands) == [2, 0, 1]
    cands = [(0, np.array([np.nan, 0.]), False)] + cands
    assert zc.candidate_order(cands) == [3, 1, 2, 0]
    theta, konst, no_law = zc.pack(V, U, cell, np.array([0.25]))
    assert no_law.tolist() == [0, 0, 0, 0, 1, 0] and theta[4, 0].tolist() == [4., 0.]
    assert (theta[5] == 0.).all() and konst[4, 0] == 0. and konst[2, 0] == 0.8


def test_host_helpers_under_the_sanitizers(tmp_path):
    """The parent table, the turn set, the bisected-edge rule and the leaf-id check of
    csrc/ehm_certify_host.h, driven by a stand-alone program built with the address and
    undefined-behaviour sanitizers."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'certify_host_main')
    src = os.path.join(ROOT, 'tests', 'native', 'certify_host_main.cpp')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror', src, '-o', exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'certify host helpers: ok' in out.stdout
