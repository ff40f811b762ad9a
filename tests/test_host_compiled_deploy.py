"""
The two deployment options of the compiled law on the host (no GPU; DESIGN.md 3.8c "rooted spine"
and "flushed narrowing"): the mirror tests/compiled_deploy_cpu.py against the double mirror and the
single mirror it is built on.

Flushing: values of magnitude 2^-130, 1e-40 and 2^-127 -- all below FLT_MIN = 2^-126, so their
floats are subnormal -- are written over entries of a synthetic law that are exactly 0 there, which
leaves every normal as it was.  The plain narrowing refuses such a law, the flushing one stores
+0.0 at exactly those places and counts them; on 2000 states (most uniform in random leaves, the
rest in leaves below the touched nodes and in the touched leaves) every turn of the flushed single
law is the double mirror's or within ``turn_bound_flush``, every input within ``u_bound_flush``, and
both bounds hold against the double records in rational arithmetic.  p = 1, 5 (32-byte single
records), 6 (64-byte single, 64-byte double) and 8 (128-byte double).

Rooting: the nested layout of a two-root and of a 130-root forest gives the header and the
root_entry the rule states, and evaluates to the (u, leaf) of the arrays with test nodes.
"""

from fractions import Fraction

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import compiled
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import compiled_deploy_cpu as cd
from tests import explicit_synth as es

N_STATES, N_EXACT = 2000, 300
WIDTHS = (1, 5, 6, 8)


def _states(law, arrays, rows, rng):
    leaves = np.concatenate([rng.choice(law.leaves, N_STATES - 400),
                             arrays['leaf_node'][rng.choice(cd.leaves_below(arrays, rows[0]), 200)],
                             arrays['leaf_node'][rng.choice(rows[1], 200)]])
    w = rng.dirichlet(np.ones(law.p + 1), N_STATES)
    return np.einsum('nv,nvc->nc', w, law.vertices[leaves])


@pytest.mark.parametrize('p', WIDTHS, ids=lambda p: 'p%d' % p)
def test_flushed_narrowing_counts_and_bounds(p, tmp_path):
    law, bad, counts, rows, rng = cd.injected_law(p)
    h = dict(zip(cc.HEADER, (int(v) for v in bad['header'])))
    n_u = h['n_u']
    with pytest.raises(c32.NarrowError) as err:
        c32.narrow(bad)
    assert err.value.reason == 'underflow'
    a32, got = cd.narrow_flush(bad)
    assert got == counts and sum(counts.values()) >= 2
    gn, gl = cd.flushed_masks(bad)
    assert int(gn.sum() + gl.sum()) == sum(counts.values())
    for mask, name in ((gn, 'node'), (gl, 'leaf_rec')):
        at = a32[name][:, :mask.shape[1]][mask]
        assert (at == 0).all() and not np.signbit(at).any(), name
    # everywhere else the flushed law is the plain narrowing of the law before the injection
    clean = {k: np.array(v, copy=True) for k, v in bad.items()}
    clean['node'][:, :p + 1][gn] = 0.
    clean['leaf_rec'][:, :gl.shape[1]][gl] = 0.
    want = c32.narrow(clean)
    for k in want:
        assert a32[k].tobytes() == want[k].tobytes(), k
    compiled.validate_arrays(a32)
    path = str(tmp_path / 'flushed.npz')
    compiled.write_file(path, a32)
    with np.load(path) as z:
        assert int(z['precision']) == 32
    back, _ = compiled.read_file(path)
    for k in a32:
        assert back[k].tobytes() == a32[k].tobytes() and back[k].dtype == a32[k].dtype, k
    # turns
    X = _states(law, bad, rows, rng)
    u64, leaf64, _, _ = cc.evaluate(bad, X)
    u32, leaf32, _, levels = c32.evaluate32(a32, X)
    node64, touched, pairs = bad['node'], set(rows[0]), []
    at_flushed = 0
    for live, nodes, s32, left in levels:
        bound, s64 = cd.turn_bound_flush(bad, nodes, X[live])
        plain, _ = c32.turn_bound(bad, nodes, X[live])
        differs = left != (s64 >= -cc.EPS)
        assert (~differs | (np.abs(s64) <= bound)).all(), (p, np.abs(s64[differs]), bound[differs])
        assert (bound >= plain).all()
        hit = np.isin(nodes, rows[0])
        at_flushed += int(hit.sum())
        pairs += [(int(q), int(k), float(s), float(b)) for q, k, s, b in
                  zip(live[hit], nodes[hit], s32[hit], bound[hit])]
        rest = np.nonzero(~hit)[0][:4]
        pairs += [(int(live[i]), int(nodes[i]), float(s32[i]), float(bound[i])) for i in rest]
    assert at_flushed >= 200            # the states below the touched nodes pass through them
    for q, k, s, b in pairs[:N_EXACT] + [t for t in pairs[N_EXACT:] if t[1] in touched][:N_EXACT]:
        assert abs(Fraction(s) - c32.exact_sum(node64[k], X[q], p)) <= Fraction(b), (p, q, k)
    # inputs, in the same leaf
    same = np.nonzero(leaf64 == leaf32)[0]
    assert 4 * same.size >= 3 * N_STATES, same.size / N_STATES
    l = np.searchsorted(bad['leaf_node'], leaf64[same])
    ub = cd.u_bound_flush(bad, l, X[same])
    assert (ub >= c32.u_bound(bad, l, X[same])).all()
    assert (np.abs(u32[same] - u64[same]) <= ub).all()
    in_touched = np.nonzero(np.isin(l, rows[1]))[0]
    assert in_touched.size >= 100
    check = np.concatenate([in_touched[:N_EXACT], np.arange(min(N_EXACT, same.size))])
    for i in check:
        for c in range(n_u):
            exact = cd.exact_input(bad['leaf_rec'][l[i]], X[same[i]], p, n_u, c)
            assert abs(Fraction(float(u32[same[i], c])) - exact) <= Fraction(float(ub[i, c])), \
                (p, i, c)


def test_flush_keeps_the_other_refusals():
    law, bad, counts, rows, rng = cd.injected_law(5)
    p = 5
    node = bad['node']
    plane = int(np.nonzero((node[:, :p] != 0.).any(axis=1))[0][0])

    def variant(name, row, col, value):
        out = {k: np.array(v, copy=True) for k, v in bad.items()}
        out[name][row, col] = value
        return out

    cases = [('zero normal', variant('node', plane, slice(0, p), 1e-50)),
             ('zero normal', variant('node', plane, slice(0, p), 2. ** -127)),
             ('overflow', variant('node', plane, 1, 1e39)),
             ('overflow', variant('leaf_rec', 0, 2, -np.inf))]
    for reason, arrs in cases:
        with pytest.raises(c32.NarrowError) as err:
            cd.narrow_flush(arrs)
        assert err.value.reason == reason
    with pytest.raises(c32.NarrowError) as err:
        cd.narrow_flush(cc.compile_flat(cc.two_point_tree())[0])
    assert err.value.reason == 'test nodes'
    # a law that needs no flush narrows to the same arrays, with nothing counted
    good, _ = cc.compile_flat(law.flat)
    a32, got = cd.narrow_flush(good)
    assert got == {'a': 0, 'b': 0, 'leaf': 0}
    want = c32.narrow(good)
    for k in want:
        assert a32[k].tobytes() == want[k].tobytes(), k


def _nested(p, n_keep, seed):
    rng = np.random.default_rng(seed)
    law = es.SynthLaw(es.kuhn_forest(p, n_keep), 2, 2, rng, n_sub=min(24, n_keep))
    flat = cd.nested_flat(cd.nest(law))
    return law, flat, rng


@pytest.mark.parametrize('p,n_keep', [(2, 2), (3, 130)], ids=['two-roots', '130-roots'])
def test_root_spine_of_a_nested_forest(p, n_keep):
    law, flat, rng = _nested(p, n_keep, [710, p])
    R = law.forest.n_roots
    assert R == n_keep and flat.vertices.shape[0] == law.n_nodes + R - 1
    tests, _ = cc.compile_flat(flat)
    ht = dict(zip(cc.HEADER, (int(v) for v in tests['header'])))
    assert ht['n_roots'] == 1 and ht['n_test'] == R - 1 and ht['has_nbr'] == 0
    rooted = cd.root_spine(flat)
    compiled.validate_arrays(rooted)
    h = dict(zip(cc.HEADER, (int(v) for v in rooted['header'])))
    assert h['n_test'] == 0 and h['n_roots'] == R and h['has_nbr'] == int(R >= 128)
    assert h['n_int'] == ht['n_int'] - (R - 1) and h['n_leaf'] == ht['n_leaf']
    assert h['n_source_nodes'] == ht['n_source_nodes'] == flat.vertices.shape[0]
    assert np.array_equal(rooted['leaf_node'], tests['leaf_node'])
    assert rooted['leaf_rec'].tobytes() == tests['leaf_rec'].tobytes()
    # root_entry: root i is the node with synth_id i -- an internal index or ~leaf, in source order
    left = np.asarray(flat.left)
    spine = flat.synth_id < 0
    internal = np.cumsum((left >= 0) & ~spine) - 1
    leaf_no = np.cumsum(left < 0) - 1
    for i in range(R):
        k = int(np.nonzero(flat.synth_id == i)[0][0])
        want = internal[k] if left[k] >= 0 else ~leaf_no[k]
        assert rooted['root_entry'][i] == want, i
        assert np.array_equal(rooted['root_rec'][i], cd.side_record(law.vertices[i])), i
    # the same arrays from the test-node arrays alone, given what they lack
    again = cd.root_spine(tests, rooted['root_rec'][-1], law.vertices[:R])
    for k in rooted:
        assert again[k].tobytes() == rooted[k].tobytes(), k
    if h['has_nbr']:
        # the adjacency is the one of the flat forest over the same roots
        assert rooted['nbr'].shape == (R, p + 1)
        sym = [(r, i) for r in range(R) for i in range(p + 1) if rooted['nbr'][r, i] >= 0]
        assert sym and all(r in rooted['nbr'][rooted['nbr'][r, i]] for r, i in sym)
    # evaluation: (u, leaf) of the test-node arrays; the same depth under the serial rule
    X = np.concatenate([law.states(rng, 600), rng.uniform(-1.1, 1.1, (200, p))])
    u_t, leaf_t, depth_t, _ = cc.evaluate(tests, X)
    u_r, leaf_r, depth_r, _ = cc.evaluate(rooted, X)
    assert np.array_equal(leaf_r, leaf_t) and np.array_equal(u_r, u_t)
    u_s, leaf_s, depth_s, _ = cc.evaluate(rooted, X, locate=False)
    assert np.array_equal(leaf_s, leaf_t) and np.array_equal(u_s, u_t)
    assert np.array_equal(depth_s, depth_t)
    if not h['has_nbr']:
        assert np.array_equal(depth_r, depth_t)
    # leaves are the nested tree's ids: through synth_id they are the law's exact leaves
    for q in range(0, X.shape[0], 16):
        ref = law.locate(X[q])
        if law.decisive(ref):
            assert flat.synth_id[leaf_r[q]] == ref.leaf, q
    # the narrowing refuses the test-node arrays for their test nodes, the rooted ones not for that
    with pytest.raises(c32.NarrowError) as err:
        c32.narrow(tests)
    assert err.value.reason == 'test nodes'
    try:
        c32.narrow(rooted)
    except c32.NarrowError as why:
        assert why.reason != 'test nodes'


def test_root_spine_without_a_spine_changes_nothing():
    """A forest (n_roots > 1), a single simplex and a tree whose top node is a plane node."""
    law = es.SynthLaw(es.kuhn_forest(2, 6), 1, 1, np.random.default_rng(3), n_sub=6)
    one = es.SynthLaw(es.KuhnForest([1], 0., 1.), 1, 1, np.random.default_rng(4), n_sub=1)
    for src in (law.flat, cd.nested_flat(cd.nest(one))):
        arrays, _ = cc.compile_flat(src)
        rooted = cd.root_spine(src)
        assert sorted(rooted) == sorted(arrays)
        for k in arrays:
            assert rooted[k].tobytes() == arrays[k].tobytes(), k
    # the two-point tree: one test node on top of two leaves
    arrays, _ = cc.compile_flat(cc.two_point_tree())
    rooted = cd.root_spine(cc.two_point_tree())
    h = dict(zip(cc.HEADER, (int(v) for v in rooted['header'])))
    assert (h['n_roots'], h['n_int'], h['n_test'], h['n_leaf']) == (2, 0, 0, 2)
    assert rooted['root_entry'].tolist() == [~0, ~1]
    X = np.linspace(-0.2, 1.2, 141)[:, None]
    a, b = cc.evaluate(arrays, X), cc.evaluate(rooted, X)
    for i in range(3):
        assert np.array_equal(a[i], b[i])
