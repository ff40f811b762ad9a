"""
The compiled explicit law on the device (csrc/ehm_compiled.hip): k_compiled_eval
and k_compiled_locate at every width against exact arithmetic (tests/explicit_synth.py) and,
bit for bit, against the numpy mirror (tests/compiled_cpu.py) run on the exported arrays; the
nested reference layout and non-bisection children (test nodes); batch and tree edges; the file
format and the validation of imported arrays; the memory the law takes.

Tolerances (none taken from the code under test): device outputs equal the mirror's exactly; a
state every decision of whose exact walk has a margin above 1e-10 (1 + kappa) must end in the exact
leaf; every other plane turn must be the exact sign of l_j - l_i or one whose exact margin is
within the left child's threshold, and the exact weights in the device's leaf are >= -threshold
(compiled_cpu.check_plane_path); |u - u_exact| <= SynthLaw.u_tol with c = 64 -- the project's bound
for an interpolated input, c doubled from 32 because the gain is built from differences u_i - u_0
of magnitude up to 2 max|U|.
"""

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled
from tests import compiled_cpu as cc
from tests import explicit_synth as es
from tests import helpers

pytestmark = pytest.mark.gpu


def _same(law_c, arrays, X, locate=True):
    """(a): device u, leaf, depth bit-equal to the mirror on the exported arrays."""
    u, leaf, depth, secs = law_c.evaluate(X, return_info=True)
    um, leafm, depthm, smin = cc.evaluate(arrays, X, locate=locate)
    assert np.array_equal(leaf, leafm)
    assert np.array_equal(depth, depthm)
    assert np.array_equal(u, um)
    assert secs >= 0.
    return u, leaf, depth, smin


@pytest.mark.parametrize('p', range(1, 9), ids=lambda p: 'p%d' % p)
def test_every_width_against_exact_arithmetic(p):
    rng = np.random.default_rng(100 + p)
    for keep in (None, 100):
        law = es.SynthLaw(es.kuhn_forest(p, keep), p % 6 + 1, 2, rng)
        assert (law.forest.n_roots >= es.LOCATE_MIN) == (keep is None)
        ex = law.explicit()
        cl = ex.compile()
        ex.close()
        arrays = cl.arrays()
        assert bool(arrays['header'][10]) == (keep is None)        # the locator's table
        X = law.states(rng, 2400)
        u, leaf, depth, _ = _same(cl, arrays, X)
        decisive = 0
        for q, x in enumerate(X):
            ref = law.locate(x)
            k = int(leaf[q])
            if law.decisive(ref):                                  # (b)
                decisive += 1
                assert k == ref.leaf, (q, k, ref.leaf, float(ref.margin), ref.kappa)
            lam = cc.check_plane_path(law, k, ref)                 # (c)
            ue = law.u_exact(k, lam, ref.D)                        # (d)
            tol = law.u_tol(max(ref.kappa, law.kappa(k)), lam, ref.D, c=64.)
            assert np.all(np.abs(u[q] - ue) <= tol), (q, u[q], ue, tol)
        assert decisive >= X.shape[0] // 4
        st = cl.stats                                              # (e)
        assert st['n_test'] == 0
        assert st['n_plane'] == int((law.left >= 0).sum()) and st['n_leaf'] == law.leaves.size
        assert st['n_roots'] == law.forest.n_roots
        cl.close()


def test_nested_reference_layout():
    """The 'lin' partition of test_gpu_explicit.py from the nested tree (its spine: test nodes)
    and from the flat forest (planes only), against ExplicitMPC.evaluate.  Leaves and inputs are
    compared on the 'clear' states, those whose smallest |s| on the path exceeds 1e-9 (more than
    3900 of the 4000, asserted): within rounding of a split face the two walks may end in sibling
    leaves, whose vertex inputs can belong to different commutations, so u need not agree there."""
    from explicit_hybrid_mpc_amd import examples, explicit, partition
    mpc = helpers.make_instance('lin', 0)
    V = examples.box_vertices(examples.theta_box(mpc))
    orc = examples.create_oracle(mpc, V, abs_frac=0.3, abs_err=None, rel_err=0.5)
    root, flat = partition.partition_set(orc, V)
    rng = np.random.default_rng(5)
    half = examples.theta_box(orc.mpc)
    X = rng.uniform(-1, 1, (4000, half.size)) * half
    p = half.size
    for tree in (root, flat):
        ex = explicit.ExplicitMPC(tree, orc)
        cl = ex.compile()
        if tree is root:
            spine = sum(1 for nd in ex.nodes if not nd.is_leaf() and (
                nd.data is None or np.asarray(nd.data.vertices).shape != (p + 1, p)))
            assert spine == flat.info['n_roots'] - 1
            assert cl.stats['n_test'] == spine
        else:
            assert cl.stats['n_test'] == 0
        u_e, leaf_e, _, _ = ex.evaluate(X, return_info=True)
        u, leaf, depth, smin = _same(cl, cl.arrays(), X)
        clear = smin > 1e-9
        assert clear.sum() > 3900
        assert np.array_equal(leaf[clear], leaf_e[clear])
        assert np.allclose(u[clear], u_e[clear], rtol=1e-10, atol=1e-12)
        st = cl.stats
        assert st['bytes'] < st['source_bytes']
        ex.close()
        cl.close()
    orc.close()


def test_non_bisection_children_keep_the_containment_test():
    from explicit_hybrid_mpc_amd import explicit
    ex = explicit.ExplicitMPC(cc.two_point_tree())
    cl = ex.compile()
    assert cl.stats['n_test'] == 1 and cl.stats['n_plane'] == 0 and cl.stats['n_leaf'] == 2
    rng = np.random.default_rng(2)
    X = np.concatenate([rng.uniform(-0.2, 1.2, 1000), 0.5 + np.arange(-20, 21) * 2. ** -53,
                        0.6 + np.arange(-20, 21) * 2. ** -53, [0., 1.]])[:, None]
    u_e, leaf_e, vis_e, _ = ex.evaluate(X, return_info=True)
    u, leaf, depth, _ = _same(cl, cl.arrays(), X)
    assert np.array_equal(leaf, leaf_e) and np.array_equal(depth, vis_e)
    assert set(leaf.tolist()) == {1, 2}
    inside = (X[:, 0] >= 0) & (X[:, 0] <= 1)
    assert np.allclose(u[inside, 0], X[inside, 0], rtol=0, atol=1e-15)
    ex.close()
    cl.close()


def test_edges():
    """n = 0, 1, 257; a single leaf; n_u = 5; -0.0 root coordinates; the source closed."""
    from explicit_hybrid_mpc_amd import explicit
    from explicit_hybrid_mpc_amd.engine import FlatTree
    rng = np.random.default_rng(21)
    law = es.SynthLaw(es.kuhn_forest(3), 5, 1, rng)
    ex = law.explicit()
    cl = ex.compile()
    ex.close()                      # the compiled law holds its own arrays
    arrays = cl.arrays()
    X = law.states(rng, 600)[:257]
    assert X.shape[0] == 257
    for n in (0, 1, 257):
        u, leaf, depth, _ = _same(cl, arrays, X[:n])
        assert u.shape == (n, 5) and leaf.shape == (n,) and depth.shape == (n,)
    for q in range(0, 257, 8):
        ref = law.locate(X[q])
        lam = cc.check_plane_path(law, int(leaf[q]), ref)
        tol = law.u_tol(max(ref.kappa, law.kappa(leaf[q])), lam, ref.D, c=64.)
        assert np.all(np.abs(u[q] - law.u_exact(leaf[q], lam, ref.D)) <= tol)
    u1, t1 = cl(X[40])
    assert np.array_equal(u1, u[40]) and t1 >= 0.
    cl.close()
    # one simplex, no split
    V = np.array([[[0., 0.], [1., 0.], [0., 1.]]])
    U = np.array([[[1., 2.], [3., 5.], [-1., 0.5]]])
    one = FlatTree(V, np.array([-1], np.int32), np.array([-1], np.int32), np.zeros(1, np.int32),
                   np.zeros((1, 3)), U, np.zeros(1, np.uint8), np.zeros(1), {'n_roots': 1}, [0])
    ex = explicit.ExplicitMPC(one)
    cl = ex.compile()
    assert cl.stats['n_plane'] == 0 and cl.stats['n_leaf'] == 1
    Xs = rng.uniform(0, 0.5, (33, 2))
    u, leaf, depth, _ = _same(cl, cl.arrays(), Xs)
    assert (leaf == 0).all() and (depth == 0).all()
    assert np.allclose(u, ex.evaluate(Xs), rtol=1e-13, atol=1e-14)
    ex.close()
    cl.close()
    # roots that write shared zero coordinates as -0.0 (test_negative_zero_vertices...): with
    # every root bisected, vertices are compared by value or these become test nodes
    F = es.KuhnForest([32, 32], -1., 2. ** -4)
    law = es.SynthLaw(F, 1, 1, np.random.default_rng(16), n_sub=40, sliver_depth=6)
    left_half = F.grid[:, 0, 0] < 16
    Vr = law.vertices[:F.n_roots]
    Vr[left_half] = np.where(Vr[left_half] == 0., np.copysign(0., -1.), Vr[left_half])
    assert np.signbit(Vr[left_half][Vr[left_half] == 0.]).any()
    ex = law.explicit()
    cl = ex.compile()
    assert cl.stats['n_test'] == 0 and cl.stats['n_plane'] == int((law.left >= 0).sum())
    cell, a = np.divmod(np.arange(F.n_roots), 2)
    i, j = np.divmod(cell, 32)
    target = ((np.where(i < 31, i + 1, i - 1) * 32 + j) * 2 + a)
    Xz = np.einsum('i,ric->rc', [0.53, 0.29, 0.18], law.vertices[target])   # off every median
    u, leaf, depth, smin = _same(cl, cl.arrays(), Xz)
    u_e, leaf_e, _, _ = ex.evaluate(Xz, return_info=True)
    assert (smin > 1e-9).all() and np.array_equal(leaf, leaf_e)
    assert np.allclose(u, u_e, rtol=1e-10, atol=1e-12)
    ex.close()
    cl.close()


def test_save_load_and_import_validation(tmp_path):
    rng = np.random.default_rng(31)
    law = es.SynthLaw(es.kuhn_forest(4), 3, 1, rng)
    ex = law.explicit()
    cl = ex.compile()
    ex.close()
    X = law.states(rng, 500)
    u, leaf, depth, _ = cl.evaluate(X, return_info=True)
    path = str(tmp_path / 'law.npz')
    cl.save(path)
    back = compiled.CompiledLaw.load(path)
    u2, leaf2, depth2, _ = back.evaluate(X, return_info=True)
    assert np.array_equal(u, u2) and np.array_equal(leaf, leaf2) and np.array_equal(depth, depth2)
    assert back.stats['bytes'] == cl.stats['bytes']
    arrays = cl.arrays()
    for k, v in back.arrays().items():      # by bytes: a child pair read as a double may be a NaN
        assert v.shape == arrays[k].shape and v.tobytes() == arrays[k].tobytes(), k
    back.close()
    # the import's own check: nothing is launched
    for name, bad in cc.malformed(arrays):
        with pytest.raises(_capi.EhmError) as err:
            compiled.CompiledLaw.from_arrays(bad)
        assert err.value.code == _capi.EHM_E_INVALID, name
    # a file of another format version
    np.savez(path, format_version=np.int64(compiled.FORMAT_VERSION + 1), **arrays)
    with pytest.raises(_capi.EhmError) as err:
        compiled.CompiledLaw.load(path)
    assert err.value.code == _capi.EHM_E_INVALID
    cl.close()


def test_memory():
    """bytes = counts x strides, and below the source evaluator's on a tree whose roots are all
    split (a root that stays a leaf keeps its v_0 twice: 8 p bytes more than in the source)."""
    law = es.SynthLaw(es.kuhn_forest(2), 2, 1, np.random.default_rng(41), n_sub=128)
    ex = law.explicit()
    cl = ex.compile()
    st = cl.stats
    want = ((st['n_plane'] + st['n_test']) * st['node_stride'] + st['n_leaf'] * (st['leaf_stride'] + 4)
            + st['n_test'] * st['side_stride'] + st['n_roots'] * (st['side_stride'] + 4)
            + st['nbr_bytes'])
    assert st['bytes'] == want
    assert st['node_stride'] == 64 and st['leaf_stride'] == 8 * cc.leaf_stride(2, 2)
    assert st['nbr_bytes'] == 4 * 3 * law.forest.n_roots
    assert st['bytes'] < st['source_bytes']
    assert st['source_bytes'] == law.n_nodes * (64 + 8 + 3 * 2 * 8) + st['nbr_bytes']
    ex.close()
    cl.close()
