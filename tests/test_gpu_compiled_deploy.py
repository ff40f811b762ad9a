"""
The two deployment options of the compiled law on the device (DESIGN.md 3.8c "rooted spine" and
"flushed narrowing"): ``compile(spine='roots')`` (ehm_compiled_create_opts) and
``to_single(flush=True)`` (ehm_compiled_narrow_opts, k_compiled_narrow), bit for bit against the
mirror tests/compiled_deploy_cpu.py and against the laws the project already has.

Rooting.  The nested 'lin' partition of test_nested_reference_layout: the rooted law's arrays are
the mirror's, its (u, leaf, depth) the test-node law's; it rolls out (257 x 12) bit-equal to the
mirror and to the law compiled from the flat forest (leaf ids mapped through the nodes' vertices:
the two trees number their nodes differently), has a single form, and survives the file.  Nested
Kuhn forests with the locator on (p = 3, 6, 8): (u, leaf) of the test-node law, the exact leaf on
decisive states.  Flushing: the injected laws of the host test, through ``from_arrays``.
"""

import types

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled, explicit
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import compiled_deploy_cpu as cd
from tests import compiled_rollout_cpu as cr
from tests import explicit_synth as es
from tests import helpers

pytestmark = pytest.mark.gpu

N_TRAJ, T = c32.N_TRAJ, c32.T_STEPS


def _same_arrays(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k         # (child pairs: by bytes)


def _same_rollout(a, b, leaf_map=None):
    for f in cr.BIT_EQUAL + ('u_norm_sum', 'mode'):
        x, y = getattr(a, f), getattr(b, f)
        if f == 'leaf' and leaf_map is not None:
            y = np.where(y >= 0, leaf_map[np.maximum(y, 0)], y)
        assert (x is None) == (y is None), f
        if x is not None:
            assert np.array_equal(x, y, equal_nan=True), f


@pytest.fixture(scope='module')
def lin():
    """The 'lin' partition in both layouts, the nested one compiled both ways."""
    from explicit_hybrid_mpc_amd import examples, partition
    mpc = helpers.make_instance('lin', 0)
    V = examples.box_vertices(examples.theta_box(mpc))
    orc = examples.create_oracle(mpc, V, abs_frac=0.3, abs_err=None, rel_err=0.5)
    root, flat = partition.partition_set(orc, V)
    ex = explicit.ExplicitMPC(root, orc)
    ex_flat = explicit.ExplicitMPC(flat, orc)
    out = types.SimpleNamespace(orc=orc, root=root, flat=flat, ex=ex, ex_flat=ex_flat,
                                tests=ex.compile(), rooted=ex.compile(spine='roots'),
                                by_flat=ex_flat.compile(), half=examples.theta_box(orc.mpc))
    # nested node id -> flat node id, through the vertices
    at = {flat.vertices[k].tobytes(): k for k in range(flat.n_nodes)}
    out.to_flat = np.array([at.get(np.ascontiguousarray(nd.data.vertices, dtype=np.float64)
                                   .tobytes(), -1) if nd.data is not None else -1
                            for nd in ex.nodes])
    yield out
    for law in (out.tests, out.rooted, out.by_flat):
        law.close()
    ex.close()
    ex_flat.close()
    orc.close()


def test_real_partition_rooted(lin):
    R = int(lin.flat.info['n_roots'])
    st = lin.rooted.stats
    assert R > 1 and lin.tests.stats['n_test'] == R - 1
    assert st['n_test'] == 0 and st['n_roots'] == R
    assert st['n_plane'] == lin.tests.stats['n_plane'] == lin.by_flat.stats['n_plane']
    assert st['bytes'] == st['n_plane'] * st['node_stride'] + st['n_leaf'] * (st['leaf_stride'] + 4) \
        + st['n_roots'] * (st['side_stride'] + 4) + st['nbr_bytes']
    assert st['source_bytes'] == lin.tests.stats['source_bytes']
    a_t, a_r, a_f = lin.tests.arrays(), lin.rooted.arrays(), lin.by_flat.arrays()
    # the last root's record is not in the test-node arrays: it is the flat forest's (the same
    # kernel on the same vertices), and so is every other root's
    assert a_r['root_rec'].tobytes() == a_f['root_rec'].tobytes()
    assert a_r['nbr'].tobytes() == a_f['nbr'].tobytes()
    _same_arrays(a_r, cd.root_spine(a_t, a_f['root_rec'][-1], lin.flat.vertices[:R]))
    compiled.validate_arrays(a_r)
    X = np.random.default_rng(5).uniform(-1, 1, (4000, lin.half.size)) * lin.half
    u_t, leaf_t, depth_t, _ = lin.tests.evaluate(X, return_info=True)
    u_r, leaf_r, depth_r, _ = lin.rooted.evaluate(X, return_info=True)
    assert np.array_equal(u_r, u_t) and np.array_equal(leaf_r, leaf_t)
    if R < cc.LOCATE_MIN:
        assert np.array_equal(depth_r, depth_t)
    u_m, leaf_m, depth_m, _ = cc.evaluate(a_r, X)
    assert np.array_equal(u_r, u_m) and np.array_equal(leaf_r, leaf_m)
    assert np.array_equal(depth_r, depth_m)
    # and it is the flat forest's law, node ids apart
    u_f, leaf_f, depth_f, _ = lin.by_flat.evaluate(X, return_info=True)
    assert np.array_equal(u_r, u_f) and np.array_equal(lin.to_flat[leaf_r], leaf_f)
    assert np.array_equal(depth_r, depth_f)
    # a forest has no spine: the flag changes nothing
    again = lin.ex_flat.compile(spine='roots')
    _same_arrays(again.arrays(), a_f)
    assert again.stats == lin.by_flat.stats
    again.close()
    for bad in ('root', None, 'Roots'):
        with pytest.raises(ValueError):
            lin.ex.compile(spine=bad)
    with pytest.raises(ValueError):
        lin.ex.compile(flush=True)


def test_real_partition_closed_loop_single_form_and_file(lin, tmp_path):
    X0 = np.random.default_rng(9).uniform(-1, 1, (N_TRAJ, lin.half.size)) * lin.half
    # the default compile of the nested tree has neither a rollout nor a single form
    with pytest.raises(_capi.EhmError) as err:
        lin.tests.rollout(X0, T)
    assert err.value.code == _capi.EHM_E_INVALID and 'test node' in str(err.value)
    with pytest.raises(_capi.EhmError) as err:
        lin.tests.to_single()
    assert err.value.code == _capi.EHM_E_INVALID and 'test node' in str(err.value)
    # the rooted one rolls out: the mirror on its arrays, and the flat forest's law
    cl = lin.rooted
    assert cl.mpc is lin.orc.mpc
    arrays = cl.arrays()
    res = cl.rollout(X0, T)
    plant = cl._rollout_plant
    cr.assert_same(res, cr.mirror(arrays, cl.leaf_mode, plant, X0, T))
    assert (res.steps > 0).any()
    _same_rollout(lin.by_flat.rollout(X0, T, plant=plant), res, lin.to_flat)
    # single form: the mirror's narrowing (flushed where the partition's inverses carry noise)
    try:
        want = c32.narrow(arrays)
        single = cl.to_single()
        assert single.flushed is None
    except c32.NarrowError as why:
        assert why.reason == 'underflow'
        with pytest.raises(_capi.EhmError):
            cl.to_single()
        want, counts = cd.narrow_flush(arrays)
        single = cl.to_single(flush=True)
        assert single.flushed == counts
    assert single.dtype is np.float32 and np.array_equal(single.leaf_mode, cl.leaf_mode)
    _same_arrays(single.arrays(), want)
    res32 = single.rollout(X0, T, plant=plant)
    cr.assert_same(res32, c32.mirror32(want, single.leaf_mode, plant, X0, T))
    # the file
    for law, ref in ((cl, res), (single, res32)):
        path = str(tmp_path / ('law%d.npz' % (32 if law is single else 64)))
        law.save(path)
        back = compiled.CompiledLaw.load(path)
        assert back.dtype is law.dtype and back.stats['n_roots'] == cl.stats['n_roots']
        _same_arrays(back.arrays(), law.arrays())
        _same_rollout(back.rollout(X0, T, plant=plant), ref)
        back.close()
    single.close()


@pytest.mark.parametrize('p', (3, 6, 8), ids=lambda p: 'p%d' % p)
def test_nested_forest_with_the_locator(p):
    rng = np.random.default_rng(720 + p)
    law = es.SynthLaw(es.kuhn_forest(p, None), p % 4 + 1, 2, rng)
    R = law.forest.n_roots
    assert R >= cc.LOCATE_MIN
    ex = explicit.ExplicitMPC(cd.nest(law), types.SimpleNamespace(mpc=cd.NestedMpc))
    synth_id = np.array([getattr(nd, 'synth_id', -1) for nd in ex.nodes])
    tests, rooted = ex.compile(), ex.compile(spine='roots')
    ex.close()
    assert tests.stats['n_test'] == R - 1 and tests.stats['nbr_bytes'] == 0
    st = rooted.stats
    assert st['n_test'] == 0 and st['n_roots'] == R and st['nbr_bytes'] == 4 * R * (p + 1)
    assert st['n_plane'] == int((law.left >= 0).sum()) and st['n_leaf'] == law.leaves.size
    arrays = rooted.arrays()
    assert arrays['header'][cc.HEADER.index('has_nbr')] == 1
    assert np.array_equal(arrays['nbr'], cd.adjacency(law.vertices[:R]))
    ids = synth_id[rooted.leaf_node]            # the nested tree numbers its nodes level by level
    assert np.array_equal(np.sort(ids), law.leaves)
    assert np.array_equal(rooted.leaf_mode, law.node_mode()[ids])
    X = law.states(rng, 2400)
    u_t, leaf_t, _, _ = tests.evaluate(X, return_info=True)
    u, leaf, depth, _ = rooted.evaluate(X, return_info=True)
    assert np.array_equal(leaf, leaf_t) and np.array_equal(u, u_t)
    u_m, leaf_m, depth_m, _ = cc.evaluate(arrays, X)
    assert np.array_equal(leaf, leaf_m) and np.array_equal(u, u_m)
    assert np.array_equal(depth, depth_m)
    decisive = 0
    for q, x in enumerate(X):
        ref = law.locate(x)
        if law.decisive(ref):
            decisive += 1
            assert synth_id[leaf[q]] == ref.leaf, (q, int(leaf[q]), ref.leaf)
    assert decisive >= X.shape[0] // 4
    tests.close()
    rooted.close()


def test_two_point_tree_rooted():
    ex = explicit.ExplicitMPC(cc.two_point_tree())
    tests, rooted = ex.compile(), ex.compile(spine='roots')
    ex.close()
    st = rooted.stats
    assert (st['n_roots'], st['n_plane'], st['n_test'], st['n_leaf']) == (2, 0, 0, 2)
    # the last root's record is in no array of the test-node law: against the host's inverse
    got = rooted.arrays()
    assert np.allclose(got['root_rec'][-1], cd.side_record(cc.two_point_tree().vertices[2]),
                       rtol=4 * cc.EPS, atol=0)
    _same_arrays(got, cd.root_spine(tests.arrays(), got['root_rec'][-1]))
    rng = np.random.default_rng(2)
    X = np.concatenate([rng.uniform(-0.2, 1.2, 1000), 0.5 + np.arange(-20, 21) * 2. ** -53,
                        0.6 + np.arange(-20, 21) * 2. ** -53, [0., 1.]])[:, None]
    a, b = tests.evaluate(X, return_info=True), rooted.evaluate(X, return_info=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert set(b[1].tolist()) == {1, 2}
    tests.close()
    rooted.close()


def _plants(law, rng, p, n_u):
    """One (kind, plant, rollout arguments) per plant kind, by the recipe of ``case32``."""
    for kind in cr.KINDS:
        cost = 'inf' if (p + n_u + cr.KINDS.index(kind)) % 2 == 0 else 'quadratic'
        kw = dict(tol_exit=1e-9)
        if kind == 'guarded':
            plant = es.random_guarded(rng, p, n_u, law.n_modes, cost, substeps=2, n_rows=5)
        else:
            plant = es.random_plant(rng, p, n_u, law.n_modes, cost, n_d=8 if kind == 'noisy' else 0)
        if kind == 'noisy':
            kw.update(noise=es.random_noise(rng, p, n_u, plant.n_d), seed=int(rng.integers(1 << 40)),
                      traj0=int(rng.integers(1 << 20)))
        elif kind == 'nominal':
            kw['v'] = rng.normal(size=(T, N_TRAJ, p)) * 1e-3
        yield kind, plant, kw


@pytest.mark.parametrize('p', (5, 6), ids=lambda p: 'p%d' % p)
def test_flushed_narrowing_on_the_device(p):
    law, bad, counts, rows, rng = cd.injected_law(p)
    n_u = law.n_u
    cl = compiled.CompiledLaw.from_arrays(bad)
    assert cl.flushed is None
    with pytest.raises(_capi.EhmError) as err:
        cl.to_single()
    assert err.value.code == _capi.EHM_E_INVALID and 'subnormal' in str(err.value)
    single = cl.to_single(flush=True)
    want, got = cd.narrow_flush(bad)
    assert got == counts and single.flushed == counts
    a32 = single.arrays()
    _same_arrays(a32, want)
    st = single.stats
    assert st['bytes'] == st['n_plane'] * st['node_stride'] + st['n_leaf'] * (st['leaf_stride'] + 4) \
        + st['n_roots'] * (st['side_stride'] + 4) + st['nbr_bytes']
    leaves = np.concatenate([rng.choice(law.leaves, 97),
                             bad['leaf_node'][rng.choice(cd.leaves_below(bad, rows[0]), 80)],
                             bad['leaf_node'][rng.choice(rows[1], 80)]])
    X = np.einsum('nv,nvc->nc', rng.dirichlet(np.ones(p + 1), 257), law.vertices[leaves])
    for n in (0, 1, 257):
        u, leaf, depth, _ = single.evaluate(X[:n], return_info=True)
        mu, mleaf, mdepth, _ = c32.evaluate32(a32, X[:n])
        assert u.shape == (n, n_u) and leaf.shape == (n,)
        assert np.array_equal(u, mu) and np.array_equal(leaf, mleaf)
        assert np.array_equal(depth, mdepth)
    # the closed loop, one instance per plant kind
    single.set_leaf_modes(cr.leaf_modes(law, a32))
    X0 = np.concatenate([rng.uniform(-0.9, 0.9, (N_TRAJ - 160, p)), X[97:]])
    assert X0.shape[0] == N_TRAJ
    for kind, plant, kw in _plants(law, rng, p, n_u):
        res = single.rollout(X0, T, plant=plant, **kw)
        cr.assert_same(res, c32.mirror32(a32, single.leaf_mode, plant, X0, T, **kw))
        assert (res.steps > 0).any(), kind
    single.close()
    cl.close()
    # refused under the flag too: a normal that flushes to zero, an overflow
    plane = int(np.nonzero((bad['node'][:, :p] != 0.).any(axis=1))[0][0])
    for word, col, value in (('normal becomes zero', slice(0, p), 2. ** -127),
                             ('overflows', 1, 1e39)):
        worse = {k: np.array(v, copy=True) for k, v in bad.items()}
        worse['node'][plane, col] = value
        with pytest.raises(c32.NarrowError):
            cd.narrow_flush(worse)
        cl = compiled.CompiledLaw.from_arrays(worse)
        with pytest.raises(_capi.EhmError) as err:
            cl.to_single(flush=True)
        assert err.value.code == _capi.EHM_E_INVALID and word in str(err.value), word
        cl.close()
    # a law that needs no flush: the same arrays with and without the flag, nothing counted
    good, _ = cc.compile_flat(law.flat)
    cl = compiled.CompiledLaw.from_arrays(good)
    plain, flushed = cl.to_single(), cl.to_single(flush=True)
    assert plain.flushed is None and flushed.flushed == {'a': 0, 'b': 0, 'leaf': 0}
    _same_arrays(flushed.arrays(), plain.arrays())
    _same_arrays(plain.arrays(), c32.narrow(good))
    for c in (cl, plain, flushed):
        c.close()
