"""
The single-precision compiled law on the device (CompiledLaw.to_single, k_compiled_narrow,
k_compiled_eval32<P>, k_compiled_rollout<float, P, NU, KIND>; DESIGN.md 3.8c "single precision"):
the narrowed arrays, the evaluation and every rollout instantiation bit for bit against the numpy
mirror tests/compiled32_cpu.py; the root every state gets is the double law's; at every applied
step of a rollout (leaf, u) is ``single.evaluate(z)``; every status; the edges; the refusals; the
file; and the reference's first cwh_z job under ``simulate.compare``.
"""

import types

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled, simulate
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import compiled_rollout_cpu as cr
from tests import explicit_synth as es

pytestmark = pytest.mark.gpu

T = c32.T_STEPS
CASES = [(kind, p, nu) for kind in cr.KINDS for p in range(1, 9) for nu in range(1, 5)]
assert len(CASES) == 96
STATUS_SEEN = {kind: set() for kind in cr.KINDS}
STATUS_CAN = {'nominal': {0, 1, 2, 3}, 'noisy': {0, 1, 2, 3}, 'guarded': {0, 1, 3}}


def _same_arrays(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k         # (child pairs: by bytes)


# what ehm_compiled_narrow says where the mirror's ``narrow`` refuses
REFUSAL = {'test nodes': 'test node', 'overflow': 'overflows', 'underflow': 'subnormal',
           'zero normal': 'normal becomes zero'}
DRAWS = 4


def _compile(law):
    """(double law, single law) of a SynthLaw; the source is closed before anything runs.  Where
    the mirror refuses the double law's arrays the device must refuse them for the same reason;
    the single law is None then."""
    ex = law.explicit()
    cl = ex.compile()
    ex.close()
    try:
        c32.narrow(cl.arrays())
    except c32.NarrowError as why:
        with pytest.raises(_capi.EhmError) as err:
            cl.to_single()
        assert err.value.code == _capi.EHM_E_INVALID and REFUSAL[why.reason] in str(err.value)
        return cl, None
    return cl, cl.to_single()


def _case(kind, p, n_u):
    """``compiled32_cpu.case32`` with its law compiled in both precisions: the first draw whose
    law has a single form."""
    for draw in range(DRAWS):
        law, plant, X0, kw = c32.case32(kind, p, n_u, draw)
        cl, single = _compile(law)
        if single is not None:
            return law, plant, X0, kw, cl, single
        cl.close()
    pytest.fail('%d laws in a row without a single form' % DRAWS)


def _top(law, leaf):
    """The root above every leaf id."""
    k = np.asarray(leaf, dtype=np.int64).copy()
    while (law.parent[k] >= 0).any():
        k = np.where(law.parent[k] >= 0, law.parent[k], k)
    return k


# p = 1 and 5: the 32-byte record, its shortest and its full form, 100 roots (the serial rule);
# p = 6 and 8: the 64-byte record with 720 and 40 320 roots (the locator), 8 the odd tail
@pytest.mark.parametrize('p,n_keep', [(1, 100), (5, 100), (6, None), (8, None)],
                         ids=['p1', 'p5', 'p6-locator', 'p8-locator'])
def test_to_single_and_evaluate_match_the_mirror(p, n_keep):
    for draw in range(DRAWS):
        rng = np.random.default_rng([40, p, draw])
        law = es.SynthLaw(es.kuhn_forest(p, n_keep), p % 4 + 1, 2, rng)
        cl, single = _compile(law)
        if single is not None:
            break
        cl.close()
    assert single is not None
    assert cl.dtype is np.float64 and single.dtype is np.float32
    a64, a32 = cl.arrays(), single.arrays()
    _same_arrays(a32, c32.narrow(a64))
    assert (a32['header'][cc.HEADER.index('has_nbr')] == 1) == (n_keep is None)
    # the stride formulas and the bytes they give
    st, n_u = single.stats, single.n_u
    assert st['node_stride'] == (32 if p <= 5 else 64) == 4 * compiled.node_stride32(p)
    assert st['leaf_stride'] == 4 * compiled.leaf_stride32(p, n_u)
    assert st['leaf_stride'] == 16 * ((4 * (p + n_u + n_u * p) + 15) // 16) and st['n_test'] == 0
    assert st['bytes'] == st['n_plane'] * st['node_stride'] + st['n_leaf'] * (st['leaf_stride'] + 4) \
        + st['n_roots'] * (st['side_stride'] + 4) + st['nbr_bytes']
    assert st['bytes'] < cl.stats['bytes'] and st['source_bytes'] == cl.stats['source_bytes']
    # ExplicitMPC.compile(dtype=np.float32) is the same law in one call
    ex = law.explicit()
    direct = ex.compile(dtype=np.float32)
    ex.close()
    assert direct.dtype is np.float32 and np.array_equal(direct.leaf_mode, single.leaf_mode)
    _same_arrays(direct.arrays(), a32)
    direct.close()
    inside = np.einsum('nv,nvc->nc', rng.dirichlet(np.ones(p + 1), 160),
                       law.vertices[rng.choice(law.leaves, 160)])
    X = np.concatenate([inside, law.states(rng, 64)[:64], rng.uniform(-1, 1, (64, p))])[:257]
    assert X.shape[0] == 257
    for n in (0, 1, 257):
        u, leaf, depth, _ = single.evaluate(X[:n], return_info=True)
        mu, mleaf, mdepth, _ = c32.evaluate32(a32, X[:n])
        assert u.shape == (n, n_u) and leaf.shape == (n,)
        assert np.array_equal(u, mu) and np.array_equal(leaf, mleaf)
        assert np.array_equal(depth, mdepth)
    # the root is the double law's for every state (and the one the double mirror chooses)
    _, leaf64, _, _ = cl.evaluate(X, return_info=True)
    root = c32.choose_root(a64, X)[0]
    assert np.array_equal(_top(law, leaf), root) and np.array_equal(_top(law, leaf64), root)
    assert 4 * (leaf == leaf64).sum() >= 3 * 160
    # a state no float holds is walked all the same (the index only grows), to a NaN input
    huge = np.full((1, p), 1e39)
    assert np.array_equal(single.evaluate(huge), c32.evaluate32(a32, huge)[0], equal_nan=True)
    cl.close()
    single.close()


def _run_case(kind, p, n_u):
    law, plant, X0, kw, cl, single = _case(kind, p, n_u)
    cl.close()
    arrays = single.arrays()
    assert np.array_equal(single.leaf_mode, cr.leaf_modes(law, arrays))
    res = single.rollout(X0, T, plant=plant, **kw)
    mir = c32.mirror32(arrays, single.leaf_mode, plant, X0, T, **kw)
    cr.assert_same(res, mir)
    STATUS_SEEN[kind].update(int(s) for s in np.unique(res.status))
    return law, plant, single, res, mir, kw


@pytest.mark.parametrize('kind,p,n_u', CASES, ids=['%s-p%d-nu%d' % c for c in CASES])
def test_rollout_instantiation(kind, p, n_u):
    """257 trajectories x 12 steps bit for bit against the mirror; at every applied step (leaf, u)
    is ``single.evaluate`` of the measured state."""
    law, plant, single, res, mir, kw = _run_case(kind, p, n_u)
    assert (res.steps > 0).any()
    applied = 0
    for t in range(T):
        on = np.nonzero(res.steps > t)[0]
        if on.size == 0:
            continue
        z = mir.z[t, on]
        if kind != 'guarded' and t > 0:
            v_t = res.v[t, on] if kind == 'noisy' else kw['v'][t, on]
            assert np.array_equal(z, res.x[t, on] + v_t)
        else:
            assert np.array_equal(z, res.x[t, on])
        u, leaf, _, _ = single.evaluate(z, return_info=True)
        assert np.array_equal(u, res.u[t, on]) and np.array_equal(leaf, res.leaf[t, on])
        applied += on.size
    assert applied >= c32.N_TRAJ // 4
    single.close()


def test_every_status_code_occurs():
    """Each status the plant kind can produce occurs in the sweep (cases not run yet run here)."""
    for kind, p, n_u in CASES:
        if STATUS_SEEN[kind] >= STATUS_CAN[kind]:
            continue
        _run_case(kind, p, n_u)[2].close()
    for kind in cr.KINDS:
        assert STATUS_SEEN[kind] >= STATUS_CAN[kind], (kind, STATUS_SEEN[kind])


def test_batch_edges_exit_tolerance_and_nan_states():
    """n = 0, 1 and 257 with tol_exit = 0 and 1e-9, T = 0, NaN initial states."""
    law, plant, X0, kw, cl, single = _case('nominal', 3, 2)
    cl.close()
    arrays = single.arrays()
    rng = np.random.default_rng(7)
    for n in (0, 1, 257):
        for tol in (0., 1e-9):
            kw2 = dict(tol_exit=tol, v=rng.normal(size=(T, n, 3)) * 1e-3)
            res = single.rollout(X0[:n], T, plant=plant, **kw2)
            assert res.x_final.shape == (n, 3) and res.steps.shape == (n,)
            cr.assert_same(res, c32.mirror32(arrays, single.leaf_mode, plant, X0[:n], T, **kw2))
    res = single.rollout(X0, 0, plant=plant)
    assert np.array_equal(res.x_final, X0) and (res.steps == 0).all() and (res.status == 0).all()
    Xn = X0[:5].copy()
    Xn[1, 2] = np.nan
    Xn[3] = np.nan
    res = single.rollout(Xn, 4, plant=plant)
    assert (res.status[[1, 3]] == 1).all() and (res.steps[[1, 3]] == 0).all()
    cr.assert_same(res, c32.mirror32(arrays, single.leaf_mode, plant, Xn, 4))
    single.close()


def test_traj0_split_under_noise():
    """Two part batches (traj0 offset) equal one whole batch."""
    law, plant, X0, kw, cl, single = _case('noisy', 4, 1)
    cl.close()
    whole = single.rollout(X0, T, plant=plant, **kw)
    h = X0.shape[0] // 2
    kw_b = dict(kw, traj0=kw['traj0'] + h)
    parts = (single.rollout(X0[:h], T, plant=plant, **kw),
             single.rollout(X0[h:], T, plant=plant, **kw_b))
    for f in cr.BIT_EQUAL + ('u_norm_sum', 'mode'):
        w = getattr(whole, f)
        axis = 0 if w.ndim == 1 or f == 'x_final' else 1
        both = np.concatenate([getattr(q, f) for q in parts], axis=axis)
        assert np.array_equal(w, both, equal_nan=True), f
    single.close()


def test_saved_single_law_loads_and_rolls_out_the_same(tmp_path):
    """save marks the file, load gives a single law with the same arrays, modes and bits; a double
    law's file has no such key and loads as a double law."""
    law, plant, X0, kw, cl, single = _case('noisy', 2, 2)
    assert plant.n_modes > 1
    path, path64 = str(tmp_path / 'single.npz'), str(tmp_path / 'double.npz')
    single.save(path)
    cl.save(path64)
    with np.load(path) as z, np.load(path64) as z64:
        assert int(z['precision']) == 32 and z['node'].dtype == np.float32
        assert 'precision' not in z64.files and z64['node'].dtype == np.float64
        assert z['header'].shape == z64['header'].shape == (12,)
    ld, ld64 = compiled.CompiledLaw.load(path), compiled.CompiledLaw.load(path64)
    assert ld.dtype is np.float32 and ld64.dtype is np.float64
    assert np.array_equal(ld.leaf_mode, single.leaf_mode) and ld.stats['bytes'] == single.stats['bytes']
    _same_arrays(ld.arrays(), single.arrays())
    _same_arrays(ld64.arrays(), cl.arrays())
    a, b = single.rollout(X0, T, plant=plant, **kw), ld.rollout(X0, T, plant=plant, **kw)
    for f in cr.BIT_EQUAL + ('u_norm_sum', 'mode'):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    # and it is another law than the double one
    c = ld64.rollout(X0, T, plant=plant, **kw)
    assert not np.array_equal(a.u, c.u, equal_nan=True)
    for law_ in (cl, single, ld, ld64):
        law_.close()


def test_refusals():
    from explicit_hybrid_mpc_amd import explicit
    lib = _capi.load()
    # a law with a test node
    ex = explicit.ExplicitMPC(cc.two_point_tree())
    cl = ex.compile()
    assert cl.stats['n_test'] == 1
    for make in (cl.to_single, lambda: ex.compile(dtype=np.float32)):
        with pytest.raises(_capi.EhmError) as err:
            make()
        assert err.value.code == _capi.EHM_E_INVALID and REFUSAL['test nodes'] in str(err.value)
    ex.close()
    cl.close()
    # values that leave the range of a float
    law = es.SynthLaw(es.kuhn_forest(2, 100), 3, 1, np.random.default_rng(5))
    good = cc.compile_flat(law.flat)[0]

    def variant(name, row, col, value):
        out = {k: np.array(v, copy=True) for k, v in good.items()}
        out[name][row, col] = value
        return out

    for word, bad in ((REFUSAL['overflow'], variant('node', 3, 1, 1e39)),
                      (REFUSAL['overflow'], variant('leaf_rec', 0, 4, -3.5e38)),
                      (REFUSAL['underflow'], variant('leaf_rec', 5, 0, 1e-46)),
                      (REFUSAL['underflow'], variant('node', 1, 2, -1e-40)),
                      (REFUSAL['zero normal'], variant('node', 2, slice(0, 2), 1e-50))):
        with pytest.raises(c32.NarrowError):
            c32.narrow(bad)
        cl = compiled.CompiledLaw.from_arrays(bad)
        with pytest.raises(_capi.EhmError) as err:
            cl.to_single()
        assert err.value.code == _capi.EHM_E_INVALID and word in str(err.value), word
        cl.close()
    # the edge below FLT_MIN that rounds to a normal float narrows, as in the mirror
    edge = variant('leaf_rec', 5, 0, float(np.nextafter(np.float64(2. ** -126), 0.)))
    cl = compiled.CompiledLaw.from_arrays(edge)
    single = cl.to_single()
    _same_arrays(single.arrays(), c32.narrow(edge))
    # a handle's arrays leave through the export of its own precision only; a single law is not
    # narrowed again
    out = np.zeros(int(good['header'][5]), dtype=np.int32)
    assert lib.ehm_compiled_export(single._handle, None, None, out.ctypes.data, None, None, None,
                                   None) == _capi.EHM_E_INVALID
    assert lib.ehm_compiled_export_single(cl._handle, None, None, out.ctypes.data, None, None,
                                     None) == _capi.EHM_E_INVALID
    assert (out == 0).all()
    with pytest.raises(_capi.EhmError):
        single.to_single()
    # malformed float arrays are refused before anything reaches the device
    bad = c32.narrow(good)
    bad['node'].view(np.int32)[0, 3] = int(good['header'][4])
    with pytest.raises(_capi.EhmError) as err:
        compiled.CompiledLaw.from_arrays(bad)
    assert err.value.code == _capi.EHM_E_INVALID
    cl.close()
    single.close()


@pytest.fixture(scope='module')
def cwh():
    """cwh_z job 1 (abs_frac 0.5, rel_err 2; 154 nodes): its oracle, its law in both precisions."""
    from explicit_hybrid_mpc_amd import examples, explicit
    from oracle import geometry
    full_set, _, oracle = examples.example('cwh_z', abs_frac=0.5, rel_err=2.0)
    roots, _ = geometry.delaunay_simplices(full_set)
    flat = oracle.gpu.partition(np.array(roots), action='ecc')
    ex = explicit.ExplicitMPC(flat, oracle)
    cl = ex.compile()
    ex.close()
    out = types.SimpleNamespace(oracle=oracle, flat=flat, cl=cl, single=cl.to_single())
    yield out
    out.cl.close()
    out.single.close()
    oracle.close()


def test_real_partition_under_simulate_compare(cwh):
    """The reference's first job: the single law rolls out bit-equal to its mirror under
    ``simulate.compare``; at step 0 -- the same state for both laws -- it is in the double law's
    leaf for at least three quarters of the states, with inputs within u_bound there."""
    from explicit_hybrid_mpc_amd import examples, explicit
    assert cwh.flat.n_nodes == 154 and cwh.single.stats['n_test'] == 0
    assert cwh.single.mpc is cwh.oracle.mpc
    assert np.array_equal(cwh.single.leaf_mode, cwh.cl.leaf_mode)
    half = examples.theta_box(cwh.oracle.mpc)
    X0 = np.random.default_rng(3).uniform(-0.5, 0.5, (32, half.size)) * half
    n_steps = 6
    im = explicit.ImplicitMPC(cwh.oracle)
    a = simulate.compare(cwh.single, im, X0, n_steps, record=True)
    b = simulate.compare(cwh.cl, im, X0, n_steps, record=True)
    arrays = cwh.single.arrays()
    mir = c32.mirror32(arrays, cwh.single.leaf_mode, cwh.single._rollout_plant, X0, n_steps)
    cr.assert_same(a['explicit'], mir)
    assert a['n'] == b['n'] == 32 and a['stopped_implicit'] == b['stopped_implicit']
    assert (a['explicit'].steps > 0).any()
    ra, rb = a['explicit'], b['explicit']
    on = np.nonzero((ra.steps > 0) & (rb.steps > 0) & (ra.leaf[0] == rb.leaf[0]))[0]
    assert 4 * on.size >= 3 * int(((ra.steps > 0) | (rb.steps > 0)).sum()) > 0
    a64 = cwh.cl.arrays()
    l = np.searchsorted(a64['leaf_node'], rb.leaf[0, on])
    assert (np.abs(ra.u[0, on] - rb.u[0, on]) <= c32.u_bound(a64, l, X0[on])).all()
