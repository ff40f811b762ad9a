"""
The one-step successors of a compiled law's leaves on the device (csrc/ehm_invariance.hip,
invariance.py): bit for bit against the numpy mirror (tests/invariance_cpu.py), the
exact cube cases of tests/test_host_invariance.py, agreement with ``CompiledLaw.rollout``, the
``mode_region`` status against dyadic vertices, and the refusals of the C entry point.
"""

import ctypes

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests.test_host_invariance import cube_cases, cube_exits, exact_margins

pytestmark = pytest.mark.gpu

PER_LEAF = ('status', 'margin', 'worst', 'max_violation', 'x_next', 'succ_root', 'succ_leaf')


def _same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _against_mirror(res, mir):
    from explicit_hybrid_mpc_amd import invariance
    for k in PER_LEAF:
        _same(getattr(res, k), getattr(mir, k), k)
    assert res.counts == dict(zip(invariance.STATUS_NAMES, mir.counts))
    if mir.worst_leaf < 0:
        assert res.worst_leaf is None and np.isnan(res.worst_margin)
    else:
        assert res.worst_leaf['leaf'] == res.leaves[mir.worst_leaf]
        assert res.worst_margin == mir.worst_margin == res.worst_leaf['margin']
    assert res.n_corners == mir.n_corners


def _same_result(a, b):
    for k in PER_LEAF:
        _same(getattr(a, k), getattr(b, k), k)
    assert a.counts == b.counts and a.worst_leaf == b.worst_leaf
    assert a.invariant_volume_fraction == b.invariant_volume_fraction
    assert a.cell_volume_fraction == b.cell_volume_fraction


# the law of test_gpu_certify (100 roots: the serial root rule), and the full forests of p = 2
# (128 roots) and p = 3 (384 roots), which have the adjacency table and take the visibility walk
@pytest.mark.parametrize('p,n_u,keep', [(2, 1, 100), (3, 2, 100), (7, 1, 100), (8, 4, 100),
                                        (2, 1, None), (3, 2, None)])
def test_successors_are_the_mirrors_bit_for_bit(p, n_u, keep, tmp_path):
    from explicit_hybrid_mpc_amd import compiled
    rng = np.random.default_rng([91, p, n_u, 0 if keep is None else keep])
    synth = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng, n_sub=12)
    plant = es.random_plant(rng, p, n_u, 2, 'inf' if p % 2 else 'quadratic', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    arrays = law.arrays()
    h = zc.header(arrays)
    n_leaf = h['n_leaf']
    assert n_leaf > 256 and bool(h['has_nbr']) == (keep is None)
    modes = rng.integers(-1, 2, n_leaf).astype(np.int32)
    assert (modes == -1).any() and (modes == 1).any()
    law.set_leaf_modes(modes)
    lo = rng.uniform(-1., 0., 2)
    hi = lo + rng.uniform(0.1, 1., 2)
    hi[1] = lo[1]                                           # one degenerate axis
    box = (lo, hi)
    res = law.successors(plant=plant, d_box=box, return_successors=True)
    mir = iv.successors(arrays, modes, plant, d_box=box)
    _against_mirror(res, mir)
    print(p, n_u, keep, res, 'kernel %.3g s' % res.seconds)
    assert res.n_corners == 4 and res.x_next.shape == (n_leaf, p + 1, 4, p)
    # (the 100 roots of p = 7, 8 are a sliver of the cube: nothing stays in them)
    assert min(res.counts[k] for k in ('exits', 'mode_region', 'no_mode')) > 0
    assert (res.counts['invariant'] > 0) == (p <= 3)
    assert res.counts['no_cell'] == 0 and abs(res.cell_volume_fraction - 1.) <= 1e-12
    assert not res.holds_on_set
    dead = res.status >= iv.NO_MODE
    assert np.isnan(res.margin[dead]).all() and (res.succ_root[dead] == -1).all()
    # the nominal successor: no box, no E term
    nominal = law.successors(plant=plant, return_successors=True)
    _against_mirror(nominal, iv.successors(arrays, modes, plant))
    assert nominal.n_corners == 1
    bare = law.successors(plant=plant, d_box=box)
    assert bare.x_next is None and bare.counts == res.counts
    _same(bare.margin, res.margin)
    # a subset in the caller's order with a leaf named twice: the rows of the full call
    pick = np.concatenate([rng.permutation(n_leaf)[:77], [0, n_leaf - 1, 0]]).astype(np.int64)
    part = law.successors(plant=plant, d_box=box, leaves=pick, return_successors=True, chunk=16)
    for k in PER_LEAF:
        _same(getattr(part, k), getattr(res, k)[pick], k)
    assert part.counts == {name: int((res.status[pick] == s).sum())
                           for s, name in enumerate(res.counts)}
    assert np.array_equal(part.leaves, pick) and part.n == pick.size and not part.holds_on_set
    _against_mirror(part, iv.successors(arrays, modes, plant, leaves=pick, d_box=box))
    # no result depends on the chunk
    for chunk in (64, 1000):
        _same_result(law.successors(plant=plant, d_box=box, return_successors=True, chunk=chunk),
                     res)
    # the same law after save / load
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    _same_result(loaded.successors(plant=plant, d_box=box, return_successors=True), res)
    loaded.close()
    # its single form against the mirror in float arithmetic
    single = law.to_single(flush=True)
    a32 = single.arrays()
    s32 = single.successors(plant=plant, d_box=box, return_successors=True)
    _against_mirror(s32, iv.successors(a32, modes, plant, d_box=box))
    live = (s32.status < iv.NO_MODE) & (res.status < iv.NO_MODE)
    assert live.sum() >= 0.5 * n_leaf
    assert not np.array_equal(s32.x_next[live], res.x_next[live])
    single.close()
    law.close()


def _cube(p, K, modes=None):
    flat = iv.cube_law(p, K, modes=modes)
    ex = rc.explicit_of(flat)
    law = ex.compile()
    ex.close()
    return flat, law


@pytest.mark.parametrize('p', [2, 3])
def test_the_cube_cases_on_the_device(p):
    forest = es.kuhn_forest(p)
    for name, K, E, d_box, scale, reach in cube_cases(p):
        flat, law = _cube(p, K)
        assert law.stats['nbr_bytes'] > 0
        plant = iv.identity_plant(p, E=E)
        res = law.successors(plant=plant, d_box=d_box, tol_exit=0., return_successors=True)
        V = flat.vertices[res.leaf_node]
        want = cube_exits(name, V, scale, reach)
        assert np.array_equal(res.status, np.where(want, iv.EXITS, iv.INVARIANT)), name
        margin, worst = exact_margins(forest, res, forest.n_roots)
        _same(res.margin, margin, name)
        _same(res.worst, worst, name)
        assert res.set_convex
        assert res.holds_on_set == (not want.any())
        assert res.holds_on_set == (name != 'expansion' and name != 'contraction_box')
        if not want.any():
            assert abs(res.invariant_volume_fraction - 1.) <= 1e-12
            via = rc.explicit_of(flat)
            again = via.successors(plant=plant, d_box=d_box, tol_exit=0.)
            via.close()
            assert again.counts == res.counts and again.holds_on_set
        else:
            assert 0. < res.invariant_volume_fraction < 1.
        law.close()


def test_agreement_with_the_rollout():
    """What ``successors`` says of a leaf is what ``rollout`` does from it.  x+ is affine in
    (x, d), so its weights in a fixed root move by at most t times their spread over the cell when
    the state moves the fraction t towards the centroid; the Kuhn roots have side 1/2, the plant's
    maps norms of a few units, so that spread is a few units and 2^-20 of it stays far below the
    1e-3 asked of an exiting leaf's margin.  Every leaf's mode is one whose region holds its whole
    cell, so that the second step of an invariant leaf's trajectories is applied too."""
    p, n_u = 3, 2
    rng = np.random.default_rng([83, 0])
    synth = es.SynthLaw(es.kuhn_forest(p), n_u, 2, rng, n_sub=12, no_law=0.)
    plant = es.random_plant(rng, p, n_u, 2, 'inf', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    cells = law.cells()
    n = len(cells)
    in_one = es.in_region(plant, cells.vertices.reshape(-1, p), np.ones(n * (p + 1), dtype=int),
                          0.).reshape(n, p + 1).all(axis=1)
    law.set_leaf_modes(in_one.astype(np.int32))
    half = rng.uniform(0.5, 2., 2)
    box = (-half, half)
    res = law.successors(plant=plant, d_box=box)
    assert res.set_convex and res.counts['mode_region'] == res.counts['no_mode'] == 0
    inv = np.nonzero((res.status == iv.INVARIANT) & (res.margin >= 1e-6))[0]
    out = np.nonzero((res.status == iv.EXITS) & (res.margin <= -1e-3))[0]
    print(res, 'invariant leaves tried %d, exiting leaves tried %d' % (inv.size, out.size))
    assert inv.size >= 10 and out.size >= 10
    # invariant: 8 points in the cell with every weight >= 1e-3, disturbances drawn in the box
    w = 1e-3 + (1. - (p + 1) * 1e-3) * rng.dirichlet(np.ones(p + 1), (inv.size, 8))
    X0 = np.einsum('nkv,nvc->nkc', w, cells.vertices[inv]).reshape(-1, p)
    d = rng.uniform(-half, half, (2, X0.shape[0], 2))
    run = law.rollout(X0, 2, d=d, plant=plant)
    assert (run.status == 0).all() and (run.steps == 2).all()
    assert np.array_equal(run.leaf[0], np.repeat(res.leaf_node[inv], 8))
    # exits: from next to the worst vertex under the worst corner the first step leaves the set
    i, j = res.worst[out] // res.n_corners, res.worst[out] % res.n_corners
    v = cells.vertices[out, i]
    X0 = v + 2. ** -20 * (cells.vertices[out].mean(axis=1) - v)
    d = np.zeros((2, out.size, 2))
    d[0] = iv.corners(box, 2)[j]
    run = law.rollout(X0, 2, d=d, plant=plant)
    assert np.array_equal(run.leaf[0], res.leaf_node[out])
    assert (run.status == 1).all() and (run.steps == 1).all()
    law.close()


@pytest.mark.parametrize('face', [0., 0.125])
def test_mode_region_on_exactly_the_straddling_leaves(face):
    """Two modes whose regions split the cube at x_0 = face, leaf modes from the centroid.  The
    Kuhn grid has a plane at 0, so no cell straddles that face and every leaf next to it touches
    it from one side; 1/8 lies inside the cubes of side 1/4."""
    p = 2
    flat, law = _cube(p, -0.5 * np.eye(p), modes=lambda C: (C[:, 0] > face).astype(np.int32))
    e0 = np.eye(p)[:1]
    plant = iv.identity_plant(p, n_modes=2, regions=[(e0, np.array([face])),
                                                     (-e0, np.array([-face]))])
    res = law.successors(plant=plant, tol_exit=0.)
    x0 = flat.vertices[res.leaf_node][:, :, 0]
    straddles = (x0.min(axis=1) < face) & (x0.max(axis=1) > face)
    touches = ~straddles & (x0 == face).any(axis=1)
    if face == 0.:
        assert touches.sum() >= 10 and not straddles.any()
    else:
        assert straddles.sum() >= 10
    assert np.array_equal(res.status == iv.MODE_REGION, straddles)
    assert (res.status[~straddles] == iv.INVARIANT).all()
    assert not np.isnan(res.margin[straddles]).any()
    law.close()


def _opts(law, plant, roots, modes, **kw):
    from explicit_hybrid_mpc_amd import _capi
    rows, H, h = plant.region_arrays()
    keep = dict(A=plant.A, B=plant.B, w=plant.w, E=plant.E, rows=rows, H=H, h=h, roots=roots,
                modes=modes)
    at = lambda a: a.ctypes.data if a.size else None
    o = dict(n=2, root_vertices=at(roots), A=at(plant.A), B=at(plant.B), w=at(plant.w),
             region_rows=at(rows), H=at(H), h=at(h), leaf_mode=at(modes), tol_exit=1e-9,
             n_modes=plant.n_modes, n_d=0, n_g=0)
    o.update(kw)
    return _capi.InvarianceOpts(**o), keep


def test_the_entry_point_refuses():
    from explicit_hybrid_mpc_amd import _capi, applied, explicit, partition
    p, n_u = 2, 1
    rng = np.random.default_rng(7)
    synth = es.SynthLaw(es.kuhn_forest(p, 20), n_u, 1, rng, n_sub=3)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    plant = es.random_plant(rng, p, n_u, 1, 'inf', n_d=2)
    n_leaf = law.stats['n_leaf']
    roots = applied.root_cells(law)['vertices']
    modes = np.zeros(n_leaf, dtype=np.int32)
    lib = _capi.load()
    out = dict(status=np.empty(2, np.int32), margin=np.empty(2), worst=np.empty(2, np.int32),
               max_violation=np.empty(2))
    lv = _capi.InvarianceLeaves(**{k: a.ctypes.data for k, a in out.items()})
    res = _capi.InvarianceResult()

    def call(handle=law._handle, **kw):
        o, keep = _opts(law, plant, roots, modes, **kw)
        rc_ = lib.ehm_compiled_successors(handle, ctypes.byref(o), ctypes.byref(res),
                                          ctypes.byref(lv))
        return rc_, lib.ehm_invariance_last_error()

    assert call()[0] == _capi.EHM_OK
    want = law.successors(plant=plant, leaves=[0, 1])
    assert np.array_equal(out['status'], want.status)
    _same(out['margin'], want.margin)
    ids = np.array([0, n_leaf], dtype=np.int32)
    code, msg = call(leaf_ids=ids.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'leaf_ids[1]' in msg
    assert call(n=-1)[0] == _capi.EHM_E_INVALID
    assert call(n=n_leaf + 1)[0] == _capi.EHM_E_INVALID
    assert call(handle=None)[0] == _capi.EHM_E_INVALID
    lo9, hi9 = np.zeros(9), np.ones(9)
    E9 = np.zeros((p, 9))
    code, msg = call(n_d=9, E=E9.ctypes.data, d_lo=lo9.ctypes.data, d_hi=hi9.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'n_d = 9' in msg
    lo, hi = np.array([0., 1.]), np.array([1., 0.5])
    E = np.ascontiguousarray(plant.E)
    code, msg = call(n_d=2, E=E.ctypes.data, d_lo=lo.ctypes.data, d_hi=hi.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'axis 1' in msg
    hi[1] = np.inf
    assert call(n_d=2, E=E.ctypes.data, d_lo=lo.ctypes.data,
                d_hi=hi.ctypes.data)[0] == _capi.EHM_E_INVALID
    hi[1] = 2.
    code, msg = call(n_d=2, d_lo=lo.ctypes.data, d_hi=hi.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'no E' in msg
    assert call(n_d=2, E=E.ctypes.data, d_lo=lo.ctypes.data, d_hi=hi.ctypes.data)[0] == _capi.EHM_OK
    assert call(A=None)[0] == _capi.EHM_E_INVALID
    assert call(leaf_mode=None)[0] == _capi.EHM_E_INVALID
    assert call(tol_exit=-1e-9)[0] == _capi.EHM_E_INVALID
    assert call(tol_exit=np.nan)[0] == _capi.EHM_E_INVALID
    assert call(n_modes=5)[0] == _capi.EHM_E_INVALID
    assert call(n_g=257)[0] == _capi.EHM_E_INVALID
    with pytest.raises(ValueError):
        law.successors(plant=plant, leaves=[n_leaf])
    empty = law.successors(plant=plant, leaves=np.zeros(0, dtype=np.int32))
    assert empty.n == 0 and empty.worst_leaf is None and not empty.holds_on_set
    law.close()
    # a law with test nodes: the default compile of a nested tree
    from tests.test_gpu_audit import _oracle
    orc, Vs = _oracle('di')
    root, _ = partition.partition_set(orc, Vs)
    nested = explicit.ExplicitMPC(root, orc)
    with_tests = nested.compile()
    assert with_tests.stats['n_test'] > 0
    with pytest.raises(_capi.EhmError) as err:
        with_tests.successors()
    assert err.value.code == _capi.EHM_E_INVALID and 'test nodes' in str(err.value)
    big = np.zeros((with_tests.stats['n_roots'], 3, 2))
    many = np.zeros(with_tests.stats['n_leaf'], dtype=np.int32)
    di = es.random_plant(rng, 2, with_tests.n_u, 1, 'inf')
    o, keep = _opts(with_tests, di, big, many, n=1)
    assert lib.ehm_compiled_successors(with_tests._handle, ctypes.byref(o), ctypes.byref(res),
                                       ctypes.byref(lv)) == _capi.EHM_E_INVALID
    assert b'test nodes' in lib.ehm_invariance_last_error()
    as_roots = nested.compile(spine='roots')
    ok = as_roots.successors()
    assert sum(ok.counts.values()) == as_roots.stats['n_leaf'] and ok.counts['no_cell'] == 0
    print('di:', ok)
    for l in (with_tests, as_roots):
        l.close()
    nested.close()
    orc.close()
