"""
The refinement of a compiled law on the device (CompiledLaw.refine, csrc/ehm_refine.hip, DESIGN.md
3.8n): every array against the numpy mirror (tests/refine_cpu.py) bit for bit, the same function at
every state, the cells against the partition engine's own split, the selection and the criteria,
the round trip through ``reduce``, the edges of what it accepts, and the analyses of 3.8h to 3.8m
on a refined law.  (p, n_u) = (1, 1), (2, 1), (3, 2), (7, 2), (8, 1): the 1 x 1 solve, both record
sizes of each precision and the register extreme; forests of 4 roots and about 260 leaves.
"""

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import compiled_cpu as cc
from tests import core_cpu as kc
from tests import cost_cpu as co
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reach_cpu as rh
from tests import reduce_cpu as rc
from tests import refine_cpu as fc
from tests.test_host_invariance import cube_cases
from tests.test_host_refine import shifted_chain

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (3, 2), (7, 2), (8, 1)]
N_ROOTS, N_SPLIT = 4, 256


def _same(got, want, what=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _compile(flat):
    ex = rc.explicit_of(flat)
    law = ex.compile()
    ex.close()
    return law


def _law(p, n_u, seed, kind='clip', n_roots=N_ROOTS, n_split=N_SPLIT, max_depth=12):
    """(law, flat, (K, centre, width)): a Kuhn tree with the inputs clip(K x) (``kind`` 'affine':
    K x + c, integer gains on dyadic vertices; 'curved': no two leaves apply one map) and two
    leaf modes."""
    rng = np.random.default_rng([95, p, n_u, seed])
    K, c = rc.integer_gain(p, n_u, rng)
    frame = rc.kink_frame(p, n_roots, K)
    inputs = {'clip': rc.clipped_inputs(K, *frame), 'affine': rc.affine_inputs(K, c),
              'curved': rc.curved_inputs(p, n_u, 1e-3)}[kind]
    modes = lambda X: (X @ K[0] > np.median(X @ K[0])).astype(np.int32)
    flat = rc.kuhn_tree(p, n_roots, n_split, rng, inputs, n_u, modes, max_depth=max_depth)
    return _compile(flat), flat, (K,) + frame


def _forms(law, tmp_path):
    """(name, law) of the double law, its single form and both after save / load."""
    from explicit_hybrid_mpc_amd import compiled
    single = law.to_single(flush=True)
    out = [('double', law), ('single', single)]
    for name, l in list(out):
        path = str(tmp_path / (name + '.npz'))
        l.save(path)
        out.append((name + '-loaded', compiled.CompiledLaw.load(path)))
    return out


def _check(law, **kw):
    """``law.refine(return_map=True, **kw)`` against the mirror on the law's own exported arrays:
    every array, ``origin``, ``stop``, the leaf modes, the counters and the residual, bit for bit."""
    arrays = law.arrays()
    fine, origin, stop = law.refine(return_map=True, **kw)
    want = fc.refine(arrays, leaf_mode=law.leaf_mode, **kw)
    got = fine.arrays()
    assert sorted(got) == sorted(want.arrays)
    for k in sorted(got):
        _same(got[k], np.asarray(want.arrays[k]).reshape(got[k].shape), k)
    _same(origin, want.origin, 'origin')
    _same(stop, want.stop, 'stop')
    if law.leaf_mode is None:
        assert fine.leaf_mode is None
    else:
        _same(fine.leaf_mode, want.leaf_mode, 'leaf_mode')
    h0, h1 = zc.header(arrays), zc.header(got)
    r = fine.refinement
    assert (r['n_leaf_before'], r['n_leaf_after'], r['n_int_before'], r['n_int_after']) == \
        (h0['n_leaf'], h1['n_leaf'], h0['n_int'], h1['n_int'])
    assert r['bytes_before'] == law.stats['bytes'] and r['bytes_after'] == fine.stats['bytes']
    assert (r['passes'], r['n_split'], r['stops']) == (want.passes, want.n_split, want.stops)
    assert r['max_plane_residual'] == want.max_plane_residual
    assert r['seconds'] > 0. and r['plan_seconds'] > 0.
    assert fine.dtype is law.dtype and fine.mpc is law.mpc and fine.flushed == law.flushed
    assert fine.reduction is None and fine._handle.value != law._handle.value
    return fine, origin, stop, want, arrays


@pytest.mark.parametrize('p,n_u', SHAPES)
def test_every_array_is_the_mirrors(p, n_u, tmp_path):
    law, flat, _ = _law(p, n_u, 0)
    assert law.stats['n_leaf'] == N_ROOTS + N_SPLIT
    first = {}
    for name, form in _forms(law, tmp_path):
        for levels in (1, 3):
            key = (name.split('-')[0], levels)
            if name.endswith('loaded'):
                # the loaded law has the arrays of the one it was saved from, so the mirror's answer
                # is the one already checked: the refined laws agree in every array and output
                fine, origin, stop = form.refine(levels=levels, return_map=True)
                for k, a in first[key][0].items():
                    _same(fine.arrays()[k], a, k)
                _same(origin, first[key][1], 'origin')
                _same(stop, first[key][2], 'stop')
                _same(fine.leaf_mode, first[key][3], 'leaf_mode')
                assert fine.refinement['max_plane_residual'] == first[key][4]
                fine.close()
                continue
            fine, origin, stop, want, arrays = _check(form, levels=levels)
            n = zc.header(arrays)['n_leaf']
            if name == 'double':
                assert fine.stats['n_leaf'] == n << levels and (stop == fc.SATISFIED).all()
            else:
                # a float plane of a deep sliver may not separate: those leaves are kept and named
                assert fine.stats['n_leaf'] >= 0.9 * (n << levels)
                assert set(np.unique(stop)) <= {fc.SATISFIED, fc.NO_CELL, fc.UNSEPARATED}
            first[key] = (fine.arrays(), origin, stop, fine.leaf_mode,
                          fine.refinement['max_plane_residual'])
            print(p, n_u, name, levels, fine.refinement)
            fine.close()
        if form is not law:
            form.close()
    law.close()


@pytest.mark.parametrize('p,n_u', SHAPES)
def test_the_refined_law_is_the_same_function(p, n_u):
    law, flat, _ = _law(p, n_u, 1)
    rng = np.random.default_rng([96, p, n_u])
    plant = es.random_plant(rng, p, n_u, 2, 'inf', n_d=2, n_g=0)
    model = es.random_noise(rng, p, n_u, 2)
    for form in (law, law.to_single(flush=True)):
        fine, origin, stop = form.refine(levels=2, return_map=True)
        fcells = fine.cells()
        W = fcells.vertices[fcells.status == zc.CELL]
        live = np.nonzero(fcells.status == zc.CELL)[0]
        r = rng.integers(0, W.shape[0], 1024)
        w = 0.02 + (1. - 0.02 * (p + 1)) * rng.dirichlet(np.ones(p + 1), 1024)
        inside = np.einsum('nv,nvc->nc', w, W[r])           # strictly inside refined cells
        i, j = rng.integers(0, p + 1, 1024), rng.integers(0, p + 1, 1024)
        # vertices of refined cells and midpoints of their edges: they lie on the new faces
        X = np.concatenate([inside, W[r[:512], i[:512]], (W[r, i] + W[r, j]) / 2.,
                            rng.uniform(-1.5, 1.5, (4096 - 2560, p))])
        assert X.shape == (4096, p)
        u0, leaf0, depth0, _ = form.evaluate(X, return_info=True)
        u1, leaf1, depth1, _ = fine.evaluate(X, return_info=True)
        _same(u1, u0, 'u')
        _same(leaf1, leaf0, 'leaf_node')
        assert (depth1 >= depth0).all() and (depth1 > depth0).any()
        # origin[leaf'] == leaf: the refined leaf that holds an inside point comes from the leaf the
        # source law evaluates the point in (a float walk may turn to the sibling where a plane
        # value is within its rounding: those few states are left out)
        rows1 = live[r]
        sure = leaf1[:1024] == fine.leaf_node[rows1]
        assert sure.all() if form is law else sure.mean() >= 0.98
        assert np.array_equal(form.leaf_node[origin[rows1]][sure], leaf0[:1024][sure])
        assert np.array_equal(fine.leaf_node, form.leaf_node[origin])
        # the closed loop, nominal and noisy
        X0 = inside[:64]
        d = rng.uniform(-1., 1., (20, 64, 2))
        for kw in (dict(d=d), dict(noise=model, seed=7)):
            a = form.rollout(X0, 20, plant=plant, **kw)
            b = fine.rollout(X0, 20, plant=plant, **kw)
            for k in ('x', 'u', 'leaf', 'status', 'steps', 'x_final', 'mode'):
                _same(getattr(b, k), getattr(a, k), k)
        fine.close()
        if form is not law:
            form.close()
    law.close()


@pytest.mark.parametrize('p,n_u', SHAPES)
def test_the_cells_are_the_partition_engines(p, n_u):
    from explicit_hybrid_mpc_amd import engine
    law, flat, _ = _law(p, n_u, 2)
    n = law.stats['n_leaf']
    rng = np.random.default_rng([97, p])
    pick = np.sort(rng.choice(n, n // 2, replace=False))
    levels = 2
    fine, origin, stop = law.refine(levels=levels, leaves=pick, return_map=True)
    V0, V1 = law.cells(), fine.cells()
    assert (V0.status == zc.CELL).all() and (V1.status == zc.CELL).all()
    # the recursive split_batch of the source cells, numbered as the refined law numbers them
    cells, src = V0.vertices[pick], pick
    want = np.array(V0.vertices, copy=True)
    ids = pick
    for _ in range(levels):
        S1, S2, ij = engine.split_batch(cells, device=law.device)
        assert (ij[:, 0] < ij[:, 1]).all()
        twins = want.shape[0] + np.arange(ids.size)
        want = np.concatenate([want, S2])
        want[ids] = S1
        order = np.argsort(np.concatenate([ids, twins]), kind='stable')
        ids = np.concatenate([ids, twins])[order]
        cells = np.concatenate([S1, S2])[order]
    _same(V1.vertices, want, 'cells')
    assert (np.bincount(origin, minlength=n)[pick] == 1 << levels).all()
    # the children tile their parent: volumes within the tolerance of the tiling tests
    vol0 = engine.volume_batch(V0.vertices, device=law.device)
    vol1 = engine.volume_batch(V1.vertices, device=law.device)
    total = np.bincount(origin, weights=vol1, minlength=n)
    assert (np.abs(total - vol0) <= 1e-12 * vol0).all()
    # untouched leaves keep their index and their bytes
    rest = np.setdiff1d(np.arange(n), pick)
    a0, a1 = law.arrays(), fine.arrays()
    assert (stop[rest] == fc.UNSELECTED).all() and np.array_equal(origin[:n], np.arange(n))
    _same(a1['leaf_rec'][rest], a0['leaf_rec'][rest])
    _same(V1.vertices[rest], V0.vertices[rest])
    _same(V1.inputs[rest], V0.inputs[rest])
    _same(a1['leaf_rec'], a0['leaf_rec'][origin])
    _same(fine.leaf_mode, law.leaf_mode[origin])
    fine.close()
    law.close()


@pytest.mark.parametrize('p,n_u', SHAPES)
def test_selection_and_criteria(p, n_u):
    law, flat, (K, centre, width) = _law(p, n_u, 3)
    n = law.stats['n_leaf']
    rng = np.random.default_rng([98, p])
    mask = rng.random(n) < 0.3
    lv = rng.integers(0, 3, n)
    for kw in (dict(leaves=mask), dict(leaves=np.nonzero(mask)[0][::-1].copy()),
               dict(levels=lv), dict(levels=lv, leaves=mask)):
        fine, origin, stop, want, _ = _check(law, **kw)
        sel = kw.get('leaves', np.ones(n, dtype=bool))
        sel = sel if sel.dtype == np.bool_ else mask
        grown = np.where(sel, 1 << np.broadcast_to(kw.get('levels', 1), (n,)), 1)
        assert np.array_equal(np.bincount(origin), grown)
        assert np.array_equal(stop[:n] == fc.UNSELECTED, ~sel)
        fine.close()
    # max_diameter: satisfied leaves are at or below the bound, `levels` leaves above it
    d0 = fc.longest_edge(law.cells().vertices)[2]
    bound = float(np.median(d0)) * 0.6
    fine, origin, stop, want, _ = _check(law, levels=2, max_diameter=bound)
    d1 = fc.longest_edge(fine.cells().vertices)[2]
    assert set(np.unique(stop)) == {fc.SATISFIED, fc.LEVELS}
    assert (d1[stop == fc.SATISFIED] <= bound).all() and (d1[stop == fc.LEVELS] > bound).all()
    assert (np.bincount(origin)[d0 <= bound] == 1).all()
    fine.close()
    # max_spread on clip(K x): leaves away from the kink are flat beyond the first criterion
    U0 = law.cells().inputs
    spread0 = U0.max(axis=1) - U0.min(axis=1)
    crit = 0.5 * spread0.max(axis=0)
    fine, origin, stop, want, _ = _check(law, levels=3, max_spread=crit)
    over = (spread0 > crit).any(axis=1)
    assert over.any() and (~over).any()
    assert (np.bincount(origin)[~over] == 1).all() and (np.bincount(origin)[over] > 1).all()
    U1 = fine.cells().inputs
    spread1 = U1.max(axis=1) - U1.min(axis=1)
    assert ((spread1 <= crit).all(axis=1) == (stop == fc.SATISFIED)).all()
    assert set(np.unique(stop)) <= {fc.SATISFIED, fc.LEVELS}
    flat0 = rc.straddles_kink(K, centre, width, law.cells().vertices)
    assert (np.bincount(origin)[(spread0 == 0.).all(axis=1) & ~flat0] == 1).all()
    fine.close()
    law.close()


def test_a_nan_input_never_splits():
    from explicit_hybrid_mpc_amd import compiled
    law = compiled.CompiledLaw.from_arrays(fc.nan_law())
    u = law.cells().inputs[0, :, 0]
    assert u[0] == 0. and np.isposinf(u[1]) and np.isnan(u[2])
    fine, origin, stop, want, _ = _check(law, levels=3, max_spread=0.)
    assert fine.stats['n_leaf'] == 1 and stop.tolist() == [fc.SATISFIED]
    assert fine.refinement['passes'] == 0
    fine.close()
    fine, origin, stop, want, _ = _check(law, levels=1, max_spread=0., max_diameter=1.)
    assert stop.tolist() == [fc.LEVELS, fc.LEVELS]
    fine.close()
    law.close()


@pytest.mark.parametrize('p,n_u', [(2, 1), (3, 2), (7, 2)])
def test_reduce_undoes_refine(p, n_u):
    # every leaf applies its own map: reduce(0.) merges nothing of the law, all of the refinement
    law, flat, _ = _law(p, n_u, 4, kind='curved')
    for form in (law, law.to_single(flush=True)):
        keep = form.reduce(0.)
        assert keep.stats['n_leaf'] == form.stats['n_leaf']
        fine = form.refine(levels=2)
        assert fine.stats['n_leaf'] == 4 * form.stats['n_leaf'] or form is not law
        back = fine.reduce(0.)
        a, b = form.arrays(), back.arrays()
        # n_source_nodes of a refined law is raised to its leaf count where it was below it (what
        # an import asks of a header), and reduce keeps the header it is given: every other entry
        # of the header and all seven arrays are the law's, bit for bit
        src = cc.HEADER.index('n_source_nodes')
        assert b['header'][src] == max(a['header'][src], fine.stats['n_leaf'])
        b['header'][src] = a['header'][src]
        for k in a:
            _same(b[k], a[k], k)
        _same(back.leaf_mode, form.leaf_mode)
        for l in (keep, fine, back):
            l.close()
        if form is not law:
            form.close()
    law.close()
    # integer gains on dyadic vertices: refine(2).reduce(0.) is reduce(0.), array for array
    law, flat, _ = _law(p, n_u, 5, kind='affine')
    fine = law.refine(levels=2)
    a, b = law.reduce(0.), fine.reduce(0.)
    assert a.stats['n_leaf'] < law.stats['n_leaf']            # one map per leaf mode and root
    aa, bb = a.arrays(), b.arrays()
    bb['header'][cc.HEADER.index('n_source_nodes')] = aa['header'][cc.HEADER.index('n_source_nodes')]
    for k in aa:
        _same(bb[k], aa[k], k)
    for l in (a, b, fine, law):
        l.close()


def test_edges_of_the_tree():
    from explicit_hybrid_mpc_amd import _capi, compiled, explicit
    # a one-leaf law becomes one plane and two leaves
    rng = np.random.default_rng(99)
    one = _compile(rc.kuhn_tree(3, 1, 0, rng, rc.affine_inputs(*rc.integer_gain(3, 2, rng)), 2))
    assert one.stats['n_plane'] == 0 and one.arrays()['root_entry'][0] == -1
    fine, origin, stop, want, _ = _check(one, levels=1)
    got = fine.arrays()
    assert fine.stats['n_plane'] == 1 and fine.stats['n_leaf'] == 2 and got['root_entry'][0] == 0
    assert zc.children(got).tolist() == [[-1, -2]] and origin.tolist() == [0, 0]
    fine.close()
    # levels = 0: an equal copy with a different handle
    same, origin, stop, want, a0 = _check(one, levels=0)
    assert same.refinement['passes'] == 0 and stop.tolist() == [fc.SATISFIED]
    for k, a in same.arrays().items():
        _same(a, a0[k], k)
    same.close()
    # max_leaves: refused with the count, nothing returned
    with pytest.raises(_capi.EhmError) as err:
        one.refine(levels=5, max_leaves=31)
    assert err.value.code == _capi.EHM_E_INVALID and '32' in str(err.value)
    lib = _capi.load()
    roots = zc.root_vertices(a0)
    out = _capi.ctypes.c_void_p()
    counts, stats, lv = np.zeros(12, np.int64), np.zeros(3), np.full(1, 5, np.int32)

    def call(levels=lv, diameter=None, spread=None, max_leaves=1 << 24, handle=one._handle):
        return lib.ehm_compiled_refine(
            handle, roots.ctypes.data, levels.ctypes.data, None,
            None if diameter is None else diameter.ctypes.data,
            None if spread is None else spread.ctypes.data, None, max_leaves, 0,
            _capi.ctypes.byref(out), None, None, None, counts.ctypes.data, stats.ctypes.data)

    assert call(max_leaves=31) == _capi.EHM_E_INVALID and not out.value
    assert b'32 leaves' in lib.ehm_refine_last_error()
    for bad in (np.full(1, -1, np.int32), np.full(1, 17, np.int32)):
        assert call(levels=bad) == _capi.EHM_E_INVALID and b'levels[0]' in lib.ehm_refine_last_error()
    for bad in (-1., np.nan, np.inf):
        assert call(diameter=np.full(1, bad)) == _capi.EHM_E_INVALID and not out.value
        assert call(spread=np.array([0., bad])) == _capi.EHM_E_INVALID
        assert b'max_spread[1]' in lib.ehm_refine_last_error()
    assert call(handle=None) == _capi.EHM_E_INVALID
    for kw in (dict(levels=-1), dict(levels=17), dict(leaves=[1]), dict(leaves=np.ones(2, bool)),
               dict(max_diameter=-1.), dict(max_spread=np.nan)):
        with pytest.raises(_capi.EhmError) as err:
            one.refine(**kw)
        assert err.value.code == _capi.EHM_E_INVALID
    one.leaf_mode = np.zeros(3, np.int32)                  # of the wrong length
    with pytest.raises(_capi.EhmError):
        one.refine()
    one.leaf_mode = None
    one.close()
    with pytest.raises(_capi.EhmError) as err:
        one.refine()
    assert err.value.code == _capi.EHM_E_INVALID and 'closed' in str(err.value)
    # a law with test nodes is refused
    ex = explicit.ExplicitMPC(cc.two_point_tree())
    tests = ex.compile()
    ex.close()
    assert tests.stats['n_test'] > 0
    with pytest.raises(_capi.EhmError) as err:
        tests.refine()
    assert err.value.code == _capi.EHM_E_INVALID and 'test nodes' in str(err.value)
    r1 = np.zeros((1, 2, 1))
    assert lib.ehm_compiled_refine(
        tests._handle, r1.ctypes.data, lv.ctypes.data, None, None, None, None, 1 << 24, 0,
        _capi.ctypes.byref(out), None, None, None, counts.ctypes.data,
        stats.ctypes.data) == _capi.EHM_E_INVALID
    assert b'test nodes' in lib.ehm_refine_last_error()
    tests.close()


@pytest.mark.parametrize('n_leaf', [1023, 1024, 1025])
def test_the_tile_boundary_of_the_scan(n_leaf):
    law, flat, _ = _law(2, 1, n_leaf, n_split=n_leaf - N_ROOTS, max_depth=16)
    assert law.stats['n_leaf'] == n_leaf
    fine, origin, stop, want, _ = _check(law, levels=1)
    assert fine.stats['n_leaf'] == 2 * n_leaf and np.array_equal(origin[n_leaf:], np.arange(n_leaf))
    fine.close()
    # every other leaf: the offsets of the appended records cross the tile too
    fine, origin, stop, want, _ = _check(law, levels=1, leaves=np.arange(1, n_leaf, 2))
    assert np.array_equal(origin[n_leaf:], np.arange(1, n_leaf, 2))
    fine.close()
    law.close()


def test_a_law_with_a_locator_keeps_it():
    law, flat, _ = _law(2, 1, 6, n_roots=None, n_split=200)
    a0 = law.arrays()
    assert zc.header(a0)['n_roots'] >= 128 and zc.header(a0)['has_nbr'] == 1
    fine, origin, stop, want, _ = _check(law, levels=1)
    a1 = fine.arrays()
    _same(a1['nbr'], a0['nbr'])
    _same(a1['root_rec'], a0['root_rec'])
    rng = np.random.default_rng(6)
    X = rng.uniform(-1.1, 1.1, (4096, 2))
    u0, leaf0, depth0, _ = law.evaluate(X, return_info=True)
    u1, leaf1, depth1, _ = fine.evaluate(X, return_info=True)
    _same(u1, u0)
    _same(leaf1, leaf0)
    assert set(np.unique(depth1 - depth0)) <= {0, 1}
    fine.close()
    law.close()


def test_leaves_that_are_kept_whole():
    from explicit_hybrid_mpc_amd import compiled
    # a broken plane: the leaves below it have no cell and are kept
    law, flat, _ = _law(3, 2, 7, n_split=60)
    arrays = law.arrays()
    below = rc.leaves_below(arrays)
    bad = next(k for k in range(len(below)) if 3 <= len(below[k]) <= 12)
    arrays['node'][bad, :4] *= 0.25
    broken = compiled.CompiledLaw.from_arrays(arrays)
    fine, origin, stop, want, _ = _check(broken, levels=2)
    assert (stop[below[bad]] == fc.NO_CELL).all() and fine.refinement['stops']['no_cell'] == len(below[bad])
    assert (np.bincount(origin)[below[bad]] == 1).all()
    assert fine.stats['n_leaf'] == 4 * (law.stats['n_leaf'] - len(below[bad])) + len(below[bad])
    for l in (fine, broken, law):
        l.close()
    # a chain of 300 levels: too_deep at depth 256, no_cell below it, the shallower leaves split
    deep = _compile(zc.chain_tree(2, 300))
    fine, origin, stop, want, _ = _check(deep, levels=1)
    depth = np.minimum(np.arange(301) + 1, 300)
    assert np.array_equal(np.nonzero(stop == fc.TOO_DEEP)[0], np.nonzero(depth == 256)[0])
    assert (stop[:301][depth > 256] == fc.NO_CELL).all()
    assert np.array_equal(np.bincount(origin), np.where(depth < 256, 2, 1))
    assert (fine.cells().status == zc.CELL).sum() == 2 * 255 + 1
    fine.close()
    deep.close()
    # a sliver chain in single precision: where the float plane no longer separates the leaf stays
    double = _compile(shifted_chain(2, 30, [1. / 3., 0.7], 0.9))
    single = double.to_single(flush=True)
    fine64, _, stop64, _, _ = _check(double, levels=1)
    fine32, origin, stop32, want, _ = _check(single, levels=1)
    assert (stop64 == fc.SATISFIED).all() and fine64.stats['n_leaf'] == 62
    kept = np.nonzero(stop32 == fc.UNSEPARATED)[0]
    assert kept.size >= 1 and (np.bincount(origin)[kept] == 1).all()
    assert (fine32.cells().status[stop32 == fc.SATISFIED] == zc.CELL).all()
    for l in (fine64, fine32, single, double):
        l.close()


@pytest.mark.parametrize('p', [2, 3])
def test_the_analyses_on_a_refined_law(p):
    """The contraction cube laws that keep a core, refined one level: the one-step test, the core,
    the reach tube and the fuel bounds against their mirrors (which read arrays), and 2 000
    rollouts of 30 steps from inside refined core leaves against the refined law's bounds."""
    from tests.test_gpu_core import _against_mirror as core_against, _inside
    from tests.test_gpu_cost import _against_mirror as cost_against, _norms
    from tests.test_gpu_invariance import _against_mirror as succ_against
    from tests.test_gpu_reach import _against_mirror as reach_against, _cells_of
    T = 30
    for name, K, E, d_box, _, _ in cube_cases(p):
        if name not in ('contraction', 'contraction_quarter_box'):
            continue
        rng = np.random.default_rng([62, p, len(name)])
        coarse = _compile(iv.cube_law(p, K))
        law, origin, stop = coarse.refine(levels=1, return_map=True)
        assert law.stats['n_leaf'] == 2 * coarse.stats['n_leaf'] and (stop == fc.SATISFIED).all()
        plant = iv.identity_plant(p, E=E)
        arrays = law.arrays()
        succ = law.successors(plant=plant, d_box=d_box, tol_exit=0., return_successors=True)
        succ_against(succ, iv.successors(arrays, None, plant, d_box=d_box, tol_exit=0.))
        core = law.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0.,
                                  return_edges=True)
        core_against(core, kc.core(arrays, None, plant, d_box=d_box, tol_exit=0., tol_side=0.), name)
        assert core.core.all() and core.set_convex and core.holds
        V = _cells_of(arrays)
        reach = law.reach(core, horizon=6, return_steps=True)
        reach_against(reach, rh.reach(core.indptr, core.indices, core.level, core.core, V=V,
                                      horizon=6), name)
        w_hi, w_lo, pad = co.weights(arrays)
        cost = law.cost(core, horizon=T, return_paths=True)
        cost_against(cost, co.bounds(core.indptr, core.indices, core.core, w_hi, w_lo, T), name)
        # the refined cells are smaller: no bound of a leaf is looser than its source leaf's
        coarse_core = coarse.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0.,
                                            return_edges=True)
        coarse_cost = coarse.cost(coarse_core, horizon=T)
        print(p, name, 'coarse', coarse_cost, 'refined', cost)
        # rollouts from inside refined core leaves: the row of the first leaf is the cell's
        rows = np.nonzero(core.core)[0]
        k = -(-2000 // rows.size)
        X0 = _inside(rng, V[rows], k, floor=1e-3)[:2000]
        row0 = np.repeat(rows, k)[:2000]
        d = None
        if d_box is not None:
            d = rng.uniform(d_box[0], d_box[1], (T, X0.shape[0], plant.n_d))
        run = law.rollout(X0, T, d=d, plant=plant, record=True)
        assert (run.status == 0).all() and (run.steps == T).all()
        assert np.array_equal(run.leaf[0], law.leaf_node[row0])
        same = coarse.rollout(X0, T, d=d, plant=plant, record=True)
        _same(run.x, same.x)
        _same(run.u, same.u)
        nrm = _norms(run.u)
        total = np.zeros(nrm.shape[1])
        last = None
        for h in range(1, T + 1):
            res = core.cost(horizon=h)
            assert res.holds
            total = total + nrm[h - 1]
            s = (h + 1) * 2. ** -52
            assert (total <= res.hi[row0] * (1. + s)).all(), (name, h)
            assert (total >= res.lo[row0] * (1. - s)).all(), (name, h)
            last = res
        assert np.array_equal(total, run.u_norm_sum)
        for span in range(1, T + 1):
            s = (span + 1) * 2. ** -52
            for t in range(T - span + 1):
                window = np.zeros(nrm.shape[1])
                for j in range(t, t + span):
                    window = window + nrm[j]
                assert (window <= span * last.rate_hi[span] * (1. + s)).all(), (name, span, t)
                assert (window >= span * last.rate_lo[span] * (1. - s)).all(), (name, span, t)
        # a state does not name its leaf record in a refined law
        with pytest.raises(ValueError, match='refined'):
            core.contains(X0)
        law.close()
        coarse.close()
