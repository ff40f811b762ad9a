"""
The reduction of a compiled law on the device (CompiledLaw.reduce, csrc/ehm_reduce.hip, DESIGN.md
3.8g) against the numpy mirror (tests/reduce_cpu.py) bit for bit, against the bound it promises,
and through every path a law takes afterwards.  p = 2, 3 (the 64-byte record, 32 in single) and 7
(the 128-byte one, 64 in single), n_u = 1, 2; a double law, its ``to_single(flush=True)`` and both
after ``save`` / ``load``; trees of a few hundred leaves on ``explicit_synth``'s Kuhn forests with
prescribed vertex inputs.
"""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import explicit_synth as es
from tests import reduce_cpu as rc

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (3, 2), (7, 1), (7, 2)]
N_ROOTS, N_SPLIT = 4, 260


def _compile(flat):
    ex = rc.explicit_of(flat)
    law = ex.compile()
    ex.close()
    return law


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


def _same_bytes(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _check(law, tol, use_modes=True):
    """``law.reduce(tol, return_map=True)`` against the mirror on the law's own exported arrays:
    every array, ``leaf_of``, the leaf modes and the counters, bit for bit."""
    arrays = law.arrays()
    mode = law.leaf_mode if use_modes else None
    if not use_modes:
        law.set_leaf_modes(None)
    red, leaf_of = law.reduce(tol, return_map=True)
    want = rc.reduce(arrays, tol, mode)
    got = red.arrays()
    assert sorted(got) == sorted(want.arrays)
    for k in sorted(got):
        _same_bytes(np.asarray(got[k]), np.asarray(want.arrays[k]).reshape(got[k].shape), k)
    _same_bytes(leaf_of, want.leaf_of, 'leaf_of')
    if mode is None:
        assert red.leaf_mode is None
    else:
        _same_bytes(red.leaf_mode, want.leaf_mode, 'leaf_mode')
    h0, h1 = zc.header(arrays), zc.header(got)
    r = red.reduction
    assert (r['n_leaf_before'], r['n_leaf_after'], r['n_int_before'], r['n_int_after']) == \
        (h0['n_leaf'], h1['n_leaf'], h0['n_int'], h1['n_int'])
    assert r['bytes_before'] == law.stats['bytes'] and r['bytes_after'] == red.stats['bytes']
    assert r['max_deviation'] == want.max_deviation and r['seconds'] > 0.
    assert np.array_equal(r['tol'], np.broadcast_to(tol, (law.n_u,)))
    assert red.dtype is law.dtype and red.mpc is law.mpc and red.flushed == law.flushed
    assert red._handle.value != law._handle.value
    return red, leaf_of, want, arrays


def _dyadic_states(V, rng, n):
    """Points 3/4 v_i + 1/4 v_j of random cells: dyadic, so integer gains sum exactly."""
    q = rng.integers(0, V.shape[0], n)
    i, j = rng.integers(0, V.shape[1], n), rng.integers(0, V.shape[1], n)
    return 0.75 * V[q, i] + 0.25 * V[q, j]


@pytest.mark.parametrize('p,n_u', SHAPES)
def test_one_affine_map_becomes_one_leaf_per_root(p, n_u, tmp_path):
    rng = np.random.default_rng([92, p, n_u])
    K, c = rc.integer_gain(p, n_u, rng)
    flat = rc.kuhn_tree(p, N_ROOTS, N_SPLIT, rng, rc.affine_inputs(K, c), n_u)
    law = _compile(flat)
    assert law.stats['n_leaf'] == N_ROOTS + N_SPLIT
    X = _dyadic_states(flat.vertices[law.leaf_node], rng, 512)
    first = None
    for name, form in _forms(law, tmp_path):
        red, leaf_of, want, arrays = _check(form, 0.)
        got = red.arrays()
        assert red.stats['n_leaf'] == N_ROOTS and red.stats['n_plane'] == 0, name
        assert (got['root_entry'] < 0).all()
        assert np.array_equal(np.sort(~got['root_entry']), np.arange(N_ROOTS))
        assert red.reduction['max_deviation'] == 0.
        assert np.array_equal(got['leaf_node'][~got['root_entry']],
                              arrays['leaf_node'][want.rep[arrays['root_entry']]])
        u, leaf, depth, _ = red.evaluate(X, return_info=True)
        assert np.array_equal(u, form.evaluate(X)) and np.array_equal(u, X @ K.T + c), name
        assert (depth <= form.evaluate(X, return_info=True)[2]).all()
        if name.endswith('loaded'):
            for k, a in first[name.split('-')[0]].items():
                _same_bytes(got[k], a, k)
        else:
            first = dict(first or {}, **{name: got})
        red.close()
        if form is not law:
            form.close()
    law.close()


@pytest.mark.parametrize('p,n_u', SHAPES)
def test_clipped_map_merges_on_either_side_of_its_kinks(p, n_u, tmp_path):
    rng = np.random.default_rng([93, p, n_u])
    K, _ = rc.integer_gain(p, n_u, rng)
    centre, width = rc.kink_frame(p, N_ROOTS, K)
    flat = rc.kuhn_tree(p, N_ROOTS, N_SPLIT, rng, rc.clipped_inputs(K, centre, width), n_u)
    law = _compile(flat)
    tol = 1e-9
    synth = SimpleNamespace(p=p, u_max=float(np.abs(flat.vertex_inputs).max()))
    for name, form in _forms(law, tmp_path):
        single = name.startswith('single')
        # a single law compares float sums: its tolerance sits above their rounding, 2^-24 (p + 4)
        # times the largest |u_0| + sum |K| |d| of its records on these roots (side <= 2)
        a0 = form.arrays()
        lr = np.abs(np.asarray(a0['leaf_rec'], dtype=np.float64))
        t = 2. ** -24 * (p + 4) * 4. * float(lr[:, p:p + n_u + n_u * p].sum(axis=1).max()) \
            if single else tol
        red, leaf_of, want, arrays = _check(form, t)
        h = zc.header(arrays)
        assert red.stats['n_leaf'] < h['n_leaf'], name
        V, st = want.cells, want.cell_status
        assert (st == zc.CELL).all()
        strad = rc.straddles_kink(K, centre, width, V)
        assert strad.any()
        if not single:
            # a straddling leaf applies the interpolant of clipped values: it shares a leaf only
            # with straddling leaves (two siblings split along an edge on one side of the kink
            # apply their parent's interpolant exactly, and merge)
            for tgt in np.unique(want.target[strad]):
                assert strad[want.target == tgt].all()
            alone = np.bincount(want.target, minlength=h['n_leaf'])[strad] == 1
            assert alone.sum() >= 0.5 * strad.sum()
        # states inside original cells: the two laws differ by at most tol plus evaluation rounding
        n = 600
        q = rng.integers(0, h['n_leaf'], n)
        w = rng.dirichlet(np.ones(p + 1), n) * (1. - 0.01 * (p + 1)) + 0.01
        X = np.einsum('nv,nvc->nc', w, V[q])
        u0, leaf0, _, _ = form.evaluate(X, return_info=True)
        u1, leaf1, _, _ = red.evaluate(X, return_info=True)
        # each law hands x to the leaf that holds it (a float walk may turn to the sibling where
        # a plane value is within its rounding: those few states are left out)
        sure = (leaf0 == arrays['leaf_node'][q]) & (leaf1 == red.leaf_node[leaf_of[q]])
        assert sure.mean() >= 0.98 if single else sure.all(), name
        cell1 = V[want.target[q]]
        kappa = np.maximum(np.linalg.cond(np.transpose(V[q][:, 1:] - V[q][:, :1], (0, 2, 1))),
                           np.linalg.cond(np.transpose(cell1[:, 1:] - cell1[:, :1], (0, 2, 1))))
        lam = np.linalg.solve(
            np.concatenate([np.transpose(cell1, (0, 2, 1)), np.ones((n, 1, p + 1))], axis=1),
            np.concatenate([X, np.ones((n, 1))], axis=1)[:, :, None])[:, :, 0]
        bound = np.array([es.SynthLaw.u_tol(synth, kappa[a], np.abs(lam[a]), 1.)
                          for a in range(n)])[:, None]
        if single:
            # four float evaluations: both maps at x and, in the rule, at the cell's vertices
            a64 = dict(arrays, node=np.asarray(arrays['node'], np.float64),
                       leaf_rec=np.asarray(arrays['leaf_rec'], np.float64))
            for leaves in (q, want.target[q]):
                bound = bound + c32.u_bound(a64, leaves, X)
                bound = bound + np.max([c32.u_bound(a64, leaves, V[q][:, i])
                                        for i in range(p + 1)], axis=0)
        print(name, 'leaves %d -> %d, max |du| %.3g, tol %.3g, rounding bound up to %.3g' % (
            h['n_leaf'], red.stats['n_leaf'], np.abs(u1 - u0).max(), t, bound.max()))
        assert (np.abs(u1 - u0) <= t + bound)[sure].all(), name
        red.close()
        if form is not law:
            form.close()
    law.close()


def test_the_bound_does_not_accumulate_over_levels():
    """Neighbouring leaves of a slowly curving input differ by about 0.6 tol: every original leaf
    stays within tol of the leaf that stands for it, and a sibling pair that agrees neighbour to
    neighbour stays apart where a deeper leaf fails against the record's representative."""
    p, n_u = 3, 2
    rng = np.random.default_rng([94])
    flat = rc.kuhn_tree(p, N_ROOTS, N_SPLIT, rng, rc.curved_inputs(p, n_u, 1e-3), n_u)
    law = _compile(flat)
    cells = law.cells()
    arrays = law.arrays()
    ch = zc.children(arrays)
    both = ch[(ch < 0).all(axis=1)]
    d = np.abs(rc.map_at(arrays, ~both[:, 0], cells.vertices[~both[:, 1]]) -
               cells.inputs[~both[:, 1]])
    tol = np.median(d.max(axis=1), axis=0) / 0.6                    # [n_u]
    red, leaf_of, want, _ = _check(law, tol)
    assert 1 < red.stats['n_leaf'] < law.stats['n_leaf']
    got = red.arrays()
    Unew = rc.map_at(got, leaf_of, cells.vertices)
    assert (np.abs(Unew - cells.inputs) <= tol).all()
    assert 0. < red.reduction['max_deviation'] <= tol.max()
    looks = 0
    for a in np.nonzero(want.open)[0]:
        l, r = (int(c) for c in ch[a])
        if not all(c < 0 or not want.open[c] for c in (l, r)) or (l < 0 and r < 0):
            continue
        rl = ~l if l < 0 else int(want.rep[l])
        rr = ~r if r < 0 else int(want.rep[r])
        dd = np.abs(rc.map_at(arrays, [rl], cells.vertices[rr:rr + 1]) - cells.inputs[rr])
        looks += bool((dd <= tol).all())
    assert looks >= 1
    red.close()
    law.close()


def test_leaves_of_different_modes_do_not_merge():
    p, n_u = 3, 1
    rng = np.random.default_rng([95])
    K, c = rc.integer_gain(p, n_u, rng)
    modes = lambda X: (X @ K[0] > np.median(X @ K[0])).astype(np.int32)
    flat = rc.kuhn_tree(p, N_ROOTS, N_SPLIT, rng, rc.affine_inputs(K, c), n_u, modes)
    law = _compile(flat)
    assert set(np.unique(law.leaf_mode).tolist()) == {0, 1}
    red, leaf_of, want, arrays = _check(law, 0.)
    assert N_ROOTS < red.stats['n_leaf'] < law.stats['n_leaf'] and red.stats['n_plane'] > 0
    assert np.array_equal(red.leaf_mode[leaf_of], law.leaf_mode)
    red.close()
    modes_kept = law.leaf_mode
    bare, _, _, _ = _check(law, 0., use_modes=False)
    assert bare.stats['n_leaf'] == N_ROOTS and bare.leaf_mode is None
    bare.close()
    # a table of the wrong length is refused
    from explicit_hybrid_mpc_amd import _capi
    law.leaf_mode = modes_kept[:-1]
    with pytest.raises(_capi.EhmError) as err:
        law.reduce(0.)
    assert err.value.code == _capi.EHM_E_INVALID
    law.close()


def _ancestors(par, leaves):
    out = set()
    for l in leaves:
        up = int(par[2][l])
        while up >= 0:
            out.add(up)
            up = int(par[0][up])
    return out


def test_leaves_without_a_cell_or_a_finite_map_keep_exactly_their_ancestors():
    from explicit_hybrid_mpc_amd import compiled
    rng = np.random.default_rng([96])
    p, n_u = 3, 1
    K, c = rc.integer_gain(p, n_u, rng)
    flat = rc.kuhn_tree(p, 3, 120, rng, rc.affine_inputs(K, c), n_u)
    arrays, _ = cc.compile_flat(flat)
    h = zc.header(arrays)
    below = rc.leaves_below(arrays)
    bad = next(k for k in range(h['n_int']) if 3 <= len(below[k]) <= 12)
    # a plane that bisects nothing
    broken = {k: np.array(v, copy=True) for k, v in arrays.items()}
    broken['node'][bad, :p + 1] *= 0.25
    law = compiled.CompiledLaw.from_arrays(broken)
    red, leaf_of, want, _ = _check(law, 0.)
    assert set(np.nonzero(want.open)[0].tolist()) == _ancestors(want.par, below[bad])
    assert (want.cell_status[below[bad]] == zc.NO_CELL).all()
    assert (leaf_of[below[bad]] != leaf_of[below[bad]][0]).sum() == len(below[bad]) - 1
    red.close()
    law.close()
    # a leaf whose map overflows: NaN against itself
    nan = {k: np.array(v, copy=True) for k, v in arrays.items()}
    l = below[bad][1]
    rc.make_leaf_overflow(nan, l, zc.cells(arrays, [l])[0][0])
    law = compiled.CompiledLaw.from_arrays(nan)
    red, leaf_of, want, _ = _check(law, 0.)
    assert set(np.nonzero(want.open)[0].tolist()) == _ancestors(want.par, [l])
    assert (leaf_of == leaf_of[l]).sum() == 1
    red.close()
    law.close()
    # 300 levels: the 45 leaves without a cell keep the whole chain, the law comes back as it was
    deep, _ = cc.compile_flat(zc.chain_tree(2, 300))
    law = compiled.CompiledLaw.from_arrays(deep)
    red, leaf_of, want, _ = _check(law, 1e300)
    assert (want.cell_status == zc.NO_CELL).sum() == 45 and want.open.all()
    got = red.arrays()
    for k, a in law.arrays().items():
        _same_bytes(got[k], a, k)
    assert np.array_equal(leaf_of, np.arange(301))
    red.close()
    law.close()
    # a single law's sliver chains: where the float planes give no cell, exactly the ancestors stay
    synth = es.SynthLaw(es.kuhn_forest(3, 100), 2, 2, np.random.default_rng([81, 3, 2]), n_sub=12)
    ex = synth.explicit()
    single = ex.compile(dtype=np.float32, flush=True)
    ex.close()
    red, leaf_of, want, _ = _check(single, 1e30, use_modes=False)
    none = np.nonzero(want.cell_status == zc.NO_CELL)[0]
    assert none.size > 0
    assert set(np.nonzero(want.open)[0].tolist()) == _ancestors(want.par, none)
    assert red.stats['n_leaf'] < single.stats['n_leaf']
    red.close()
    single.close()


def _volumes(V):
    p = V.shape[2]
    return np.abs(np.linalg.det(V[:, 1:] - V[:, :1])) / float(np.prod(np.arange(1, p + 1)))


@pytest.mark.parametrize('p,n_u', [(2, 1), (7, 2)])
def test_a_reduced_law_goes_everywhere_a_law_goes(p, n_u, tmp_path):
    from explicit_hybrid_mpc_amd import compiled
    rng = np.random.default_rng([97, p, n_u])
    K, _ = rc.integer_gain(p, n_u, rng)
    centre, width = rc.kink_frame(p, N_ROOTS, K)
    flat = rc.kuhn_tree(p, N_ROOTS, N_SPLIT, rng, rc.clipped_inputs(K, centre, width), n_u)
    law = _compile(flat)
    red, leaf_of, want, arrays = _check(law, 1e-9)
    got = red.arrays()
    compiled.validate_arrays(got)
    path = str(tmp_path / 'reduced.npz')
    red.save(path)
    loaded = compiled.CompiledLaw.load(path)
    for k, a in loaded.arrays().items():
        _same_bytes(a, got[k], k)
    assert np.array_equal(loaded.leaf_mode, red.leaf_mode)
    loaded.close()
    # the cells: the mirror's on the reduced arrays bit for bit; each holds the original cells
    # merged into it and together they have the roots' volume
    cells = red.cells()
    V1, st1 = zc.cells(got)
    assert (st1 == zc.CELL).all() and np.array_equal(cells.status, st1)
    _same_bytes(cells.vertices, V1)
    _same_bytes(cells.inputs, zc.vertex_inputs(got, np.arange(st1.size), V1, st1))
    V0 = want.cells
    vol0, vol1 = _volumes(V0), _volumes(V1)
    assert np.allclose(np.bincount(leaf_of, weights=vol0), vol1, rtol=1e-12, atol=0.)
    assert abs(vol1.sum() - _volumes(zc.root_vertices(arrays)).sum()) <= 1e-12 * vol1.sum()
    merged = V1[leaf_of]
    lam = np.linalg.solve(
        np.concatenate([np.transpose(merged, (0, 2, 1)), np.ones((merged.shape[0], 1, p + 1))],
                       axis=1)[:, None].repeat(p + 1, axis=1),
        np.concatenate([V0, np.ones(V0.shape[:2] + (1,))], axis=2)[..., None])[..., 0]
    assert lam.min() >= -1e-9
    # both orders of narrowing and reducing
    s1 = red.to_single(flush=True)
    s0 = law.to_single(flush=True)
    s2 = s0.reduce(1e-5)
    assert s1.dtype is np.float32 and s2.dtype is np.float32
    assert s1.stats['n_leaf'] == red.stats['n_leaf'] and s2.stats['n_leaf'] <= s0.stats['n_leaf']
    # the closed loop: every applied step is the reduced law's own evaluate
    T, n = 8, 200
    plant = es.random_plant(rng, p, n_u, 1, 'inf', n_g=0)
    w = rng.dirichlet(np.ones(p + 1), n)
    X0 = np.einsum('nv,nvc->nc', w, zc.root_vertices(arrays)[rng.integers(0, N_ROOTS, n)])
    v = rng.normal(size=(T, n, p)) * 1e-3
    for l in (red, s1):
        res = l.rollout(X0, T, plant=plant, v=v)
        applied = 0
        for t in range(T):
            on = np.nonzero(res.steps > t)[0]
            if on.size == 0:
                continue
            z = res.x[t, on] + v[t, on] if t > 0 else res.x[t, on]
            u, leaf, _, _ = l.evaluate(z, return_info=True)
            assert np.array_equal(u, res.u[t, on]) and np.array_equal(leaf, res.leaf[t, on])
            applied += on.size
        assert applied >= n
    for l in (s0, s1, s2, red, law):
        l.close()


def test_refusals_and_the_copy_of_a_law_in_which_nothing_merges():
    from explicit_hybrid_mpc_amd import _capi, explicit
    rng = np.random.default_rng([98])
    p, n_u = 2, 2
    flat = rc.kuhn_tree(p, N_ROOTS, 100, rng, rc.curved_inputs(p, n_u, 1.), n_u)
    law = _compile(flat)
    # nothing merges at tol = 0: an equal, independent copy
    red, leaf_of, want, arrays = _check(law, 0.)
    got = red.arrays()
    for k, a in arrays.items():
        _same_bytes(got[k], a, k)
    assert np.array_equal(leaf_of, np.arange(law.stats['n_leaf']))
    assert np.array_equal(red.leaf_mode, law.leaf_mode) and red.leaf_mode is not law.leaf_mode
    X = rng.uniform(-1., -0.6, (64, p))
    want_u = law.evaluate(X)
    law.close()
    assert np.array_equal(red.evaluate(X), want_u)              # it outlives its source
    # the default tolerance is the audit's
    from explicit_hybrid_mpc_amd import applied
    again = red.reduce()
    assert again.reduction['tol'][0] == applied.default_input_tol(got['leaf_rec'][:, p:p + n_u])
    again.close()
    for bad in (-1e-9, np.nan, np.inf, [1e-9, -1.]):
        with pytest.raises(_capi.EhmError) as err:
            red.reduce(bad)
        assert err.value.code == _capi.EHM_E_INVALID
    with pytest.raises(ValueError):
        red.reduce([1e-9, 1e-9, 1e-9])
    lib = _capi.load()
    roots = zc.root_vertices(got)
    out = _capi.ctypes.c_void_p()
    counts, stats = np.zeros(4, np.int64), np.zeros(2)
    for tol in ([-1., 0.], [0., np.nan]):
        t = np.array(tol)
        assert lib.ehm_compiled_reduce(red._handle, roots.ctypes.data, t.ctypes.data, None,
                                       _capi.ctypes.byref(out), None, None, counts.ctypes.data,
                                       stats.ctypes.data) == _capi.EHM_E_INVALID
        assert b'tol[' in lib.ehm_reduce_last_error() and not out.value
    assert lib.ehm_compiled_reduce(None, roots.ctypes.data, roots.ctypes.data, None,
                                   _capi.ctypes.byref(out), None, None, counts.ctypes.data,
                                   stats.ctypes.data) == _capi.EHM_E_INVALID
    red.close()
    with pytest.raises(ValueError):
        red.reduce()
    # a law with test nodes has no cells to compare on
    ex = explicit.ExplicitMPC(cc.two_point_tree())
    tests = ex.compile()
    ex.close()
    assert tests.stats['n_test'] > 0
    with pytest.raises(_capi.EhmError) as err:
        tests.reduce()
    assert err.value.code == _capi.EHM_E_INVALID and 'test nodes' in str(err.value)
    t = np.zeros(1)
    r1 = np.zeros((1, 2, 1))
    assert lib.ehm_compiled_reduce(tests._handle, r1.ctypes.data, t.ctypes.data, None,
                                   _capi.ctypes.byref(out), None, None, counts.ctypes.data,
                                   stats.ctypes.data) == _capi.EHM_E_INVALID
    assert b'test nodes' in lib.ehm_reduce_last_error()
    tests.close()
    # the shorthand
    ex = rc.explicit_of(flat)
    short = ex.compile(reduce=1e300)
    ex.close()
    assert short.stats['n_leaf'] == N_ROOTS and short.reduction['n_leaf_before'] == N_ROOTS + 100
    short.close()
