"""
The reach tube, the limit set and the step sets of a compiled law's closed loop on the device
(csrc/ehm_reach.hip, invariance.py): bit for bit against the numpy mirror
(tests/reach_cpu.py) on the relations of real laws and on graphs no plant makes, the exact cube and
two-mode numbers of tests/test_host_reach.py, soundness against ``CompiledLaw.rollout`` (nominal and
noisy) independent of the mirror, ``max_sweeps``, ``ReachResult.contains`` and the refusals of the C
entry point.
"""

import ctypes

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reach_cpu as rh
from tests import reduce_cpu as rc
from tests.test_gpu_core import _cube, _inside
from tests.test_host_core import two_mode_case
from tests.test_host_invariance import cube_cases
from tests.test_host_reach import (CUBE_TABLE, check_cube_numbers, check_properties, csr,
                                   cube_start, mask_of)

pytestmark = pytest.mark.gpu

ROW_MAPS = ('thread', 'wave')


def _same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _same_box(got, want, what=''):
    """Equal as numbers, NaN where NaN, and a zero of the same sign."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    assert np.array_equal(got, want, equal_nan=True), what
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), what


def _against_mirror(res, mir, what=''):
    for k in ('arrival', 'depart', 'tube_count', 'step_count'):
        _same(getattr(res, k), getattr(mir, k), what + k)
    for k in ('n_arrival', 'leak_step', 'safe', 'settle', 'converged'):
        assert getattr(res, k) == getattr(mir, k), what + k
    assert np.array_equal(res.closure, mir.closure), what
    for k in ('limit', 'limit_outer', 'settle_count', 'settle_box', 'limit_box'):
        assert (getattr(res, k) is None) == (getattr(mir, k) is None), what + k
    for k in ('limit', 'limit_outer'):
        if getattr(mir, k) is not None:
            assert np.array_equal(getattr(res, k), getattr(mir, k)), what + k
    if mir.settle_count is not None:
        _same(res.settle_count, mir.settle_count, what + 'settle_count')
        _same_box(res.settle_box, mir.settle_box, what + 'settle_box')
        _same_box(res.limit_box, mir.limit_box, what + 'limit_box')
    _same_box(res.tube_box, mir.tube_box, what + 'tube_box')
    _same_box(res.step_box, mir.step_box, what + 'step_box')
    assert np.array_equal(res.leaf_box, mir.leaf_box, equal_nan=True), what + 'leaf_box'
    if res.steps is not None:
        _same(res.steps, mir.steps, what + 'steps')


def _cells_of(arrays):
    """The mirror's cells [n_leaf, p+1, p], NaN without one."""
    V, st = zc.cells(arrays)
    V = np.array(V, copy=True)
    V[st != zc.CELL] = np.nan
    return V


def _mirror_of(core, V, start, **kw):
    n = core.level.size
    S = start if start.dtype == np.bool_ else mask_of(n, start)
    return rh.reach(core.indptr, core.indices, core.level, S, V=V, **kw), S


@pytest.mark.parametrize('p,n_u,keep', [(2, 1, 100), (3, 2, 100), (7, 1, 100), (8, 4, 100)])
def test_the_reach_is_the_mirrors_bit_for_bit(p, n_u, keep, tmp_path):
    from explicit_hybrid_mpc_amd import compiled
    rng = np.random.default_rng([91, p, n_u, keep])
    synth = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng, n_sub=12)
    plant = es.random_plant(rng, p, n_u, 2, 'inf' if p % 2 else 'quadratic', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    n_leaf = law.stats['n_leaf']
    modes = rng.integers(-1, 2, n_leaf).astype(np.int32)
    law.set_leaf_modes(modes)
    lo = rng.uniform(-1., 0., 2)
    box = (lo, lo + rng.uniform(0.1, 1., 2))
    X0 = synth.states(rng, 50)

    def run(law_, what):
        core = law_.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True)
        V = _cells_of(law_.arrays())
        assert np.array_equal(law_.cells().vertices, V, equal_nan=True)
        # every leaf with a row always exists; the invariant leaves and the core where there are any
        # (at p = 7, 8 this plant leaves no leaf invariant, and an empty start is refused)
        starts = [('rows', np.diff(core.indptr) > 0)]
        invariant = core.status == iv.INVARIANT
        if invariant.any():
            starts.append(('invariant', invariant))
        if core.core.any():
            starts.append(('core', None))
        assert p > 3 or invariant.any()
        out = {}
        for name, start in starts:
            res = core.reach(start=start, horizon=6, return_steps=True)
            mir, S = _mirror_of(core, V, core.core if start is None else start, horizon=6)
            _against_mirror(res, mir, '%s %s: ' % (what, name))
            check_properties(mir, core.indptr, core.indices, core.level, S)
            assert res.holds == bool(core.set_convex and mir.safe and mir.converged)
            out[name] = res
        # the invariant leaves hold every leaf of level >= 1: they leak, unless all are core
        if invariant.any():
            assert (out['invariant'].leak_step >= 0) == bool((core.level > 0).any())
        assert out['rows'].leak_step == 0 or not (core.level == 0)[np.diff(core.indptr) > 0].any()
        # X0: the leaves the law evaluates the states in
        res = core.reach(X0=X0, horizon=6, return_steps=True)
        u, leaf, _, _ = law_.evaluate(X0, return_info=True)
        ok = np.isfinite(u).all(axis=1)
        rows = np.unique(np.searchsorted(law_.leaf_node, leaf[ok]))
        assert res.n_outside == int((~ok).sum()) and rows.size >= 10
        mir, S = _mirror_of(core, V, rows, horizon=6)
        _against_mirror(res, mir, what + ' X0: ')
        check_properties(mir, core.indptr, core.indices, core.level, S)
        # the other row mapping changes nothing
        other = core.reach(X0=X0, horizon=6, return_steps=True, row_map='wave')
        _against_mirror(other, mir, what + ' X0 wave: ')
        print(p, what, res, 'tube %s, steps %s' % (res.tube_count.tolist(), res.step_count.tolist()))
        assert law_.reach(core, X0=X0).tube_count.tolist() == res.tube_count.tolist()
        return core, list(out.values()) + [res]

    core, first = run(law, 'double')
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    loaded.set_leaf_modes(modes)
    _, again = run(loaded, 'loaded')
    for a, b in zip(first, again):
        _same(a.arrival, b.arrival)
        _same(a.steps, b.steps)
        _same_box(a.tube_box, b.tube_box)
    with pytest.raises(ValueError, match='another law'):
        loaded.reach(core)
    loaded.close()
    single = law.to_single(flush=True)
    run(single, 'single')
    single.close()
    law.close()
    with pytest.raises(ValueError, match='closed'):
        core.reach()


def _graph(n, rng):
    """Rows of every width the lane-stride loop has an edge at (duplicates where the width exceeds
    n), random sparse rows, 10 % seeds, and -- from 65 leaves on -- two tails, one into a 2-cycle and
    one into a 3-cycle, at the end."""
    rows = [rng.integers(0, n, w).tolist() for w in rng.choice([0, 1, 2, 3, 5], n)]
    for l, w in enumerate((0, 1, 63, 64, 65, 300)):
        if l < n:
            rows[l] = rng.integers(0, n, w).tolist()
    level = np.where(rng.random(n) < 0.1, 0, -1).astype(np.int32)
    heads = []
    if n >= 65:
        a = n - 10                      # a -> a+1 -> a+2 <-> a+3;  a+4 -> a+5 -> a+6 -> a+7 -> a+8 -> a+6
        for l, t in ((a, a + 1), (a + 1, a + 2), (a + 2, a + 3), (a + 3, a + 2), (a + 4, a + 5),
                     (a + 5, a + 6), (a + 6, a + 7), (a + 7, a + 8), (a + 8, a + 6)):
            rows[l] = [t, t]            # a duplicate target within the row
        level[a:a + 9] = -1
        heads = [a, a + 4]
    return rows, level, heads


@pytest.fixture(scope='module')
def law1000():
    """A law of exactly 1000 leaves (8 Kuhn roots of the square, 992 bisections) and its cells."""
    rng = np.random.default_rng(1000)
    flat = rc.kuhn_tree(2, 8, 992, rng, rc.affine_inputs(np.array([[1., -2.]]), np.zeros(1)), 1)
    law = _cube(flat)
    assert law.stats['n_leaf'] == 1000
    yield law, _cells_of(law.arrays())
    law.close()


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
def test_graphs_no_plant_makes(n, law1000):
    from explicit_hybrid_mpc_amd import invariance
    law, V = law1000
    rng = np.random.default_rng([7, n])
    rows, level, heads = _graph(n, rng)
    indptr, indices = csr(rows)
    width = np.diff(indptr)
    assert set(width[:6].tolist()) == set((0, 1, 63, 64, 65, 300)[:min(n, 6)])
    starts = [rng.choice(n, min(n, 5), replace=False).astype(np.int32)]
    if n > 6:
        starts.append(np.array([2, 3, 4, 5], dtype=np.int32))           # the wide rows
    if heads:
        starts.append(np.array(heads, dtype=np.int32))
    for s, start in enumerate(starts):
        mir = rh.reach(indptr, indices, level, mask_of(n, start), V=V[:n], horizon=20)
        for row_map in ROW_MAPS:
            res = invariance.reach_relation(law, indptr, indices, level, start, horizon=20,
                                            return_steps=True, row_map=row_map)
            _against_mirror(res, mir, 'n %d start %d %s: ' % (n, s, row_map))
            assert res.row_map == row_map and not res.holds
        # a mask says what the rows say
        res = invariance.reach_relation(law, indptr, indices, level, mask_of(n, start))
        _same(res.arrival, mir.arrival)
        assert res.steps is None and res.step_count.tolist() == [int(start.size)]
    if heads:
        # from the two tails' heads the step sets run into the cycles and have period 6 for ever,
        # long after the closure converged (n_arrival = 4)
        assert mir.safe and mir.n_arrival == 4 and mir.limit.sum() == 5 and mir.settle == 2
        st = mir.steps.astype(bool)
        assert (st.sum(axis=1) == 2).all() and np.array_equal(st[4:14], st[10:20])
        assert not np.array_equal(st[8], st[9]) and not np.array_equal(st[8], st[10])
        assert not np.array_equal(st[8], st[11])
    # the rows of seeds are never read
    seeds = np.nonzero(level == 0)[0]
    if seeds.size:
        bare = [[] if level[l] == 0 else r for l, r in enumerate(rows)]
        res = invariance.reach_relation(law, *csr(bare), level, starts[0], horizon=20,
                                        return_steps=True)
        _against_mirror(res, rh.reach(indptr, indices, level, mask_of(n, starts[0]), V=V[:n],
                                      horizon=20), 'bare ')


def _case(name, p):
    """(flat, plant, d_box, leaf modes or None) of a cube case or of the two-mode case."""
    if name == 'two_mode':
        flat, plant = two_mode_case(p)
        return flat, plant, None, True
    _, K, E, d_box, _, _ = next(c for c in cube_cases(p) if c[0] == name)
    return iv.cube_law(p, K), iv.identity_plant(p, E=E), d_box, False


@pytest.mark.parametrize('name,p,start,want', CUBE_TABLE)
def test_the_cube_and_two_mode_numbers_on_the_device(name, p, start, want):
    flat, plant, d_box, _ = _case(name, p)
    law = _cube(flat)
    single = law.to_single(flush=True)
    for law_, what in ((law, 'double'), (single, 'single')):
        core = law_.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0., rows='all',
                                   return_edges=True)
        V = _cells_of(law_.arrays())
        S = cube_start(core, V, start)
        res = core.reach(start=S, horizon=6, return_steps=True)
        mir, _ = _mirror_of(core, V, S, horizon=6)
        _against_mirror(res, mir, '%s %s: ' % (name, what))
        check_properties(mir, core.indptr, core.indices, core.level, S)
        assert res.set_convex and res.holds == ('leak_step' not in want)
        if what == 'double':
            check_cube_numbers(res, name, V, core, want)
            first = res
            inv = law_.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0.,
                                      return_edges=True)
            _against_mirror(inv.reach(start=S, horizon=6, return_steps=True), mir, 'invariant ')
        else:
            # the single law's side decisions are widened: its relation, and with
            # it every set here, holds the double law's
            assert res.leak_step == first.leak_step
            assert not (first.closure & ~res.closure).any()
            if first.limit is not None:
                assert not (first.limit & ~res.limit).any() and res.settle <= first.settle
        if res.limit is not None:
            vol = np.abs(np.linalg.det(V[:, 1:] - V[:, :1]))
            assert abs(res.limit_volume_fraction - vol[res.limit].sum() / vol.sum()) <= 1e-12
            assert abs(res.closure_volume_fraction - vol[res.closure].sum() / vol.sum()) <= 1e-12
    single.close()
    law.close()


def _walk_is_inside(law, plant, core, res, run, z, T, scale):
    """The records of ``run`` (T steps; ``z`` [T, n, p] the states the law was evaluated at) against
    the result ``res`` of horizon T: leaves and boxes, step by step."""
    assert (run.status == 0).all() and (run.steps == T).all()
    assert res.safe and res.converged and res.holds and res.steps.shape[0] == T + 1
    pad = 1e-12 * scale
    row = np.searchsorted(law.leaf_node, run.leaf)                          # [T, n]
    steps = res.steps.astype(bool)
    for k in range(T):
        assert steps[k][row[k]].all(), k
        assert res.closure[row[k]].all() and core.core[row[k]].all(), k
        assert (z[k] >= res.step_box[k, 0] - pad).all() and \
            (z[k] <= res.step_box[k, 1] + pad).all(), k
        if k >= res.settle:
            assert res.limit[row[k]].all(), k
            assert (z[k] >= res.limit_box[0] - pad).all() and \
                (z[k] <= res.limit_box[1] + pad).all(), k
        j = min(k, res.settle)
        assert (res.closure[row[k]] & ((res.depart[row[k]] < 0) | (res.depart[row[k]] > j))).all()


@pytest.mark.parametrize('name,p', [('two_mode', 2), ('two_mode', 3),
                                    ('contraction_quarter_box', 2)])
def test_no_trajectory_leaves_the_tube(name, p):
    """Independent of the mirror: 2 000 trajectories of 30 steps from points inside start leaves,
    a fresh disturbance of the box each step."""
    rng = np.random.default_rng([53, p, len(name)])
    flat, plant, d_box, _ = _case(name, p)
    law = _cube(flat)
    core = law.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0.,
                              return_edges=True)
    V = law.cells().vertices
    M = np.abs(V).max(axis=(1, 2))
    # two modes: all core leaves; the contraction: the leaves that touch the cube's boundary
    start = core.core if name == 'two_mode' else core.core & (M == 1.)
    assert start.sum() >= 10
    T = 30
    res = core.reach(start=start, horizon=T, return_steps=True)
    print(name, p, res, res.step_count.tolist(), res.limit_box.tolist())
    k = -(-2000 // int(start.sum()))
    X0 = _inside(rng, V[start], k, floor=1e-3)[:2000]
    d = None
    if d_box is not None:
        d = rng.uniform(d_box[0], d_box[1], (T, X0.shape[0], plant.n_d))
    run = law.rollout(X0, T, d=d, plant=plant)
    assert np.array_equal(run.leaf[0], np.repeat(law.leaf_node[start], k)[:2000])
    _walk_is_inside(law, plant, core, res, run, run.x[:T], T, float(np.abs(V).max()))
    assert res.settle >= 1 and res.limit.sum() < res.closure.sum()      # the tube does narrow
    law.close()


@pytest.mark.parametrize('p', [2, 3])
def test_no_noisy_trajectory_leaves_the_tube(p):
    """The same for a ``robust_core`` with small v and e boxes on the two-mode law; the state meant is
    the measured one, x + v of the noisy rollout's records."""
    from tests.test_gpu_robust import _box_model, sym
    rng = np.random.default_rng([59, p])
    flat, plant = two_mode_case(p)
    law = _cube(flat)
    boxes = dict(process=None, state=sym(1. / 64, p), input=sym(1. / 64, p))
    core = law.robust_core(plant=plant, v_box=boxes['state'], e_box=boxes['input'], tol_exit=0.,
                           tol_set=0., tol_side=0., return_edges=True)
    V = law.cells().vertices
    assert core.set_convex and core.core.sum() >= 10
    T = 30
    res = core.reach(horizon=T, return_steps=True)
    print(p, core, res, res.step_count.tolist(), res.limit_box.tolist())
    k = -(-2000 // int(core.core.sum()))
    X0 = _inside(rng, V[core.core], k, floor=1e-3)[:2000]
    run = law.rollout(X0, T, plant=plant, noise=_box_model(p, p, plant.n_d, boxes), seed=5)
    # the draws reach well into the v box; the law's input is 0, so no input error is drawn
    assert np.abs(run.v[1:]).max() >= 0.9 / 64 and not run.e.any()
    v = run.v.copy()
    v[0] = 0.                                               # drawn, not applied: z_0 = x_0
    _walk_is_inside(law, plant, core, res, run, run.x[:T] + v, T, float(np.abs(V).max()))
    law.close()


def test_max_sweeps_and_contains(law1000):
    from explicit_hybrid_mpc_amd import invariance
    law, V = law1000
    n = 1000
    # 0 -> 1 -> .. -> 20 -> 20; the other leaves have no row
    rows = [[l + 1] for l in range(20)] + [[20]] + [[] for _ in range(n - 21)]
    indptr, indices = csr(rows)
    level = np.full(n, -1, dtype=np.int32)
    start = np.array([0, 10], dtype=np.int32)
    full = invariance.reach_relation(law, indptr, indices, level, start)
    mir = rh.reach(indptr, indices, level, mask_of(n, start), V=V)
    _against_mirror(full, mir, 'full ')
    assert full.converged and full.n_arrival == 10 and full.settle == 20
    assert full.limit.sum() == 1 and full.limit[20]
    for m in (1, full.n_arrival - 1, full.n_arrival):
        cut = invariance.reach_relation(law, indptr, indices, level, start, max_sweeps=m,
                                        horizon=12, return_steps=True)
        _against_mirror(cut, rh.reach(indptr, indices, level, mask_of(n, start), V=V,
                                      max_sweeps=m, horizon=12), 'max_sweeps %d ' % m)
        assert not cut.converged and cut.limit is None and cut.limit_outer is None
        assert np.array_equal(cut.arrival, np.where(full.arrival <= m, full.arrival, -1))
        assert cut.tube_box.shape[0] == m + 1 and cut.steps.shape[0] == m + 1
    # enough for phase A (10 sweeps that reach a leaf and one that does not), short of phase B (21)
    for m in (11, 15, 16, 17, 20):
        cut = invariance.reach_relation(law, indptr, indices, level, start, max_sweeps=m)
        _against_mirror(cut, rh.reach(indptr, indices, level, mask_of(n, start), V=V,
                                      max_sweeps=m), 'max_sweeps %d ' % m)
        assert not cut.converged and cut.limit is None and cut.settle == m
        assert not (full.limit & ~cut.limit_outer).any()
        assert np.array_equal(cut.limit_outer, mir.D[m]) and np.array_equal(cut.arrival,
                                                                           full.arrival)
    done = invariance.reach_relation(law, indptr, indices, level, start, max_sweeps=21)
    _against_mirror(done, mir, 'max_sweeps 21 ')
    # contains: the leaf the law evaluates the state in, against D_min(k, settle)
    rng = np.random.default_rng(3)
    X = np.concatenate([_inside(rng, V[:30], 2), rng.uniform(0., 1., (200, 2))])
    row = np.searchsorted(law.leaf_node, law.evaluate(X, return_info=True)[1])
    assert np.array_equal(row[:60], np.repeat(np.arange(30), 2))
    assert np.array_equal(full.contains(X), full.limit[row])
    assert full.contains(X).sum() == 2 + (row[60:] == 20).sum()
    for k in (0, 1, 7, 19, 20, 21, 1000):
        assert np.array_equal(full.contains(X, k=k), mir.D[min(k, full.settle)][row]), k
    with pytest.raises(ValueError, match='limit'):
        cut.contains(X)
    with pytest.raises(ValueError, match='k must'):
        full.contains(X, k=-1)


def test_the_entry_point_refuses(law1000):
    from explicit_hybrid_mpc_amd import _capi, applied
    law, _ = law1000
    lib = _capi.load()
    n = 50
    rng = np.random.default_rng(11)
    rows, level, _ = _graph(n, rng)
    indptr, indices = csr(rows)
    roots = applied.root_cells(law)['vertices']
    start = np.array([0, 7], dtype=np.int32)

    def call(handle=0, leaves=None, **kw):
        o = dict(root_vertices=roots.ctypes.data, indptr=indptr.ctypes.data,
                 indices=indices.ctypes.data, level=level.ctypes.data, start=start.ctypes.data,
                 n_leaf=n, n_edges=indices.size, n_level=n, n_start=start.size, max_sweeps=n,
                 horizon=3, want_steps=0, row_map=0)
        o.update(kw)
        cap = n + 1
        out = dict(arrival=np.empty(n, np.int32), depart=np.empty(n, np.int32),
                   limit=np.empty(n, np.uint8), tube_box=np.empty((cap, 2, 2)),
                   tube_count=np.empty(cap, np.int64), settle_box=np.empty((cap, 2, 2)),
                   settle_count=np.empty(cap, np.int64), step_box=np.empty((4, 2, 2)),
                   step_count=np.empty(4, np.int64))
        lv = {k: a.ctypes.data for k, a in out.items()}
        lv.update(leaves or {})
        res = _capi.ReachResult()
        code = lib.ehm_compiled_reach(law._handle if handle == 0 else handle,
                                      ctypes.byref(_capi.ReachOpts(**o)), ctypes.byref(res),
                                      ctypes.byref(_capi.ReachLeaves(**lv)))
        return code, lib.ehm_reach_last_error(), out, res

    code, _, out, res = call()
    assert code == _capi.EHM_OK
    mir = rh.reach(indptr, indices, level, mask_of(n, start), horizon=3)
    _same(out['arrival'], mir.arrival)
    assert res.n_arrival == mir.n_arrival and res.leak_step == mir.leak_step
    assert res.n_steps == mir.steps.shape[0]
    # a NULL argument
    code, msg, _, _ = call(handle=None)
    assert code == _capi.EHM_E_INVALID and b'bad argument' in msg
    assert lib.ehm_compiled_reach(law._handle, None, None, None) == _capi.EHM_E_INVALID
    for k in ('root_vertices', 'indptr', 'indices', 'level', 'start'):
        code, msg, _, _ = call(**{k: None})
        assert code == _capi.EHM_E_INVALID and b'required array is NULL' in msg, k
    code, msg, _, _ = call(leaves=dict(arrival=None))
    assert code == _capi.EHM_E_INVALID and b'required output is NULL' in msg
    code, msg, _, _ = call(want_steps=1)                    # no array for the step sets
    assert code == _capi.EHM_E_INVALID and b'required output is NULL' in msg
    # a decreasing indptr
    bad = indptr.copy()
    bad[3] = bad[4] + 1
    code, msg, _, _ = call(indptr=bad.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'indptr decreases at row 3' in msg
    bad = indptr.copy()
    bad[0] = 1
    code, msg, _, _ = call(indptr=bad.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'indptr[0] = 1' in msg
    # an index out of range
    for value in (n, -1):
        bad = indices.copy()
        bad[17] = value
        code, msg, _, _ = call(indices=bad.ctypes.data)
        assert code == _capi.EHM_E_INVALID and b'indices[17] = %d' % value in msg
    # an indptr end that is not n_edges
    code, msg, _, _ = call(n_edges=indices.size - 1)
    assert code == _capi.EHM_E_INVALID and b'indptr ends at %d' % indices.size in msg
    code, msg, _, _ = call(n_edges=1 << 31)
    assert code == _capi.EHM_E_INVALID and b'n_edges' in msg
    # an empty start, a start row out of range
    code, msg, _, _ = call(n_start=0)
    assert code == _capi.EHM_E_INVALID and b'start set is empty' in msg
    far = np.array([0, n], dtype=np.int32)
    code, msg, _, _ = call(start=far.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'start[1] = %d' % n in msg
    # the options
    code, msg, _, _ = call(horizon=-1)
    assert code == _capi.EHM_E_INVALID and b'horizon = -1' in msg
    code, msg, _, _ = call(max_sweeps=0)
    assert code == _capi.EHM_E_INVALID and b'max_sweeps' in msg
    code, msg, _, _ = call(row_map=2)
    assert code == _capi.EHM_E_INVALID and b'row_map' in msg
    code, msg, _, _ = call(n_level=n - 1)
    assert code == _capi.EHM_E_INVALID and b'level array' in msg
    for leaves in (0, 1001):
        code, msg, _, _ = call(n_leaf=leaves)
        assert code == _capi.EHM_E_INVALID and b'n_leaf' in msg
    sizes = (ctypes.c_int64 * 3)()
    assert lib.ehm_reach_abi_sizes(ctypes.addressof(sizes), 3) == 3
    assert list(sizes) == [ctypes.sizeof(_capi.ReachOpts), ctypes.sizeof(_capi.ReachResult),
                           ctypes.sizeof(_capi.ReachLeaves)]
