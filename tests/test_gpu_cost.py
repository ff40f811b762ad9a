"""
Certified fuel bounds of a compiled law's closed loop on the device (csrc/ehm_cost.hip,
invariance.py): every array bit for bit against the numpy mirror (tests/cost_cpu.py)
on the relations of synthetic laws of both precisions and on graphs no plant makes, the refusals of
a domain with their named rows, and soundness against ``CompiledLaw.rollout`` (nominal, disturbed and
noisy) independent of the mirror's recurrence: no trajectory spends more than the upper bound or less
than the lower one, over any window.
"""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import cost_cpu as co
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests.test_gpu_core import _cube, _inside
from tests.test_host_cost import check_properties
from tests.test_host_invariance import cube_cases
from tests.test_host_reach import csr, mask_of

pytestmark = pytest.mark.gpu

ARRAYS = ('w_hi', 'w_lo', 'hi', 'lo', 'max_hi', 'min_lo', 'start_hi', 'start_lo', 'rate_hi',
          'rate_lo')


def _same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _against_mirror(res, mir, what='', paths=True):
    for k in ARRAYS:
        _same(getattr(res, k), getattr(mir, k), what + k)
    for k in ('best_rate_hi', 'best_k_hi', 'best_rate_lo', 'best_k_lo', 'n_domain', 'n_start',
              'horizon'):
        assert getattr(res, k) == getattr(mir, k), what + k
    if paths:
        _same(res.path_hi, mir.path_hi, what + 'path_hi')
        _same(res.path_lo, mir.path_lo, what + 'path_lo')
    else:
        assert res.path_hi is None and res.path_lo is None


@pytest.mark.parametrize('p,n_u,keep', [(2, 1, 100), (3, 2, 100), (8, 4, 100)])
def test_the_bounds_are_the_mirrors_bit_for_bit(p, n_u, keep, tmp_path):
    from explicit_hybrid_mpc_amd import _capi, compiled, invariance
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
    H = 6
    S = mask_of(n_leaf, rng.choice(n_leaf, 7, replace=False))

    def run(law_, what):
        core = law_.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True)
        # every leaf, no seed: closed by construction
        level = np.ones(n_leaf, dtype=np.int32)
        arrays = law_.arrays()
        cells = law_.cells()
        w_hi, w_lo, pad = co.weights(arrays, cells.vertices, cells.inputs)
        again = co.weights(arrays)                      # the mirror's own cells and inputs
        for a, b in zip(again, (w_hi, w_lo, pad)):
            assert np.array_equal(a, b, equal_nan=True), what
        D = cells.status == zc.CELL
        indptr, indices = core.indptr, core.indices
        if not D.all():
            # the float planes no longer bisect the deepest sliver cells: those leaves are refused
            # by name, and the bounds are taken on the others, without the edges into them
            assert what == 'single' and D.sum() > 0.9 * n_leaf
            with pytest.raises(_capi.EhmError, match='leaf %d of the domain has no cell'
                               % np.nonzero(~D)[0][0]):
                invariance.cost_relation(law_, indptr, indices, level, np.ones(n_leaf, dtype=bool),
                                         horizon=H)
            keep = D[indices]
            src = np.repeat(np.arange(n_leaf), np.diff(indptr))[keep]
            indptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n_leaf))])
            indices = indices[keep]
        core = SimpleNamespace(indptr=indptr.astype(np.int64), indices=indices)
        assert np.isfinite(w_hi[D]).all() and (w_lo[D] >= 0.).all() and (w_lo[D] <= w_hi[D]).all()
        out = []
        for start, paths in ((None, True), (S, True), (S, False)):
            res = invariance.cost_relation(law_, core.indptr, core.indices, level, D, start=start,
                                           horizon=H, return_paths=paths)
            mir = co.bounds(core.indptr, core.indices, D, w_hi, w_lo, H, start=start)
            _against_mirror(res, mir, '%s: ' % what, paths)
            _same(res.pad, pad, what)
            assert not res.holds and res.seconds_sweeps > 0. and res.seconds_weights > 0.
            out.append(res)
        check_properties(out[0], core.indptr, core.indices, D)
        print(p, what, out[0], 'pad / w_hi <= %.3g' % (pad[D] / np.maximum(w_hi[D], 1e-300)).max())
        return out

    first = run(law, 'double')
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    loaded.set_leaf_modes(modes)
    again = run(loaded, 'loaded')
    for a, b in zip(first, again):
        for k in ARRAYS + ('pad',):
            _same(getattr(a, k), getattr(b, k), k)
    loaded.close()
    single = law.to_single(flush=True)
    narrow = run(single, 'single')
    # the float law's pad is the float roundoff's: wider by about 2^29
    has = ~np.isnan(narrow[0].pad)
    assert (narrow[0].pad[has] > first[0].pad[has] * 2. ** 27).all()
    single.close()
    law.close()


def _graph(n, rng):
    """Rows of every width the lane-stride loop has an edge at (duplicates where the width exceeds
    n), random sparse rows and -- from 65 leaves on -- two tails, one into a 2-cycle and one into a
    3-cycle, at the end, their edges doubled."""
    rows = [rng.integers(0, n, w).tolist() for w in rng.choice([0, 1, 2, 3, 5], n)]
    for l, w in enumerate((0, 1, 63, 64, 65, 300)):
        if l < n:
            rows[l] = rng.integers(0, n, w).tolist()
    heads = []
    if n >= 65:
        a = n - 10
        for l, t in ((a, a + 1), (a + 1, a + 2), (a + 2, a + 3), (a + 3, a + 2), (a + 4, a + 5),
                     (a + 5, a + 6), (a + 6, a + 7), (a + 7, a + 8), (a + 8, a + 6)):
            rows[l] = [t, t]
        heads = [a, a + 4]
    return rows, heads


def _closure(indptr, indices, seen):
    while True:
        more = seen.copy()
        more[indices[np.repeat(seen, np.diff(indptr))]] = True
        if np.array_equal(more, seen):
            return seen
        seen = more


@pytest.fixture(scope='module')
def law1000():
    """A law of exactly 1000 leaves (8 Kuhn roots of the square, 992 bisections)."""
    rng = np.random.default_rng(1000)
    flat = rc.kuhn_tree(2, 8, 992, rng, rc.affine_inputs(np.array([[1., -2.]]), np.zeros(1)), 1)
    law = _cube(flat)
    assert law.stats['n_leaf'] == 1000
    yield law
    law.close()


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
def test_graphs_no_plant_makes(n, law1000):
    from explicit_hybrid_mpc_amd import invariance
    law = law1000
    rng = np.random.default_rng([7, n])
    rows, heads = _graph(n, rng)
    indptr, indices = csr(rows)
    width = np.diff(indptr)
    assert set(width[:6].tolist()) == set((0, 1, 63, 64, 65, 300)[:min(n, 6)])
    level = np.full(n, -1, dtype=np.int32)
    every = np.ones(n, dtype=bool)
    H = 20
    cases = [('random', rng.uniform(0., 1., n), every), ('equal', np.ones(n), every)]
    # few distinct values: ties on most rows, decided by the leaf's index
    cases.append(('few', rng.integers(0, 3, n).astype(np.float64), every))
    if heads:
        tails = _closure(indptr, indices, mask_of(n, heads))
        assert tails.sum() == 9 and not tails.all()            # a strict closed subset
        cases.append(('tails', np.where(tails, np.arange(n) % 4 + 1., np.nan), tails))
    for name, w_lo, D in cases:
        w_hi = w_lo + (rng.integers(0, 2, n) if name != 'equal' else 0.)
        S = D & (rng.random(n) < 0.3)
        S[np.nonzero(D)[0][-1]] = True
        mir = co.bounds(indptr, indices, D, w_hi, w_lo, H, start=S)
        res = invariance.cost_relation(law, indptr, indices, level, D, start=S, horizon=H,
                                       w_hi=w_hi, w_lo=w_lo, return_paths=True)
        _against_mirror(res, mir, 'n %d %s: ' % (n, name))
        assert (res.pad[D] == 0.).all() and np.isnan(res.pad[~D]).all()
        assert res.seconds_weights == 0.
        check_properties(res, indptr, indices, D, S)
        # int rows say what a mask says; no paths: the same values
        bare = invariance.cost_relation(law, indptr, indices, level, np.nonzero(D)[0],
                                        start=np.nonzero(S)[0][::-1], horizon=H, w_hi=w_hi,
                                        w_lo=w_lo)
        _against_mirror(bare, mir, 'n %d %s rows: ' % (n, name), paths=False)
        if name == 'equal' and n > 1:
            # every target ties: the args are the smallest leaf of each row
            one = co.bounds(indptr, indices, D, w_hi, w_lo, 1)
            first = np.array([min(r) if r else -1 for r in rows])
            assert np.array_equal(one.arg_hi[0], first) and np.array_equal(one.arg_lo[0], first)
        if name == 'tails':
            # the worst path runs down a tail into its cycle and goes round it
            a = n - 10
            assert set(res.path_hi[-6:].tolist()) in ({a + 2, a + 3}, {a + 6, a + 7, a + 8})
            top = max(co.cycle_mean(indptr, indices, D, w_hi, True), 0.)
            assert (res.rate_hi[1:] >= top).all() and res.rate_hi[12] >= top
            assert (res.rate_lo[1:] <= co.cycle_mean(indptr, indices, D, w_lo, False)).all()


def test_the_device_refuses_a_domain(law1000):
    from explicit_hybrid_mpc_amd import _capi, invariance
    law = law1000
    n = 1000
    # a ring over the first 900 leaves, every row doubled; the rest feed into it
    rows = [[(l + 1) % 900, (l + 1) % 900] for l in range(900)] + [[0, l] for l in range(900, n)]
    indptr, indices = csr(rows)
    level = np.full(n, -1, dtype=np.int32)
    ring = np.arange(n) < 900
    w = np.ones(n)
    ok = invariance.cost_relation(law, indptr, indices, level, ring, horizon=3, w_hi=w, w_lo=w)
    assert ok.max_hi.tolist() == [0., 1., 2., 3.] and ok.n_domain == 900
    # a seed in the domain: the smallest is named, whatever else is wrong with later rows
    seeded = level.copy()
    seeded[[899, 411, 950]] = 0
    with pytest.raises(_capi.EhmError, match='row 411 is a seed'):
        invariance.cost_relation(law, indptr, indices, seeded, ring, horizon=3, w_hi=w, w_lo=w)
    # not closed: the last row of the domain, in the last wavefront, leaves it
    cut = np.arange(n) < 899
    with pytest.raises(_capi.EhmError, match='row 897 of the domain reaches leaf 898 outside it'):
        invariance.cost_relation(law, indptr, indices, level, np.arange(n) < 898, horizon=3,
                                 w_hi=w, w_lo=w)
    with pytest.raises(_capi.EhmError, match='row 898 of the domain reaches leaf 899 outside it'):
        invariance.cost_relation(law, indptr, indices, level, cut, horizon=3, w_hi=w, w_lo=w)
    # two offenders: the smaller row and its smallest target outside
    rows[5] = [700, 950, 6, 930]
    with pytest.raises(_capi.EhmError, match='row 5 of the domain reaches leaf 930 outside it'):
        invariance.cost_relation(law, *csr(rows), level, ring, horizon=3, w_hi=w, w_lo=w)
    # a seed outside the domain is no matter
    outside = level.copy()
    outside[950] = 0
    res = invariance.cost_relation(law, indptr, indices, outside, ring, horizon=3)
    assert np.isfinite(res.w_hi[ring]).all() and np.isnan(res.w_hi[~ring]).all()


def test_a_leaf_without_a_cell_is_refused():
    """A node that does not bisect the cell that reaches it (tests/test_gpu_certify.py) leaves the
    leaves below it without a cell: in the domain the smallest is refused by name, outside it they
    are no matter."""
    from explicit_hybrid_mpc_amd import _capi, compiled, invariance
    from tests import compiled_cpu as cc
    from tests.test_host_certify import split_tree
    flat, _ = split_tree(3, 2, 1, n_split=60, sliver=30)
    arrays, _ = cc.compile_flat(flat)
    h = zc.header(arrays)
    broken = {k: np.array(v, copy=True) for k, v in arrays.items()}
    broken['node'][h['n_int'] // 2, :h['p'] + 1] *= 0.25
    law = compiled.CompiledLaw.from_arrays(broken)
    st = law.cells().status
    bad = np.nonzero(st != zc.CELL)[0]
    n = st.size
    assert 0 < bad.size < n // 2
    indptr, indices = csr([[l] for l in range(n)])
    level = np.full(n, -1, dtype=np.int32)
    with pytest.raises(_capi.EhmError, match='leaf %d of the domain has no cell' % bad[0]):
        invariance.cost_relation(law, indptr, indices, level, np.ones(n, dtype=bool), horizon=2)
    if bad.size > 1:
        with pytest.raises(_capi.EhmError, match='leaf %d of the domain has no cell' % bad[1]):
            invariance.cost_relation(law, indptr, indices, level, np.arange(n) != bad[0], horizon=2)
    good = st == zc.CELL
    res = invariance.cost_relation(law, indptr, indices, level, good, horizon=2)
    w_hi, w_lo, pad = co.weights(broken)
    _same(res.w_hi, np.where(good, w_hi, np.nan))
    _same(res.hi, np.where(good, w_hi + w_hi, np.nan))
    assert np.isnan(w_hi[~good]).all()
    law.close()


def _norms(u):
    """[T, n]: the 2-norm of every recorded input by the rollout's expression."""
    s = np.zeros(u.shape[:2])
    for c in range(u.shape[2]):
        s = s + u[:, :, c] * u[:, :, c]
    return np.sqrt(s)


def _no_trajectory_outside(law, core, run, T, what):
    """``run``: T recorded steps from states inside core leaves.  Every prefix against U_k, L_k of
    its first leaf and every window against K rate[K], with the slack of the rollout's own
    summation only."""
    assert (run.status == 0).all() and (run.steps == T).all(), what
    nrm = _norms(run.u)
    row0 = np.searchsorted(law.leaf_node, run.leaf[0])
    assert core.core[np.searchsorted(law.leaf_node, run.leaf)].all(), what
    total = np.zeros(nrm.shape[1])
    worst_hi = worst_lo = 0.
    last = None
    for k in range(1, T + 1):
        res = core.cost(horizon=k)
        assert res.holds and res.n_domain == core.core.sum()
        total = total + nrm[k - 1]
        s = (k + 1) * 2. ** -52
        assert (total <= res.hi[row0] * (1. + s)).all(), (what, k)
        assert (total >= res.lo[row0] * (1. - s)).all(), (what, k)
        worst_hi = max(worst_hi, float((total / np.maximum(res.hi[row0], 1e-300)).max()))
        last = res
    assert np.array_equal(total, run.u_norm_sum), what
    for K in range(1, T + 1):
        s = (K + 1) * 2. ** -52
        for t in range(T - K + 1):
            window = np.zeros(nrm.shape[1])
            for j in range(t, t + K):
                window = window + nrm[j]
            assert (window <= K * last.rate_hi[K] * (1. + s)).all(), (what, K, t)
            assert (window >= K * last.rate_lo[K] * (1. - s)).all(), (what, K, t)
    return last, worst_hi


@pytest.mark.parametrize('p', [2, 3])
def test_no_trajectory_spends_more_or_less(p):
    """Independent of the mirror: 2 000 trajectories of 30 steps from points inside core leaves of
    the cube's contraction cases, a fresh disturbance of the box each step, the double law and the
    single law."""
    T = 30
    for name, K, E, d_box, _, _ in cube_cases(p):
        if name not in ('contraction', 'contraction_quarter_box'):     # the nonempty cores
            continue
        rng = np.random.default_rng([61, p, len(name)])
        law = _cube(iv.cube_law(p, K))
        single = law.to_single(flush=True)
        plant = iv.identity_plant(p, E=E)
        for law_, what in ((law, name + ' double'), (single, name + ' single')):
            core = law_.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0.,
                                       return_edges=True)
            assert core.core.any() and core.set_convex
            V = law_.cells().vertices
            k = -(-2000 // int(core.core.sum()))
            X0 = _inside(rng, V[core.core], k, floor=1e-3)[:2000]
            d = None
            if d_box is not None:
                d = rng.uniform(d_box[0], d_box[1], (T, X0.shape[0], plant.n_d))
            run = law_.rollout(X0, T, d=d, plant=plant, record=True)
            assert np.array_equal(run.leaf[0], np.repeat(law_.leaf_node[core.core], k)[:2000])
            res, tight = _no_trajectory_outside(law_, core, run, T, what)
            print(p, what, res, 'closest to the upper bound: %.4f of it' % tight)
            assert tight > 0.5                                      # the bound is no formality
            assert law_.cost(core, horizon=T).hi.tobytes() == res.hi.tobytes()
        single.close()
        law.close()


@pytest.mark.parametrize('p', [2, 3])
def test_no_noisy_trajectory_spends_more_or_less(p):
    """The same under a ``robust_core`` with v and e boxes of 1/64: the leaf is that of the measured
    state and the input the commanded one, which is what ``u_norm_sum`` sums."""
    from tests.test_gpu_robust import _box_model, sym
    T = 30
    rng = np.random.default_rng([67, p])
    law = _cube(iv.cube_law(p, -0.5 * np.eye(p)))
    plant = iv.identity_plant(p)
    boxes = dict(process=None, state=sym(1. / 64, p), input=sym(1. / 64, p))
    core = law.robust_core(plant=plant, v_box=boxes['state'], e_box=boxes['input'], tol_exit=0.,
                           tol_set=0., tol_side=0., return_edges=True)
    assert core.set_convex and core.core.sum() >= 10
    V = law.cells().vertices
    k = -(-2000 // int(core.core.sum()))
    X0 = _inside(rng, V[core.core], k, floor=1e-3)[:2000]
    run = law.rollout(X0, T, plant=plant, noise=_box_model(p, p, plant.n_d, boxes), seed=5,
                      record=True)
    assert np.abs(run.v[1:]).max() >= 0.9 / 64 and np.abs(run.e).max() >= 0.9 / 64
    res, tight = _no_trajectory_outside(law, core, run, T, 'noisy')
    print(p, 'noisy', core, res, 'closest to the upper bound: %.4f of it' % tight)
    # through the limit set of the reach: a smaller domain, no looser a rate
    reach = core.reach()
    lim = reach.cost(core, which='limit', horizon=T)
    assert lim.n_domain == reach.limit.sum() and lim.best_rate_hi <= res.best_rate_hi
    law.close()


def test_the_entry_point_refuses(law1000):
    from explicit_hybrid_mpc_amd import _capi, applied
    law = law1000
    lib = _capi.load()
    n = 50
    rows = [[(l + 1) % n] for l in range(n)]
    indptr, indices = csr(rows)
    level = np.full(n, -1, dtype=np.int32)
    roots = applied.root_cells(law)['vertices']
    dom = np.arange(n, dtype=np.int32)
    start = np.array([0, 7], dtype=np.int32)
    w = np.ones(n)
    H = 3

    def call(handle=0, leaves=None, **kw):
        o = dict(root_vertices=roots.ctypes.data, indptr=indptr.ctypes.data,
                 indices=indices.ctypes.data, level=level.ctypes.data, domain=dom.ctypes.data,
                 start=start.ctypes.data, w_hi=None, w_lo=None, n_leaf=n, n_edges=indices.size,
                 n_level=n, n_domain=n, n_start=start.size, horizon=H, want_paths=0)
        o.update(kw)
        out = dict(w_hi=np.empty(n), w_lo=np.empty(n), pad=np.empty(n), hi=np.empty(n),
                   lo=np.empty(n), max_hi=np.empty(H + 1), min_lo=np.empty(H + 1),
                   start_hi=np.empty(H + 1), start_lo=np.empty(H + 1))
        lv = {k: a.ctypes.data for k, a in out.items()}
        lv.update(leaves or {})
        res = _capi.CostResult()
        code = lib.ehm_compiled_cost(law._handle if handle == 0 else handle,
                                     ctypes.byref(_capi.CostOpts(**o)), ctypes.byref(res),
                                     ctypes.byref(_capi.CostLeaves(**lv)))
        return code, lib.ehm_cost_last_error(), out, res

    code, _, out, res = call(w_hi=w.ctypes.data, w_lo=w.ctypes.data)
    assert code == _capi.EHM_OK and out['max_hi'].tolist() == [0., 1., 2., 3.]
    assert res.n_domain == n and res.n_start == 2
    code, msg, _, _ = call(handle=None)
    assert code == _capi.EHM_E_INVALID and b'bad argument' in msg
    for k in ('root_vertices', 'indptr', 'indices', 'level', 'domain', 'start'):
        code, msg, _, _ = call(**{k: None})
        assert code == _capi.EHM_E_INVALID and b'required array is NULL' in msg, k
    code, msg, _, _ = call(leaves=dict(hi=None))
    assert code == _capi.EHM_E_INVALID and b'required output is NULL' in msg
    code, msg, _, _ = call(want_paths=1)                    # no arrays for the paths
    assert code == _capi.EHM_E_INVALID and b'required output is NULL' in msg
    code, msg, _, _ = call(horizon=0)
    assert code == _capi.EHM_E_INVALID and b'horizon = 0 < 1' in msg
    code, msg, _, _ = call(w_hi=w.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'come together' in msg
    bad = w.copy()
    bad[9] = np.nan
    code, msg, _, _ = call(w_hi=bad.ctypes.data, w_lo=w.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'row 9' in msg and b'not finite' in msg
    code, msg, _, _ = call(w_hi=w.ctypes.data, w_lo=(w + (np.arange(n) == 4)).ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'on row 4' in msg
    code, msg, _, _ = call(n_domain=0)
    assert code == _capi.EHM_E_INVALID and b'domain set is empty' in msg
    code, msg, _, _ = call(n_start=0)
    assert code == _capi.EHM_E_INVALID and b'start set is empty' in msg
    far = np.array([0, n], dtype=np.int32)
    code, msg, _, _ = call(start=far.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'start[1] = %d' % n in msg
    code, msg, _, _ = call(n_domain=5)
    assert code == _capi.EHM_E_INVALID and b'start row 7 is not in the domain' in msg
    ptr_bad = indptr.copy()
    ptr_bad[3] = ptr_bad[4] + 1
    code, msg, _, _ = call(indptr=ptr_bad.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'cost: indptr decreases at row 3' in msg
    idx_bad = indices.copy()
    idx_bad[17] = n
    code, msg, _, _ = call(indices=idx_bad.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'indices[17] = %d' % n in msg
    for leaves in (0, 1001):
        code, msg, _, _ = call(n_leaf=leaves)
        assert code == _capi.EHM_E_INVALID and b'n_leaf' in msg
    sizes = (ctypes.c_int64 * 3)()
    assert lib.ehm_cost_abi_sizes(ctypes.addressof(sizes), 3) == 3
    assert list(sizes) == [ctypes.sizeof(_capi.CostOpts), ctypes.sizeof(_capi.CostResult),
                           ctypes.sizeof(_capi.CostLeaves)]
