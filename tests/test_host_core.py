"""
The may-reach relation between a compiled law's leaves and the invariant core (invariance.py,
DESIGN.md 3.8i) without a device: exact answers of the numpy mirror (tests/core_cpu.py) on the cube,
the fixed point checked from the mirror's own edges, the widening of a single law's side decisions
against numpy-float32 sums, and the refusals ``invariant_core`` makes before it uses the device.
"""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import compiled_cpu as cc
from tests import core_cpu as kc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests.test_host_invariance import cube_cases


def largest_coordinate(V):
    """M per leaf: the largest |coordinate| of the leaf's vertices."""
    return np.abs(V).max(axis=(1, 2))


def _det(M):
    """Laplace expansion along the first row: exact on dyadic entries of this size."""
    n = M.shape[-1]
    if n == 1:
        return M[..., 0, 0]
    cols = np.arange(n)
    return sum((-1.) ** j * M[..., 0, j] * _det(M[..., 1:, cols != j]) for j in range(n))


def dyadic_volumes(V):
    """p! times the volume of the cells V [n, p+1, p], exactly."""
    return np.abs(_det(V[:, 1:] - V[:, :1]))


def two_mode_case(p):
    """(flat, plant): x+ = x / 2 (mode 0) on the leaves of the inner box [-1/2, 1/2]^p, x+ = 2 x
    (mode 1) on the others; the law's input is 0.  The inner box is a union of the forest's grid
    cubes (side 1/4), so no cell straddles its faces and the centroid decides the mode."""
    from explicit_hybrid_mpc_amd import simulate
    flat = iv.cube_law(p, np.zeros((p, p)), modes=lambda C: (np.abs(C).max(axis=1) > 0.5)
                       .astype(np.int32))
    eye = np.eye(p)
    plant = simulate.Plant([0.5 * eye, 2. * eye], [eye, eye], [np.zeros(p)] * 2, None,
                           [None, None], None, None, eye, eye, 'inf')
    return flat, plant


def check_fixed_point(out):
    """The levels against the edges, whatever computed them: level 0 iff seed; level k > 0 iff the
    smallest level in the row is k - 1; the rows of core leaves lie in the core."""
    n = out.level.size
    seed = out.status != iv.INVARIANT
    assert np.array_equal(out.level == 0, seed)
    big = np.iinfo(np.int32).max
    for l in range(n):
        t = out.indices[out.indptr[l]:out.indptr[l + 1]]
        lv = out.level[t]
        lowest = lv[lv >= 0].min() if (lv >= 0).any() else big
        if seed[l]:
            continue
        if out.level[l] < 0:
            assert lowest == big, l
        else:
            assert out.level[l] == lowest + 1, l
    assert out.n_sweeps == out.level.max() + 1
    assert out.counts['core'] == int((out.level < 0).sum())
    assert sum(out.counts.values()) == n


@pytest.mark.parametrize('p', [2, 3])
def test_the_mirror_knows_the_cube(p):
    for name, K, E, d_box, scale, reach in cube_cases(p):
        flat = iv.cube_law(p, K)
        arrays, _ = cc.compile_flat(flat)
        plant = iv.identity_plant(p, E=E)
        out = kc.core(arrays, None, plant, d_box=d_box, tol_exit=0., tol_side=0.)
        check_fixed_point(out)
        V = flat.vertices[arrays['leaf_node']]
        M = largest_coordinate(V)
        n = M.size
        if name in ('contraction', 'contraction_quarter_box'):
            assert out.core.all() and out.n_sweeps == 0, name
            assert out.counts == dict(zip(kc.COUNT_NAMES, [n, 0, 0, 0, 0, 0, 0]))
            assert (np.diff(out.indptr) >= 1).all()
        else:
            assert not out.core.any(), name
            assert out.counts['unresolved'] == 0 and out.n_sweeps >= 2
        if name == 'expansion':
            # the steps that are safe for the vertex farthest out: min{k >= 0 : 2^(k+1) M > 1}
            safe = np.array([next(k for k in range(64) if 2. ** (k + 1) * m > 1.) for m in M])
            assert (out.level <= safe).all()
            assert np.array_equal(out.level == 0, M > 0.5)
            assert (out.level >= 1).any()
        if name == 'contraction_box':
            assert np.array_equal(out.level == 0, M > 0.75)


@pytest.mark.parametrize('p', [2, 3])
def test_two_modes_the_core_is_the_inner_box(p):
    flat, plant = two_mode_case(p)
    arrays, _ = cc.compile_flat(flat)
    modes = rc.leaf_modes(flat, arrays)
    assert (modes == 0).any() and (modes == 1).any()
    out = kc.core(arrays, modes, plant, tol_exit=0., tol_side=0.)
    check_fixed_point(out)
    V = flat.vertices[arrays['leaf_node']]
    inner = largest_coordinate(V) <= 0.5
    assert np.array_equal(inner, modes == 0)
    assert np.array_equal(out.core, inner)
    assert np.array_equal(out.level, np.where(inner, -1, 0)) and out.n_sweeps == 1
    vol = dyadic_volumes(V)
    assert vol[out.core].sum() / vol.sum() == 2. ** -p
    # the whole graph: an outer leaf has a row too, and it is a seed all the same
    full = kc.core(arrays, modes, plant, tol_exit=0., tol_side=0., rows='all')
    assert np.array_equal(full.level, out.level)
    assert full.n_edges > out.n_edges
    inner_rows = np.repeat(inner, np.diff(full.indptr))
    assert np.array_equal(full.indices[inner_rows], out.indices)


def test_a_row_holds_what_the_evaluator_returns():
    """The relation against ``compiled_cpu.evaluate``, independent of how it was built: successors
    of points inside a leaf's cell, under disturbances of the box, land in leaves of its row."""
    p = 2
    rng = np.random.default_rng([17, p])
    K = np.array([[-0.4, 0.3], [-0.2, -0.6]])
    flat = iv.cube_law(p, K, c=np.array([0.05, -0.1]), n_split=60)
    arrays, _ = cc.compile_flat(flat)
    plant = iv.identity_plant(p, E=np.array([[0.1, 0.02], [0., 0.07]]))
    box = (np.array([-1., -0.5]), np.array([0.5, 1.]))
    out = kc.core(arrays, None, plant, d_box=box, rows='all')
    n = out.level.size
    assert (np.diff(out.indptr) >= 1).all() and (out.status == iv.INVARIANT).sum() >= n // 2
    w = rng.dirichlet(np.ones(p + 1), (n, 16))
    X = np.einsum('nkv,nvc->nkc', w, out.vertices).reshape(-1, p)
    U, leaf = cc.evaluate(arrays, X)[:2]
    assert np.array_equal(leaf, np.repeat(arrays['leaf_node'], 16))
    D = rng.uniform(box[0], box[1], (X.shape[0], p))
    Z = es.nominal_step(plant, X, U, np.zeros(X.shape[0], dtype=int), D)
    inside = (np.abs(Z) <= 1.).all(axis=1)
    assert inside.sum() >= 0.9 * inside.size
    to = np.searchsorted(arrays['leaf_node'], cc.evaluate(arrays, Z)[1])
    for q in np.nonzero(inside)[0]:
        l = q // 16
        assert to[q] in out.indices[out.indptr[l]:out.indptr[l + 1]], (l, to[q])


def test_the_fixed_point_on_a_hand_made_graph():
    # 0 -> 1 -> 2 (seed); 3 <-> 4 closed; 5 -> {3, 0}; 6 has no row and is no seed
    rows = [[1], [2], [], [4], [3], [3, 0], []]
    indptr = np.cumsum([0] + [len(r) for r in rows])
    indices = np.array([t for r in rows for t in r], dtype=np.int32)
    seed = np.array([0, 0, 1, 0, 0, 0, 0], dtype=bool)
    level = kc.fixed_point(seed, indptr, indices)
    assert level.tolist() == [2, 1, 0, -1, -1, 3, -1]


@pytest.mark.parametrize('p', [1, 2, 5, 6, 8])
def test_the_widening_bounds_the_float_walk(p):
    """|s as walk32 sums it - s| <= widening32 for points of a box: the narrowed state, every
    product and every sum rounded to float, against the sum in extended precision."""
    rng = np.random.default_rng([29, p])
    worst = 0.
    for trial in range(400):
        scale = 10. ** rng.uniform(-3, 3)
        a = (rng.normal(size=p + 1) * scale).astype(np.float32)
        if trial % 7 == 0:
            a[p] = np.float32(-(a[:p].astype(np.float64) @ np.ones(p)))    # cancellation
        X = 10. ** rng.uniform(-3, 2, p)
        Z = rng.uniform(-1., 1., (64, p)) * X
        Z[:8] = np.where(rng.integers(0, 2, (8, p)) > 0, X, -X)             # corners of the box
        xs = Z.astype(np.float32)
        s32 = np.zeros(64, dtype=np.float32)
        for c in range(p):
            s32 = s32 + a[c] * xs[:, c]
        s32 = s32 + a[p]
        assert s32.dtype == np.float32
        exact = np.zeros(64, dtype=np.longdouble)
        for c in range(p):
            exact = exact + np.longdouble(a[c]) * Z[:, c].astype(np.longdouble)
        exact = exact + np.longdouble(a[p])
        err = np.abs(s32.astype(np.longdouble) - exact).max()
        bound = kc.widening32(a.astype(np.float64), X, p)
        assert err <= bound, (trial, float(err), bound)
        worst = max(worst, float(err / bound))
    print('p = %d: largest error / bound %.3f' % (p, worst))
    assert worst > 0.01                                 # the bound is not vacuous


def test_refusals_before_the_device():
    from explicit_hybrid_mpc_amd import invariance
    rng = np.random.default_rng(5)
    p, n_u = 3, 2
    law = SimpleNamespace(_handle=1, _rollout_plant=None, mpc=None, p=p, n_u=n_u)
    plant = es.random_plant(rng, p, n_u, 2, 'inf', n_d=2)
    guarded = es.random_guarded(rng, p, n_u, 2, 'inf', substeps=2, n_rows=3)
    with pytest.raises(ValueError, match='guarded'):
        invariance.invariant_core(law, plant=guarded)
    with pytest.raises(ValueError, match='does not fit'):
        invariance.invariant_core(law, plant=es.random_plant(rng, p + 1, n_u, 1, 'inf'))
    for bad in ((np.zeros(3), np.ones(3)), (np.array([0., 1.]), np.array([1., 0.5])),
                (np.zeros(2), np.array([1., np.inf]))):
        with pytest.raises(ValueError, match='d_box'):
            invariance.invariant_core(law, plant=plant, d_box=bad)
    with pytest.raises(ValueError, match='tol_exit'):
        invariance.invariant_core(law, plant=plant, tol_exit=-1.)
    for bad in (-1e-9, np.nan):
        with pytest.raises(ValueError, match='tol_side'):
            invariance.invariant_core(law, plant=plant, tol_side=bad)
    with pytest.raises(ValueError, match='rows'):
        invariance.invariant_core(law, plant=plant, rows='some')
    with pytest.raises(ValueError, match='max_fan'):
        invariance.invariant_core(law, plant=plant, max_fan=0)
    with pytest.raises(ValueError, match='max_edges'):
        invariance.invariant_core(law, plant=plant, max_edges=2 ** 31)
    with pytest.raises(ValueError, match='needs a plant'):
        invariance.invariant_core(law)
    with pytest.raises(ValueError, match='closed'):
        invariance.invariant_core(SimpleNamespace(_handle=None), plant=plant)
    assert invariance.CORE_STATUS_NAMES == invariance.STATUS_NAMES + ('unresolved',)
    assert invariance.CORE_COUNT_NAMES == kc.COUNT_NAMES
    assert not hasattr(invariance.invariant_core, 'leaves')
    import inspect
    assert 'leaves' not in inspect.signature(invariance.invariant_core).parameters
