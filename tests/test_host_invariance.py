"""
The one-step successors of a compiled law's leaves (invariance.py) without a
device: known answers of the numpy mirror (tests/invariance_cpu.py) on the cube, ``roots_convex``,
and the refusals ``CompiledLaw.successors`` makes before it uses the device.
"""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import compiled_cpu as cc
from tests import explicit_synth as es
from tests import invariance_cpu as iv


def exact_margins(forest, out, n_roots):
    """(margin, worst) per leaf from the exact weights of the dyadic successors: in the root the
    mirror chose where the successor is inside, else in the last root (the serial rule's answer
    for a point no root contains)."""
    n, nv, n_c, p = out.x_next.shape
    margin, worst = np.empty(n), np.empty(n, dtype=np.int32)
    for q in range(n):
        m = np.empty(nv * n_c)
        for i in range(nv):
            for j in range(n_c):
                r = int(out.succ_root[q, i, j])
                w = iv.exact_cube_weights(forest, r if r >= 0 else n_roots - 1, out.x_next[q, i, j])
                assert (w.min() >= 0.) == (r >= 0)
                m[i * n_c + j] = w.min()
        margin[q], worst[q] = m.min(), int(np.argmin(m))
    return margin, worst


def cube_cases(p):
    """(name, K, E, d_box, scale, reach): the successors are scale x + d with |d_c| <= reach, so a
    leaf exits iff one of its vertices has a coordinate with scale |x_c| + reach > 1 -- exact on
    the dyadic vertices.  The box of a quarter never pushes the contraction out (1/2 + 1/4 < 1);
    the box of 5/8 does where a coordinate has modulus above 3/4."""
    box = lambda r: (-r * np.ones(p), r * np.ones(p))
    return [('contraction', -0.5 * np.eye(p), None, None, 0.5, 0.),
            ('expansion', np.eye(p), None, None, 2., 0.),
            ('contraction_quarter_box', -0.5 * np.eye(p), np.eye(p), box(0.25), 0.5, 0.25),
            ('contraction_box', -0.5 * np.eye(p), np.eye(p), box(0.625), 0.5, 0.625)]


def cube_exits(name, V, scale, reach):
    """bool [n]: the leaves with the cells V that exit, from the dyadic vertices; both classes
    are asserted nonempty where the case has both."""
    want = (scale * np.abs(V) + reach > 1.).any(axis=(1, 2))
    if name in ('expansion', 'contraction_box'):
        assert 0 < want.sum() < want.size, name
        bound = 0.5 if name == 'expansion' else 0.75
        assert np.array_equal(want, (np.abs(V) > bound).any(axis=(1, 2)))
    else:
        assert not want.any(), name
    return want


@pytest.mark.parametrize('p', [2, 3])
def test_the_mirror_knows_the_cube(p):
    forest = es.kuhn_forest(p)
    for name, K, E, d_box, scale, reach in cube_cases(p):
        flat = iv.cube_law(p, K)
        arrays, _ = cc.compile_flat(flat)
        plant = iv.identity_plant(p, E=E)
        out = iv.successors(arrays, None, plant, d_box=d_box, tol_exit=0.)
        V = flat.vertices[arrays['leaf_node']]
        assert np.array_equal(out.vertices, V)
        want = cube_exits(name, V, scale, reach)
        assert np.array_equal(out.status, np.where(want, iv.EXITS, iv.INVARIANT)), name
        margin, worst = exact_margins(forest, out, forest.n_roots)
        assert np.array_equal(out.margin, margin), name
        assert np.array_equal(out.worst, worst), name
        assert out.counts == [int((~want).sum()), int(want.sum()), 0, 0, 0]
        assert out.worst_margin == margin.min()
        assert out.worst_leaf == int(np.argmin(margin))
        # the successors themselves: x / 2, 2 x, x / 2 + d
        D = iv.corners(d_box, p) if d_box is not None else np.zeros((1, p))
        assert np.array_equal(out.x_next, scale * V[:, :, None, :] + D[None, None])


def test_roots_convex():
    from explicit_hybrid_mpc_amd.invariance import roots_convex
    rng = np.random.default_rng(11)
    for p in (2, 3, 4):
        full = es.kuhn_forest(p).vertices
        assert roots_convex(full)
        assert roots_convex(full[:1])
        # shifted and scaled by numbers that are not dyadic: shared vertices differ in their last
        # bits between roots
        scale, shift = rng.uniform(0.3, 3., p), rng.uniform(-1., 1., p)
        moved = (full * scale) + shift
        moved = moved * (1. + es.EPS * rng.integers(-2, 3, moved.shape))
        assert len(np.unique(moved.reshape(-1, p), axis=0)) > \
            len(np.unique(full.reshape(-1, p), axis=0))
        assert roots_convex(moved)
        if p == 3:
            R = full.shape[0]
            assert not roots_convex(full[:R - 1])
            assert not roots_convex(moved[:R - 1])
    # an L of three squares (six triangles) is not convex, the two squares in a row are
    full = es.kuhn_forest(2).vertices
    cells = full.reshape(8, 8, 2, 3, 2)
    assert roots_convex(cells[0, :2].reshape(-1, 3, 2))
    ell = np.concatenate([cells[0, :2].reshape(-1, 3, 2), cells[1, :1].reshape(-1, 3, 2)])
    assert not roots_convex(ell)
    with pytest.raises(ValueError):
        roots_convex(np.zeros((3, 3, 3)))


def test_refusals_before_the_device():
    from explicit_hybrid_mpc_amd import invariance
    rng = np.random.default_rng(5)
    p, n_u = 3, 2
    # nothing of a law but what the checks read: a refusal comes before anything else is touched
    law = SimpleNamespace(_handle=1, _rollout_plant=None, mpc=None, p=p, n_u=n_u)
    plant = es.random_plant(rng, p, n_u, 2, 'inf', n_d=2)
    guarded = es.random_guarded(rng, p, n_u, 2, 'inf', substeps=2, n_rows=3)
    with pytest.raises(ValueError, match='guarded'):
        invariance.successors(law, plant=guarded)
    for other in (es.random_plant(rng, p + 1, n_u, 1, 'inf'),
                  es.random_plant(rng, p, n_u + 1, 1, 'inf')):
        with pytest.raises(ValueError, match='does not fit'):
            invariance.successors(law, plant=other)
    for bad in ((np.zeros(3), np.ones(3)), (np.zeros(1), np.ones(1)), (np.zeros(2),),
                (np.array([0., 1.]), np.array([1., 0.5])), (np.zeros(2), np.array([1., np.inf])),
                (np.array([np.nan, 0.]), np.ones(2))):
        with pytest.raises(ValueError, match='d_box'):
            invariance.successors(law, plant=plant, d_box=bad)
    with pytest.raises(ValueError, match='tol_exit'):
        invariance.successors(law, plant=plant, tol_exit=-1.)
    with pytest.raises(ValueError, match='needs a plant'):
        invariance.successors(law)
    with pytest.raises(ValueError, match='closed'):
        invariance.successors(SimpleNamespace(_handle=None), plant=plant)
    assert invariance.STATUS_NAMES == ('invariant', 'exits', 'mode_region', 'no_mode', 'no_cell')
