"""
Invariance under measurement and input error (robust.py, noise.bounding_boxes)
without a device: the numpy mirror (tests/robust_cpu.py) against closed forms on the cube, against the
corner-enumerating mirror of 3.8h, against ``compiled_cpu.evaluate`` for the rows; the interval hulls
of a ``NoiseModel`` against its own draws; and the refusals made before the device is used.
"""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import compiled_cpu as cc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests import robust_cpu as rb
from tests.robust_cpu import (ALL_STAY, NO_ERROR, SOME_EXIT, closed_form, cube,
                              largest_coordinate, sym)
from tests.test_host_core import check_fixed_point

@pytest.mark.parametrize('p', [2, 3])
@pytest.mark.parametrize('ab', [ALL_STAY, SOME_EXIT, NO_ERROR])
def test_the_mirror_knows_the_cube(p, ab):
    a, b = ab
    flat, arrays = cube(p)
    plant = iv.identity_plant(p)
    want = closed_form(flat, arrays, a, b)
    assert (np.abs(want) > 1e-6).all()                      # no status hangs on rounding
    out = rb.core(arrays, None, plant, v_box=sym(a, p), e_box=sym(b, p), tol_exit=0., tol_set=0.,
                  tol_side=0.)
    one = out.seeds
    assert one.set_convex and one.n_generators == 3 * p and one.n_facets >= 2 * p
    assert np.abs(one.margin - want).max() <= 1e-12
    assert np.array_equal(one.status, np.where(want < 0., rb.EXITS, rb.INVARIANT))
    check_fixed_point(out)
    n = want.size
    if ab == SOME_EXIT:
        assert 0 < one.counts[rb.EXITS] < n
        assert np.array_equal(out.level == 0, want < 0.)
        assert not out.core[want < 0.].any()
    else:
        assert one.counts == [n, 0, 0, 0, 0]
        assert out.core.all() and out.n_sweeps == 0
    if ab == NO_ERROR:
        assert np.abs(one.margin - (1. - largest_coordinate(
            flat.vertices[arrays['leaf_node']]) / 2.)).max() <= 1e-12
    # the facet and the vertex `worst` names give the margin
    f, i = one.worst // (p + 1), one.worst % (p + 1)
    val = np.einsum('nc,nc->n', one.normals[f], one.y[np.arange(n), i]) - one.offsets[f] + \
        one.slack[f, 0]
    assert np.abs(val - one.margin).max() <= 1e-15


# (p, a, b), None for no box: n_g = 6, 6, 3, 6; the last three make some leaves exit
CORNER_CASES = [(2,) + ALL_STAY, (2,) + SOME_EXIT, (3, 1. / 4 + 2. ** -10, None),
                (3, None, 1. / 2 + 2. ** -10), (3, 1. / 8, None)]


@pytest.mark.parametrize('p,a,b', CORNER_CASES)
def test_closed_form_extrema_agree_with_enumerated_corners(p, a, b):
    """The robust status against the corner-enumerating mirror of 3.8h run on a one-mode plant whose
    E is G and whose box is the stacked box: on a convex set, with no margin at 0, they agree."""
    flat, arrays = cube(p)
    kw = dict(v_box=None if a is None else sym(a, p), e_box=None if b is None else sym(b, p))
    out = rb.successors(arrays, None, iv.identity_plant(p), tol_exit=0., tol_set=0., **kw)
    assert out.n_generators <= 8 and (np.abs(out.margin) > 1e-6).all()
    assert np.abs(out.margin - closed_form(flat, arrays, a or 0., b or 0.)).max() <= 1e-12
    old = iv.successors(arrays, None, iv.identity_plant(p, E=out.G[0]), d_box=(out.lo, out.hi),
                        tol_exit=0.)
    assert old.n_corners == 1 << out.n_generators
    assert np.array_equal(out.status, old.status)
    exits = (out.status == rb.EXITS).sum()
    assert (0 < exits < out.status.size) if (a, b) != ALL_STAY and a != 1. / 8 else exits == 0


@pytest.mark.parametrize('face', [0., 0.125])
def test_mode_region_on_exactly_the_leaves_within_the_v_box_of_the_face(face):
    """Two modes whose regions split the cube at x_0 = face, leaf modes from the centroid: the true
    state of a leaf of mode 0 can pass the face iff max x_0 + a > face, of mode 1 iff
    min x_0 - a < face."""
    p, a = 2, 0.125
    flat, arrays = cube(p, modes=lambda C: (C[:, 0] > face).astype(np.int32))
    modes = rc.leaf_modes(flat, arrays)
    e0 = np.eye(p)[:1]
    plant = iv.identity_plant(p, n_modes=2, regions=[(e0, np.array([face])),
                                                     (-e0, np.array([-face]))])
    out = rb.successors(arrays, modes, plant, v_box=sym(a, p), tol_exit=0., tol_set=0.)
    x0 = flat.vertices[arrays['leaf_node']][:, :, 0]
    near = np.where(modes == 0, x0.max(axis=1) + a > face, x0.min(axis=1) - a < face)
    assert near.sum() >= 10 and (~near).sum() >= 10
    assert np.array_equal(out.status == rb.MODE_REGION, near)
    assert (out.status[~near] == rb.INVARIANT).all()        # 1/2 + 2/8 < 1
    none = rb.successors(arrays, modes, plant, tol_exit=0., tol_set=0.)
    straddles = (x0.min(axis=1) < face) & (x0.max(axis=1) > face)
    assert np.array_equal(none.status == rb.MODE_REGION, straddles)


@pytest.mark.parametrize('p', [2, 3])
def test_a_row_holds_what_the_evaluator_returns(p):
    """The relation against ``compiled_cpu.evaluate``, independent of how it was built: the measured
    successor of a measured state inside a leaf's cell, under errors of the boxes, lands in a leaf
    of the leaf's row."""
    rng = np.random.default_rng([19, p])
    K = -0.5 * np.eye(p) + 0.1 * rng.uniform(-1., 1., (p, p))
    flat, arrays = cube(p, K, c=0.05 * rng.uniform(-1., 1., p), n_split=60)
    E = 0.1 * rng.uniform(-1., 1., (p, 2))
    plant = iv.identity_plant(p, E=E)
    d_box = (np.array([-1., -0.5]), np.array([0.5, 1.]))
    v_box = (-rng.uniform(0., 0.05, p), rng.uniform(0., 0.05, p))
    e_box = (-rng.uniform(0., 0.05, p), rng.uniform(0., 0.05, p))
    out = rb.core(arrays, None, plant, d_box=d_box, v_box=v_box, e_box=e_box, rows='all')
    check_fixed_point(out)
    n = out.level.size
    assert out.seeds.n_generators == 2 + 3 * p and (np.diff(out.indptr) >= 1).all()
    k = -(-2000 // n)
    w = rng.dirichlet(np.ones(p + 1), (n, k))
    Z = np.einsum('nkv,nvc->nkc', w, out.vertices).reshape(-1, p)
    U, leaf = cc.evaluate(arrays, Z)[:2]
    assert np.array_equal(leaf, np.repeat(arrays['leaf_node'], k)) and Z.shape[0] >= 2000
    draw = lambda box: rng.uniform(box[0], box[1], (Z.shape[0], box[0].size))
    D, V, Ee, V1 = draw(d_box), draw(v_box), draw(e_box), draw(v_box)
    Zn = es.nominal_step(plant, Z - V, U + Ee, np.zeros(Z.shape[0], dtype=int), D) + V1
    inside = (np.abs(Zn) <= 1.).all(axis=1)
    assert inside.sum() >= 0.8 * inside.size
    to = np.searchsorted(arrays['leaf_node'], cc.evaluate(arrays, Zn)[1])
    for q in np.nonzero(inside)[0]:
        l = q // k
        assert to[q] in out.indices[out.indptr[l]:out.indptr[l + 1]], (l, to[q])
    # a state of an invariant leaf never leaves the set
    assert inside[np.repeat(out.seeds.status == rb.INVARIANT, k)].all()


# -- the interval hulls of a NoiseModel --------------------------------------------------------------
def test_bounding_boxes_of_box_terms_are_exact():
    from explicit_hybrid_mpc_amd.noise import NoiseModel, bounding_boxes
    rng = np.random.default_rng(3)
    m = NoiseModel(3, 2, 2)
    terms = {'process': [], 'state': [], 'input': []}
    for kind, out, dim in (('state', 3, 4), ('state', 3, 3), ('input', 2, 2), ('process', 2, 5)):
        lb = rng.uniform(-1., 0.5, dim)
        ub = lb + rng.uniform(0., 1., dim)
        M = rng.normal(size=(out, dim))
        m.addIndependentTerm(kind, lb, ub, M=M)
        terms[kind].append(((lb + ub) / 2., (ub - lb) / 2., M))
    got = bounding_boxes(m, np.ones(3), np.ones(2))
    for kind, out in (('process', 2), ('state', 3), ('input', 2)):
        lo, hi = np.zeros(out), np.zeros(out)
        for c, h, M in terms[kind]:
            lo, hi = lo + (M @ c - np.abs(M) @ h), hi + (M @ c + np.abs(M) @ h)
        assert np.array_equal(got[kind][0], lo) and np.array_equal(got[kind][1], hi)


def _models():
    from explicit_hybrid_mpc_amd.mpc_library import SatelliteZ
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    mpc = SatelliteZ(4)
    half = np.array([0.3, 1.5, 0.7])
    return [('from_mpc', NoiseModel.from_mpc(mpc), 0.5 * np.ones(mpc.n_x), 2. * np.ones(mpc.n_u)),
            ('state_input', state_input_model(half, 2), half, np.array([0.8, 0.1]))]


@pytest.mark.parametrize('which', [0, 1])
def test_draws_lie_inside_the_bounding_boxes(which):
    from explicit_hybrid_mpc_amd.noise import KINDS, bounding_boxes, state_bound
    name, model, set_abs, u_abs = _models()[which]
    x_abs = state_bound(model, set_abs, u_abs)
    # the verification itself: set_abs + v_half(x_abs) <= x_abs, and x_abs is not far from the set
    lo, hi = bounding_boxes(model, x_abs, u_abs)['state']
    assert (set_abs + np.maximum(np.abs(lo), np.abs(hi)) <= x_abs).all()
    assert (x_abs >= set_abs).all() and (x_abs <= 1.2 * set_abs + 1e-3).all()
    boxes = bounding_boxes(model, x_abs, u_abs)
    rng = np.random.default_rng([23, which])
    n = 100000
    X = rng.uniform(-1., 1., (n, model.n_x)) * x_abs
    U = rng.uniform(-1., 1., (n, model.n_u)) * u_abs
    X[:64] = np.where(rng.integers(0, 2, (64, model.n_x)) > 0, x_abs, -x_abs)    # corners
    U[:64] = np.where(rng.integers(0, 2, (64, model.n_u)) > 0, u_abs, -u_abs)
    for kind in KINDS:
        if model.out_dim(kind) == 0:
            continue
        S = model.sample(kind, 7, np.arange(n), 3, X, U)
        lo, hi = boxes[kind]
        assert (S >= lo).all() and (S <= hi).all(), (name, kind)
        # not vacuous: the draws fill a good part of every axis that has an error at all
        wide = hi > lo
        assert ((S.max(axis=0) - S.min(axis=0))[wide] >= 0.2 * (hi - lo)[wide]).all(), (name, kind)


def test_state_bound_refuses_an_error_that_does_not_contract():
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_bound
    for sigma in (1., 3., 1e4):
        m = NoiseModel(2, 1, 0)
        m.addDependentTerm('state', sigma, norm=np.inf, L=np.eye(2), Fx=np.eye(2), px=np.inf)
        with pytest.raises(ValueError, match='100 %'):
            state_bound(m, np.ones(2), np.ones(1))
    m = NoiseModel(2, 1, 0)
    m.addDependentTerm('state', 0.5, norm=np.inf, L=np.eye(2), Fx=np.eye(2), px=np.inf)
    x_abs = state_bound(m, np.ones(2), np.ones(1))
    assert np.abs(x_abs - 2.).max() <= 1e-5 and (x_abs >= 2.).all()     # a = 1 + a / 2


def test_refusals_before_the_device():
    from explicit_hybrid_mpc_amd import robust
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    rng = np.random.default_rng(5)
    p, n_u = 3, 2
    law = SimpleNamespace(_handle=1, _rollout_plant=None, mpc=None, p=p, n_u=n_u)
    plant = es.random_plant(rng, p, n_u, 2, 'inf', n_d=2)
    guarded = es.random_guarded(rng, p, n_u, 2, 'inf', substeps=2, n_rows=3)
    ok_v, ok_e, ok_d = sym(0.1, p), sym(0.1, n_u), sym(0.1, 2)
    for call in (robust.robust_successors, robust.robust_core):
        with pytest.raises(ValueError, match='guarded'):
            call(law, plant=guarded, v_box=ok_v)
        with pytest.raises(ValueError, match='does not fit'):
            call(law, plant=es.random_plant(rng, p + 1, n_u, 1, 'inf'))
        with pytest.raises(ValueError, match='not both'):
            call(law, plant=plant, noise=NoiseModel(p, n_u, 2), v_box=ok_v)
        with pytest.raises(ValueError, match='not both'):
            call(law, plant=plant, noise=NoiseModel(p, n_u, 2), d_box=ok_d)
        for name, size in (('d_box', 2), ('v_box', p), ('e_box', n_u)):
            for bad in ((np.zeros(size + 1), np.ones(size + 1)),
                        (-np.ones(size), np.concatenate([[-2.], np.ones(size - 1)])),
                        (-np.ones(size), np.concatenate([[np.inf], np.ones(size - 1)])), 1.):
                with pytest.raises(ValueError, match=name):
                    call(law, plant=plant, **{name: bad})
        # the v and e boxes hold 0; the d box need not
        for name, size in (('v_box', p), ('e_box', n_u)):
            for bad in ((0.1 * np.ones(size), np.ones(size)), (-np.ones(size), -0.1 * np.ones(size))):
                with pytest.raises(ValueError, match=name + ' must hold 0'):
                    call(law, plant=plant, **{name: bad})
        with pytest.raises(ValueError, match='tol_set'):
            call(law, plant=plant, v_box=ok_v, tol_set=-1.)
        with pytest.raises(ValueError, match='tol_exit'):
            call(law, plant=plant, v_box=ok_v, tol_exit=-1.)
        with pytest.raises(ValueError, match='needs a plant'):
            call(law, v_box=ok_v)
        with pytest.raises(ValueError, match='closed'):
            call(SimpleNamespace(_handle=None), plant=plant)
    wide = es.random_plant(rng, 8, 4, 1, 'inf', n_d=45)
    big = SimpleNamespace(_handle=1, _rollout_plant=None, mpc=None, p=8, n_u=4)
    with pytest.raises(ValueError, match='65 generators'):
        robust.robust_successors(big, plant=wide, d_box=sym(1., 45), v_box=sym(0.1, 8),
                                 e_box=sym(0.1, 4))
    with pytest.raises(ValueError, match='rows'):
        robust.robust_core(law, plant=plant, rows='some')
    with pytest.raises(ValueError, match='max_fan'):
        robust.robust_core(law, plant=plant, max_fan=0)
    import inspect
    assert 'leaves' not in inspect.signature(robust.robust_core).parameters
