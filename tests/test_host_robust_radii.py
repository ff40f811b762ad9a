"""
Per-leaf error boxes of the noisy closed loop on the host: the numpy mirror
(tests/robust_radii_cpu.py) against ``noise.bounding_boxes``, the properties of the iteration, the
model's own draws inside the per-leaf boxes, the exact anisotropic cube, and the refusals of the
Python layer that need no law.  No GPU.
"""

import numpy as np
import pytest

from tests import invariance_cpu as iv
from tests import robust_cpu as rb
from tests import robust_radii_cpu as rr

EPS = 2. ** -52


def _models():
    from explicit_hybrid_mpc_amd.mpc_library import SatelliteZ
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    mpc = SatelliteZ(4)
    half = np.array([0.5, 2., 1., 0.25, 3.])
    return [('from_mpc', NoiseModel.from_mpc(mpc)), ('state_input', state_input_model(half, 3))]


def _process_terms(model, rng):
    """The model with a box and a state-dependent ball of kind process more (n_d = 2 where the
    model has no process input of its own)."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    n_d = model.n_d or 2
    m = NoiseModel(model.n_x, model.n_u, n_d)
    m.terms = list(model.terms)
    m.addIndependentTerm('process', lb=[-0.3, -0.1][:n_d], ub=[0.2, 0.4][:n_d])
    m.addDependentTerm('process', 0.05, norm=2, dim=n_d, Fx=rng.uniform(-1., 1., (3, model.n_x)),
                       px=1)
    return m


@pytest.mark.parametrize('which', [0, 1])
def test_boxes_at_is_bounding_boxes_within_the_rounding_of_its_sums(which):
    """The mirror sums |F| a, the norms and the duals in the device's loop order, ``bounding_boxes``
    by BLAS and numpy reductions.  A term's contribution r dual passes through at most
    cols + rows + dim + 4 roundings (the row sums of |F| a, the norm over the rows, the square root,
    sigma r, the dual's sum and root, r dual), each of relative size 2^-52 on sums of non-negative
    numbers; with cols, rows <= 8 and dim <= 8 that is 28, and adding the terms of a kind costs one
    more each.  Both models are symmetric, so every partial sum is at most the bound's modulus: the
    allowed gap is 29 (terms of the kind) 2^-52 max(|lo|, |hi|)."""
    from explicit_hybrid_mpc_amd import noise
    name, model = _models()[which]
    rng = np.random.default_rng([31, which])
    n = 200
    a = rng.uniform(0., 3., (n, model.n_x))
    b = rng.uniform(0., 2., (n, model.n_u))
    a[0], b[0] = 0., 0.
    got = rr.boxes_at(model, a, b)
    worst = 0.
    for q in range(n):
        want = noise.bounding_boxes(model, a[q], b[q])
        for kind in noise.KINDS:
            terms = sum(t.kind == kind for t in model.terms)
            for s in (0, 1):
                g, w = got[kind][s][q], want[kind][s]
                tol = 29. * terms * EPS * np.maximum(np.abs(want[kind][0]), np.abs(want[kind][1]))
                assert (np.abs(g - w) <= tol).all(), (name, kind, q, g, w)
                with np.errstate(invalid='ignore', divide='ignore'):
                    worst = max(worst, float(np.nanmax(np.abs(g - w) / np.where(tol > 0, tol, np.nan),
                                                       initial=0.)))
    print(name, 'largest gap / allowed gap: %.3g' % worst)
    # a kind without terms: zeros
    assert model.n_d == 0 or any(t.kind == 'process' for t in model.terms)


def _random_cells(rng, model, L, half):
    """Random cells, vertex inputs and successors of L leaves in the box of half-widths ``half``, a
    random two-mode plant, and the global bounds the Python layer would start from."""
    from explicit_hybrid_mpc_amd import noise, simulate
    p, n_u, n_d = model.n_x, model.n_u, model.n_d
    centre = rng.uniform(-0.8, 0.8, (L, 1, p)) * half
    V = centre + rng.uniform(-0.2, 0.2, (L, p + 1, p)) * half
    V = np.clip(V, -half, half)
    U = rng.uniform(-1., 1., (L, 1, n_u)) * rng.uniform(0., 1., (L, p + 1, n_u))
    A = [0.5 * np.eye(p) + 0.1 * rng.uniform(-1., 1., (p, p)) for _ in range(2)]
    B = [0.2 * rng.uniform(-1., 1., (p, n_u)) for _ in range(2)]
    w = [0.01 * rng.uniform(-1., 1., p) for _ in range(2)]
    E = 0.05 * rng.uniform(-1., 1., (p, n_d)) if n_d else None
    plant = simulate.Plant(A, B, w, E, [None, None], None, None, np.eye(p), np.eye(n_u), 'inf')
    modes = rng.integers(0, 2, L)
    Y = np.einsum('lij,lvj->lvi', np.array(A)[modes], V) + \
        np.einsum('lij,lvj->lvi', np.array(B)[modes], U) + np.array(w)[modes][:, None, :]
    u_abs = np.abs(U).max(axis=(0, 1))
    x_abs = noise.state_bound(model, half, u_abs)
    return plant, V, U, Y, modes, x_abs, u_abs


@pytest.mark.parametrize('which', [0, 1])
def test_the_iteration_only_ever_lowers_a_valid_bound(which):
    from explicit_hybrid_mpc_amd import noise
    name, model = _models()[which]
    rng = np.random.default_rng([37, which])
    model = _process_terms(model, rng)
    half = np.array([0.5, 2., 1., 0.25, 3.])[:model.n_x]
    plant, V, U, Y, modes, x_abs, u_abs = _random_cells(rng, model, 300, half)
    one = rr.leaf_radii(model, plant, V, U, Y, modes, x_abs, u_abs, iters=1)
    rad = rr.leaf_radii(model, plant, V, U, Y, modes, x_abs, u_abs, iters=3)
    far = rr.leaf_radii(model, plant, V, U, Y, modes, x_abs, u_abs, iters=16)
    its = far.iterates
    assert len(its) == 17 and (its[0] == x_abs).all()
    for k in range(16):
        assert (its[k + 1] <= its[k]).all()                     # non-increasing, and a_L <= x_abs
    assert (rad.x_abs_leaf == its[3]).all() and (one.x_abs_leaf == its[1]).all()
    assert (rad.x_abs_leaf <= x_abs).all() and (rad.x_abs_leaf < x_abs).any()
    assert (one.x_abs_leaf != rad.x_abs_leaf).any()
    # every iterate from the first on is a post-fixed point, up to the rounding of the one sum
    # c_L + vhalf (vhalf is monotone, so vhalf(a^k) <= vhalf(a^(k-1)) needs no allowance)
    for k in (1, 3, 16):
        lo, hi = rr.boxes_at(model, its[k], u_abs, ('state',))['state']
        t = rad.c_leaf + rr.half_of(lo, hi)
        assert (t <= its[k] * (1. + 2. * EPS)).all(), k
    # every per-leaf box inside the global one
    glob = noise.bounding_boxes(model, x_abs, u_abs)
    gl = rr.boxes_at(model, x_abs, u_abs)
    kind_of = dict(process='process', state='state', input='input', state_next='state')
    for k, kind in kind_of.items():
        box = rad.boxes[k]
        assert box is not None and box.shape == (300, 2, model.out_dim(kind))
        assert (box[:, 0] >= gl[kind][0]).all() and (box[:, 1] <= gl[kind][1]).all(), k
        assert (box[:, 0] <= 0.).all() or kind == 'process'
        width = box[:, 1] - box[:, 0]
        assert (width < (glob[kind][1] - glob[kind][0]) * (1. - 1e-3)).any(), k   # and tighter
    assert (rad.x_next_abs <= x_abs).all() and (rad.u_abs_leaf <= u_abs).all()
    # the columns in the order of G_m: [d; v; e; v']
    n_d = model.n_d
    n_g = n_d + 2 * model.n_x + model.n_u
    assert rad.lo.shape == (300, n_g)
    assert (rad.lo[:, n_d:n_d + model.n_x] == rad.boxes['state'][:, 0]).all()
    assert (rad.hi[:, -model.n_x:] == rad.boxes['state_next'][:, 1]).all()
    print(name, 'median a_L / x_abs', np.median(rad.x_abs_leaf / x_abs, axis=0))


@pytest.mark.parametrize('which', [0, 1])
def test_the_models_own_draws_lie_in_the_per_leaf_boxes(which):
    """10^5 draws of ``model.sample`` per kind, at states with |x| <= a_L (a'_L for the next
    measurement) and inputs with |u| <= ubar_L (u_abs for the measurement now), half of them at the
    corner of those bounds.  ``bounding_boxes`` says of itself that a draw may pass a bound by
    rounding: a term's draw is sigma ||F x|| s with |s| <= 1 summed in another order than the bound,
    so the allowance is the one of the first test."""
    name, model = _models()[which]
    rng = np.random.default_rng([41, which])
    model = _process_terms(model, rng)
    p, n_u = model.n_x, model.n_u
    half = np.array([0.5, 2., 1., 0.25, 3.])[:p]
    L, per = 500, 200
    plant, V, U, Y, modes, x_abs, u_abs = _random_cells(rng, model, L, half)
    rad = rr.leaf_radii(model, plant, V, U, Y, modes, x_abs, u_abs, iters=3)
    n = L * per
    assert n == 100000
    leaf = np.repeat(np.arange(L), per)
    ids = np.arange(n)

    def within(bound):
        s = rng.uniform(-1., 1., (n, bound.shape[1]))
        s[::2] = np.sign(s[::2])                                # every other one at a corner
        return s * bound[leaf]

    ug = np.broadcast_to(u_abs, (L, n_u))
    cases = [('state', 'state', rad.x_abs_leaf, ug), ('input', 'input', rad.x_abs_leaf, rad.u_abs_leaf),
             ('process', 'process', rad.x_abs_leaf, rad.u_abs_leaf),
             ('state_next', 'state', rad.x_next_abs, rad.u_abs_leaf)]
    for key, kind, xa, ua in cases:
        draw = model.sample(kind, 7, ids, 3, within(xa), within(ua))
        lo, hi = rad.boxes[key][leaf, 0], rad.boxes[key][leaf, 1]
        terms = sum(t.kind == kind for t in model.terms)
        tol = 29. * terms * EPS * np.maximum(np.abs(lo), np.abs(hi))
        assert (draw >= lo - tol).all() and (draw <= hi + tol).all(), key
        reach = np.abs(draw).max(axis=0) / np.maximum(np.abs(lo), np.abs(hi)).max(axis=0)
        print(name, key, 'largest draw / largest bound', reach)
        assert (reach > 0.5).all(), key                         # the draws are not quiet ones


def test_the_anisotropic_cube_per_leaf_and_global():
    """cube_law(2, K = -diag(1/8, 1/2)) on the identity plant under one state term on coordinate 0 of
    radius sigma |x_1|, sigma = 5/64: z0+ = 7/8 z0 - v0 + v0', z1+ = z1 / 2.  Coordinate 1 has no
    error, so a_L[1] = c_L[1] and a'_L[1] = c_L[1] / 2 exactly, |v0| <= sigma c_L[1],
    |v0'| <= sigma c_L[1] / 2, and the facets +-x_0 give 1 - (7/8 M0 + sigma (3/2) c_L[1]), the facets
    +-x_1 give 1 - c_L[1] / 2.  Per leaf every leaf is invariant (the corner: 1 - 0.9921875 > 0) and
    the core is the whole set; globally |v0|, |v0'| <= sigma (1 + 1e-6) and every leaf with
    M0 > (1 - 2 sigma (1 + 1e-6)) / (7/8) exits."""
    from explicit_hybrid_mpc_amd import noise
    flat, arrays = rb.cube(2, K=rr.ANISO_K)
    plant = iv.identity_plant(2)
    model = rr.aniso_model()
    nominal = iv.successors(arrays, None, plant)
    V = nominal.vertices
    u_abs = np.abs(nominal.inputs).max(axis=(0, 1))
    assert (u_abs == [1. / 8, 1. / 2]).all()
    x_abs = noise.state_bound(model, np.ones(2), u_abs)
    assert x_abs[1] == 1. + 1e-6 and abs(x_abs[0] - (1. + rr.SIGMA) * (1. + 1e-6)) <= 1e-15
    kw = dict(tol_exit=0., tol_set=0.)
    want0, M0, c1 = rr.aniso_closed_form(V)
    want = np.minimum(want0, 1. - c1 / 2.)
    assert (np.abs(want) > 1e-6).all()                          # no margin within 1e-6 of 0
    res = rr.core(arrays, None, plant, model, x_abs, u_abs, iters=3, tol_side=0., **kw)
    one = res.seeds
    assert (one.x_abs_leaf[:, 1] == c1).all() and (one.x_next_abs[:, 1] == c1 / 2.).all()
    assert (one.leaf_boxes['state'][:, 1, 0] == rr.SIGMA * c1).all()
    assert (one.leaf_boxes['state_next'][:, 1, 0] == rr.SIGMA * (c1 / 2.)).all()
    assert (one.leaf_boxes['state'][:, :, 1] == 0.).all()
    assert one.leaf_boxes['input'] is None and one.leaf_boxes['process'] is None
    assert one.n_generators == 4 and one.set_convex
    assert np.abs(one.margin - want).max() <= 1e-12
    assert (one.status == rr.INVARIANT).all() and one.margin.min() > 0.
    assert (1. - want0).max() <= 0.9921875                      # 7/8 + (5/64) (3/2), at a corner
    assert res.core.all() and res.n_sweeps == 0
    # the global boxes on the same law
    bb = noise.bounding_boxes(model, x_abs, u_abs)
    glob = rb.core(arrays, None, plant, v_box=bb['state'], e_box=bb['input'], tol_side=0., **kw)
    g_want = np.minimum(1. - (7. / 8 * M0 + 2. * rr.SIGMA * (1. + 1e-6)), 1. - c1 / 2.)
    assert (np.abs(g_want) > 1e-6).all()
    assert np.abs(glob.seeds.margin - g_want).max() <= 1e-12
    exits = M0 > (1. - 2. * rr.SIGMA * (1. + 1e-6)) / (7. / 8)
    assert 0 < exits.sum() < exits.size
    assert np.array_equal(glob.seeds.status, np.where(exits, rr.EXITS, rr.INVARIANT))
    assert (one.margin >= glob.seeds.margin).all() and not glob.core.all()


def test_constant_boxes_give_the_slack_of_the_global_path_bit_for_bit():
    """With a model of box terms only the leaf's box is the global one, and the facet value summed
    from nG and the box is ``robust_cpu.facet_slack``'s."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel, bounding_boxes
    flat, arrays = rb.cube(3)
    plant = iv.identity_plant(3)
    m = NoiseModel(3, 3, 0)
    m.addIndependentTerm('state', lb=[-0.01, -0.02, 0.], ub=[0.03, 0.01, 0.])
    m.addIndependentTerm('input', lb=-0.05 * np.ones(3), ub=0.02 * np.ones(3))
    x_abs, u_abs = 1.1 * np.ones(3), 0.5 * np.ones(3)
    bb = bounding_boxes(m, x_abs, u_abs)
    leaf = rr.core(arrays, None, plant, m, x_abs, u_abs)
    glob = rb.core(arrays, None, plant, v_box=bb['state'], e_box=bb['input'])
    for k in ('status', 'margin', 'worst'):
        assert getattr(leaf.seeds, k).tobytes() == getattr(glob.seeds, k).tobytes(), k
    for k in ('level', 'status', 'indptr', 'indices'):
        assert getattr(leaf, k).tobytes() == getattr(glob, k).tobytes(), k
    assert (leaf.seeds.leaf_boxes['state'][:, 0] == bb['state'][0]).all()


def test_the_python_layer_refuses_before_it_needs_a_law():
    from explicit_hybrid_mpc_amd import robust
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    model = state_input_model(np.ones(2), 1)
    box = (-np.ones(2), np.ones(2))
    for fn in (robust.robust_successors, robust.robust_core):
        with pytest.raises(ValueError, match="'global' or 'leaf'"):
            fn(None, noise=model, radii='cell')
        with pytest.raises(ValueError, match='noise='):
            fn(None, radii='leaf')
        with pytest.raises(ValueError, match='no boxes'):
            fn(None, noise=model, v_box=box, radii='leaf')
        for bad in (0, 17, -1, 2.5, None, 'three'):
            with pytest.raises(ValueError, match='radius_iters'):
                fn(None, noise=model, radii='leaf', radius_iters=bad)
        with pytest.raises(ValueError, match='radius_iters'):
            fn(None, noise=model, radius_iters=0)               # also where it is not used
        for kind, name in (('state', 'v box'), ('input', 'e box')):
            off = NoiseModel(2, 1, 0)
            off.addIndependentTerm(kind, lb=0.1 * np.ones(off.out_dim(kind)),
                                   ub=0.2 * np.ones(off.out_dim(kind)))
            with pytest.raises(ValueError, match='constant part of the %s' % name):
                fn(None, noise=off, radii='leaf')
        # a state-dependent part may be anything: only the constant part is asked about
        with pytest.raises((ValueError, AttributeError)):
            fn(None, noise=model, radii='leaf')                 # passes the radii checks, then no law


def test_the_new_entry_points_are_declared_and_exported():
    import os
    from explicit_hybrid_mpc_amd import _capi
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, '..', 'include', 'ehmpc.h')).read()
    for name in ('ehm_compiled_robust_successors_leaf', 'ehm_compiled_robust_core_leaf',
                 'ehm_robust_radii_abi_sizes'):
        assert name in _capi.EXPORTED and name + '(' in header
