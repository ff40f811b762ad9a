"""
Per-leaf error boxes of the noisy closed loop on the device (csrc/ehm_radii_dev.h, the LEAF instances
of csrc/ehm_robust.hip and csrc/ehm_core.hip, robust.py): bit for bit against the numpy
mirror (tests/robust_radii_cpu.py), box models against the global path, the exact anisotropic cube,
containment in the global boxes, soundness against the noisy rollout under the state- and
input-dependent model itself, and the refusals of the two C entry points and of the Python layer.
"""

import ctypes

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests import robust_radii_cpu as rr
from tests.test_host_core import check_fixed_point

pytestmark = pytest.mark.gpu

ONE_STEP = ('status', 'margin', 'worst')
PER_LEAF = ('x_abs_leaf', 'x_next_abs', 'u_abs_leaf')
BOXES = ('process', 'state', 'input', 'state_next')
CORE = ('level', 'status', 'indptr', 'indices')
EPS = 2. ** -52


def _same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _step_against_mirror(res, mir, what=''):
    from explicit_hybrid_mpc_amd import invariance
    assert res.radii == 'leaf'
    for k in ONE_STEP + PER_LEAF:
        _same(getattr(res, k), getattr(mir, k), what + k)
    for k in BOXES:
        if mir.leaf_boxes[k] is None:
            assert res.leaf_boxes[k] is None, what + k
        else:
            _same(res.leaf_boxes[k], mir.leaf_boxes[k], what + k)
    assert res.counts == dict(zip(invariance.STATUS_NAMES, mir.counts)), what
    assert res.n_facets == mir.n_facets and res.n_generators == mir.n_generators
    assert res.set_convex == mir.set_convex
    if mir.worst_leaf < 0:
        assert res.worst_leaf is None and np.isnan(res.worst_margin)
    else:
        assert res.worst_leaf['leaf'] == res.leaves[mir.worst_leaf]
        assert res.worst_margin == mir.worst_margin == res.worst_leaf['margin']


def _core_against_mirror(res, mir, what=''):
    for k in CORE:
        _same(getattr(res, k), getattr(mir, k), what + k)
    assert res.counts == mir.counts, what
    assert res.n_sweeps == mir.n_sweeps and res.n_edges == mir.n_edges, what
    _step_against_mirror(res.seeds, mir.seeds, what)


def _same_core(a, b):
    for k in CORE:
        _same(getattr(a, k), getattr(b, k), k)
    for k in ONE_STEP:
        _same(getattr(a.seeds, k), getattr(b.seeds, k), k)
    assert a.counts == b.counts and a.n_sweeps == b.n_sweeps and a.n_edges == b.n_edges
    assert a.core_volume_fraction == b.core_volume_fraction
    assert a.cell_volume_fraction == b.cell_volume_fraction
    assert a.seeds.invariant_volume_fraction == b.seeds.invariant_volume_fraction
    assert a.seeds.cell_volume_fraction == b.seeds.cell_volume_fraction


def _inside(rng, V, k, floor=1e-3):
    """k points per cell of V [n, p+1, p] with every weight >= floor."""
    n, nv, p = V.shape
    w = floor + (1. - nv * floor) * rng.dirichlet(np.ones(nv), (n, k))
    return np.einsum('nkv,nvc->nkc', w, V).reshape(-1, p)


def _synth(p, n_u, keep, seed):
    """A random law of 100 to 600 leaves over ``kuhn_forest(p, keep)`` with two modes and leaves
    without a mode, a random plant with n_d = 2, and a model with a fixed, a state-dependent and an
    input-dependent part of every kind, scaled to the set [-1, 1]^p."""
    rng = np.random.default_rng([seed, p, n_u])
    synth = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng, n_sub=4)
    plant = es.random_plant(rng, p, n_u, 2, 'inf' if p % 2 else 'quadratic', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    n_leaf = law.stats['n_leaf']
    assert 100 < n_leaf < 600
    modes = rng.integers(-1, 2, n_leaf).astype(np.int32)
    assert (modes == -1).any() and (modes == 1).any()
    law.set_leaf_modes(modes)
    model = rr.scaled_model(np.ones(p), n_u, 2, 1., rng)
    return rng, law, plant, modes, model


# the shapes of test_gpu_robust: 100 roots (a sliver of the cube at p = 7, 8) and the full forests of
# p = 2, 3 (a convex set); two modes, leaves without a mode, n_d = 2
@pytest.mark.parametrize('p,n_u,keep', [(2, 1, 100), (3, 2, 100), (7, 1, 100), (8, 4, 100),
                                        (2, 1, None), (3, 2, None)])
def test_both_checks_are_the_mirrors_bit_for_bit(p, n_u, keep, tmp_path):
    from explicit_hybrid_mpc_amd import compiled
    rng, law, plant, modes, model = _synth(p, n_u, keep, 95)
    arrays = law.arrays()
    n_leaf = law.stats['n_leaf']
    kw = dict(plant=plant, noise=model, radii='leaf')
    res = law.robust_core(rows='all', return_edges=True, **kw)
    one = res.seeds
    assert one.radius_iters == 3 and 'leaf' in repr(one)
    x_abs, u_abs = one.x_abs, one.u_abs
    mir = rr.core(arrays, modes, plant, model, x_abs, u_abs, 3, rows='all')
    _core_against_mirror(res, mir, 'all ')
    check_fixed_point(res)
    assert one.n_generators == 2 + 2 * p + n_u and one.n_facets > p
    print(p, n_u, one, res, 'radii %.3g s, step %.3g s, nG %.3g s, reach %.3g s' % (
        one.seconds_radii, one.seconds, one.seconds_slack, res.seconds_reach))
    assert one.counts['no_mode'] > 0 and one.counts['no_cell'] == 0
    dead = one.status >= iv.NO_MODE
    assert np.isnan(one.margin[dead]).all() and np.isnan(one.x_abs_leaf[dead]).all()
    assert np.isnan(one.leaf_boxes['state'][dead]).all()
    live = ~dead
    assert (one.x_abs_leaf[live] <= x_abs).all() and (one.x_abs_leaf[live] < x_abs).any()
    # the one-step call alone, and a subset in the caller's order with a leaf named twice
    alone = law.robust_successors(**kw)
    _step_against_mirror(alone, mir.seeds, 'alone ')
    pick = np.concatenate([rng.permutation(n_leaf)[:50], [0, n_leaf - 1, 0]]).astype(np.int64)
    part = law.robust_successors(leaves=pick, chunk=16, **kw)
    for k in ONE_STEP + PER_LEAF:
        _same(getattr(part, k), getattr(one, k)[pick], k)
    for k in BOXES:
        _same(part.leaf_boxes[k], one.leaf_boxes[k][pick], k)
    assert part.n == pick.size and not part.holds_on_set
    # chunk 16 against one chunk: every array and both volumes
    few = law.robust_successors(chunk=16, **kw)
    _step_against_mirror(few, mir.seeds, 'chunk ')
    assert few.worst_leaf == one.worst_leaf
    assert few.invariant_volume_fraction == one.invariant_volume_fraction
    assert few.cell_volume_fraction == one.cell_volume_fraction
    # one iteration against three: another bound, and its own mirror's
    it1 = law.robust_core(rows='all', return_edges=True, radius_iters=1, **kw)
    _core_against_mirror(it1, rr.core(arrays, modes, plant, model, x_abs, u_abs, 1, rows='all'),
                         'iters 1 ')
    assert not np.array_equal(it1.seeds.x_abs_leaf[live], one.x_abs_leaf[live])
    assert (it1.seeds.x_abs_leaf[live] >= one.x_abs_leaf[live]).all()
    # the same law after save / load
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    _same_core(loaded.robust_core(rows='all', return_edges=True, **kw), res)
    loaded.close()
    # its single form against the mirror in float arithmetic
    single = law.to_single(flush=True)
    s32 = single.robust_core(rows='all', return_edges=True, **kw)
    s_one = s32.seeds
    _core_against_mirror(s32, rr.core(single.arrays(), modes, plant, model, s_one.x_abs,
                                      s_one.u_abs, 3, rows='all'), 'single ')
    assert not np.array_equal(s_one.margin[live], one.margin[live])
    single.close()
    law.close()


def test_a_model_of_boxes_gives_the_global_path_bit_for_bit():
    """Box terms with identity maps have no radius to shrink: the leaf's box is the global one, the
    facet value summed from nG and the box is k_robust_slack's, and every one-step and core array
    is the global path's."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    p, n_u = 3, 2
    rng, law, plant, modes, _ = _synth(p, n_u, None, 96)
    m = NoiseModel(p, n_u, 2)
    m.addIndependentTerm('process', lb=[-0.5, -0.1], ub=[0.25, 0.3])
    m.addIndependentTerm('state', lb=[-0.01, -0.02, 0.], ub=[0.03, 0.01, 0.])
    m.addIndependentTerm('input', lb=-0.05 * np.ones(n_u), ub=0.02 * np.ones(n_u))
    m.addIndependentTerm('state', lb=-0.005 * np.ones(p), ub=0.005 * np.ones(p))
    kw = dict(plant=plant, noise=m, rows='all', return_edges=True)
    leaf = law.robust_core(radii='leaf', **kw)
    glob = law.robust_core(**kw)
    assert glob.seeds.radii == 'global' and glob.seeds.leaf_boxes is None
    _same_core(leaf, glob)
    assert leaf.seeds.counts == glob.seeds.counts and leaf.seeds.worst_leaf == glob.seeds.worst_leaf
    live = leaf.seeds.status < iv.NO_MODE
    for k, kind in zip(BOXES, ('process', 'state', 'input', 'state')):
        for s in (0, 1):
            want = np.broadcast_to(glob.seeds.boxes[kind][s], leaf.seeds.leaf_boxes[k][live, s].shape)
            _same(np.ascontiguousarray(leaf.seeds.leaf_boxes[k][live, s]),
                  np.ascontiguousarray(want), k)
    assert (leaf.level > 0).any() and leaf.seeds.counts['invariant'] > 0
    law.close()


def _cube(flat):
    ex = rc.explicit_of(flat)
    law = ex.compile()
    ex.close()
    return law


def test_the_anisotropic_cube_on_the_device():
    """The exact case of tests/test_host_robust_radii.py: per leaf every leaf is invariant and the
    core is the whole set, globally the leaves with M0 > (1 - 2 sigma (1 + 1e-6)) / (7/8) exit."""
    flat = iv.cube_law(2, rr.ANISO_K)
    law = _cube(flat)
    arrays = law.arrays()
    plant = iv.identity_plant(2)
    model = rr.aniso_model()
    kw = dict(plant=plant, noise=model, tol_exit=0., tol_set=0., tol_side=0., return_edges=True)
    res = law.robust_core(radii='leaf', **kw)
    one = res.seeds
    _core_against_mirror(res, rr.core(arrays, None, plant, model, one.x_abs, one.u_abs, 3,
                                      tol_exit=0., tol_set=0., tol_side=0.))
    V = law.cells().vertices
    want0, M0, c1 = rr.aniso_closed_form(V)
    want = np.minimum(want0, 1. - c1 / 2.)
    assert (np.abs(want) > 1e-6).all()
    assert np.abs(one.margin - want).max() <= 1e-12
    assert (one.status == iv.INVARIANT).all() and one.holds_on_set
    assert (one.x_abs_leaf[:, 1] == c1).all() and (one.x_next_abs[:, 1] == c1 / 2.).all()
    assert one.leaf_boxes['input'] is None and one.leaf_boxes['process'] is None
    assert one.n_generators == 4
    assert res.holds and res.core.all() and res.n_sweeps == 0
    assert abs(res.core_volume_fraction - 1.) <= 1e-12
    glob = law.robust_core(**kw)
    g_want = np.minimum(1. - (7. / 8 * M0 + 2. * rr.SIGMA * (1. + 1e-6)), 1. - c1 / 2.)
    assert (np.abs(g_want) > 1e-6).all()
    assert np.abs(glob.seeds.margin - g_want).max() <= 1e-12
    exits = M0 > (1. - 2. * rr.SIGMA * (1. + 1e-6)) / (7. / 8)
    assert 0 < exits.sum() < exits.size
    assert np.array_equal(glob.seeds.status, np.where(exits, iv.EXITS, iv.INVARIANT))
    assert not glob.core.all()
    law.close()


@pytest.mark.parametrize('p,n_u', [(2, 1), (3, 2)])
def test_the_per_leaf_boxes_lie_in_the_global_ones_and_certify_no_less(p, n_u):
    """Every sum of the facet value and of the relation is monotone in the box under rounding (a
    product with a fixed factor and a sum in a fixed order are), and both paths have the same
    columns, so containment needs no tolerance."""
    rng, law, plant, modes, model = _synth(p, n_u, None, 97)
    kw = dict(plant=plant, noise=model)
    leaf = law.robust_core(radii='leaf', **kw)
    glob = law.robust_core(**kw)
    lo, go = leaf.seeds, glob.seeds
    live = lo.status < iv.NO_MODE
    assert np.array_equal(live, go.status < iv.NO_MODE) and lo.n_generators == go.n_generators
    for k, kind in zip(BOXES, ('process', 'state', 'input', 'state')):
        box = lo.leaf_boxes[k][live]
        assert (box[:, 0] >= go.boxes[kind][0]).all() and (box[:, 1] <= go.boxes[kind][1]).all(), k
        assert (box[:, 1] - box[:, 0] < go.boxes[kind][1] - go.boxes[kind][0]).any(), k
    assert (lo.margin[live] >= go.margin[live]).all()
    assert (lo.margin[live] > go.margin[live]).any()
    assert (lo.status[go.status == iv.INVARIANT] == iv.INVARIANT).all()
    assert leaf.core[glob.core].all()
    print(p, 'global', go.counts, glob.counts, 'leaf', lo.counts, leaf.counts)
    law.close()


def _random_law_p8(rng):
    """``tests/test_gpu_robust._random_law_p8``: one root simplex of the Kuhn forest, 150 bisections,
    a random affine input, a plant that contracts to the centroid by about a fifth."""
    from explicit_hybrid_mpc_amd import simulate
    p, n_u = 8, 4
    K = 0.05 * rng.uniform(-1., 1., (n_u, p))
    flat = rc.kuhn_tree(p, 1, 150, rng, rc.affine_inputs(K, 0.1 * rng.uniform(-1., 1., n_u)), n_u)
    c = flat.vertices[0].mean(axis=0)
    A = 0.2 * np.eye(p) + 0.005 * rng.uniform(-1., 1., (p, p))
    B = 0.02 * rng.uniform(-1., 1., (p, n_u))
    w = c - A @ c - B @ (K @ c)
    E = 0.002 * rng.uniform(-1., 1., (p, 2))
    return flat, simulate.Plant([A], [B], [w], E, [None], None, None, np.eye(p), np.eye(n_u), 'inf')


# the scale of the p = 8 model, picked with the mirror on the CPU: at 1.5 the mirror's per-leaf core is
# the whole law (151 leaves) while under the global boxes every leaf exits; at 2 every leaf exits
# per leaf too
P8_SCALE = 1.5


@pytest.mark.parametrize('case', ['aniso2', 'random8'])
def test_no_noisy_trajectory_from_the_per_leaf_core_ever_stops(case):
    """Independent of the mirror: 4 096 trajectories of 50 steps of the noisy rollout under the state-
    and input-dependent model itself, from states sampled in core leaves.  No trajectory stops, every
    visited leaf is core, and every draw lies in the box of the leaf visited when it was made --
    within the rounding ``bounding_boxes`` states of itself: 29 roundings per term of the kind
    (tests/test_host_robust_radii.py derives the figure)."""
    rng = np.random.default_rng([71, 7, 8])
    if case == 'random8':
        flat, plant = _random_law_p8(rng)
        law = _cube(flat)
        half = np.abs(law.cells().vertices).max(axis=(0, 1))
        model = rr.scaled_model(half, law.n_u, 2, P8_SCALE)
    else:
        flat, plant, model = iv.cube_law(2, rr.ANISO_K), iv.identity_plant(2), rr.aniso_model()
        law = _cube(flat)
    p, n_u = law.p, law.n_u
    res = law.robust_core(plant=plant, noise=model, radii='leaf')
    one = res.seeds
    print(case, one, res)
    assert res.set_convex and res.holds and res.core.sum() >= 10        # else this shows nothing
    V = law.cells().vertices
    k = -(-4096 // int(res.core.sum()))
    X0 = _inside(rng, V[res.core], k)[:4096]
    assert X0.shape[0] == 4096
    T = 50
    run = law.rollout(X0, T, plant=plant, noise=model, seed=11)
    assert (run.status == 0).all() and (run.steps == T).all()
    row = np.searchsorted(law.leaf_node, run.leaf)              # [T, n] rows of the leaf records
    assert (law.leaf_node[row] == run.leaf).all() and res.core[np.unique(row)].all()

    def check(key, kind, draw, at):
        box = one.leaf_boxes[key]
        if box is None:
            assert not any(t.kind == kind for t in model.terms) or draw is None or draw.shape[2] == 0
            return None
        lo, hi = box[at, 0], box[at, 1]
        big = np.maximum(np.abs(lo), np.abs(hi))
        tol = 29. * sum(t.kind == kind for t in model.terms) * EPS * big
        assert (draw >= lo - tol).all() and (draw <= hi + tol).all(), key
        with np.errstate(invalid='ignore', divide='ignore'):
            return float(np.nanmax(np.abs(draw) / np.where(big > 0., big, np.nan)))

    reach_v = check('state', 'state', run.v, row)               # v_t at the leaf of z_t (v_0 = 0)
    reach_n = check('state_next', 'state', run.v[1:], row[:-1])  # v_(t+1) at the leaf visited at t
    reach_e = check('input', 'input', run.e, row)
    reach_d = check('process', 'process', run.w, row)
    print(case, 'largest draw over its leaf\'s bound: v %s, v\' %s, e %s, d %s' % (
        reach_v, reach_n, reach_e, reach_d))
    # the draws reached well into some leaf's own box: the run is not a quiet one
    # (the process draw is not asked: its ball's bound takes || |F| a_L ||_1 with a random F, whose
    # rows cancel at any one state, so no draw comes near it)
    assert reach_v >= 0.9 and reach_n >= 0.9
    if case == 'random8':
        assert reach_e >= 0.9 and reach_d > 0.
    law.close()


def test_the_entry_points_refuse():
    from explicit_hybrid_mpc_amd import _capi, applied, invariance
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    p, n_u = 2, 1
    rng = np.random.default_rng(7)
    synth = es.SynthLaw(es.kuhn_forest(p, 20), n_u, 1, rng, n_sub=3)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    plant = es.random_plant(rng, p, n_u, 1, 'inf', n_d=2)
    guarded = es.random_guarded(rng, p, n_u, 2, 'inf', substeps=2, n_rows=3)
    lib = _capi.load()
    keep = []

    def at(a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    good = state_input_model(np.ones(p), n_u)
    n = law.stats['n_leaf']
    roots = applied.root_cells(law)['vertices']
    nrm, off, _ = invariance.boundary_facets(roots)
    facets = np.ascontiguousarray(np.hstack([nrm, off[:, None]]))
    modes, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)

    def call(core, handle=0, model=good, radii=None, robust=None, with_radii=True, **kw):
        o = dict(n=n, root_vertices=roots.ctypes.data, A=at(plant.A), B=at(plant.B), w=at(plant.w),
                 leaf_mode=modes.ctypes.data, tol_exit=1e-9, n_modes=plant.n_modes, n_d=0, n_g=0)
        o.update(kw)
        r = dict(facets=facets.ctypes.data, n_facets=facets.shape[0], tol_set=1e-9)
        r.update(robust or {})
        desc, data = model.pack()
        q = dict(desc=at(desc, np.int32) if desc.size else None, data=at(data) if data.size else None,
                 x_abs=at(1.1 * np.ones(p)), u_abs=at(np.ones(n_u)), n_terms=desc.shape[0],
                 n_data=data.size, n_x=model.n_x, n_u=model.n_u, n_d=model.n_d, radius_iters=3)
        q.update(radii or {})
        rad = ctypes.byref(_capi.RobustRadii(**q)) if with_radii else None
        st, mg, wo = np.empty(n, np.int32), np.empty(n), np.empty(n, np.int32)
        h = law._handle if handle == 0 else handle
        if core:
            c = _capi.CoreOpts(status=status.ctypes.data, n_status=n, max_edges=1 << 20,
                               tol_side=1e-9, max_fan=4096, rows=1, want_edges=0)
            lv = _capi.CoreLeaves(level=wo.ctypes.data, status=st.ctypes.data)
            res = _capi.CoreResult()
            code = lib.ehm_compiled_robust_core_leaf(
                h, ctypes.byref(_capi.InvarianceOpts(**o)), ctypes.byref(_capi.RobustOpts(**r)),
                rad, ctypes.byref(c), ctypes.byref(res), ctypes.byref(lv))
            return code, lib.ehm_core_last_error()
        lv = _capi.RobustLeaves(status=st.ctypes.data, margin=mg.ctypes.data, worst=wo.ctypes.data)
        res = _capi.RobustResult()
        code = lib.ehm_compiled_robust_successors_leaf(
            h, ctypes.byref(_capi.InvarianceOpts(**o)), ctypes.byref(_capi.RobustOpts(**r)), rad,
            ctypes.byref(res), ctypes.byref(lv), None)
        return code, lib.ehm_robust_last_error()

    bad = _capi.EHM_E_INVALID
    # a model with a process term needs the plant's E; one whose doubles do not fit the LDS cap
    with_d = rr.scaled_model(np.ones(p), n_u, 2)
    padded = np.zeros(9000)
    padded[:good.pack()[1].size] = good.pack()[1]
    off0 = NoiseModel(p, n_u, 0)
    off0.addIndependentTerm('state', lb=0.1 * np.ones(p), ub=0.2 * np.ones(p))
    for core in (False, True):
        assert call(core)[0] == _capi.EHM_OK
        assert call(core, model=with_d, n_d=2, E=at(plant.E))[0] == _capi.EHM_OK
        assert call(core, model=NoiseModel(p, n_u, 0))[0] == _capi.EHM_OK        # no terms: no box
        assert call(core, handle=None)[0] == bad
        assert call(core, with_radii=False)[0] == bad
        assert call(core, A=None)[0] == bad
        assert call(core, leaf_mode=None)[0] == bad
        assert call(core, n_modes=5)[0] == bad
        # the descriptor: the message names the term
        desc, _ = good.pack()
        broken = desc.copy()
        broken[2, 2] = 9                                        # a ball of dimension 9
        code, msg = call(core, radii=dict(desc=at(broken, np.int32)))
        assert code == bad and b'term 2' in msg
        code, msg = call(core, radii=dict(n_terms=17))
        assert code == bad and b'terms' in msg
        assert call(core, radii=dict(desc=None))[0] == bad
        # dimensions that are not the plant's
        for wrong in (dict(n_x=3), dict(n_u=2), dict(n_d=1)):
            code, msg = call(core, radii=wrong)
            assert code == bad and b'does not fit the plant' in msg
        code, msg = call(core, model=with_d, n_d=2)
        assert code == bad and b'no E' in msg
        for iters in (0, 17, -3):
            code, msg = call(core, radii=dict(radius_iters=iters))
            assert code == bad and b'radius_iters' in msg
        for key, size in (('x_abs', p), ('u_abs', n_u)):
            assert call(core, radii={key: None})[0] == bad
            for v in (-1., np.nan, np.inf):
                code, msg = call(core, radii={key: at(v * np.ones(size))})
                assert code == bad and key.encode() in msg
        code, msg = call(core, model=off0)
        assert code == bad and b'constant part' in msg and b'does not hold 0' in msg
        code, msg = call(core, radii=dict(data=at(padded), n_data=padded.size))
        assert code == bad and b'LDS' in msg
    # more than 64 generators cannot be reached under a model (n_d <= 8): n_d itself is refused
    E9 = np.zeros((p, 9))
    nine = NoiseModel(p, n_u, 9)
    code, msg = call(False, model=nine, n_d=9, E=at(E9))
    assert code == bad and b'n_d = 9' in msg
    code, msg = call(False, robust=dict(n_facets=0))
    assert code == bad and b'facets' in msg
    for tol in (-1e-9, np.nan):
        code, msg = call(False, robust=dict(tol_set=tol))
        assert code == bad and b'tol_set' in msg
    assert call(False, chunk=-1)[0] == bad
    # the Python layer
    box = (-np.ones(p), np.ones(p))
    for fn in (law.robust_successors, law.robust_core):
        with pytest.raises(ValueError, match='guarded'):
            fn(plant=guarded, noise=good, radii='leaf')
        with pytest.raises(ValueError, match="'global' or 'leaf'"):
            fn(plant=plant, noise=good, radii='cell')
        with pytest.raises(ValueError, match='noise='):
            fn(plant=plant, radii='leaf')
        with pytest.raises(ValueError, match='no boxes'):
            fn(plant=plant, noise=good, v_box=box, radii='leaf')
        with pytest.raises(ValueError, match='radius_iters'):
            fn(plant=plant, noise=good, radii='leaf', radius_iters=0)
        with pytest.raises(ValueError, match='constant part'):
            fn(plant=plant, noise=off0, radii='leaf')
        with pytest.raises(ValueError, match='does not fit the plant'):
            fn(plant=plant, noise=good, radii='leaf')           # the plant has n_d = 2
    law.close()
