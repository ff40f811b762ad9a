"""
Invariance under measurement and input error on the device (csrc/ehm_robust.hip, the per-mode
generator block of csrc/ehm_core.hip, robust.py): bit for bit against the numpy mirror
(tests/robust_cpu.py), the exact cube cases of tests/test_host_robust.py, soundness against the noisy
rollout independent of the mirror, and the refusals of the two C entry points.
"""

import ctypes

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests import robust_cpu as rb
from tests.robust_cpu import ALL_STAY, NO_ERROR, SOME_EXIT, closed_form, sym
from tests.test_host_core import check_fixed_point

pytestmark = pytest.mark.gpu

ONE_STEP = ('status', 'margin', 'worst')
CORE = ('level', 'status', 'indptr', 'indices')


def _same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _step_against_mirror(res, mir, what=''):
    from explicit_hybrid_mpc_amd import invariance
    for k in ONE_STEP:
        _same(getattr(res, k), getattr(mir, k), what + k)
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


def _box(rng, n, width):
    """A random box with 0 inside; one axis degenerate."""
    lo, hi = -rng.uniform(0., width, n), rng.uniform(0., width, n)
    hi[-1] = lo[-1] = 0.
    return lo, hi


# the shapes of test_gpu_invariance: 100 roots (a sliver of the cube at p = 7, 8: nothing stays) and
# the full forests of p = 2, 3 (a convex set with invariant leaves and levels); two modes, leaves
# without a mode, leaves without a law
@pytest.mark.parametrize('p,n_u,keep', [(2, 1, 100), (3, 2, 100), (7, 1, 100), (8, 4, 100),
                                        (2, 1, None), (3, 2, None)])
def test_both_checks_are_the_mirrors_bit_for_bit(p, n_u, keep, tmp_path):
    from explicit_hybrid_mpc_amd import _capi, compiled
    rng = np.random.default_rng([93, p, n_u])
    synth = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng, n_sub=4)
    plant = es.random_plant(rng, p, n_u, 2, 'inf' if p % 2 else 'quadratic', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    arrays = law.arrays()
    n_leaf = zc.header(arrays)['n_leaf']
    assert 100 < n_leaf < 600
    modes = rng.integers(-1, 2, n_leaf).astype(np.int32)
    assert (modes == -1).any() and (modes == 1).any()
    law.set_leaf_modes(modes)
    boxes = dict(d_box=_box(rng, 2, 1.), v_box=_box(rng, p, 0.05), e_box=_box(rng, n_u, 0.1))
    kw = dict(plant=plant, **boxes)
    res = law.robust_core(rows='all', return_edges=True, **kw)
    mir = rb.core(arrays, modes, plant, rows='all', **boxes)
    _core_against_mirror(res, mir, 'all ')
    check_fixed_point(res)
    one = res.seeds
    assert one.n_generators == 2 + 2 * p + n_u and one.n_facets > p
    width = np.diff(res.indptr)
    print(p, n_u, one, res, 'step %.3g s, slack %.3g s, reach %.3g s, widest row %d' % (
        one.seconds, one.seconds_slack, res.seconds_reach, width.max()))
    assert (width > 1).sum() >= 10 and res.n_edges == width.sum() == res.indices.size
    assert one.counts['no_mode'] > 0 and one.counts['no_cell'] == 0
    assert one.counts['exits'] > 0 and (one.counts['invariant'] > 0) == (keep is None)
    assert one.set_convex == (keep is None) and (res.level > 0).any() == (keep is None)
    assert abs(one.cell_volume_fraction - 1.) <= 1e-12 and not one.holds_on_set
    dead = one.status >= iv.NO_MODE
    assert np.isnan(one.margin[dead]).all() and (one.worst[dead] == -1).all()
    # the one-step call alone, and a subset in the caller's order with a leaf named twice
    alone = law.robust_successors(**kw)
    for k in ONE_STEP:
        _same(getattr(alone, k), getattr(one, k), k)
    pick = np.concatenate([rng.permutation(n_leaf)[:50], [0, n_leaf - 1, 0]]).astype(np.int64)
    part = law.robust_successors(leaves=pick, chunk=16, **kw)
    for k in ONE_STEP:
        _same(getattr(part, k), getattr(one, k)[pick], k)
    assert part.n == pick.size and not part.holds_on_set
    # without v and e boxes: the closed-form test under d alone (2 generators)
    d_only = law.robust_core(plant=plant, d_box=boxes['d_box'], rows='all', return_edges=True)
    _core_against_mirror(d_only, rb.core(arrays, modes, plant, d_box=boxes['d_box'], rows='all',
                                         seeds=None), 'd only ')
    assert d_only.seeds.n_generators == 2
    # chunk 16 against one chunk: every array and both volumes
    few = law.robust_successors(chunk=16, **kw)
    for k in ONE_STEP:
        _same(getattr(few, k), getattr(one, k), 'chunk ' + k)
    assert few.counts == one.counts and few.worst_leaf == one.worst_leaf
    assert few.invariant_volume_fraction == one.invariant_volume_fraction
    assert few.cell_volume_fraction == one.cell_volume_fraction
    # a cap below the widest row: exactly the wider rows are cut off
    fan = int(np.median(width[width > 0]))
    assert 0 < fan < width.max()
    cut = law.robust_core(rows='all', return_edges=True, max_fan=fan, **kw)
    assert np.array_equal(cut.status == 5, width > fan)
    assert cut.counts['unresolved'] == int((width > fan).sum()) > 0
    assert (np.diff(cut.indptr)[width > fan] == 0).all() and (cut.level[width > fan] == 0).all()
    _core_against_mirror(cut, rb.core(arrays, modes, plant, rows='all', max_fan=fan,
                                      seeds=mir.seeds, **boxes), 'cut ')
    # a cap below the total: nothing partial
    with pytest.raises(_capi.EhmError) as err:
        law.robust_core(rows='all', max_edges=res.n_edges - 1, **kw)
    assert err.value.code == _capi.EHM_E_CAPACITY and str(res.n_edges) in str(err.value)
    assert law.robust_core(rows='all', max_edges=res.n_edges, **kw).counts == res.counts
    # the same law after save / load
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    _same_core(loaded.robust_core(rows='all', return_edges=True, **kw), res)
    loaded.close()
    # its single form against the mirror in float arithmetic
    single = law.to_single(flush=True)
    s32 = single.robust_core(rows='all', return_edges=True, **kw)
    _core_against_mirror(s32, rb.core(single.arrays(), modes, plant, rows='all', **boxes),
                         'single ')
    live = ~dead
    assert not np.array_equal(s32.seeds.margin[live], one.margin[live])
    single.close()
    law.close()


def _cube(flat):
    ex = rc.explicit_of(flat)
    law = ex.compile()
    ex.close()
    return law


@pytest.mark.parametrize('p', [2, 3])
def test_the_cube_cases_on_the_device(p):
    flat = iv.cube_law(p, -0.5 * np.eye(p))
    law = _cube(flat)
    arrays = law.arrays()
    plant = iv.identity_plant(p)
    for ab in (ALL_STAY, SOME_EXIT, NO_ERROR):
        a, b = ab
        want = closed_form(flat, arrays, a, b)
        kw = dict(v_box=sym(a, p), e_box=sym(b, p), tol_exit=0., tol_set=0., tol_side=0.)
        res = law.robust_core(plant=plant, return_edges=True, **kw)
        _core_against_mirror(res, rb.core(arrays, None, plant, **kw), str(ab))
        one = res.seeds
        assert one.set_convex and one.n_generators == 3 * p
        assert np.abs(one.margin - want).max() <= 1e-12
        assert np.array_equal(one.status, np.where(want < 0., iv.EXITS, iv.INVARIANT))
        if ab == SOME_EXIT:
            assert 0 < one.counts['exits'] < want.size and not one.holds_on_set
            assert np.array_equal(res.level == 0, want < 0.)
        else:
            assert one.holds_on_set and res.holds and res.core.all() and res.n_sweeps == 0
            assert abs(res.core_volume_fraction - 1.) <= 1e-12
    law.close()


@pytest.mark.parametrize('face', [0., 0.125])
def test_mode_region_on_exactly_the_leaves_within_the_v_box_of_the_face(face):
    p, a = 2, 0.125
    flat = iv.cube_law(p, -0.5 * np.eye(p), modes=lambda C: (C[:, 0] > face).astype(np.int32))
    law = _cube(flat)
    modes = rc.leaf_modes(flat, law.arrays())
    e0 = np.eye(p)[:1]
    plant = iv.identity_plant(p, n_modes=2, regions=[(e0, np.array([face])),
                                                     (-e0, np.array([-face]))])
    res = law.robust_successors(plant=plant, v_box=sym(a, p), tol_exit=0., tol_set=0.)
    x0 = flat.vertices[res.leaf_node][:, :, 0]
    near = np.where(modes == 0, x0.max(axis=1) + a > face, x0.min(axis=1) - a < face)
    assert near.sum() >= 10 and (~near).sum() >= 10
    assert np.array_equal(res.status == iv.MODE_REGION, near)
    assert (res.status[~near] == iv.INVARIANT).all()
    assert not np.isnan(res.margin[near]).any()
    law.close()


def _box_model(p, n_u, n_d, boxes):
    """A NoiseModel whose draws fill exactly the boxes certified."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    m = NoiseModel(p, n_u, n_d)
    for kind, box in boxes.items():
        if box is not None:
            m.addIndependentTerm(kind, box[0], box[1])
    return m


def _random_law_p8(rng):
    """One root simplex of the Kuhn forest (a convex set), 150 bisections, a random affine input, and
    a plant that contracts to the root's centroid by about a fifth (the Kuhn simplex is thin: its
    centroid is 0.16 from the nearest facet)."""
    from explicit_hybrid_mpc_amd import simulate
    p, n_u = 8, 4
    K = 0.05 * rng.uniform(-1., 1., (n_u, p))
    flat = rc.kuhn_tree(p, 1, 150, rng, rc.affine_inputs(K, 0.1 * rng.uniform(-1., 1., n_u)), n_u)
    c = flat.vertices[0].mean(axis=0)
    A = 0.2 * np.eye(p) + 0.005 * rng.uniform(-1., 1., (p, p))
    B = 0.02 * rng.uniform(-1., 1., (p, n_u))
    u_c = K @ c
    w = c - A @ c - B @ u_c
    E = 0.002 * rng.uniform(-1., 1., (p, 2))
    plant = simulate.Plant([A], [B], [w], E, [None], None, None, np.eye(p), np.eye(n_u), 'inf')
    boxes = dict(process=sym(1., 2), state=sym(1e-3, p), input=sym(0.01, n_u))
    return flat, plant, boxes


@pytest.mark.parametrize('case', ['cube2', 'cube3', 'random8'])
def test_no_noisy_trajectory_from_the_core_ever_stops(case):
    """Independent of the mirror: 4 096 trajectories of 50 steps of the noisy rollout, its model
    drawing from exactly the boxes certified, from states sampled in core leaves."""
    rng = np.random.default_rng([71, len(case), int(case[-1])])
    if case == 'random8':
        flat, plant, boxes = _random_law_p8(rng)
    else:
        p = int(case[-1])
        flat, plant = iv.cube_law(p, -0.5 * np.eye(p)), iv.identity_plant(p)
        boxes = dict(process=None, state=sym(ALL_STAY[0], p), input=sym(ALL_STAY[1], p))
    law = _cube(flat)
    p, n_u = law.p, law.n_u
    res = law.robust_core(plant=plant, d_box=boxes['process'], v_box=boxes['state'],
                          e_box=boxes['input'])
    print(case, res.seeds, res)
    assert res.set_convex and res.holds and res.core.sum() >= 10        # else this shows nothing
    V = law.cells().vertices
    k = -(-4096 // int(res.core.sum()))
    X0 = _inside(rng, V[res.core], k)[:4096]
    assert X0.shape[0] == 4096
    model = _box_model(p, n_u, plant.n_d, boxes)
    T = 50
    run = law.rollout(X0, T, plant=plant, noise=model, seed=11)
    assert (run.status == 0).all() and (run.steps == T).all()
    visited = np.searchsorted(law.leaf_node, np.unique(run.leaf))
    assert res.core[visited].all()
    # the draws reached well into the boxes: the test is not about a quiet run
    assert np.abs(run.v[1:]).max() >= 0.9 * np.abs(boxes['state'][1]).max()
    assert np.abs(run.e).max() >= 0.9 * np.abs(boxes['input'][1]).max()
    law.close()


def test_boxes_from_a_noise_model():
    """``noise=``: the boxes are ``bounding_boxes`` at the verified x_abs and the law's u_abs, and
    the call is the call with those boxes."""
    from explicit_hybrid_mpc_amd import noise
    p = 2
    flat = iv.cube_law(p, -0.5 * np.eye(p))
    law = _cube(flat)
    plant = iv.identity_plant(p)
    model = noise.state_input_model(np.ones(p), p)
    res = law.robust_core(plant=plant, noise=model)
    one = res.seeds
    assert np.abs(one.u_abs - 0.5).max() <= 1e-15            # |u| = |x| / 2 on [-1, 1]^2
    assert (one.x_abs > 1.).all() and (one.x_abs < 1.05).all()
    bb = noise.bounding_boxes(model, one.x_abs, one.u_abs)
    assert one.boxes['process'] is None and one.n_generators == 3 * p
    for kind in ('state', 'input'):
        for s in (0, 1):
            _same(one.boxes[kind][s], bb[kind][s])
    again = law.robust_core(plant=plant, v_box=bb['state'], e_box=bb['input'])
    _same(again.level, res.level)
    _same(again.seeds.margin, one.margin)
    # about 3 % of state error and 0.03 of input error: 1/2 + 2 (0.03) + 0.03 < 1 everywhere
    assert res.holds and res.core.all() and one.holds_on_set and one.worst_margin > 0.35
    X0 = _inside(np.random.default_rng(5), law.cells().vertices[res.core], 4)
    run = law.rollout(X0, 50, plant=plant, noise=model, seed=3)
    assert (run.status == 0).all()
    assert res.core[np.searchsorted(law.leaf_node, np.unique(run.leaf))].all()
    law.close()


def test_the_entry_points_refuse():
    from explicit_hybrid_mpc_amd import _capi, applied, explicit, invariance, partition
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

    def at(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data

    def call(law_, plant_, core, handle=0, robust=None, **kw):
        n = law_.stats['n_leaf']
        if law_.stats['n_test'] > 0:            # refused before anything is read
            roots = np.zeros((law_.stats['n_roots'], law_.p + 1, law_.p))
            facets = np.zeros((3, law_.p + 1))
        else:
            roots = applied.root_cells(law_)['vertices']
            nrm, off, _ = invariance.boundary_facets(roots)
            facets = np.ascontiguousarray(np.hstack([nrm, off[:, None]]))
        modes, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        o = dict(n=n, root_vertices=roots.ctypes.data, A=at(plant_.A), B=at(plant_.B),
                 w=at(plant_.w), leaf_mode=modes.ctypes.data, tol_exit=1e-9,
                 n_modes=plant_.n_modes, n_d=0, n_g=0)
        o.update(kw)
        r = dict(facets=facets.ctypes.data, n_facets=facets.shape[0], tol_set=1e-9)
        r.update(robust or {})
        st, mg, wo = np.empty(n, np.int32), np.empty(n), np.empty(n, np.int32)
        if core:
            c = _capi.CoreOpts(status=status.ctypes.data, n_status=n, max_edges=1 << 20,
                               tol_side=1e-9, max_fan=4096, rows=1, want_edges=0)
            lv = _capi.CoreLeaves(level=wo.ctypes.data, status=st.ctypes.data)
            res = _capi.CoreResult()
            code = lib.ehm_compiled_robust_core(
                law_._handle if handle == 0 else handle, ctypes.byref(_capi.InvarianceOpts(**o)),
                ctypes.byref(_capi.RobustOpts(**r)), ctypes.byref(c), ctypes.byref(res),
                ctypes.byref(lv))
            return code, lib.ehm_core_last_error()
        lv = _capi.RobustLeaves(status=st.ctypes.data, margin=mg.ctypes.data, worst=wo.ctypes.data)
        res = _capi.RobustResult()
        code = lib.ehm_compiled_robust_successors(
            law_._handle if handle == 0 else handle, ctypes.byref(_capi.InvarianceOpts(**o)),
            ctypes.byref(_capi.RobustOpts(**r)), ctypes.byref(res), ctypes.byref(lv))
        return code, lib.ehm_robust_last_error()

    bad = _capi.EHM_E_INVALID
    zero, one = np.zeros(p), np.ones(p)
    v_ok = dict(v_lo=at(-0.1 * one), v_hi=at(0.1 * one))
    for core in (False, True):
        assert call(law, plant, core)[0] == _capi.EHM_OK
        assert call(law, plant, core, robust=v_ok)[0] == _capi.EHM_OK
        assert call(law, plant, core, handle=None)[0] == bad
        assert call(law, plant, core, A=None)[0] == bad
        assert call(law, plant, core, leaf_mode=None)[0] == bad
        assert call(law, plant, core, n_modes=5)[0] == bad
        # a v or e box without 0, with one bound missing, upside down, not finite
        code, msg = call(law, plant, core, robust=dict(v_lo=at(0.1 * one), v_hi=at(one)))
        assert code == bad and b'does not hold 0' in msg and b'v box' in msg
        code, msg = call(law, plant, core, robust=dict(e_lo=at([-1.]), e_hi=at([-0.5])))
        assert code == bad and b'does not hold 0' in msg and b'e box' in msg
        code, msg = call(law, plant, core, robust=dict(v_lo=at(-one)))
        assert code == bad and b'one bound NULL' in msg
        code, msg = call(law, plant, core, robust=dict(v_lo=at(-one), v_hi=at([1., np.inf])))
        assert code == bad and b'generator' in msg
        code, msg = call(law, plant, core, robust=dict(e_lo=at([-np.inf]), e_hi=at([0.])))
        assert code == bad and b'generator' in msg
        lo, hi = np.array([0., 1.]), np.array([1., 0.5])
        code, msg = call(law, plant, core, n_d=2, E=at(plant.E), d_lo=at(lo), d_hi=at(hi))
        assert code == bad and b'axis 1' in msg
        code, msg = call(law, plant, core, n_d=2, d_lo=at(lo), d_hi=at(hi))
        assert code == bad and b'no E' in msg
        # more than 64 generators: n_d + 2 p + n_u = 60 + 4 + 1 with both boxes; 64 with v alone
        E60 = np.zeros((p, 60))
        d60 = dict(n_d=60, E=at(E60), d_lo=at(-np.ones(60)), d_hi=at(np.ones(60)))
        code, msg = call(law, plant, core, robust=dict(v_ok, e_lo=at([-0.1]), e_hi=at([0.1])),
                         **d60)
        assert code == bad and b'n_g = 65' in msg and b'64' in msg
        assert call(law, plant, core, robust=v_ok, **d60)[0] == _capi.EHM_OK
        assert call(law, plant, core, **d60)[0] == _capi.EHM_OK
    # the facets: the one-step test needs them, the core does not read them
    code, msg = call(law, plant, False, robust=dict(n_facets=0))
    assert code == bad and b'facets' in msg
    assert call(law, plant, False, robust=dict(facets=None))[0] == bad
    assert call(law, plant, True, robust=dict(facets=None, n_facets=0))[0] == _capi.EHM_OK
    for tol in (-1e-9, np.nan):
        code, msg = call(law, plant, False, robust=dict(tol_set=tol))
        assert code == bad and b'tol_set' in msg
    assert call(law, plant, False, chunk=-1)[0] == bad
    with pytest.raises(ValueError, match='guarded'):
        law.robust_successors(plant=guarded, v_box=sym(0.1, p))
    with pytest.raises(ValueError, match='guarded'):
        law.robust_core(plant=guarded, v_box=sym(0.1, p))
    law.close()
    # a law with test nodes: the default compile of a nested tree
    from tests.test_gpu_audit import _oracle
    orc, Vs = _oracle('di')
    root, _ = partition.partition_set(orc, Vs)
    nested = explicit.ExplicitMPC(root, orc)
    with_tests = nested.compile()
    assert with_tests.stats['n_test'] > 0
    for fn in (with_tests.robust_successors, with_tests.robust_core):
        with pytest.raises(_capi.EhmError) as err:
            fn(v_box=sym(0.01, 2))
        assert err.value.code == bad and 'test nodes' in str(err.value)
    di = es.random_plant(rng, 2, with_tests.n_u, 1, 'inf')
    for core in (False, True):
        code, msg = call(with_tests, di, core)
        assert code == bad and b'test nodes' in msg
    as_roots = nested.compile(spine='roots')
    ok = as_roots.robust_core(v_box=sym(1e-3, 2), e_box=sym(1e-3, as_roots.n_u))
    assert sum(ok.counts.values()) == as_roots.stats['n_leaf'] and ok.counts['no_cell'] == 0
    via = nested.robust_core(v_box=sym(1e-3, 2), e_box=sym(1e-3, as_roots.n_u))
    assert via.counts == ok.counts
    _same(via.level, ok.level)
    one = nested.robust_successors(v_box=sym(1e-3, 2), e_box=sym(1e-3, as_roots.n_u))
    _same(one.status, ok.seeds.status)
    print('di:', ok.seeds, ok)
    for l in (with_tests, as_roots):
        l.close()
    nested.close()
