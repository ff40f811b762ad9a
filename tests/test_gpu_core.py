"""
The may-reach relation between a compiled law's leaves and the invariant core on the device
(csrc/ehm_core.hip, invariance.py): bit for bit against the numpy mirror
(tests/core_cpu.py), soundness of the rows against the evaluator, the exact cube cases of
tests/test_host_core.py, agreement with ``CompiledLaw.rollout`` from core leaves,
``CoreResult.contains``, and the refusals of the C entry point.
"""

import ctypes

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import core_cpu as kc
from tests import explicit_synth as es
from tests import invariance_cpu as iv
from tests import reduce_cpu as rc
from tests.test_host_core import check_fixed_point, largest_coordinate, two_mode_case
from tests.test_host_invariance import cube_cases

pytestmark = pytest.mark.gpu


def _same(got, want, what=''):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _against_mirror(res, mir, what=''):
    for k in ('level', 'status', 'indptr', 'indices'):
        _same(getattr(res, k), getattr(mir, k), what + k)
    assert res.counts == mir.counts, what
    assert res.n_sweeps == mir.n_sweeps and res.n_edges == mir.n_edges, what
    assert np.array_equal(res.core, mir.core)


def _same_result(a, b):
    for k in ('level', 'status', 'indptr', 'indices'):
        _same(getattr(a, k), getattr(b, k), k)
    assert a.counts == b.counts and a.n_sweeps == b.n_sweeps and a.n_edges == b.n_edges
    assert a.core_volume_fraction == b.core_volume_fraction
    assert a.cell_volume_fraction == b.cell_volume_fraction


def _inside(rng, V, k, floor=1e-3):
    """k points per cell of V [n, p+1, p] with every weight >= floor."""
    n, nv, p = V.shape
    w = floor + (1. - nv * floor) * rng.dirichlet(np.ones(nv), (n, k))
    return np.einsum('nkv,nvc->nkc', w, V).reshape(-1, p)


# the shapes of test_gpu_invariance: 100 roots (the narrow node record at p <= 6, the wide one at
# p = 7, 8; the serial scan over few roots) and the full forests of p = 2 (128 roots) and p = 3 (384)
@pytest.mark.parametrize('p,n_u,keep', [(2, 1, 100), (3, 2, 100), (7, 1, 100), (8, 4, 100),
                                        (2, 1, None), (3, 2, None)])
def test_the_core_is_the_mirrors_bit_for_bit(p, n_u, keep, tmp_path):
    from explicit_hybrid_mpc_amd import _capi, compiled
    rng = np.random.default_rng([91, p, n_u, 0 if keep is None else keep])
    synth = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng, n_sub=12)
    plant = es.random_plant(rng, p, n_u, 2, 'inf' if p % 2 else 'quadratic', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    arrays = law.arrays()
    n_leaf = zc.header(arrays)['n_leaf']
    modes = rng.integers(-1, 2, n_leaf).astype(np.int32)
    law.set_leaf_modes(modes)
    lo = rng.uniform(-1., 0., 2)
    hi = lo + rng.uniform(0.1, 1., 2)
    hi[1] = lo[1]                                           # one degenerate axis
    box = (lo, hi)
    seeds = iv.successors(arrays, modes, plant, d_box=box)
    nominal = iv.successors(arrays, modes, plant)
    res = law.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True)
    mir = kc.core(arrays, modes, plant, d_box=box, rows='all', seeds=seeds, nominal=nominal)
    _against_mirror(res, mir, 'all ')
    _same(res.seeds.status, seeds.status)
    check_fixed_point(res)
    width = np.diff(res.indptr)
    print(p, n_u, keep, res, 'reach %.3g s, sweeps %.3g s, widest row %d' % (
        res.seconds_reach, res.seconds_sweeps, width.max()))
    assert (width > 1).sum() >= 20 and res.n_edges == width.sum() == res.indices.size
    assert res.indices.min() >= 0 and res.indices.max() < n_leaf
    assert (width[res.seeds.status >= iv.NO_MODE] == 0).all()
    assert res.counts['unresolved'] == 0 and res.counts['no_mode'] > 0
    assert abs(res.cell_volume_fraction - 1.) <= 1e-12
    assert not res.holds or res.core.any()
    bare = law.invariant_core(plant=plant, d_box=box, rows='all')
    assert bare.indptr is None and bare.indices is None and bare.counts == res.counts
    _same(bare.level, res.level)
    if p <= 3:
        inv = law.invariant_core(plant=plant, d_box=box, return_edges=True)
        _against_mirror(inv, kc.core(arrays, modes, plant, d_box=box, seeds=seeds,
                                     nominal=nominal), 'invariant ')
        _same(inv.level, res.level)                         # the rows of seeds change no level
        assert 0 < inv.n_edges < res.n_edges
    # the nominal successor: no box, no E term
    nom = law.invariant_core(plant=plant, rows='all', return_edges=True)
    _against_mirror(nom, kc.core(arrays, modes, plant, rows='all', seeds=nominal,
                                 nominal=nominal), 'nominal ')
    # a cap below the widest row: exactly the wider rows are cut off
    fan = int(np.median(width[width > 0]))
    assert 0 < fan < width.max()
    cut = law.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True, max_fan=fan)
    assert np.array_equal(cut.status == kc.UNRESOLVED, width > fan)
    assert cut.counts['unresolved'] == int((width > fan).sum()) > 0
    assert (np.diff(cut.indptr)[width > fan] == 0).all() and (cut.level[width > fan] == 0).all()
    _against_mirror(cut, kc.core(arrays, modes, plant, d_box=box, rows='all', seeds=seeds,
                                 nominal=nominal, max_fan=fan), 'cut ')
    # a cap below the total: nothing partial
    with pytest.raises(_capi.EhmError) as err:
        law.invariant_core(plant=plant, d_box=box, rows='all', max_edges=res.n_edges - 1)
    assert err.value.code == _capi.EHM_E_CAPACITY and str(res.n_edges) in str(err.value)
    assert law.invariant_core(plant=plant, d_box=box, rows='all',
                              max_edges=res.n_edges).counts == res.counts
    # the same law after save / load
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    _same_result(loaded.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True), res)
    loaded.close()
    # its single form against the mirror in float arithmetic
    single = law.to_single(flush=True)
    a32 = single.arrays()
    s32 = single.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True)
    _against_mirror(s32, kc.core(a32, modes, plant, d_box=box, rows='all'), 'single ')
    assert s32.n_edges >= 0.5 * res.n_edges
    single.close()
    law.close()


def _held(roots, Z):
    """bool [n]: some root holds Z[i] (barycentric weights in float64, all >= 0)."""
    E = np.transpose(roots[:, 1:] - roots[:, :1], (0, 2, 1))
    Minv = np.linalg.inv(E)
    out = np.zeros(Z.shape[0], dtype=bool)
    for s in range(0, Z.shape[0], 4096):
        al = np.einsum('rqc,nrc->nrq', Minv, Z[s:s + 4096, None, :] - roots[None, :, 0, :])
        out[s:s + 4096] = ((al >= 0.).all(axis=2) & (1. - al.sum(axis=2) >= 0.)).any(axis=1)
    return out


@pytest.mark.parametrize('p,n_u,keep', [(2, 1, None), (3, 2, None), (8, 4, 100)])
def test_a_row_holds_every_leaf_the_evaluator_returns(p, n_u, keep):
    """Independent of the mirror: successors of points strictly inside a leaf's cell, under a
    disturbance of the box, are evaluated by the law; every one some root holds lands in a leaf
    of the row."""
    from explicit_hybrid_mpc_amd import applied
    rng = np.random.default_rng([91, p, n_u, 0 if keep is None else keep])
    synth = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng, n_sub=12)
    plant = es.random_plant(rng, p, n_u, 2, 'inf' if p % 2 else 'quadratic', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    n_leaf = law.stats['n_leaf']
    modes = rng.integers(-1, 2, n_leaf).astype(np.int32)
    law.set_leaf_modes(modes)
    lo = rng.uniform(-1., 0., 2)
    hi = lo + rng.uniform(0.1, 1., 2)
    box = (lo, hi)
    res = law.invariant_core(plant=plant, d_box=box, rows='all', return_edges=True)
    width = np.diff(res.indptr)
    cells = law.cells()
    live = (modes >= 0) & np.isfinite(law.evaluate(cells.vertices.mean(axis=1))).all(axis=1)
    rows = np.nonzero(live)[0]                  # every leaf with a row (it may be empty)
    assert rows.size >= 100 and (width[~live] == 0).all()
    if p <= 3:
        assert (res.status[rows] == iv.INVARIANT).mean() >= 0.5
    k = 32
    X = _inside(rng, cells.vertices[rows], k)
    U, leaf, _, _ = law.evaluate(X, return_info=True)
    assert np.array_equal(leaf, np.repeat(law.leaf_node[rows], k))
    D = rng.uniform(lo, hi, (X.shape[0], 2))
    Z = es.nominal_step(plant, X, U, np.repeat(modes[rows], k), D)
    held = _held(applied.root_cells(law)['vertices'], Z)
    to = np.searchsorted(law.leaf_node, law.evaluate(Z, return_info=True)[1])
    print(p, 'leaves %d, successors %d, held by a root %d' % (rows.size, Z.shape[0], held.sum()))
    assert held.sum() >= (0.5 if p <= 3 else 0.) * held.size
    src = np.repeat(rows, k)
    for q in np.nonzero(held)[0]:
        l = src[q]
        assert to[q] in res.indices[res.indptr[l]:res.indptr[l + 1]], (l, to[q])
    law.close()


def _cube(flat):
    ex = rc.explicit_of(flat)
    law = ex.compile()
    ex.close()
    return law


@pytest.mark.parametrize('p', [2, 3])
def test_the_cube_cases_on_the_device(p):
    for name, K, E, d_box, scale, reach in cube_cases(p):
        flat = iv.cube_law(p, K)
        law = _cube(flat)
        plant = iv.identity_plant(p, E=E)
        res = law.invariant_core(plant=plant, d_box=d_box, tol_exit=0., tol_side=0.,
                                 return_edges=True)
        _against_mirror(res, kc.core(law.arrays(), None, plant, d_box=d_box, tol_exit=0.,
                                     tol_side=0.), name)
        M = largest_coordinate(flat.vertices[law.leaf_node])
        assert res.set_convex
        if name in ('contraction', 'contraction_quarter_box'):
            assert res.core.all() and res.n_sweeps == 0 and res.holds
            assert abs(res.core_volume_fraction - 1.) <= 1e-12
        else:
            assert not res.core.any() and not res.holds and res.core_volume_fraction == 0.
        if name == 'expansion':
            safe = np.array([next(k for k in range(64) if 2. ** (k + 1) * m > 1.) for m in M])
            assert (res.level <= safe).all() and np.array_equal(res.level == 0, M > 0.5)
        if name == 'contraction_box':
            assert np.array_equal(res.level == 0, M > 0.75)
        law.close()


@pytest.mark.parametrize('p', [2, 3])
def test_two_modes_on_the_device_and_the_rollout_from_the_core(p):
    rng = np.random.default_rng([61, p])
    flat, plant = two_mode_case(p)
    law = _cube(flat)
    res = law.invariant_core(plant=plant, tol_exit=0., tol_side=0., return_edges=True)
    modes = rc.leaf_modes(flat, law.arrays())
    _against_mirror(res, kc.core(law.arrays(), modes, plant, tol_exit=0., tol_side=0.))
    V = flat.vertices[law.leaf_node]
    inner = largest_coordinate(V) <= 0.5
    assert np.array_equal(res.core, inner) and res.n_sweeps == 1 and res.holds
    # volumes are rounded determinants over p!, summed: a few units in the last place each
    assert abs(res.core_volume_fraction - 2. ** -p) <= 1e-12
    X0 = _inside(rng, V[res.core], 4)
    run = law.rollout(X0, 50, plant=plant)
    assert (run.status == 0).all() and (run.steps == 50).all()
    # contains: the leaf the law evaluates the state in
    X = np.concatenate([_inside(rng, V, 2), rng.uniform(-1., 1., (500, p))])
    row = np.searchsorted(law.leaf_node, law.evaluate(X, return_info=True)[1])
    got = res.contains(X)
    assert np.array_equal(got, res.core[row])
    assert np.array_equal(got[:2 * V.shape[0]], np.repeat(res.core, 2))
    assert np.array_equal(got[2 * V.shape[0]:], (np.abs(X[2 * V.shape[0]:]) < 0.5).all(axis=1))
    law.close()
    with pytest.raises(ValueError, match='contains'):
        res.contains(X)


@pytest.mark.parametrize('p,n_u,seed', [(2, 1, 3), (3, 2, 1)])
def test_agreement_with_the_rollout(p, n_u, seed):
    """No trajectory from a core leaf ever stops: 50 steps under a fresh disturbance of the box
    each.  The seeds were chosen on the numpy mirror for a core that is neither empty nor
    everything."""
    rng = np.random.default_rng([83, p, seed])
    synth = es.SynthLaw(es.kuhn_forest(p), n_u, 2, rng, n_sub=12, no_law=0.)
    plant = es.random_plant(rng, p, n_u, 2, 'inf', n_d=2)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    cells = law.cells()
    n = len(cells)
    in_one = es.in_region(plant, cells.vertices.reshape(-1, p), np.ones(n * (p + 1), dtype=int),
                          0.).reshape(n, p + 1).all(axis=1)
    law.set_leaf_modes(in_one.astype(np.int32))
    half = rng.uniform(0.5, 2., 2)
    res = law.invariant_core(plant=plant, d_box=(-half, half))
    print(p, res)
    assert res.set_convex and res.holds
    assert res.core.sum() >= 10 and (~res.core).sum() >= 10
    assert 0. < res.core_volume_fraction < 1.
    T = 50
    X0 = _inside(rng, cells.vertices[res.core], 8)
    d = rng.uniform(-half, half, (T, X0.shape[0], 2))
    run = law.rollout(X0, T, d=d, plant=plant)
    assert (run.status == 0).all() and (run.steps == T).all()
    assert np.array_equal(run.leaf[0], np.repeat(law.leaf_node[res.core], 8))
    # every leaf the trajectories visit is a core leaf
    visited = np.searchsorted(law.leaf_node, np.unique(run.leaf))
    assert res.core[visited].all()
    assert res.contains(X0).all()
    law.close()


def test_the_entry_point_refuses():
    from explicit_hybrid_mpc_amd import _capi, applied, explicit, partition
    p, n_u = 2, 1
    rng = np.random.default_rng(7)
    synth = es.SynthLaw(es.kuhn_forest(p, 20), n_u, 1, rng, n_sub=3)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    plant = es.random_plant(rng, p, n_u, 1, 'inf', n_d=2)
    guarded = es.random_guarded(rng, p, n_u, 2, 'inf', substeps=2, n_rows=3)
    n_leaf = law.stats['n_leaf']
    lib = _capi.load()

    def call(law_, plant_, handle=0, core=None, outputs=None, **kw):
        n = law_.stats['n_leaf']
        if law_.stats['n_test'] > 0:            # refused before anything is read
            roots = np.zeros((law_.stats['n_roots'], law_.p + 1, law_.p))
        else:
            roots = applied.root_cells(law_)['vertices']
        modes, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        A, B, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (plant_.A, plant_.B,
                                                                       plant_.w))
        o = dict(n=0, root_vertices=roots.ctypes.data, A=A.ctypes.data, B=B.ctypes.data,
                 w=w.ctypes.data, leaf_mode=modes.ctypes.data, tol_exit=1e-9,
                 n_modes=plant_.n_modes, n_d=0, n_g=0)
        o.update(kw)
        c = dict(status=status.ctypes.data, n_status=n, max_edges=1 << 20, tol_side=1e-9,
                 max_fan=4096, rows=1, want_edges=0)
        c.update(core or {})
        level, out = np.empty(n, np.int32), np.empty(n, np.int32)
        lv = _capi.CoreLeaves(level=level.ctypes.data, status=out.ctypes.data)
        indptr, got = np.empty(n + 1, np.int64), ctypes.c_void_p(None)
        edges = outputs is not None and c['want_edges']
        if edges:                               # the outputs of want_edges; `outputs` takes them
            lv.indptr, lv.indices_out = indptr.ctypes.data, ctypes.addressof(got)
        res = _capi.CoreResult()
        rc_ = lib.ehm_compiled_core(law_._handle if handle == 0 else handle,
                                    ctypes.byref(_capi.InvarianceOpts(**o)),
                                    ctypes.byref(_capi.CoreOpts(**c)), ctypes.byref(res),
                                    ctypes.byref(lv))
        if outputs is not None:
            outputs.update(status=out)
        if edges:
            indices = np.empty(res.n_edges if got.value else 0, np.int32)
            if indices.size:
                ctypes.memmove(indices.ctypes.data, got.value, indices.nbytes)
            if got.value:
                lib.ehm_host_free(got)
            outputs.update(indptr=indptr, indices=indices)
        return rc_, lib.ehm_core_last_error(), level, res

    code, _, level, res = call(law, plant)
    assert code == _capi.EHM_OK
    # all leaves called invariant: nothing is a seed, everything is core
    assert (level == -1).all() and res.counts[0] == n_leaf and res.n_sweeps == 0
    code, msg, _, _ = call(law, plant, core=dict(n_status=n_leaf - 1))
    assert code == _capi.EHM_E_INVALID and b'status array' in msg
    bad = np.zeros(n_leaf, dtype=np.int32)
    bad[3] = 5
    code, msg, _, _ = call(law, plant, core=dict(status=bad.ctypes.data))
    assert code == _capi.EHM_E_INVALID and b'status[3]' in msg
    for tol in (-1e-9, np.nan):
        code, msg, _, _ = call(law, plant, core=dict(tol_side=tol))
        assert code == _capi.EHM_E_INVALID and b'tol_side' in msg
    assert call(law, plant, core=dict(max_fan=0))[0] == _capi.EHM_E_INVALID
    assert call(law, plant, core=dict(max_edges=1 << 31))[0] == _capi.EHM_E_INVALID
    assert call(law, plant, core=dict(rows=2))[0] == _capi.EHM_E_INVALID
    assert call(law, plant, core=dict(want_edges=1))[0] == _capi.EHM_E_INVALID     # no outputs
    assert call(law, plant, handle=None)[0] == _capi.EHM_E_INVALID
    assert call(law, plant, A=None)[0] == _capi.EHM_E_INVALID
    assert call(law, plant, leaf_mode=None)[0] == _capi.EHM_E_INVALID
    assert call(law, plant, n_modes=5)[0] == _capi.EHM_E_INVALID
    # the chunk of the count pass: several chunks (every one after the first starts at a leaf
    # other than 0 and writes its volumes behind the earlier ones') give what one chunk gives, bit
    # for bit; on the whole square, which the plant's contraction maps into itself
    ex = es.SynthLaw(es.kuhn_forest(p), n_u, 1, rng, n_sub=3).explicit()
    whole = ex.compile()
    ex.close()
    n_whole = whole.stats['n_leaf']
    assert n_whole > 2 * 16
    mixed = (np.arange(n_whole) % 3 == 0).astype(np.int32)      # some seeds, so levels differ
    for want in (0, 1):
        runs = []
        for chunk in (16, 0):
            e = {}
            code, _, level, res = call(whole, plant, chunk=chunk, outputs=e,
                                       core=dict(status=mixed.ctypes.data, want_edges=want))
            assert code == _capi.EHM_OK
            runs.append(dict(e, level=level, counts=np.array(res.counts[:]),
                             volumes=np.array([res.core_volume, res.cell_volume]),
                             n_edges=np.array([res.n_edges])))
        assert sorted(runs[0]) == sorted(runs[1]) and ('indices' in runs[0]) == bool(want)
        assert 'status' in runs[0]
        for k in runs[0]:
            _same(runs[0][k], runs[1][k], 'chunk 16 against 0: ' + k)
        print('chunks:', n_whole, 'leaves,', runs[0]['n_edges'][0], 'edges, levels up to',
              runs[0]['level'].max(), 'volumes', runs[0]['volumes'])
        assert runs[0]['n_edges'][0] > 0 and runs[0]['volumes'][0] < runs[0]['volumes'][1]
    code, msg, _, _ = call(whole, plant, chunk=-1)
    assert code == _capi.EHM_E_INVALID and b'chunk' in msg
    whole.close()
    lo, hi = np.array([0., 1.]), np.array([1., 0.5])
    E = np.ascontiguousarray(plant.E)
    code, msg, _, _ = call(law, plant, n_d=2, E=E.ctypes.data, d_lo=lo.ctypes.data,
                           d_hi=hi.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'axis 1' in msg
    code, msg, _, _ = call(law, plant, n_d=2, d_lo=lo.ctypes.data, d_hi=hi.ctypes.data)
    assert code == _capi.EHM_E_INVALID and b'no E' in msg
    with pytest.raises(ValueError, match='guarded'):
        law.invariant_core(plant=guarded)
    law.close()
    # a law with test nodes: the default compile of a nested tree
    from tests.test_gpu_audit import _oracle
    orc, Vs = _oracle('di')
    root, _ = partition.partition_set(orc, Vs)
    nested = explicit.ExplicitMPC(root, orc)
    with_tests = nested.compile()
    assert with_tests.stats['n_test'] > 0
    with pytest.raises(_capi.EhmError) as err:
        with_tests.invariant_core()
    assert err.value.code == _capi.EHM_E_INVALID and 'test nodes' in str(err.value)
    di = es.random_plant(rng, 2, with_tests.n_u, 1, 'inf')
    code, msg, _, _ = call(with_tests, di)
    assert code == _capi.EHM_E_INVALID and b'core: the law has' in msg and b'test nodes' in msg
    as_roots = nested.compile(spine='roots')
    ok = as_roots.invariant_core()
    assert sum(ok.counts.values()) == as_roots.stats['n_leaf'] and ok.counts['no_cell'] == 0
    via = nested.invariant_core()
    assert via.counts == ok.counts
    _same(via.level, ok.level)
    print('di:', ok)
    for l in (with_tests, as_roots):
        l.close()
    nested.close()
    orc.close()
