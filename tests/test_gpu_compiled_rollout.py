"""
The compiled law in closed loop on the device (CompiledLaw.rollout, k_compiled_rollout<P, NU, KIND>,
DESIGN.md 3.8c): every instantiation (8 x 4 x 3 = 96, one test id each) bit for bit against the
numpy mirror on the exported arrays (tests/compiled_rollout_cpu) and against exact arithmetic
(``check_exact``: the plane path, the exact leaf where decisive, |u - u_exact| <= u_tol with
c = 64, the exit test on the exact root weights with slack 64 eps (1 + kappa)); every status; the
applied steps against ``CompiledLaw.evaluate``; the edges; the refusals; and a real partition
against ``ExplicitMPC.rollout`` and under ``simulate.compare``.
"""

import types

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled, simulate
from tests import compiled_cpu as cc
from tests import compiled_rollout_cpu as cr
from tests import explicit_synth as es
from tests import helpers

pytestmark = pytest.mark.gpu

XP, MAX_NU = 8, 4
CASES = [(kind, p, nu) for kind in cr.KINDS for p in range(1, XP + 1)
         for nu in range(1, MAX_NU + 1)]
assert len(CASES) == 96
T = cr.T_STEPS
STATUS_SEEN = {kind: set() for kind in cr.KINDS}
STATUS_CAN = {'nominal': {0, 1, 2, 3}, 'noisy': {0, 1, 2, 3}, 'guarded': {0, 1, 3}}
OUTPUTS = ('x_final', 'steps', 'status', 'cost', 'u_norm_sum', 'max_violation')


def _compile(law):
    """The compiled law of a SynthLaw; its source is closed before anything is rolled out."""
    ex = law.explicit()
    cl = ex.compile()
    ex.close()
    return cl


def _run_case(kind, p, n_u, exact=True):
    law, plant, X0, kw = cr.case(kind, p, n_u)
    cl = _compile(law)
    arrays = cl.arrays()
    assert np.array_equal(cl.leaf_mode, cr.leaf_modes(law, arrays))
    res = cl.rollout(X0, T, plant=plant, **kw)
    mir = cr.mirror(arrays, cl.leaf_mode, plant, X0, T, **kw)
    cr.assert_same(res, mir)
    if exact:
        cr.check_exact(law, res, mir.roots, mir.z, plant, cl.leaf_mode, kw['tol_exit'])
    bare = cl.rollout(X0, T, plant=plant, record=False, **kw)
    for f in OUTPUTS:
        assert np.array_equal(getattr(bare, f), getattr(res, f)), f
    assert bare.x is None and bare.u is None and bare.leaf is None and bare.v is None
    assert res.commutation is None
    assert (res.mode is None) == plant.guarded
    STATUS_SEEN[kind].update(int(s) for s in np.unique(res.status))
    return law, plant, cl, res, mir, kw


@pytest.mark.parametrize('kind,p,n_u', CASES, ids=['%s-p%d-nu%d' % c for c in CASES])
def test_rollout_instantiation(kind, p, n_u):
    law, plant, cl, res, mir, _ = _run_case(kind, p, n_u)
    assert (res.steps > 0).any()
    if not plant.guarded:
        live = res.leaf >= 0
        modes = cr.plant_modes(cl.leaf_mode, plant, cl.leaf_mode.size)
        by_node = dict(zip(cl.leaf_node.tolist(), modes.tolist()))
        assert np.array_equal(res.mode[live], [by_node[k] for k in res.leaf[live].tolist()])
        assert (res.mode[~live] == -1).all()
    cl.close()


def test_every_status_code_occurs():
    """Each status the plant kind can produce occurs in the sweep (cases not run yet run here)."""
    for kind, p, n_u in CASES:
        if STATUS_SEEN[kind] >= STATUS_CAN[kind]:
            continue
        _run_case(kind, p, n_u, exact=False)[2].close()
    for kind in cr.KINDS:
        assert STATUS_SEEN[kind] >= STATUS_CAN[kind], (kind, STATUS_SEEN[kind])


@pytest.mark.parametrize('kind,p,n_u', [('nominal', 4, 2), ('noisy', 3, 3)])
def test_applied_steps_are_evaluate(kind, p, n_u):
    """At every applied step (leaf, u) is CompiledLaw.evaluate(z_t), bit for bit."""
    law, plant, cl, res, mir, kw = _run_case(kind, p, n_u, exact=False)
    applied = 0
    for t in range(T):
        on = np.nonzero(res.steps > t)[0]
        if on.size == 0:
            continue
        v_t = res.v[t, on] if kind == 'noisy' else kw['v'][t, on]
        z = res.x[t, on] + v_t if t > 0 else res.x[t, on]
        assert np.array_equal(z, mir.z[t, on])
        u, leaf, _, _ = cl.evaluate(z, return_info=True)
        assert np.array_equal(u, res.u[t, on]) and np.array_equal(leaf, res.leaf[t, on])
        applied += on.size
    assert applied > cr.N_TRAJ
    cl.close()


def test_batch_edges_and_exit_tolerance():
    """n = 0, 1 and 257 (a partial block), tol_exit = 0, T = 0, a NaN initial state."""
    law, plant, X0, kw = cr.case('nominal', 3, 2)
    cl = _compile(law)
    arrays = cl.arrays()
    rng = np.random.default_rng(7)
    X = np.concatenate([X0, law.states(rng, 64)])[:257]
    assert X.shape[0] == 257
    for n in (0, 1, 257):
        for tol in (0., 1e-9):
            kw2 = dict(tol_exit=tol, v=rng.normal(size=(T, n, 3)) * 1e-3)
            res = cl.rollout(X[:n], T, plant=plant, **kw2)
            assert res.x_final.shape == (n, 3) and res.steps.shape == (n,)
            mir = cr.mirror(arrays, cl.leaf_mode, plant, X[:n], T, **kw2)
            cr.assert_same(res, mir)
            if n:
                cr.check_exact(law, res, mir.roots, mir.z, plant, cl.leaf_mode, tol)
    res = cl.rollout(X, 0, plant=plant)
    assert np.array_equal(res.x_final, X) and (res.steps == 0).all() and (res.status == 0).all()
    assert (res.cost == 0).all() and (res.u_norm_sum == 0).all()
    assert np.all(res.max_violation == -np.inf)
    assert res.x.shape == (1, 257, 3) and np.array_equal(res.x[0], X)
    Xn = X[:5].copy()
    Xn[1, 2] = np.nan
    Xn[3] = np.nan
    res = cl.rollout(Xn, 4, plant=plant)
    assert (res.status[[1, 3]] == 1).all() and (res.steps[[1, 3]] == 0).all()
    cr.assert_same(res, cr.mirror(arrays, cl.leaf_mode, plant, Xn, 4))
    cl.close()


def test_saved_law_with_modes_rolls_out_the_same(tmp_path):
    """save / load keep leaf_mode; the loaded law (no source, no compile) gives the same bits."""
    law, plant, X0, kw = cr.case('noisy', 2, 2)
    assert plant.n_modes > 1
    cl = _compile(law)
    path = str(tmp_path / 'law.npz')
    cl.save(path)
    ld = compiled.CompiledLaw.load(path)
    assert ld.mpc is None and np.array_equal(ld.leaf_mode, cl.leaf_mode)
    assert ld.stats['bytes'] == cl.stats['bytes']
    a, b = cl.rollout(X0, T, plant=plant, **kw), ld.rollout(X0, T, plant=plant, **kw)
    for f in cr.BIT_EQUAL + ('u_norm_sum', 'mode'):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    # a file without the key loads without modes: a multi-mode plant is then refused
    cl.set_leaf_modes(None)
    cl.save(path)
    bare = compiled.CompiledLaw.load(path)
    assert bare.leaf_mode is None
    with pytest.raises(ValueError):
        bare.rollout(X0, T, plant=plant)
    for c in (cl, ld, bare):
        c.close()


def test_traj0_split_under_noise():
    """Two half batches (traj0 offset) equal one whole batch."""
    law, plant, X0, kw = cr.case('noisy', 4, 1)
    cl = _compile(law)
    whole = cl.rollout(X0, T, plant=plant, **kw)
    h = X0.shape[0] // 2
    kw_b = dict(kw, traj0=kw['traj0'] + h)
    parts = (cl.rollout(X0[:h], T, plant=plant, **kw), cl.rollout(X0[h:], T, plant=plant, **kw_b))
    for f in cr.BIT_EQUAL + ('u_norm_sum', 'mode'):
        w = getattr(whole, f)
        axis = 0 if w.ndim == 1 or f == 'x_final' else 1
        both = np.concatenate([getattr(q, f) for q in parts], axis=axis)
        assert np.array_equal(w, both, equal_nan=True), f
    cl.close()


class _PaddedModel(es.NoiseModel):
    """A model whose packed data carries unused doubles after its terms (to size the LDS)."""

    pad = 0

    def pack(self):
        desc, data = super().pack()
        return desc, np.concatenate([data, np.zeros(self.pad)])


def _refused(cl, code=_capi.EHM_E_INVALID):
    """After a refusal the device holds no plant: a raw rollout is refused too, so no kernel ran."""
    lib = _capi.load()
    n = 2
    out = [np.zeros(n * cl.p), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32),
           np.zeros(n), np.zeros(n), np.zeros(n)]
    rc = lib.ehm_compiled_rollout(cl._handle, n, 3, np.zeros(n * cl.p).ctypes.data, None, None,
                                  1e-9, None, None, None, *[a.ctypes.data for a in out], None)
    assert rc == code and b'no plant' in lib.ehm_compiled_last_error()
    assert (out[1] == 0).all() and (out[0] == 0).all()


def test_refusals():
    from explicit_hybrid_mpc_amd import explicit
    rng = np.random.default_rng(21)
    X1 = np.zeros((4, 1))
    # a law with a test node
    ex = explicit.ExplicitMPC(cc.two_point_tree())
    cl = ex.compile()
    ex.close()
    assert cl.stats['n_test'] == 1
    for plant in (es.random_plant(rng, 1, 1, 1, 'inf'),
                  es.random_guarded(rng, 1, 1, 2, 'inf', substeps=2, n_rows=2)):
        cl.set_leaf_modes(np.zeros(2, dtype=np.int32))
        with pytest.raises(_capi.EhmError) as err:
            cl.rollout(X1, 3, plant=plant)
        assert err.value.code == _capi.EHM_E_INVALID and 'test node' in str(err.value)
        _refused(cl)
    cl.close()
    # five inputs
    law = es.SynthLaw(es.kuhn_forest(2), 5, 1, rng, n_sub=2)
    cl = _compile(law)
    with pytest.raises(_capi.EhmError) as err:
        cl.set_plant(es.random_plant(rng, 2, 5, 1, 'inf'))
    assert err.value.code == _capi.EHM_E_INVALID
    _refused(cl)
    cl.close()
    # a multi-mode plant without leaf_mode, a mode >= n_modes, noise with a guarded plant
    law = es.SynthLaw(es.kuhn_forest(2), 2, 3, rng, n_sub=4)
    cl = _compile(law)
    X2 = rng.uniform(-0.5, 0.5, (8, 2))
    two, three = es.random_plant(rng, 2, 2, 2, 'inf'), es.random_plant(rng, 2, 2, 3, 'inf')
    assert cl.leaf_mode.max() == 2
    with pytest.raises(_capi.EhmError) as err:
        cl.rollout(X2, 3, plant=two)
    assert err.value.code == _capi.EHM_E_INVALID
    _refused(cl)
    modes = cl.leaf_mode.copy()
    cl.set_leaf_modes(None)
    with pytest.raises(ValueError):
        cl.rollout(X2, 3, plant=three)
    guarded = es.random_guarded(rng, 2, 2, 3, 'inf', substeps=2, n_rows=3)
    with pytest.raises(ValueError):
        cl.rollout(X2, 3, plant=guarded)
    _refused(cl)
    low = modes.copy()
    low[0] = -2
    for bad in (modes[:-1], low):
        with pytest.raises(_capi.EhmError):
            cl.set_leaf_modes(bad)
    cl.set_leaf_modes(modes)
    with pytest.raises(ValueError):
        cl.rollout(X2, 3, plant=guarded, noise=es.random_noise(rng, 2, 2, 0))
    with pytest.raises(ValueError):
        cl.rollout(X2, 3, plant=three, noise=es.random_noise(rng, 2, 2, 0), v=np.zeros((3, 8, 2)))
    with pytest.raises(ValueError):
        cl.rollout(X2, 3, plant=three, d=np.zeros((3, 8, 1)))
    _refused(cl)
    assert cl.rollout(X2, 3, plant=three).steps.shape == (8,)       # and the good call runs
    cl.close()


def test_noisy_lds_cap():
    """Plant + model of exactly 8192 doubles runs and matches the mirror; one more is refused."""
    p, n_u = 8, 4
    rng = np.random.default_rng(11)
    plant = es.random_plant(rng, p, n_u, 4, 'inf', n_d=8, n_g=256)
    rows, _, _ = plant.region_arrays()
    total = (4 * p * p + 4 * p * n_u + 4 * p + 256 * p + 256 + p * p + n_u * n_u + p * 8
             + int(rows.sum()) * (p + 1))
    law = es.SynthLaw(es.kuhn_forest(p), n_u, 4, rng)
    base = es.random_noise(rng, p, n_u, 8)
    X0 = rng.uniform(-0.8, 0.8, (64, p))
    for extra, ok in ((0, True), (1, False)):
        model = _PaddedModel(p, n_u, 8)
        model.terms = base.terms
        model.pad = 8192 - total - base.pack()[1].size + extra
        assert model.pad > 0
        cl = _compile(law)
        if ok:
            res = cl.rollout(X0, 8, plant=plant, noise=model, seed=5)
            cr.assert_same(res, cr.mirror(cl.arrays(), cl.leaf_mode, plant, X0, 8, noise=model,
                                          seed=5))
        else:
            with pytest.raises(_capi.EhmError) as err:
                cl.rollout(X0, 8, plant=plant, noise=model, seed=5)
            assert err.value.code == _capi.EHM_E_INVALID
        cl.close()


@pytest.fixture(scope='module')
def lin():
    """The 'lin' partition of test_nested_reference_layout from the flat forest: the oracle, the
    explicit law, its compiled law, initial states, and the two rollouts.  Eight steps: the closed
    loop converges to the origin, a vertex of the roots, so from step 9 on the root weights come
    within 1e-6 of 0 (measured: 250 of these 256 trajectories are clear at T = 8, 46 at T = 12)."""
    from explicit_hybrid_mpc_amd import examples, explicit, partition
    mpc = helpers.make_instance('lin', 0)
    V = examples.box_vertices(examples.theta_box(mpc))
    orc = examples.create_oracle(mpc, V, abs_frac=0.3, abs_err=None, rel_err=0.5)
    _, flat = partition.partition_set(orc, V)
    ex = explicit.ExplicitMPC(flat, orc)
    cl = ex.compile()
    half = examples.theta_box(orc.mpc)
    X0 = np.random.default_rng(9).uniform(-1, 1, (256, half.size)) * half
    out = types.SimpleNamespace(orc=orc, ex=ex, cl=cl, X0=X0, T=8)
    out.res_e = ex.rollout(X0, out.T)
    out.res_c = cl.rollout(X0, out.T)
    arrays = cl.arrays()
    out.mir = cr.mirror(arrays, cl.leaf_mode, cl._rollout_plant, X0, out.T)
    # clear trajectories: every step's smin > 1e-9, the root's weights more than 1e-6 from 0
    p = half.size
    clear = np.ones(X0.shape[0], dtype=bool)
    for t in range(out.T):
        on = np.nonzero(out.mir.roots[t] >= 0)[0]
        if on.size == 0:
            continue
        z = out.mir.z[t, on]
        smin = cc.evaluate(arrays, z)[3]
        alpha, a0 = cc._weights(arrays['root_rec'][out.mir.roots[t, on]], z, p)
        near = np.minimum(np.abs(alpha).min(axis=1), np.abs(a0))
        clear[on[(smin <= 1e-9) | (near <= 1e-6)]] = False
    out.clear = clear
    yield out
    ex.close()
    cl.close()
    orc.close()


def test_real_partition_against_explicit_rollout(lin):
    """ExplicitMPC.compile attaches the plant's source and the modes; on the clear trajectories
    the compiled rollout takes the steps of ExplicitMPC.rollout."""
    assert lin.cl.mpc is lin.orc.mpc and lin.cl.stats['n_test'] == 0
    if hasattr(lin.orc.mpc, 'step0_mode'):
        assert lin.cl.leaf_mode.shape == (lin.cl.stats['n_leaf'],)
    cr.assert_same(lin.res_c, lin.mir)
    c = lin.clear
    assert c.sum() > c.size // 2
    for f in ('steps', 'status'):
        assert np.array_equal(getattr(lin.res_c, f)[c], getattr(lin.res_e, f)[c]), f
    assert np.array_equal(lin.res_c.leaf[:, c], lin.res_e.leaf[:, c])
    assert np.allclose(lin.res_c.x[:, c], lin.res_e.x[:, c], rtol=1e-9, atol=0, equal_nan=True)
    assert np.array_equal(lin.res_c.mode[:, c], lin.res_e.mode[:, c])
    assert (lin.res_c.steps > 0).any()


def test_simulate_compare_takes_the_compiled_law(lin):
    from explicit_hybrid_mpc_amd import explicit
    im = explicit.ImplicitMPC(lin.orc)
    X0 = lin.X0[lin.clear][:48]
    a = simulate.compare(lin.cl, im, X0, lin.T)
    b = simulate.compare(lin.ex, im, X0, lin.T)
    assert a['both_ok'] == b['both_ok'] and a['n'] == X0.shape[0]
    assert a['stopped_explicit'] == b['stopped_explicit']
    assert np.isclose(a['u_norm_explicit'], b['u_norm_explicit'], rtol=1e-9)
