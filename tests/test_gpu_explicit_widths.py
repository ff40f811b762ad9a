"""
The explicit law's kernels at every compiled width against exact arithmetic (tests/explicit_synth):
k_explicit_setup / _locate / _eval for p = 1..8 (with and without the root locator), every
k_explicit_rollout<P, NU, KIND> of k_rollout_table (8 x 4 x 3 = 96 instantiations, one test id
each) against the order-faithful host mirror, and the edges: batch sizes, T = 0, tol_exit = 0,
record=False, the noisy kernel's LDS cap, n_u = 5, the guarded limits, a spine just under the
locator's 2^20 roots, and roots whose shared zero coordinates are written as -0.0.

Tolerances follow from the condition number kappa of the nodes on a state's path: the device
leaf must be the exact one where every decision's exact margin exceeds 1e-10 (1 + kappa);
elsewhere every turn of the device's walk must be the exact turn or one whose exact margin is
within that threshold (SynthLaw.check_path; after such a turn the reference's rule -- right
without a test -- may end in a leaf far from x), and where the device leaf is the exact one, x's
exact weights in it must be >= -max(1e-9, 64 kappa eps); the input must be within
32 p kappa eps max|U| (times the largest |weight| when they extrapolate) of the exact
interpolation in the device leaf.
"""

from fractions import Fraction

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, noise as ehm_noise
from tests import explicit_synth as es

pytestmark = pytest.mark.gpu

KINDS = ('nominal', 'noisy', 'guarded')       # PlantKind order
XP, MAX_NU = 8, 4                             # EHM_XP, EHM_R_MAX_NU
CASES = [(kind, p, nu) for kind in KINDS for p in range(1, XP + 1) for nu in range(1, MAX_NU + 1)]
assert len(CASES) == XP * MAX_NU * len(KINDS) == 96      # every k_rollout_table entry
N_TRAJ, T_STEPS = 256, 16
STATUS_SEEN = {kind: set() for kind in KINDS}
STATUS_CAN = {'nominal': {0, 1, 2, 3}, 'noisy': {0, 1, 2, 3}, 'guarded': {0, 1, 3}}


def _weight_floor(kappa):
    return -Fraction(max(1e-9, 64 * kappa * es.EPS))


def _check_eval(law, ex, X, locator):
    """Device leaf / input / visited of X against the exact walk; returns the number of states
    whose root lies beyond LOCATE_STEPS and that the locator resolved."""
    u, leaf, visited, _ = ex.evaluate(X, return_info=True)
    beyond = decisive = 0
    for q, x in enumerate(X):
        ref = law.locate(x)
        k = int(leaf[q])
        dec = law.decisive(ref)
        if dec:
            decisive += 1
            assert k == ref.leaf, (q, k, ref.leaf, float(ref.margin), ref.kappa)
        lam = law.check_path(k, ref)
        if k == ref.leaf:
            assert lam == ref.lam
            assert Fraction(min(lam), ref.D) >= _weight_floor(ref.kappa), q
        ue = law.u_exact(k, lam, ref.D)
        tol = law.u_tol(max(ref.kappa, law.kappa(k)), lam, ref.D)
        assert np.all(np.abs(u[q] - ue) <= tol), (q, u[q], ue, tol)
        if not dec:
            continue
        if not locator:
            assert visited[q] == ref.tests, (q, visited[q], ref.tests)
        elif ref.root_margin > 1e-6:
            # the visibility walk's steps, or (a walk longer than EHM_X_STEPS) the serial walk's
            walk = visited[q] - ref.internal
            assert 1 <= walk <= es.LOCATE_STEPS or visited[q] == ref.tests, (q, visited[q])
            if ref.root > es.LOCATE_STEPS and walk <= es.LOCATE_STEPS:
                beyond += 1
    assert decisive >= X.shape[0] // 4
    return beyond


@pytest.mark.parametrize('p', range(1, XP + 1), ids=lambda p: 'p%d' % p)
def test_evaluator_against_exact_walk(p):
    """k_explicit_eval at runtime p, setup's Gauss-Jordan Minv, and the visibility walk: a
    locator-sized Kuhn forest and its first 100 roots (the serial spine walk)."""
    rng = np.random.default_rng(100 + p)
    n_u = p % 6 + 1
    for keep in (None, 100):
        law = es.SynthLaw(es.kuhn_forest(p, keep), n_u, 2, rng)
        assert (law.forest.n_roots >= es.LOCATE_MIN) == (keep is None)
        ex = law.explicit()
        X = law.states(rng, 2400)
        beyond = _check_eval(law, ex, X, keep is None)
        if keep is None:
            assert beyond > 0           # the locator, not the serial walk, found far roots
        ex.close()


def _case(kind, p, n_u):
    """The law, plant, model and rollout arguments of one instantiation."""
    rng = np.random.default_rng([KINDS.index(kind), p, n_u])
    cost = 'inf' if (p + n_u + KINDS.index(kind)) % 2 == 0 else 'quadratic'
    kw = dict(tol_exit=1e-9)
    if kind == 'guarded':
        n_modes = 2 + (p + n_u) % 7
        plant = es.random_guarded(rng, p, n_u, n_modes, cost, substeps=1 + (p * n_u) % 4,
                                  n_rows=1 + (p + 3 * n_u) % 16)
    else:
        n_modes = 1 + (p + 2 * n_u) % 4
        n_d = 8 if (p + n_u) % 2 else 0
        plant = es.random_plant(rng, p, n_u, n_modes, cost, n_d=n_d)
    law = es.SynthLaw(es.kuhn_forest(p), n_u, n_modes, rng)
    X0 = np.concatenate([rng.uniform(-0.9, 0.9, (N_TRAJ // 2, p)),
                         law.states(rng, N_TRAJ)[:N_TRAJ // 2]])
    if kind == 'noisy':
        kw.update(noise=es.random_noise(rng, p, n_u, plant.n_d), seed=int(rng.integers(1 << 40)),
                  traj0=int(rng.integers(1 << 20)))
    elif kind == 'nominal':
        kw['v'] = rng.normal(size=(T_STEPS, X0.shape[0], p)) * 1e-3
        if plant.n_d:
            kw['d'] = rng.normal(size=(T_STEPS, X0.shape[0], plant.n_d))
    return law, plant, X0, kw


def _run_case(kind, p, n_u):
    law, plant, X0, kw = _case(kind, p, n_u)
    ex = law.explicit()
    res = ex.rollout(X0, T_STEPS, plant=plant, **kw)
    mirror = es.replay(law, plant, res, X0, T_STEPS, **kw)
    es.check_replay(mirror, res)
    # record=False computes the same
    bare = ex.rollout(X0, T_STEPS, plant=plant, record=False, **kw)
    for f in ('x_final', 'steps', 'status', 'cost', 'u_norm_sum', 'max_violation'):
        assert np.array_equal(getattr(bare, f), getattr(res, f)), f
    assert bare.x is None and bare.u is None and bare.leaf is None
    ex.close()
    STATUS_SEEN[kind].update(int(s) for s in np.unique(res.status))
    return res


@pytest.mark.parametrize('kind,p,n_u', CASES, ids=['%s-p%d-nu%d' % c for c in CASES])
def test_rollout_instantiation(kind, p, n_u):
    """k_rollout_table[kind][p-1][n_u-1] against the exact walk and the order-faithful mirror."""
    res = _run_case(kind, p, n_u)
    assert (res.steps > 0).any()


def test_every_status_code_occurs():
    """Each status the plant kind can produce occurs in the sweep (cases not run yet run here)."""
    for kind, p, n_u in CASES:
        if STATUS_SEEN[kind] >= STATUS_CAN[kind]:
            continue
        _run_case(kind, p, n_u)
    for kind in KINDS:
        assert STATUS_SEEN[kind] >= STATUS_CAN[kind], (kind, STATUS_SEEN[kind])


def test_batch_edges_and_exit_tolerance():
    """n = 0, 1 and 257 (a partial block), T = 0, tol_exit = 0."""
    law, plant, X0, kw = _case('nominal', 3, 2)
    ex = law.explicit()
    rng = np.random.default_rng(7)
    X = np.concatenate([X0, law.states(rng, 64)])[:257]
    assert X.shape[0] == 257
    for n in (0, 1, 257):
        for tol in (0., 1e-9):
            kw2 = dict(tol_exit=tol, v=rng.normal(size=(T_STEPS, n, 3)) * 1e-3)
            res = ex.rollout(X[:n], T_STEPS, plant=plant, **kw2)
            assert res.x_final.shape == (n, 3) and res.steps.shape == (n,)
            mirror = es.replay(law, plant, res, X[:n], T_STEPS, **kw2)
            es.check_replay(mirror, res)
    res = ex.rollout(X, 0, plant=plant)
    assert np.array_equal(res.x_final, X) and (res.steps == 0).all() and (res.status == 0).all()
    assert (res.cost == 0).all() and (res.u_norm_sum == 0).all()
    assert np.all(res.max_violation == -np.inf)
    assert res.x.shape == (1, 257, 3) and np.array_equal(res.x[0], X)
    ex.close()


class _PaddedModel(ehm_noise.NoiseModel):
    """A model whose packed data carries unused doubles after its terms (to size the LDS)."""

    pad = 0

    def pack(self):
        desc, data = super().pack()
        return desc, np.concatenate([data, np.zeros(self.pad)])


def test_noisy_lds_cap():
    """Plant + model of exactly EHM_N_MAX_LDS (8192) doubles runs and is correct; one more is
    refused with EHM_E_INVALID."""
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
        ex = law.explicit()
        if ok:
            res = ex.rollout(X0, 8, plant=plant, noise=model, seed=5)
            mirror = es.replay(law, plant, res, X0, 8, tol_exit=1e-9, noise=model, seed=5)
            es.check_replay(mirror, res)
        else:
            with pytest.raises(_capi.EhmError) as err:
                ex.rollout(X0, 8, plant=plant, noise=model, seed=5)
            assert err.value.code == _capi.EHM_E_INVALID
        ex.close()


def test_five_inputs_are_refused_by_set_plant():
    rng = np.random.default_rng(12)
    law = es.SynthLaw(es.kuhn_forest(2), 5, 1, rng, n_sub=2)
    ex = law.explicit()
    with pytest.raises(_capi.EhmError) as err:
        ex.set_plant(es.random_plant(rng, 2, 5, 1, 'inf'))
    assert err.value.code == _capi.EHM_E_INVALID
    ex.close()


def test_guarded_limits():
    """8 modes, 16 guard rows (strict and non-strict), 64 substeps."""
    rng = np.random.default_rng(13)
    plant = es.random_guarded(rng, 3, 2, 8, 'quadratic', substeps=64, n_rows=16)
    stricts = [r[4] for _, rows in plant.guards for r in rows]
    assert len(stricts) == 16 and any(stricts) and not all(stricts)
    law = es.SynthLaw(es.kuhn_forest(3), 2, 8, rng)
    X0 = rng.uniform(-0.9, 0.9, (256, 3))
    ex = law.explicit()
    res = ex.rollout(X0, 12, plant=plant)
    es.check_replay(es.replay(law, plant, res, X0, 12, tol_exit=1e-9), res)
    assert (res.steps > 0).any()
    ex.close()


def test_locator_root_ids_above_2_19():
    """A 724 x 724 Kuhn grid (1 048 352 roots, just under 2^20): state q sits in the root next to
    its start root q, so the walk takes two steps and returns ids up to 2^20."""
    F = es.KuhnForest([724, 724], 0., 2. ** -10)
    assert es.MAX_ROOTS // 2 < F.n_roots < es.MAX_ROOTS
    law = es.SynthLaw(F, 1, 1, np.random.default_rng(14), n_sub=0)
    target = np.arange(F.n_roots) ^ 1
    X = law.vertices[target].mean(axis=1)
    ex = law.explicit()
    u, leaf, visited, _ = ex.evaluate(X, return_info=True)
    assert np.array_equal(leaf, target)
    assert (visited == 2).all()
    rng = np.random.default_rng(15)
    for q in np.concatenate([rng.integers(1 << 19, F.n_roots, 512), [F.n_roots - 1]]):
        ref = law.locate(X[q])
        assert ref.leaf == target[q] and law.decisive(ref)
        assert abs(u[q, 0] - law.u_exact(ref.leaf, ref.lam, ref.D)[0]) <= law.u_tol(ref.kappa)
    ex.close()


def test_negative_zero_vertices_keep_the_face_adjacency():
    """Roots of [-1, 1]^2 left of x0 = 0 write their zero coordinates as -0.0: the locator must
    still cross those faces (vertex keys by value, not by bytes)."""
    F = es.KuhnForest([32, 32], -1., 2. ** -4)
    law = es.SynthLaw(F, 1, 1, np.random.default_rng(16), n_sub=0)
    left_half = F.grid[:, 0, 0] < 16
    V = law.vertices[:F.n_roots]
    V[left_half] = np.where(V[left_half] == 0., np.copysign(0., -1.), V[left_half])
    assert np.signbit(V[left_half][V[left_half] == 0.]).all()
    start = np.arange(F.n_roots)
    cell, a = np.divmod(start, 2)
    i, j = np.divmod(cell, 32)
    target = ((np.where(i < 31, i + 1, i - 1) * 32 + j) * 2 + a)
    X = law.vertices[target].mean(axis=1)
    ex = law.explicit()
    _, leaf, visited, _ = ex.evaluate(X, return_info=True)
    assert np.array_equal(leaf, target)
    crossing = (i == 15)
    assert crossing.sum() == 64 and target[crossing].min() > 1000
    assert visited.max() <= 8, np.sort(visited)[-8:]
    ex.close()
