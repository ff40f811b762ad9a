"""
The inverted-pendulum law and its guarded plant on the device: the point oracles P_theta and
P_theta_delta against the CPU restatement (tests/pendulum_cpu.py), a partition grown from roots of
each of the three sections (volume closure, epsilon-suboptimality at sampled points), guarded
rollouts against the host mirror bit for bit, and compare / Simulator on both laws.
"""

import types

import numpy as np
import pytest

from tests import pendulum_cpu, rollout_cpu

pytestmark = pytest.mark.gpu

RTOL = 1e-7
MARGIN = 1e-6        # blocks whose feasible set has less interior are not compared


@pytest.fixture(scope='module')
def law():
    from explicit_hybrid_mpc_amd import mpc_library
    return mpc_library.InvertedPendulumOnCart(4)


def _thetas(law, rng, n):
    lo, hi = -np.diag(law.D_x), np.diag(law.D_x)
    out = [rng.uniform(a, b) for a, b in law.sections()]
    out += [rng.uniform(lo, hi) * 0.3 for _ in range(n)]
    return out


def test_point_oracles_match_cpu_restatement(law):
    from explicit_hybrid_mpc_amd.oracle import Oracle
    can = law.compile()
    gpu = Oracle(law, 1., 1.)
    rng = np.random.default_rng(21)
    compared = 0
    try:
        for theta in _thetas(law, rng, 3):
            thetas = np.repeat(theta[None], can.n_delta, axis=0)
            feas, _ = gpu.gpu.feasible_ptd(thetas, can.deltas)
            J, u0, st, _ = gpu.gpu.solve_ptd(thetas, can.deltas)
            best = np.inf
            for d in range(can.n_delta):
                margin = pendulum_cpu.interior_margin(can, d, theta)
                if margin == -np.inf or margin < -1e-9:
                    assert not feas[d], d
                    continue
                if margin < MARGIN:
                    continue
                ok, Jr, ur, conv = pendulum_cpu.solve_bigm(law, theta, can.deltas[d])
                assert ok and conv and feas[d] and st[d] == 0, d
                assert abs(J[d] - Jr) <= RTOL * (1 + abs(Jr)), (d, J[d], Jr)
                assert abs(u0[d][0] - ur[0]) <= 1e-6, (d, u0[d], ur)
                best = min(best, Jr)
                compared += 1
            u, delta, Jp, _ = gpu.P_theta(theta)
            if np.isfinite(best):
                assert Jp is not None and Jp <= best + RTOL * (1 + abs(best))
    finally:
        gpu.close()
    assert compared >= 10


def _eps_a(law, oracle, abs_frac=0.5):
    """create_oracle's rule over the scaled vertices of the box that are feasible."""
    J, _, didx = oracle.gpu.solve_pt(abs_frac * law.box_vertices())
    return float(np.max(J[didx >= 0]))


@pytest.fixture(scope='module')
def grown(law):
    """A few roots of each section, all vertices feasible, grown at a coarse tolerance."""
    from explicit_hybrid_mpc_amd import examples
    from explicit_hybrid_mpc_amd.oracle import Oracle
    oracle = Oracle(law, 1., 1.)
    eps_a, eps_r = _eps_a(law, oracle), 2.0
    oracle.eps_a, oracle.eps_r = eps_a, eps_r
    oracle.gpu.set_eps(eps_a, eps_r)
    roots, owner = examples.pendulum_roots(law)
    pick = []
    for sec in range(3):
        cand = np.flatnonzero(owner == sec)
        _, _, didx = oracle.gpu.solve_pt(roots[cand].reshape(-1, 4))
        ok = (didx.reshape(len(cand), 5) >= 0).all(axis=1)
        pick += list(cand[ok][:2])
    roots = roots[pick]
    flat = oracle.gpu.partition(np.array(roots), action='ecc', max_depth=14)
    yield law, oracle, flat, roots, owner[pick]
    oracle.close()


def _simplex_volume(R):
    return abs(np.linalg.det(R[1:] - R[0])) / 24.


def test_grown_roots_of_every_section(grown):
    from explicit_hybrid_mpc_amd import examples
    law, oracle, flat, roots, owner = grown
    assert set(owner.tolist()) == {0, 1, 2}, 'a section has no root with all vertices feasible'
    leaves = [k for k in range(flat.n_nodes) if flat.is_leaf(k)]
    vol_leaves = sum(_simplex_volume(flat.vertices[k]) for k in leaves)
    vol_roots = sum(_simplex_volume(R) for R in roots)
    assert abs(vol_leaves - vol_roots) <= 1e-9 * vol_roots
    closed = [k for k in leaves if flat.flags[k] & 1]
    assert len(closed) >= 3
    # sampled closed leaves: the interpolated vertex cost is epsilon-suboptimal against the
    # CPU restatement's optimum (min over the commutations of the uncondensed program)
    can = law.compile()
    rng = np.random.default_rng(4)
    checked = 0
    for k in rng.choice(closed, size=min(4, len(closed)), replace=False):
        lam = rng.dirichlet(np.ones(5))
        theta = lam @ flat.vertices[k]
        J_interp = float(lam @ flat.vertex_costs[k])
        best = np.inf
        for d in range(can.n_delta):
            if pendulum_cpu.interior_margin(can, d, theta) < MARGIN:
                continue
            ok, Jr, _, conv = pendulum_cpu.solve_bigm(law, theta, can.deltas[d])
            if ok and conv:
                best = min(best, Jr)
        assert np.isfinite(best)
        assert J_interp - best <= max(oracle.eps_a, oracle.eps_r * best) + 1e-7 * (1 + best)
        checked += 1
    assert checked >= 3


def _starts(flat, rng, n):
    leaves = np.array([k for k in range(flat.n_nodes) if flat.is_leaf(k) and flat.flags[k] & 1])
    k = rng.choice(leaves, size=n)
    lam = rng.dirichlet(np.ones(5), size=n)
    return np.einsum('nj,njc->nc', lam, flat.vertices[k])


def test_guarded_rollout_matches_host_mirror(grown):
    from explicit_hybrid_mpc_amd import explicit, simulate
    law, oracle, flat, roots, owner = grown
    ex = explicit.ExplicitMPC(flat, types.SimpleNamespace(mpc=law))
    rng = np.random.default_rng(9)
    X0 = _starts(flat, rng, 600)
    T = 15
    res = ex.rollout(X0, T, record=True)
    plant = ex._rollout_plant
    assert isinstance(plant, simulate.GuardedPlant) and res.mode is None
    assert set(np.unique(res.status).tolist()) <= {0, 1, 3}
    cpu = rollout_cpu.flat_cpu(flat)
    assert np.array_equal(res.x[0], X0)
    applied = 0
    cost = np.zeros(X0.shape[0])
    unorm = np.zeros(X0.shape[0])
    for t in range(T):
        on = np.nonzero(res.steps > t)[0]
        assert np.all(res.leaf[t, res.steps <= t] == -1)
        stop = np.nonzero((res.steps == t) & (res.status == 1))[0]
        if stop.size:
            _, leaf_s, _, _ = ex.evaluate(res.x[t, stop], return_info=True)
            lam = np.array([rollout_cpu.weights(cpu, int(leaf_s[i]), res.x[t, stop[i]]).min()
                            for i in range(stop.size)])
            assert np.all(lam < -1e-9)
        if on.size == 0:
            continue
        x = res.x[t, on]
        u_e, leaf_e, _, _ = ex.evaluate(x, return_info=True)
        assert np.array_equal(res.u[t, on], u_e)                   # bit-equal
        assert np.array_equal(res.leaf[t, on], leaf_e)
        x_np = plant.step(x, u_e)
        assert np.array_equal(res.x[t + 1, on], x_np)              # bit-equal, 10 plant steps
        cost[on] += plant.stage_cost(x, u_e)
        unorm[on] += np.sqrt(np.sum(u_e * u_e, axis=1))
        applied += on.size
    assert applied >= 600
    assert np.array_equal(res.cost, cost) and np.allclose(res.u_norm_sum, unorm, rtol=1e-15)
    fin = np.array([res.x[res.steps[q], q] for q in range(X0.shape[0])])
    assert np.array_equal(res.x_final, fin)
    # without records: the same summaries
    res2 = ex.rollout(X0, T, record=False)
    for key in ('x_final', 'steps', 'status', 'cost', 'u_norm_sum'):
        assert np.array_equal(getattr(res2, key), getattr(res, key))
    with pytest.raises(ValueError, match='guarded'):
        from explicit_hybrid_mpc_amd.noise import NoiseModel
        ex.rollout(X0[:2], 2, noise=NoiseModel(4, 1, 0))
    ex.close()


def test_compare_and_simulator_on_both_laws(grown):
    from explicit_hybrid_mpc_amd import explicit, simulate
    law, oracle, flat, roots, owner = grown
    ex = explicit.ExplicitMPC(flat, oracle)
    im = explicit.ImplicitMPC(oracle)
    rng = np.random.default_rng(12)
    X0 = _starts(flat, rng, 40)
    out = simulate.compare(ex, im, X0, 5, record=True)
    assert out['n'] == 40
    assert out['explicit'].status.shape == (40,) and out['implicit'].status.shape == (40,)
    imr = out['implicit']
    applied = imr.steps > 0
    assert applied.any()
    # the implicit law's plant steps are the host mirror's
    for t in range(5):
        on = np.nonzero(imr.steps > t)[0]
        if on.size:
            assert np.array_equal(imr.x[t + 1, on], im._rollout_plant.step(imr.x[t, on], imr.u[t, on]))
    sim = simulate.Simulator(ex, 1.0).run(X0[0])
    assert sim.x.shape[0] == 4 and sim.x.shape[1] <= 101
    K = sim.x.shape[1]
    assert K == 10 * int(ex.rollout(X0[:1], 11).steps[0]) or K == 101
    with pytest.raises(ValueError, match='every 10'):
        simulate.Simulator(ex, 3.0).run(X0[0])
    ex.close()
