"""
Batched closed-loop simulation on the device (ehm_explicit_rollout, simulate.py): every recorded
step against the one-step evaluator (ehm_explicit_eval_batch) and a numpy plant step, the
warm-started root locator, the applied modes of a hybrid law, recursive feasibility of the cwh_z
law, the implicit law against the CPU oracle, and the reference's Simulator signature.
"""

import types

import numpy as np
import pytest

from tests import helpers
from tests import rollout_cpu

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _lin():
    from explicit_hybrid_mpc_amd import examples, partition
    mpc = helpers.make_instance('lin', 0)
    V = examples.box_vertices(examples.theta_box(mpc))
    orc = examples.create_oracle(mpc, V, abs_frac=0.3, abs_err=None, rel_err=0.5)
    _, flat = partition.partition_set(orc, V)
    orc.close()
    return mpc, flat


def _pwa_small():
    from explicit_hybrid_mpc_amd import engine
    mpc = helpers.make_instance('pwa_small', 0)
    roots, _ = helpers.roots_of(mpc)
    gp = engine.GpuProblem(mpc.compile(), helpers.eps_a_rule(mpc, 0.25), 0.2)
    flat = gp.partition(np.array(roots), action='ecc')
    gp.close()
    return mpc, flat


@pytest.fixture(scope='module')
def cwh():
    """cwh_z job 1 (abs_frac 0.5, rel_err 2): its partition and its oracle."""
    from explicit_hybrid_mpc_amd import examples
    from oracle import geometry
    full_set, _, oracle = examples.example('cwh_z', abs_frac=0.5, rel_err=2.0)
    roots, _ = geometry.delaunay_simplices(full_set)
    flat = oracle.gpu.partition(np.array(roots), action='ecc')
    yield oracle, flat
    oracle.close()


def _law(mpc, flat):
    from explicit_hybrid_mpc_amd import explicit
    return explicit.ExplicitMPC(flat, types.SimpleNamespace(mpc=mpc))


def _check_steps(ex, flat, res, X0, T, d=None, v=None):
    """Every recorded step of `res` against the one-step evaluator and the numpy plant."""
    pl = ex._rollout_plant
    cpu = rollout_cpu.flat_cpu(flat)
    assert np.array_equal(res.x[0], X0)
    applied = 0
    for t in range(T):
        on = np.nonzero(res.steps > t)[0]               # trajectories that applied step t
        stop = np.nonzero((res.steps == t) & (res.status != 0))[0]
        assert np.all(res.leaf[t, res.steps <= t] == -1)
        assert np.all(np.isnan(res.u[t, res.steps <= t]))
        idx = np.concatenate([on, stop])
        if idx.size == 0:
            continue
        z = res.x[t, idx] + (v[t, idx] if (v is not None and t > 0) else 0.)
        u_e, leaf_e, _, _ = ex.evaluate(z, return_info=True)
        k = on.size
        assert np.array_equal(res.u[t, on], u_e[:k])            # bit-equal
        assert np.array_equal(res.leaf[t, on], leaf_e[:k])
        # the exit test on the leaf the evaluator finds
        lam = np.array([rollout_cpu.weights(cpu, int(leaf_e[i]), z[i]).min() for i in range(idx.size)])
        assert np.all(lam[:k] >= -TOL)
        exits = res.status[stop] == 1
        assert np.all(lam[k:][exits] < -TOL)
        m = ex._node_mode[leaf_e[:k]]
        assert np.array_equal(res.mode[t, on], m)
        x_np = pl.step(res.x[t, on], res.u[t, on], m, None if d is None else d[t, on])
        # relative to the size of the summed terms (x+ may cancel to far below them)
        scale = np.einsum('nij,nj->ni', np.abs(pl.A[m]), np.abs(res.x[t, on])) \
            + np.einsum('nij,nj->ni', np.abs(pl.B[m]), np.abs(res.u[t, on])) + np.abs(pl.w[m])
        if d is not None:
            scale = scale + np.abs(d[t, on]) @ np.abs(pl.E.T)
        assert np.all(np.abs(res.x[t + 1, on] - x_np) <= 1e-12 * scale)
        applied += k
    assert applied > 0
    fin = res.steps == T
    assert np.array_equal(res.x_final[fin], res.x[T, fin])
    assert np.all(res.status[fin] == 0) and np.all(res.status[~fin] != 0)
    # the accumulated figures from the records
    u = np.nan_to_num(res.u)
    assert np.allclose(res.u_norm_sum, np.linalg.norm(u, axis=2).sum(axis=0), rtol=1e-12, atol=1e-300)
    return applied


@pytest.mark.parametrize('kind', ['lin', 'pwa_small', 'cwh_z'])
def test_rollout_matches_the_one_step_evaluator(kind, cwh):
    from explicit_hybrid_mpc_amd import examples
    if kind == 'cwh_z':
        oracle, flat = cwh
        mpc = oracle.mpc
    else:
        mpc, flat = _lin() if kind == 'lin' else _pwa_small()
    ex = _law(mpc, flat)
    half = examples.theta_box(mpc)
    rng = np.random.default_rng(1)
    n, T = 4096, 50
    X0 = rng.uniform(-1, 1, (n, half.size)) * half
    res = ex.rollout(X0, T)
    assert _check_steps(ex, flat, res, X0, T) > n
    assert not res.mode_violations.any()
    # with measurement errors (and process disturbances where the plant takes them)
    v = rng.uniform(-1, 1, (T, n, half.size)) * 1e-2 * half
    d = None
    if ex._rollout_plant.n_d:
        d = rng.uniform(-1, 1, (T, n, ex._rollout_plant.n_d)) * mpc.pars['w_max']
    res2 = ex.rollout(X0, T, d=d, v=v)
    _check_steps(ex, flat, res2, X0, T, d=d, v=v)
    # record=False gives the same figures
    res3 = ex.rollout(X0, T, d=d, v=v, record=False)
    for f in ('x_final', 'steps', 'status', 'cost', 'u_norm_sum', 'max_violation'):
        assert np.array_equal(getattr(res3, f), getattr(res2, f)), f
    if kind == 'pwa_small':
        # the applied mode is the step-0 mode of the leaf's commutation
        for t in range(T):
            on = res.steps > t
            lf = res.leaf[t, on]
            want = [mpc.step0_mode(flat.deltas[flat.delta_idx[k]]) for k in lf]
            assert np.array_equal(res.mode[t, on], want)
        assert len(np.unique(res.mode[res.mode >= 0])) == 2
    ex.close()


def test_long_spine_warm_started_locator():
    """652 Delaunay roots (p = 6): the visibility walk starts at the last step's root."""
    from explicit_hybrid_mpc_amd import engine, examples
    from explicit_hybrid_mpc_amd import tools as ehm_tools
    mpc = helpers.make_instance('chain', 0)
    half = examples.theta_box(mpc)
    roots, _ = ehm_tools.delaunay_roots(examples.box_vertices(half))
    R = np.array(roots)
    assert len(R) >= 128
    gp = engine.GpuProblem(mpc.compile(), 1., 1.)
    _, u0, didx = gp.solve_pt(R.reshape(-1, R.shape[2]))
    gp.close()
    assert (didx >= 0).all()
    K = len(R)
    flat = engine.FlatTree(R, -np.ones(K, np.int32), -np.ones(K, np.int32), np.zeros(K, np.int32),
                           np.zeros((K, R.shape[1])), u0.reshape(K, R.shape[1], -1),
                           np.zeros(K, np.uint8), np.zeros(K), {'n_roots': K},
                           mpc.compile().deltas[:1])
    ex = _law(mpc, flat)
    rng = np.random.default_rng(2)
    X0 = rng.uniform(-1, 1, (2048, half.size)) * half * 0.9
    res = ex.rollout(X0, 20)
    assert _check_steps(ex, flat, res, X0, 20) > 2048 * 10
    ex.close()


def test_cwh_z_closed_loop_stays_in_the_set(cwh):
    """The partitioned set is the constraint box and every interpolated input is feasible for
    the leaf's commutation: the nominal closed loop never leaves the set."""
    from explicit_hybrid_mpc_amd import examples
    oracle, flat = cwh
    ex = _law(oracle.mpc, flat)
    half = examples.theta_box(oracle.mpc)
    X0 = np.random.default_rng(4).uniform(-1, 1, (10000, 2)) * half
    res = ex.rollout(X0, 100, record=False)
    assert (res.status == 0).all(), np.bincount(res.status)
    assert (res.steps == 100).all()
    assert res.max_violation.max() <= 1e-9 * oracle.mpc.gx.max(), res.max_violation.max()
    ex.close()


def test_implicit_rollout_matches_the_cpu_oracle(cwh):
    from explicit_hybrid_mpc_amd import examples, explicit, simulate
    from oracle.oracle_cpu import OracleCPU
    from oracle.satellite_cpu import SatelliteZCPU
    oracle, flat = cwh
    im = explicit.ImplicitMPC(oracle)
    half = examples.theta_box(oracle.mpc)
    X0 = np.random.default_rng(6).uniform(-1, 1, (4, 2)) * half * 0.8
    res = im.rollout(X0, 8)
    cpu = OracleCPU(SatelliteZCPU(4), oracle.eps_a, oracle.eps_r)
    pl = simulate.Plant.from_mpc(oracle.mpc)
    checked = 0
    for t in range(8):
        for i in range(4):
            if res.steps[i] <= t:
                continue
            u, delta, _, _ = cpu.P_theta(res.x[t, i])
            assert u is not None
            assert np.allclose(res.u[t, i], u, rtol=1e-6, atol=1e-6 * 2e-3)
            assert np.array_equal(oracle.canonical.deltas[res.commutation[t, i]], delta)
            assert res.mode[t, i] == oracle.mpc.step0_mode(delta)
            x_np = pl.step(res.x[t, i][None], res.u[t, i][None], res.mode[t, i][None])[0]
            assert np.allclose(res.x[t + 1, i], x_np, rtol=1e-12, atol=0)
            checked += 1
    assert checked >= 16
    # compare: finite figures, and the ones numpy recomputes from the two recorded trajectories
    ex = _law(oracle.mpc, flat)
    X0 = np.random.default_rng(7).uniform(-1, 1, (64, 2)) * half
    fig = simulate.compare(ex, im, X0, 12, record=True)
    e, m = fig['explicit'], fig['implicit']
    both = (e.status == 0) & (m.status == 0)
    assert fig['both_ok'] == both.sum() > 32
    se = np.linalg.norm(np.nan_to_num(e.u), axis=2).sum(axis=0)[both].sum()
    si = np.linalg.norm(np.nan_to_num(m.u), axis=2).sum(axis=0)[both].sum()
    assert np.isfinite(fig['overconsumption_total']) and np.isfinite(fig['cost_ratio_total'])
    assert fig['overconsumption_total'] == pytest.approx((se - si) / si, rel=1e-10)
    ce = pl.stage_cost(np.nan_to_num(e.x[:-1]).reshape(-1, 2), np.nan_to_num(e.u).reshape(-1, 1))
    ci = pl.stage_cost(np.nan_to_num(m.x[:-1]).reshape(-1, 2), np.nan_to_num(m.u).reshape(-1, 1))
    ce, ci = ce.reshape(12, -1).sum(axis=0), ci.reshape(12, -1).sum(axis=0)
    assert fig['cost_ratio_total'] == pytest.approx(ce[both].sum() / ci[both].sum(), rel=1e-10)
    ex.close()


def test_simulator_has_the_reference_signature(cwh):
    from explicit_hybrid_mpc_amd.simulate import Simulator
    oracle, flat = cwh
    ex = _law(oracle.mpc, flat)
    x0 = np.array([0.03, -2e-4])
    sim = Simulator(ex, 1000.).run(x0, label='explicit')
    K = 11                                     # t = 0, 100, .., 1000 s
    assert sim.t.shape == (K,) and sim.x.shape == (2, K) and sim.u.shape == (1, K)
    assert sim.w.shape == (1, K) and sim.v.shape == (2, K) and sim.e.shape == (1, K)
    assert sim.label == 'explicit'
    res = ex.rollout(x0[None], K)
    assert np.array_equal(sim.x, res.x[:K, 0].T) and np.array_equal(sim.u, res.u[:, 0].T)
    ex.close()
