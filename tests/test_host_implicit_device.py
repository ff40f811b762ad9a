"""
The device loop around the implicit law, as far as it can be checked without a device: its numpy
mirror (tests/implicit_cpu.py) keeps the conventions of ``simulate.rollout_implicit`` (the host
loop driven by the same CPU law), ``on_device=True`` refuses what it cannot run before it touches a
device, and the compaction and selection rules agree with a brute-force statement on random
verdict tables.
"""

import types

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import examples, simulate
from explicit_hybrid_mpc_amd.noise import NoiseModel
from oracle.oracle_cpu import OracleCPU
from tests import implicit_cpu


class _CpuLaw:
    """``OracleCPU.P_theta`` behind the surface the loops use (``gpu.solve_pt``, ``canonical``)."""

    def __init__(self, mpc):
        self.mpc = mpc
        self.cpu = OracleCPU(mpc, 1., 1.)
        self.canonical = mpc.compile()
        self.gpu = types.SimpleNamespace(solve_pt=self.solve_pt)

    def solve_pt(self, Z):
        Z = np.atleast_2d(Z)
        J = np.full(Z.shape[0], np.inf)
        u0 = np.full((Z.shape[0], self.canonical.n_u), np.nan)
        didx = np.full(Z.shape[0], -1, dtype=np.int32)
        for k, z in enumerate(Z):
            u, delta, Jk, _ = self.cpu.P_theta(z)
            if u is not None:
                J[k], u0[k], didx[k] = Jk, u, self.cpu.delta_index(delta)
        return J, u0, didx

    def law(self, Z):
        _, u0, didx = self.solve_pt(Z)
        return u0, didx


@pytest.fixture(scope='module')
def di():
    mpc = examples.double_integrator(3)
    return mpc, _CpuLaw(mpc)


def _plant_with_region(mpc):
    """The law's plant with a mode region x_0 <= 0.1 that some trajectories leave (status 2)."""
    pl = simulate.Plant.from_mpc(mpc)
    H = np.zeros((1, pl.n_x))
    H[0, 0] = 1.
    pl.regions = [(H, np.array([0.1]))] + list(pl.regions[1:])
    return pl


def test_mirror_keeps_the_host_loops_conventions(di):
    mpc, orc = di
    plant = _plant_with_region(mpc)
    half = examples.theta_box(mpc)
    rng = np.random.default_rng(3)
    X0 = rng.uniform(-1, 1, (24, plant.n_x)) * half * 0.8
    X0[:4] = half * 3.                                   # no law there: status 3 at t = 0
    X0[4:8, 0] = 0.5 * half[0] + 0.2                     # outside the mode region: status 2
    T = 6
    noise = NoiseModel(plant.n_x, plant.n_u, plant.n_d)
    noise.addIndependentTerm('state', -1e-3 * np.ones(plant.n_x), 1e-3 * np.ones(plant.n_x))
    noise.addDependentTerm('input', 0.05, norm=2, dim=plant.n_u, Fu=np.eye(plant.n_u), pu=2)
    mode_of = [mpc.step0_mode(dl) for dl in orc.canonical.deltas]
    for kw in (dict(), dict(noise=noise, seed=5, traj0=7)):
        ref = simulate.rollout_implicit(orc, plant, X0, T, **kw)
        got = implicit_cpu.rollout(orc.law, plant, mode_of, X0, T, **kw)
        assert np.array_equal(got['status'], ref.status)
        assert np.array_equal(got['steps'], ref.steps)
        assert {2, 3} <= set(ref.status.tolist()) and (ref.status == 0).any()
        assert np.array_equal(got['commutation'], ref.commutation)
        assert np.array_equal(got['mode'], ref.mode)
        assert np.array_equal(np.isnan(got['x']), np.isnan(ref.x))
        # the host loop's einsum has no fixed order: equal up to rounding, not bit for bit
        assert np.allclose(got['x'], ref.x, rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(got['u'], ref.u, rtol=0, atol=0, equal_nan=True)
        assert np.allclose(got['cost'], ref.cost, rtol=1e-12, atol=1e-14)
        assert np.allclose(got['u_norm_sum'], ref.u_norm_sum, rtol=1e-14)
        assert np.allclose(got['max_violation'], ref.max_violation, rtol=0, atol=1e-12)
        # a stopped trajectory keeps NaN / -1 records from its stop step on
        for q in np.flatnonzero(ref.status != 0):
            s = int(ref.steps[q])
            assert np.isnan(got['u'][s:, q]).all() and (got['commutation'][s:, q] == -1).all()
            assert np.isnan(got['x'][s + 1:, q]).all() and not np.isnan(got['x'][s, q]).any()
        if kw:
            for k in ('v', 'e', 'w'):
                assert np.array_equal(got[k], getattr(ref, k), equal_nan=True), k
            # v is drawn at every step a trajectory reaches and applied from t = 1
            live0 = ref.status != 3
            assert not np.isnan(got['v'][0]).any() and (got['v'][0] != 0).any()
            z0 = X0[live0]
            u_at_x0, _ = orc.law(z0)
            assert np.array_equal(got['u'][0, live0 & (ref.steps > 0)],
                                  u_at_x0[(ref.steps > 0)[live0]])
            # e = 0 where the commanded input is 0
            zero = np.all(got['u'] == 0., axis=2)
            assert (got['e'][zero] == 0.).all()


def test_e_is_zero_where_u_is_zero(di):
    mpc, orc = di
    plant = simulate.Plant.from_mpc(mpc)
    noise = NoiseModel(plant.n_x, plant.n_u, plant.n_d)
    noise.addIndependentTerm('input', -np.ones(plant.n_u), np.ones(plant.n_u))
    zero_law = lambda Z: (np.zeros((Z.shape[0], plant.n_u)), np.zeros(Z.shape[0], dtype=np.int32))
    got = implicit_cpu.rollout(zero_law, plant, [0], np.ones((3, plant.n_x)) * 0.1, 4, noise=noise)
    assert (got['e'] == 0.).all() and (got['u'] == 0.).all() and (got['status'] == 0).all()


def test_on_device_refusals_need_no_device(di):
    mpc, orc = di
    plant = simulate.Plant.from_mpc(mpc)
    X0 = np.zeros((2, plant.n_x))
    # an oracle whose sequences are not enumerated (the surface of bnb.PrefixOracle)
    prefix = types.SimpleNamespace(mpc=mpc, table=object())
    with pytest.raises(ValueError, match='enumerated'):
        simulate.rollout_implicit(prefix, plant, X0, 3, on_device=True)
    # too many inputs / parameters for the step kernels
    for n_u, p in ((5, plant.n_x), (plant.n_u, 9)):
        big = types.SimpleNamespace(mpc=mpc, gpu=object(),
                                    canonical=types.SimpleNamespace(n_u=n_u, p=p, n_delta=1))
        with pytest.raises(ValueError, match='n_u <= 4 and p <= 8'):
            simulate.rollout_implicit(big, plant, X0, 3, on_device=True)
    # noise with a guarded plant, and the other shared refusals
    from explicit_hybrid_mpc_amd import mpc_library
    pend = mpc_library.InvertedPendulumOnCart(4)
    gplant = simulate.Plant.from_mpc(pend)
    gorc = types.SimpleNamespace(mpc=pend, gpu=object(), canonical=pend.compile())
    noise = NoiseModel(gplant.n_x, gplant.n_u, 0)
    with pytest.raises(ValueError, match='guarded'):
        simulate.rollout_implicit(gorc, gplant, np.zeros((1, gplant.n_x)), 2, noise=noise,
                                  on_device=True)
    with pytest.raises(ValueError, match='not both'):
        simulate.rollout_implicit(orc, plant, X0, 3, v=np.zeros((3, 2, plant.n_x)),
                                  noise=NoiseModel(plant.n_x, plant.n_u, plant.n_d), on_device=True)
    # ImplicitMPC and compare pass the keyword on
    from explicit_hybrid_mpc_amd.explicit import ImplicitMPC
    with pytest.raises(ValueError, match='enumerated'):
        ImplicitMPC(prefix).rollout(X0, 3, plant=plant, on_device=True)
    ex = types.SimpleNamespace(rollout=lambda *a, **k: None)
    with pytest.raises(ValueError, match='enumerated'):
        simulate.compare(ex, ImplicitMPC(prefix), X0, 3, implicit_on_device=True)


def _brute(tau, st2, J, u0, live, st1):
    """The rules stated pair by pair, in the words of ehm_solve_pt_batch."""
    nd, n = tau.shape
    src, dst, seg = [], [], [0]
    for d in range(nd):
        for q in range(n):
            if live[q] and tau[d, q] <= implicit_cpu.FEAS_TOL:
                src.append(q)
                dst.append(d * n + q)
        seg.append(len(dst))
    u = np.full((n, u0.shape[2]), np.nan)
    didx = np.full(n, -1, dtype=np.int32)
    stalled = np.zeros(n, dtype=np.int64)
    for q in range(n):
        if not live[q]:
            continue
        feas = [d for d in range(nd) if tau[d, q] <= implicit_cpu.FEAS_TOL]
        stalled[q] = sum(1 for d in feas if st2[d, q] != 0) \
            + sum(1 for d in range(nd) if st1[d, q] != 0)
        good = [d for d in feas if st2[d, q] == 0]
        if not good:
            continue
        jm = min(J[d, q] for d in good)
        first = next(d for d in good
                     if J[d, q] <= jm + implicit_cpu.TIE_TOL * (1. + abs(jm)))
        didx[q], u[q] = first, u0[first, q]
    return (np.array(src, dtype=np.int64), np.array(dst, dtype=np.int32),
            np.array(seg, dtype=np.int32)), (u, didx, stalled)


@pytest.mark.parametrize('seed', range(6))
def test_compaction_and_selection_rules(seed):
    rng = np.random.default_rng(seed)
    nd, n, n_u = int(rng.integers(1, 9)), int(rng.integers(1, 700)), 2
    tau = np.where(rng.random((nd, n)) < 0.5, rng.uniform(-1e-9, 1e-8, (nd, n)),
                   rng.uniform(1e-8, 1., (nd, n)))
    tau[:, rng.random(n) < 0.1] = 0.5                    # all-infeasible rows
    tau[rng.random((nd, n)) < 0.02] = np.nan
    J = rng.uniform(-2., 2., (nd, n))
    base = rng.uniform(-2., 2., n)
    close = rng.random((nd, n)) < 0.4                    # ties within and just outside TIE_TOL
    J[close] = (base[None, :] + rng.uniform(0, 3e-6, (nd, n)))[close]
    st2 = np.where(rng.random((nd, n)) < 0.1, 2, 0).astype(np.int32)      # stalled pairs
    # stalled phase-one pairs, on either side of the verdict: their tau stands, they are counted
    st1 = np.where(rng.random((nd, n)) < 0.05, 2, 0).astype(np.int32)
    u0 = rng.normal(size=(nd, n, n_u))
    live = rng.random(n) < 0.85
    (src, dst, seg), (u, didx, stalled) = _brute(tau, st2, J, u0, live, st1)
    got_src, got_dst, got_seg = implicit_cpu.compact(tau, live)
    assert np.array_equal(got_src, src) and np.array_equal(got_dst, dst)
    assert np.array_equal(got_seg, seg)
    got_u, got_didx, got_stalled = implicit_cpu.select(tau, st2, J, u0, live, st1)
    assert (st1 != 0)[:, live].any() or n < 20
    assert np.array_equal(got_didx, didx)
    assert np.array_equal(got_u, u, equal_nan=True)
    assert np.array_equal(got_stalled, stalled)
    assert (didx[~live] == -1).all()


def test_summation_order_does_not_switch_commutations_on_cwh_z():
    """
    The CPU side of the host-loop comparison of tests/test_gpu_implicit_device.py: the same law
    (OracleCPU on the uncondensed cwh_z model) in closed loop under the device's fixed summation
    order and under the host loop's einsum.  Trajectories whose commutations ever differ may be at
    most 1 % of the batch, the cap the GPU test holds the two loops to.  Size: the first 16 in-box
    states of the GPU test's 512 (``implicit_cpu.cwh_states``) over 8 of its 60 steps -- a CPU
    P_theta of this law is 81 QPs, a third of a second, so the full batch would be 2.5 million
    QPs; with 16 trajectories the cap admits none.  The number that differ is printed.
    """
    from oracle.satellite_cpu import SatelliteZCPU
    mpc = examples.EXAMPLES['cwh_z']()
    cpu = OracleCPU(SatelliteZCPU(4), 1., 1.)
    can = mpc.compile()
    assert all(np.array_equal(np.asarray(a).astype(int), np.asarray(b).astype(int))
               for a, b in zip(cpu.deltas, can.deltas))
    plant = simulate.Plant.from_mpc(mpc)
    assert plant.n_modes == 3 and np.array_equal(plant.A[0], plant.A[1])
    mode_of = [mpc.step0_mode(dl) for dl in can.deltas]

    def law(Z):
        u0 = np.full((Z.shape[0], can.n_u), np.nan)
        didx = np.full(Z.shape[0], -1, dtype=np.int32)
        for k, z in enumerate(Z):
            u, delta, _, _ = cpu.P_theta(z)
            if u is not None:
                u0[k], didx[k] = u, cpu.delta_index(delta)
        return u0, didx

    X0 = implicit_cpu.cwh_states(examples.theta_box(mpc))[24:40]
    T = 8
    fixed = implicit_cpu.rollout(law, plant, mode_of, X0, T)
    einsum = implicit_cpu.rollout(law, plant, mode_of, X0, T,
                                  step=lambda pl, X, U, m, D=None: pl.step(X, U, m, D))
    differ = (fixed['commutation'] != einsum['commutation']).any(axis=0)
    print('summation orders: %d of %d trajectories differ in a commutation; largest state '
          'difference %.3g' % (differ.sum(), X0.shape[0],
                               np.nanmax(np.abs(fixed['x'] - einsum['x']))))
    assert (fixed['status'] == 0).all() and np.array_equal(fixed['status'], einsum['status'])
    assert differ.sum() <= 0.01 * X0.shape[0]
