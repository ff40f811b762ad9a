"""
The device loop around the implicit law (``rollout(..., on_device=True)``,
csrc/ehm_implicit.hip) against its numpy mirror (tests/implicit_cpu.py) driven by
``oracle.gpu.solve_pt``: every record and output bit for bit.  That is derivable, not a tolerance:
the two solves of a step are the launches ``solve_pt`` makes (same kernel instance, same
(z, commutation) inputs), the generator is counter-based, and every sum of the step kernels runs in
the mirror's order without FMA.  Each case asserts that no solve stalled, in phase one or in the
point solve (the one place the device loop and ``solve_pt`` may part: the host path repeats a
stalled LP on the generation-1 kernels).

Then: one-step replay through ``solve_pt``, the device loop against the host loop, and
``simulate.compare(..., implicit_on_device=True)``.
"""

import numpy as np
import pytest

from tests import helpers, implicit_cpu

pytestmark = pytest.mark.gpu

FIELDS = ('x', 'u', 'commutation', 'mode', 'steps', 'status', 'cost', 'u_norm_sum',
          'max_violation')
NOISE_FIELDS = ('v', 'e', 'w')
EPS = np.finfo(np.float64).eps


def _law(oracle):
    def law(Z):
        _, u0, didx = oracle.gpu.solve_pt(Z)
        return u0, didx
    return law


def _mode_of(oracle):
    return [oracle.mpc.step0_mode(dl) for dl in oracle.canonical.deltas]


def _assert_equal(res, ref, noisy, guarded=False):
    print('stalled pairs %d (phase one %d), trajectories %s' % (
        res.n_stalled_pairs, res.n_stalled_phase_one, np.flatnonzero(res.stalled).tolist()))
    assert res.n_stalled_pairs == 0 and res.n_stalled_phase_one == 0 and not res.stalled.any()
    for k in FIELDS + (NOISE_FIELDS if noisy else ()):
        if k == 'mode' and guarded:
            assert res.mode is None
            continue
        a, b = getattr(res, k), ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), k
    assert np.array_equal(res.x_final, ref['x_final'])


@pytest.fixture(scope='module')
def cwh():
    from explicit_hybrid_mpc_amd import examples, simulate
    from explicit_hybrid_mpc_amd.explicit import ImplicitMPC
    full_set, _, oracle = examples.example('cwh_z', abs_frac=0.5, rel_err=2.0)
    half = examples.theta_box(oracle.mpc)
    X0 = implicit_cpu.cwh_states(half)      # states from which no solve stalls
    plant = simulate.Plant.from_mpc(oracle.mpc)
    yield oracle, ImplicitMPC(oracle), plant, X0
    oracle.close()


T_CWH = 60


def test_a_cwh_nominal(cwh):
    oracle, im, plant, X0 = cwh
    res = im.rollout(X0, T_CWH, on_device=True, record=True)
    ref = implicit_cpu.rollout(_law(oracle), plant, _mode_of(oracle), X0, T_CWH)
    _assert_equal(res, ref, False)
    assert (res.status == 3).any() and (res.status == 0).any()
    assert res.lp_solves[0] == 512 * oracle.canonical.n_delta * T_CWH
    assert 0 < res.lp_solves[1] < res.lp_solves[0] and res.seconds > 0


@pytest.fixture(scope='module')
def cwh_noisy(cwh):
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    oracle, im, plant, X0 = cwh
    model = NoiseModel.from_mpc(oracle.mpc)
    res = im.rollout(X0, T_CWH, on_device=True, record=True, noise=model, seed=0, traj0=0)
    return model, res


def test_b_cwh_noisy_and_split(cwh, cwh_noisy):
    oracle, im, plant, X0 = cwh
    model, res = cwh_noisy
    ref = implicit_cpu.rollout(_law(oracle), plant, _mode_of(oracle), X0, T_CWH, noise=model,
                               seed=0, traj0=0)
    _assert_equal(res, ref, True)
    halves = [im.rollout(X0[a:a + 256], T_CWH, on_device=True, record=True, noise=model, seed=0,
                         traj0=a) for a in (0, 256)]
    for k in FIELDS + NOISE_FIELDS:
        axis = 1 if getattr(res, k).ndim > 1 and k not in ('x_final',) else 0
        both = np.concatenate([getattr(h, k) for h in halves], axis=axis)
        assert np.array_equal(both, getattr(res, k), equal_nan=both.dtype.kind == 'f'), k
    assert sum(h.n_stalled_pairs for h in halves) == 0


def test_b_one_step_replay(cwh, cwh_noisy):
    """Every recorded (t, q): solve_pt at x_t + v_t returns the recorded input and commutation."""
    oracle, im, plant, X0 = cwh
    _, res = cwh_noisy
    live = res.commutation >= 0                                   # [T, n]
    z = res.x[:-1].copy()
    z[1:] += res.v[1:]
    _, u0, didx = oracle.gpu.solve_pt(z[live])
    assert np.array_equal(didx, res.commutation[live])
    assert np.array_equal(u0, res.u[live])


def test_c_pwa_two_modes_with_given_d_and_v():
    from explicit_hybrid_mpc_amd import examples, simulate
    from explicit_hybrid_mpc_amd.explicit import ImplicitMPC
    from explicit_hybrid_mpc_amd.oracle import Oracle
    mpc = helpers.make_instance('pwa_small', 0)
    oracle = Oracle(mpc, 1., 1.)
    try:
        plant = simulate.Plant.from_mpc(mpc)
        assert plant.n_modes == 2
        half = examples.theta_box(mpc)
        rng = np.random.default_rng(5)
        n, T = 256, 12
        X0 = rng.uniform(-1.15, 1.15, (n, half.size)) * half
        v = rng.uniform(-0.02, 0.02, (T, n, half.size)) * half
        d = rng.uniform(-0.01, 0.01, (T, n, plant.n_d)) if plant.n_d else None
        res = ImplicitMPC(oracle).rollout(X0, T, d=d, v=v, on_device=True, record=True)
        ref = implicit_cpu.rollout(_law(oracle), plant, _mode_of(oracle), X0, T, d=d, v=v)
        _assert_equal(res, ref, False)
        assert ((res.status == 2) | (res.status == 3)).any() and (res.status == 0).any()
        assert len(set(res.mode[res.mode >= 0].tolist())) == 2
    finally:
        oracle.close()


def test_d_pendulum_guarded():
    from explicit_hybrid_mpc_amd import mpc_library, simulate
    from explicit_hybrid_mpc_amd.explicit import ImplicitMPC
    from explicit_hybrid_mpc_amd.oracle import Oracle
    law = mpc_library.InvertedPendulumOnCart(4)
    oracle = Oracle(law, 1., 1.)
    try:
        plant = simulate.Plant.from_mpc(law)
        assert plant.guarded
        rng = np.random.default_rng(2)
        cand = rng.uniform(-1, 1, (1024, 4)) * np.diag(law.D_x) * 0.5
        _, _, didx = oracle.gpu.solve_pt(cand)
        X0 = cand[didx >= 0][:64]
        assert X0.shape[0] == 64
        res = ImplicitMPC(oracle).rollout(X0, 20, on_device=True, record=True)
        ref = implicit_cpu.rollout(_law(oracle), plant, _mode_of(oracle), X0, 20)
        _assert_equal(res, ref, False, guarded=True)
        assert (res.steps > 0).all()
    finally:
        oracle.close()


def test_e_double_integrator_inf_norm():
    from explicit_hybrid_mpc_amd import examples, simulate
    from explicit_hybrid_mpc_amd.explicit import ImplicitMPC
    from explicit_hybrid_mpc_amd.oracle import Oracle
    mpc = examples.double_integrator(3)
    oracle = Oracle(mpc, 1., 1.)
    try:
        assert oracle.canonical.n_delta == 1
        plant = simulate.Plant.from_mpc(mpc)
        assert plant.cost == 'inf'
        half = examples.theta_box(mpc)
        X0 = np.random.default_rng(9).uniform(-1.1, 1.1, (300, half.size)) * half
        res = ImplicitMPC(oracle).rollout(X0, 25, on_device=True, record=True)
        ref = implicit_cpu.rollout(_law(oracle), plant, _mode_of(oracle), X0, 25)
        _assert_equal(res, ref, False)
        assert (res.status == 0).any()
    finally:
        oracle.close()


def test_against_the_host_loop(cwh):
    """
    on_device=False against on_device=True from the same inputs (case a): equal status and steps;
    until the first step at which a trajectory's commutations differ its states agree to
    8 eps (|A||x| + |B||u| + |w|) componentwise (the rounding bound of an (n_x + n_u + 1)-term
    sum: the host einsum has no fixed order); at most 1 % of the trajectories ever differ in a
    commutation.  The CPU side -- OracleCPU in closed loop under both summation orders on a part
    of these states -- is tests/test_host_implicit_device.py::
    test_summation_order_does_not_switch_commutations_on_cwh_z.
    """
    oracle, im, plant, X0 = cwh
    host = im.rollout(X0, T_CWH, record=True)
    dev = im.rollout(X0, T_CWH, on_device=True, record=True)
    assert dev.n_stalled_pairs == 0
    differ = (host.commutation != dev.commutation)
    first = np.where(differ.any(axis=0), differ.argmax(axis=0), T_CWH)      # [n]
    n_diff = int((first < T_CWH).sum())
    # one set of dynamics whatever the mode (off / piece 0 / piece 1 of the input)
    assert all(np.array_equal(plant.A[m], plant.A[0]) and np.array_equal(plant.B[m], plant.B[0])
               and np.array_equal(plant.w[m], plant.w[0]) for m in range(plant.n_modes))
    A, B, w = np.abs(plant.A[0]), np.abs(plant.B[0]), np.abs(plant.w[0])
    worst, within = 0., True
    for t in range(T_CWH):
        sel = (first >= t) & ~np.isnan(host.x[t + 1]).any(axis=1) \
            & ~np.isnan(dev.x[t + 1]).any(axis=1)
        # up to and including the step whose commutations are still equal
        sel &= first > t
        if not sel.any():
            continue
        bound = 8 * EPS * (np.abs(host.x[t, sel]) @ A.T + np.abs(host.u[t, sel]) @ B.T + w)
        err = np.abs(host.x[t + 1, sel] - dev.x[t + 1, sel])
        within = within and bool((err <= bound).all())
        with np.errstate(divide='ignore', invalid='ignore'):
            worst = max(worst, float(np.max(np.where(err > 0, err / bound, 0.))))
    print('host vs device loop: %d of %d trajectories differ in a commutation; worst state '
          'difference / bound = %.3g' % (n_diff, X0.shape[0], worst))
    assert np.array_equal(host.status, dev.status)
    assert np.array_equal(host.steps, dev.steps)
    assert n_diff <= 0.01 * X0.shape[0]
    assert within


def test_compare_with_the_implicit_law_on_the_device(cwh):
    from explicit_hybrid_mpc_amd import simulate
    from explicit_hybrid_mpc_amd.explicit import ExplicitMPC
    from oracle import geometry
    from explicit_hybrid_mpc_amd import examples
    oracle, im, plant, X0 = cwh
    full_set = examples.box_vertices(examples.theta_box(oracle.mpc))
    roots, _ = geometry.delaunay_simplices(full_set)
    flat = oracle.gpu.partition(np.array(roots), action='ecc')
    ex = ExplicitMPC(flat, oracle)
    try:
        a = simulate.compare(ex, im, X0, T_CWH)
        b = simulate.compare(ex, im, X0, T_CWH, implicit_on_device=True)
        assert set(a) == set(b)
        assert a['both_ok'] == b['both_ok'] and a['n'] == b['n']
        assert b['implicit'].n_stalled_pairs == 0
    finally:
        ex.close()
