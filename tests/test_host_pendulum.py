"""
The inverted-pendulum law and its guarded multi-rate plant on the host: the linearisation against
finite differences and hand-derived entries, the reference's commutation indexing against brute
force, every condensed block against the uncondensed big-M program (tests/pendulum_cpu.py), the
existing PWAMPC examples against the condensation before input-dependent regions existed, and the
plant's numpy step against a literal transcription of the reference's if-cascade.
"""

import itertools

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import examples, mpc_library, simulate
from tests import pendulum_cpu


@pytest.fixture(scope='module')
def law():
    return mpc_library.InvertedPendulumOnCart(4)


def _numeric_f(case, x, F, pars):
    xdd, thdd = mpc_library.pendulum_accelerations(case, x[1], x[3], F, pars, np.sin, np.cos)
    return np.array([x[2], x[3], xdd, thdd])


def test_linearization_matches_finite_differences():
    pars = mpc_library.pendulum_parameters()
    A_c, B_c, w_c = mpc_library.pendulum_linearization(pars)
    h = 1e-6
    for case in range(5):
        J = np.zeros((4, 4))
        for j in range(4):
            e = np.zeros(4)
            e[j] = h
            J[:, j] = (_numeric_f(case, e, 0., pars) - _numeric_f(case, -e, 0., pars)) / (2 * h)
        Jb = (_numeric_f(case, np.zeros(4), h, pars) - _numeric_f(case, np.zeros(4), -h, pars)) / (2 * h)
        assert np.allclose(A_c[case], J, rtol=1e-7, atol=1e-7)
        assert np.allclose(B_c[case], Jb, rtol=1e-7, atol=1e-7)
        assert np.allclose(w_c[case], _numeric_f(case, np.zeros(4), 0., pars), rtol=0, atol=1e-15)


def test_linearization_hand_entries():
    pars = mpc_library.pendulum_parameters()
    g, l, m, M = pars['g'], pars['l'], pars['m'], pars['M']
    A_c, B_c, w_c = mpc_library.pendulum_linearization(pars)
    for case in range(5):
        assert np.array_equal(A_c[case][0], [0, 0, 1, 0])
        assert np.array_equal(A_c[case][1], [0, 0, 0, 1])
    for case, (s, key) in enumerate(mpc_library.PENDULUM_CASES[:4]):
        mu = s * pars[key]
        assert B_c[case][2] == pytest.approx(1. / M, rel=1e-14)           # d^2x/dF = 1/M
        assert B_c[case][3] == pytest.approx(-1. / (M * l), rel=1e-14)
        # x'' at the origin: -mu (M + m) g / M ; theta'' = -x''/l
        assert w_c[case][2] == pytest.approx(-mu * (M + m) * g / M, rel=1e-14)
        assert w_c[case][3] == pytest.approx(mu * (M + m) * g / (M * l), rel=1e-14)
        # d x''/d theta = (N' D - N D') / D^2 with N = -mu (M + m) g, N' = -m g, D = M, D' = m mu
        assert A_c[case][2][1] == pytest.approx((-m * g * M + mu * (M + m) * g * m * mu) / M ** 2,
                                                rel=1e-13)
    assert np.array_equal(B_c[4], np.zeros(4)) and np.array_equal(w_c[4], np.zeros(4))
    assert A_c[4][3][1] == pytest.approx(g / l, rel=1e-14)
    assert np.array_equal(A_c[4][2], np.zeros(4))


def _brute_force(N):
    """Sequences of every 0/1 vector over the used entries with one 1 in each window
    delta[k*N : k*N+5] (lib/mpc_library.py:524, sum z[k] == 1)."""
    used = (N - 1) * N + 5
    bits = ((np.arange(2 ** used)[:, None] >> np.arange(used)[None, :]) & 1).astype(np.int8)
    ok = np.ones(bits.shape[0], dtype=bool)
    for k in range(N):
        ok &= bits[:, k * N:k * N + 5].sum(axis=1) == 1
    out = set()
    for b in bits[ok]:
        out.add(tuple(int(np.argmax(b[k * N:k * N + 5])) for k in range(N)))
    return out, int(ok.sum())


@pytest.mark.parametrize('N,count', [(2, 7), (3, 21), (4, 185)])
def test_reference_indexing_matches_brute_force(N, count):
    seqs, deltas = mpc_library.pendulum_sequences(N)
    brute, n_vectors = _brute_force(N)
    assert len(seqs) == count == len(brute) == n_vectors
    assert set(seqs) == brute
    for s, d in zip(seqs, deltas):
        assert d.size == 5 * N
        for k in range(N):
            assert np.array_equal(d[k * N:k * N + 5], np.eye(5)[s[k]])
        assert d[(N - 1) * N + 5:].sum() == 0.


def test_commutation_layouts(law):
    assert law.mode_sequences() == sorted(law.mode_sequences())
    can = law.compile()
    assert can.n_delta == 185 and can.deltas.shape == (185, 20)
    for s, d in zip(law.mode_sequences(), can.deltas):
        assert np.array_equal(d, law.sequence_to_delta(s))
        assert law.step0_mode(d) == s[0]
    k5 = mpc_library.InvertedPendulumOnCart(3, reference_indexing=False)
    assert len(k5.mode_sequences()) == 125
    d = k5.sequence_to_delta((4, 0, 2))
    assert np.flatnonzero(d).tolist() == [4, 5, 12] and k5.step0_mode(d) == 4
    with pytest.raises(ValueError, match='256'):
        mpc_library.InvertedPendulumOnCart(4, reference_indexing=False)
    with pytest.raises(ValueError, match='256'):
        mpc_library.InvertedPendulumOnCart(5)
    with pytest.raises(ValueError):
        law.sequence_to_delta((0, 0, 0, 0))          # z[0][4] = z[1][0] couples the steps


def test_sizes_fit_the_hybrid_engine(law):
    can = law.compile()
    assert can.quadratic and can.n == 4 and can.p == 4 and can.m == 168
    assert can.n + can.p + 1 <= 32 and can.m <= 256 and can.n_delta <= 256


def _thetas(law, rng):
    th = [rng.uniform(lo, hi) for lo, hi in law.sections()]
    th.append(rng.uniform(-1., 1., 4) * np.diag(law.D_x) * 0.3)
    small = rng.uniform(-1., 1., 4) * np.diag(law.D_x) * 0.05
    small[2] = 0.
    th.append(small)
    return th


def test_condensed_blocks_match_bigm_program(law):
    rng = np.random.default_rng(7)
    can = law.compile()
    n_feasible = n_thin = 0
    for theta in _thetas(law, rng):
        for d, delta in enumerate(can.deltas):
            if pendulum_cpu.interior_margin(can, d, theta) < 1e-7:
                # infeasible, or feasible without interior: some sequences pin a state to a
                # threshold (v = v_eps between a held and a sliding step); feasibility only
                f_c = pendulum_cpu.feasible(can.G[d], can.w[d] + can.S[d] @ theta)
                P, c, A_ub, b_ub, A_eq, b_eq = pendulum_cpu.bigm_program(law, theta, delta)
                assert f_c == pendulum_cpu.feasible(A_ub, b_ub, A_eq, b_eq), (theta, d)
                n_thin += f_c
                continue
            f_c, J_c, u_c, ok_c = pendulum_cpu.solve_condensed(can, d, theta)
            f_b, J_b, u_b, ok_b = pendulum_cpu.solve_bigm(law, theta, delta)
            assert f_c and f_b and ok_c and ok_b, (theta, d)
            n_feasible += 1
            assert abs(J_c - J_b) <= 1e-7 * max(1., abs(J_b)), (theta, d, J_c, J_b)
            assert np.allclose(u_c, u_b, rtol=0, atol=1e-6), (theta, d, u_c, u_b)
    assert n_feasible >= 20


def _condense_before_input_regions(mpc, seq, m_pad):
    """PWAMPC._condense as it was before mode regions could depend on the input."""
    n_x, n_u, N = mpc.n_x, mpc.n_u, mpc.N
    nU = N * n_u
    n = nU + (2 * N if mpc.cost_type == 'inf' else 0)
    Phi, Gam, om = mpc._prediction(seq)
    rows_G, rows_w, rows_S = [], [], []

    def add(Gz, wv, Sv):
        rows_G.append(Gz)
        rows_w.append(wv)
        rows_S.append(Sv)

    def pad(M_u):
        out = np.zeros((M_u.shape[0], n))
        out[:, :nU] = M_u
        return out
    for k in range(1, N + 1):
        add(pad(mpc.Gx @ Gam[k]), mpc.gx - mpc.Gx @ om[k], -mpc.Gx @ Phi[k])
    for k in range(N):
        M_u = np.zeros((mpc.Gu.shape[0], nU))
        M_u[:, k * n_u:(k + 1) * n_u] = mpc.Gu
        add(pad(M_u), mpc.gu.copy(), np.zeros((mpc.Gu.shape[0], n_x)))
    for k in (range(1, N + 1) if mpc.cost_type == 'inf' else ()):
        for sgn in (1., -1.):
            Gz = pad(sgn * mpc.Q @ Gam[k])
            Gz[:, nU + (k - 1)] = -1.
            add(Gz, -sgn * mpc.Q @ om[k], -sgn * mpc.Q @ Phi[k])
    for k in (range(N) if mpc.cost_type == 'inf' else ()):
        for sgn in (1., -1.):
            M_u = np.zeros((mpc.R.shape[0], nU))
            M_u[:, k * n_u:(k + 1) * n_u] = sgn * mpc.R
            Gz = pad(M_u)
            Gz[:, nU + N + k] = -1.
            add(Gz, np.zeros(mpc.R.shape[0]), np.zeros((mpc.R.shape[0], n_x)))
    for k in range(N):
        r = mpc.regions[seq[k]]
        if r is not None:
            Hx, hx = r
            add(pad(Hx @ Gam[k]), hx - Hx @ om[k], -Hx @ Phi[k])
    G, w, S = np.vstack(rows_G), np.concatenate(rows_w), np.vstack(rows_S)
    m = G.shape[0]
    if m < m_pad:
        G = np.vstack([G, np.zeros((m_pad - m, n))])
        w = np.concatenate([w, np.ones(m_pad - m)])
        S = np.vstack([S, np.zeros((m_pad - m, n_x))])
    return G, w, S


@pytest.mark.parametrize('build', [
    lambda: examples.double_integrator(3), lambda: examples.double_integrator(3, cost='quadratic'),
    lambda: examples.linear_mpc(0), lambda: examples.linear_mpc(1, cost='quadratic'),
    lambda: examples.pwa_mpc(0), lambda: examples.pwa_mpc(2, cost='quadratic'),
    lambda: examples.pwa4_mpc(0), lambda: examples.integrator_chain_mpc()])
def test_existing_examples_compile_bit_identically(build):
    mpc = build()
    can = mpc.compile()
    seqs = mpc.mode_sequences()
    m_pad = max(mpc.n_rows_per_sequence(s) for s in seqs)
    for d, s in enumerate(seqs):
        G, w, S = _condense_before_input_regions(mpc, s, m_pad)
        assert G.tobytes() == can.G[d].tobytes()
        assert w.tobytes() == can.w[d].tobytes()
        assert S.tobytes() == can.S[d].tobytes()
    if mpc.cost_type == 'inf':
        for pre in [(), (0,), tuple(seqs[-1][:2])]:
            a = mpc.condense_prefix(pre)
            b = mpc._condense_prefix_reference(pre)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_input_dependent_region_rows():
    """A 3-tuple region adds Hu at the step's input column; (Hx, 0, h) equals (Hx, h)."""
    mpc = examples.pwa_mpc(0, N=3, cost='quadratic')
    regs3 = [(r[0], np.zeros((r[0].shape[0], mpc.n_u)), r[1]) for r in mpc.regions]
    twin = mpc_library.PWAMPC(mpc.A, mpc.B, mpc.w, regs3, mpc.Gx, mpc.gx, mpc.Gu, mpc.gu,
                              mpc.Q, mpc.R, mpc.N, cost='quadratic')
    assert np.array_equal(twin.compile().G, mpc.compile().G)
    Hu = np.ones((1, mpc.n_u))
    regs3 = [(r[0], Hu, r[1]) for r in mpc.regions]
    twin = mpc_library.PWAMPC(mpc.A, mpc.B, mpc.w, regs3, mpc.Gx, mpc.gx, mpc.Gu, mpc.gu,
                              mpc.Q, mpc.R, mpc.N, cost='quadratic')
    a, b = twin.compile(), mpc.compile()
    off = mpc.N * (mpc.Gx.shape[0] + mpc.Gu.shape[0])
    for k in range(mpc.N):
        cols = slice(k * mpc.n_u, (k + 1) * mpc.n_u)
        assert np.allclose(a.G[:, off + k, cols] - b.G[:, off + k, cols], 1.)
    with pytest.raises(ValueError):
        simulate.Plant.from_mpc(twin)


# ---- the guarded plant ------------------------------------------------------------------------
def _threshold_states(law, rng):
    """(x, u) on, just inside and just outside each threshold of the cascade."""
    out = []
    ve = law.v_eps
    for v0 in (ve, -ve):
        for v in (v0, np.nextafter(v0, np.inf), np.nextafter(v0, -np.inf), v0 * (1 + 1e-9),
                  v0 * (1 - 1e-9)):
            x = rng.uniform(-1., 1., 4) * np.diag(law.D_x)
            x[2] = v
            out.append((x, rng.uniform(-20., 20.)))
    for i, thr in ((2, law.a_eps), (3, -law.a_eps)):
        for _ in range(4):
            x = rng.uniform(-1., 1., 4) * np.diag(law.D_x)
            x[2] = rng.uniform(-ve, ve) * 0.999
            a, b, c = law.A_c[i][2], law.B_c[i][2], law.w_c[i][2]
            u0 = (thr - a.dot(x) - c) / b
            cands = [u0]
            for direction in (np.inf, -np.inf):
                u = u0
                for _ in range(4):
                    u = np.nextafter(u, direction)
                    cands.append(u)
            # the exact threshold, where one exists among neighbouring doubles
            for u in cands:
                out.append((x.copy(), float(u)))
    return out


def test_guarded_plant_matches_reference_cascade(law):
    plant = simulate.Plant.from_mpc(law)
    assert isinstance(plant, simulate.GuardedPlant)
    assert plant.substeps == 10 and plant.n_modes == 5 and plant.default_mode == 4
    rng = np.random.default_rng(3)
    A, B, w = plant.A, plant.B[:, :, 0], plant.w
    states = _threshold_states(law, rng)
    X = np.array([s[0] for s in states])
    U = np.array([[s[1]] for s in states])
    xn, modes = plant.plant_step(X, U)
    seen = set()
    on_threshold = 0
    for q, (x, u) in enumerate(states):
        x_ref, case = pendulum_cpu.cascade_step(law, A, B, w, x, u)
        assert modes[q] == case, (q, x, u)
        assert np.allclose(xn[q], x_ref, rtol=1e-14, atol=1e-16)
        seen.add(case)
        acc = [law.A_c[i][2].dot(x) + law.B_c[i][2] * u + law.w_c[i][2] for i in (2, 3)]
        on_threshold += int(abs(x[2]) == law.v_eps or acc[0] == law.a_eps or acc[1] == -law.a_eps)
    assert seen == {0, 1, 2, 3, 4}
    assert on_threshold >= 2


def test_guarded_step_is_a_fixed_order_sum(law):
    """The plant step equals its scalar transcription bit for bit (the device's order)."""
    plant = simulate.Plant.from_mpc(law)
    rng = np.random.default_rng(5)
    X = rng.uniform(-1., 1., (50, 4)) * np.diag(law.D_x)
    X[:25, 2] *= 1e-3
    U = rng.uniform(-20., 20., (50, 1))
    xn, m = plant.plant_step(X, U)
    for q in range(50):
        mm = int(m[q])
        for i in range(4):
            s = 0.
            for c in range(4):
                s = s + plant.A[mm, i, c] * X[q, c]
            s = s + plant.B[mm, i, 0] * U[q, 0]
            assert (s + plant.w[mm, i]) == xn[q, i]
    x10 = plant.step(X, U)
    x = X
    for _ in range(10):
        x, _ = plant.plant_step(x, U)
    assert np.array_equal(x10, x)


@pytest.mark.parametrize('T', [0.5, 1.0, 1.5, 2.0])
def test_controller_schedule_is_every_substeps(law, T):
    calls, times = simulate.reference_call_steps(T, law.T_s_plant, law.T_s)
    assert np.array_equal(calls, np.arange(0, len(times), 10))


def test_reference_schedule_drifts_after_2_3_seconds(law):
    """From t = 2.4 s on the reference's rule t - t_last >= T_s - eps misses a call by one plant
    step (2.4 - 2.3 < 0.1 - eps in floating point): Simulator refuses such T for a guarded plant."""
    calls, times = simulate.reference_call_steps(3.0, law.T_s_plant, law.T_s)
    assert calls[23] == 230 and calls[24] == 241


def test_simulator_refuses_a_drifting_schedule(law):
    import types
    fake = types.SimpleNamespace(mpc=law, T_s=law.T_s, _rollout_plant=None)
    with pytest.raises(ValueError, match='every 10'):
        simulate.Simulator(fake, 3.0).run(np.zeros(4))


def test_guarded_plant_refuses_noise(law):
    plant = simulate.Plant.from_mpc(law)
    with pytest.raises(ValueError, match='guarded'):
        simulate.rollout_implicit(None, plant, np.zeros((1, 4)), 3, noise=object())


def test_pendulum_sections_cover_the_box(law):
    secs = examples.pendulum_sections(law)
    vol = sum(np.prod(V.max(0) - V.min(0)) for V in secs)
    assert vol == pytest.approx(np.prod(2 * np.diag(law.D_x)), rel=1e-12)
    assert secs[0][:, 2].min() == law.v_eps and secs[1][:, 2].max() == -law.v_eps
