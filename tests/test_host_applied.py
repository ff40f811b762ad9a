"""
The applied-input problem (explicit_hybrid_mpc_amd/applied.py) and the numpy mirror
of its audit (tests/applied_cpu.py), on the host: the substitution u_0 = ubar is exact algebra, the
reduced LP is the full LP with the bounds of u_0 fixed (an independent solver agrees), and the
status logic, histogram and worst-sample rule at their boundaries.
"""

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, applied, examples
from tests import applied_cpu as apc
from tests import helpers

EPS = np.finfo(np.float64).eps


def _can(kind):
    if kind == 'lin_quadratic':
        return examples.linear_mpc(0, cost='quadratic').compile()
    return helpers.make_instance(kind, 0).compile()


@pytest.fixture(scope='module')
def cans():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _can(kind)
        return made[kind]
    return get


def _abs_cost_terms(can, d, z, theta):
    """Sum of the magnitudes of every term of cost_value."""
    s = np.abs(can.c) @ np.abs(z)
    if can.quadratic:
        s += 0.5 * np.abs(z) @ np.abs(can.H[d]) @ np.abs(z)
        s += (np.abs(can.f0[d]) + np.abs(can.F[d]) @ np.abs(theta)) @ np.abs(z)
        s += 0.5 * np.abs(theta) @ np.abs(can.C[d]) @ np.abs(theta)
        s += np.abs(can.c1[d]) @ np.abs(theta) + abs(can.c0[d])
    return float(s)


@pytest.mark.parametrize('kind', ['di', 'lin', 'lin_quadratic', 'pwa_small'])
def test_the_substitution_is_exact_algebra(cans, kind):
    can = cans(kind)
    n_u, p, n = can.n_u, can.p, can.n
    red = applied.applied_input_problem(can)
    assert (red.n, red.p, red.m, red.n_delta) == (n - n_u, p + n_u, can.m, can.n_delta)
    assert red.n_u == 1 and red.N == can.N and red.delta_size == can.delta_size
    assert np.array_equal(red.deltas, can.deltas) and red.quadratic == can.quadratic
    assert np.array_equal(red.w, can.w) and red.input_tol == 0.
    if not can.quadratic:
        assert np.array_equal(red.cost_u, can.c[:n_u])
    rng = np.random.default_rng(7)
    for trial in range(20):
        d = int(rng.integers(can.n_delta))
        theta = rng.normal(size=p) * 2.
        ubar = rng.normal(size=n_u) * 3.
        zr = rng.normal(size=n - n_u) * 2.
        z = np.concatenate([ubar, zr])
        th2 = np.concatenate([theta, ubar])
        full = can.G[d] @ z - can.w[d] - can.S[d] @ theta
        mine = red.G[d] @ zr - red.w[d] - red.S[d] @ th2
        terms = np.abs(can.G[d]) @ np.abs(z) + np.abs(can.w[d]) + np.abs(can.S[d]) @ np.abs(theta)
        # the two forms add the same terms in two orders: n^2 eps sum |terms|
        assert (np.abs(full - mine) <= n ** 2 * EPS * terms).all()
        v_full = can.cost_value(d, z, theta)
        v_mine = red.cost_value(d, zr, th2) + float(red.cost_u @ ubar)
        assert abs(v_full - v_mine) <= n ** 2 * EPS * _abs_cost_terms(can, d, z, theta)
    # the relaxation shifts exactly the rows that touch u_0, by input_tol ||G_u row||_1
    tol = 0.125
    rel = applied.applied_input_problem(can, tol)
    assert np.array_equal(rel.w, can.w + tol * np.abs(can.G[:, :, :n_u]).sum(axis=2))
    assert np.array_equal((rel.w != can.w), (can.G[:, :, :n_u] != 0.).any(axis=2))
    assert np.array_equal(rel.G, red.G) and np.array_equal(rel.S, red.S)
    assert rel.input_tol == tol
    # rows on u_0 alone lose every entry of G' and stay in the problem
    zero_rows = ~(red.G != 0.).any(axis=2)
    assert (zero_rows & (can.G[:, :, :n_u] != 0.).any(axis=2)).any()


def test_refusals_of_the_problem(cans):
    can = cans('lin')
    wide = examples.linear_mpc(0).compile()
    wide.p = _capi.EHM_MAX_P - wide.n_u + 1            # one parameter too many
    with pytest.raises(ValueError, match='EHM_MAX_P'):
        applied.applied_input_problem(wide)
    with pytest.raises(ValueError):
        applied.applied_input_problem(can, -1.)

    class NoBatch:                  # an oracle without the batched P_theta (bnb.PrefixOracle)
        eps_a = eps_r = 1.
    with pytest.raises(_capi.EhmError):
        applied.oracle_gpu(NoBatch())
    assert applied.default_input_tol([[0.5, np.nan], [-0.25, np.inf]]) == 1e-7
    assert applied.default_input_tol([[3., -40.]]) == 1e-7 * 40.


@pytest.mark.parametrize('kind', ['di', 'lin'])
def test_an_independent_solver_agrees(cans, kind):
    """scipy's linprog (HiGHS) on the applied LP and on the full LP with the bounds of u_0 fixed
    to ubar: the same optimum and the same feasibility verdict.  Tolerance: the optimality
    tolerance scipy documents for HiGHS in the installed version (show_options('linprog',
    'highs'): ``ipm_optimality_tolerance`` default 1e-08, the only one by that name and the
    smaller of the defaults it lists; the feasibility tolerances default to 1e-07), relative to
    1 + |V|."""
    opt = pytest.importorskip('scipy.optimize')
    TOL = 1e-8
    can = cans(kind)
    n_u, p, n = can.n_u, can.p, can.n
    red = applied.applied_input_problem(can)
    mpc = helpers.make_instance(kind, 0)
    box = examples.theta_box(mpc)
    rng = np.random.default_rng(3)
    free = [(None, None)]
    verdicts = {True: 0, False: 0}
    for trial in range(24):
        theta = rng.uniform(-0.6, 0.6, p) * box
        rhs = can.w[0] + can.S[0] @ theta
        best = opt.linprog(can.c, A_ub=can.G[0], b_ub=rhs, bounds=free * n, method='highs')
        assert best.status == 0
        if trial % 3 == 0:
            ubar = best.x[:n_u].copy()                  # the optimal input: V_u = V*
        elif trial % 3 == 1:
            ubar = 0.5 * best.x[:n_u] + rng.normal(size=n_u) * 0.05
        else:
            ubar = best.x[:n_u] + rng.normal(size=n_u) * 10.       # far outside the input set
        fixed = [(float(v), float(v)) for v in ubar]
        full = opt.linprog(can.c, A_ub=can.G[0], b_ub=rhs, bounds=fixed + free * (n - n_u),
                           method='highs')
        th2 = np.concatenate([theta, ubar])
        mine = opt.linprog(red.c, A_ub=red.G[0], b_ub=red.w[0] + red.S[0] @ th2,
                           bounds=free * (n - n_u), method='highs')
        assert full.status in (0, 2) and mine.status == full.status, (trial, full.status,
                                                                       mine.status)
        verdicts[full.status == 0] += 1
        if full.status == 0:
            v_mine = mine.fun + float(red.cost_u @ ubar)
            assert abs(v_mine - full.fun) <= TOL * (1. + abs(full.fun))
            assert full.fun >= best.fun - TOL * (1. + abs(best.fun))
            if trial % 3 == 0:
                assert abs(full.fun - best.fun) <= TOL * (1. + abs(best.fun))
    assert verdicts[True] >= 8 and verdicts[False] >= 4


def test_pack_mirror():
    X = np.array([[1., 2.], [3., 4.], [5., 6.]])
    U = np.array([[0.5, -1.], [np.nan, 2.], [1., np.inf]])
    theta, k, bad = apc.pack(X, U, np.array([2., 0.25]))
    assert np.array_equal(theta, [[1., 2., 0.5, -1.], [3., 4., 0., 2.], [5., 6., 1., 0.]])
    assert np.array_equal(k, [0.75, 0.5, 2.]) and np.array_equal(bad, [0, 1, 1])


def test_fall_back_mirror():
    didx = np.array([0, 0, -1, 2, 1], np.int32)
    ju = np.array([1., np.inf, np.inf, np.inf, np.inf])
    du = np.array([0, -1, -1, -1, -1], np.int32)
    asked = []

    def solve_relaxed(idx):
        asked.append(idx.tolist())
        return np.array([5., np.inf, 7.]), np.array([3, -1, 0], np.int32)
    j2, d2, relaxed = apc.fall_back(didx, ju, du, solve_relaxed)
    assert asked == [[1, 3, 4]]             # x feasible, the exact problem without a commutation
    assert j2.tolist() == [1., 5., np.inf, np.inf, 7.] and d2.tolist() == [0, 3, -1, -1, 0]
    assert relaxed.tolist() == [0, 1, 0, 0, 1]
    assert ju[1] == np.inf and du[1] == -1  # the inputs are left as they were


def test_status_logic_on_both_sides_of_each_threshold():
    eps_a, eps_r, rtol = 0.5, 0.1, 1e-3
    vstar = np.array([1., 1., 1., 1., 1., 10., 10., 1., 1., 1., np.inf])
    slack = rtol * (1. + np.abs(vstar))
    bound = np.maximum(eps_a, eps_r * vstar)
    up = bound + slack                                  # the violation threshold on the gap
    gap = np.array([0., up[1], np.nextafter(up[2], np.inf), -slack[3],
                    np.nextafter(-slack[4], -np.inf), up[5], np.nextafter(up[5], np.inf) * 1.001,
                    np.nan, 0., 0., 0.])
    ju = vstar + gap
    ju[10] = 3.
    konst = np.zeros(11)
    didx = np.zeros(11, np.int32)
    didx_u = np.zeros(11, np.int32)
    no_law = np.zeros(11, np.int32)
    didx_u[8] = -1
    no_law[9] = 1
    didx[10] = -1
    vu, st, ratio = apc.statuses(ju, konst, vstar, didx, didx_u, no_law, eps_a, eps_r, rtol)
    # (vstar + gap) - vstar rounds: place the samples by the gap the mirror itself forms
    g = vu - vstar
    want = np.where(g > up, 1, np.where(~(g >= -slack), 2, 0))
    want[8], want[9], want[10] = 3, 4, 5
    assert np.array_equal(st, want)
    assert st[0] == 0 and st[2] == 1 and st[4] == 2 and st[6] == 1 and st[7] == 2
    assert bound[5] == 1. and bound[0] == 0.5           # the relative and the absolute branch
    # the order of precedence: infeasible over no_law over inadmissible over the judged ones
    every = np.full(3, -1, np.int32)
    _, st2, _ = apc.statuses(np.full(3, 99.), np.zeros(3), np.ones(3), np.array([-1, 0, 0]),
                             every, np.array([1, 1, 0]), eps_a, eps_r, rtol)
    assert st2.tolist() == [5, 4, 3]
    # the constant enters V_u before the gap is formed
    vu3, st3, _ = apc.statuses(np.array([1.]), np.array([2.]), np.array([1.]), [0], [0], [0],
                               eps_a, eps_r, rtol)
    assert vu3[0] == 3. and st3[0] == 1


def test_histogram_and_worst_sample():
    ids = np.arange(100, 110)
    status = np.array([0, 0, 1, 2, 3, 4, 5, 0, 1, 0], dtype=np.int32)
    ratio = np.array([0., 0.5, 2.5, -0.25, 9., 9., 9., 1., 2.5, 31.99 / 32.])
    counts, hist, best, worst = apc.summary(ids, status, ratio)
    assert counts.tolist() == [4, 2, 1, 1, 1, 1]
    want = np.zeros(33, np.int64)
    want[0] = 2                 # ratio 0 and the negative one
    want[16] = 1                # 0.5
    want[31] = 2                # 1.0 (the closed end) and 31.99 / 32
    want[32] = 2                # above 1
    assert np.array_equal(hist, want) and hist.sum() == 7
    assert best == 2.5 and worst == 102                 # a tie goes to the smaller id
    # statuses 3-5 never enter, whatever their ratio
    counts, hist, best, worst = apc.summary(ids[4:7], status[4:7], ratio[4:7])
    assert hist.sum() == 0 and best == -np.inf and worst == -1
    # a NaN ratio is binned in 0 and never wins
    counts, hist, best, worst = apc.summary(np.arange(3), np.array([2, 0, 0], np.int32),
                                            np.array([np.nan, 0.25, 0.25]))
    assert hist[0] == 1 and hist[8] == 2 and best == 0.25 and worst == 1
