"""
The streaming wide kernels (ehm_k3.hip + ehm_ipm3.h: one workgroup of four wavefronts per LP, the
constant block streamed from L2, normal matrix on the matrix cores) against the CPU oracle.  The
library runs them for every law the LDS-resident family (ehm_k4.hip) refuses, and since k2_pick
prefers that family no other module reaches them.  Five laws that do, with no environment switch
for the routing (tests/helpers.py, STREAMING_WIDE_ROWS):

  A  'chain' with nothing eliminated: 57 factorised columns   8 slots   4-tile normal matrix
  B  30 x 520, handle WITH eliminated columns                 16 slots  3 tiles
  C  50 x 520, the largest shape, eliminated columns too      16 slots  4 tiles
  D  40 x 440, nothing eliminated: refused on LDS             8 slots   3 tiles
  E  15 x 515, 32 commutations (segment walk, hybrid engine)  16 slots

so both compiled instances (ehm_k3_api_2 / _4), both tile forms, handles with and without
eliminated columns, one and many commutations.  What each handle really runs is asserted through
ehm_problem_batch_kernel.  D4 is D's law on a default handle, which k4 takes: the partner of the
cross-family comparison.

Bars: optimal values within 1e-7 (1 + |value|) of the CPU oracle (HiGHS), verdicts, statuses and
trees equal, vertices bit-equal.  The inter-family differences are printed, not asserted (DESIGN.md
section 5 quotes them).
"""

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

RTOL = 1e-7
MARGIN = 1e-6         # the suite's margin: verdicts are compared where |t*| exceeds it
KINDS = ('point', 'feas', 'min_simplex', 'slack')
K3_THREADS, K3_COLUMNS = 256, 64
# sub-forest per case: (root slice, abs_frac of eps_a_rule, eps_r, nodes the CPU partition has)
FOREST = {'A': (slice(None, None, 160), 0.5, 1.0, 133),
          'B': (slice(0, 4), 0.2, 0.1, 278),
          'C': (slice(0, 4), 0.2, 0.1, 420),
          'D': (slice(0, 4), 0.2, 0.1, 288)}


def row_of(name):
    return helpers.STREAMING_CHAIN if name == 'A' else helpers.STREAMING_WIDE_ROWS[name]


def law_of(name):
    if name == 'A':
        return helpers.make_instance('chain', 0)
    return helpers.persistent_width_instance(row_of(name))


def within(got, ref):
    return abs(got - ref) <= RTOL * (1 + abs(ref))


class Case:
    """One law: its handle, the CPU oracle and the CPU references the tests share."""

    def __init__(self, name):
        from oracle.oracle_cpu import OracleCPU
        self.name, self.row = name, row_of(name)
        self.mpc = law_of(name)
        self.can = self.mpc.compile()
        self.gp = helpers.make_gp(self.row, self.can, 0.05, 0.1)
        self.orc = OracleCPU(self.mpc, 0.05, 0.1)
        self.delta = self.orc.deltas[0]
        self._simplices = None
        self._forest = None

    def simplices(self):
        """24 random simplices, the oracle's vertex costs, slacks and minima over them."""
        if self._simplices is None:
            orc = self.orc
            R = helpers.random_simplices(self.mpc, np.random.default_rng(1), 24)
            Vbar = np.array([[orc.P_theta_delta(v, self.delta)[1] for v in Rk] for Rk in R])
            t = np.array([orc.slack(R[k], Vbar[k], 0)[0] for k in range(len(R))])
            Jmin = np.array([orc._solve(orc.models[0].lp_min_over_simplex(Rk)).fun for Rk in R])
            self._simplices = R, Vbar, t, Jmin
        return self._simplices

    def forest(self):
        """(roots, locations, eps_a, eps_r, CPU partition) of the case's sub-forest."""
        if self._forest is None:
            from oracle.oracle_cpu import OracleCPU
            from oracle.partition_cpu import PartitionCPU
            pick, frac, eps_r, _ = FOREST[self.name]
            eps_a = helpers.eps_a_rule(self.mpc, frac)
            roots, locs = helpers.roots_of(self.mpc)
            roots, locs = list(roots[pick]), list(locs[pick])
            cpu = PartitionCPU(OracleCPU(self.mpc, eps_a, eps_r))
            cpu.run(roots, locs, 'ecc')
            self._forest = roots, locs, eps_a, eps_r, cpu
        return self._forest


@pytest.fixture(scope='module', params=['A', 'B', 'C', 'D'])
def case(request):
    c = Case(request.param)
    yield c
    c.gp.close()


def test_batches_route_to_the_streaming_instance(case):
    can, gp, row = case.can, case.gp, case.row
    lay = gp.layout()
    assert (lay['nE'] == 0) == row[8]        # B and C run k3 on a handle with eliminated columns
    for kind in KINDS:
        assert gp.batch_kernel(kind) == ('k3', K3_COLUMNS, row[3], K3_THREADS), kind
    assert gp.batch_kernel(3) == gp.batch_kernel('slack')
    print('\n%s: %d x %d, p %d, %d columns eliminated -> %s'
          % (case.name, can.n, can.G[0].shape[0], can.p, lay['nE'], gp.batch_kernel()))


def test_point_lps_match_oracle(case):
    """k3_point_batch, optimisation form: optimal values, statuses, iteration counts, and the
    first input through the cost (the lexicographic stage is another module's)."""
    from scipy.optimize import linprog
    from explicit_hybrid_mpc_amd import examples
    mpc, can, gp, orc = case.mpc, case.can, case.gp, case.orc
    rng = np.random.default_rng(11)
    half = examples.theta_box(mpc)
    p = half.size
    V = examples.box_vertices(half)
    theta = np.vstack([V[::max(1, len(V) // 8)], rng.uniform(-1, 1, (24, p)) * half])
    assert theta.shape[0] == 32
    J, u0, status, iters = gp.solve_ptd(theta, case.delta)
    print('\n%s: point LPs, %.1f iterations on average, %d at most'
          % (case.name, iters.mean(), iters.max()))
    assert (status == 0).all()
    for k in range(theta.shape[0]):
        J_ref = orc.P_theta_delta(theta[k], case.delta)[1]
        assert within(J[k], J_ref), (k, J[k], J_ref)
    assert iters.max() <= 30
    # u0 belongs to an optimal solution: re-solve with u0 fixed and compare the optimum
    Aeq = np.zeros((can.n_u, can.n))
    Aeq[:, :can.n_u] = np.eye(can.n_u)
    for k in range(0, theta.shape[0], 4):
        h = can.w[0] + can.S[0] @ theta[k]
        res = linprog(can.c, A_ub=can.G[0], b_ub=h + 1e-9, A_eq=Aeq, b_eq=u0[k],
                      bounds=(None, None), method='highs')
        assert res.status == 0, k
        assert abs(res.fun - J[k]) <= 1e-6 * (1 + abs(J[k])), (k, res.fun, J[k])


def test_feasibility_verdicts_match_oracle(case):
    """k3_point_batch, feasibility form, in- and outside the feasible set."""
    from explicit_hybrid_mpc_amd import examples
    mpc, gp, orc = case.mpc, case.gp, case.orc
    half = examples.theta_box(mpc)
    theta = np.random.default_rng(11).uniform(-1, 1, (32, half.size)) * half * 2.0
    feas, _ = gp.feasible_ptd(theta, case.delta)
    ref = np.array([orc.P_theta_delta(t, case.delta, check_feasibility=True) for t in theta])
    print('\n%s: %d of 32 feasible (oracle %d)' % (case.name, feas.sum(), ref.sum()))
    assert feas.any() and (~feas).any()
    assert np.array_equal(feas, ref)
    # clearly infeasible: a status, never a value
    far = (50 * half)[None]
    assert not gp.feasible_ptd(far, case.delta)[0][0]
    assert gp.solve_ptd(far, case.delta)[2][0] != 0
    J, _, didx = gp.solve_pt(far)
    assert didx[0] == -1 and np.isinf(J[0])


def test_empty_batches(case):
    gp, p, n_u = case.gp, case.can.p, case.can.n_u
    J, u0, st, it = gp.solve_ptd(np.zeros((0, p)))
    assert J.shape == (0,) and u0.shape == (0, n_u) and st.shape == (0,) and it.shape == (0,)
    assert gp.feasible_ptd(np.zeros((0, p)))[0].shape == (0,)
    assert gp.solve_pt(np.zeros((0, p)))[2].shape == (0,)
    R0, V0 = np.zeros((0, p + 1, p)), np.zeros((0, p + 1))
    assert gp.v_r(R0)[0].shape == (0,)
    assert gp.slack(R0, V0)[0].shape == (0,)
    assert gp.bar_e(R0, V0)[0].shape == (0,)
    assert gp.min_simplex(R0)[0].shape == (0,)
    assert gp.bar_d(R0, V0, np.ones((0, case.delta.size)))[0].shape == (0,)


def test_simplex_lps_match_oracle(case):
    """k3_simplex_batch in its three modes (slack, minimum over the simplex, simplex feasibility
    behind V_R), and V_R / bar_E_delta_R on the same simplices."""
    gp, orc = case.gp, case.orc
    R, Vbar, t_ref, Jmin_ref = case.simplices()
    n, na = R.shape[0], R.shape[1]
    t, alpha, status = gp.slack(R, Vbar, case.delta)
    assert (status == 0).all()
    Jmin, st2 = gp.min_simplex(R, case.delta)
    assert (st2 == 0).all()
    for k in range(n):
        assert within(t[k], t_ref[k]), (k, t[k], t_ref[k])
        assert abs(alpha[k].sum() - 1) < 1e-9 and (alpha[k] > -1e-9).all(), k
        assert within(Jmin[k], Jmin_ref[k]), (k, Jmin[k], Jmin_ref[k])
    assert (t > 0).any() and (t < 0).any()
    # V_R: the one commutation is feasible on every vertex; the vertex costs are the oracle's
    didx, vJ, _ = gp.v_r(R)
    for k in range(n):
        delta, vx = orc.V_R(R[k])
        assert delta is not None and didx[k] == 0, k
        for j in range(na):
            assert within(vJ[k, j], vx[j][1]), (k, j)
    # bar_E_delta_R where the slack is off the threshold by the suite's margin
    closed, tb = gp.bar_e(R, Vbar)
    clear = np.abs(t_ref) > MARGIN
    print('\n%s: %d of %d simplices within %g of the threshold are left out of the verdicts'
          % (case.name, n - clear.sum(), n, MARGIN))
    assert (n - clear.sum()) * 24 <= n
    ref = np.array([orc.bar_E_delta_R(R[k], Vbar[k]) for k in range(n)])
    assert np.array_equal(closed[clear], ref[clear])
    assert np.array_equal(tb[clear] > 0, t_ref[clear] > 0)


def test_sub_forest_identical_to_cpu_partition(case):
    """k3_vertex_solve, k3_lcss_decide, k3_lcss_expand and the midpoint table inside the sweeps:
    node for node against the CPU partition, suboptimality test to sign only and in full."""
    from oracle import geometry
    gp = case.gp
    roots, locs, eps_a, eps_r, cpu = case.forest()
    assert len(cpu.nodes) == FOREST[case.name][3]
    total = sum(geometry.simplex_volume(R) for R in roots)
    gp.set_eps(eps_a, eps_r)
    try:
        for decide_full in (0, 1):
            gp.set_option('decide_full', decide_full)
            flat = gp.partition(np.array(roots), action='ecc')
            # the streaming family has no persistent kernel: level-synchronous sweeps
            assert flat.info['persist_kernel'][0] == 'none'
            assert flat.info['decide_launches'] > 1
            loc = flat.locations(locs)
            assert set(loc) == set(cpu.nodes.keys())
            for k, name in enumerate(loc):
                ref = cpu.nodes[name]
                assert np.array_equal(flat.vertices[k], ref['vertices']), name
                assert flat.is_leaf(k) == ref['leaf'], name
                assert bool(flat.flags[k] & 1) == ref['is_epsilon_suboptimal'], name
                assert np.allclose(flat.vertex_costs[k], ref['vertex_costs'], rtol=RTOL,
                                   atol=RTOL), name
            assert abs(flat.info['volume_closed'] - total) <= 1e-9 * total
            assert min(cpu.min_margin, flat.info['min_margin']) > MARGIN
    finally:
        gp.set_option('decide_full', 0)
        gp.set_eps(0.05, 0.1)


# ---- D on the streaming family against the same law on the LDS-resident family -------------------
def same_tree(a, b, locs):
    la = {name: k for k, name in enumerate(a.locations(locs))}
    lb = {name: k for k, name in enumerate(b.locations(locs))}
    assert set(la) == set(lb)
    ka = np.array([la[name] for name in la])
    kb = np.array([lb[name] for name in la])
    assert np.array_equal(a.vertices[ka], b.vertices[kb])
    assert np.array_equal(a.left[ka] < 0, b.left[kb] < 0)
    assert np.array_equal(a.flags[ka] & 1, b.flags[kb] & 1)
    ref = b.vertex_costs[kb]
    assert (np.abs(a.vertex_costs[ka] - ref) <= RTOL * (1 + np.abs(ref))).all()


def test_streaming_and_lds_resident_families_agree():
    """One law, two handles: nothing eliminated (k3, case D) and the default (k4).  The whole
    partition is grown by k3's sweeps, k4's persistent launch and k4's sweeps; the LP batches of
    the tests above run on both.  Discrete results are equal; the differences of the optima are
    printed only."""
    from explicit_hybrid_mpc_amd import examples
    rows = helpers.STREAMING_WIDE_ROWS
    mpc = law_of('D')
    can = mpc.compile()
    eps_a, eps_r = helpers.eps_a_rule(mpc, 0.2), 0.1
    roots, locs = helpers.roots_of(mpc)
    roots, locs = np.array(roots), list(locs)
    assert len(roots) == 22
    g3 = helpers.make_gp(rows['D'], can, eps_a, eps_r)
    g4 = helpers.make_gp(rows['D4'], can, eps_a, eps_r)
    try:
        assert g4.layout()['nd0'] == 20
        for kind in KINDS:
            assert g3.batch_kernel(kind) == ('k3', K3_COLUMNS, 8, K3_THREADS), kind
            assert g4.batch_kernel(kind) == ('k4', 48, 8, 512), kind
        t3 = g3.partition(roots, action='ecc')
        assert t3.info['persist_kernel'][0] == 'none' and t3.info['decide_launches'] > 1
        t4 = g4.partition(roots, action='ecc')
        assert t4.info['persist_kernel'] == ('k4', 48, 48, 8)
        assert t4.info['decide_launches'] == 1
        t4s = g4.partition(roots, action='ecc', engine=0)
        assert t4s.info['persist_kernel'][0] == 'none' and t4s.info['decide_launches'] > 1
        print('\nD: %d nodes, min margin %.3g (k3 sweeps), %.3g (k4 persistent), %.3g (k4 sweeps)'
              % (t3.n_nodes, t3.info['min_margin'], t4.info['min_margin'],
                 t4s.info['min_margin']))
        same_tree(t3, t4, locs)
        same_tree(t4s, t4, locs)
        # the LP batches of the tests above on both handles
        half = examples.theta_box(mpc)
        p = half.size
        rng = np.random.default_rng(11)
        V = examples.box_vertices(half)
        theta = np.vstack([V[::2], rng.uniform(-1, 1, (24, p)) * half])
        theta2 = np.random.default_rng(11).uniform(-1, 1, (32, p)) * half * 2.0
        R = helpers.random_simplices(mpc, np.random.default_rng(1), 24)
        out = {}
        for fam, g in (('k3', g3), ('k4', g4)):
            J, _, st, it = g.solve_ptd(theta, can.deltas[0])
            feas, _ = g.feasible_ptd(theta2, can.deltas[0])
            Vbar, stv = g.solve_ptd(R.reshape(-1, p), can.deltas[0])[0::2]
            out[fam] = dict(J=J, st=st, it=it, feas=feas, Vbar=Vbar, stv=stv)
        Vbar = out['k3']['Vbar'].reshape(R.shape[0], p + 1)
        for fam, g in (('k3', g3), ('k4', g4)):
            t, _, sts = g.slack(R, Vbar, can.deltas[0])
            Jmin, st2 = g.min_simplex(R, can.deltas[0])
            closed, _ = g.bar_e(R, Vbar)
            out[fam].update(t=t, sts=sts, Jmin=Jmin, st2=st2, closed=closed)
        a, b = out['k3'], out['k4']
        for key in ('st', 'stv', 'sts', 'st2', 'feas', 'closed'):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a['t'] > 0, b['t'] > 0)
        for key in ('J', 'Vbar', 't', 'Jmin'):
            print('D: largest relative difference of %s between k3 and k4: %.3g'
                  % (key, np.max(np.abs(a[key] - b[key]) / (1 + np.abs(b[key])))))
        print('D: iterations per point LP, k3 %.2f, k4 %.2f' % (a['it'].mean(), b['it'].mean()))
    finally:
        g3.close()
        g4.close()


# ---- E: many commutations on the streaming family ------------------------------------------------
E_BOX_SCALE = 0.45      # of test_gpu_wide's hybrid batches; the CPU oracle finds 32 of 96 feasible


@pytest.fixture(scope='module')
def pwa():
    from explicit_hybrid_mpc_amd import engine
    from oracle.oracle_cpu import OracleCPU
    mpc = helpers.streaming_pwa_instance()
    can = mpc.compile()
    assert can.n_delta == 32 and can.G[0].shape[0] > 512
    gp = engine.GpuProblem(can, 0.05, 0.1)
    orc = OracleCPU(mpc, 0.05, 0.1)
    orc.memoize = True
    yield mpc, can, gp, orc
    gp.close()


def test_hybrid_batches_on_the_streaming_instance(pwa):
    """Instances arrive unsorted over the 32 commutations; k3's batch kernels walk the segments."""
    from explicit_hybrid_mpc_amd import examples
    mpc, can, gp, orc = pwa
    for kind in KINDS:
        assert gp.batch_kernel(kind) == ('k3', K3_COLUMNS, 16, K3_THREADS), kind
    rng = np.random.default_rng(21)
    half = examples.theta_box(mpc, scale=E_BOX_SCALE)
    n = 96
    theta = rng.uniform(-1, 1, (n, can.p)) * half
    pick = rng.integers(can.n_delta, size=n)
    pick[::3] = 0
    pick[1::3] = can.n_delta - 1
    delta = can.deltas[pick]
    feas, _ = gp.feasible_ptd(theta, delta)
    ref = np.array([orc.P_theta_delta(theta[k], delta[k], check_feasibility=True)
                    for k in range(n)])
    assert np.array_equal(feas, ref)
    assert feas.any() and (~feas).any()
    J, _, st, _ = gp.solve_ptd(theta[feas], delta[feas])
    assert (st == 0).all()
    for k, kk in enumerate(np.where(feas)[0]):
        J_ref = orc.P_theta_delta(theta[kk], delta[kk])[1]
        assert within(J[k], J_ref), (kk, J[k], J_ref)
    # P_theta: minimum over all 32 commutations per parameter (None = infeasible in all of them)
    Jp, _, didx = gp.solve_pt(theta[:6])
    for k in range(6):
        J_ref = orc.P_theta(theta[k])[2]
        if J_ref is None:
            assert didx[k] == -1, k
        else:
            assert didx[k] >= 0 and within(Jp[k], J_ref), (k, Jp[k], J_ref)


def test_hybrid_partition_on_the_streaming_instance(pwa):
    """The whole partition on the multi-commutation engine (K2Gather, shared midpoint solves)
    against the CPU partition: tree, commutations, closed leaves, vertex costs."""
    from oracle.oracle_cpu import OracleCPU
    from oracle.partition_cpu import PartitionCPU
    from tests.test_gpu_partition import compare_trees
    mpc, can, gp, _ = pwa
    eps_a, eps_r = helpers.eps_a_rule(mpc, 0.25), 0.1
    roots, locs = helpers.roots_of(mpc)
    assert len(roots) == 2
    orc = OracleCPU(mpc, eps_a, eps_r)
    orc.memoize = True
    cpu = PartitionCPU(orc)
    cpu.run(roots, locs, 'ecc')
    assert len(cpu.nodes) == 60
    gp.set_eps(eps_a, eps_r)
    try:
        flat = gp.partition(np.array(roots), action='ecc')
    finally:
        gp.set_eps(0.05, 0.1)
    assert flat.info['persist_kernel'][0] == 'none'
    for nd in cpu.nodes.values():
        if nd['vertex_costs'] is None:
            nd['vertex_costs'] = np.zeros(nd['vertices'].shape[0])
    compare_trees(flat, cpu.nodes, locs)
    used = set()
    for k, name in enumerate(flat.locations(locs)):
        ref = cpu.nodes[name]
        if ref['commutation'] is not None and (flat.flags[k] & 2):
            assert np.array_equal(flat.deltas[flat.delta_idx[k]].astype(int),
                                  np.asarray(ref['commutation']).astype(int)), name
            used.add(int(flat.delta_idx[k]))
    assert len(used) == 2
    assert min(cpu.min_margin, flat.info['min_margin']) > MARGIN
