"""
The triangular solves of the shared-block LP solver (csrc/ehm_ipm2.h: lu_solve) on instances of at
most 16 columns broadcast y_k / x_k with a DPP row broadcast (row_newbcast) instead of lane reads.
The broadcast stays inside a row of 16 lanes, so what these tests are chosen for is WHERE the
lanes that matter sit: the last source lane of the capacity (NP - 1, lane 15 for NP = 16), and the
lanes of the eliminated columns, nr .. nr + nE - 1, which take their solution from LDS and may lie
beyond lane 15, where the broadcasts deliver other values.  Members of
examples.linear_mpc(seed=0, n_x, n_u, N), sized on the CPU (asserted below through
ehm_problem_layout / ehm_problem_batch_kernel):

    (n_x, n_u, N)   nE   factorised columns, point / slack LP   capacities   covers
    (3, 2, 6)       12   12 / 16                                12 / 16      both exactly full: the source lane is
                                                                             NP - 1, and lane 15
    (3, 2, 4)        8    8 / 12                                 8 / 12      capacity 8 and capacity 12 full
    (2, 1, 5)       10    5 /  8                                 8 /  8      p = 2, a short chain below a full
                                                                             capacity-8 instance
    (4, 2, 5)       10   10 / 15                                12 / 16      the headline sizes; eliminated lanes
                                                                             15 .. 24 cross the DPP row boundary
    (4, 2, 7)       14   14 / 19                                16 / 20      the slack LP on a capacity-20 instance,
                                                                             which keeps the lane reads
    (2, 1, 9)       18    9 / 12                                12 / 12      18 eliminated columns: lanes 9 .. 29

and (3, 2, 4) again without the eliminated block (EHM_SPARSE=0: 16 / 20 factorised columns, no
eliminated lane at all), and with the quadratic cost (the -DEHM2_QUAD instances, capacities 8 / 16).

Every point LP and every suboptimality-test LP of six random simplices per law is solved at full
accuracy and compared with the dense numpy restatement of the same method, oracle/ipm_numpy.py:
optimum to 1e-9 (1 + |obj|) -- both stop at a relative gap and residual of 1e-10, so two converged
optima differ by about 2e-10 relative -- and, for the linear programmes, THE SAME ITERATION COUNT
(the references and the loop of tests/test_gpu_solver_loops.py at this file's cases).  For two of
the laws the whole partition grown by the persistent frontier kernel is the tree of the
level-synchronous sweeps, array for array.
"""
import numpy as np
import pytest

from explicit_hybrid_mpc_amd import examples
from explicit_hybrid_mpc_amd import tools as ehm_tools
from oracle import ipm_numpy as ip
from tests import test_gpu_solver_loops as loops

pytestmark = pytest.mark.gpu

#        (n_x, n_u, N): nE, (point nr, capacity), (slack nr, capacity)
CASES = {(3, 2, 6): (12, (12, 12), (16, 16)),
         (3, 2, 4): (8, (8, 8), (12, 12)),
         (2, 1, 5): (10, (5, 8), (8, 8)),
         (4, 2, 5): (10, (10, 12), (15, 16)),
         (4, 2, 7): (14, (14, 16), (19, 20)),
         (2, 1, 9): (18, (9, 12), (12, 12))}
DENSE = (3, 2, 4)           # also with EHM_SPARSE=0: point 8 + 8 = 16, slack 12 + 8 = 20 columns
DENSE_CAPS = (16, 20)
QUAD = (3, 2, 4)            # also with the quadratic cost: no epigraph columns, 8 / 12 columns
QUAD_CAPS = (8, 16)         # the quadratic instances come at capacities 8, 16, 24, 32
PARTITION_LAWS = [(3, 2, 6), (3, 2, 4)]
TOL = loops.TOL
N_SIMPLICES = loops.N_SIMPLICES


def sizes(can, nE):
    """Factorised columns of the point and of the suboptimality-test LP: the z-columns that stay,
    and with them the p weights and t."""
    return can.n - nE, can.n - nE + can.p + 1


def assert_capacities(gp, caps):
    got = (gp.batch_kernel('point'), gp.batch_kernel('slack'))
    assert [g[0] for g in got] == ['k2', 'k2'], got
    assert (got[0][1], got[1][1]) == tuple(caps), got


def check_case(case, sparse, caps):
    """The loop of tests/test_gpu_solver_loops.py::check_case on a handle whose instances are
    asserted first."""
    mpc, can, Rs, pt_obj, pt_it, sl_obj, sl_it = loops.reference(case)
    nE = CASES[case][0]
    p = can.p
    gp = loops.make_gp(can, sparse)
    try:
        assert gp.layout()['nE'] == (nE if sparse else 0), gp.layout()
        assert_capacities(gp, caps)
        theta = Rs.reshape(-1, p)
        # the point LP at every vertex: optimum from P_theta, iterations per solve from
        # P_theta_delta (the same LP: the law has one commutation)
        J, _, didx = gp.solve_pt(theta)
        J2, _, status, iters = gp.solve_ptd(theta, can.deltas[0])
        ref = pt_obj.reshape(-1)
        err_pt = np.abs(J - ref) / (1. + np.abs(ref))
        # the suboptimality-test LP on every simplex, one call each: the handle's counters give
        # the call's iterations
        err_sl = np.empty(N_SIMPLICES)
        it_sl = np.empty(N_SIMPLICES, dtype=int)
        n_sl = np.empty(N_SIMPLICES, dtype=int)
        st_sl = np.empty(N_SIMPLICES, dtype=int)
        for k in range(N_SIMPLICES):
            s0 = gp.stats()
            t, _, st = gp.slack(Rs[k], pt_obj[k], can.deltas[0])
            s1 = gp.stats()
            err_sl[k] = abs(-t[0] - sl_obj[k]) / (1. + abs(sl_obj[k]))       # t* = -(min -t)
            it_sl[k] = s1['ipm_iters'] - s0['ipm_iters']
            n_sl[k] = s1['lp_solves'] - s0['lp_solves']
            st_sl[k] = st[0]
        print('\n%s nE %d, capacities %s: point LPs max err %.2e, iterations %s (ref %s); slack LPs '
              'max err %.2e, iterations %s (ref %s)'
              % (case, gp.layout()['nE'], caps, err_pt.max(), iters.tolist(),
                 pt_it.reshape(-1).tolist(), err_sl.max(), it_sl.tolist(), sl_it.tolist()))
        assert (didx == 0).all() and (status == 0).all() and (st_sl == 0).all()
        assert np.array_equal(J, J2)
        assert err_pt.max() <= TOL
        assert np.array_equal(iters, pt_it.reshape(-1))
        assert (n_sl == 1).all()
        assert err_sl.max() <= TOL
        assert np.array_equal(it_sl, sl_it)
    finally:
        gp.close()


@pytest.mark.parametrize('case', list(CASES), ids=['%d_%d_%d' % c for c in CASES])
def test_point_and_slack_lps_equal_the_dense_method(case):
    nE, (nr_pt, cap_pt), (nr_sl, cap_sl) = CASES[case]
    assert sizes(loops.reference(case)[1], nE) == (nr_pt, nr_sl)
    check_case(case, True, (cap_pt, cap_sl))


def test_without_the_eliminated_block():
    check_case(DENSE, False, DENSE_CAPS)


def test_quadratic_cost():
    """Point and suboptimality-test programmes of the quadratic-cost law against
    oracle/ipm_numpy.py::solve_cp, the numpy restatement of the solver's quadratic block (same
    stopping rule, so the same bar on the optimum; its step rule is its own, so no iteration
    counts)."""
    from explicit_hybrid_mpc_amd import engine
    n_x, n_u, N = QUAD
    can = examples.linear_mpc(seed=0, n_x=n_x, n_u=n_u, N=N, cost='quadratic').compile()
    p = can.p
    Rs = loops.reference(QUAD)[2]       # the simplices of the linear case: the same constraints
    pt_ref = np.empty((N_SIMPLICES, p + 1))
    sl_ref = np.empty(N_SIMPLICES)
    for k, R in enumerate(Rs):
        for v in range(p + 1):
            o = ip.solve_cp(ip.assemble_point_quad(can, 0, R[v]))
            assert o.status == 0, (k, v)
            pt_ref[k, v] = o.obj
        o = ip.solve_cp(ip.assemble_bar_E_quad(can, 0, R, pt_ref[k], loops.EPS_A, loops.EPS_R))
        assert o.status == 0, k
        sl_ref[k] = o.obj
    gp = engine.GpuProblem(can, loops.EPS_A, loops.EPS_R)
    try:
        gp.set_option('decide_full', 1)
        assert gp.layout()['nE'] == 0
        assert_capacities(gp, QUAD_CAPS)
        J, _, status, _ = gp.solve_ptd(Rs.reshape(-1, p), can.deltas[0])
        ref = pt_ref.reshape(-1)
        err_pt = np.abs(J - ref) / (1. + np.abs(ref))
        t, _, st = gp.slack(Rs, pt_ref, np.repeat(can.deltas[:1], N_SIMPLICES, axis=0))
        err_sl = np.abs(-t - sl_ref) / (1. + np.abs(sl_ref))
    finally:
        gp.close()
    print('\nquadratic %s: point programmes max err %.2e, suboptimality tests max err %.2e'
          % (QUAD, err_pt.max(), err_sl.max()))
    assert (status == 0).all() and (st == 0).all()
    assert err_pt.max() <= TOL
    assert err_sl.max() <= TOL


# The partitions below: root simplices of the box |theta_i| <= 0.09, eps_r = 0.1, eps_a = the
# largest optimal cost at ABS_FRAC x the box vertices (the recipe of tests/test_gpu_solver_loops.py).
# Measured: 866 nodes at 0.1, 1674 at 0.07, 4002 at 0.05, 8130 at 0.035 -- for both laws: at these
# parameters the longer horizon changes the LPs (24 against 16 columns, 168 against 112 rows) and
# the kernels (widths 16 / 12 against 12 / 8), not the tree.
ABS_FRAC = 0.05
PARTITION_NODES, PARTITION_CLOSED = 4002, 2004
ARRAYS = ('vertices', 'left', 'right', 'delta_idx', 'vertex_costs', 'vertex_inputs', 'flags')


@pytest.mark.parametrize('case', PARTITION_LAWS, ids=['%d_%d_%d' % c for c in PARTITION_LAWS])
def test_persistent_partition_is_the_sweeps_tree(case):
    from explicit_hybrid_mpc_amd import engine
    can = loops.reference(case)[1]
    V = examples.box_vertices(loops.HALF * np.ones(can.p))
    roots, _ = ehm_tools.delaunay_roots(V)
    gp = engine.GpuProblem(can, 1., 1.)
    try:
        eps_a = float(np.max(gp.solve_pt(ABS_FRAC * V)[0]))
        gp.set_eps(eps_a, 0.1)
        a = gp.partition(roots, action='ecc')
        b = gp.partition(roots, action='ecc', engine=0)
    finally:
        gp.close()
    print('\npartition %s: %d nodes, %d closed, kernel %s' %
          (case, a.n_nodes, a.info['n_closed'], a.info['persist_kernel']))
    assert a.info['persist_kernel'][0] in ('kp', 'kpm', 'k2') and a.info['decide_launches'] == 1
    assert a.info['persist_kernel'][1] <= 16        # both widths on the row broadcast
    assert b.info['persist_kernel'][0] == 'none'
    assert a.n_nodes == PARTITION_NODES and a.info['n_closed'] == PARTITION_CLOSED
    assert a.n_nodes == b.n_nodes and a.info['n_closed'] == b.info['n_closed']
    for name in ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.tstar >= 0, b.tstar >= 0)
