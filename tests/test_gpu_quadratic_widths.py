"""
The quadratic block of the shared-block solver (csrc/ehm_ipm2.h under EHM2_QUAD, the
-DEHM2_QUAD=1 instances of csrc/ehm_k2.hip) at every compiled column capacity and row slot count,
with inputs at which the constraint rows decide the answer.

One member of examples.linear_mpc(..., cost='quadratic') per instance (tests/helpers.py,
QUADRATIC_WIDTH_ROWS).  Of the sixteen instances build.K2Q_NPS x build.K2_SLOTS the rows reach
fifteen; (32, 1) is reached by no law of the family: 25 or more columns n_u N + n_x + 1 with
n_u <= 3 need N >= 7, and then the 2 N (n_x + n_u) box rows alone, with the n_x + 3 extra rows,
pass 64.  Further rows sit on the edges of the layout: n + p + 1 equal to each capacity (t, the
last factorised column, in lane NP - 1), m + p + 3 = 256 (the second quadratic row in lane 63 of
slot 4, the row limit of the generation-1 kernels), m = 64 (the extras open a slot of their own),
and (m mod 64) + p + 3 = 64 and 65 (the extras just fit behind the rows; lp_xbase moves them to
the next slot and leaves a gap of invalid rows).

Inputs (tests/quadratic_widths_cpu.py): parameters at 0.5, 0.9, 0.98 and 0.999 of the largest
feasible multiple of fixed unit directions, and small simplices between 0.9 and 0.98 of it -- over
the calibrated box no row is active and the optimum is the unconstrained one.  Every law runs in
its natural row order and with its rows rotated by 64 k and 64 k + 1 for every occupied slot k, so
that the binding rows visit every slot, at lane 0 and at lane 63
(tests/test_host_quadratic_widths.py: some rotation has a positive multiplier in every slot, the
references do not depend on the rotation -- solve_cp to 1e-11, which is why one reference per row
serves all rotations here -- and both converge on every input).

Per row and rotation, on the default handle (generation 2) with decide_full = 1:
- batch_kernel names the row's instance for 'slack' and the instance of n columns, m rows for
  'point';
- solve_ptd, slack and min_simplex optima equal oracle/ipm_numpy.py::solve_cp to
  1e-9 (1 + |obj|) (both stop at a relative gap and residual of 1e-10; no iteration counts, the
  reference's step rule is its own), status 0 everywhere;
- the same optima equal oracle/qp_numpy.py::solve, another algorithm with its own scaling, to
  1e-7 relative;
- u0 of the point programmes to 1e-7 absolute;
- feasible_ptd says feasible at 0.999 t_max and infeasible at 1.001 t_max, as HiGHS does;
- generation 1 (every law fits its 32 columns / 256 rows) agrees to 1e-9 with identical verdicts.
No input is dropped for a row (DROPPED is empty): the device converges wherever the references do.
Measured over all rows and rotations: optima within 1.9e-10 of solve_cp and of qp_numpy, u0 within
3.6e-9, the generations within 1.9e-10 of each other.  (What a drop would be for: generation 2
steps 0.999 of the way to the boundary, the references 0.99, and a solve that stalls within 1000 x
the tolerances is accepted by all of them; with another seed of the directions one
suboptimality-test programme of the (32, 2) row stalled so on the device, and in solve_cp run with
the device's step fraction, and came back 1.6e-9 off in one rotation.)

The persistent frontier kernel of a quadratic handle (the single-width k2 kernel, always
midpoint-first) on the rows (24, 1), (24, 4), (32, 2) and the short-horizon (32, 4) row -- the CPU
partition solves the uncondensed programmes, and N = 20 takes it most of a minute -- over a box
of 0.999 x the largest feasible scale so that its corner regions are constrained, eps_r = 1e-2 and
eps_a from the first rung of the ladder of tests/test_gpu_persistent_widths.py at which the tree
has 500 nodes (TREE_SIZES: 1228, 1218, 686 and 726 nodes): one launch of the table's instance, the
tree of the generation-1 sweeps array for array (vertex costs to 1e-9), volume closed to 1e-9, a
sub-forest of 100 to 250 nodes equal to the CPU partition node for node, three dealt ranks tiling
it and two budgeted ranks merging into it.
"""

import numpy as np
import pytest

from tests import helpers
from tests import quadratic_widths_cpu as qw

pytestmark = pytest.mark.gpu

ROWS = helpers.QUADRATIC_WIDTH_ROWS
IDS = [helpers.quadratic_width_name(r) for r in ROWS]
UNREACHED = {(32, 1)}
TOL = 1e-9          # against solve_cp and between the generations, relative to 1 + |obj|
RTOL = 1e-7         # against qp_numpy (the project's bar on optimal costs)
U0_TOL = 1e-7
# point parameters (indices into qw.inputs(row).theta) left out of a row's comparisons because the
# device stalls where both references converge -- none
DROPPED = {}


def _coverage():
    from explicit_hybrid_mpc_amd import build
    assert qw.K2Q_NPS == tuple(build.K2Q_NPS)
    want = {(c, s) for c in build.K2Q_NPS for s in build.K2_SLOTS} - UNREACHED
    got = {r[:2] for r in ROWS}
    assert got == want, got ^ want
    assert len(set(IDS)) == len(IDS)
    for r in ROWS:
        n_x, n_u, N, n_random = r[2:6]
        n, m, p = n_u * N, N * (2 * n_x + n_random + 2 * n_u), n_x
        assert qw.expected_instances(n, m, p)[1] == r[:2], r
        assert n + p + 1 <= 32 and m + p + 3 <= 256, r           # fits generation 1
        if r[6] == 'full':
            assert n + p + 1 == r[0], r
    tags = {r[6]: r for r in ROWS if r[6] and r[6] != 'full'}
    dims = {t: (r[4] * (2 * r[2] + r[5] + 2 * r[3]), r[2]) for t, r in tags.items()}
    assert sum(dims['rows256']) + 3 == 256
    assert dims['m64'][0] == 64
    assert dims['fit64'][0] % 64 + dims['fit64'][1] + 3 == 64
    assert dims['gap65'][0] % 64 + dims['gap65'][1] + 3 == 65


_coverage()


def rel(a, b):
    return np.abs(a - b) / (1. + np.abs(b))


class Batch:
    """What one handle (one rotation, one generation) returns for the row's inputs."""


def run_batches(gp, can, inp, ref):
    p = can.p
    d0 = can.deltas[0]
    ns = inp.R.shape[0]
    out = Batch()
    out.kernels = (gp.batch_kernel('point'), gp.batch_kernel('slack'))
    out.J, out.u0, out.st, _ = gp.solve_ptd(inp.theta, d0)
    out.vJ, _, out.vst, _ = gp.solve_ptd(inp.R.reshape(-1, p), d0)
    dl = np.repeat(can.deltas[:1], ns, axis=0)
    t, out.alpha, out.sl_st = gp.slack(inp.R, ref.vbar, dl)
    out.sl = -t                                                     # the programme minimises -t
    out.ms, out.ms_st = gp.min_simplex(inp.R, dl)
    out.feas_in = gp.feasible_ptd(inp.inside, d0)[0]
    out.feas_out = gp.feasible_ptd(inp.outside, d0)[0]
    return out


class Case:
    def __init__(self, row):
        from explicit_hybrid_mpc_amd import engine
        self.row = row
        self.name = helpers.quadratic_width_name(row)
        self.can = qw.law(row)
        self.inp = qw.inputs(row)
        self.ref = qw.reference(row, 0)
        self.shifts = qw.rotations(self.can.m)
        self.keep = np.ones(self.inp.theta.shape[0], dtype=bool)
        self.keep[list(DROPPED.get(self.name, ()))] = False
        self.layouts = {}
        self.gen2, self.gen1 = {}, {}
        for shift in self.shifts:
            can = qw.rotate(self.can, shift)
            gp = engine.GpuProblem(can, self.ref.eps_a, qw.EPS_R)
            try:
                gp.set_option('decide_full', 1)
                self.layouts[shift] = gp.layout()
                self.gen2[shift] = run_batches(gp, can, self.inp, self.ref)
                gp.set_solver(1)
                self.gen1[shift] = run_batches(gp, can, self.inp, self.ref)
            finally:
                gp.close()


@pytest.fixture(scope='module', params=ROWS, ids=IDS)
def case(request):
    return Case(request.param)


def test_instances_are_the_tables(case):
    can = case.can
    point, slack = qw.expected_instances(can.n, can.m, can.p)
    assert slack == case.row[:2]
    for shift in case.shifts:
        assert case.layouts[shift]['nE'] == 0
        got = case.gen2[shift].kernels
        assert got[0][:3] == ('k2',) + point and got[1][:3] == ('k2',) + slack, (shift, got)
        assert [g[0] for g in case.gen1[shift].kernels] == ['k1', 'k1']


def errors(case, b):
    """Largest errors of a batch against (solve_cp, qp_numpy): point, slack, min-simplex."""
    ref, k = case.ref, case.keep
    pt = max(rel(b.J[k], ref.pt[k]).max(), rel(b.vJ, ref.vbar.reshape(-1)).max())
    pt_qp = rel(b.J[k], ref.pt_qp[k]).max()
    return ((pt, rel(b.sl, ref.sl).max(), rel(b.ms, ref.ms).max()),
            (pt_qp, rel(b.sl, ref.sl_qp).max(), rel(b.ms, ref.ms_qp).max()))


def test_optima_equal_both_references(case):
    assert case.ref.ok
    worst = np.zeros((2, 3))
    for shift in case.shifts:
        b = case.gen2[shift]
        worst = np.maximum(worst, np.array(errors(case, b)))
    print('\n%s: point / slack instances %s %s, %d rotations, active rows per point %s; max err vs '
          'solve_cp point %.1e slack %.1e min-simplex %.1e, vs qp_numpy %.1e %.1e %.1e; %d dropped'
          % (case.name, case.gen2[0].kernels[0][1:3], case.gen2[0].kernels[1][1:3],
             len(case.shifts), case.ref.n_active, *worst[0], *worst[1], int((~case.keep).sum())))
    for shift in case.shifts:
        b = case.gen2[shift]
        assert (b.st[case.keep] == 0).all() and (b.vst == 0).all(), (shift, b.st, b.vst)
        assert (b.sl_st == 0).all() and (b.ms_st == 0).all(), (shift, b.sl_st, b.ms_st)
        cp, qp = errors(case, b)
        assert max(cp) <= TOL, (shift, cp)
        assert max(qp) <= RTOL, (shift, qp)
        # the maximiser of the suboptimality test is a point of the simplex
        assert np.abs(b.alpha.sum(axis=1) - 1.).max() <= 1e-9 and b.alpha.min() >= -1e-9
    assert 20 * int((~case.keep).sum()) <= case.keep.size


def test_first_inputs(case):
    k = case.keep
    worst = max(np.abs(case.gen2[s].u0[k] - case.ref.u0[k]).max() for s in case.shifts)
    print('\n%s: u0 max err %.1e' % (case.name, worst))
    for shift in case.shifts:
        assert np.abs(case.gen2[shift].u0[k] - case.ref.u0[k]).max() <= U0_TOL, shift


def test_feasibility_verdicts(case):
    for th in case.inp.inside:
        assert qw.feasible_highs(case.can, th)
    for th in case.inp.outside:
        assert not qw.feasible_highs(case.can, th)
    for shift in case.shifts:
        for b in (case.gen2[shift], case.gen1[shift]):
            assert b.feas_in.all(), (shift, b.feas_in)
            assert not b.feas_out.any(), (shift, b.feas_out)


def test_generations_agree(case):
    k = case.keep
    for shift in case.shifts:
        a, b = case.gen1[shift], case.gen2[shift]
        assert (a.st[k] == 0).all() and (a.vst == 0).all()
        assert (a.sl_st == 0).all() and (a.ms_st == 0).all()
        assert rel(a.J[k], b.J[k]).max() <= TOL and rel(a.vJ, b.vJ).max() <= TOL, shift
        assert rel(a.sl, b.sl).max() <= TOL and rel(a.ms, b.ms).max() <= TOL, shift
        assert np.array_equal(a.feas_in, b.feas_in) and np.array_equal(a.feas_out, b.feas_out)


# ---- the persistent frontier kernel of a quadratic handle ------------------------------------------
PERSISTENT = [r for r in ROWS if r in helpers.QUADRATIC_PERSISTENT_ROWS]
PERSISTENT_IDS = [helpers.quadratic_width_name(r) for r in PERSISTENT]
assert {r[:2] for r in PERSISTENT} == {(24, 1), (24, 4), (32, 2), (32, 4)}
LADDER = 0.5 * 0.8 ** np.arange(32)      # eps_a = max optimal cost at LADDER[k] x the box vertices
EPS_R_TREE = 1e-2
# measured: the first rung of the ladder at which the whole tree has 500 nodes or more, its nodes
# and its closed leaves
TREE_SIZES = {'k2q_24_1-nx4_nu3_N4_r0': (1, 1228, 625),
              'k2q_24_4-nx4_nu1_N12_r8': (0, 1218, 620),
              'k2q_32_2-nx3_nu3_N7_r0': (0, 686, 346),
              'k2q_32_4-nx3_nu3_N7_r16_short': (3, 726, 366)}


class TreeCase:
    """One row's law over its box (0.999 x the largest feasible scale), its roots, and the eps_a of
    the first rung of the ladder at which the whole tree has 500 nodes or more."""

    def __init__(self, row):
        from explicit_hybrid_mpc_amd import examples
        self.row = row
        self.name = helpers.quadratic_width_name(row)
        self.mpc = helpers.quadratic_width_instance(row, helpers.QUADRATIC_PERSISTENT_ROWS[row])
        self.can = self.mpc.compile()
        self.V = examples.box_vertices(examples.theta_box(self.mpc))
        roots, locs = helpers.roots_of(self.mpc)
        self.roots, self.locs = np.array(roots), list(locs)
        self.total = sum(helpers.geometry.simplex_volume(R) for R in self.roots)
        self.gps = []
        self.gp = self.extra_gp(1., 1.)
        self.sizes = {}
        for rung, frac in enumerate(LADDER):
            self.eps_a = self.eps_at(frac)
            self.gp.set_eps(self.eps_a, EPS_R_TREE)
            info = self.gp.partition(self.roots, export=False, max_nodes=1 << 16)
            self.sizes[rung] = info['n_nodes']
            if info['n_nodes'] >= 500:
                break
        self.rung, self.n_nodes, self.n_closed = rung, info['n_nodes'], info['n_closed']

    def eps_at(self, frac):
        return float(np.max(self.gp.solve_pt(frac * self.V)[0]))

    def extra_gp(self, eps_a=None, eps_r=EPS_R_TREE):
        from explicit_hybrid_mpc_amd import engine
        gp = engine.GpuProblem(self.can, self.eps_a if eps_a is None else eps_a, eps_r)
        self.gps.append(gp)
        return gp

    def kernel(self):
        return ('k2', self.row[0], self.row[0], self.row[1])

    def close(self):
        for g in self.gps:
            g.close()


@pytest.fixture(scope='module', params=PERSISTENT, ids=PERSISTENT_IDS)
def tree_case(request):
    c = TreeCase(request.param)
    yield c
    c.close()


def test_persistent_tree_is_the_generation_1_sweeps_tree(tree_case):
    c, gp = tree_case, tree_case.gp
    t = gp.partition(c.roots, action='ecc')
    print('\n%s: rung %d of the ladder, %d nodes, %d closed leaves, kernel %s (sizes down the '
          'ladder %s)' % (c.name, c.rung, t.n_nodes, t.info['n_closed'], t.info['persist_kernel'],
                          c.sizes))
    assert t.info['persist_kernel'] == c.kernel() and t.info['decide_launches'] == 1
    assert (c.rung, t.n_nodes, int(t.info['n_closed'])) == TREE_SIZES[c.name]
    assert 500 <= t.n_nodes and (c.rung == 0 or c.sizes[c.rung - 1] < 500)
    assert abs(t.info['volume_closed'] - c.total) <= 1e-9 * c.total
    # the corner regions of the box are constrained: at some box vertex a row is active
    from oracle import ipm_numpy as ip
    lam = [ip.solve_cp(ip.assemble_point_quad(c.can, 0, v)).lam for v in c.V]
    assert max(int((l > qw.ACTIVE).sum()) for l in lam) >= 1
    gp.set_solver(1)
    try:
        ref = gp.partition(c.roots, action='ecc', engine=0)
    finally:
        gp.set_solver(2)
    assert ref.info['persist_kernel'][0] == 'none'
    assert t.n_nodes == ref.n_nodes
    for name in ('vertices', 'left', 'right', 'delta_idx'):
        assert np.array_equal(getattr(t, name), getattr(ref, name)), name
    assert np.array_equal(t.flags & 1, ref.flags & 1)                # the same closed leaves
    err_J = rel(t.vertex_costs, ref.vertex_costs).max()
    err_u = np.abs(t.vertex_inputs - ref.vertex_inputs).max()
    print('%s: vertex costs of the two generations differ by %.1e, inputs by %.1e'
          % (c.name, err_J, err_u))
    assert err_J <= TOL
    assert abs(t.info['volume_closed'] - ref.info['volume_closed']) <= 1e-9 * c.total


def test_sub_forest_is_the_cpu_partition(tree_case):
    """Roots taken in order, skipping those that would take the sub-forest beyond 250 nodes, until
    it has 100: node for node the partition of PartitionCPU over OracleCPU (qp_numpy on the
    uncondensed law), at both settings of decide_full."""
    from oracle.oracle_cpu import OracleCPU
    from oracle.partition_cpu import PartitionCPU
    from tests.test_gpu_partition import compare_trees
    from tests.test_gpu_persistent_widths import root_of
    c, gp = tree_case, tree_case.gp
    whole = gp.partition(c.roots)
    per_root = np.bincount(root_of(whole), minlength=len(c.roots))
    pick, n = [], 0
    for r, size in enumerate(per_root):
        if n + size > 250:
            continue
        pick.append(r)
        n += size
        if n >= 100:
            break
    assert 100 <= n <= 250, per_root
    roots = c.roots[pick]
    locs = [c.locs[r] for r in pick]
    orc = OracleCPU(c.mpc, c.eps_a, EPS_R_TREE)
    orc.memoize = True
    cpu = PartitionCPU(orc)
    cpu.run(list(roots), locs, 'ecc')
    total = sum(helpers.geometry.simplex_volume(R) for R in roots)
    try:
        for decide_full in (0, 1):
            gp.set_option('decide_full', decide_full)
            flat = gp.partition(roots, action='ecc')
            assert flat.info['persist_kernel'] == c.kernel()
            compare_trees(flat, cpu.nodes, locs, inputs_tol=1e-5)    # strictly convex: unique inputs
            assert abs(flat.info['volume_closed'] - total) <= 1e-9 * total
            assert min(cpu.min_margin, flat.info['min_margin']) > 1e-6
    finally:
        gp.set_option('decide_full', 0)


def test_dealt_shares_tile_the_tree(tree_case):
    c = tree_case
    full, parts = helpers.check_dealt_shares(c.gp, c.roots, c.locs, world=3, per_rank=32)
    assert full.info['persist_kernel'] == c.kernel()
    for part in parts:
        assert part.info['persist_kernel'] == c.kernel()


def test_budgeted_rounds_merge_into_the_tree(tree_case):
    c = tree_case
    gps = [c.extra_gp(), c.extra_gp(), c.gp]
    # (trees of 700 to 1200 nodes: from 64 pops on they are done in two rounds)
    ref, parts = helpers.check_budgeted_rounds(gps, c.roots, c.locs, first_budget=16)
    assert ref.info['persist_kernel'] == c.kernel()
    for part in parts:
        assert part.info['persist_kernel'] == c.kernel()
