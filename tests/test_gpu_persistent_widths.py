"""
The persistent frontier kernel at every compiled width.  A single-commutation partition runs in
one launch of it, and persistent_run (csrc/ehm_capi.hip) picks the kernel by the LP's shape: a
two-width pair kp / kpm (EHM_KP_ALL), a single-width k2 instance where no pair matches, or the
LDS-resident family k4 at >= 24 factorised columns and 4 row slots.  One member of
examples.linear_mpc per kernel (tests/helpers.py, PERSISTENT_WIDTH_ROWS), and for each:

- the library reports the kernel the table names (ehm_tree_persist_kernel), midpoint first or not;
- a sub-forest of about a hundred nodes is the CPU partition node for node, in all four flows;
- the whole tree is the one the generation-1 sweeps grow, bit for bit;
- three dealt ranks tile it, and two ranks with a pop budget merge into it.

k4's persistent kernel ignores PersistDeal, so the dealt, budgeted and witness-checking launches
of the k4 rows must report the single-width kernel of the same size.  chain_small, an instance
with the row-major image of the wide kernels (DevProblem::Wr3), pins the guard of that path: it
sweeps when dealt and refuses a budget.
"""

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

ROWS = helpers.PERSISTENT_WIDTH_ROWS
IDS = [helpers.persistent_width_name(r) for r in ROWS]
RTOL = 1e-7

# The rows cover every compiled pair (explicit_hybrid_mpc_amd/build.py mirrors EHM_KP_ALL), the
# single-width persistent kernels that a linear MPC without a matching pair reaches, and k4.
# (The other k2 instances are not reached by these problems: at their shapes a pair is compiled.)
K2_PERSIST_REACHED = {(8, 1), (8, 2), (8, 3), (12, 1), (12, 2), (12, 3), (12, 4), (16, 1),
                      (16, 4), (20, 4), (24, 4), (24, 2), (24, 3), (28, 2), (28, 3)}
# the one instance of ehm_k4.hip: 48 factorised columns, 8 row slots of 64 rows
K4_INSTANCE = ('k4', 48, 48, 8)
LADDER = 0.5 * 0.8 ** np.arange(32)      # eps_a = max optimal cost at LADDER[k] x the box vertices


def _coverage():
    from explicit_hybrid_mpc_amd import build
    kp = {tuple(r[1:4]) for r in ROWS if r[0] == 'kp'}
    assert kp == set(build.KP_INSTANCES), set(build.KP_INSTANCES) ^ kp
    assert set(build.KPM_INSTANCES) == set(build.KP_INSTANCES)
    k2 = {(r[1], r[3]) for r in ROWS if r[0] == 'k2'}
    assert k2 == K2_PERSIST_REACHED, k2 ^ K2_PERSIST_REACHED
    assert all(np_ in build.K2_NPS and sl in build.K2_SLOTS for np_, sl in k2)
    assert any(r[0] == 'k4' for r in ROWS)
    assert len(set(IDS)) == len(IDS)


_coverage()


def expected_kernel(row, mid_first=1, decide_full=0, restricted=False):
    """What ehm_tree_persist_kernel reports for the row.  restricted: a dealt, budgeted or
    witness-checking launch, which k4 leaves to the single-width kernel of its size."""
    fam, d, e, sl = row[:4]
    if fam == 'kp':
        return ('kpm' if mid_first and not decide_full else 'kp', d, e, sl)
    if fam == 'k4':
        return ('k2', d, e, sl) if restricted else K4_INSTANCE
    return (fam, d, e, sl)


make_gp = helpers.make_gp


def root_of(tree):
    """Index of the root each node descends from."""
    out = np.arange(tree.n_nodes)
    for k in range(tree.n_nodes):          # children always have larger indices
        if tree.left[k] >= 0:
            out[tree.left[k]] = out[k]
            out[tree.right[k]] = out[k]
    return out


class Case:
    """One row: its problem, roots and the tolerances the tests use."""

    def __init__(self, row):
        from explicit_hybrid_mpc_amd import _capi, examples
        self.row = row
        self.mpc = helpers.persistent_width_instance(row)
        self.can = self.mpc.compile()
        self.V = examples.box_vertices(examples.theta_box(self.mpc))
        roots, locs = helpers.roots_of(self.mpc)
        self.roots, self.locs = np.array(roots), list(locs)
        self.gp = make_gp(row, self.can, 1., 1.)
        self.gps = [self.gp]
        self.total = sum(helpers.geometry.simplex_volume(R) for R in self.roots)
        # eps_a from the optimal costs at scaled box vertices, down a ladder of ratio 0.8: the
        # first rung at which the whole tree has 2000 nodes or more (and at most 8000: else the one
        # above) for the device comparisons
        self.eps_big = None
        self.sizes = {}
        for frac in LADDER:
            eps_a = self.eps_at(frac)
            self.gp.set_eps(eps_a, 1e-2)
            try:
                n = self.gp.partition(self.roots, export=False, max_nodes=1 << 16)['n_nodes']
            except _capi.EhmError as e:
                assert e.code == _capi.EHM_E_CAPACITY, e
                n = 1 << 16
            self.sizes[frac] = n
            if n > 8000:
                break
            self.eps_big, self.n_big = eps_a, n
            if n >= 2000:
                break
        assert self.eps_big is not None and self.n_big >= 1000, self.sizes
        self.gp.set_eps(self.eps_big, 1e-2)

    def eps_at(self, frac):
        return float(np.max(self.gp.solve_pt(frac * self.V)[0]))

    def extra_gp(self):
        gp = make_gp(self.row, self.can, self.eps_big, 1e-2)
        self.gps.append(gp)
        return gp

    def close(self):
        for g in self.gps:
            g.close()


@pytest.fixture(scope='module', params=ROWS, ids=IDS)
def case(request):
    c = Case(request.param)
    yield c
    c.close()


def test_reported_kernel_is_the_rows(case):
    gp, row = case.gp, case.row
    for mid_first in (1, 0):
        gp.set_option('mid_first', mid_first)
        info = gp.partition(case.roots, export=False)
        assert info['persist_kernel'] == expected_kernel(row, mid_first), (mid_first, info)
        assert info['decide_launches'] == 1
    gp.set_option('mid_first', 1)
    # the witness cross-check is a PersistDeal field: k4 leaves it to the single-width kernel
    gp.set_option('check_witness', 1)
    try:
        checked = gp.partition(case.roots, export=False)
    finally:
        gp.set_option('check_witness', 0)
    assert checked['persist_kernel'] == expected_kernel(row, restricted=True)
    assert checked['n_nodes'] == info['n_nodes'] and checked['n_closed'] == info['n_closed']
    # the sweeps launch no persistent kernel
    assert gp.partition(case.roots, export=False, engine=0)['persist_kernel'][0] == 'none'
    print('\n%s: %s, %d nodes' % (helpers.persistent_width_name(row),
                                   expected_kernel(row), case.n_big))


def test_sub_forest_identical_to_cpu_partition(case):
    """Node for node against the CPU partition (the bars of test_gpu_wide.py), in the four
    flows: suboptimality test to full accuracy or sign only, midpoint solve first or not."""
    from oracle.oracle_cpu import OracleCPU
    from oracle.partition_cpu import PartitionCPU
    from oracle import geometry
    gp, row = case.gp, case.row
    eps_r = 1e-2
    try:
        # the first rung of the ladder at which some roots, taken in order and skipping those that
        # would take it beyond 300 nodes, make a sub-forest of 100 nodes or more
        for frac in LADDER:
            eps_a = case.eps_at(frac)
            gp.set_eps(eps_a, eps_r)
            whole = gp.partition(case.roots)
            per_root = np.bincount(root_of(whole), minlength=len(case.roots))
            pick, n = [], 0
            for r, size in enumerate(per_root):
                if n + size > 300:
                    continue
                pick.append(r)
                n += size
                if n >= 100:
                    break
            if n >= 100 or whole.n_nodes > 8000:
                break
        assert 100 <= n <= 300, per_root
        roots = case.roots[pick]
        locs = [case.locs[r] for r in pick]
        cpu = PartitionCPU(OracleCPU(case.mpc, eps_a, eps_r))
        cpu.run(list(roots), locs, 'ecc')
        total = sum(geometry.simplex_volume(R) for R in roots)
        for decide_full in (0, 1):
            for mid_first in (0, 1):
                gp.set_option('decide_full', decide_full)
                gp.set_option('mid_first', mid_first)
                flat = gp.partition(roots, action='ecc')
                assert flat.info['persist_kernel'] == expected_kernel(row, mid_first, decide_full)
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
                assert flat.info['min_margin'] > 1e-6
    finally:
        gp.set_option('decide_full', 0)
        gp.set_option('mid_first', 1)
        gp.set_eps(case.eps_big, 1e-2)


def test_whole_tree_identical_to_generation_1_sweeps(case):
    gp, row = case.gp, case.row
    gp.set_solver(1)
    try:
        ref = gp.partition(case.roots, engine=0)
    finally:
        gp.set_solver(2)
    assert ref.n_nodes == case.n_big
    assert abs(ref.info['volume_closed'] - case.total) <= 1e-9 * case.total
    for mid_first in (1, 0):
        gp.set_option('mid_first', mid_first)
        t = gp.partition(case.roots)
        assert t.info['persist_kernel'] == expected_kernel(row, mid_first)
        assert t.n_nodes == ref.n_nodes
        assert np.array_equal(t.vertices, ref.vertices)          # bit-identical geometry
        assert np.array_equal(t.left, ref.left)
        assert np.array_equal(t.flags & 1, ref.flags & 1)        # same closed leaves
        err = np.abs(t.vertex_costs - ref.vertex_costs) / (1 + np.abs(ref.vertex_costs))
        assert err.max() <= 1e-8
        assert abs(t.info['volume_closed'] - ref.info['volume_closed']) <= 1e-9 * case.total
    gp.set_option('mid_first', 1)


def test_dealt_shares_tile_the_tree(case):
    full, parts = helpers.check_dealt_shares(case.gp, case.roots, case.locs, world=3,
                                             per_rank=32)
    assert full.info['persist_kernel'] == expected_kernel(case.row)
    for part in parts:
        assert part.info['persist_kernel'] == expected_kernel(case.row, restricted=True)


def test_budgeted_rounds_merge_into_the_tree(case):
    gps = [case.extra_gp(), case.extra_gp(), case.gp]
    ref, parts = helpers.check_budgeted_rounds(gps, case.roots, case.locs)
    assert ref.info['persist_kernel'] == expected_kernel(case.row)
    for part in parts:
        assert part.info['persist_kernel'] == expected_kernel(case.row, restricted=True)


def test_wide_image_row_sweeps_when_dealt_and_refuses_a_budget():
    """chain_small: a problem with the row-major image of the wide kernels (DevProblem::Wr3)
    runs its persistent kernel on single-rank runs to completion only."""
    from explicit_hybrid_mpc_amd import engine, _capi
    mpc = helpers.make_instance('chain_small', 0)
    eps_a = helpers.eps_a_rule(mpc, 0.5)
    roots, locs = helpers.roots_of(mpc)
    roots = np.array(roots)
    can = mpc.compile()
    assert can.n + can.p + 1 > 32
    gps = [engine.GpuProblem(can, eps_a, 0.2) for _ in range(2)]
    try:
        full, parts = helpers.check_dealt_shares(gps[0], roots, list(locs), world=3,
                                                 per_rank=32, one_launch=False)
        assert full.info['decide_launches'] == 1
        assert full.info['persist_kernel'][0] != 'none'
        assert all(p_.info['persist_kernel'][0] == 'none' for p_ in parts)
        assert all(p_.info['decide_launches'] > 1 for p_ in parts)
        # a budgeted launch would grow the whole tree: advance refuses the problem
        runs = [gps[r].begin(roots, shard=(r, 2, -1)) for r in range(2)]
        with pytest.raises(_capi.EhmError):
            runs[0].advance(64)
        for run in runs:
            run.abort()
        # the witness cross-check is a PersistDeal field too: never k4
        gps[1].set_option('check_witness', 1)
        checked = gps[1].partition(roots)
        assert checked.info['persist_kernel'][0] != 'k4'
        if full.info['persist_kernel'][0] != 'k4':
            assert checked.info['persist_kernel'] == full.info['persist_kernel']
        print('\nchain_small: %s, %d nodes' % (full.info['persist_kernel'], full.n_nodes))
        assert checked.n_nodes == full.n_nodes
        assert np.array_equal(checked.vertices, full.vertices)
        assert np.array_equal(checked.flags & 1, full.flags & 1)
    finally:
        for g in gps:
            g.close()
