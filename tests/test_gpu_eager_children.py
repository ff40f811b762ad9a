"""
Eager children of the persistent frontier kernel (option "eager_children", csrc/ehm_persist.h):
the wavefront that splits a node runs both children's LP-free tests when it creates them, writes a
child the tangent-plane bound closes as a closed leaf that never enters the queue, and keeps a
child that still needs work.  A node's fate depends on its own record only, so the tree must be
the one the kernel grows with every child decided by a visit of its own (option off) -- in every
flow the kernel has: witness cross-check, no kept child, no inherited witness, the legacy order of
the two solves, a depth limit, budgeted launches that are resumed, dealt launches.

Two rows of the persistent-width table (tests/helpers.py): a two-width kp_persist instance and a
single-width k2_persist one (a law created with EHM_SPARSE=0), at the tolerance the width tests
choose for them (a partition of 1 000 - 8 000 nodes).
"""

import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_persistent_widths import Case, expected_kernel

pytestmark = pytest.mark.gpu

ROWS = tuple(r for r in helpers.PERSISTENT_WIDTH_ROWS
             if r[:4] in (('kp', 20, 12, 3), ('k2', 16, 16, 1)))
IDS = [helpers.persistent_width_name(r) for r in ROWS]
assert len(ROWS) == 2 and ROWS[1][8]            # the k2 row is an EHM_SPARSE=0 law


class EagerCase(Case):
    """The row's problem with its reference: the tree grown with eager_children = 0."""

    def __init__(self, row):
        super().__init__(row)
        self.gp.set_option('eager_children', 0)
        try:
            self.ref = self.gp.partition(self.roots)
        finally:
            self.gp.set_option('eager_children', 1)
        assert self.ref.info['persist_kernel'] == expected_kernel(row)


@pytest.fixture(scope='module', params=ROWS, ids=IDS)
def case(request):
    c = EagerCase(request.param)
    yield c
    c.close()


def closed_at_creation(info):
    return info['persist_ticks'][9]


def assert_same_tree(t, ref, total):
    """Identity and accounting of two runs of the persistent kernel on the same roots."""
    assert t.n_nodes == ref.n_nodes and t.info['n_closed'] == ref.info['n_closed']
    assert np.array_equal(t.vertices, ref.vertices)
    assert np.array_equal(t.left, ref.left)                 # breadth-first export
    assert np.array_equal(t.flags & 1, ref.flags & 1)
    err = np.abs(t.vertex_costs - ref.vertex_costs) / (1 + np.abs(ref.vertex_costs))
    assert err.max() <= 1e-8
    assert abs(t.info['volume_closed'] - ref.info['volume_closed']) <= 1e-9 * total
    # a cert closure depends on the node's record and gradients only
    assert t.info['cert_closed'] == ref.info['cert_closed']
    assert case_errors(t) == 0 and case_errors(ref) == 0


def case_errors(t):
    """The library's error count of a run (stalled solves, conflicts of the two LP-free verdicts
    under check_witness) is not exported: a run with errors != 0 raises EHM_E_NUMERIC instead of
    returning a tree, so every tree these tests hold has errors == 0.  What is left to look at
    are the per-node marks of stalled solves, flag bits 8 and 16."""
    return int(np.count_nonzero(t.flags & (8 | 16)))


def test_same_tree_fewer_pushes(case):
    ref = case.ref
    t = case.gp.partition(case.roots)
    assert t.info['persist_kernel'] == expected_kernel(case.row)
    assert 1000 <= t.n_nodes <= 8000
    # at least one leaf closed by the bound under every root
    roots_of_nodes = np.arange(t.n_nodes)
    for k in range(t.n_nodes):
        if t.left[k] >= 0:
            roots_of_nodes[t.left[k]] = roots_of_nodes[t.right[k]] = roots_of_nodes[k]
    assert t.info['cert_closed'] >= len(case.roots)
    assert set(roots_of_nodes[(t.flags & 1) > 0]) == set(range(len(case.roots)))
    assert_same_tree(t, ref, case.total)
    n_eager = closed_at_creation(t.info)
    print('\n%s: %d nodes, %d cert-closed, %d closed at creation, pushes %d -> %d' %
          (helpers.persistent_width_name(case.row), t.n_nodes, t.info['cert_closed'], n_eager,
           ref.info['persist_pushes'], t.info['persist_pushes']))
    assert closed_at_creation(ref.info) == 0
    assert 0 < n_eager <= t.info['cert_closed']
    splits = (ref.n_nodes - len(case.roots)) // 2
    # Pushes.  Without work first every child that needs a visit is pushed, and the option takes
    # exactly the children closed at creation out of the queue:
    pushes = {}
    case.gp.set_option('work_first', 0)
    try:
        for eager in (1, 0):
            case.gp.set_option('eager_children', eager)
            info = case.gp.partition(case.roots, export=False)
            pushes[eager] = info['persist_pushes']
            assert closed_at_creation(info) == (n_eager if eager else 0)
    finally:
        case.gp.set_option('work_first', 1)
        case.gp.set_option('eager_children', 1)
    assert pushes[0] == 2 * splits
    assert pushes[1] <= pushes[0] - n_eager
    # With work first (the default) a split pushes its survivors but one: 1 with the option off,
    # max(s - 1, 0) for s survivors with it on.  Summed, pushes_on = pushes_off - n_eager + B,
    # B = the splits that lose BOTH children at creation (they push nothing, not "minus one"), and
    # B <= n_eager / 2: so "on <= off - n_eager" itself can hold only for a tree with B = 0, and
    # what does hold for every tree is asserted.
    assert ref.info['persist_pushes'] == splits
    assert t.info['persist_pushes'] <= ref.info['persist_pushes'] - (n_eager + 1) // 2
    assert t.info['persist_pushes'] >= ref.info['persist_pushes'] - n_eager


@pytest.mark.parametrize('option', ['check_witness', 'work_first', 'inherit_witness', 'mid_first'])
def test_other_options_keep_the_tree(case, option):
    """check_witness on (errors == 0: the run returns); work_first, inherit_witness, mid_first off.
    mid_first = 0 takes the two-width row to its legacy instance ('kp'), which has no eager
    children; the single-width instances are compiled midpoint first only and lose just the
    witnesses and the midpoint table with it."""
    gp = case.gp
    default = 0 if option == 'check_witness' else 1
    gp.set_option(option, 1 - default)
    try:
        t = gp.partition(case.roots)
    finally:
        gp.set_option(option, default)
    assert_same_tree(t, case.ref, case.total)
    if option == 'mid_first' and case.row[0] == 'kp':
        assert t.info['persist_kernel'][0] == 'kp'
        assert closed_at_creation(t.info) == 0
    else:
        assert closed_at_creation(t.info) > 0
    if option == 'work_first':
        # nothing is kept: every child that survives its creation is pushed
        assert t.info['persist_pushes'] == t.n_nodes - len(case.roots) - closed_at_creation(t.info)


def test_depth_limit(case):
    """max_depth two levels above the deepest level: the open leaves left there are the same
    with the option on and off (closing never depended on the depth limit)."""
    gp = case.gp
    depth = int(helpers.node_depths(case.ref).max())
    assert depth >= 4
    out = []
    for eager in (1, 0):
        gp.set_option('eager_children', eager)
        try:
            t = gp.partition(case.roots, max_depth=depth - 2)
        finally:
            gp.set_option('eager_children', 1)
        assert t.info['truncated'] == 1
        leaves = t.left < 0
        out.append((t, int(np.count_nonzero(leaves & ((t.flags & 1) == 0)))))
    (t1, open1), (t0, open0) = out
    assert open1 == open0 and open1 > 0
    assert_same_tree(t1, t0, case.total)
    assert closed_at_creation(t1.info) > 0 and closed_at_creation(t0.info) == 0


def test_budgeted_rounds_resumed_to_completion(case):
    """Budgeted launches close eagerly and queue every surviving child: what a launch leaves is the
    slice behind its pop limit, and the resumed, rebalanced shares merge into the tree of one
    launch (helpers.check_budgeted_rounds, the entry of tests/test_gpu_rebalance.py)."""
    gps = [case.extra_gp(), case.extra_gp(), case.gp]
    ref, parts = helpers.check_budgeted_rounds(gps, case.roots, case.locs)
    assert_same_tree(ref, case.ref, case.total)
    assert sum(closed_at_creation(p_.info) for p_ in parts) > 0


def test_dealt_pair_tiles_the_tree(case):
    """Two dealt launches on one GPU: the union of the shares is the unsharded tree, every closed
    leaf counted once (nothing is closed eagerly at the deal depth, where children have owners)."""
    full, parts = helpers.check_dealt_shares(case.gp, case.roots, case.locs, world=2,
                                             per_rank=32)
    assert_same_tree(full, case.ref, case.total)
    assert all(closed_at_creation(p_.info) > 0 for p_ in parts)
