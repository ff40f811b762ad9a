"""
Idle time of the persistent frontier kernel (csrc/ehm_persist.h): option "requeue_undecided" -- a
node that finds its midpoint being solved by another wavefront goes back into the queue (once)
whether or not its fate is known, instead of only the nodes the inherited witness has opened.  It
changes who visits a node and when, never what a visit computes: the exported tree must be the one
the kernel grows with the option off, and the one the level-synchronous sweeps grow, array for
array.  (tstar, the slack of a node's last decision, is compared by its sign: its value is that of
whichever test decided the node -- bound, witness or LP -- which differs between the engines by
construction and, in the persistent kernel, with the order of the visits; bench.py dumps it the
same way.)

The law is the headline's (examples.linear_mpc(seed=0, cost='inf'), 22 Delaunay roots) at
tolerances so coarse that the tree has one to a few thousand nodes (the budgeted rounds of
tests/helpers.py need a thousand to have something to rebalance): fewer nodes than wavefronts, so
the kernel is starved from its first pop to its last, which is where midpoints are found busy.  A
p = 2 law of the persistent-width table (tests/helpers.py) repeats the comparison at another
dimension.

That the option takes effect is read off two counters of ehm_tree_info.persist_ticks, [5] the
waits for a busy midpoint and [8] the nodes put back:
  off: only nodes the inherited witness opened are put back, so [8] <= witness_inherited;
  on:  a node waits only if it has come back once already, so [5] <= [8].
"""

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

OPTION = 'requeue_undecided'        # on by default (csrc/ehm_capi.hip)
LADDER = 0.5 * 0.8 ** np.arange(32)
ARRAYS = ('vertices', 'left', 'right', 'delta_idx', 'vertex_costs', 'vertex_inputs', 'flags')


def assert_equal_export(t, ref):
    assert t.n_nodes == ref.n_nodes and t.info['n_closed'] == ref.info['n_closed']
    for name in ARRAYS:
        assert np.array_equal(getattr(t, name), getattr(ref, name)), name
    assert np.array_equal(t.tstar >= 0, ref.tstar >= 0)


def assert_option_took_effect(info, on):
    waits, put_back = info['persist_ticks'][5], info['persist_ticks'][8]
    if on:
        assert waits <= put_back, (waits, put_back)
    else:
        assert put_back <= info['witness_inherited'], (put_back, info['witness_inherited'])


def assert_same_tree_as_sweeps(t, sweeps):
    """Against the level-synchronous engine (engine=0), after the breadth-first relabelling."""
    assert_equal_export(t, sweeps)


class Law:
    """A law, its roots, a starved tolerance and the two reference trees at it."""

    def __init__(self, mpc):
        from explicit_hybrid_mpc_amd import engine, examples
        self.mpc = mpc
        self.can = mpc.compile()
        self.V = examples.box_vertices(examples.theta_box(mpc))
        roots, locs = helpers.roots_of(mpc)
        self.roots, self.locs = np.array(roots), list(locs)
        self.gp = engine.GpuProblem(self.can, 1., 1.)       # the option at its default: on
        self.gps = [self.gp]
        # the first rung of the ladder with 1000 nodes or more (eps_r = 0.05: eps_a decides)
        self.eps_r = 5e-2
        for frac in LADDER:
            self.eps_a = float(np.max(self.gp.solve_pt(frac * self.V)[0]))
            self.gp.set_eps(self.eps_a, self.eps_r)
            n = self.gp.partition(self.roots, export=False, max_nodes=1 << 16)['n_nodes']
            if n >= 1000:
                break
        assert 1000 <= n <= 8000, n
        self.gp.set_option(OPTION, 0)
        try:
            self.off = self.gp.partition(self.roots)
        finally:
            self.gp.set_option(OPTION, 1)
        self.sweeps = self.gp.partition(self.roots, engine=0)
        assert self.off.info['persist_kernel'][0] in ('kpm', 'k2')
        assert self.sweeps.info['persist_kernel'][0] == 'none'

    def extra_gp(self):
        from explicit_hybrid_mpc_amd import engine
        gp = engine.GpuProblem(self.can, self.eps_a, self.eps_r)
        self.gps.append(gp)
        return gp

    def close(self):
        for g in self.gps:
            g.close()


@pytest.fixture(scope='module')
def headline():
    from explicit_hybrid_mpc_amd import examples
    law = Law(examples.linear_mpc(seed=0, cost='inf'))
    assert len(law.roots) == 22
    yield law
    law.close()


@pytest.fixture(scope='module')
def planar():
    row = next(r for r in helpers.PERSISTENT_WIDTH_ROWS if r[:4] == ('kp', 12, 8, 2))
    law = Law(helpers.persistent_width_instance(row))
    assert law.can.p == 2
    yield law
    law.close()


def test_option_against_the_reference_runs(headline):
    t = headline.gp.partition(headline.roots)
    off = headline.off
    print('\n%d nodes; midpoint waits %d (off: %d), nodes put back %d (off: %d), opened by the '
          'inherited witness %d' % (t.n_nodes, t.info['persist_ticks'][5], off.info['persist_ticks'][5],
                                    t.info['persist_ticks'][8], off.info['persist_ticks'][8],
                                    t.info['witness_inherited']))
    assert t.info['persist_kernel'] == off.info['persist_kernel']
    assert_equal_export(t, off)
    assert_same_tree_as_sweeps(t, headline.sweeps)
    assert_same_tree_as_sweeps(off, headline.sweeps)
    # starved from start to end: midpoints are found busy, and the option decides what then happens
    assert off.info['persist_ticks'][5] > 0 and t.info['persist_ticks'][8] > 0
    assert_option_took_effect(t.info, on=True)
    assert_option_took_effect(off.info, on=False)


def test_every_root_closes_at_once(headline):
    """22 nodes for 3072 wavefronts: all but 22 of them draw a queue position nothing is ever
    pushed to and leave when `pending` reaches zero."""
    gp = headline.gp
    big = float(np.max(gp.solve_pt(headline.V)[0]))
    gp.set_eps(1e3 * big, 1.0)
    try:
        for value in (1, 0):
            gp.set_option(OPTION, value)
            t = gp.partition(headline.roots)
            assert t.n_nodes == 22 and t.info['n_closed'] == 22
            assert np.all(t.left < 0) and np.all(t.flags & 1)
    finally:
        gp.set_option(OPTION, 1)
        gp.set_eps(headline.eps_a, headline.eps_r)


def test_budgeted_rounds_merge_into_the_tree(headline):
    """ehm_partition_advance with the option on: a budgeted launch puts nothing back, so what it
    leaves is still the slice behind the pop limit (helpers.check_budgeted_rounds)."""
    gps = [headline.extra_gp(), headline.extra_gp(), headline.gp]
    ref, parts = helpers.check_budgeted_rounds(gps, headline.roots, headline.locs)
    assert_equal_export(ref, headline.off)
    # budgeted launches put nothing back: their left-over must stay contiguous
    assert all(p_.info['persist_ticks'][8] == 0 for p_ in parts)


def test_dealt_pair_tiles_the_tree(headline):
    full, parts = helpers.check_dealt_shares(headline.gp, headline.roots, headline.locs, world=2,
                                             per_rank=32)
    assert_equal_export(full, headline.off)


def test_node_pool_exhausted_returns(headline):
    """The abort path with put-back nodes in the queue: the capacity error, and the launch returns."""
    from explicit_hybrid_mpc_amd import _capi
    gp = headline.gp
    cap = headline.off.n_nodes // 2
    with pytest.raises(_capi.EhmError) as e:
        gp.partition(headline.roots, max_nodes=cap)
    assert e.value.code == _capi.EHM_E_CAPACITY
    # the handle is usable again, and the next run is the tree
    assert_equal_export(gp.partition(headline.roots), headline.off)


def test_planar_law(planar):
    t = planar.gp.partition(planar.roots)
    assert_equal_export(t, planar.off)
    assert_same_tree_as_sweeps(t, planar.sweeps)
    assert_option_took_effect(t.info, on=True)
    assert_option_took_effect(planar.off.info, on=False)
