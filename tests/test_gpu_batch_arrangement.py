"""
The batched oracles do not care how a batch is arranged.  Every instance of a batch is one LP,
solved by one wavefront (or one workgroup) from its own data and the constant block of its
commutation; the host sorts a batch by commutation, stages it, launches once and puts the answers
back (csrc/ehm_capi.hip, run_batch).  So every returned array -- optimum, u0, alpha, status,
iteration count -- must be BIT FOR BIT the same whether an instance travels in the batch as drawn,
in a permuted batch, in a batch of its own commutation only, among the first 13, or alone; and a
generation-2 call is one launch and one timed entry in its own slot of ``batch_launches``.

61 instances = five workgroups of 12 wavefronts plus one.  pwa_small: several commutations (one of
them left out of the batch, so the segment table has an empty run); lin: one commutation and
eliminated columns; chain_small: the wide kernels (no generation-1 kernel fits it).
"""

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

N = 61
CASES = [('pwa_small', 2), ('pwa_small', 1), ('lin', 2), ('lin', 1), ('chain_small', 2)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Batch:
    """Seeded inputs of one instance, and every plain entry point as a function of the rows
    (indices into the batch as drawn) it is asked for."""

    def __init__(self, kind):
        from explicit_hybrid_mpc_amd import engine, examples
        self.mpc = helpers.make_instance(kind, 0)
        self.can = can = self.mpc.compile()
        self.gp = gp = engine.GpuProblem(can, 0.05, 0.05)
        rng = np.random.default_rng(61)
        nd, p = can.n_delta, can.p
        half = examples.theta_box(self.mpc)
        allowed = np.ones(nd, dtype=bool)
        if nd > 2:
            allowed[rng.integers(nd)] = False          # one commutation never appears

        def pick(ok):
            """N rows with an allowed commutation among ok[row], and a random one of them each"""
            ok = ok & allowed
            rows = np.flatnonzero(ok.any(axis=1))[:N]
            assert rows.size == N
            return rows, np.array([rng.choice(np.flatnonzero(ok[r])) for r in rows], dtype=np.int32)

        # P_theta_delta: parameters with a commutation that is feasible there
        theta = rng.uniform(-0.9, 0.9, (6 * N, p)) * half
        rows, self.slot = pick(gp.feas_all(theta))
        self.theta = theta[rows]
        # phase one: any allowed commutation, parameters in- and outside the feasible set
        self.theta_any = rng.uniform(-1.3, 1.3, (N, p)) * half
        self.slot_any = rng.choice(np.flatnonzero(allowed), N).astype(np.int32)
        # simplices with a commutation that is feasible at every vertex, and its vertex optima
        R = helpers.random_simplices(self.mpc, rng, 10 * N, -2.5, -0.5)
        rows, self.rslot = pick(gp.feas_all(R.reshape(-1, p)).reshape(-1, p + 1, nd).all(axis=1))
        self.R = R[rows]
        V, _, st = gp.point_idx(self.R.reshape(-1, p), np.repeat(self.rslot, p + 1))
        assert (st == 0).all()
        self.Vbar = V.reshape(N, p + 1)
        if nd > 1:
            assert np.unique(self.slot).size > 1 and np.unique(self.rslot).size > 1
        d = can.deltas
        # name -> (timed slot, commutations of the batch, call, where the status comes back:
        # all of it 0 in the batch as drawn; None = the call returns none)
        self.calls = {
            'solve_ptd': (0, self.slot, lambda i: gp.solve_ptd(self.theta[i], d[self.slot[i]]), 2),
            'feasible_ptd': (0, self.slot_any,
                             lambda i: gp.feasible_ptd(self.theta_any[i], d[self.slot_any[i]]), None),
            'point_idx[0]': (0, self.slot,
                             lambda i: gp.point_idx(self.theta[i], self.slot[i], False), 2),
            'point_idx[1]': (0, self.slot_any,
                             lambda i: gp.point_idx(self.theta_any[i], self.slot_any[i], True), 2),
            'slack': (1, self.rslot,
                      lambda i: gp.slack(self.R[i], self.Vbar[i], d[self.rslot[i]]), 2),
            'min_simplex': (1, self.rslot,
                            lambda i: gp.min_simplex(self.R[i], d[self.rslot[i]]), 1),
            'simplex_idx[0]': (1, self.rslot,
                               lambda i: gp.simplex_idx(self.R[i], self.rslot[i], 0), 2),
            'simplex_idx[1]': (1, self.rslot,
                               lambda i: gp.simplex_idx(self.R[i], self.rslot[i], 1,
                                                        self.Vbar[i]), 2),
            'simplex_idx[2]': (1, self.slot_any,
                               lambda i: gp.simplex_idx(self.R[i], self.slot_any[i], 2), 2),
        }


@pytest.fixture(scope='module')
def batches():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Batch(kind)
        return made[kind]
    yield get
    for b in made.values():
        b.gp.close()


@pytest.mark.parametrize('kind,generation', CASES)
def test_answers_do_not_depend_on_the_arrangement(batches, kind, generation):
    b = batches(kind)
    gp = b.gp
    gp.set_solver(generation)
    rng = np.random.default_rng(13)

    def counted(name, rows):
        """the call, and what one call does to the handle's counters"""
        slot, _, fn, _ = b.calls[name]
        s0 = gp.stats()
        out = fn(np.asarray(rows))
        s1 = gp.stats()
        launches = s1['kernel_launches'] - s0['kernel_launches']
        timed = [s1['batch_launches'][k] - s0['batch_launches'][k] for k in (0, 1)]
        if generation == 2:
            assert launches == (2 if s1['fallbacks'] > s0['fallbacks'] else 1), (name, launches)
            assert timed[slot] == 1 and timed[1 - slot] == 0, (name, timed)
        else:
            assert launches == 1 and timed == [0, 0], (name, launches, timed)
        return out

    try:
        for name, (_, slots, _, status_at) in b.calls.items():
            base = counted(name, np.arange(N))
            if status_at is not None:
                assert (base[status_at] == 0).all(), (name, base[status_at])
            arrangements = [('permuted', rng.permutation(N)), ('first 13', np.arange(13)),
                            ('alone', np.arange(1))]
            arrangements += [('commutation %d' % c, np.flatnonzero(slots == c))
                             for c in np.unique(slots)]
            for what, rows in arrangements:
                got = counted(name, rows)
                assert len(got) == len(base)
                for k, (g, a) in enumerate(zip(got, base)):
                    assert same_bits(g, a[rows]), (
                        name, what, k, np.abs(g.astype(float) - a[rows]).max())
    finally:
        gp.set_solver(2)


def test_chain_small_has_no_generation_1(batches):
    """Why CASES has no ('chain_small', 1): 37 columns, the one-wavefront kernels hold 32."""
    with pytest.raises(Exception):
        batches('chain_small').gp.set_solver(1)
