"""
Closed-loop simulation, the host side (explicit_hybrid_mpc_amd/simulate.py): the plant each law
is closed around, the commutation -> step-0 mode map, a CPU restatement of one rollout step, and
no CPU fallback for the device rollout.
"""

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, examples
from explicit_hybrid_mpc_amd.simulate import Plant
from tests import helpers
from tests import rollout_cpu


def test_plant_of_the_double_integrator():
    mpc = examples.double_integrator(3)
    pl = Plant.from_mpc(mpc)
    assert (pl.n_modes, pl.n_x, pl.n_u, pl.n_d) == (1, 2, 1, 0)
    assert np.array_equal(pl.A[0], [[1., 1.], [0., 1.]])
    assert np.array_equal(pl.B[0], [[0.5], [1.]])
    assert np.array_equal(pl.w[0], [0., 0.])
    assert pl.regions == [None]
    assert np.array_equal(pl.Gx, mpc.Gx) and np.array_equal(pl.gx, mpc.gx)
    assert np.array_equal(pl.Q, np.eye(2)) and np.array_equal(pl.R, np.eye(1))
    assert pl.cost == 'inf'
    rows, H, h = pl.region_arrays()
    assert rows.tolist() == [0] and H.shape == (0, 2) and h.shape == (0,)


def test_plant_of_the_pwa_law():
    mpc = examples.pwa_mpc(0)
    pl = Plant.from_mpc(mpc)
    assert pl.n_modes == 2 and pl.n_d == 0
    for i in range(2):
        assert np.array_equal(pl.A[i], mpc.A[i]) and np.array_equal(pl.B[i], mpc.B[i])
        assert np.array_equal(pl.w[i], mpc.w[i])
        assert np.array_equal(pl.regions[i][0], mpc.regions[i][0])
        assert np.array_equal(pl.regions[i][1], mpc.regions[i][1])
    rows, H, h = pl.region_arrays()
    assert rows.tolist() == [1, 1]
    assert np.array_equal(H, np.vstack([mpc.regions[0][0], mpc.regions[1][0]]))
    assert np.array_equal(pl.Q, mpc.Q) and np.array_equal(pl.R, mpc.R) and pl.cost == 'inf'
    # the region test: mode 0 holds x_1 >= -overlap, mode 1 x_1 <= overlap
    X = np.array([[-0.2, 0, 0, 0], [0.2, 0, 0, 0]])
    assert pl.in_region(X, np.array([0, 0]), 0.).tolist() == [False, True]
    assert pl.in_region(X, np.array([1, 1]), 0.).tolist() == [True, False]


def test_plant_of_the_satellite_law():
    import scipy.linalg as sla
    mpc = examples.satellite_z(4)
    pl = Plant.from_mpc(mpc)
    pars = mpc.pars
    A_c = np.array([[0., 1.], [-pars['wo'] ** 2, 0.]])
    A = sla.expm(A_c * pars['T_s'])
    assert pl.n_modes == 3 and pl.n_d == 1 and pl.T_s == pars['T_s']
    for m in range(3):                     # off, piece 0, piece 1: one set of dynamics
        assert np.allclose(pl.A[m], A, rtol=1e-14, atol=0)
        assert np.allclose(pl.B[m], A @ [[0.], [1.]], rtol=1e-14, atol=0)
        assert not pl.w[m].any() and pl.regions[m] is None
    M = np.zeros((3, 3))
    M[:2, :2], M[:2, 2:] = A_c, [[0.], [1.]]
    assert np.allclose(pl.E, sla.expm(M * pars['T_s'])[:2, 2:], rtol=1e-14, atol=0)
    assert pl.cost == 'quadratic'
    assert np.allclose(pl.R, [[1. / 2e-3 ** 2]], rtol=1e-14)
    assert np.allclose(pl.Q, 1e-2 * np.diag([1. / 0.1 ** 2, 1. / 1e-3 ** 2]), rtol=1e-14)
    assert np.array_equal(pl.Gx, mpc.Gx) and np.array_equal(pl.gx, mpc.gx)


@pytest.mark.parametrize('kind', ['pwa_small', 'cwh_z'])
def test_step0_mode_inverts_sequence_to_delta(kind):
    mpc = examples.satellite_z(4) if kind == 'cwh_z' else helpers.make_instance('pwa_small')
    seqs = mpc.mode_sequences()
    assert len(seqs) == (81 if kind == 'cwh_z' else 8)
    for s in seqs:
        assert mpc.step0_mode(mpc.sequence_to_delta(s)) == s[0]
    # and through the compiled commutation table the device reports indices into
    can = mpc.compile()
    assert [mpc.step0_mode(d) for d in can.deltas] == [s[0] for s in seqs]


class _Flat:
    def __init__(self, vertices, vertex_inputs):
        self.vertices = np.asarray(vertices, dtype=np.float64)
        self.vertex_inputs = np.asarray(vertex_inputs, dtype=np.float64)
        K = self.vertices.shape[0]
        self.left = -np.ones(K, dtype=np.int32)
        self.right = -np.ones(K, dtype=np.int32)
        self.info = {'n_roots': K}


def test_cpu_rollout_step_by_hand():
    """One step of the double integrator under a law interpolated on two triangles."""
    pl = Plant.from_mpc(examples.double_integrator(3))
    # roots: the lower-left and the upper-right triangle of [0, 2]^2; u at the vertices
    flat = _Flat([[[0, 0], [2, 0], [0, 2]], [[2, 2], [0, 2], [2, 0]]],
                 [[[0.], [-1.], [1.]], [[0.5], [1.], [-1.]]])
    cpu = rollout_cpu.flat_cpu(flat)
    modes = np.zeros(2, dtype=np.int32)
    x = np.array([0.5, 0.25])
    st, k, u, xn = rollout_cpu.step(cpu, pl, modes, x, x, 1e-9)
    # barycentric in root 0: x = 0.25 (2,0) + 0.125 (0,2) + 0.625 (0,0)
    assert (st, k) == (0, 0)
    assert u[0] == pytest.approx(0.625 * 0. + 0.25 * -1. + 0.125 * 1.)      # -0.125
    assert xn == pytest.approx([0.5 + 0.25 + 0.5 * -0.125, 0.25 - 0.125])
    # in the second root (the walk tests root 0 first, then takes the last one)
    x = np.array([1.5, 1.5])
    st, k, u, xn = rollout_cpu.step(cpu, pl, modes, x, x, 1e-9)
    # x = 0.5 (2,2) + 0.25 (0,2) + 0.25 (2,0)
    assert (st, k) == (0, 1) and u[0] == pytest.approx(0.5 * 0.5 + 0.25 - 0.25)
    assert xn == pytest.approx([1.5 + 1.5 + 0.125, 1.5 + 0.25])
    # a measurement error moves the located state; the plant steps from the true one
    st, k, u, xn = rollout_cpu.step(cpu, pl, modes, x, np.array([0.5, 0.25]), 1e-9)
    assert (st, k) == (0, 0) and u[0] == pytest.approx(-0.125)
    assert xn == pytest.approx([1.5 + 1.5 - 0.0625, 1.5 - 0.125])
    # outside the set: the walk ends in the last root, whose weights are negative -> stop
    st, k, u, xn = rollout_cpu.step(cpu, pl, modes, x, np.array([3., 3.]), 1e-9)
    assert st == 1 and u is None
    # stage costs of the two cost kinds
    X, U = np.array([[1., -3.]]), np.array([[2.]])
    assert pl.stage_cost(X, U)[0] == 3. + 2.
    pq = Plant(pl.A, pl.B, pl.w, None, pl.regions, pl.Gx, pl.gx, pl.Q, pl.R, 'quadratic')
    assert pq.stage_cost(X, U)[0] == 10. + 4.


def test_rollout_has_no_cpu_fallback():
    """The rollout runs on the device or not at all."""
    lib = _capi.load()
    out = [np.zeros(4), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32),
           np.zeros(2), np.zeros(2), np.zeros(2)]
    rc = lib.ehm_explicit_rollout(None, 2, 3, np.zeros(4).ctypes.data, None, None, 1e-9, None,
                                  None, None, *[a.ctypes.data for a in out], None)
    assert rc == _capi.EHM_E_INVALID
    rc = lib.ehm_explicit_set_plant(None, 1, None, None, None, 0, None, None, None, None, 0, None,
                                    None, None, 0, None, None)
    assert rc == _capi.EHM_E_INVALID
    # through the public class: where the library finds no device, the law cannot even be set up
    from explicit_hybrid_mpc_amd import explicit
    from explicit_hybrid_mpc_amd.engine import FlatTree
    f = _Flat([[[0, 0], [2, 0], [0, 2]]], [[[0.], [1.], [1.]]])
    flat = FlatTree(f.vertices, f.left, f.right, np.zeros(1, dtype=np.int32), np.zeros((1, 3)),
                    f.vertex_inputs, np.zeros(1, dtype=np.uint8), np.zeros(1), f.info,
                    np.ones((1, 3)))
    try:
        law = explicit.ExplicitMPC(flat)
    except _capi.EhmError as err:
        assert err.code == _capi.EHM_E_NO_DEVICE
        return
    # a device is present: a rollout before a plant is set is refused, not computed
    with pytest.raises(ValueError):
        law.rollout(np.zeros((1, 2)), 3)
    rc = lib.ehm_explicit_rollout(law._handle, 2, 3, np.zeros(4).ctypes.data, None, None, 1e-9,
                                  None, None, None, *[a.ctypes.data for a in out], None)
    assert rc == _capi.EHM_E_INVALID and b'no plant' in lib.ehm_explicit_last_error()
    law.close()


def test_flatten_tree_reads_the_commutations():
    """Nested reference trees: every node's commutation comes out with the flat arrays."""
    from explicit_hybrid_mpc_amd import explicit
    from explicit_hybrid_mpc_amd.tree import NodeData, Tree
    mpc = helpers.make_instance('pwa_small')
    seqs = mpc.mode_sequences()
    V = np.array([[0., 0.], [1., 0.], [0., 1.]])
    vi = np.zeros((3, 1))
    root = Tree(NodeData(V, mpc.sequence_to_delta(seqs[0]), np.zeros(3), vi))
    root.grow(NodeData(V * 0.5, mpc.sequence_to_delta(seqs[5]), np.zeros(3), vi),
              NodeData(V + 1., None, np.zeros(3), vi))
    *arrays, nodes, comm = explicit.flatten_tree(root, commutations=True)
    assert len(explicit.flatten_tree(root)) == 5
    assert [n is m for n, m in zip(nodes, [root, root.left, root.right])] == [True] * 3
    assert np.array_equal(comm[1], mpc.sequence_to_delta(seqs[5])) and comm[2] is None
    assert [None if c is None else mpc.step0_mode(c) for c in comm] == [seqs[0][0], seqs[5][0], None]
