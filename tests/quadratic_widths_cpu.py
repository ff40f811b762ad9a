"""
CPU side of the tests of the quadratic shared-block instances (tests/test_gpu_quadratic_widths.py,
tests/test_host_quadratic_widths.py): the inputs of a row of helpers.QUADRATIC_WIDTH_ROWS, the row
rotations of its canonical form, and the two CPU references of every programme.

Why the inputs look as they do: over the calibrated box of a quadratic linear MPC the optimum of
the point programme has no active inequality, so a kernel that mishandled a constraint row would
still return the (unconstrained) optimum.  The parameters here lie along fixed unit directions at
given fractions of the largest feasible multiple t_max of the direction (one HiGHS LP:
max t s.t. G z - (S d) t <= w), where the rows bind; and since the rows that bind are among the
first 64 (the early stages), every law is also run with its rows rotated by 64 k and 64 k + 1,
which puts the binding rows into every row slot in turn, at lane 0 and at lane 63.
"""

import functools

import numpy as np
from scipy.optimize import linprog

from explicit_hybrid_mpc_amd.mpc_library import CanonicalLP
from oracle import ipm_numpy as ip
from oracle import qp_numpy
from oracle.oracle_cpu import HIGHS_OPTIONS
from tests import helpers

# The seed of the directions.  Any would do for the optima; for the first inputs it is one at which
# no point parameter has a weakly active row (a multiplier of 1e-6 on a slack of 1e-5, say): there
# u0 moves by 1e-6 within the 1e-10 stopping rule, and the two CPU references themselves differ by
# more than the 1e-7 asked of the device.  test_host_quadratic_widths.py asserts that they agree
# on u0 to U0_REF_TOL at every point parameter of every row.
SEED = 29
U0_REF_TOL = 1e-8
N_DIRECTIONS = 5
POINT_FRACTIONS = (0.5, 0.9, 0.98, 0.999)     # of t_max, per direction
SIMPLEX_FRACTIONS = (0.9, 0.98)               # vertices of the simplices lie between these
N_SIMPLICES = 2
NEIGHBOUR = 0.05        # the directions of a simplex: d and d + NEIGHBOUR e_j, normalised
EPS_A_FRAC, EPS_R = 0.05, 0.1     # eps_a = EPS_A_FRAC x the largest vertex cost of the simplices
ACTIVE = 1e-6           # a multiplier above this counts as a binding row
K2Q_NPS = (8, 16, 24, 32)


# ---- the row layout of csrc/ehm_k2.h, restated -----------------------------------------------------
def lp_xbase(m, ne):
    if ne == 0:
        return m
    r = m & 63
    return m if (r != 0 and r + ne <= 64) else (m + 63) & ~63


def lp_slots(m, ne):
    return (lp_xbase(m, ne) + ne + 63) >> 6


def capacity(cols):
    return next(c for c in K2Q_NPS if c >= cols)


def expected_instances(n, m, p):
    """(capacity, slots) of the point programme and of the suboptimality-test programme: k2_pick
    (csrc/ehm_capi.hip) on n columns / m rows and on n + p + 1 columns / m rows + p + 3 extras."""
    return (capacity(n), lp_slots(m, 0)), (capacity(n + p + 1), lp_slots(m, p + 3))


def row_slot(i, m, ne):
    """Slot of row i of a programme with m MPC rows and ne extras (i >= m: extra i - m)."""
    return (i if i < m else lp_xbase(m, ne) + i - m) >> 6


# ---- rotations ---------------------------------------------------------------------------------------
def rotations(m):
    """Row shifts: 64 k and 64 k + 1 for every slot k the MPC rows occupy (0 = the natural order)."""
    return [64 * k + j for k in range((m + 63) // 64) for j in (0, 1)]


def rotate(can, shift):
    """The same law with MPC row i moved to row (i + shift) mod m."""
    if shift == 0:
        return can
    perm = (np.arange(can.m) - shift) % can.m
    quad = {k: getattr(can, k) for k in ('H', 'F', 'f0', 'C', 'c1', 'c0')}
    return CanonicalLP(can.G[:, perm], can.w[:, perm], can.S[:, perm], can.c, can.deltas,
                       can.n_u, can.N, can.delta_size, quad=quad)


# ---- inputs -------------------------------------------------------------------------------------------
def t_max(can, d):
    """Largest t with t d feasible: max t s.t. G z - (S d) t <= w (HiGHS)."""
    A = np.hstack([can.G[0], -(can.S[0] @ d)[:, None]])
    c = np.zeros(can.n + 1)
    c[-1] = -1.
    res = linprog(c, A_ub=A, b_ub=can.w[0], bounds=(None, None), method='highs',
                  options=HIGHS_OPTIONS)
    assert res.status == 0, res.message
    return -float(res.fun)


class Inputs:
    """theta (n_pt, p) point parameters; R (N_SIMPLICES, p + 1, p); inside / outside (n_dir, p):
    0.999 and 1.001 of t_max along each direction."""


@functools.lru_cache(maxsize=None)
def law(row):
    return helpers.quadratic_width_instance(row).compile()


@functools.lru_cache(maxsize=None)
def inputs(row):
    can = law(row)
    p = can.p
    rng = np.random.default_rng(SEED)
    dirs = rng.standard_normal((N_DIRECTIONS, p))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    tm = np.array([t_max(can, d) for d in dirs])
    out = Inputs()
    out.theta = np.array([f * t * d for d, t in zip(dirs, tm) for f in POINT_FRACTIONS])
    out.inside = 0.999 * tm[:, None] * dirs
    out.outside = 1.001 * tm[:, None] * dirs
    R = np.empty((N_SIMPLICES, p + 1, p))
    for k in range(N_SIMPLICES):
        nb = np.vstack([dirs[k], dirs[k] + NEIGHBOUR * np.eye(p)])
        nb /= np.linalg.norm(nb, axis=1)[:, None]
        frac = np.random.default_rng(SEED + 1 + k).uniform(*SIMPLEX_FRACTIONS, p + 1)
        R[k] = np.array([f * t_max(can, d) * d for f, d in zip(frac, nb)])
    out.R = R
    for a in (out.theta, out.inside, out.outside, out.R):
        a.setflags(write=False)
    return out


# ---- the programmes and the two references -------------------------------------------------------------
def solve_qp(pr):
    """oracle/qp_numpy.py on a QuadProgram: (objective, solution, status) -- the augmented-system
    method with its own equilibration, against the normal-equation method of solve_cp."""
    lin = [i for i in range(pr.A.shape[0]) if i not in pr.iq]
    quad = [(k * pr.Q, k * pr.q + pr.A[i], -pr.b[i]) for i, k in zip(pr.iq, pr.kap)]
    out = qp_numpy.solve(pr.c_lin + pr.kappa0 * pr.q, pr.A[lin], pr.b[lin],
                         P=pr.kappa0 * pr.Q, quad=quad)
    ok = out.status == 0 or max(out.res_p, out.res_d, out.gap) <= 1e-9    # OracleCPU.qp_accept
    return float(out.fun) + pr.kappa0 * pr.v0, out.x, 0 if ok else 1


class Reference:
    """Optima of one (row, rotation) by both references.  pt / sl / ms: solve_cp optima of the
    point, suboptimality-test and min-over-simplex programmes, *_qp the same by qp_numpy; u0 the
    first input of the point programmes; vbar (N_SIMPLICES, p + 1) the vertex costs of the
    simplices; slots_hit: the row slots in which some programme has a multiplier above ACTIVE;
    n_active: positive multipliers per point programme; ok: both references converged everywhere."""


@functools.lru_cache(maxsize=None)
def reference(row, shift=0):
    can = rotate(law(row), shift)
    inp = inputs(row)
    m, p = can.m, can.p
    ref = Reference()
    ref.ok = True
    ref.slots_hit = set()
    ref.n_active = []

    def both(pr, ne):
        o = ip.solve_cp(pr)
        obj, x, st = solve_qp(pr)
        ref.ok = ref.ok and o.status == 0 and st == 0
        for i in np.nonzero(o.lam > ACTIVE)[0]:
            ref.slots_hit.add(row_slot(int(i), m, ne))
        return o, obj, x

    n_pt = inp.theta.shape[0]
    ref.pt, ref.pt_qp = np.empty(n_pt), np.empty(n_pt)
    ref.u0, ref.u0_qp = np.empty((n_pt, can.n_u)), np.empty((n_pt, can.n_u))
    for k, th in enumerate(inp.theta):
        o, obj, x = both(ip.assemble_point_quad(can, 0, th), 0)
        ref.pt[k], ref.pt_qp[k] = o.obj, obj
        ref.u0[k], ref.u0_qp[k] = o.x[:can.n_u], x[:can.n_u]
        ref.n_active.append(int((o.lam > ACTIVE).sum()))
    ns = inp.R.shape[0]
    ref.vbar = np.empty((ns, p + 1))
    ref.sl, ref.sl_qp, ref.ms, ref.ms_qp = (np.empty(ns) for _ in range(4))
    for k, R in enumerate(inp.R):
        for v in range(p + 1):
            o, _, _ = both(ip.assemble_point_quad(can, 0, R[v]), 0)
            ref.vbar[k, v] = o.obj
    ref.eps_a = EPS_A_FRAC * float(ref.vbar.max())
    for k, R in enumerate(inp.R):
        o, obj, _ = both(ip.assemble_bar_E_quad(can, 0, R, ref.vbar[k], ref.eps_a, EPS_R), p + 3)
        ref.sl[k], ref.sl_qp[k] = o.obj, obj
        o, obj, _ = both(ip.assemble_min_simplex_quad(can, 0, R), p + 1)
        ref.ms[k], ref.ms_qp[k] = o.obj, obj
    return ref


def feasible_highs(can, theta):
    res = linprog(np.zeros(can.n), A_ub=can.G[0], b_ub=can.w[0] + can.S[0] @ theta,
                  bounds=(None, None), method='highs', options=HIGHS_OPTIONS)
    return res.status == 0
