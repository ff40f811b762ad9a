"""CPU restatement of the inverted-pendulum law (test infrastructure): the UNCONDENSED big-M program
of lib/mpc_library.py:515-554 for a fixed commutation vector -- states as variables, the active
mode's dynamics as equalities, every other row as the reference writes it with the binaries
substituted -- solved with oracle.qp_numpy, and a literal transcription of the plant's if-cascade
(lib/mpc_library.py:601-623)."""

import numpy as np
import scipy.optimize

from oracle import qp_numpy


def bigm_program(mpc, theta, delta):
    """(P, c, A_ub, b_ub, A_eq, b_eq) in v = [x_0 .. x_N, u_0 .. u_{N-1}], cost 1/2 v'Pv + c'v."""
    N, nx, nm = mpc.N, mpc.n_x, mpc.delta_size
    nv = (N + 1) * nx + N
    X = lambda k: slice(k * nx, (k + 1) * nx)
    U = lambda k: (N + 1) * nx + k
    stride = N if mpc.reference_indexing else nm
    z = [[float(delta[k * stride + i]) for i in range(nm)] for k in range(N)]
    A_ub, b_ub, A_eq, b_eq = [], [], [], []

    def le(coef, rhs):                       # coef . v <= rhs
        A_ub.append(coef)
        b_ub.append(rhs)
    for k in range(N):
        assert sum(z[k]) == 1.
    r = np.zeros((nx, nv))                   # x[0] == theta
    r[:, X(0)] = np.eye(nx)
    A_eq.append(r)
    b_eq.append(np.asarray(theta, dtype=np.float64))
    bigM = mpc.bigM
    for i in range(nm):
        A, B, w = mpc.A[i], mpc.B[i][:, 0], mpc.w[i]
        for k in range(N):
            # x[k+1] <= A x[k] + B u[k] + w + bigM (1 - z)   and   >= ... - bigM (1 - z)
            r = np.zeros((nx, nv))
            r[:, X(k + 1)] = np.eye(nx)
            r[:, X(k)] = -A
            r[:, U(k)] = -B
            if z[k][i] == 1.:
                A_eq.append(r)
                b_eq.append(w.copy())
            else:
                for j in range(nx):
                    le(r[j], w[j] + bigM[j] * (1 - z[k][i]))
                    le(-r[j], -w[j] + bigM[j] * (1 - z[k][i]))
    ve, ae, am, bM2 = mpc.v_eps, mpc.a_eps, mpc.a_max, bigM[2]
    for k in range(N):
        zk = z[k]
        vel = np.zeros(nv)
        vel[k * nx + 2] = 1.
        le(-vel, -(ve * zk[0] - bM2 * (1 - zk[0])))          # x[k][2] >= v_eps z0 - bigM2 (1 - z0)
        le(vel, -ve * zk[1] + bM2 * (1 - zk[1]))             # x[k][2] <= -v_eps z1 + bigM2 (1 - z1)
        s = zk[2] + zk[3] + zk[4]
        le(vel, ve * s + bM2 * (1 - s))
        le(-vel, ve * s + bM2 * (1 - s))

        def accel(i):
            a = np.zeros(nv)
            a[X(k)] = mpc.A_c[i][2]
            a[U(k)] = mpc.B_c[i][2]
            return a, mpc.w_c[i][2]
        a, c = accel(2)                                      # accel_3 >= a_eps z2 - a_max (1 - z2)
        le(-a, c - (ae * zk[2] - am * (1 - zk[2])))
        a, c = accel(3)                                      # accel_4 <= -a_eps z3 + a_max (1 - z3)
        le(a, -ae * zk[3] + am * (1 - zk[3]) - c)
        a, c = accel(4)                                      # -a_eps z4 - a_max .. <= accel_5 <= ..
        le(-a, c + ae * zk[4] + am * (1 - zk[4]))
        le(a, ae * zk[4] + am * (1 - zk[4]) - c)
    for k in range(N):
        e = np.zeros(nv)
        e[U(k)] = 1.
        le(e, mpc.F_max)
        le(-e, mpc.F_max)
    P = np.zeros((nv, nv))
    for k in range(N):
        P[U(k), U(k)] = 2. * mpc.R[0, 0]
    for k in range(1, N + 1):
        P[X(k), X(k)] = 2. * (mpc.P if k == N else mpc.Q)
    return P, np.zeros(nv), np.array(A_ub), np.array(b_ub), np.vstack(A_eq), np.concatenate(b_eq)


def feasible(A_ub, b_ub, A_eq=None, b_eq=None):
    n = A_ub.shape[1]
    r = scipy.optimize.linprog(np.zeros(n), A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq,
                               bounds=[(None, None)] * n, method='highs')
    return r.status == 0


def _check(r):
    """qp_numpy converged, or stalled on a feasible set without interior (some mode sequences
    pin a state to a threshold, e.g. v = v_eps between a held and a sliding step) with a small
    duality gap.  Returns whether it converged."""
    if r.status == 0:
        return True
    assert r.res_p < 1e-9 and r.gap < 1e-6, (r.status, r.res_p, r.gap)
    return False


def solve_bigm(mpc, theta, delta):
    """(feasible, cost, u_0, converged) of the uncondensed program."""
    P, c, A_ub, b_ub, A_eq, b_eq = bigm_program(mpc, theta, delta)
    if not feasible(A_ub, b_ub, A_eq, b_eq):
        return False, np.inf, None, True
    r = qp_numpy.solve(c, A_ub, b_ub, A_eq, b_eq, P=P)
    ok = _check(r)
    return True, float(r.fun), r.x[(mpc.N + 1) * mpc.n_x:(mpc.N + 1) * mpc.n_x + 1], ok


def interior_margin(can, d, theta):
    """Largest r such that a ball of radius r (rows normalised) fits in block d's feasible set."""
    A, b = can.G[d], can.w[d] + can.S[d] @ np.asarray(theta, dtype=np.float64)
    n = A.shape[1]
    r = scipy.optimize.linprog(np.r_[np.zeros(n), -1.], A_ub=np.c_[A, np.linalg.norm(A, axis=1)],
                               b_ub=b, bounds=[(None, None)] * n + [(None, 1.)], method='highs')
    return -r.fun if r.status == 0 else -np.inf


def solve_condensed(can, d, theta):
    """(feasible, cost, u_0, converged) of block d of the compiled law:
    min V(z, theta) s.t. G z <= w + S theta."""
    theta = np.asarray(theta, dtype=np.float64)
    A_ub, b_ub = can.G[d], can.w[d] + can.S[d] @ theta
    if not feasible(A_ub, b_ub):
        return False, np.inf, None, True
    c = can.c + can.f0[d] + can.F[d] @ theta
    r = qp_numpy.solve(c, A_ub, b_ub, P=can.H[d])
    ok = _check(r)
    const = 0.5 * theta @ can.C[d] @ theta + can.c1[d] @ theta + can.c0[d]
    return True, float(r.fun) + const, r.x[:can.n_u], ok


def cascade_step(mpc, A, B, w, x, u):
    """One plant step of lib/mpc_library.py:601-623 as written there: (x_next, case)."""
    v_eps, a_eps = mpc.v_eps, mpc.a_eps
    dxdt = x[2]
    accel = lambda i: (mpc.A_c[i][2].dot(x) + mpc.B_c[i][2] * u + mpc.w_c[i][2])
    if dxdt >= v_eps:
        return A[0].dot(x) + B[0] * u + w[0], 0
    elif dxdt <= -v_eps:
        return A[1].dot(x) + B[1] * u + w[1], 1
    else:
        x_next, case = A[2].dot(x) + B[2] * u + w[2], 2
        d2xdt2 = accel(2)
        if d2xdt2 <= a_eps:
            x_next, case = A[3].dot(x) + B[3] * u + w[3], 3
            d2xdt2 = accel(3)
            if d2xdt2 >= -a_eps:
                x_next, case = A[4].dot(x) + B[4] * u + w[4], 4
        return x_next, case
