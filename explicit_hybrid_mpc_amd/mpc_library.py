"""
MPC problem definitions for the partitioning hot path, and their compilation into
the dense canonical form the HIP kernels consume.

Role in the reference: ``lib/mpc_library.py`` builds CVXPY variables/constraints for
each MPC law and hands ``make_constraints``, ``cost``, ``V``, ``x0``, ``delta``,
``delta_size``, ``N``, ``n_x`` to the Oracle (contract at lib/mpc_library.py:26-39,
constraint pattern at :186-216 and, for big-M PWA dynamics, :521-552).  Here the same
information is carried as plain arrays (a piecewise-affine system, polyhedral state and
input sets, an infinity-norm stage cost), and ``PWAMPC.compile()`` condenses the states
out for every admissible mode sequence ("commutation") so that each oracle sub-problem
becomes

    J*(theta, d) = min_z  c^T z   s.t.   G_d z <= w_d + S_d theta ,      u0 = z[:n_u]

with z = [u_0 .. u_{N-1}, ex_1 .. ex_N, eu_0 .. eu_{N-1}] (inputs, state-cost epigraphs,
input-cost epigraphs).  A fixed commutation turns the reference's big-M rows
(lib/mpc_library.py:530-534) into exact mode dynamics, which is what the condensation
encodes.

Quadratic costs.  Every MPC law of the reference has a ``cvx.quad_form`` cost
(lib/mpc_library.py:180-183, :515-517).  With ``cost='quadratic'`` (and for ``SatelliteZ``)
the compiled form additionally carries, per commutation,

    V(z, theta) = c^T z + 1/2 z^T H_d z + (f0_d + F_d theta)^T z
                  + 1/2 theta^T C_d theta + c1_d^T theta + c0_d ,

so P_theta_delta is a convex QP and the suboptimality test (lib/oracle.py:89-97) a convex
QCQP with two quadratic rows; the infinity-norm epigraph variables are then absent.

The commutation vector layout follows the reference: ``delta[delta_size*k+i] == 1`` iff
mode ``i`` is active at step ``k`` (lib/mpc_library.py:160, lib/oracle.py:463-470); it is a
float64 0/1 vector of length ``delta_size*N``.
"""

import itertools
import numpy as np


class CanonicalLP:
    """
    Dense canonical data for all commutations of one MPC instance.

    Attributes
    ----------
    n, m, p, n_u, N, delta_size : int
        Decision dimension, inequality rows, parameter dimension, inputs, horizon,
        modes per step.
    n_delta : int
        Number of admissible commutations (mode sequences).
    G : (n_delta, m, n) float64     inequality matrix per commutation.
    w : (n_delta, m)    float64     right-hand-side offset.
    S : (n_delta, m, p) float64     right-hand-side parameter gain.
    c : (n,)            float64     linear cost (shared by all commutations).
    deltas : (n_delta, delta_size*N) float64   the 0/1 commutation vectors, in
        enumeration order (this order is the canonical tie-break order).
    """

    def __init__(self, G, w, S, c, deltas, n_u, N, delta_size, quad=None):
        self.G = np.ascontiguousarray(G, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.S = np.ascontiguousarray(S, dtype=np.float64)
        self.c = np.ascontiguousarray(c, dtype=np.float64)
        self.deltas = np.ascontiguousarray(deltas, dtype=np.float64)
        self.n_delta, self.m, self.n = self.G.shape
        self.p = self.S.shape[2]
        self.n_u = int(n_u)
        self.N = int(N)
        self.delta_size = int(delta_size)
        # quadratic part of the cost (None for a pure LP cost): dict with
        #   H (n_delta,n,n), F (n_delta,n,p), f0 (n_delta,n), C (n_delta,p,p), c1 (n_delta,p),
        #   c0 (n_delta,)
        self.quadratic = quad is not None
        if quad is not None:
            for key in ('H', 'F', 'f0', 'C', 'c1', 'c0'):
                setattr(self, key, np.ascontiguousarray(quad[key], dtype=np.float64))
            assert self.H.shape == (self.n_delta, self.n, self.n)
            assert self.F.shape == (self.n_delta, self.n, self.p)

    def cost_value(self, d, z, theta):
        """V(z, theta) of commutation index d."""
        z = np.asarray(z, dtype=np.float64)
        theta = np.asarray(theta, dtype=np.float64)
        v = float(self.c @ z)
        if self.quadratic:
            v += 0.5 * z @ self.H[d] @ z + (self.f0[d] + self.F[d] @ theta) @ z
            v += 0.5 * theta @ self.C[d] @ theta + self.c1[d] @ theta + self.c0[d]
        return float(v)

    def delta_index(self, delta):
        """
        Map a commutation vector to its enumeration index.  The comparison is the
        reference's ``astype(int)`` one (lib/oracle.py:384-385).
        """
        key = np.asarray(delta).astype(int)
        hit = np.nonzero((self.deltas.astype(int) == key[None, :]).all(axis=1))[0]
        if hit.size == 0:
            raise ValueError('commutation %s is not an admissible mode sequence' %
                             (key.tolist(),))
        return int(hit[0])


class PWAMPC:
    """
    Piecewise-affine (hybrid) MPC with polyhedral constraints and an infinity-norm
    stage cost.  A single-mode instance is an ordinary linear MPC.

        x_{k+1} = A_i x_k + B_i u_k + w_i     if mode i is active at step k,
        Hx_i x_k <= hx_i                      (mode region, may be empty),
        Hx_i x_k + Hu_i u_k <= hx_i           (input-dependent mode region, a 3-tuple),
        Gx x_k <= gx , k = 1..N ;  Gu u_k <= gu , k = 0..N-1 ;  x_0 = theta ,
        V = sum_{k=1..N} ||Q x_k||_inf + sum_{k=0..N-1} ||R u_k||_inf          (cost='inf')
        V = sum_{k=0..N-1} u_k'R u_k + sum_{k=1..N-1} x_k'Q x_k + x_N'P x_N     (cost='quadratic',
            the form of lib/mpc_library.py:515-517; Q, R, P symmetric positive semidefinite,
            P defaults to Q).

    Exposes the attribute names of the reference's MPC contract
    (lib/mpc_library.py:26-39): ``N``, ``n_x``, ``n_u``, ``delta_size``.
    """

    def __init__(self, A, B, w, regions, Gx, gx, Gu, gu, Q, R, N, name='pwa_mpc',
                 cost='inf', P=None):
        self.A = [np.asarray(a, dtype=np.float64) for a in A]
        self.B = [np.asarray(b, dtype=np.float64) for b in B]
        self.w = [np.asarray(v, dtype=np.float64) for v in w]
        # regions[i] = (Hx_i, hx_i), (Hx_i, Hu_i, hx_i) or None
        self.regions = [None if r is None else
                        tuple(np.asarray(a, dtype=np.float64) for a in r) for r in regions]
        for r in self.regions:
            if r is not None and len(r) not in (2, 3):
                raise ValueError('a mode region is (Hx, hx) or (Hx, Hu, hx)')
        self.Gx = np.asarray(Gx, dtype=np.float64)
        self.gx = np.asarray(gx, dtype=np.float64)
        self.Gu = np.asarray(Gu, dtype=np.float64)
        self.gu = np.asarray(gu, dtype=np.float64)
        self.Q = np.asarray(Q, dtype=np.float64)
        self.R = np.asarray(R, dtype=np.float64)
        self.N = int(N)
        self.n_x = self.A[0].shape[0]
        self.n_u = self.B[0].shape[1]
        self.delta_size = len(self.A)
        self.name = name
        if cost not in ('inf', 'quadratic'):
            raise ValueError("cost must be 'inf' or 'quadratic'")
        self.cost_type = cost
        self.P = self.Q if P is None else np.asarray(P, dtype=np.float64)
        if cost == 'quadratic':
            for M_, dim in ((self.Q, self.n_x), (self.P, self.n_x), (self.R, self.n_u)):
                if M_.shape != (dim, dim) or not np.allclose(M_, M_.T):
                    raise ValueError('quadratic cost weights must be symmetric and square')
        self._canonical = None

    # -- commutations ---------------------------------------------------------------
    def mode_sequences(self):
        """
        The admissible mode sequences, lexicographic with step 0 most significant: all of them,
        or the subset a caller has restricted the instance to (``restrict``).
        """
        if getattr(self, '_sequences', None) is not None:
            return list(self._sequences)
        return list(itertools.product(range(self.delta_size), repeat=self.N))

    def with_horizon(self, N):
        """The same law over the first ``N`` steps (infinity-norm cost: the stage costs are a plain
        sum, so the relaxation of a mode prefix of at most ``N`` steps -- the undecided steps cost
        nothing and constrain nothing PROVIDED u = 0 is admissible, G_u 0 <= g_u, which
        ``sequences.short_horizon`` checks before it offers the split -- is the same problem in
        either horizon)."""
        if self.cost_type != 'inf':
            raise ValueError('with_horizon: the quadratic cost has a terminal term')
        return PWAMPC(self.A, self.B, self.w, self.regions, self.Gx, self.gx, self.Gu, self.gu,
                      self.Q, self.R, N, name='%s_first%d' % (self.name, N), cost='inf')

    def restrict(self, sequences):
        """
        A copy of this instance whose commutation set is ``sequences`` (sorted into enumeration
        order): what a search over mode prefixes found feasible on a region
        (``sequences.feasible_sequences``) -- the sequences outside cannot be feasible there, so
        every oracle restricted to the region returns what it would with all of them.
        """
        import copy
        out = copy.copy(self)
        out._sequences = sorted(tuple(int(i) for i in s) for s in sequences)
        out._canonical = None
        out._prefix_template = None
        out._prefix_pred = {}
        out.name = '%s_restricted%d' % (self.name, len(out._sequences))
        return out

    def sequence_to_delta(self, seq):
        """Mode sequence -> reference-layout 0/1 vector (lib/mpc_library.py:160)."""
        d = np.zeros(self.delta_size * self.N)
        for k, i in enumerate(seq):
            d[self.delta_size * k + i] = 1.
        return d

    def step0_mode(self, delta):
        """The mode a commutation vector applies at step 0: inverse of ``sequence_to_delta`` on
        the first step (the dynamics the plant follows under this commutation's first input)."""
        return int(np.argmax(np.asarray(delta)[:self.delta_size]))

    # -- condensation ---------------------------------------------------------------
    def _prediction(self, seq):
        """x_k = Phi[k] theta + Gam[k] U + om[k],  U = [u_0;..;u_{N-1}]."""
        n_x, n_u, N = self.n_x, self.n_u, self.N
        Phi = [np.eye(n_x)]
        Gam = [np.zeros((n_x, N * n_u))]
        om = [np.zeros(n_x)]
        for k in range(N):
            i = seq[k]
            A, B, w = self.A[i], self.B[i], self.w[i]
            Phi.append(A @ Phi[k])
            G_next = A @ Gam[k]
            G_next[:, k * n_u:(k + 1) * n_u] += B
            Gam.append(G_next)
            om.append(A @ om[k] + w)
        return Phi, Gam, om

    def n_rows_per_sequence(self, seq):
        m = self.N * (self.Gx.shape[0] + self.Gu.shape[0])
        if self.cost_type == 'inf':
            m += 2 * self.N * (self.Q.shape[0] + self.R.shape[0])
        for k in range(self.N):
            r = self.regions[seq[k]]
            if r is not None:
                m += r[0].shape[0]
        return m

    def _condense(self, seq, m_pad):
        n_x, n_u, N = self.n_x, self.n_u, self.N
        nU = N * n_u
        n = nU + (2 * N if self.cost_type == 'inf' else 0)
        Phi, Gam, om = self._prediction(seq)
        rows_G, rows_w, rows_S = [], [], []

        def add(Gz, wv, Sv):
            rows_G.append(Gz)
            rows_w.append(wv)
            rows_S.append(Sv)

        def pad(M_u):
            out = np.zeros((M_u.shape[0], n))
            out[:, :nU] = M_u
            return out
        # state constraints, k = 1..N :  Gx (Phi th + Gam U + om) <= gx
        for k in range(1, N + 1):
            add(pad(self.Gx @ Gam[k]), self.gx - self.Gx @ om[k], -self.Gx @ Phi[k])
        # input constraints
        for k in range(N):
            M_u = np.zeros((self.Gu.shape[0], nU))
            M_u[:, k * n_u:(k + 1) * n_u] = self.Gu
            add(pad(M_u), self.gu.copy(), np.zeros((self.Gu.shape[0], n_x)))
        # state-cost epigraphs:  +-Q x_k <= ex_k
        for k in (range(1, N + 1) if self.cost_type == 'inf' else ()):
            for sgn in (1., -1.):
                Gz = pad(sgn * self.Q @ Gam[k])
                Gz[:, nU + (k - 1)] = -1.
                add(Gz, -sgn * self.Q @ om[k], -sgn * self.Q @ Phi[k])
        # input-cost epigraphs:  +-R u_k <= eu_k
        for k in (range(N) if self.cost_type == 'inf' else ()):
            for sgn in (1., -1.):
                M_u = np.zeros((self.R.shape[0], nU))
                M_u[:, k * n_u:(k + 1) * n_u] = sgn * self.R
                Gz = pad(M_u)
                Gz[:, nU + N + k] = -1.
                add(Gz, np.zeros(self.R.shape[0]), np.zeros((self.R.shape[0], n_x)))
        # mode regions, k = 0..N-1 :  Hx_i x_k (+ Hu_i u_k) <= hx_i
        for k in range(N):
            r = self.regions[seq[k]]
            if r is not None:
                Hx, hx = r[0], r[-1]
                M_u = Hx @ Gam[k]
                if len(r) == 3:
                    M_u[:, k * n_u:(k + 1) * n_u] += r[1]
                add(pad(M_u), hx - Hx @ om[k], -Hx @ Phi[k])
        G = np.vstack(rows_G)
        w = np.concatenate(rows_w)
        S = np.vstack(rows_S)
        m = G.shape[0]
        if m < m_pad:
            # pad with trivially satisfied rows  0 <= 1  so every commutation shares m
            G = np.vstack([G, np.zeros((m_pad - m, n))])
            w = np.concatenate([w, np.ones(m_pad - m)])
            S = np.vstack([S, np.zeros((m_pad - m, n_x))])
        return G, w, S

    def condense_prefix(self, prefix):
        """
        ``_condense_prefix_reference`` (see there for what the block is), built directly: the
        rows that do not depend on the modes come from a template, the prediction matrices of
        a prefix from its parent's (cached), and only the rows of the decided steps are
        computed.  Bit-identical to the reference form (tests/test_host_logic.py).
        """
        if self.cost_type != 'inf':
            raise ValueError('prefix relaxations are implemented for the infinity-norm cost')
        prefix = tuple(int(i) for i in prefix)
        k, N, n_u, n_x = len(prefix), self.N, self.n_u, self.n_x
        nU = N * n_u
        nGx, nGu, nQ, nR = self.Gx.shape[0], self.Gu.shape[0], self.Q.shape[0], self.R.shape[0]
        tpl = getattr(self, '_prefix_template', None)
        if tpl is None:
            G, w, S = self._condense_prefix_reference(())
            tpl = self._prefix_template = (G, w, S)
            self._prefix_pred = {(): (np.eye(n_x), np.zeros((n_x, nU)), np.zeros(n_x))}
        G, w, S = tpl[0].copy(), tpl[1].copy(), tpl[2].copy()
        pred = self._prefix_pred
        if len(pred) > 200000:
            pred.clear()
            pred[()] = (np.eye(n_x), np.zeros((n_x, nU)), np.zeros(n_x))
        states = [pred[()]]                              # (Phi_j, Gam_j, om_j), j = 0..k
        for j in range(k):
            q = prefix[:j + 1]
            st = pred.get(q)
            if st is None:
                Phi, Gam, om = states[j]
                A, B, wv = self.A[q[j]], self.B[q[j]], self.w[q[j]]
                G_next = A @ Gam
                G_next[:, j * n_u:(j + 1) * n_u] += B
                st = pred[q] = (A @ Phi, G_next, A @ om + wv)
            states.append(st)
        off_q = N * nGx + N * nGu
        off_r = off_q + 2 * N * nQ + 2 * N * nR
        row_r = off_r
        for kk in range(1, k + 1):
            Phi, Gam, om = states[kk]
            r0 = (kk - 1) * nGx                          # state constraints of x_kk
            G[r0:r0 + nGx, :nU] = self.Gx @ Gam
            w[r0:r0 + nGx] = self.gx - self.Gx @ om
            S[r0:r0 + nGx] = -self.Gx @ Phi
            for b, sgn in enumerate((1., -1.)):          # +-Q x_kk <= ex_kk
                r0 = off_q + (2 * (kk - 1) + b) * nQ
                G[r0:r0 + nQ, :nU] = sgn * self.Q @ Gam
                w[r0:r0 + nQ] = -sgn * self.Q @ om
                S[r0:r0 + nQ] = -sgn * self.Q @ Phi
        for kk in range(k):                              # mode regions of x_kk, kk < k
            reg = self.regions[prefix[kk]]
            if reg is not None:
                Hx, hx = reg[0], reg[-1]
                Phi, Gam, om = states[kk]
                nr = Hx.shape[0]
                G[row_r:row_r + nr, :nU] = Hx @ Gam
                if len(reg) == 3:
                    G[row_r:row_r + nr, kk * n_u:(kk + 1) * n_u] += reg[1]
                w[row_r:row_r + nr] = hx - Hx @ om
                S[row_r:row_r + nr] = -Hx @ Phi
                row_r += nr
        return G, w, S

    def _condense_prefix_reference(self, prefix):
        """
        (G, w, S) of the RELAXATION shared by every mode sequence that starts with ``prefix``
        (k = len(prefix) steps fixed): the rows that involve the states x_j, j > k -- state
        constraints, mode regions of the steps >= k -- become 0 <= 1, the epigraph rows of the
        stage costs of x_j, j > k, become e_j >= 0.  Same variables and the same m rows as a
        full sequence, so it is one more block of the commutation table.  Its optimal cost is a
        lower bound, its suboptimality-test optimum an upper bound, and its feasibility a
        necessary condition for every completion (the uncondensed
        statement is oracle/prefix_bb.py).  Infinity-norm costs.
        """
        if self.cost_type != 'inf':
            raise ValueError('prefix relaxations are implemented for the infinity-norm cost')
        prefix = tuple(int(i) for i in prefix)
        k, N, n_u = len(prefix), self.N, self.n_u
        seq = prefix + (0,) * (N - k)
        widest = max(range(self.delta_size),
                     key=lambda i: 0 if self.regions[i] is None else self.regions[i][0].shape[0])
        m_pad = self.n_rows_per_sequence((widest,) * N)      # the m of the compiled table
        G, w, S = self._condense(seq, m_pad)
        nU = N * n_u
        nGx, nGu, nQ, nR = self.Gx.shape[0], self.Gu.shape[0], self.Q.shape[0], self.R.shape[0]
        row = 0
        for kk in range(1, N + 1):                       # state constraints of x_kk
            if kk > k:
                G[row:row + nGx] = 0.
                w[row:row + nGx] = 1.
                S[row:row + nGx] = 0.
            row += nGx
        row += N * nGu                                   # input constraints: kept
        for kk in range(1, N + 1):                       # +-Q x_kk <= ex_kk
            for _ in range(2):
                if kk > k:
                    G[row:row + nQ] = 0.
                    G[row:row + nQ, nU + (kk - 1)] = -1.
                    w[row:row + nQ] = 0.
                    S[row:row + nQ] = 0.
                row += nQ
        row += 2 * N * nR                                # input-cost epigraphs: kept
        for kk in range(N):                              # mode regions of x_kk
            r = self.regions[seq[kk]]
            if r is not None:
                nr = r[0].shape[0]
                if kk >= k:
                    G[row:row + nr] = 0.
                    w[row:row + nr] = 1.
                    S[row:row + nr] = 0.
                row += nr
        return G, w, S

    def _quadratic_cost(self, seq):
        """
        V as a function of (U, theta) for one mode sequence (x_k = Phi_k theta + Gam_k U + om_k):
        1/2 U'H U + (f0 + F theta)'U + 1/2 theta'C theta + c1'theta + c0.
        """
        n_x, n_u, N = self.n_x, self.n_u, self.N
        nU = N * n_u
        Phi, Gam, om = self._prediction(seq)
        H = np.zeros((nU, nU))
        F = np.zeros((nU, n_x))
        f0 = np.zeros(nU)
        C = np.zeros((n_x, n_x))
        c1 = np.zeros(n_x)
        c0 = 0.
        for k in range(N):
            H[k * n_u:(k + 1) * n_u, k * n_u:(k + 1) * n_u] += 2. * self.R
        for k in range(1, N + 1):
            W = self.P if k == N else self.Q
            H += 2. * Gam[k].T @ W @ Gam[k]
            F += 2. * Gam[k].T @ W @ Phi[k]
            f0 += 2. * Gam[k].T @ W @ om[k]
            C += 2. * Phi[k].T @ W @ Phi[k]
            c1 += 2. * Phi[k].T @ W @ om[k]
            c0 += om[k] @ W @ om[k]
        return dict(H=0.5 * (H + H.T), F=F, f0=f0, C=0.5 * (C + C.T), c1=c1, c0=c0)

    def compile(self):
        """Condense every admissible commutation.  Returns a CanonicalLP."""
        if self._canonical is not None:
            return self._canonical
        seqs = self.mode_sequences()
        m_pad = max(self.n_rows_per_sequence(s) for s in seqs)
        Gs, ws, Ss, ds = [], [], [], []
        for s in seqs:
            G, w, S = self._condense(s, m_pad)
            Gs.append(G)
            ws.append(w)
            Ss.append(S)
            ds.append(self.sequence_to_delta(s))
        nU = self.N * self.n_u
        quad = None
        if self.cost_type == 'quadratic':
            c = np.zeros(nU)
            parts = [self._quadratic_cost(s) for s in seqs]
            quad = {key: np.stack([q[key] for q in parts]) for key in parts[0]}
        else:
            c = np.concatenate([np.zeros(nU), np.ones(2 * self.N)])
        self._canonical = CanonicalLP(np.stack(Gs), np.stack(ws), np.stack(Ss), c,
                                      np.stack(ds), self.n_u, self.N, self.delta_size,
                                      quad=quad)
        return self._canonical


def satellite_parameters():
    """Common CWH parameters, lib/mpc_library.py:794-823 (same names and values)."""
    pars = {'mu': 3.986004418e14,   # [m^3*s^-2] standard gravitational parameter
            'R_E': 6378137.,        # [m] Earth mean radius
            'h_E': 415e3,           # [m] orbit height
            'T_s': 100,             # [s] silent time
            'pos_err_max': 10e-2,   # [m]
            'vel_err_max': 1e-3,    # [m/s]
            'delta_v_max': 2e-3,    # [m/s]
            'w_max': 50e-9,         # [m/s^2] exogenous acceleration
            'sigma_fix': 1e-6,      # [m/s] fixed input error
            'sigma_pos': 2e-2,      # position estimate error growth slope
            'sigma_vel': 1e-3,      # velocity estimate error growth slope
            'input_ang_err': 2.,    # [deg] input error cone opening angle
            'p_max': 0.4e-2,        # [m] position estimate error
            'v_max': 4e-6}          # [m/s] velocity estimate error
    pars['a'] = pars['h_E'] + pars['R_E']
    pars['wo'] = np.sqrt(pars['mu'] / pars['a'] ** 3)
    pars['delta_v_min'] = pars['delta_v_max'] * 0.01
    pars['sigma_rcs'] = np.tan(np.deg2rad(pars['input_ang_err']) / 2.)
    return pars


class SatelliteZ:
    """
    The reference's ``SatelliteZ`` law ("cwh_z", lib/mpc_library.py:221-272 on top of
    ``MPC.setup_RMPC`` :61-219): CWH out-of-plane dynamics, input either off or on with a
    minimum impulse (U_ext minus U_int = two intervals, so ``delta_size`` = 2 and a step may
    also have no active piece), state constraints tightened against box-bounded process /
    estimation noise and against noise whose bound grows with |position|, |velocity| and
    |input|, quadratic cost  sum_k (u_k/dv_max)^2 + 1e-2 sum_{k=1..N} |D_x^-1 x_k|^2.

    With one position dimension every norm of the uncertainty model is an absolute value, so
    for a fixed commutation the law is a convex QP; ``compile()`` condenses it to

        z = [u_0..u_{N-1} | apos_0, avel_0, .., apos_{N-1}, avel_{N-1}]      (n = 3N)

    with ``a >= |x|`` epigraph rows (|u_k| needs none: its sign is fixed by the active
    input piece).  A step with no active piece has u_k = 0: its column is removed from the
    constraints and from the state part of the cost, and the input weight keeps the
    variable at zero.  Commutation sequences are per-step values 0 (off) or 1 + piece.

    The two- and three-axis laws (lib/mpc_library.py:274-405) carry genuine second-order
    cone rows (2-norms of 2-/3-vectors) and are outside this LP/QP path.
    """

    def __init__(self, N=4, name='cwh_z'):
        import scipy.linalg as sla
        pars = satellite_parameters()
        self.pars = pars
        self.N = int(N)
        self.n_x, self.n_u = 2, 1
        self.delta_size = 2
        self.T_s = pars['T_s']
        self.name = name
        A_c = np.array([[0., 1.], [-pars['wo'] ** 2, 0.]])
        B_c = np.array([[0.], [1.]])
        self.A = sla.expm(A_c * self.T_s)                         # :260-261
        self.B = self.A @ B_c
        Mx = np.block([[A_c, B_c], [np.zeros((1, 3))]])
        self.E = sla.expm(Mx * self.T_s)[:2, 2:]                  # :262-263
        self.Gx = np.array([[1., 0.], [-1., 0.], [0., 1.], [0., -1.]])
        self.gx = np.array([pars['pos_err_max']] * 2 + [pars['vel_err_max']] * 2)
        self.u_pieces = [(-pars['delta_v_max'], -pars['delta_v_min']),
                         (pars['delta_v_min'], pars['delta_v_max'])]
        self._canonical = None
        self._tightening()

    def _tightening(self):
        """sum_sigma and the dependent-noise coefficients, lib/mpc_library.py:107-138, 197-204."""
        pars, N, A = self.pars, self.N, self.A
        # disturbance gain, lib/plant.py:93-115: p = (process, state est., input, state, state, input)
        D = np.hstack([self.E, -A, self.B, -A, -A, self.B])       # 2 x 9
        ind = D[:, :3]                                             # independent, box-bounded
        ub = np.array([pars['w_max'], pars['p_max'], pars['v_max']])
        dep = [D[:, 3:4], D[:, 4:5], D[:, 7:8], D[:, 8:9]]         # D L_l, one column each
        n_g = self.gx.size
        self.sum_sigma = np.zeros((N + 1, n_g))
        self.coef = np.zeros((N + 1, N, 4, n_g))
        Apow = [np.linalg.matrix_power(A, k) for k in range(N + 1)]
        for k in range(1, N + 1):
            for i in range(k):
                GA = self.Gx @ Apow[k - 1 - i]
                self.sum_sigma[k] += np.abs(GA @ ind) @ ub
                for l in range(4):
                    self.coef[k, i, l] = np.abs(GA @ dep[l])[:, 0]
        self.sigma = np.array([pars['sigma_fix'], pars['sigma_pos'], pars['sigma_vel'],
                               pars['sigma_rcs']])

    # -- commutations ---------------------------------------------------------------
    def mode_sequences(self):
        """Per step 0 = no piece active, 1 + i = input piece i; step 0 most significant."""
        return list(itertools.product(range(self.delta_size + 1), repeat=self.N))

    def sequence_to_delta(self, seq):
        d = np.zeros(self.delta_size * self.N)
        for k, s in enumerate(seq):
            if s > 0:
                d[self.delta_size * k + (s - 1)] = 1.
        return d

    def step0_mode(self, delta):
        """Step-0 value of the commutation: 0 input off, 1 + i input piece i (the plant's
        dynamics are the same in all three)."""
        head = np.asarray(delta)[:self.delta_size]
        return 0 if not head.any() else 1 + int(np.argmax(head))

    def box_vertices(self):
        """Vertices of the partitioned set (lib/examples.py:77-79)."""
        pe, ve = self.pars['pos_err_max'], self.pars['vel_err_max']
        return np.array(list(itertools.product([-pe, pe], [-ve, ve])))

    def _condense(self, seq):
        N = self.N
        n = 3 * N
        oa = N                                   # apos_i at oa + 2 i, avel_i at oa + 2 i + 1
        on = [s > 0 for s in seq]
        Phi = [np.eye(2)]
        Gam = [np.zeros((2, N))]
        for k in range(N):
            Phi.append(self.A @ Phi[k])
            Gn = self.A @ Gam[k]
            if on[k]:
                Gn[:, k] += self.B[:, 0]
            Gam.append(Gn)
        sign_u = [0. if s == 0 else (-1. if s == 1 else 1.) for s in seq]
        rows_G, rows_w, rows_S = [], [], []
        n_g = self.gx.size
        # tightened state rows, k = 1..N
        for k in range(1, N + 1):
            Gz = np.zeros((n_g, n))
            Gz[:, :N] = self.Gx @ Gam[k]
            const = self.sum_sigma[k].copy()
            for i in range(k):
                const += self.coef[k, i, 0] * self.sigma[0]
                Gz[:, oa + 2 * i] += self.coef[k, i, 1] * self.sigma[1]
                Gz[:, oa + 2 * i + 1] += self.coef[k, i, 2] * self.sigma[2]
                Gz[:, i] += self.coef[k, i, 3] * self.sigma[3] * sign_u[i]     # |u_i| = sign u_i
            rows_G.append(Gz)
            rows_w.append(self.gx - const)
            rows_S.append(-self.Gx @ Phi[k])
        # epigraphs  +-x_i[c] - a_{i,c} <= 0 ,  i = 0..N-1
        for i in range(N):
            for cidx in range(2):
                for sgn in (1., -1.):
                    Gz = np.zeros((1, n))
                    Gz[0, :N] = sgn * Gam[i][cidx]
                    Gz[0, oa + 2 * i + cidx] = -1.
                    rows_G.append(Gz)
                    rows_w.append(np.zeros(1))
                    rows_S.append(-sgn * Phi[i][cidx:cidx + 1])
        # input pieces (an inactive step keeps two trivially true rows so m is shared)
        for k in range(N):
            Gz = np.zeros((2, n))
            if on[k]:
                lo, hi = self.u_pieces[seq[k] - 1]
                Gz[0, k], Gz[1, k] = 1., -1.
                rows_w.append(np.array([hi, -lo]))
            else:
                rows_w.append(np.ones(2))
            rows_G.append(Gz)
            rows_S.append(np.zeros((2, 2)))
        G = np.vstack(rows_G)
        w = np.concatenate(rows_w)
        S = np.vstack(rows_S)
        # cost, lib/mpc_library.py:178-184
        H = np.zeros((n, n))
        F = np.zeros((n, 2))
        C = np.zeros((2, 2))
        du = self.pars['delta_v_max']
        H[:N, :N] += 2. * np.eye(N) / du ** 2
        Dxi = np.diag([1. / self.pars['pos_err_max'], 1. / self.pars['vel_err_max']])
        W = 1e-2 * Dxi @ Dxi
        for k in range(1, N + 1):
            H[:N, :N] += 2. * Gam[k].T @ W @ Gam[k]
            F[:N] += 2. * Gam[k].T @ W @ Phi[k]
            C += 2. * Phi[k].T @ W @ Phi[k]
        return G, w, S, dict(H=0.5 * (H + H.T), F=F, f0=np.zeros(n), C=0.5 * (C + C.T),
                             c1=np.zeros(2), c0=0.)

    def compile(self):
        if self._canonical is not None:
            return self._canonical
        seqs = self.mode_sequences()
        Gs, ws, Ss, qs, ds = [], [], [], [], []
        for s in seqs:
            G, w, S, q = self._condense(s)
            Gs.append(G)
            ws.append(w)
            Ss.append(S)
            qs.append(q)
            ds.append(self.sequence_to_delta(s))
        quad = {key: np.stack([q[key] for q in qs]) for key in qs[0]}
        self._canonical = CanonicalLP(np.stack(Gs), np.stack(ws), np.stack(Ss),
                                      np.zeros(3 * self.N), np.stack(ds), self.n_u, self.N,
                                      self.delta_size, quad=quad)
        return self._canonical


# ---------------------------------------------------------------------------------------
# inverted pendulum on a cart with static / kinetic friction (lib/mpc_library.py:407-626,
# lib/pendulum_linearize.py)
# ---------------------------------------------------------------------------------------
def pendulum_parameters():
    """Physical and timing parameters (lib/pendulum_linearize.py:19-41, same names and values)."""
    return {'mu_s': 0.16,        # static friction coefficient
            'mu_d': 0.03,        # kinetic friction coefficient
            'g': 9.81,           # [m/s^2]
            'l': 3.,             # [m] rod length
            'm': 0.3,            # [kg] tip mass
            'M': 1.,             # [kg] cart mass
            'v_eps': 1e-3,       # [m/s] below this speed the cart may stick
            'a_eps': 1e-3,       # [m/s^2] below this acceleration static friction holds
            'T_s': 1 / 10.,      # [s] controller period
            'T_s_plant': 1 / 100.}   # [s] plant period of the simulation


# friction case -> (sign of the friction direction, which coefficient); case 4: stuck
PENDULUM_CASES = ((1., 'mu_d'), (-1., 'mu_d'), (1., 'mu_s'), (-1., 'mu_s'), None)


def pendulum_accelerations(case, theta, dtheta, F, pars, sin, cos):
    """
    (cart acceleration, angular acceleration) of friction case ``case`` (0 sliding right, 1
    sliding left, 2 breaking away right, 3 breaking away left, 4 held), for any arithmetic with
    ``sin`` / ``cos`` (sympy or numpy).  A cart sliding or breaking away in direction s feels a
    friction force -s mu N through the normal force N of the pendulum-loaded cart; held, it does not
    accelerate.  The rod swings as g/l sin(theta) - xdd/l cos(theta).
    """
    g, l, m, M = pars['g'], pars['l'], pars['m'], pars['M']
    if PENDULUM_CASES[case] is None:
        xdd = 0 * F
    else:
        s, key = PENDULUM_CASES[case]
        mu = s * pars[key]
        num = (F - m * g / 2 * sin(2 * theta) + m * l * dtheta ** 2 * (sin(theta) + mu * cos(theta))
               - mu * (M + m * cos(theta) ** 2) * g)
        xdd = num / (M + m * (sin(theta) ** 2 + mu / 2 * sin(2 * theta)))
    return xdd, g / l * sin(theta) - xdd / l * cos(theta)


def pendulum_linearization(pars=None):
    """
    Continuous-time linearisation of the five friction cases at x = 0, F = 0, state
    (position, angle, velocity, angular rate): xdot = A_c x + B_c F + w_c with w_c = f(0)
    (lib/pendulum_linearize.py:43-104).  Returns lists A_c [4x4], B_c [4], w_c [4], float64.
    """
    import sympy as sp
    pars = pendulum_parameters() if pars is None else pars
    pos, th, v, dth, F = sp.symbols('pos theta v dtheta F')
    state = sp.Matrix([pos, th, v, dth])
    at0 = {pos: 0, th: 0, v: 0, dth: 0, F: 0}
    A_c, B_c, w_c = [], [], []
    for case in range(len(PENDULUM_CASES)):
        xdd, thdd = pendulum_accelerations(case, th, dth, F, pars, sp.sin, sp.cos)
        f = sp.Matrix([v, dth, xdd, thdd])
        A_c.append(np.array(f.jacobian(state).subs(at0), dtype=np.float64))
        B_c.append(np.array(f.jacobian(sp.Matrix([F])).subs(at0), dtype=np.float64).ravel())
        w_c.append(np.array(f.subs(at0), dtype=np.float64).ravel())
    return A_c, B_c, w_c


def discretize_affine(A_c, B_c, w_c, h):
    """(A, B, w) of xdot = A_c x + B_c u + w_c held over h (lib/mpc_library.py:556-586)."""
    import scipy.linalg as sla
    n = A_c.shape[0]
    B_c = np.asarray(B_c, dtype=np.float64).reshape(n, -1)
    A = sla.expm(A_c * h)
    nb = B_c.shape[1]
    B = sla.expm(np.block([[A_c, B_c], [np.zeros((nb, n + nb))]]) * h)[:n, n:]
    W = sla.expm(np.block([[A_c, np.eye(n)], [np.zeros((n, 2 * n))]]) * h)[:n, n:]
    return A, B, W @ np.asarray(w_c, dtype=np.float64)


def pendulum_sequences(N, reference_indexing=True):
    """
    Admissible mode sequences (step 0 most significant) and their 0/1 commutation vectors.  The
    reference reads the binaries of step k as z[k][i] = delta[k*N + i] (lib/mpc_library.py:524),
    so for N < 5 consecutive steps share entries: a sequence is admissible iff the vector with
    delta[k*N + m_k] = 1 (all else 0) has exactly e_{m_k} in every window z[k].  With
    ``reference_indexing=False`` the layout is delta[5k + i], every sequence admissible.
    """
    n_modes = len(PENDULUM_CASES)
    seqs, deltas = [], []
    for seq in itertools.product(range(n_modes), repeat=N):
        d = np.zeros(n_modes * N)
        stride = N if reference_indexing else n_modes
        for k, i in enumerate(seq):
            d[stride * k + i] = 1.
        if all(np.array_equal(d[stride * k:stride * k + n_modes], np.eye(n_modes)[i])
               for k, i in enumerate(seq)):
            seqs.append(seq)
            deltas.append(d)
    return seqs, deltas


class InvertedPendulumOnCart(PWAMPC):
    """
    The reference's ``InvertedPendulumOnCart`` law (lib/mpc_library.py:407-626): five friction
    cases linearised at the origin and discretised at T_s, quadratic cost with the terminal
    weight of the frictionless LQR design, and the big-M constraints of ``make_constraints``
    (:521-554) with the binaries fixed to a mode sequence.  For mode j active at step k the
    rows are, in (x_k, u_k):

        |(A_j - A_i) x_k + (B_j - B_i) u_k + w_j - w_i| <= bigM   every inactive mode i,
        the four velocity rows and the four acceleration rows of the friction conditions,
        |u_k| <= F_max,

    carried as an input-dependent mode region (Hx, Hu, h) per mode plus the input rows Gu.
    ``reference_indexing`` selects the commutation layout (``pendulum_sequences``).
    """

    def __init__(self, N=4, reference_indexing=True, name=None):
        import scipy.linalg as sla
        pars = pendulum_parameters()
        self.pars = pars
        self.reference_indexing = bool(reference_indexing)
        n_modes = len(PENDULUM_CASES)
        seqs, deltas = pendulum_sequences(N, reference_indexing)
        if len(seqs) > 256:
            raise ValueError(
                'InvertedPendulumOnCart(N=%d, reference_indexing=%s) has %d admissible commutations; '
                'the hybrid engine enumerates at most 256 (N <= 4 with the reference layout, '
                'N <= 3 with the delta[5k+i] layout), and the branch-and-bound engine states only '
                'infinity-norm costs' % (N, reference_indexing, len(seqs)))
        g, l, m, M = pars['g'], pars['l'], pars['m'], pars['M']
        self.v_eps, self.a_eps = pars['v_eps'], pars['a_eps']
        self.T_s, self.T_s_plant = pars['T_s'], pars['T_s_plant']
        self.A_c, self.B_c, self.w_c = pendulum_linearization(pars)
        disc = [discretize_affine(self.A_c[i], self.B_c[i], self.w_c[i], self.T_s)
                for i in range(n_modes)]
        A, B, w = [d[0] for d in disc], [d[1] for d in disc], [d[2] for d in disc]
        # scalings, set and limits (:441-469)
        p_max, v_max, rate_max = 1., 1., np.deg2rad(50)
        ang_max = np.deg2rad(10)
        self.a_max, self.F_max = 30., 20.
        self.bigM = np.array([p_max, ang_max, v_max, rate_max])
        self.p_err, self.v_err = 1., 1.
        self.ang_err, self.rate_err = np.deg2rad(5), np.deg2rad(20)
        self.D_x = np.diag([self.p_err, self.ang_err, self.v_err, self.rate_err])
        self.D_u = np.diag([self.F_max])
        Dxi, Dui = np.linalg.inv(self.D_x), np.linalg.inv(self.D_u)
        Q = Dxi.T @ np.diag([0.1, 1., 1., 10.]) @ Dxi
        R = Dui.T @ np.eye(1) @ Dui
        # terminal weight: DARE of the frictionless model (:443-471)
        A_lqr = np.array([[0, 0, 1, 0], [0, 0, 0, 1], [0, -m * g / M, 0, 0],
                          [0, g / l * (1 + m / M), 0, 0]], dtype=np.float64)
        B_lqr = np.array([0, 0, 1 / M, -1 / (M * l)])
        A_d, B_d, _ = discretize_affine(A_lqr, B_lqr, np.zeros(4), self.T_s)
        P = sla.solve_discrete_are(A_d, B_d, Q, R)
        self.P_dare = P
        regions = [self._mode_region(j, A, B, w) for j in range(n_modes)]
        Gu = np.array([[1.], [-1.]])
        gu = np.array([self.F_max, self.F_max])
        super().__init__(A, B, w, regions, np.zeros((0, 4)), np.zeros(0), Gu, gu, Q, R, N,
                         name=name or 'pendulum_N%d%s' % (N, '' if reference_indexing else '_k5'),
                         cost='quadratic', P=0.5 * (P + P.T))
        self._sequences = list(seqs)
        self._deltas = {s: d for s, d in zip(seqs, deltas)}

    def _mode_region(self, j, A, B, w):
        """(Hx, Hu, h) of the rows that hold at a step whose active mode is j."""
        Hx, Hu, h = [], [], []

        def row(hx, hu, rhs):
            Hx.append(np.asarray(hx, dtype=np.float64))
            Hu.append(np.atleast_1d(np.asarray(hu, dtype=np.float64)))
            h.append(float(rhs))
        # inactive modes' dynamics, relaxed by bigM, with x_{k+1} = A_j x + B_j u + w_j
        for i in range(len(PENDULUM_CASES)):
            if i == j:
                continue
            dA, dB, dw = A[j] - A[i], B[j][:, 0] - B[i][:, 0], w[j] - w[i]
            for r in range(4):
                row(dA[r], dB[r], self.bigM[r] - dw[r])
                row(-dA[r], -dB[r], self.bigM[r] + dw[r])
        z = np.eye(len(PENDULUM_CASES))[j]
        e2 = np.eye(4)[2]
        bM, ve, ae, am = self.bigM[2], self.v_eps, self.a_eps, self.a_max
        s = z[2] + z[3] + z[4]
        row(-e2, 0., -(ve * z[0] - bM * (1 - z[0])))          # v >= v_eps z0 - bigM (1 - z0)
        row(e2, 0., -ve * z[1] + bM * (1 - z[1]))             # v <= -v_eps z1 + bigM (1 - z1)
        row(e2, 0., ve * s + bM * (1 - s))                    # v <= v_eps s + bigM (1 - s)
        row(-e2, 0., ve * s + bM * (1 - s))                   # v >= -v_eps s - bigM (1 - s)
        acc = [(self.A_c[i][2], self.B_c[i][2], self.w_c[i][2]) for i in range(5)]
        a, b, c = acc[2]                                      # accel_3 >= a_eps z2 - a_max (1 - z2)
        row(-a, -b, -(ae * z[2] - am * (1 - z[2])) + c)
        a, b, c = acc[3]                                      # accel_4 <= -a_eps z3 + a_max (1 - z3)
        row(a, b, -ae * z[3] + am * (1 - z[3]) - c)
        a, b, c = acc[4]                                      # |accel_5| <= a_eps z4 + a_max (1 - z4)
        row(-a, -b, ae * z[4] + am * (1 - z[4]) + c)
        row(a, b, ae * z[4] + am * (1 - z[4]) - c)
        return np.array(Hx), np.array(Hu), np.array(h)

    def sequence_to_delta(self, seq):
        """Mode sequence -> the reference's 5N-long 0/1 vector (unused entries 0)."""
        d = self._deltas.get(tuple(int(i) for i in seq))
        if d is None:
            raise ValueError('%s is not an admissible mode sequence' % (tuple(seq),))
        return d.copy()

    def step0_mode(self, delta):
        """The mode of step 0: z[0] = delta[0:5] in either layout."""
        return int(np.argmax(np.asarray(delta)[:self.delta_size]))

    def box_vertices(self):
        """Vertices of the box D_x that is partitioned (lib/examples.py:120-124)."""
        return np.array(list(itertools.product(*[(-h, h) for h in np.diag(self.D_x)])))

    def sections(self):
        """The three boxes the set is split into (v >= v_eps, v <= -v_eps, |v| <= v_eps),
        as (lower, upper) bounds (lib/examples.py:125-145)."""
        lo, hi = -np.diag(self.D_x), np.diag(self.D_x).copy()
        out = []
        for vlo, vhi in ((self.v_eps, self.v_err), (-self.v_err, -self.v_eps),
                         (-self.v_eps, self.v_eps)):
            a, b = lo.copy(), hi.copy()
            a[2], b[2] = vlo, vhi
            out.append((a, b))
        return out

    def guarded_plant(self):
        """The multi-rate friction plant of lib/mpc_library.py:588-626 (simulate.GuardedPlant)."""
        from .simulate import GuardedPlant
        return GuardedPlant.pendulum(self)
