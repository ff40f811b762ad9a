"""
Closed-loop simulation of the explicit and the implicit law (lib/simulator.py,
lib/post_process.py:242-266, 405-420), for whole batches of initial states.

    plant = Plant.from_mpc(mpc)                       # x+ = A_m x + B_m u + w_m + E d
    res = ExplicitMPC(flat, oracle).rollout(X0, T)    # one device thread per trajectory
    res = ImplicitMPC(oracle).rollout(X0, T)          # one batched P_theta per step
    fig = compare(explicit, implicit, X0, T)          # delta-v overconsumption, cost ratio
    sim = Simulator(law, T_final).run(x0)             # the reference's SimulationOutput

Conventions (both laws): at step t the law sees z_t = x_t + v_t (no error at t = 0, as in
lib/simulator.py:168); the plant steps in the step-0 mode m of the commutation the law used;
a trajectory STOPS -- no input applied, ``steps`` = t -- with status 1 if the explicit law's leaf
does not hold z_t (a barycentric weight < -tol_exit: the state left the partitioned set; the
reference would extrapolate), 2 if mode m's region does not hold x_t (theory says this cannot
happen: a check), 3 if there is no law at z_t (implicit: P_theta infeasible; explicit: a leaf
without a commutation).  Disturbances d [T][n][n_d] and measurement errors v [T][n][p] are passed
in by the caller, or drawn from an uncertainty model (``noise=``, a ``noise.NoiseModel``; the
reference's samplers, lib/simulator.py:160-180): at step t, v_t at the true state x_t and the last
commanded input, then the law's u_t, then the input error e_t (0 where u_t = 0) and d_t at x_t and
u_t; the plant steps with u_t + e_t, while cost, sum ||u|| and the recorded u stay the commanded
input's.  Both laws draw with the same counters (trajectory id traj0 + q), so the explicit and the
implicit rollout of one seed see common random numbers.

A ``GuardedPlant`` (the pendulum's, ``Plant.from_mpc`` of an ``InvertedPendulumOnCart``) runs S
plant steps per controller step with u held and picks each step's mode itself from ordered guards
on (x, u); there is no status 2, no d and no noise model, and ``mode`` is not recorded.
"""

import time

import numpy as np

STATUS_OK, STATUS_EXIT, STATUS_MODE, STATUS_NO_LAW = 0, 1, 2, 3


class _PlantBase:
    """What both kinds of plant hold: modes A [m, n_x, n_x], B [m, n_x, n_u], w [m, n_x], the
    disturbance map E [n_x, n_d], the state rows Gx x <= gx (taken at controller steps) and the
    stage cost ||Q x||_inf + ||R u||_inf (cost 'inf') or x'Qx + u'Ru ('quadratic').  ``guarded``
    tells the kinds apart."""

    guarded = False

    def __init__(self, A, B, w, E, Gx, gx, Q, R, cost, T_s):
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.B = np.ascontiguousarray(B, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.n_modes, self.n_x, self.n_u = self.B.shape
        self.E = np.zeros((self.n_x, 0)) if E is None else np.ascontiguousarray(E, dtype=np.float64)
        self.n_d = self.E.shape[1]
        self.Gx = np.zeros((0, self.n_x)) if Gx is None else np.ascontiguousarray(Gx, np.float64)
        self.gx = np.zeros(0) if gx is None else np.ascontiguousarray(gx, np.float64)
        self.Q = np.ascontiguousarray(Q, dtype=np.float64)
        self.R = np.ascontiguousarray(R, dtype=np.float64)
        if cost not in ('inf', 'quadratic'):
            raise ValueError("cost must be 'inf' or 'quadratic'")
        self.cost = cost
        self.T_s = T_s


class Plant(_PlantBase):
    """
    Plant of a law with the controller's period: x+ = A[m] x + B[m] u + w[m] + E d, mode m
    admissible where H_m x <= h_m (``regions[m]``, None = everywhere).
    """

    def __init__(self, A, B, w, E, regions, Gx, gx, Q, R, cost, T_s=None):
        super().__init__(A, B, w, E, Gx, gx, Q, R, cost, T_s)
        self.regions = list(regions)

    @classmethod
    def from_mpc(cls, mpc):
        """The plant of a ``PWAMPC`` (its modes, regions and cost) or of a ``SatelliteZ``
        (``LinearPlant(T_s, A, B, E)`` of lib/mpc_library.py:258-269; one mode per step-0
        commutation value -- off, piece 0, piece 1 -- all with the same dynamics; the quadratic
        weights of its cost, R = 1/dv_max^2, Q = 1e-2 D_x^-2)."""
        if hasattr(mpc, 'guarded_plant'):
            return mpc.guarded_plant()
        if any(r is not None and len(r) == 3 for r in getattr(mpc, 'regions', ())):
            raise ValueError('a law with input-dependent mode regions needs a plant of its own')
        if hasattr(mpc, 'u_pieces'):
            pars = mpc.pars
            k = mpc.delta_size + 1
            Dxi = np.diag([1. / pars['pos_err_max'], 1. / pars['vel_err_max']])
            return cls([mpc.A] * k, [mpc.B] * k, [np.zeros(mpc.n_x)] * k, mpc.E, [None] * k,
                       mpc.Gx, mpc.gx, 1e-2 * Dxi @ Dxi,
                       np.array([[1. / pars['delta_v_max'] ** 2]]), 'quadratic', T_s=mpc.T_s)
        return cls(mpc.A, mpc.B, mpc.w, None, mpc.regions, mpc.Gx, mpc.gx, mpc.Q, mpc.R,
                   mpc.cost_type, T_s=getattr(mpc, 'T_s', None))

    def region_arrays(self):
        """(rows per mode, H stacked, h stacked) of the mode regions."""
        rows, H, h = [], [np.zeros((0, self.n_x))], [np.zeros(0)]
        for r in self.regions:
            rows.append(0 if r is None else len(r[1]))
            if r is not None:
                H.append(np.asarray(r[0], dtype=np.float64).reshape(-1, self.n_x))
                h.append(np.asarray(r[1], dtype=np.float64).ravel())
        return np.array(rows, dtype=np.int32), np.vstack(H), np.concatenate(h)

    def in_region(self, X, m, tol):
        """bool [n]: mode m[i]'s region holds X[i] (within tol)."""
        X = np.atleast_2d(X)
        ok = np.ones(X.shape[0], dtype=bool)
        for mode in np.unique(m):
            r = self.regions[int(mode)]
            if r is None:
                continue
            sel = m == mode
            ok[sel] = np.all(X[sel] @ r[0].T <= r[1] + tol, axis=1)
        return ok

    def step(self, X, U, m, D=None):
        """x+ for rows X [n, n_x], U [n, n_u], modes m [n], disturbances D [n, n_d] or None."""
        out = np.einsum('nij,nj->ni', self.A[m], X) + np.einsum('nij,nj->ni', self.B[m], U) \
            + self.w[m]
        if D is not None:
            out = out + D @ self.E.T
        return out

    def stage_cost(self, X, U):
        if self.cost == 'inf':
            return np.abs(X @ self.Q.T).max(axis=1) + np.abs(U @ self.R.T).max(axis=1)
        return np.einsum('ni,ij,nj->n', X, self.Q, X) + np.einsum('ni,ij,nj->n', U, self.R, U)


def _dot_rows(M, X):
    """[n, r] = X @ M.T summed in column order from 0.0, one rounding per product and per sum (no
    FMA): the order of the device's sums."""
    out = np.zeros((X.shape[0], M.shape[0]))
    for c in range(M.shape[1]):
        out = out + X[:, c:c + 1] * M[None, :, c]
    return out


class GuardedPlant(_PlantBase):
    """
    A multi-rate piecewise-affine plant that picks its own mode (lib/simulator.py:124-188 with a
    plant such as lib/mpc_library.py:588-626): modes x+ = A[m] x + B[m] u + w[m] at the plant
    period, ``substeps`` S plant steps per controller period (an integer, as lib/simulator.py:91
    assumes), u held over them.  Before each plant step the mode is the first guard whose rows all
    hold, else ``default_mode``; a guard row is

        r = ((sum_c a_c x_c) + sum_c b_c u_c) + c      compared  r <= t  (or  r < t, ``strict``),

    i.e. a.x + b.u + c - t (<= | <) 0 with the sum rounded independently of the threshold t.
    ``guards``: list of (mode, rows), rows a list of (a [n_x], b [n_u], c, t, strict).  Stage cost
    x'Qx + u'Ru (or inf-norm) and the state rows Gx x <= gx are taken at controller steps.  The
    numpy step below is the device's (ehm_explicit_set_plant_guarded) bit for bit: sums in a fixed
    order from 0.0, no FMA.
    """

    guarded = True

    def __init__(self, A, B, w, substeps, guards, default_mode, Q, R, cost='quadratic', Gx=None,
                 gx=None, T_s=None, T_s_plant=None):
        super().__init__(A, B, w, None, Gx, gx, Q, R, cost, T_s)
        if int(substeps) != substeps or substeps < 1:
            raise ValueError('substeps must be a positive integer')
        self.substeps = int(substeps)
        self.default_mode = int(default_mode)
        self.guards = []
        for mode, rows in guards:
            if not 0 <= int(mode) < self.n_modes or not rows:
                raise ValueError('a guard needs a mode of the plant and at least one row')
            self.guards.append((int(mode), [(np.asarray(a, dtype=np.float64).reshape(self.n_x),
                                             np.asarray(b, dtype=np.float64).reshape(self.n_u),
                                             float(c), float(t), bool(st))
                                            for a, b, c, t, st in rows]))
        if not 0 <= self.default_mode < self.n_modes:
            raise ValueError('the default mode is not a mode of the plant')
        self.T_s_plant = T_s_plant

    @classmethod
    def pendulum(cls, mpc):
        """The friction plant of an ``InvertedPendulumOnCart``: its five cases discretised at
        T_s_plant, guards [v >= v_eps -> 0, v <= -v_eps -> 1, accel_2 > a_eps -> 2,
        accel_3 < -a_eps -> 3], default 4 -- the if-cascade of lib/mpc_library.py:601-623, accel_i
        the continuous-time row A_c[i][2] x + B_c[i][2] u + w_c[i][2]."""
        from .mpc_library import discretize_affine
        S = mpc.T_s / mpc.T_s_plant
        if abs(S - round(S)) > 1e-9:
            raise ValueError('the controller period is not a multiple of the plant period')
        disc = [discretize_affine(mpc.A_c[i], mpc.B_c[i], mpc.w_c[i], mpc.T_s_plant)
                for i in range(len(mpc.A_c))]
        e2 = np.eye(mpc.n_x)[2]
        z = np.zeros(mpc.n_u)
        acc = lambda i: (mpc.A_c[i][2], np.atleast_1d(mpc.B_c[i][2]), mpc.w_c[i][2])
        a2, b2, c2 = acc(2)
        a3, b3, c3 = acc(3)
        guards = [(0, [(-e2, z, 0., -mpc.v_eps, False)]),        # v >= v_eps
                  (1, [(e2, z, 0., -mpc.v_eps, False)]),         # v <= -v_eps
                  (2, [(-a2, -b2, -c2, -mpc.a_eps, True)]),      # accel_2 > a_eps
                  (3, [(a3, b3, c3, -mpc.a_eps, True)])]         # accel_3 < -a_eps
        return cls([d[0] for d in disc], [d[1] for d in disc], [d[2] for d in disc], round(S),
                   guards, 4, mpc.Q, mpc.R, cost=mpc.cost_type, T_s=mpc.T_s,
                   T_s_plant=mpc.T_s_plant)

    def guard_arrays(self):
        """Packed guards: mode [g] int32, row0 [g+1] int32, a [r, n_x], b [r, n_u], c [r], t [r],
        strict [r] int32."""
        mode, row0, a, b, c, t, st = [], [0], [], [], [], [], []
        for m, rows in self.guards:
            mode.append(m)
            for ra, rb, rc, rt, rs in rows:
                a.append(ra)
                b.append(rb)
                c.append(rc)
                t.append(rt)
                st.append(int(rs))
            row0.append(len(c))
        i32 = lambda v: np.array(v, dtype=np.int32)
        return (i32(mode), i32(row0), np.array(a, dtype=np.float64).reshape(-1, self.n_x),
                np.array(b, dtype=np.float64).reshape(-1, self.n_u), np.array(c, dtype=np.float64),
                np.array(t, dtype=np.float64), i32(st))

    def select_mode(self, X, U):
        """int [n]: the mode each (x, u) row steps in."""
        X, U = np.atleast_2d(X), np.atleast_2d(U)
        mode = np.full(X.shape[0], self.default_mode, dtype=np.int64)
        open_ = np.ones(X.shape[0], dtype=bool)
        for m, rows in self.guards:
            ok = open_.copy()
            for a, b, c, t, strict in rows:
                r = _dot_rows(a[None], X)[:, 0]
                for j in range(self.n_u):
                    r = r + b[j] * U[:, j]
                r = r + c
                ok &= (r < t) if strict else (r <= t)
            mode[ok] = m
            open_ &= ~ok
        return mode

    def plant_step(self, X, U):
        """One plant period: (x+ [n, n_x], mode [n])."""
        X, U = np.atleast_2d(X), np.atleast_2d(U)
        m = self.select_mode(X, U)
        out = np.zeros_like(X)
        for i in range(self.n_x):
            s = np.zeros(X.shape[0])
            for c in range(self.n_x):
                s = s + self.A[m, i, c] * X[:, c]
            for c in range(self.n_u):
                s = s + self.B[m, i, c] * U[:, c]
            out[:, i] = s + self.w[m, i]
        return out, m

    def step(self, X, U, m=None, D=None):
        """x after one controller period (S plant steps with u held); ``m`` is ignored -- the
        plant chooses its own modes."""
        if D is not None:
            raise ValueError('a guarded plant takes no disturbance')
        for _ in range(self.substeps):
            X, _ = self.plant_step(X, U)
        return X

    def stage_cost(self, X, U):
        """The stage cost at a controller step, in the device's summation order."""
        if self.cost == 'inf':
            return np.abs(_dot_rows(self.Q, X)).max(axis=1) + np.abs(_dot_rows(self.R, U)).max(axis=1)
        s = np.zeros(X.shape[0])
        QX = _dot_rows(self.Q, X)
        for i in range(self.n_x):
            s = s + X[:, i] * QX[:, i]
        RU = _dot_rows(self.R, U)
        for i in range(self.n_u):
            s = s + U[:, i] * RU[:, i]
        return s

    def in_region(self, X, m, tol):
        return np.ones(np.atleast_2d(X).shape[0], dtype=bool)


def reference_call_steps(T_f, h_plant, h_ctrl):
    """The plant-step indices at which lib/simulator.py:150-165 calls the controller: plant times
    linspace(0, T_f, int(T_f / h_plant + 1)), a call where t - t_last >= h_ctrl - eps."""
    times = np.linspace(0, T_f, int(T_f / h_plant + 1))
    eps = np.finfo(float).eps
    calls, last = [], None
    for j, t in enumerate(times):
        if last is None or t - last >= h_ctrl - eps:
            last = t
            calls.append(j)
    return np.array(calls, dtype=np.int64), times


class ClosedLoop:
    """
    Result of a batched rollout (n trajectories, T steps).  Records, time-major, None unless
    asked for: x [T+1, n, n_x], u [T, n, n_u] (NaN after a stop), leaf [T, n] (explicit law,
    -1 after a stop), commutation [T, n] (index into the law's commutations, -1 after a stop),
    mode [T, n] (applied mode, -1 after a stop); under a noise model also v [T, n, n_x] (NaN
    after the step a trajectory stopped at), e [T, n, n_u] and w [T, n, n_d] (NaN from it on).  Always: x_final [n, n_x], steps [n], status [n]
    (STATUS_*), cost [n] (summed stage cost), u_norm_sum [n] (sum_t ||u_t||_2), max_violation [n]
    (max_t max_j (Gx x_{t+1} - gx)_j, -inf without a step), seconds (device time of the explicit
    rollout kernel / wall time of the implicit loop / device time of the implicit device loop,
    which also sets stalled [n] and n_stalled_pairs).
    """

    def __init__(self, **kw):
        self.x = self.u = self.leaf = self.commutation = self.mode = None
        self.v = self.e = self.w = None
        self.seconds = 0.
        self.__dict__.update(kw)

    @property
    def exited(self):
        return self.status == STATUS_EXIT

    @property
    def mode_violations(self):
        return self.status == STATUS_MODE


def _check_rollout_args(plant, noise, d, v, n, p, T):
    """The refusals every rollout shares, before any use of the device.  Returns d [T, n, n_d] and
    v [T, n, p] as contiguous float64 arrays (or None)."""
    if noise is not None and (d is not None or v is not None):
        raise ValueError('noise draws d and v itself: give noise or d / v, not both')
    if plant is None:
        raise ValueError('rollout needs a plant (or an oracle whose mpc gives one)')
    if plant.guarded and noise is not None:
        raise ValueError('noise is not supported with a guarded plant')
    out = []
    for a, shape, name in ((d, (T, n, plant.n_d), 'd'), (v, (T, n, p), 'v')):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != shape:
                raise ValueError('%s must have shape %s, not %s' % (name, shape, a.shape))
        out.append(a)
    return out


def rollout_implicit(oracle, plant, X0, T, d=None, v=None, record=True, tol_exit=1e-9, noise=None,
                     seed=0, traj0=0, on_device=False):
    """
    The implicit law in closed loop: per step one batched ``solve_pt`` (the device's
    mixed-integer oracle) over the live trajectories, the plant step on the host with the
    conventions of the module docstring (``noise``: v, e, d from the host sampler of the
    model).  Returns a ClosedLoop (commutation, no leaf).

    ``on_device=True`` runs the whole loop on the device instead (implicit_device.py,
    ``ehm_implicit_rollout``): the same conventions and ClosedLoop fields, plus ``stalled`` [n] and
    ``n_stalled_pairs`` -- a solve that stalls, in phase one or in the point solve, is not
    repeated on the generation-1 kernels there (phase one keeps its tau, a point solve is left out
    of the minimum), so flagged trajectories may differ from this loop's; ``seconds`` is then the
    device time between the first and the last launch.  It needs an oracle with enumerated
    commutations (not ``bnb.PrefixOracle``), n_u <= 4 and p <= 8.
    """
    X0 = np.ascontiguousarray(np.atleast_2d(X0), dtype=np.float64)
    n, p = X0.shape
    d, v = _check_rollout_args(plant, noise, d, v, n, p, T)
    if noise is not None and (noise.n_x, noise.n_u, noise.n_d) != (p, plant.n_u, plant.n_d):
        raise ValueError('the noise model does not fit the plant')
    if on_device:
        from . import implicit_device
        implicit_device.check_args(oracle, plant)
        return implicit_device.rollout(oracle, plant, X0, T, d=d, v=v, record=record,
                                       tol_exit=tol_exit, noise=noise, seed=seed, traj0=traj0)
    ids = np.uint64(int(traj0)) + np.arange(n, dtype=np.uint64)
    u_prev = np.zeros((n, plant.n_u))
    can = oracle.canonical
    mode_of = np.array([oracle.mpc.step0_mode(dl) for dl in can.deltas], dtype=np.int64)
    x = X0.copy()
    steps = np.full(n, T, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    cost, unorm = np.zeros(n), np.zeros(n)
    maxv = np.full(n, -np.inf)
    if record:
        xs = np.full((T + 1, n, p), np.nan)
        xs[0] = x
        us = np.full((T, n, plant.n_u), np.nan)
        cs = np.full((T, n), -1, dtype=np.int32)
        ms = np.full((T, n), -1, dtype=np.int32)
        if noise is not None:
            vs = np.full((T, n, p), np.nan)
            es = np.full((T, n, plant.n_u), np.nan)
            ws = np.full((T, n, plant.n_d), np.nan)
    live = np.arange(n)
    tic = time.time()
    for t in range(T):
        if live.size == 0:
            break
        if noise is not None:
            vt = noise.sample('state', seed, ids[live], t, x[live], u_prev[live])
            if record:
                vs[t, live] = vt
            z = x[live] + vt if t > 0 else x[live]
        else:
            z = x[live] + v[t, live] if (v is not None and t > 0) else x[live]
        _, u0, didx = oracle.gpu.solve_pt(z)
        bad = (didx < 0) | ~np.all(np.isfinite(u0), axis=1)
        m = mode_of[np.maximum(didx, 0)]
        off = ~bad & ~plant.in_region(x[live], m, tol_exit)
        for sel, code in ((bad, STATUS_NO_LAW), (off, STATUS_MODE)):
            status[live[sel]] = code
            steps[live[sel]] = t
        go = ~(bad | off)
        live, u0, m, didx = live[go], u0[go], m[go], didx[go]
        xl = x[live]
        cost[live] += plant.stage_cost(xl, u0)
        unorm[live] += np.sqrt(np.sum(u0 * u0, axis=1))
        if noise is not None:
            su = np.zeros(live.size)
            for c in range(plant.n_u):
                su = su + u0[:, c] * u0[:, c]
            et = noise.sample('input', seed, ids[live], t, xl, u0)
            et[su == 0.] = 0.
            wt = noise.sample('process', seed, ids[live], t, xl, u0)
            u_prev[live] = u0
            if record:
                es[t, live], ws[t, live] = et, wt
            xn = plant.step(xl, u0 + et, m, wt if plant.n_d else None)
        else:
            xn = plant.step(xl, u0, m, None if d is None else d[t, live])
        if plant.gx.size:
            maxv[live] = np.maximum(maxv[live], (xn @ plant.Gx.T - plant.gx).max(axis=1))
        x[live] = xn
        if record:
            us[t, live] = u0
            cs[t, live] = didx
            ms[t, live] = m
            xs[t + 1, live] = xn
    out = ClosedLoop(x_final=x, steps=steps, status=status, cost=cost, u_norm_sum=unorm,
                     max_violation=maxv, seconds=time.time() - tic)
    if record:
        out.x, out.u, out.commutation, out.mode = xs, us, cs, (None if plant.guarded else ms)
        if noise is not None:
            out.v, out.e, out.w = vs, es, ws
    return out


def compare(explicit, implicit, X0, T, d=None, v=None, tol_exit=1e-9, record=False, noise=None,
            seed=0, implicit_on_device=False):
    """
    The explicit against the implicit law from the same initial states under the same d / v, or
    under the same draws of a noise model (common random numbers: one seed, the same trajectory
    ids) (total_delta_v_usage, lib/post_process.py:242-266).  Per trajectory: ``overconsumption``
    = (sum ||u||_ex - sum ||u||_im) / sum ||u||_im and ``cost_ratio`` = cost_ex / cost_im (NaN
    where the implicit figure is 0).  Aggregates over the trajectories both laws ran for all T
    steps (``both_ok``): ``overconsumption_total`` (the statistic of total_delta_v_usage over
    the summed usage) and ``cost_ratio_total``.  Also the exit / stop counts and the two
    ClosedLoop results (``explicit``, ``implicit``).  ``implicit_on_device``: the implicit law's
    rollout runs on the device (``rollout_implicit(..., on_device=True)``).
    """
    kw = dict(d=d, v=v, record=record, tol_exit=tol_exit)
    if noise is not None:
        kw.update(noise=noise, seed=seed)
    ex = explicit.rollout(X0, T, **kw)
    if implicit_on_device:
        kw['on_device'] = True
    im = implicit.rollout(X0, T, **kw)
    both = (ex.status == STATUS_OK) & (im.status == STATUS_OK)
    with np.errstate(divide='ignore', invalid='ignore'):
        over = np.where(im.u_norm_sum > 0, (ex.u_norm_sum - im.u_norm_sum) / im.u_norm_sum,
                        np.nan)
        ratio = np.where(im.cost > 0, ex.cost / im.cost, np.nan)
    su_ex, su_im = float(ex.u_norm_sum[both].sum()), float(im.u_norm_sum[both].sum())
    sc_ex, sc_im = float(ex.cost[both].sum()), float(im.cost[both].sum())
    return dict(overconsumption=over, cost_ratio=ratio,
                overconsumption_total=(su_ex - su_im) / su_im if su_im > 0 else float('nan'),
                cost_ratio_total=sc_ex / sc_im if sc_im > 0 else float('nan'),
                u_norm_explicit=su_ex, u_norm_implicit=su_im,
                both_ok=int(both.sum()), n=int(both.size),
                exits_explicit=int(ex.exited.sum()),
                mode_violations_explicit=int(ex.mode_violations.sum()),
                stopped_explicit=int((ex.status != STATUS_OK).sum()),
                stopped_implicit=int((im.status != STATUS_OK).sum()),
                explicit=ex, implicit=im)


class SimulationOutput:
    """The reference's simulation record (lib/simulator.py:31-71), already compiled to arrays:
    t, t_call [K]; x [n_x, K], u [n_u, K], w [n_d, K], v [n_x, K], e [n_u, K] column-stacked,
    column k = the state before step k and what acted on it."""

    def __init__(self):
        self.t, self.t_call, self.x, self.u, self.w, self.v, self.e = [], [], [], [], [], [], []


class Simulator:
    """
    ``Simulator(mpc, T).run(x_0, label)`` of lib/simulator.py:73-188 for a law with a
    ``rollout`` (``ExplicitMPC`` / ``ImplicitMPC``): T is the final time, the plant runs at the
    controller's period T_s (1 if the law has none), so the run has int(T / T_s + 1) steps, as
    the reference's time grid.  ``noise``: a ``noise.NoiseModel``, 'reference' for the one the law
    was tightened against (``NoiseModel.from_mpc``), or None (nominal); w, v and e of the record
    are its draws.  A trajectory that stops ends the record.  A law whose plant is guarded (the
    pendulum's) runs the plant at its own period T_s_plant, the grid int(T / T_s_plant + 1) plant
    steps long, and the controller every ``substeps`` of them -- checked against the reference's
    floating-point rule (``reference_call_steps``); the plant-rate record comes from the host
    mirror of the plant, which is the device's bit for bit.
    """

    def __init__(self, mpc, T, noise=None, seed=0):
        self.law = mpc
        self.T_f = T
        if isinstance(noise, str):
            if noise != 'reference':
                raise ValueError("noise must be a NoiseModel, 'reference' or None")
            from .noise import NoiseModel
            noise = NoiseModel.from_mpc(mpc.mpc)
            if noise is None:
                raise ValueError('the law has no uncertainty model of its own')
        self.noise, self.seed = noise, seed
        self.h = getattr(mpc, 'T_s', None) or 1.
        self.sim_history = SimulationOutput()

    def _guarded_plant(self):
        plant = getattr(self.law, '_rollout_plant', None)
        if plant is None and getattr(self.law, 'mpc', None) is not None:
            plant = Plant.from_mpc(self.law.mpc)
        return plant if plant is not None and plant.guarded else None

    def _run_guarded(self, plant, x_0, out):
        calls, times = reference_call_steps(self.T_f, plant.T_s_plant, plant.T_s)
        _check_rollout_args(plant, self.noise, None, None, 1, plant.n_x, len(calls))
        S = plant.substeps
        if not np.array_equal(calls, np.arange(0, len(times), S)):
            raise ValueError('for T = %r the reference calls the controller at plant steps %s, not '
                             'every %d' % (self.T_f, calls[:8].tolist(), S))
        res = self.law.rollout(np.asarray(x_0, dtype=np.float64)[None], len(calls), record=True,
                               plant=plant)
        xs, us, ts, tc = [], [], [], []
        for c in range(int(res.steps[0])):
            x, u = res.x[c, 0], res.u[c, 0]
            for j in range(min(S, len(times) - c * S)):
                xs.append(x)
                us.append(u)
                ts.append(times[c * S + j])
                tc.append(res.seconds / max(len(calls), 1) if j == 0 else 0.)
                x = plant.plant_step(x[None], u[None])[0][0]
        K = len(xs)
        n_x, n_u = plant.n_x, plant.n_u
        out.t, out.t_call = np.array(ts), np.array(tc)
        out.x = np.array(xs).T.reshape(n_x, K)
        out.u = np.array(us).T.reshape(n_u, K)
        out.w, out.v, out.e = np.zeros((0, K)), np.zeros((n_x, K)), np.zeros((n_u, K))
        return out

    def run(self, x_0, label=None):
        out = self.sim_history = SimulationOutput()
        if label is not None:
            out.label = label
        plant = self._guarded_plant()
        if plant is not None:
            return self._run_guarded(plant, x_0, out)
        times = np.linspace(0, self.T_f, int(self.T_f / self.h + 1))
        kw = {} if self.noise is None else dict(noise=self.noise, seed=self.seed)
        res = self.law.rollout(np.asarray(x_0, dtype=np.float64)[None], len(times), record=True,
                               **kw)
        K = int(res.steps[0])
        n_x, n_u = res.x.shape[2], res.u.shape[2]
        n_d = getattr(getattr(self.law, '_rollout_plant', None), 'n_d', 0)
        out.t = times[:K]
        out.t_call = np.full(K, res.seconds / max(len(times), 1))
        out.x = res.x[:K, 0].T.copy().reshape(n_x, K)
        out.u = res.u[:K, 0].T.copy().reshape(n_u, K)
        if self.noise is None:
            out.w = np.zeros((n_d, K))
            out.v = np.zeros((n_x, K))
            out.e = np.zeros((n_u, K))
        else:
            out.w = res.w[:K, 0].T.copy().reshape(n_d, K)
            out.v = res.v[:K, 0].T.copy().reshape(n_x, K)
            out.e = res.e[:K, 0].T.copy().reshape(n_u, K)
        return out
