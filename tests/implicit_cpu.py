"""
Host mirror of the device loop around the implicit law (csrc/ehm_implicit.hip,
``simulate.rollout_implicit(..., on_device=True)``) in numpy: the same step order, the draws of
``NoiseModel.sample`` (the device sampler bit for bit, tests/noise_cpu.py), and every sum in the
device's order -- columns from 0.0, one rounding per product and per sum (``simulate._dot_rows``):

    x+ = ((A_m x) + (B_m (u + e))) + w_m,  then  + (E d)       (a guarded plant: GuardedPlant.step)

The law is a callable ``z [k, p] -> (u0 [k, n_u], didx [k])`` over the running trajectories (didx
< 0: no law), so a CPU test plugs in ``OracleCPU`` and a GPU test ``oracle.gpu.solve_pt``.  Also the
compaction and selection rules of the device loop restated on whole verdict tables (``compact``,
``select``), pair index i = d n + q as on the device.
"""

import numpy as np

from explicit_hybrid_mpc_amd import simulate
from explicit_hybrid_mpc_amd.simulate import _dot_rows

FEAS_TOL = 1e-8      # EHM_FEAS_TOL
TIE_TOL = 1e-6       # EHM_TIE_TOL


def compact(tau, live):
    """tau [n_delta, n] phase-one optima, live [n]: the second solve's instance list -- (q, pair
    index) of the listed pairs in ascending pair index, and the segment offsets [n_delta + 1]."""
    nd, n = tau.shape
    listed = (tau <= FEAS_TOL) & live[None, :]
    flat = np.flatnonzero(listed.ravel())
    seg = np.concatenate([[0], np.cumsum(listed.sum(axis=1))]).astype(np.int32)
    return (flat % n).astype(np.int64), flat.astype(np.int32), seg


def select(tau, status2, J, u0, live, status1=None):
    """The minimum over the listed pairs with status 0 and the FIRST commutation within TIE_TOL
    (1 + |Jmin|) of it.  tau, status2, J [n_delta, n], u0 [n_delta, n, n_u]; status1 [n_delta, n]
    the status of the phase-one solves (None: all 0) -- a stalled one keeps its tau and is
    counted.  Returns (u [n, n_u] NaN where none, didx [n] -1 where none, stalled pairs of both
    solves per trajectory [n]); rows of stopped trajectories are (NaN, -1, 0)."""
    nd, n = tau.shape
    listed = (tau <= FEAS_TOL) & live[None, :]
    ok = listed & (status2 == 0)
    Jm = np.where(ok, J, np.inf).min(axis=0) if nd else np.full(n, np.inf)
    with np.errstate(invalid='ignore'):
        bound = Jm + TIE_TOL * (1.0 + np.abs(Jm))
        tie = ok & (J <= bound[None, :])
    has = tie.any(axis=0)
    didx = np.where(has, tie.argmax(axis=0), -1).astype(np.int32)
    u = np.full((n, u0.shape[2]), np.nan)
    u[has] = u0[didx[has], np.flatnonzero(has)]
    stalled = (listed & (status2 != 0)).sum(axis=0)
    if status1 is not None:
        stalled = stalled + ((status1 != 0) & live[None, :]).sum(axis=0)
    return u, didx, stalled


def plant_step(plant, X, U, m, D=None):
    """((A_m x) + (B_m u)) + w_m, then + (E d): each product summed over its columns from 0.0."""
    ax = np.zeros_like(X)
    for c in range(plant.n_x):
        ax = ax + plant.A[m, :, c] * X[:, c:c + 1]
    bu = np.zeros_like(X)
    for c in range(plant.n_u):
        bu = bu + plant.B[m, :, c] * U[:, c:c + 1]
    out = (ax + bu) + plant.w[m]
    if D is not None:
        out = out + _dot_rows(plant.E, D)
    return out


def in_region(plant, X, m, tol):
    ok = np.ones(X.shape[0], dtype=bool)
    for mode in np.unique(m):
        r = plant.regions[int(mode)]
        if r is None:
            continue
        sel = m == mode
        H = np.asarray(r[0], dtype=np.float64).reshape(-1, plant.n_x)
        h = np.asarray(r[1], dtype=np.float64).ravel()
        ok[sel] = np.all(_dot_rows(H, X[sel]) <= h + tol, axis=1)
    return ok


def stage_cost(plant, X, U):
    return simulate.GuardedPlant.stage_cost(plant, X, U)


def cwh_states(half, n=512, outside=24):
    """The initial states of the cwh_z cases: uniform in the box `half`, the first `outside` of
    them 1.2 .. 8 half-widths out (no law there: status 3).  With this generator no solve of the
    nominal or of the noisy 60-step run stalls -- about one LP in 2.5 million does, and the
    bit-for-bit comparison with solve_pt holds only where none did."""
    rng = np.random.default_rng(20)
    X0 = rng.uniform(-1, 1, (n, half.size)) * half
    X0[:outside] = rng.uniform(1.2, 8., (outside, half.size)) * half \
        * rng.choice([-1., 1.], (outside, half.size))
    return X0


def rollout(law, plant, mode_of, X0, T, d=None, v=None, noise=None, seed=0, traj0=0,
            tol_exit=1e-9, step=None):
    """The device loop's records and outputs as a dict of arrays (v, e, w only under noise).
    ``step``: another plant step in place of ``plant_step`` (the host loop's einsum, to see what the
    summation order changes)."""
    step = step or plant_step
    X0 = np.ascontiguousarray(np.atleast_2d(X0), dtype=np.float64)
    n, p = X0.shape
    n_u, n_d = plant.n_u, plant.n_d
    mode_of = np.asarray(mode_of, dtype=np.int64)
    ids = np.uint64(int(traj0)) + np.arange(n, dtype=np.uint64)
    x = X0.copy()
    u_prev = np.zeros((n, n_u))
    steps = np.full(n, T, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    cost, unorm = np.zeros(n), np.zeros(n)
    maxv = np.full(n, -np.inf)
    xs = np.full((T + 1, n, p), np.nan)
    xs[0] = x
    us = np.full((T, n, n_u), np.nan)
    cs = np.full((T, n), -1, dtype=np.int32)
    ms = np.full((T, n), -1, dtype=np.int32)
    vs, es, ws = (np.full((T, n, k), np.nan) for k in (p, n_u, n_d))
    for t in range(T):
        live = np.flatnonzero(status == 0)
        if live.size == 0:
            break
        # stage 1: measure
        if noise is not None:
            vt = noise.sample('state', seed, ids[live], t, x[live], u_prev[live])
            vs[t, live] = vt
            z = x[live] + vt if t > 0 else x[live]
        else:
            z = x[live] + v[t, live] if (v is not None and t > 0) else x[live]
        # stages 2-4: the law
        u0, didx = law(z)
        u0, didx = np.asarray(u0, dtype=np.float64), np.asarray(didx)
        bad = (didx < 0) | ~np.all(np.isfinite(u0), axis=1)
        status[live[bad]] = simulate.STATUS_NO_LAW
        steps[live[bad]] = t
        live, u0, didx = live[~bad], u0[~bad], didx[~bad]
        # stage 5: region check at the true state, cost, noise, plant
        m = mode_of[didx]
        xl = x[live]
        if not plant.guarded:
            off = ~in_region(plant, xl, m, tol_exit)
            status[live[off]] = simulate.STATUS_MODE
            steps[live[off]] = t
            live, u0, didx, m, xl = live[~off], u0[~off], didx[~off], m[~off], xl[~off]
        us[t, live], cs[t, live], ms[t, live] = u0, didx, m
        su = np.zeros(live.size)
        for c in range(n_u):
            su = su + u0[:, c] * u0[:, c]
        unorm[live] += np.sqrt(su)
        cost[live] += stage_cost(plant, xl, u0)
        if plant.guarded:
            xn = plant.step(xl, u0)
        elif noise is not None:
            et = noise.sample('input', seed, ids[live], t, xl, u0)
            et[su == 0.] = 0.
            wt = noise.sample('process', seed, ids[live], t, xl, u0)
            es[t, live], ws[t, live] = et, wt
            xn = step(plant, xl, u0 + et, m, wt if n_d else None)
        else:
            xn = step(plant, xl, u0, m, None if d is None else d[t, live])
        if plant.gx.size:
            maxv[live] = np.maximum(maxv[live], (_dot_rows(plant.Gx, xn) - plant.gx).max(axis=1))
        x[live] = xn
        u_prev[live] = u0
        xs[t + 1, live] = xn
    out = dict(x=xs, u=us, commutation=cs, mode=ms, x_final=x, steps=steps, status=status,
               cost=cost, u_norm_sum=unorm, max_violation=maxv)
    if noise is not None:
        out.update(v=vs, e=es, w=ws)
    return out
