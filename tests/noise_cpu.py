"""CPU check of a noisy closed loop (test infrastructure): the recorded v / e / w against the host
sampler of the model, leaf and input at z = x + v against the one-step evaluator, the plant step
with u + e and E w against numpy."""

import numpy as np


def check_noisy_steps(ex, res, X0, T, model, seed, traj0=0):
    """Every recorded step of a noisy explicit rollout; returns the number of applied steps."""
    pl = ex._rollout_plant
    n = X0.shape[0]
    ids = np.arange(traj0, traj0 + n)
    assert np.array_equal(res.x[0], X0)
    u_prev = np.zeros((n, ex.n_u))
    applied = 0
    for t in range(T):
        seen = np.nonzero(res.steps >= t)[0]
        seen = seen[(res.steps[seen] > t) | (res.status[seen] != 0)]      # v of step t drawn
        on = np.nonzero(res.steps > t)[0]                                # step t applied
        assert np.all(np.isnan(res.v[t, res.steps < t]))
        assert np.all(np.isnan(res.e[t, res.steps <= t])) and np.all(np.isnan(res.w[t, res.steps <= t]))
        if seen.size == 0:
            continue
        x = res.x[t, seen]
        v = model.sample('state', seed, ids[seen], t, x, u_prev[seen])
        assert np.array_equal(res.v[t, seen], v)                         # bit-equal
        z = x + v if t > 0 else x
        u_e, leaf_e, _, _ = ex.evaluate(z, return_info=True)
        k = np.isin(seen, on)
        assert np.array_equal(res.u[t, on], u_e[k])                      # bit-equal
        assert np.array_equal(res.leaf[t, on], leaf_e[k])
        if on.size == 0:
            continue
        xo, uo = res.x[t, on], res.u[t, on]
        e = model.sample('input', seed, ids[on], t, xo, uo)
        e[np.sum(uo * uo, axis=1) == 0.] = 0.
        w = model.sample('process', seed, ids[on], t, xo, uo)
        assert np.array_equal(res.e[t, on], e) and np.array_equal(res.w[t, on], w)
        m = ex._node_mode[leaf_e[k]]
        x_np = pl.step(xo, uo + e, m, w if pl.n_d else None)
        scale = np.einsum('nij,nj->ni', np.abs(pl.A[m]), np.abs(xo)) \
            + np.einsum('nij,nj->ni', np.abs(pl.B[m]), np.abs(uo) + np.abs(e)) + np.abs(pl.w[m])
        if pl.n_d:
            scale = scale + np.abs(w) @ np.abs(pl.E.T)
        assert np.all(np.abs(res.x[t + 1, on] - x_np) <= 1e-12 * scale)
        u_prev[on] = uo
        applied += on.size
    fin = res.steps == T
    assert np.array_equal(res.x_final[fin], res.x[T, fin])
    # cost and delta-v stay the commanded input's
    u = np.nan_to_num(res.u)
    assert np.allclose(res.u_norm_sum, np.linalg.norm(u, axis=2).sum(axis=0), rtol=1e-12,
                       atol=1e-300)
    return applied
