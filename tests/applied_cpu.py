"""
Numpy mirror of the applied-input audit (csrc/ehm_applied.hip); test
infrastructure, host only.  Everything is stated in the device's order of operations -- sums from
0.0 on, one rounding per product and per sum -- so on the same inputs it is bit-equal to the device.
The sampler is the one of tests/audit_cpu.py, run on the law's root cells.
"""

import numpy as np

BINS = 33
N_STATUS = 6


def pack(X, U, cost_u):
    """(theta' [n, p + n_u], constant [n], no_law [n]) as k_applied_pack writes them: a component
    of U that is not finite enters as 0 and flags the sample; constant = 0 + c_0 u_0 + c_1 u_1 .."""
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    bad = ~np.isfinite(U)
    Uz = np.where(bad, 0.0, U)
    k = np.zeros(X.shape[0])
    for j in range(U.shape[1]):
        k = k + cost_u[j] * Uz[:, j]
    return np.concatenate([X, Uz], axis=1), k, bad.any(axis=1).astype(np.int32)


def fall_back(delta_idx, ju, delta_idx_applied, solve_relaxed):
    """(J_u, delta_idx_applied, relaxed) after the second pass of ehm_compiled_audit: the samples at
    which x is feasible and no commutation of the exact problem is are handed, in their order, to
    ``solve_relaxed(indices) -> (J, delta_idx)``; where that finds a commutation its optimum and
    commutation take the exact problem's place and the sample is marked."""
    ju, du = np.array(ju), np.array(delta_idx_applied)
    relaxed = np.zeros(ju.shape[0], dtype=np.int32)
    again = np.nonzero((np.asarray(delta_idx) >= 0) & (du < 0))[0]
    if again.size:
        J, d = solve_relaxed(again)
        took = d >= 0
        ju[again[took]] = J[took]
        du[again[took]] = d[took]
        relaxed[again[took]] = 1
    return ju, du, relaxed


def statuses(ju, konst, vstar, delta_idx, delta_idx_applied, no_law, eps_a, eps_r, rtol):
    """(V_u, status, gap / bound) per sample: 5 infeasible, 4 no_law, 3 inadmissible, 2 negative,
    1 violation, 0 within -- the first that applies."""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        vu = ju + konst
        gap = vu - vstar
        bound = np.maximum(eps_a, eps_r * vstar)
        slack = rtol * (1.0 + np.abs(vstar))
        st = np.zeros(vu.shape[0], dtype=np.int32)
        st[gap > bound + slack] = 1
        st[~(gap >= -slack)] = 2
        st[np.asarray(delta_idx_applied) < 0] = 3
        st[np.asarray(no_law) != 0] = 4
        st[np.asarray(delta_idx) < 0] = 5
        return vu, st, gap / bound


def summary(ids, status, ratio):
    """(counts [6], histogram [33], max ratio, id of the worst sample or -1) as k_applied_reduce and
    the host merge report them."""
    counts = np.bincount(status, minlength=N_STATUS).astype(np.int64)
    judged = status <= 2
    r = ratio[judged]
    bins = np.zeros(r.shape[0], dtype=np.int64)
    inside = (r >= 0.0) & (r <= 1.0)
    bins[inside] = np.minimum((r[inside] * 32.0).astype(np.int64), 31)
    bins[r > 1.0] = BINS - 1
    hist = np.bincount(bins, minlength=BINS).astype(np.int64)
    if r.size == 0 or np.all(np.isnan(r)):
        return counts, hist, -np.inf, -1
    best = np.nanmax(r)
    worst = int(np.min(np.asarray(ids)[judged][r == best]))
    return counts, hist, float(best), worst
