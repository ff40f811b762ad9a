"""
Numpy mirror of the sampled audit (csrc/ehm_audit.hip); test infrastructure, host
only.  Everything is stated in the device's order of operations -- sums from the first term on,
one rounding per product and per sum -- so on the same inputs it is bit-equal to the device.  The
barycentric weights in the located leaf are the evaluation kernel's (products fused into the sums:
``compiled_cpu._weights`` on the records the device holds, ``ExplicitMPC.records``).
"""

import numpy as np

from explicit_hybrid_mpc_amd.noise import philox4x64_10
from tests.compiled_cpu import _weights

UNIFORM, PER_LEAF = 0, 1
BINS = 33


def words(ids, seed, p):
    """uint64 [n, p+1]: word k of sample s is word k % 4 of the Philox block with counter
    (s, k // 4, 0, 0) under the key (seed, 1)."""
    ids = np.asarray(ids, dtype=np.uint64)
    blocks = [philox4x64_10(ids, j, 0, 0, seed, 1) for j in range((p + 4) // 4)]
    return np.stack([blocks[k // 4][k % 4] for k in range(p + 1)], axis=1)


def uniform01(r):
    """Raw words -> doubles in [0, 1): (r >> 11) 2^-53 (exact)."""
    return (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def choose_uniform(u, cdf):
    """First i with cdf[i] > u cdf[-1], at most the last cell."""
    t = u * cdf[-1]
    return np.minimum(np.searchsorted(cdf, t, side='right'), cdf.size - 1).astype(np.int32)


def choose_per_leaf(ids, k):
    return (np.asarray(ids, dtype=np.uint64) // np.uint64(k)).astype(np.int32)


def spacings(U):
    """Barycentric weights [n, p+1] from the uniforms U [n, p]: sorted ascending, then
    w_0 = g_1, w_i = g_(i+1) - g_i, w_p = 1 - g_p."""
    g = np.sort(U, axis=1)
    return np.concatenate([g[:, :1], g[:, 1:] - g[:, :-1], 1.0 - g[:, -1:]], axis=1)


def points(W, R):
    """x_c = w_0 v_0c, then + w_i v_ic for i = 1..p, for weights W [n, p+1] in cells R [n, p+1, p]."""
    x = W[:, 0, None] * R[:, 0]
    for i in range(1, W.shape[1]):
        x = x + W[:, i, None] * R[:, i]
    return x


def sample(cell_vertices, cdf, ids, seed, mode, k=0):
    """(X [n, p], cell [n]) of the sample ids, as k_audit_sample draws them."""
    p = cell_vertices.shape[2]
    w = words(ids, seed, p)
    if mode == PER_LEAF:
        cell = choose_per_leaf(ids, k)
    else:
        cell = choose_uniform(uniform01(w[:, 0]), cdf)
    W = spacings(uniform01(w[:, 1:]))
    return points(W, cell_vertices[cell]), cell


def interpolated_cost(rec, vertex_costs, leaf, X):
    """(Vbar, smallest weight) of X in the leaves `leaf`: Vbar = a_0 c_0, then + c_(i+1) a_(i+1)."""
    p = X.shape[1]
    alpha, a0 = _weights(rec[leaf], X, p)
    c = vertex_costs[leaf]
    v = a0 * c[:, 0]
    lo = a0.copy()
    for i in range(p):
        v = v + c[:, i + 1] * alpha[:, i]
        lo = np.where(alpha[:, i] < lo, alpha[:, i], lo)
    return v, lo


def statuses(vbar, vstar, closed, delta_idx, eps_a, eps_r, rtol):
    """(status, gap / bound) per sample: 4 infeasible, 3 open, 2 negative, 1 violation, 0 within
    contract -- the first that applies."""
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = vbar - vstar
        bound = np.maximum(eps_a, eps_r * vstar)
        slack = rtol * (1.0 + np.abs(vstar))
        st = np.zeros(vbar.shape[0], dtype=np.int32)
        st[gap > bound + slack] = 1
        st[~(gap >= -slack)] = 2
        st[~np.asarray(closed, dtype=bool)] = 3
        st[np.asarray(delta_idx) < 0] = 4
        return st, gap / bound


def summary(ids, status, ratio):
    """(counts [5], histogram [33], max ratio, id of the worst sample or -1) as k_audit_reduce and
    the host merge report them."""
    counts = np.bincount(status, minlength=5).astype(np.int64)
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
