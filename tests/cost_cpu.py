"""
The numpy mirror of csrc/ehm_cost.hip: the per-leaf weights from a law's cells and
vertex inputs, the max-plus and min-plus recurrences over a relation given as CSR with the empty-row
and tie rules, the paths, and Karp's maximum and minimum cycle mean for the checks of the tests.

Every value of the recurrence is one double addition of a maximum or minimum, so the device's arrays
are these bit for bit; the weights follow the kernel's expression operation for operation.
"""

from types import SimpleNamespace

import numpy as np

from tests import certify_cpu as zc

INT_MAX = np.iinfo(np.int32).max


def pad_constant(p, n_u):
    """c of pad = c eps |R| (the pad)."""
    return float(2 * p + n_u + 8)


def weights(arrays, V=None, U=None):
    """(w_hi, w_lo, pad) [n_leaf] of a law's arrays, NaN for a leaf without a cell.  ``V`` [n, p+1, p]
    and ``U`` [n, p+1, n_u]: the cells and the vertex inputs (None: ``certify_cpu``'s; the device's
    ``cells()`` returns the same)."""
    h = zc.header(arrays)
    p, n_u, n = h['p'], h['n_u'], h['n_leaf']
    single = zc.is_single(arrays)
    if V is None:
        V, st = zc.cells(arrays)
        U = zc.vertex_inputs(arrays, np.arange(n), V, st)
    V = np.asarray(V, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    lr = np.ascontiguousarray(arrays['leaf_rec']).reshape(n, h['leaf_stride']).astype(np.float64)
    has = ~np.isnan(V).any(axis=(1, 2))
    w_hi, w_lo, pad = (np.full(n, np.nan) for _ in range(3))
    with np.errstate(invalid='ignore'):
        top = np.zeros(n)
        for i in range(p + 1):
            su = np.zeros(n)
            for c in range(n_u):
                su = su + U[:, i, c] * U[:, i, c]
            nrm = np.sqrt(su)
            top = nrm if i == 0 else np.where(nrm > top, nrm, top)
        span = np.abs(V - lr[:, None, :p]).max(axis=1)
        if single:
            span = span + np.abs(V).max(axis=1)
        sg, sr = np.zeros(n), np.zeros(n)
        for c in range(n_u):
            mn, mx = U[:, :, c].min(axis=1), U[:, :, c].max(axis=1)
            g = np.where(mn > 0., mn, np.where(-mx > 0., -mx, 0.))
            sg = sg + g * g
            r = np.abs(lr[:, p + c])
            for j in range(p):
                r = r + np.abs(lr[:, p + n_u + c * p + j]) * span[:, j]
            sr = sr + r * r
        eps = 2. ** -24 if single else 2. ** -53
        pd = (pad_constant(p, n_u) * eps) * np.sqrt(sr)
        low = np.sqrt(sg) - pd
    pad[has] = pd[has]
    w_hi[has] = (top + pd)[has]
    w_lo[has] = np.where(low > 0., low, 0.)[has]
    return w_hi, w_lo, pad


def _row_best(value, indptr, indices, largest):
    """(best [n], arg [n]) per row: the largest (smallest) value among the row's targets and the
    smallest target that attains it; (0, -1) for an empty row."""
    n = indptr.size - 1
    width = np.diff(indptr)
    full = width > 0
    best, arg = np.zeros(n), np.full(n, -1, dtype=np.int32)
    if not full.any():
        return best, arg
    at = indptr[:-1][full]
    vals = value[indices]
    red = np.maximum if largest else np.minimum
    b = red.reduceat(vals, at)
    best[full] = b
    cand = np.where(vals == np.repeat(b, width[full]), indices, INT_MAX)
    arg[full] = np.minimum.reduceat(cand, at)
    return best, arg


def right_nested(w, path):
    """w[l_0] + (w[l_1] + (.. + (w[l_(H-1)] + 0))) along path [H + 1], cut at the first -1."""
    s = 0.
    for l in [int(t) for t in path[:-1] if t >= 0][::-1]:
        s = w[l] + s
    return s


def bounds(indptr, indices, domain, w_hi, w_lo, horizon, start=None):
    """``domain``, ``start`` (None: the domain): bool [n].  The fields of ``invariance.CostResult``
    that do not come from a law; ``arg_hi`` / ``arg_lo`` [H, n] and the paths always there."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    domain = np.asarray(domain, dtype=bool)
    start = domain if start is None else np.asarray(start, dtype=bool)
    n = domain.size
    H = int(horizon)
    assert indptr.size == n + 1 and domain.any() and start.any() and not (start & ~domain).any()
    assert domain[indices[np.repeat(domain, np.diff(indptr))]].all(), 'the domain is not closed'
    w_hi = np.where(domain, np.asarray(w_hi, dtype=np.float64), np.nan)
    w_lo = np.where(domain, np.asarray(w_lo, dtype=np.float64), np.nan)
    U = np.where(domain, 0., np.nan)
    L = U.copy()
    max_hi, min_lo, start_hi, start_lo = ([] for _ in range(4))
    arg_hi, arg_lo = np.empty((H, n), np.int32), np.empty((H, n), np.int32)

    def book():
        max_hi.append(U[domain].max())
        min_lo.append(L[domain].min())
        start_hi.append(U[start].max())
        start_lo.append(L[start].min())

    book()
    for k in range(H):
        with np.errstate(invalid='ignore'):
            bu, au = _row_best(U, indptr, indices, True)
            bl, al = _row_best(L, indptr, indices, False)
        U, L = w_hi + bu, w_lo + bl
        arg_hi[k], arg_lo[k] = np.where(domain, au, -1), np.where(domain, al, -1)
        book()
    rows = np.nonzero(start)[0]

    def path(value, target, arg):
        out = np.full(H + 1, -1, dtype=np.int32)
        out[0] = rows[value[rows] == target][0]
        for t in range(H):
            out[t + 1] = -1 if out[t] < 0 else arg[H - 1 - t][out[t]]
        return out

    max_hi, min_lo = np.array(max_hi), np.array(min_lo)
    k = np.arange(H + 1, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        rate_hi, rate_lo = max_hi / k, min_lo / k
    rate_hi[0] = rate_lo[0] = np.nan
    best_k_hi, best_k_lo = 1 + int(np.argmin(rate_hi[1:])), 1 + int(np.argmax(rate_lo[1:]))
    return SimpleNamespace(
        w_hi=w_hi, w_lo=w_lo, hi=U, lo=L, max_hi=max_hi, min_lo=min_lo,
        start_hi=np.array(start_hi), start_lo=np.array(start_lo), rate_hi=rate_hi,
        rate_lo=rate_lo, best_rate_hi=float(rate_hi[best_k_hi]), best_k_hi=best_k_hi,
        best_rate_lo=float(rate_lo[best_k_lo]), best_k_lo=best_k_lo, arg_hi=arg_hi, arg_lo=arg_lo,
        path_hi=path(U, start_hi[-1], arg_hi), path_lo=path(L, start_lo[-1], arg_lo),
        n_domain=int(domain.sum()), n_start=int(start.sum()), horizon=H)


def cycle_mean(indptr, indices, domain, w, largest):
    """Karp's maximum (minimum) cycle mean of the relation on ``domain`` with weight w[l] on every
    edge out of l; None without a cycle.  G_j(v): the best weight of a walk of j edges ending at v,
    from any leaf (a source with free edges to every leaf in front of them)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    rows = np.nonzero(domain)[0]
    m = rows.size
    src = np.repeat(np.arange(domain.size), np.diff(indptr))
    keep = domain[src]
    src, dst = src[keep], indices[keep]
    sign = 1. if largest else -1.
    G = np.full((m + 1, domain.size), -np.inf)
    G[0][rows] = 0.
    for j in range(m):
        np.maximum.at(G[j + 1], dst, G[j][src] + sign * w[src])
    best = None
    for v in rows:
        if G[m][v] == -np.inf:
            continue
        ks = np.nonzero(G[:m, v] > -np.inf)[0]
        lam = min((G[m][v] - G[j][v]) / (m - j) for j in ks)
        best = lam if best is None else max(best, lam)
    return None if best is None else sign * best
