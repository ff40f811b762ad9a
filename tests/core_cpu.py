"""
Numpy mirror of the may-reach relation between a compiled law's leaves and of the invariant core
(csrc/ehm_core.hip); test infrastructure, host only.

    out = core(arrays, leaf_mode, plant, d_box=None, tol_exit=1e-9, tol_side=None, rows='invariant',
               max_fan=4096)
    out.level, out.core, out.status, out.counts, out.n_sweeps       # the fixed point
    out.indptr, out.indices, out.n_edges                            # the relation as CSR
    out.seeds, out.vertices, out.y                                  # what it was built from

``arrays`` are in the layout of ``CompiledLaw.arrays()`` in either precision.  The seeds, the cells
and the vertex successors are ``tests/invariance_cpu.successors``', the plane sums
``tests/certify_cpu.plane_values``', the root sums ``tests/compiled_cpu._weights``'.  Every decision
is a comparison of sums taken in the kernel's order, so the relation and the levels are the
device's bit for bit.
"""

from types import SimpleNamespace

import numpy as np

from tests import certify_cpu as zc
from tests import invariance_cpu as iv

cc = zc.cc
UNRESOLVED = 5
EPS64 = 2. ** -52
EPS32 = 2. ** -23
U32 = 2. ** -24
TINY = 2. ** -126
COUNT_NAMES = ('core', 'transient', 'exits', 'mode_region', 'no_mode', 'no_cell', 'unresolved')


def widening32(a, X, p):
    """The bound on |s as walk32 sums it - s| for a point whose |x_c| <= X_c:
    (p + 3) 2^-24 (((0 + |a_0| X_0) + ..) + |b|) + 2^-126, in the kernel's order."""
    m = 0.
    for c in range(p):
        m = m + abs(a[c]) * X[c]
    m = m + abs(a[p])
    return (float(p + 3) * U32) * m + TINY


def box_terms(G, E, lo, hi):
    """(dmax, dmin) [n]: what the box adds to the extrema of the forms with gradients G [n, p]."""
    n, p = G.shape
    dmax, dmin = np.zeros(n), np.zeros(n)
    if E is None:
        return dmax, dmin
    for k in range(E.shape[1]):
        ge = np.zeros(n)
        for c in range(p):
            ge = ge + G[:, c] * E[c, k]
        a, b = ge * lo[k], ge * hi[k]
        dmax = dmax + np.where(a > b, a, b)
        dmin = dmin + np.where(a < b, a, b)
    return dmax, dmin


def root_boxes(roots):
    return roots.min(axis=1), roots.max(axis=1)


class Image:
    """I(L) = hull{Y} + E [lo, hi]: the vertex successors Y [p+1, p] and the box."""

    def __init__(self, Y, E, lo, hi):
        self.Y, self.E, self.lo, self.hi = Y, E, lo, hi
        self.p = Y.shape[1]
        dmax, dmin = box_terms(np.eye(self.p), E, lo, hi)
        self.hi_x = Y.max(axis=0) + dmax
        self.lo_x = Y.min(axis=0) + dmin
        self.X = np.where(np.abs(self.hi_x) > np.abs(self.lo_x), np.abs(self.hi_x),
                          np.abs(self.lo_x))

    def plane_range(self, rec):
        """(smax, smin) of the plane record over the image."""
        s = zc.plane_values(rec, self.Y, self.p)
        dmax, dmin = box_terms(np.asarray(rec[:self.p], dtype=np.float64)[None], self.E, self.lo,
                               self.hi)
        return s.max() + dmax[0], s.min() + dmin[0]


def candidate_roots(img, root_rec, box_lo, box_hi, tol_side):
    """The roots that can hold a point of the image, ascending: the boxes, then the weights."""
    p = img.p
    pad = float(p + 1) * tol_side
    w = pad * (box_hi - box_lo)
    apart = ((box_lo - w > img.hi_x) | (box_hi + w < img.lo_x)).any(axis=1)
    cand = np.nonzero(~apart)[0]
    if cand.size == 0:
        return cand
    K = cand.size
    rec = root_rec[cand]
    alpha, a0 = cc._weights(np.repeat(rec, p + 1, axis=0), np.tile(img.Y, (K, 1)), p)
    wmax = alpha.reshape(K, p + 1, p).max(axis=1)
    w0max = a0.reshape(K, p + 1).max(axis=1)
    M = rec[:, p:p + p * p].reshape(K, p, p)
    holds = np.ones(K, dtype=bool)
    n_d = 0 if img.E is None else img.E.shape[1]
    ge = np.zeros((K, p, n_d))
    for c in range(p):
        if n_d:
            ge = ge + M[:, :, c, None] * img.E[None, None, c, :]
    d0 = np.zeros(K)
    dq = np.zeros((K, p))
    for k in range(n_d):
        a, b = ge[:, :, k] * img.lo[k], ge[:, :, k] * img.hi[k]
        dq = dq + np.where(a > b, a, b)
        sg = np.zeros(K)
        for q in range(p):
            sg = sg + ge[:, q, k]
        g0 = 0. - sg
        a, b = g0 * img.lo[k], g0 * img.hi[k]
        d0 = d0 + np.where(a > b, a, b)
    holds = ~((wmax + dq) < -tol_side).any(axis=1) & ~((w0max + d0) < -tol_side)
    return cand[holds]


def descend(img, node, ch, entry, single, tol_side, out, max_fan):
    """The leaves below ``entry`` the walk can return for a point of the image, left before right,
    appended to ``out``; False when the row grows beyond max_fan."""
    p = img.p
    stack = [int(entry)]
    while stack:
        k = stack.pop()
        if k < 0:
            out.append(~k)
            if len(out) > max_fan:
                return False
            continue
        rec = node[k]
        smax, smin = img.plane_range(rec)
        slack = tol_side
        if single:
            slack = slack + widening32(np.asarray(rec[:p + 1], dtype=np.float64), img.X, p)
        eps = EPS32 if single else EPS64
        go_left = smax >= -eps - slack
        go_right = smin < -eps + slack
        if go_right:
            stack.append(int(ch[k, 1]))
        if go_left:
            stack.append(int(ch[k, 0]))
    return True


def fixed_point(seed, indptr, indices):
    """level int32 [n]: 0 for a seed, k for a leaf not of a lower level whose row names level
    k - 1, -1 for the rest -- by sweeps, as k_core_sweep."""
    n = seed.size
    level = np.where(seed, 0, -1).astype(np.int32)
    row = np.repeat(np.arange(n), np.diff(indptr))
    for s in range(1, n + 1):
        lt = level[indices]
        hit = (lt >= 0) & (lt < s)
        new = (np.bincount(row[hit], minlength=n) > 0) & (level < 0)
        if not new.any():
            break
        level[new] = s
    return level


def core(arrays, leaf_mode, plant, d_box=None, tol_exit=1e-9, tol_side=None, rows='invariant',
         max_fan=4096, roots=None, seeds=None, nominal=None):
    """``seeds`` / ``nominal``: ``invariance_cpu.successors`` under the box and without it, where
    the caller has them already."""
    h = zc.header(arrays)
    assert h['n_test'] == 0
    p, n_leaf = h['p'], h['n_leaf']
    tol_side = float(tol_exit) if tol_side is None else float(tol_side)
    single = zc.is_single(arrays)
    roots = zc.root_vertices(arrays) if roots is None else roots
    if seeds is None:
        seeds = iv.successors(arrays, leaf_mode, plant, roots=roots, d_box=d_box,
                              tol_exit=tol_exit)
    if nominal is None:
        nominal = seeds if d_box is None else iv.successors(arrays, leaf_mode, plant, roots=roots,
                                                            tol_exit=tol_exit)
    Y = nominal.x_next[:, :, 0, :]
    n_d = 0 if d_box is None else plant.n_d
    E = np.asarray(plant.E, dtype=np.float64).reshape(p, n_d) if n_d else None
    lo, hi = (np.asarray(a, dtype=np.float64).reshape(n_d) for a in d_box) if n_d else (None, None)
    node = np.ascontiguousarray(arrays['node']).reshape(h['n_int'], h['node_stride'])
    ch = zc.children(arrays)
    entry = np.asarray(arrays['root_entry'])
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    box_lo, box_hi = root_boxes(roots)
    status = seeds.status.astype(np.int32).copy()
    wanted = status < iv.NO_MODE
    if rows != 'all':
        wanted &= status == iv.INVARIANT
    wanted &= np.isfinite(Y).all(axis=(1, 2))           # no image without finite successors
    rows_out = [[] for _ in range(n_leaf)]
    for l in np.nonzero(wanted)[0]:
        img = Image(Y[l], E, lo, hi)
        out, ok = [], True
        for r in candidate_roots(img, root_rec, box_lo, box_hi, tol_side):
            ok = descend(img, node, ch, entry[r], single, tol_side, out, max_fan)
            if not ok:
                break
        if ok:
            rows_out[l] = out
        else:
            status[l] = UNRESOLVED
    indptr = np.zeros(n_leaf + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows_out])
    indices = np.array([t for r in rows_out for t in r], dtype=np.int32)
    level = fixed_point(status != iv.INVARIANT, indptr, indices)
    counts = [int((level < 0).sum()), int((level > 0).sum())] + \
        [int(((level == 0) & (status == s)).sum()) for s in range(1, 6)]
    return SimpleNamespace(level=level, core=level < 0, status=status,
                           counts=dict(zip(COUNT_NAMES, counts)), n_sweeps=int(level.max()) + 1,
                           indptr=indptr, indices=indices, n_edges=int(indices.size), seeds=seeds,
                           vertices=seeds.vertices, y=Y, tol_side=tol_side)
