"""
Numpy mirror of the one-step test and of the core under process, measurement and input error
(csrc/ehm_robust.hip, the per-mode generator block of csrc/ehm_core.hip); test
infrastructure, host only.

    out = successors(arrays, leaf_mode, plant, d_box=None, v_box=None, e_box=None, leaves=None,
                     tol_exit=1e-9, tol_set=1e-9)
    out.status, out.margin, out.worst, out.counts, out.worst_leaf, out.worst_margin
    out.G, out.lo, out.hi, out.slack, out.y, out.vertices, out.modes
    out = core(arrays, leaf_mode, plant, ..., tol_side=None, rows='invariant', max_fan=4096)

The facets are the package's (``invariance.boundary_facets`` of the law's roots), the cells and the
nominal vertex successors ``tests/invariance_cpu.successors``', the rows ``tests/core_cpu``'s with
G_m of the leaf's mode as the image's generator block.  The facet minima and the region maxima are
summed in the kernel's order, so every array is the device's bit for bit.
"""

from types import SimpleNamespace

import numpy as np

from explicit_hybrid_mpc_amd import invariance
from tests import certify_cpu as zc
from tests import core_cpu as kc
from tests import invariance_cpu as iv

INVARIANT, EXITS, MODE_REGION, NO_MODE, NO_CELL = range(5)


def _pair(box, n):
    return tuple(np.asarray(a, dtype=np.float64).reshape(n) for a in box)


def generators(plant, p, n_u, d_box, v_box, e_box):
    """(G [n_modes, p, n_g], lo, hi): G_m = [E | -A_m | B_m | I], the box [d; v; e; v]; the columns
    of a box that is None are left out."""
    n_d = plant.n_d if d_box is not None else 0
    blocks, lo, hi = [], [], []
    for m in range(plant.n_modes):
        A = np.asarray(plant.A[m], dtype=np.float64).reshape(p, p)
        B = np.asarray(plant.B[m], dtype=np.float64).reshape(p, n_u)
        cols = []
        if n_d:
            cols.append(np.asarray(plant.E, dtype=np.float64).reshape(p, n_d))
        if v_box is not None:
            cols.append(-A)
        if e_box is not None:
            cols.append(B)
        if v_box is not None:
            cols.append(np.eye(p))
        blocks.append(np.hstack(cols) if cols else np.zeros((p, 0)))
    for box, n in ((d_box if n_d else None, n_d), (v_box, p), (e_box, n_u), (v_box, p)):
        if box is not None:
            a, b = _pair(box, n)
            lo.append(a)
            hi.append(b)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
    return np.array(blocks).reshape(plant.n_modes, p, -1), cat(lo), cat(hi)


def facet_slack(normals, G, lo, hi):
    """[n_f, n_modes]: sum_k min(nG_k lo_k, nG_k hi_k) from 0, nG_k = ((0 + n_0 G_0k) + ..)."""
    n_f, p = normals.shape
    n_modes, _, n_g = G.shape
    out = np.zeros((n_f, n_modes))
    for m in range(n_modes):
        s = np.zeros(n_f)
        for k in range(n_g):
            ng = np.zeros(n_f)
            for c in range(p):
                ng = ng + normals[:, c] * G[m, c, k]
            a, b = ng * lo[k], ng * hi[k]
            s = s + np.where(a < b, a, b)
        out[:, m] = s
    return out


def region_holds(plant, V, modes, v_box, tol_exit):
    """bool [L]: every region row of the leaf's mode holds on cell - v box (the kernel's sums)."""
    L, nv, p = V.shape
    rows, H, h = plant.region_arrays()
    rows = np.asarray(rows, dtype=np.int64)
    H = np.asarray(H, dtype=np.float64).reshape(-1, p)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    row0 = np.concatenate([[0], np.cumsum(rows)])
    v_lo, v_hi = _pair(v_box, p) if v_box is not None else (np.zeros(p), np.zeros(p))
    ok = np.ones(L, dtype=bool)
    for m in range(plant.n_modes):
        at = np.nonzero(modes == m)[0]
        if at.size == 0:
            continue
        for r in range(row0[m], row0[m + 1]):
            smax = None
            for i in range(nv):
                s = np.zeros(at.size)
                for c in range(p):
                    s = s + H[r, c] * V[at, i, c]
                smax = s if smax is None else np.where(s > smax, s, smax)
            rs = 0.
            for c in range(p):
                g = 0. - H[r, c]
                a, b = g * v_lo[c], g * v_hi[c]
                rs = rs + (a if a > b else b)
            ok[at] &= (smax + rs) <= h[r] + tol_exit
    return ok


def successors(arrays, leaf_mode, plant, d_box=None, v_box=None, e_box=None, leaves=None,
               roots=None, tol_exit=1e-9, tol_set=1e-9, nominal=None):
    h = zc.header(arrays)
    p, n_u = h['p'], h['n_u']
    roots = zc.root_vertices(arrays) if roots is None else roots
    normals, offsets, convex = invariance.boundary_facets(roots)
    if nominal is None:
        nominal = iv.successors(arrays, leaf_mode, plant, leaves=leaves, roots=roots,
                                tol_exit=tol_exit)
    n = nominal.status.size
    G, lo, hi = generators(plant, p, n_u, d_box, v_box, e_box)
    slack = facet_slack(normals, G, lo, hi)
    thr = float(tol_set) * float(np.abs(roots).max())
    status = np.where(nominal.status >= NO_MODE, nominal.status, INVARIANT).astype(np.int32)
    margin = np.full(n, np.nan)
    worst = np.full(n, -1, dtype=np.int32)
    Y = nominal.x_next[:, :, 0, :]
    live = np.nonzero(status == INVARIANT)[0]
    if live.size:
        L = live.size
        modes = nominal.modes[live]
        in_region = region_holds(plant, nominal.vertices[live], modes, v_box, tol_exit)
        best, best_at = np.zeros(L), np.full(L, -1, dtype=np.int32)
        all_hold = np.ones(L, dtype=bool)
        with np.errstate(invalid='ignore', over='ignore'):
            for f in range(normals.shape[0]):
                mn, at = None, np.zeros(L, dtype=np.int32)
                for i in range(p + 1):
                    s = np.zeros(L)
                    for c in range(p):
                        s = s + normals[f, c] * Y[live, i, c]
                    if mn is None:
                        mn = s
                    else:
                        b = iv.beats(s, mn)
                        mn, at = np.where(b, s, mn), np.where(b, i, at).astype(np.int32)
                val = (mn - offsets[f]) + slack[f, modes]
                all_hold &= val >= -thr
                b = (best_at < 0) | iv.beats(val, best)
                best = np.where(b, val, best)
                best_at = np.where(b, f * (p + 1) + at, best_at).astype(np.int32)
        margin[live], worst[live] = best, best_at
        status[live] = np.where(~in_region, MODE_REGION, np.where(all_hold, INVARIANT, EXITS))
    counts = [int((status == k).sum()) for k in range(5)]
    worst_leaf, worst_margin = -1, np.nan
    for q in np.nonzero(((status == INVARIANT) | (status == EXITS)) & ~np.isnan(margin))[0]:
        if worst_leaf < 0 or margin[q] < worst_margin:
            worst_leaf, worst_margin = int(q), float(margin[q])
    return SimpleNamespace(status=status, margin=margin, worst=worst, counts=counts,
                           worst_leaf=worst_leaf, worst_margin=worst_margin, G=G, lo=lo, hi=hi,
                           slack=slack, y=Y, vertices=nominal.vertices, modes=nominal.modes,
                           set_convex=convex, n_facets=normals.shape[0], n_generators=lo.size,
                           nominal=nominal, normals=normals, offsets=offsets)


def core(arrays, leaf_mode, plant, d_box=None, v_box=None, e_box=None, tol_exit=1e-9, tol_set=1e-9,
         tol_side=None, rows='invariant', max_fan=4096, roots=None, seeds=None):
    """``tests/core_cpu.core`` with the image of leaf l spanned by G_m, m the leaf's mode."""
    h = zc.header(arrays)
    assert h['n_test'] == 0
    p, n_leaf = h['p'], h['n_leaf']
    tol_side = float(tol_exit) if tol_side is None else float(tol_side)
    single = zc.is_single(arrays)
    roots = zc.root_vertices(arrays) if roots is None else roots
    if seeds is None:
        seeds = successors(arrays, leaf_mode, plant, d_box, v_box, e_box, roots=roots,
                           tol_exit=tol_exit, tol_set=tol_set)
    Y, G = seeds.y, seeds.G
    node = np.ascontiguousarray(arrays['node']).reshape(h['n_int'], h['node_stride'])
    ch = zc.children(arrays)
    entry = np.asarray(arrays['root_entry'])
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    box_lo, box_hi = kc.root_boxes(roots)
    status = seeds.status.astype(np.int32).copy()
    wanted = status < NO_MODE
    if rows != 'all':
        wanted &= status == INVARIANT
    wanted &= np.isfinite(Y).all(axis=(1, 2))
    rows_out = [[] for _ in range(n_leaf)]
    for l in np.nonzero(wanted)[0]:
        E = G[seeds.modes[l]] if seeds.lo.size else None
        img = kc.Image(Y[l], E, seeds.lo, seeds.hi)
        out, ok = [], True
        for r in kc.candidate_roots(img, root_rec, box_lo, box_hi, tol_side):
            ok = kc.descend(img, node, ch, entry[r], single, tol_side, out, max_fan)
            if not ok:
                break
        if ok:
            rows_out[l] = out
        else:
            status[l] = kc.UNRESOLVED
    indptr = np.zeros(n_leaf + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows_out])
    indices = np.array([t for r in rows_out for t in r], dtype=np.int32)
    level = kc.fixed_point(status != INVARIANT, indptr, indices)
    counts = [int((level < 0).sum()), int((level > 0).sum())] + \
        [int(((level == 0) & (status == s)).sum()) for s in range(1, 6)]
    return SimpleNamespace(level=level, core=level < 0, status=status,
                           counts=dict(zip(kc.COUNT_NAMES, counts)), n_sweeps=int(level.max()) + 1,
                           indptr=indptr, indices=indices, n_edges=int(indices.size), seeds=seeds,
                           vertices=seeds.vertices, y=Y, tol_side=tol_side)


# -- the cube cases the host and the device tests share ---------------------------------------------
# (a, b): |v_c| <= a, |e_c| <= b, dyadic.  With K = -I/2 on the identity plant z+ = z/2 - v + e + v',
# so a leaf whose largest vertex modulus is M has the margin 1 - (M/2 + 2 a + b).
ALL_STAY = (1. / 8, 1. / 8)
SOME_EXIT = (1. / 4, 1. / 8 + 2. ** -10)
NO_ERROR = (0., 0.)


def sym(r, n):
    """The box [-r, r]^n."""
    return (-r * np.ones(n), r * np.ones(n))


def cube(p, K=None, **kw):
    """(flat, arrays) of ``invariance_cpu.cube_law(p, K)``, K = -I/2 by default."""
    from tests import compiled_cpu
    flat = iv.cube_law(p, -0.5 * np.eye(p) if K is None else K, **kw)
    arrays, _ = compiled_cpu.compile_flat(flat)
    return flat, arrays


def largest_coordinate(V):
    """M per leaf: the largest |coordinate| of the leaf's vertices."""
    return np.abs(V).max(axis=(1, 2))


def closed_form(flat, arrays, a, b):
    """The margin of every leaf of ``cube(p)`` under |v| <= a, |e| <= b."""
    M = largest_coordinate(flat.vertices[arrays['leaf_node']])
    return 1. - (M / 2. + 2. * a + b)
