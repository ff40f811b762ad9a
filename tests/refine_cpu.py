"""
Numpy mirror of the refinement of a compiled law (csrc/ehm_refine.hip, csrc/ehm_refine_host.h,
DESIGN.md 3.8n); test infrastructure, host only.

    out = refine(arrays, levels=1, leaves=None, max_diameter=None, max_spread=None, leaf_mode=None)
    out.arrays, out.leaf_mode, out.origin, out.stop      # as CompiledLaw.refine gives them
    out.passes, out.n_split, out.max_plane_residual, out.stops
    out.trace                                            # per pass: (leaf ids split, (i, j), planes)

``arrays`` are in the layout of ``CompiledLaw.arrays()`` in either precision.  The cells and the
leaf maps are ``tests/certify_cpu.py``'s, the longest edge, the solve, the rounding and the
acceptance test restate ``ehm_refine_host.h`` operation for operation (numpy rounds every product
and every sum once), so on exported arrays every array is bit-equal to the device's.
"""

from types import SimpleNamespace

import numpy as np

from tests import certify_cpu as zc
from tests import compiled_cpu as cc
from tests import compiled32_cpu as c32
from tests import reduce_cpu as rc

MAX_LEVELS = 16
PENDING, UNSELECTED, SATISFIED, LEVELS, NO_CELL, UNSEPARATED, TOO_DEEP = -1, 0, 1, 2, 3, 4, 5
STOPS = ('unselected', 'satisfied', 'levels', 'no_cell', 'unseparated', 'too_deep')


def longest_edge(V):
    """(i, j, length) per cell of V [n, p+1, p]: sqrt of the fma chain of the squared differences
    from 0, the first maximal edge in itertools.combinations order (longest_edge_of)."""
    n, p1, p = V.shape
    best = np.full(n, -1.)
    bi, bj = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(p1):
            for j in range(i + 1, p1):
                s = np.zeros(n)
                for k in range(p):
                    df = V[:, i, k] - V[:, j, k]
                    s = cc.fma(df, df, s)
                length = np.sqrt(s)
                better = length > best
                best = np.where(better, length, best)
                bi, bj = np.where(better, i, bi), np.where(better, j, bj)
    return bi, bj, best


def solve_plane(V, i, j):
    """(a [n, p], b [n]): solve_plane of ehm_refine_host.h for the cells V [n, p+1, p] and their
    edges (i [n], j [n]), in its operation order."""
    n, p1, p = V.shape
    idx = np.arange(n)
    vi = V[idx, i]
    k_of = np.arange(p)[None, :] + (np.arange(p)[None, :] >= i[:, None])
    M = V[idx[:, None], k_of] - vi[:, None, :]
    t = np.where(k_of == j[:, None], 2., 1.)
    a = np.zeros((n, p))
    with np.errstate(all='ignore'):
        for k in range(p):
            piv = k + np.argmax(np.abs(M[:, k:, k]), axis=1)        # the first largest
            Mk, Mp, tk, tp = M[idx, k].copy(), M[idx, piv].copy(), t[idx, k].copy(), t[idx, piv].copy()
            M[idx, k], t[idx, k] = Mp, tp
            M[idx, piv], t[idx, piv] = Mk, tk                      # piv == k: Mp is Mk
            for r in range(k + 1, p):
                f = M[:, r, k] / M[:, k, k]
                for c in range(k + 1, p):
                    M[:, r, c] = M[:, r, c] - f * M[:, k, c]
                t[:, r] = t[:, r] - f * t[:, k]
        for k in range(p - 1, -1, -1):
            s = t[:, k].copy()
            for c in range(k + 1, p):
                s = s - M[:, k, c] * a[:, c]
            a[:, k] = s / M[:, k, k]
        d = np.zeros(n)
        for c in range(p):
            d = d + a[:, c] * vi[:, c]
        b = -1. - d
    return a, b


def store_plane(a, b, single):
    """(rec [n, p+1] in the law's scalar, storable [n]): store_plane."""
    with np.errstate(over='ignore', invalid='ignore'):
        rec = np.concatenate([a, b[:, None]], axis=1).astype(np.float32 if single else np.float64)
    ok = np.isfinite(rec)
    if single:
        ok &= (rec == 0.) | (np.abs(rec) >= np.float32(c32.FLT_MIN))
    return rec, ok.all(axis=1)


def plane_at_vertices(rec, V):
    """s [n, p+1]: the stored planes rec [n, p+1], widened, at the vertices of V, as leaf_cell sums."""
    p = V.shape[2]
    w = rec.astype(np.float64)
    s = np.zeros(V.shape[:2])
    with np.errstate(all='ignore'):
        for c in range(p):
            s = s + w[:, c, None] * V[:, :, c]
        return s + w[:, p, None]


def accept_plane(rec, V, i, j):
    """(accepted [n], residual [n]): accept_plane."""
    s = plane_at_vertices(rec, V)
    n = V.shape[0]
    idx = np.arange(n)
    with np.errstate(invalid='ignore'):
        pos, neg = s > 0.5, s < -0.5
        ok = (pos.sum(axis=1) == 1) & (neg.sum(axis=1) == 1) & pos[idx, j] & neg[idx, i]
        target = np.zeros(s.shape)
        target[idx, j], target[idx, i] = 1., -1.
        off = np.abs(s - target)
        residual = np.where(np.isnan(off), 0., off).max(axis=1)     # a NaN is never the larger
    return ok, residual


def selection(n_leaf, levels, leaves):
    """(levels int32 [n_leaf], selected bool [n_leaf]) as ``compiled.refine_selection``."""
    lv = np.ascontiguousarray(np.broadcast_to(np.asarray(levels), (n_leaf,)), dtype=np.int32)
    if leaves is None:
        return lv, np.ones(n_leaf, dtype=bool)
    sel = np.asarray(leaves)
    if sel.dtype == np.bool_:
        return lv, sel.copy()
    mask = np.zeros(n_leaf, dtype=bool)
    mask[sel] = True
    return lv, mask


def worst_case(levels, selected):
    return int((1 << levels.astype(np.int64))[selected].sum() + (~selected).sum())


def plan(arrays, par, rem, stop, roots, max_diameter, max_spread):
    """One k_refine_plan over the leaves that are PENDING: writes their stop codes and returns
    (ids of the leaves to split, (i, j) of their edges, their stored planes, the largest residual)."""
    single = zc.is_single(arrays)
    pend = np.nonzero(stop == PENDING)[0]
    none = (pend[:0], (pend[:0], pend[:0]), None, 0.)
    if pend.size == 0:
        return none
    V, st = zc.cells(arrays, pend, roots, par=par)
    stop[pend[st != zc.CELL]] = NO_CELL
    live = st == zc.CELL
    pend, V = pend[live], V[live]
    if pend.size == 0:
        return none
    i, j, length = longest_edge(V)
    want = rem[pend] > 0
    code = np.full(pend.size, SATISFIED, dtype=np.int8)
    if max_diameter is not None or max_spread is not None:
        over = np.zeros(pend.size, dtype=bool)
        with np.errstate(all='ignore'):
            if max_diameter is not None:
                over |= length > max_diameter
            if max_spread is not None:
                U = zc.vertex_inputs(arrays, pend, V, np.full(pend.size, zc.CELL, dtype=np.int32))
                spread = U.max(axis=1) - U.min(axis=1)              # NaN if any input is
                over |= (spread > np.broadcast_to(max_spread, (U.shape[2],))).any(axis=1)
        code[over] = LEVELS
        want &= over
    depth = np.array([len(zc.walk_up(par, int(l))[1]) for l in pend])
    deep = want & (depth >= zc.MAX_DEPTH)
    code[deep] = TOO_DEEP
    solve = want & ~deep
    a, b = solve_plane(V[solve], i[solve], j[solve])
    rec, storable = store_plane(a, b, single)
    ok, residual = accept_plane(rec, V[solve], i[solve], j[solve])
    ok &= storable
    at = np.nonzero(solve)[0]
    code[at[~ok]] = UNSEPARATED
    code[at[ok]] = PENDING
    stop[pend] = code
    res = float(residual[ok].max()) if ok.any() else 0.
    return pend[at[ok]], (i[solve][ok], j[solve][ok]), rec[ok], res


def rewrite(arrays, par, ids, planes, leaf_mode, rem, stop, origin):
    """k_refine_rewrite: the arrays after the leaves ``ids`` (ascending) are split by ``planes``."""
    h = zc.header(arrays)
    p, n_int, n_leaf = h['p'], h['n_int'], h['n_leaf']
    pn, sn, pl, sl = par
    m = ids.size
    node = np.asarray(arrays['node']).reshape(n_int, h['node_stride'])
    new = np.zeros((m, h['node_stride']), dtype=node.dtype)
    new[:, :p + 1] = planes
    twins = n_leaf + np.arange(m, dtype=np.int32)
    rc.set_children(arrays, new, np.stack([~ids.astype(np.int32), ~twins], axis=1))
    node = np.concatenate([node, new], axis=0)
    ch = zc.children(dict(arrays, node=node, header=_with(arrays, n_int + m, n_leaf + m)))
    entry = np.array(arrays['root_entry'], dtype=np.int32, copy=True)
    for q, l in enumerate(ids):
        up = int(pl[l])
        assert up != int(zc.UNREACHED)
        if up >= 0:
            assert ch[up, int(sl[l])] == ~int(l)
            ch[up, int(sl[l])] = n_int + q
        else:
            assert entry[~up] == ~int(l)
            entry[~up] = n_int + q
    rc.set_children(arrays, node, ch)
    out = {k: np.array(v, copy=True) for k, v in arrays.items()}
    out['node'] = node
    leaf_rec = np.asarray(arrays['leaf_rec']).reshape(n_leaf, h['leaf_stride'])
    out['leaf_rec'] = np.concatenate([leaf_rec, leaf_rec[ids]], axis=0)
    leaf_node = np.asarray(arrays['leaf_node'], dtype=np.int32)
    out['leaf_node'] = np.concatenate([leaf_node, leaf_node[ids]])
    out['root_entry'] = entry
    out['header'] = _with(arrays, n_int + m, n_leaf + m)
    rem = rem.copy()
    rem[ids] -= 1
    grow = lambda a: np.concatenate([a, a[ids]])
    return out, None if leaf_mode is None else grow(leaf_mode), grow(rem), grow(stop), grow(origin)


def _with(arrays, n_int, n_leaf):
    header = np.array(arrays['header'], dtype=np.int64, copy=True)
    header[cc.HEADER.index('n_int')] = n_int
    header[cc.HEADER.index('n_leaf')] = n_leaf
    # leaves of a refined law share source nodes: the node count never falls below the leaves
    src = cc.HEADER.index('n_source_nodes')
    header[src] = max(int(header[src]), n_leaf)
    return header


def refine(arrays, levels=1, leaves=None, max_diameter=None, max_spread=None, leaf_mode=None,
           roots=None):
    """The refined law of ``arrays`` and everything on the way (module docstring)."""
    h = zc.header(arrays)
    rem, selected = selection(h['n_leaf'], levels, leaves)
    rem = rem.copy()
    stop = np.where(selected, PENDING, UNSELECTED).astype(np.int8)
    origin = np.arange(h['n_leaf'], dtype=np.int32)
    mode = None if leaf_mode is None else np.asarray(leaf_mode, dtype=np.int32).copy()
    roots = zc.root_vertices(arrays) if roots is None else roots
    cur = {k: np.array(v, copy=True) for k, v in arrays.items()}
    passes = n_split = 0
    res = 0.
    trace = []
    while True:
        par = zc.parents(cur)
        ids, ij, planes, r = plan(cur, par, rem, stop, roots, max_diameter, max_spread)
        res = max(res, r)
        if ids.size == 0:
            break
        trace.append((ids, ij, planes, par))
        cur, mode, rem, stop, origin = rewrite(cur, par, ids, planes, mode, rem, stop, origin)
        passes += 1
        n_split += int(ids.size)
    assert (stop >= 0).all()
    return SimpleNamespace(arrays=cur, leaf_mode=mode, origin=origin, stop=stop, passes=passes,
                           n_split=n_split, max_plane_residual=res, trace=trace,
                           stops=dict(zip(STOPS, np.bincount(stop, minlength=len(STOPS)).tolist())))


def split_cells(V):
    """(S_1, S_2) of the cells V [n, p+1, p]: the partitioner's bisection along the first longest
    edge, the midpoint (v_i + v_j) / 2 in place of v_i in S_1 and of v_j in S_2."""
    i, j, _ = longest_edge(V)
    idx = np.arange(V.shape[0])
    mid = (V[idx, i] + V[idx, j]) / 2.
    S1, S2 = V.copy(), V.copy()
    S1[idx, i], S2[idx, j] = mid, mid
    return S1, S2


def nan_law():
    """The arrays of a one-leaf double law on the cell (0, 0), (4, 0), (4, 4) whose finite record
    (K = [1.7e308, -1.7e308]) gives inf + -inf = NaN at the third vertex and +inf at the second: its
    spread is NaN, so no ``max_spread`` may split it."""
    from explicit_hybrid_mpc_amd.engine import FlatTree
    V = np.array([[[0., 0.], [4., 0.], [4., 4.]]])
    flat = FlatTree(V, np.array([-1], np.int32), np.array([-1], np.int32), np.zeros(1, np.int32),
                    np.zeros((1, 3)), np.zeros((1, 3, 1)), np.zeros(1, np.uint8), np.zeros(1),
                    {'n_roots': 1}, [0])
    arrays, _ = cc.compile_flat(flat)
    arrays['leaf_rec'][0, :5] = [0., 0., 0., 1.7e308, -1.7e308]
    return arrays
