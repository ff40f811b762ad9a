"""
Numpy mirror of the leaf cells of a compiled law (csrc/ehm_certify.hip); test
infrastructure, host only.

    roots = root_vertices(arrays)                       # applied.root_cells without the device
    par = parents(arrays)                               # k_certify_roots / k_certify_parents
    V, status = cells(arrays, leaves, roots)            # k_certify_cells, the device's order
    U = vertex_inputs(arrays, leaves, V, status)        # the leaf's own map at its vertices
    out = certify(V, U, status, cost_u, n_delta, point, relaxed_point, bar_e, volume, max_tries)

``arrays`` are in the layout of ``CompiledLaw.arrays()`` in either precision.  Every sum is taken
in the device's order with one rounding per product and per sum, so on exported arrays the results
are bit-equal to ``CompiledLaw.cells``.
"""

import numpy as np

from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc

MAX_DEPTH = 256
UNREACHED = np.int32(-2 ** 31)
CELL, NO_CELL = 0, 1
CERTIFIED, UNCERTIFIED, INADMISSIBLE, NO_LAW, CERT_NO_CELL, STALLED = range(6)
FEAS_TOL = 1e-8


def header(arrays):
    return dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))


def is_single(arrays):
    return np.asarray(arrays['node']).dtype == np.float32


def root_vertices(arrays):
    """[n_roots, p+1, p]: v_i = v_0 + column i of inv(inv(E)) of the root records, the expression of
    ``applied.root_cells``."""
    p = header(arrays)['p']
    rec = np.ascontiguousarray(arrays['root_rec'], dtype=np.float64)[:, :p + p * p]
    v0 = rec[:, :p]
    E = np.linalg.inv(rec[:, p:].reshape(-1, p, p))
    V = np.concatenate([v0[:, None, :], v0[:, None, :] + np.transpose(E, (0, 2, 1))], axis=1)
    return np.ascontiguousarray(V, dtype=np.float64)


def children(arrays):
    """int32 [n_int, 2] (left, right) of a law of either precision."""
    h = header(arrays)
    p = h['p']
    node = np.ascontiguousarray(arrays['node']).reshape(h['n_int'], h['node_stride'])
    if is_single(arrays):
        return node.view(np.int32)[:, p + 1:p + 3].copy()
    return node[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)


def parents(arrays):
    """(node parent, node side, leaf parent, leaf side): the parent's index with the side the child
    hangs on, ~root for a root's entry, UNREACHED for a record nothing names.  The internal records
    first, the roots last, as the device launches them."""
    h = header(arrays)
    ch = children(arrays)
    pn = np.full(h['n_int'], UNREACHED, dtype=np.int32)
    sn = np.zeros(h['n_int'], dtype=np.uint8)
    pl = np.full(h['n_leaf'], UNREACHED, dtype=np.int32)
    sl = np.zeros(h['n_leaf'], dtype=np.uint8)
    k = np.arange(h['n_int'], dtype=np.int32)
    for side in (0, 1):
        c = ch[:, side]
        pn[c[c >= 0]], sn[c[c >= 0]] = k[c >= 0], side
        pl[~c[c < 0]], sl[~c[c < 0]] = k[c < 0], side
    entry = np.asarray(arrays['root_entry'], dtype=np.int32)
    r = np.arange(entry.size, dtype=np.int32)
    pn[entry[entry >= 0]] = ~r[entry >= 0]
    pl[~entry[entry < 0]] = ~r[entry < 0]
    return pn, sn, pl, sl


def walk_up(par, leaf, max_depth=MAX_DEPTH):
    """(root, turns root first) of one leaf, or None: unreached, or deeper than max_depth."""
    pn, sn, pl, sl = par
    up, side = int(pl[leaf]), int(sl[leaf])
    turns = []
    while up >= 0:
        if len(turns) >= max_depth:
            return None
        turns.append(side)
        up, side = int(pn[up]), int(sn[up])
    if up == int(UNREACHED):
        return None
    return ~up, turns[::-1]


def plane_values(rec, V, p):
    """s_i = ((0 + a_0 v_i0) + .. + a_(p-1) v_i(p-1)) + b in double; float coefficients widened."""
    a = np.asarray(rec[:p + 1], dtype=np.float64)
    s = np.zeros(p + 1)
    for c in range(p):
        s = s + a[c] * V[:, c]
    return s + a[p]


def cells(arrays, leaves=None, roots=None, max_depth=MAX_DEPTH, par=None, trace=None,
          magnitude=None):
    """(vertices [n, p+1, p], status [n]) of the leaf records ``leaves`` (None: all), walked down
    from ``roots`` (None: ``root_vertices``).  ``trace`` (a list) receives the plane values of
    every node visited, ``magnitude`` (float64 [n]) per leaf the largest sum |a_0 v_i0| + .. +
    |a_(p-1) v_i(p-1)| + |b| over the vertices and planes of its path: what a relative change of
    the coefficients is multiplied by."""
    h = header(arrays)
    p = h['p']
    node = np.ascontiguousarray(arrays['node']).reshape(h['n_int'], h['node_stride'])
    ch = children(arrays)
    entry = np.asarray(arrays['root_entry'])
    roots = root_vertices(arrays) if roots is None else roots
    par = parents(arrays) if par is None else par
    leaves = np.arange(h['n_leaf']) if leaves is None else np.asarray(leaves)
    out = np.full((leaves.size, p + 1, p), np.nan)
    status = np.full(leaves.size, NO_CELL, dtype=np.int32)
    for q, l in enumerate(leaves):
        path = walk_up(par, int(l), max_depth)
        if path is None:
            continue
        root, turns = path
        V = roots[root].copy()
        k = int(entry[root])
        ok = True
        for turn in turns:
            if k < 0:
                ok = False
                break
            s = plane_values(node[k], V, p)
            if trace is not None:
                trace.append(s)
            if magnitude is not None:
                a = np.abs(np.asarray(node[k][:p + 1], dtype=np.float64))
                magnitude[q] = max(magnitude[q], float((np.abs(V) @ a[:p] + a[p]).max()))
            pos, neg = np.nonzero(s > 0.5)[0], np.nonzero(s < -0.5)[0]
            if pos.size != 1 or neg.size != 1:
                ok = False
                break
            mid = (V[neg[0]] + V[pos[0]]) / 2.
            V[pos[0] if turn else neg[0]] = mid
            k = int(ch[k, turn])
        if ok and k == ~int(l):
            out[q], status[q] = V, CELL
    return out, status


def vertex_inputs(arrays, leaves, V, status):
    """[n, p+1, n_u]: the map of leaf record leaves[q] at every vertex of V[q] in the law's own
    arithmetic (NaN where status is NO_CELL): a double law as ``compiled_cpu.evaluate`` sums it, a
    single law through ``compiled32_cpu.walk32_from`` entered at the leaf itself."""
    h = header(arrays)
    p, n_u = h['p'], h['n_u']
    leaves = np.asarray(leaves)
    n = leaves.size
    out = np.full((n, p + 1, n_u), np.nan)
    live = np.nonzero(status == CELL)[0]
    if live.size == 0:
        return out
    X = V[live].reshape(-1, p)
    l = np.repeat(leaves[live], p + 1)
    if is_single(arrays):
        entered = dict(arrays, root_entry=(~l).astype(np.int32))
        _, u, _ = c32.walk32_from(entered, c32._header(arrays), np.arange(l.size), X)
    else:
        lr = np.ascontiguousarray(arrays['leaf_rec'], dtype=np.float64).reshape(
            h['n_leaf'], h['leaf_stride'])[l]
        d = X - lr[:, :p]
        u = np.empty((l.size, n_u))
        for c in range(n_u):
            t = np.zeros(l.size)
            for q in range(p):
                t = t + lr[:, p + n_u + c * p + q] * d[:, q]
            u[:, c] = lr[:, p + c] + t
    out[live] = u.reshape(live.size, p + 1, n_u)
    return out


def narrow_flushed(arrays):
    """``compiled32_cpu.narrow`` of a double law's arrays with every value below the normal range of
    a float set to zero first: the arrays of ``to_single(flush=True)``."""
    h = header(arrays)
    p, used = h['p'], h['p'] + h['n_u'] + h['n_u'] * h['p']
    out = {k: np.array(v, copy=True) for k, v in arrays.items()}
    for name, cols in (('node', p + 1), ('leaf_rec', used)):
        part = out[name][:, :cols]
        part[np.abs(part) < c32.FLT_MIN] = 0.
    return c32.narrow(out)


def chain_tree(p, depth):
    """A FlatTree over the standard simplex (0, e_1 .. e_p) whose edge (0, e_1) is bisected
    ``depth`` times, always in the child at the origin: every vertex is exact, the left child of
    level k is a leaf k levels below the root."""
    from explicit_hybrid_mpc_amd.engine import FlatTree
    root = np.concatenate([np.zeros((1, p)), np.eye(p)])
    V, left, right = [root], [-1], [-1]
    k = 0
    for _ in range(depth):
        S1, S2 = V[k].copy(), V[k].copy()
        S1[0] = S2[1] = (V[k][0] + V[k][1]) / 2.
        left[k], right[k] = len(V), len(V) + 1
        V += [S1, S2]
        left += [-1, -1]
        right += [-1, -1]
        k = right[k]
    K = len(V)
    V = np.array(V)
    U = V.sum(axis=2, keepdims=True) + 1.
    return FlatTree(V, np.array(left, np.int32), np.array(right, np.int32), np.zeros(K, np.int32),
                    np.zeros((K, p + 1)), U, np.zeros(K, np.uint8), np.zeros(K), {'n_roots': 1},
                    [0])


# -- the certificate (ehm_compiled_certify) ---------------------------------------------------------
def pack(V, U, status, cost_u):
    """k_certify_pack: (theta' [n, p+1, p+n_u], constant [n, p+1], no_law [n]); rows of a leaf
    without a cell are zero, an input that is not finite enters as 0 and flags the leaf."""
    has = (status == CELL)[:, None, None]
    Vz = np.where(has, V, 0.)
    Uz = np.where(has, U, 0.)
    bad = ~np.isfinite(Uz)
    Uz = np.where(bad, 0., Uz)
    k = np.zeros(Uz.shape[:2])
    for j in range(Uz.shape[2]):
        k = k + cost_u[j] * Uz[:, :, j]
    return np.concatenate([Vz, Uz], axis=2), k, bad.any(axis=(1, 2)).astype(np.int32)


def candidates(point, theta, konst, todo, n_delta):
    """The candidates of the leaves ``todo`` on one problem: {leaf: [(d, W [p+1], aside)]} by d
    ascending.  ``point(theta rows, slots, feas)`` is ``GpuProblem.point_idx``: (J or tau, u0,
    status)."""
    out = {int(q): [] for q in todo}
    if len(todo) == 0:
        return out
    nv, pp = theta.shape[1], theta.shape[2]
    rows = np.repeat(theta[todo].reshape(-1, pp), n_delta, axis=0)
    slots = np.tile(np.arange(n_delta, dtype=np.int32), len(todo) * nv)
    tau = point(rows, slots, True)[0].reshape(len(todo), nv, n_delta)
    feasible = (tau <= FEAS_TOL).all(axis=1)
    a, d = np.nonzero(feasible)
    if a.size == 0:
        return out
    rows = theta[np.asarray(todo)[a]].reshape(-1, pp)
    J, _, st = point(rows, np.repeat(d.astype(np.int32), nv), False)
    W = J.reshape(-1, nv) + konst[np.asarray(todo)[a]]
    aside = (st.reshape(-1, nv) != 0).any(axis=1)
    for i in range(a.size):
        out[int(todo[a[i]])].append((int(d[i]), W[i], bool(aside[i])))
    return out


def candidate_order(cands):
    """Positions of the candidates that are tried, by ((0 + W_0) + ..) + W_p ascending, the lowest
    commutation first on ties, NaN sums last (insertion sort, as the device's host code)."""
    live = [i for i, c in enumerate(cands) if not c[2]]
    keys = []
    for i in live:
        k = 0.
        for w in cands[i][1]:
            k = k + w
        keys.append(k)
    order = []
    for a in range(len(live)):
        at = len(order)
        while at > 0 and (keys[a] < keys[order[at - 1]] or
                          (keys[order[at - 1]] != keys[order[at - 1]] and keys[a] == keys[a])):
            at -= 1
        order.insert(at, a)
    return [live[a] for a in order]


def status_of(has_cell, no_law, n_cand, n_aside, closed):
    if not has_cell:
        return CERT_NO_CELL
    if no_law:
        return NO_LAW
    if closed:
        return CERTIFIED
    if n_cand == 0:
        return INADMISSIBLE
    if n_aside > 0:
        return STALLED
    return UNCERTIFIED


def certify(V, U, cell_status, cost_u, n_delta, point, relaxed_point, bar_e, volume, max_tries):
    """
    The per-leaf arrays of ``ehm_compiled_certify`` from the cells, the vertex inputs and the
    batched oracles given as callables: ``point`` / ``relaxed_point`` (None: no relaxed problem)
    as ``GpuProblem.point_idx`` of the applied problems, ``bar_e(R, Vbar)`` -> (closed, tbest) as
    ``GpuProblem.bar_e_batch`` of the oracle, ``volume(R)`` as ``engine.volume_batch``.  Returns
    a dict of status, delta_idx, tbest, tries, relaxed, n_candidates, volume, W and the worst
    uncertified leaf (position, tbest) or None.
    """
    n, nv = V.shape[0], V.shape[1]
    theta, konst, no_law = pack(V, U, cell_status, cost_u)
    todo = np.nonzero((cell_status == CELL) & (no_law == 0))[0]
    cand = candidates(point, theta, konst, todo, n_delta)
    relaxed = np.zeros(n, dtype=np.int32)
    if relaxed_point is not None:
        again = np.array([q for q in todo if not cand[int(q)]], dtype=np.int64)
        for q, found in candidates(relaxed_point, theta, konst, again, n_delta).items():
            if found:
                cand[q] = found
                relaxed[q] = 1
    order = {q: candidate_order(c) for q, c in cand.items()}
    tries = np.zeros(n, dtype=np.int32)
    tbest = np.full(n, np.nan)
    delta_idx = np.full(n, -1, dtype=np.int32)
    W = np.full((n, nv), np.nan)
    open_ = [q for q in order if order[q]]
    t = 0
    while open_ and (max_tries == 0 or t < max_tries):
        Vb = np.array([cand[q][order[q][t]][1] for q in open_])
        closed, tb = bar_e(V[open_], Vb)
        nxt = []
        for a, q in enumerate(open_):
            tries[q], tbest[q], W[q] = t + 1, tb[a], Vb[a]
            if closed[a]:
                delta_idx[q] = cand[q][order[q][t]][0]
            elif t + 1 < len(order[q]):
                nxt.append(q)
        open_, t = nxt, t + 1
    vol = np.full(n, np.nan)
    has = np.nonzero(cell_status == CELL)[0]
    if has.size:
        vol[has] = volume(V[has])
    n_cand = np.array([len(cand.get(q, [])) for q in range(n)], dtype=np.int32)
    n_aside = np.array([len(cand.get(q, [])) - len(order.get(q, [])) for q in range(n)])
    status = np.array([status_of(cell_status[q] == CELL, no_law[q], n_cand[q], n_aside[q],
                                 delta_idx[q] >= 0) for q in range(n)], dtype=np.int32)
    worst = None
    for q in np.nonzero((status == UNCERTIFIED) & ~np.isnan(tbest))[0]:
        if worst is None or tbest[q] > worst[1]:
            worst = (int(q), float(tbest[q]))
    certified_volume = 0.
    for q in np.nonzero(status == CERTIFIED)[0]:
        certified_volume = certified_volume + vol[q]
    return dict(status=status, delta_idx=delta_idx, tbest=tbest, tries=tries, relaxed=relaxed,
                n_candidates=n_cand, volume=vol, W=W, worst=worst,
                certified_volume=certified_volume)
