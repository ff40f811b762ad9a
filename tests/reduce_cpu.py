"""
Numpy mirror of the reduction of a compiled law (csrc/ehm_reduce.hip); test
infrastructure, host only.

    out = reduce(arrays, tol, leaf_mode=None, roots=None)
    out.arrays, out.leaf_mode, out.leaf_of        # the reduced law, as CompiledLaw.reduce gives it
    out.rep, out.open, out.keep_int, out.keep_leaf, out.target, out.max_deviation
    out.cells, out.cell_status                    # the cells of the ORIGINAL leaves

``arrays`` are in the layout of ``CompiledLaw.arrays()`` in either precision.  The cells and both
maps are ``tests/certify_cpu.py``'s (the device's arithmetic and order), the difference is taken in
double, so on exported arrays every array is bit-equal to the device's.

Small builders of trees with prescribed vertex inputs on ``explicit_synth``'s Kuhn forests:

    flat = kuhn_tree(p, n_roots, n_split, rng, lambda X: X @ K.T, n_u)       # a FlatTree
    ex = explicit_of(flat)                        # ExplicitMPC over it (public API)
"""

from types import SimpleNamespace

import numpy as np

from explicit_hybrid_mpc_amd.engine import FlatTree
from oracle.geometry import split_along_longest_edge
from tests import certify_cpu as zc
from tests import explicit_synth as es


# -- the rules of csrc/ehm_reduce_host.h -------------------------------------------------------------
def is_forest(arrays, par):
    """Every internal record is the parent the table holds for both of its children, on their
    sides, and every root for its entry."""
    pn, sn, pl, sl = par
    ch = zc.children(arrays)
    for k in range(ch.shape[0]):
        for side, c in enumerate(ch[k]):
            c = int(c)
            got = (int(pn[c]), int(sn[c])) if c >= 0 else (int(pl[~c]), int(sl[~c]))
            if got != (k, side):
                return False
    for r, e in enumerate(np.asarray(arrays['root_entry'])):
        e = int(e)
        if int(pn[e] if e >= 0 else pl[~e]) != ~r:
            return False
    return True


def representatives(par, n_int):
    """int32 [n_int]: the leftmost leaf below every internal record (k_reduce_rep)."""
    pn, sn, pl, sl = par
    rep = np.full(n_int, -1, dtype=np.int32)
    for l in range(pl.size):
        up, side = int(pl[l]), int(sl[l])
        while up >= 0 and side == 0:
            rep[up] = l
            up, side = int(pn[up]), int(sn[up])
    return rep


def flags(arrays, par, rep, V, U, status, tol, leaf_mode=None):
    """(open uint8 [n_int], the largest accepted difference): k_reduce_flags, level by level --
    every leaf against the representative of each of its ancestors at its own vertices."""
    pn, sn, pl, sl = par
    open_ = np.zeros(pn.size, dtype=np.uint8)
    dev = 0.
    ok = status == zc.CELL
    cur = pl.astype(np.int64).copy()
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (U.shape[2],))
    while True:
        act = np.nonzero(cur >= 0)[0]
        if act.size == 0:
            break
        a = cur[act]
        open_[a[~ok[act]]] = 1                      # no cell: every ancestor stays
        live, al = act[ok[act]], a[ok[act]]
        if live.size:
            r = rep[al]
            if leaf_mode is not None:
                open_[al[leaf_mode[r] != leaf_mode[live]]] = 1
            Ur = zc.vertex_inputs(arrays, r, V[live], status[live])
            with np.errstate(invalid='ignore'):
                diff = np.abs(Ur - U[live])
                passed = diff <= tol
            if passed.any():
                dev = max(dev, float(diff[passed].max()))
            open_[al[~passed.all(axis=(1, 2))]] = 1
        cur[act] = pn[a]
    return open_, dev


def topmost_merged(pn, up, open_):
    top = -1
    while up >= 0:
        if not open_[up]:
            top = up
        up = int(pn[up])
    return top


def survivors(par, rep, open_):
    """(keep_int, keep_leaf, target): k_reduce_survive."""
    pn, sn, pl, sl = par
    keep_int = np.array([bool(open_[a]) and topmost_merged(pn, int(pn[a]), open_) < 0
                         for a in range(pn.size)], dtype=bool).reshape(pn.size)
    target = np.empty(pl.size, dtype=np.int32)
    for l in range(pl.size):
        top = topmost_merged(pn, int(pl[l]), open_)
        target[l] = l if top < 0 else rep[top]
    return keep_int, target == np.arange(pl.size), target


def set_children(arrays, node, pairs):
    """Writes int32 [n, 2] child pairs into the records ``node`` of a law of either precision."""
    p = zc.header(arrays)['p']
    if zc.is_single(arrays):
        node.view(np.int32)[:, p + 1:p + 3] = pairs
    else:
        node[:, p + 1:p + 2] = np.ascontiguousarray(pairs, dtype=np.int32).view(np.float64)


def reduce(arrays, tol, leaf_mode=None, roots=None):
    """The reduced law of ``arrays`` and everything on the way (module docstring)."""
    h = zc.header(arrays)
    n_int, n_leaf = h['n_int'], h['n_leaf']
    par = zc.parents(arrays)
    assert is_forest(arrays, par)
    rep = representatives(par, n_int)
    assert (rep >= 0).all()
    leaves = np.arange(n_leaf)
    V, status = zc.cells(arrays, leaves, roots, par=par)
    mode = None if leaf_mode is None else np.asarray(leaf_mode, dtype=np.int32)
    with np.errstate(over='ignore', invalid='ignore'):      # a map that overflows is a case
        U = zc.vertex_inputs(arrays, leaves, V, status)
        open_, dev = flags(arrays, par, rep, V, U, status, tol, mode)
    keep_int, keep_leaf, target = survivors(par, rep, open_)
    new_int = (np.cumsum(keep_int) - keep_int).astype(np.int32)
    new_leaf = (np.cumsum(keep_leaf) - keep_leaf).astype(np.int32)

    def renumber(c):
        c = np.asarray(c, dtype=np.int64)
        out = np.empty(c.shape, dtype=np.int32)
        neg = c < 0
        out[neg] = ~new_leaf[~c[neg]]
        ci = c[~neg]
        out[~neg] = np.where(open_[ci] != 0, new_int[ci], ~new_leaf[rep[ci]])
        return out

    ch = zc.children(arrays)
    node = np.array(np.asarray(arrays['node']).reshape(n_int, h['node_stride'])[keep_int],
                    copy=True)
    if node.shape[0]:
        set_children(arrays, node, np.stack([renumber(ch[keep_int, 0]),
                                             renumber(ch[keep_int, 1])], axis=1))
    out = {k: np.array(v, copy=True) for k, v in arrays.items()}
    out['node'] = node
    out['leaf_rec'] = np.array(np.asarray(arrays['leaf_rec']).reshape(
        n_leaf, h['leaf_stride'])[keep_leaf], copy=True)
    out['leaf_node'] = np.asarray(arrays['leaf_node'], dtype=np.int32)[keep_leaf].copy()
    out['root_entry'] = renumber(np.asarray(arrays['root_entry']))
    out['header'] = np.array(arrays['header'], dtype=np.int64, copy=True)
    out['header'][zc.cc.HEADER.index('n_int')] = int(keep_int.sum())
    out['header'][zc.cc.HEADER.index('n_leaf')] = int(keep_leaf.sum())
    return SimpleNamespace(arrays=out, leaf_mode=None if mode is None else mode[keep_leaf].copy(),
                           leaf_of=new_leaf[target].astype(np.int32), rep=rep, open=open_,
                           keep_int=keep_int, keep_leaf=keep_leaf, target=target,
                           max_deviation=dev, cells=V, cell_status=status, inputs=U, par=par)


def leaves_below(arrays):
    """Per internal record the list of the leaf records below it."""
    ch = zc.children(arrays)
    below = [None] * ch.shape[0]
    for k in range(ch.shape[0] - 1, -1, -1):
        got = []
        for c in ch[k]:
            got += below[c] if c >= 0 else [~int(c)]
        below[k] = got
    return below


# -- trees with prescribed vertex inputs --------------------------------------------------------------
def kuhn_tree(p, n_roots, n_split, rng, inputs, n_u, modes=None, max_depth=12):
    """A FlatTree over the first ``n_roots`` roots of ``explicit_synth.kuhn_forest(p)``: ``n_split``
    longest-edge bisections of random leaves (exact midpoints: every vertex stays dyadic), vertex
    inputs ``inputs(X [m, p]) -> [m, n_u]``, and per node the commutation ``modes(centroids) ->
    int [n]`` (None: all 0)."""
    forest = es.kuhn_forest(p, n_roots)
    R = forest.n_roots
    V = [forest.vertices[r] for r in range(R)]
    left, right, depth = [-1] * R, [-1] * R, [0] * R
    for _ in range(n_split):
        open_ = [k for k in range(len(V)) if left[k] < 0 and depth[k] < max_depth]
        k = open_[rng.integers(len(open_))]
        _, _, (i, j) = split_along_longest_edge(V[k])
        m = es._exact_midpoint(V[k][i], V[k][j])
        S1, S2 = V[k].copy(), V[k].copy()
        S1[i], S2[j] = m, m
        left[k], right[k] = len(V), len(V) + 1
        V += [S1, S2]
        left += [-1, -1]
        right += [-1, -1]
        depth += [depth[k] + 1] * 2
    return flat_tree(np.array(V), left, right, R, inputs, n_u, modes)


def flat_tree(V, left, right, n_roots, inputs, n_u, modes=None):
    K, p = V.shape[0], V.shape[2]
    U = np.ascontiguousarray(np.asarray(inputs(V.reshape(-1, p)), dtype=np.float64).reshape(
        K, p + 1, n_u))
    didx = np.zeros(K, np.int32) if modes is None else np.asarray(modes(V.mean(axis=1)), np.int32)
    return FlatTree(np.ascontiguousarray(V), np.array(left, np.int32), np.array(right, np.int32),
                    didx, np.zeros((K, p + 1)), U, np.zeros(K, np.uint8), np.zeros(K),
                    {'n_roots': n_roots}, list(range(int(didx.max()) + 1)))


def explicit_of(flat):
    """The device law over ``flat`` (step-0 mode of commutation d is d)."""
    from explicit_hybrid_mpc_amd import explicit
    return explicit.ExplicitMPC(flat, SimpleNamespace(
        mpc=SimpleNamespace(step0_mode=lambda d: int(d))))


def leaf_modes(flat, arrays):
    """int32 [n_leaf]: what ``ExplicitMPC.compile`` attaches for ``explicit_of(flat)``."""
    return np.asarray(flat.delta_idx, dtype=np.int32)[np.asarray(arrays['leaf_node'])]


# -- the vertex inputs the tests prescribe --------------------------------------------------------------
def integer_gain(p, n_u, rng):
    """K [n_u, p] of small integers, no row zero, and an integer offset [n_u]."""
    K = rng.integers(-3, 4, (n_u, p)).astype(np.float64)
    K[np.arange(n_u), rng.integers(0, p, n_u)] += 4.
    return K, rng.integers(-2, 3, n_u).astype(np.float64)


def affine_inputs(K, c):
    return lambda X: X @ K.T + c


def kink_frame(p, n_roots, K):
    """(centre, width): a vertex of the first ``n_roots`` Kuhn roots and a power of two such that
    the kinks K_c (x - centre) = +-width cross those roots."""
    Vr = es.kuhn_forest(p, n_roots).vertices.reshape(-1, p)
    centre = Vr[Vr.shape[0] // 2].copy()
    reach = np.abs((Vr - centre) @ K.T).max(axis=0).min()
    return centre, 2. ** np.floor(np.log2(0.25 * reach))


def clipped_inputs(K, centre, width):
    """u = clip(K (x - centre), -width, width): affine on either side of its kinks."""
    return lambda X: np.clip((X - centre) @ K.T, -width, width)


def straddles_kink(K, centre, width, V):
    """bool [n]: the cell V [n, p+1, p] has vertices strictly on both sides of a kink of some
    input of ``clipped_inputs(K, centre, width)``."""
    s = (V - centre) @ K.T                            # [n, p+1, n_u]
    out = np.zeros(V.shape[0], dtype=bool)
    for kink in (-width, width):
        out |= ((s.max(axis=1) > kink) & (s.min(axis=1) < kink)).any(axis=1)
    return out


def curved_inputs(p, n_u, scale):
    """u_c = scale (c + 1) |x|^2: no two leaves apply the same map, neighbours differ a little."""
    return lambda X: scale * (X * X).sum(axis=1)[:, None] * (1. + np.arange(n_u))


def map_at(arrays, leaf, V):
    """[n, p+1, n_u]: the map of leaf record leaf[q] at the vertices V[q], the law's arithmetic."""
    leaf = np.asarray(leaf)
    return zc.vertex_inputs(arrays, leaf, V, np.full(leaf.size, zc.CELL, dtype=np.int32))


def make_leaf_overflow(arrays, l, cell):
    """Finite values in leaf record l of a double law whose map overflows at vertex 1 of ``cell``
    [p+1, p] (u_0 = 1.79e308, K_cj = 1.7e308 sign(d_j)): the leaf's difference with itself is
    inf - inf = NaN there, so it must never merge."""
    h = zc.header(arrays)
    p, n_u = h['p'], h['n_u']
    d = cell[1] - arrays['leaf_rec'][l, :p]
    assert np.abs(d).sum() >= 0.005
    arrays['leaf_rec'][l, p:p + n_u] = 1.79e308
    arrays['leaf_rec'][l, p + n_u:p + n_u + n_u * p] = np.tile(
        np.where(d < 0., -1.7e308, 1.7e308), n_u)
