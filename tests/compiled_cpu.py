"""
Numpy mirror of the compiled explicit law (csrc/ehm_compiled.hip); test
infrastructure, host only.

    arrays, split = compile_flat(flat)      # classification and records, np.linalg.inv
    u, leaf, depth, smin = evaluate(arrays, X)

``evaluate`` walks arrays in the layout of ``CompiledLaw.arrays()`` in the device's order of
operations, so on exported arrays it is bit-equal to the device: plane tests and leaf gains one
rounding per product and per sum; containment tests (roots, test nodes, the root locator) with the
products fused into the sums, ``fma`` below being an exact float64 fused multiply-add.
"""

import numpy as np

from explicit_hybrid_mpc_amd.engine import FlatTree

EPS = 2.220446049250313e-16
LOCATE_MIN, LOCATE_STEPS, STRICT = 128, 96, 1e-9
VERSION = 1
HEADER = ('version', 'p', 'n_u', 'n_roots', 'n_int', 'n_leaf', 'n_test', 'node_stride',
          'leaf_stride', 'side_stride', 'has_nbr', 'n_source_nodes')


def node_stride(p):
    return 8 if p <= 6 else 16


def leaf_stride(p, n_u):
    return (p + n_u + n_u * p + 1) // 2 * 2


def side_stride(p):
    return (p + p * p + 1) // 2 * 2


# -- exact fused multiply-add (Boldo & Melquiond: the sum of three by rounding to odd) ---------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729. * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c), one rounding, elementwise on float64 arrays (no over- / underflow)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64),
                                  np.asarray(c, np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    z, e = _two_sum(vl, tl)
    # z rounded to odd: where inexact and the last bit is even, the neighbour on e's side
    z = np.array(z, dtype=np.float64)
    bits = z.view(np.int64)
    fix = (e != 0.) & ((bits & 1) == 0)
    up = (e > 0.) == (z > 0.)
    bits += np.where(fix, np.where(up, 1, -1), 0)
    return vh + z


# -- host compile ------------------------------------------------------------------------------
def compile_flat(flat):
    """The arrays of a FlatTree-like object (vertices, vertex_inputs, left, right,
    info['n_roots']) and, per source node, the (i, j) of a plane node (None elsewhere)."""
    V = np.asarray(flat.vertices, dtype=np.float64)
    U = np.asarray(flat.vertex_inputs, dtype=np.float64)
    left, right = np.asarray(flat.left), np.asarray(flat.right)
    n, p, n_u = V.shape[0], V.shape[2], U.shape[2]
    n_roots = int(flat.info['n_roots'])
    Minv = np.linalg.inv(np.transpose(V[:, 1:] - V[:, :1], (0, 2, 1)))
    is_leaf = left < 0
    newid = np.where(is_leaf, ~(np.cumsum(is_leaf) - 1), np.cumsum(~is_leaf) - 1).astype(np.int32)
    internal = np.nonzero(~is_leaf)[0]
    assert (left[internal] > internal).all() and (right[internal] > internal).all()
    ns, ls, ss = node_stride(p), leaf_stride(p, n_u), side_stride(p)
    side = np.zeros((n, ss))
    side[:, :p] = V[:, 0]
    side[:, p:p + p * p] = Minv.reshape(n, p * p)
    node = np.zeros((internal.size, ns))
    split = [None] * n
    tests = []
    for row, k in enumerate(internal):
        L, R = int(left[k]), int(right[k])
        dl = np.nonzero((V[L] != V[k]).any(axis=1))[0]
        dr = np.nonzero((V[R] != V[k]).any(axis=1))[0]
        if dl.size == 1 and dr.size == 1 and dl[0] != dr[0] and (V[L, dl[0]] == V[R, dr[0]]).all():
            i, j = int(dl[0]), int(dr[0])
            split[k] = (i, j)
            a = Minv[L, j - 1] if j >= 1 else -Minv[L].sum(axis=0)
            node[row, :p] = a
            node[row, p] = (1. if j == 0 else 0.) - a @ V[L, 0]
        else:
            node[row, p] = len(tests)
            tests.append(L)
        node[row, p + 1:p + 2].view(np.int32)[:] = (newid[L], newid[R])
    leaves = np.nonzero(is_leaf)[0]
    leaf_rec = np.zeros((leaves.size, ls))
    leaf_rec[:, :p] = V[leaves, 0]
    leaf_rec[:, p:p + n_u] = U[leaves, 0]
    K = np.einsum('lic,liq->lcq', U[leaves, 1:] - U[leaves, :1], Minv[leaves])
    leaf_rec[:, p + n_u:p + n_u + n_u * p] = K.reshape(leaves.size, n_u * p)
    header = np.array([VERSION, p, n_u, n_roots, internal.size, leaves.size, len(tests), ns, ls,
                       ss, 0, n], dtype=np.int64)
    arrays = {'header': header, 'node': node, 'leaf_rec': leaf_rec,
              'leaf_node': leaves.astype(np.int32),
              'test_rec': side[np.array(tests, dtype=np.int64)].reshape(len(tests), ss),
              'root_rec': side[:n_roots].copy(), 'root_entry': newid[:n_roots].copy(),
              'nbr': np.zeros((0, p + 1), dtype=np.int32)}
    return arrays, split


# -- evaluation in the device's order ----------------------------------------------------------
def _weights(rec, X, p):
    """(alpha [n, p], a0 [n]) of X[i] in the [v0 | inv(E)] record rec[i] (c_contains' sums)."""
    d = X - rec[:, :p]
    alpha = np.empty((X.shape[0], p))
    s = np.zeros(X.shape[0])
    for q in range(p):
        a = np.zeros(X.shape[0])
        for c in range(p):
            a = fma(rec[:, p + q * p + c], d[:, c], a)
        alpha[:, q] = a
        s = s + a
    return alpha, 1. - s


def _contains(rec, X, p):
    alpha, a0 = _weights(rec, X, p)
    ok = ((alpha >= -EPS) & (alpha <= 1. + EPS)).all(axis=1)
    return ok & (a0 >= -EPS) & (a0 <= 1. + EPS)


def _locate(root_rec, nbr, X, p):
    """k_compiled_locate: (root or -1, steps) per state."""
    n, R = X.shape[0], root_rec.shape[0]
    k = (np.arange(n) % R).astype(np.int64)
    found = np.full(n, -1, dtype=np.int64)
    steps = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    for _ in range(LOCATE_STEPS):
        if live.size == 0:
            break
        steps[live] += 1
        alpha, a0 = _weights(root_rec[k[live]], X[live], p)
        lo, at = a0.copy(), np.zeros(live.size, dtype=np.int64)
        for i in range(p):
            less = alpha[:, i] < lo
            lo = np.where(less, alpha[:, i], lo)
            at = np.where(less, i + 1, at)
        inside = lo > STRICT
        found[live[inside]] = k[live[inside]]
        k2 = nbr[k[live], at]
        go = ~inside & ~(lo >= -STRICT) & (k2 >= 0)
        k[live[go]] = k2[go]
        live = live[go]
    return found, steps


def _first_root(root_rec, X, p):
    """The serial spine walk: (first root 0..R-2 that contains x, else R-1; tests made).  Roots
    whose float64 weights miss [-eps, 1+eps] by more than a rigorous bound on the rounding error of
    either evaluation cannot pass the device's test; the others are tested in its arithmetic."""
    n, R = X.shape[0], root_rec.shape[0]
    root = np.full(n, R - 1, dtype=np.int64)
    tests = np.full(n, R - 1, dtype=np.int64)
    if R == 1 or n == 0:
        return root, tests
    M = root_rec[:R - 1, p:p + p * p].reshape(R - 1, p, p)
    v0 = root_rec[:R - 1, :p]
    c = np.einsum('rqc,rc->rq', M, v0)
    cb = np.einsum('rqc,rc->rq', np.abs(M), np.abs(v0))
    Mf, Af = M.reshape(-1, p), np.abs(M).reshape(-1, p)
    chunk = max(1, (1 << 22) // ((R - 1) * p))
    pairs_q, pairs_r = [], []
    for s in range(0, n, chunk):
        Xc = X[s:s + chunk]
        A = (Xc @ Mf.T).reshape(-1, R - 1, p) - c
        B = 8 * (p + 2) * EPS * ((np.abs(Xc) @ Af.T).reshape(-1, R - 1, p) + cb)
        a0 = 1. - A.sum(axis=2)
        b0 = B.sum(axis=2) + 8 * (p + 2) * EPS * (1. + np.abs(A).sum(axis=2))
        cand = ((A >= -EPS - B) & (A <= 1. + EPS + B)).all(axis=2) & (a0 >= -EPS - b0) & \
            (a0 <= 1. + EPS + b0)
        q, r = np.nonzero(cand)
        pairs_q.append(q + s)
        pairs_r.append(r)
    q, r = np.concatenate(pairs_q), np.concatenate(pairs_r)
    ok = _contains(root_rec[r], X[q], p)
    q, r = q[ok], r[ok]
    order = np.lexsort((r, q))
    q, r = q[order], r[order]
    first = np.ones(q.size, dtype=bool)
    first[1:] = q[1:] != q[:-1]
    root[q[first]] = r[first]
    tests[q[first]] = r[first] + 1
    return root, tests


def evaluate(arrays, X, locate=True):
    """(u [n, n_u], leaf [n] source node ids, depth [n], smin [n]: the smallest |s| over the plane
    nodes of the path, inf without one) of the states X in the device's order of operations."""
    h = dict(zip(HEADER, (int(v) for v in arrays['header'])))
    p, n_u, R = h['p'], h['n_u'], h['n_roots']
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
    n = X.shape[0]
    node = np.ascontiguousarray(arrays['node'], dtype=np.float64).reshape(h['n_int'],
                                                                         h['node_stride'])
    children = node[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    root = np.full(n, -1, dtype=np.int64)
    depth = np.zeros(n, dtype=np.int64)
    if h['has_nbr'] and locate:
        root, depth = _locate(root_rec, np.asarray(arrays['nbr']), X, p)
        depth = np.where(root >= 0, depth, 0)
    todo = np.nonzero(root < 0)[0]
    root[todo], depth[todo] = _first_root(root_rec, X[todo], p)
    k = np.asarray(arrays['root_entry'])[root].astype(np.int64)
    smin = np.full(n, np.inf)
    live = np.nonzero(k >= 0)[0]
    while live.size:
        rec = node[k[live]]
        depth[live] += 1
        s = np.zeros(live.size)
        for c in range(p):
            s = s + rec[:, c] * X[live, c]
        s = s + rec[:, p]
        go_left = s >= -EPS
        test = (rec[:, :p].view(np.int64) == 0).all(axis=1)
        if test.any():
            t = rec[test, p].astype(np.int64)
            go_left[test] = _contains(np.asarray(arrays['test_rec'])[t], X[live[test]], p)
        smin[live[~test]] = np.minimum(smin[live[~test]], np.abs(s[~test]))
        k[live] = np.where(go_left, children[k[live], 0], children[k[live], 1])
        live = live[k[live] >= 0]
    l = ~k
    lr = np.asarray(arrays['leaf_rec'], dtype=np.float64)[l]
    d = X - lr[:, :p]
    u = np.empty((n, n_u))
    for c in range(n_u):
        t = np.zeros(n)
        for q in range(p):
            t = t + lr[:, p + n_u + c * p + q] * d[:, q]
        u[:, c] = lr[:, p + c] + t
    return u, np.asarray(arrays['leaf_node'])[l].astype(np.int32), depth.astype(np.int32), smin


# -- a walk against exact arithmetic (tests/explicit_synth.SynthLaw) ----------------------------
def check_plane_path(law, k, ref):
    """
    Asserts that the compiled walk to leaf k is the exact walk of ref's point (``law.locate``) up to
    decisions within ``law.threshold``: the root is judged as ``SynthLaw.check_path`` judges it; at
    every node the turn is the exact sign of l_j - l_i (the split face's weight in the left child)
    or one whose exact |l_j - l_i| / D is within the left child's threshold; and the exact weights
    in k are >= -threshold(k).  Returns those weights (integers over ref.D).
    """
    from fractions import Fraction
    path = [int(k)]
    while law.parent[path[-1]] >= 0:
        path.append(int(law.parent[path[-1]]))
    path.reverse()
    r, D = path[0], ref.D
    lam = law.forest.root_weights(r, ref.Y, D)
    if r != ref.root:
        assert ref.margin <= law.threshold(ref.root), ('root', r, ref.root)
        assert Fraction(min(lam), D) >= -law.threshold(r), ('root', r, ref.root)
    for a, b in zip(path[:-1], path[1:]):
        L = int(law.left[a])
        i, j, _ = law.split[L]
        diff = lam[j] - lam[i]
        if (b == L) != (diff >= 0):
            assert Fraction(abs(diff), D) <= law.threshold(L), ('turn', a, b)
        lam = law.child_weights(lam, *law.split[b])
    assert Fraction(min(lam), D) >= -law.threshold(k), ('leaf', k, float(Fraction(min(lam), D)))
    return lam


# -- fixtures the host and the device tests share ------------------------------------------------
def two_point_tree():
    """Root [0, 1] whose children [0, 0.5] and [0.6, 1] carry different split points."""
    V = np.array([[[0.], [1.]], [[0.], [0.5]], [[0.6], [1.]]])
    U = np.array([[[0.], [1.]], [[0.], [0.5]], [[0.6], [1.]]])
    left, right = np.array([1, -1, -1], np.int32), np.array([2, -1, -1], np.int32)
    return FlatTree(V, left, right, np.zeros(3, np.int32), np.zeros((3, 2)), U,
                    np.zeros(3, np.uint8), np.zeros(3), {'n_roots': 1}, [0])


def malformed(arrays):
    """(name, arrays) of the malformed variants the validator must refuse."""
    p = int(arrays['header'][1])

    def variant(**kw):
        out = {k: np.array(v, copy=True) for k, v in arrays.items()}
        for k, fn in kw.items():
            fn(out[k])
        return out

    def child(value):
        def fn(node):
            node[0, p + 1:p + 2].view(np.int32)[0] = value
        return fn

    n_int, n_leaf = int(arrays['header'][4]), int(arrays['header'][5])

    def nan_leaf(a):
        a[0, 0] = np.nan

    def nan_plane(a):
        a[0, 0] = np.nan

    def version(hd):
        hd[0] = VERSION + 1

    def leaf_id(a):
        a[0] = int(arrays['header'][11])

    return [('child out of range', variant(node=child(n_int))),
            ('leaf child out of range', variant(node=child(~n_leaf))),
            ('child not after its parent', variant(node=child(0))),
            ('NaN leaf record', variant(leaf_rec=nan_leaf)),
            ('NaN plane', variant(node=nan_plane)),
            ('leaf id out of range', variant(leaf_node=leaf_id)),
            ('wrong version', variant(header=version))]
