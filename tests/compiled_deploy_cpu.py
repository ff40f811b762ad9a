"""
Numpy mirror of the two deployment options of the compiled law ("rooted spine" and
"flushed narrowing"; csrc/ehm_compiled.hip ehm_compiled_create_opts, csrc/ehm_compiled32.hip
k_compiled_narrow under EHM_NARROW_FLUSH); test infrastructure, host only, built on
tests/compiled_cpu.py and tests/compiled32_cpu.py.

    root = nest(law)                              # a SynthLaw in the reference's nested layout
    rooted = root_spine(nested_flat(root))        # the arrays compile(spine='roots') gives
    rooted = root_spine(arrays, last_rec, root_vertices)     # the same from a law's own arrays
    a32, counts = narrow_flush(arrays)            # to_single(flush=True) and its ``flushed``
    bound, s64 = turn_bound_flush(arrays, nodes, X)
    bound = u_bound_flush(arrays, leaves, X)

The two bounds, with u = 2^-24 and F the entries of a record the narrowing flushes (nonzero, float
zero or subnormal, so |v| < 2^-126).  A flushed entry is +0.0f: its product with a finite float is
an exact zero and adding it is exact, so the float sum is the sum over the entries outside F, each
of which passes at most the roundings ``compiled32_cpu`` counts.  Hence

``turn_bound_flush`` = turn_bound + sum_{i in F} |a_i x_i| + [b in F] |b|: the single sum is within
turn_bound of the exact sum without the flushed terms, and those terms are what is missing.

``u_bound_flush`` = u_bound + sum_{i: K_ci in F} |K_ci (x_i - v_0i)| + [u_0c in F] |u_0c|
+ (1 + (p + 4) u) sum_i |K_ci| [v_0i in F] |v_0i|: a flushed K_ci or u_0c drops its term; a flushed
v_0i makes d_i = xs_i exact, which moves the term by K_ci v_0i and raises |d_i| in u_bound's own
count by at most |v_0i| -- the factor (p + 4) u on that part.
"""

from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from explicit_hybrid_mpc_amd.explicit import flatten_tree
from explicit_hybrid_mpc_amd.tree import NodeData, Tree
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import explicit_synth as es

INJECTED = (2. ** -130, -1e-40, 2. ** -127)     # float: subnormal, subnormal, subnormal (2^-127)


def _h(arrays):
    return dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))


# -- the reference's nested layout ----------------------------------------------------------------
def nest(law):
    """A ``SynthLaw`` as the reference stores a partition: a right-leaning spine of data-less
    ``tree.Tree`` nodes with the roots, in forest order, as their left children (the last root is
    the last spine node's right child; a single root is the tree itself).  Every node with data
    carries ``synth_id``, its id in ``law``; commutations are one-element vectors [delta_idx].
    Built without recursion."""
    def make(k):
        data = NodeData(law.vertices[k].copy(), vertex_inputs=law.vertex_inputs[k].copy(),
                        commutation=(np.array([float(law.delta_idx[k])])
                                     if law.delta_idx[k] >= 0 else None))
        nd = Tree(data, top=False)
        nd.synth_id = int(k)
        return nd

    R = law.forest.n_roots
    tops = []
    for r in range(R):
        top = make(r)
        stack = [top]
        while stack:
            nd = stack.pop()
            k = nd.synth_id
            if law.left[k] >= 0:
                nd.left, nd.right = make(law.left[k]), make(law.right[k])
                stack += [nd.left, nd.right]
        tops.append(top)
    if R == 1:
        return tops[0]
    root = at = Tree(None)
    for r in range(R - 1):
        at.left = tops[r]
        at.right = tops[r + 1] if r == R - 2 else Tree(None, top=False)
        at = at.right
    return root


class NestedMpc:
    """``mpc`` of a nested synthetic law: the step-0 mode of the commutation [d] is d."""

    @staticmethod
    def step0_mode(c):
        return int(np.asarray(c).ravel()[0])


def nested_flat(root):
    """What ``ExplicitMPC`` sets a nested tree up from (``flatten_tree``), as a FlatTree-like object
    for ``compiled_cpu.compile_flat``; ``synth_id`` [n_nodes] is -1 on the spine."""
    V, U, left, right, nodes = flatten_tree(root)
    return SimpleNamespace(vertices=V, vertex_inputs=U, left=left, right=right,
                           info={'n_roots': 1},
                           synth_id=np.array([getattr(nd, 'synth_id', -1) for nd in nodes]))


# -- spine='roots' ---------------------------------------------------------------------------------
def adjacency(root_vertices):
    """nbr [R, p+1] of ehm_root_adjacency: vertices by value (-0.0 == 0.0), faces by their sorted
    vertex ids, the first owner of a face paired with every later one."""
    V = np.asarray(root_vertices, dtype=np.float64) + 0.       # -0.0 + 0.0 = +0.0
    R, p1, p = V.shape
    vid, ids = {}, np.empty((R, p1), dtype=np.int64)
    for r in range(R):
        for i in range(p1):
            ids[r, i] = vid.setdefault(V[r, i].tobytes(), len(vid))
    nbr = np.full((R, p1), -1, dtype=np.int32)
    face = {}
    for r in range(R):
        for i in range(p1):
            key = tuple(sorted(ids[r, j] for j in range(p1) if j != i))
            if key not in face:
                face[key] = (r, i)
            else:
                o = face[key]
                nbr[r, i] = o[0]
                nbr[o] = r
    return nbr


def side_record(vertices):
    """[v_0 | inv(E)] of one simplex as ``compiled_cpu.compile_flat`` computes it."""
    V = np.asarray(vertices, dtype=np.float64)[None]
    p = V.shape[2]
    Minv = np.linalg.inv(np.transpose(V[:, 1:] - V[:, :1], (0, 2, 1)))
    rec = np.zeros(cc.side_stride(p))
    rec[:p] = V[0, 0]
    rec[p:p + p * p] = Minv.reshape(p * p)
    return rec


def spine_of(arrays):
    """Internal indices of the chain s_0 = entry of the only root, s_(i+1) = right(s_i), taken
    while s_i is a test node; [] for a law with more than one root."""
    h = _h(arrays)
    p = h['p']
    if h['n_roots'] != 1 or h['n_int'] == 0:
        return []
    node = np.ascontiguousarray(arrays['node'], dtype=np.float64).reshape(h['n_int'],
                                                                         h['node_stride'])
    children = node[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)
    is_test = (node[:, :p].copy().view(np.int64) == 0).all(axis=1)
    spine, k = [], int(np.asarray(arrays['root_entry'])[0])
    while k >= 0 and is_test[k]:
        spine.append(k)
        k = int(children[k, 1])
    return spine


def root_spine(src, last_rec=None, root_vertices=None):
    """
    The arrays of ``compile(spine='roots')`` from those of ``compile()``.  ``src`` is a FlatTree-like
    object (compiled with ``compiled_cpu.compile_flat``; the last root's record and the roots'
    vertices are taken from it) or the arrays themselves; these hold the records of the spine's left
    children (test_rec) but not of the last root, so the caller gives ``last_rec`` [side_stride] and,
    from 128 roots on, ``root_vertices`` [R, p+1, p] for the adjacency.  Without a spine the arrays
    come back unchanged.
    """
    if isinstance(src, dict):
        arrays = src
    else:
        arrays = cc.compile_flat(src)[0]
    out = {k: np.array(v, copy=True) for k, v in arrays.items()}
    spine = spine_of(arrays)
    if not spine:
        return out
    h = _h(arrays)
    p, m = h['p'], len(spine)
    node = out['node'].reshape(h['n_int'], h['node_stride'])
    children = node[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)
    entries = [int(children[s, 0]) for s in spine] + [int(children[spine[-1], 1])]
    if not isinstance(src, dict):
        left, right = np.asarray(src.left), np.asarray(src.right)
        internal = np.nonzero(left >= 0)[0]
        ids = [int(left[internal[s]]) for s in spine] + [int(right[internal[spine[-1]]])]
        last_rec = side_record(src.vertices[ids[-1]])
        root_vertices = np.asarray(src.vertices)[ids]
    rows = [int(node[s, p]) for s in spine]
    root_rec = np.vstack([np.asarray(arrays['test_rec'])[rows],
                          np.asarray(last_rec, dtype=np.float64)[None]])
    keep = np.ones(h['n_int'], dtype=bool)
    keep[spine] = False
    new_int = np.cumsum(keep) - 1
    keep_t = np.ones(h['n_test'], dtype=bool)
    keep_t[rows] = False
    new_t = np.cumsum(keep_t) - 1
    remap = lambda c: np.where(c >= 0, new_int[np.maximum(c, 0)], c).astype(np.int32)
    kept = node[keep].copy()
    is_test = (kept[:, :p].copy().view(np.int64) == 0).all(axis=1)
    kept[is_test, p] = new_t[kept[is_test, p].astype(np.int64)]
    kept[:, p + 1:p + 2].view(np.int32)[:] = remap(children[keep]).reshape(-1, 2)
    R = m + 1
    has_nbr = R >= cc.LOCATE_MIN
    out['node'] = kept
    out['test_rec'] = np.asarray(arrays['test_rec'])[keep_t].copy()
    out['root_rec'] = root_rec
    out['root_entry'] = remap(np.array(entries, dtype=np.int64))
    out['nbr'] = adjacency(root_vertices) if has_nbr else np.zeros((0, p + 1), dtype=np.int32)
    hd = out['header']
    for name, value in (('n_roots', R), ('n_int', h['n_int'] - m), ('n_test', h['n_test'] - m),
                        ('has_nbr', int(has_nbr))):
        hd[cc.HEADER.index(name)] = value
    return out


# -- flush=True ------------------------------------------------------------------------------------
def flushed_masks(arrays):
    """(node [n_int, p+1], leaf [n_leaf, used]) bool: the entries the flushing narrowing sets to
    zero -- nonzero doubles whose float is zero or subnormal."""
    h = _h(arrays)
    p, used = h['p'], h['p'] + h['n_u'] + h['n_u'] * h['p']
    node = np.asarray(arrays['node'], dtype=np.float64).reshape(h['n_int'], h['node_stride'])
    leaf = np.asarray(arrays['leaf_rec'], dtype=np.float64).reshape(h['n_leaf'], h['leaf_stride'])

    def gone(a):
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            f = a.astype(np.float32)
        return (a != 0.) & (np.abs(f) < c32.FLT_MIN)

    return gone(node[:, :p + 1]), gone(leaf[:, :used])


def narrow_flush(arrays):
    """(arrays of the single law, {'a', 'b', 'leaf'} counts): ``compiled32_cpu.narrow`` with the
    values that would underflow stored as +0.0 and counted; the other refusals stand (test nodes,
    overflow, a normal that is zero after narrowing and flushing)."""
    h = _h(arrays)
    if h['n_test'] > 0:
        raise c32.NarrowError('test nodes')
    p = h['p']
    gn, gl = flushed_masks(arrays)
    work = {k: np.array(v, copy=True) for k, v in arrays.items()}
    work['node'] = work['node'].reshape(h['n_int'], h['node_stride'])
    work['leaf_rec'] = work['leaf_rec'].reshape(h['n_leaf'], h['leaf_stride'])
    work['node'][:, :p + 1][gn] = 0.
    work['leaf_rec'][:, :gl.shape[1]][gl] = 0.
    counts = {'a': int(gn[:, :p].sum()), 'b': int(gn[:, p].sum()), 'leaf': int(gl.sum())}
    return c32.narrow(work), counts


def turn_bound_flush(arrays, nodes, X):
    """turn_bound + sum_{i in F} |a_i x_i| + [b in F] |b| for the double law's records ``nodes`` and
    the states X, and s64 (``compiled32_cpu.turn_bound``)."""
    h = _h(arrays)
    p = h['p']
    bound, s64 = c32.turn_bound(arrays, nodes, X)
    rec = np.asarray(arrays['node'], dtype=np.float64).reshape(h['n_int'], h['node_stride'])[nodes]
    gone = flushed_masks(arrays)[0][nodes]
    extra = (np.abs(rec[:, :p] * X) * gone[:, :p]).sum(axis=1) + np.abs(rec[:, p]) * gone[:, p]
    return bound + extra, s64


def u_bound_flush(arrays, leaves, X):
    """u_bound + sum_{K_ci in F} |K_ci (x_i - v_0i)| + [u_0c in F] |u_0c|
    + (1 + (p + 4) 2^-24) sum_i |K_ci| [v_0i in F] |v_0i|, [n, n_u]."""
    h = _h(arrays)
    p, n_u = h['p'], h['n_u']
    lr = np.asarray(arrays['leaf_rec'], dtype=np.float64).reshape(h['n_leaf'], h['leaf_stride'])[
        leaves]
    gone = flushed_masks(arrays)[1][leaves]
    v0, u0 = lr[:, :p], lr[:, p:p + n_u]
    K = lr[:, p + n_u:p + n_u + n_u * p].reshape(-1, n_u, p)
    gv, gu = gone[:, :p], gone[:, p:p + n_u]
    gK = gone[:, p + n_u:].reshape(-1, n_u, p)
    extra = (np.abs(K * (X - v0)[:, None, :]) * gK).sum(axis=2) + np.abs(u0) * gu + \
        (1. + (p + 4) * c32.U32) * np.einsum('nci,ni->nc', np.abs(K), np.abs(v0) * gv)
    return c32.u_bound(arrays, leaves, X) + extra


def exact_input(lr, x, p, n_u, c):
    """u_0c + sum_i K_ci (x_i - v_0i) of one double leaf record in rational arithmetic."""
    return sum((Fraction(float(lr[p + n_u + c * p + i])) *
                (Fraction(float(x[i])) - Fraction(float(lr[i]))) for i in range(p)),
               Fraction(float(lr[p + c])))


# -- the injected laws the host and the device tests share -------------------------------------------
def inject(arrays, rng, n_each=4):
    """``arrays`` with the values of ``INJECTED`` written over up to ``n_each`` entries per class that
    are exactly 0 there: plane coefficients and offsets of plane nodes, used leaf entries.  Returns
    (arrays, counts {'a', 'b', 'leaf'}, (node rows, leaf rows) that were touched)."""
    h = _h(arrays)
    p, used = h['p'], h['p'] + h['n_u'] + h['n_u'] * h['p']
    out = {k: np.array(v, copy=True) for k, v in arrays.items()}
    node = out['node'].reshape(h['n_int'], h['node_stride'])
    leaf = out['leaf_rec'].reshape(h['n_leaf'], h['leaf_stride'])
    plane = (node[:, :p] != 0.).any(axis=1)
    places = {'a': np.argwhere((node[:, :p] == 0.) & plane[:, None]),
              'b': np.argwhere((node[:, p:p + 1] == 0.) & plane[:, None]) + [0, p],
              'leaf': np.argwhere(leaf[:, :used] == 0.)}
    counts, rows = {}, {'a': [], 'b': [], 'leaf': []}
    at = 0
    for name, where in places.items():
        pick = where[rng.choice(where.shape[0], min(n_each, where.shape[0]), replace=False)] \
            if where.shape[0] else where
        target = leaf if name == 'leaf' else node
        for r, c in pick:
            target[r, c] = INJECTED[at % len(INJECTED)]
            at += 1
            rows[name].append(int(r))
        counts[name] = int(pick.shape[0])
    return out, counts, (sorted(set(rows['a'] + rows['b'])), sorted(set(rows['leaf'])))


DRAWS = 8


def injected_law(p):
    """(law, arrays with the injected values, counts, touched rows, rng): the first draw whose
    host-compiled arrays narrow as they are and hold an exact zero in every class (p = 1: in the
    offsets and the leaves -- its only plane coefficient is the whole normal)."""
    # forests with zero coordinates among their vertices: p = 5 the unit cube from the origin (the
    # first 100 roots of kuhn_forest(5) lie in [-1, 0]^5 away from it), p = 1 a grid shifted by half a
    # cell with every root split (the midpoint of root 63 is 0: its plane has b = 0, its left child
    # v_0 = 0)
    forest = {1: es.KuhnForest([100], -1. + 2. ** -7, 2. ** -6),
              5: es.KuhnForest([1] * 5, 0., 1.)}.get(p) or es.kuhn_forest(p, 100)
    for draw in range(DRAWS):
        rng = np.random.default_rng([700, p, draw])
        law = es.SynthLaw(forest, p % 4 + 1, 2, rng, n_sub=100 if p == 1 else 24)
        arrays, _ = cc.compile_flat(law.flat)
        try:
            c32.narrow(arrays)
        except c32.NarrowError:
            continue
        bad, counts, rows = inject(arrays, rng)
        if min(counts['b'], counts['leaf']) > 0 and (p == 1 or counts['a'] > 0):
            return law, bad, counts, rows, rng
    raise AssertionError('%d laws in a row without an exact zero in every class' % DRAWS)


def leaves_below(arrays, nodes):
    """For every internal index in ``nodes`` the leaf indices (of the compiled arrays) reached by
    going left all the way and right all the way."""
    h = _h(arrays)
    p = h['p']
    node = np.ascontiguousarray(arrays['node'], dtype=np.float64).reshape(h['n_int'],
                                                                         h['node_stride'])
    children = node[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)
    out = []
    for k0 in nodes:
        for first in (0, 1):
            k = int(children[k0, first])
            while k >= 0:
                k = int(children[k, first])
            out.append(~k)
    return out
