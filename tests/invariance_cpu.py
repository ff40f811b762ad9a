"""
Numpy mirror of the one-step successors of a compiled law's leaves (csrc/ehm_invariance.hip,
DESIGN.md 3.8h); test infrastructure, host only.

    out = successors(arrays, leaf_mode, plant, leaves=None, roots=None, d_box=None, tol_exit=1e-9)
    out.status, out.margin, out.worst, out.max_violation        # per leaf
    out.x_next, out.succ_root, out.succ_leaf                    # per (leaf, vertex, corner)
    out.counts, out.worst_leaf, out.worst_margin                # the summary
    out.vertices, out.inputs                                    # the cells, as certify_cpu gives them

``arrays`` are in the layout of ``CompiledLaw.arrays()`` in either precision.  The cells and the
leaf's map are ``tests/certify_cpu.py``'s, the plant step, the region test and the violation
``tests/explicit_synth.py``'s, the root choice and the walk ``tests/compiled_rollout_cpu.py``'s, so on
exported arrays every array is bit-equal to the device's.
"""

from types import SimpleNamespace

import numpy as np

from tests import certify_cpu as zc
from tests import compiled_rollout_cpu as cr
from tests import explicit_synth as es

INVARIANT, EXITS, MODE_REGION, NO_MODE, NO_CELL = range(5)
cc = zc.cc


def corners(d_box, n_d):
    """[2^n_d, n_d]: corner j takes hi[b] where bit b of j is set, else lo[b]."""
    lo, hi = (np.asarray(a, dtype=np.float64).reshape(n_d) for a in d_box)
    j = np.arange(1 << n_d)[:, None]
    return np.where((j >> np.arange(n_d)[None, :]) & 1, hi[None, :], lo[None, :])


def beats(a, b):
    """a replaces b as the smaller margin: the smaller number, a NaN before any number."""
    with np.errstate(invalid='ignore'):
        return (a < b) | (np.isnan(a) & ~np.isnan(b))


def leaf_roots(arrays, leaves, par=None):
    par = zc.parents(arrays) if par is None else par
    out = np.full(len(leaves), -1, dtype=np.int64)
    for q, l in enumerate(leaves):
        path = zc.walk_up(par, int(l))
        if path is not None:
            out[q] = path[0]
    return out


def locate(arrays, Z, start):
    """(root, alpha, a0) of the states Z as one rollout step finds them, the visibility walk
    started at the roots ``start``."""
    h = zc.header(arrays)
    p = h['p']
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    r = np.full(Z.shape[0], -1, dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        if h['has_nbr']:
            r = cr.locate_warm(root_rec, np.asarray(arrays['nbr']), Z, p, start)
        todo = np.nonzero(r < 0)[0]
        r[todo] = cc._first_root(root_rec, Z[todo], p)[0]
        alpha, a0 = cc._weights(root_rec[r], Z, p)
    return r, alpha, a0


def walk(arrays, root, Z):
    """The leaf record the law's walk from ``root`` ends in, in the law's own arithmetic."""
    if zc.is_single(arrays):
        return zc.c32.walk32_from(arrays, zc.c32._header(arrays), root, Z)[0]
    return cr.walk_from(arrays, zc.header(arrays), root, Z)[0]


def successors(arrays, leaf_mode, plant, leaves=None, roots=None, d_box=None, tol_exit=1e-9):
    h = zc.header(arrays)
    assert h['n_test'] == 0
    p, n_u, n_leaf = h['p'], h['n_u'], h['n_leaf']
    leaves = np.arange(n_leaf) if leaves is None else np.asarray(leaves)
    n = leaves.size
    par = zc.parents(arrays)
    V, cell = zc.cells(arrays, leaves, roots, par=par)
    with np.errstate(over='ignore', invalid='ignore'):
        U = zc.vertex_inputs(arrays, leaves, V, cell)
    modes = cr.plant_modes(leaf_mode, plant, n_leaf)[leaves]
    n_d = 0 if d_box is None else plant.n_d
    n_c = 1 << n_d
    nv = p + 1
    status = np.full(n, INVARIANT, dtype=np.int32)
    no_mode = (modes < 0) | (modes >= plant.n_modes)
    status[no_mode] = NO_MODE
    status[cell != zc.CELL] = NO_CELL
    margin = np.full(n, np.nan)
    worst = np.full(n, -1, dtype=np.int32)
    maxv = np.full(n, np.nan)
    x_next = np.full((n, nv, n_c, p), np.nan)
    succ_root = np.full((n, nv, n_c), -1, dtype=np.int32)
    succ_leaf = np.full((n, nv, n_c), -1, dtype=np.int32)
    live = np.nonzero(status == INVARIANT)[0]
    if live.size:
        L = live.size
        Xf = V[live].reshape(L * nv, p)
        mf = np.repeat(modes[live], nv)
        in_region = es.in_region(plant, Xf, mf, tol_exit).reshape(L, nv).all(axis=1)
        Xp = np.repeat(Xf, n_c, axis=0)
        Up = np.repeat(U[live].reshape(L * nv, n_u), n_c, axis=0)
        mp = np.repeat(mf, n_c)
        D = np.tile(corners(d_box, n_d), (L * nv, 1)) if n_d else None
        with np.errstate(over='ignore', invalid='ignore'):
            Z = es.nominal_step(plant, Xp, Up, mp, D)
        start = np.repeat(leaf_roots(arrays, leaves[live], par), nv * n_c)
        r, alpha, a0 = locate(arrays, Z, start)
        with np.errstate(invalid='ignore'):
            inside = (a0 >= -tol_exit) & (alpha >= -tol_exit).all(axis=1)
        mg = a0.copy()
        for c in range(p):
            mg = np.where(beats(alpha[:, c], mg), alpha[:, c], mg)
        mg = mg.reshape(L, nv * n_c)
        best, at = mg[:, 0].copy(), np.zeros(L, dtype=np.int32)
        for e in range(1, nv * n_c):
            b = beats(mg[:, e], best)
            best, at = np.where(b, mg[:, e], best), np.where(b, e, at).astype(np.int32)
        margin[live], worst[live] = best, at
        with np.errstate(invalid='ignore', over='ignore'):
            viol = es.violation(plant, Z).reshape(L, nv * n_c)
        mv = np.full(L, -np.inf)
        for e in range(nv * n_c):
            mv = np.fmax(mv, viol[:, e])
        maxv[live] = mv
        x_next[live] = Z.reshape(L, nv, n_c, p)
        sr = np.where(inside, r, -1).astype(np.int32)
        sl = np.full(Z.shape[0], -1, dtype=np.int32)
        w_in = np.nonzero(inside)[0]
        if w_in.size:
            sl[w_in] = walk(arrays, r[w_in], Z[w_in])
        succ_root[live] = sr.reshape(L, nv, n_c)
        succ_leaf[live] = sl.reshape(L, nv, n_c)
        all_inside = inside.reshape(L, nv * n_c).all(axis=1)
        status[live] = np.where(~in_region, MODE_REGION, np.where(all_inside, INVARIANT, EXITS))
    counts = [int((status == k).sum()) for k in range(5)]
    worst_leaf, worst_margin = -1, np.nan
    for q in np.nonzero(((status == INVARIANT) | (status == EXITS)) & ~np.isnan(margin))[0]:
        if worst_leaf < 0 or margin[q] < worst_margin:
            worst_leaf, worst_margin = int(q), float(margin[q])
    return SimpleNamespace(status=status, margin=margin, worst=worst, max_violation=maxv,
                           x_next=x_next, succ_root=succ_root, succ_leaf=succ_leaf, counts=counts,
                           worst_leaf=worst_leaf, worst_margin=worst_margin, vertices=V, inputs=U,
                           cell_status=cell, modes=modes, n_corners=n_c)


# -- the cube cases the host and the device tests share ---------------------------------------------
def cube_law(p, K, c=None, n_split=40, seed=0, modes=None):
    """A FlatTree over the full ``kuhn_forest(p)`` (the set is [-1, 1]^p, every vertex dyadic) with
    ``n_split`` random bisections and the vertex inputs K x + c."""
    from tests import reduce_cpu as rc
    rng = np.random.default_rng([97, p, seed])
    K = np.asarray(K, dtype=np.float64)
    c = np.zeros(K.shape[0]) if c is None else np.asarray(c, dtype=np.float64)
    return rc.kuhn_tree(p, None, n_split, rng, rc.affine_inputs(K, c), K.shape[0], modes=modes)


def identity_plant(p, n_modes=1, E=None, regions=None):
    """x+ = x + u (+ E d) in every mode, no state rows."""
    from explicit_hybrid_mpc_amd import simulate
    eye = np.eye(p)
    return simulate.Plant([eye] * n_modes, [eye] * n_modes, [np.zeros(p)] * n_modes, E,
                          [None] * n_modes if regions is None else regions, None, None, eye, eye,
                          'inf')


def exact_cube_weights(forest, root, x):
    """The exact weights of the dyadic point x in root ``root`` of the forest, as floats."""
    Y, D = forest.scaled(x)
    return np.array([w / D for w in forest.root_weights(int(root), Y, D)])
