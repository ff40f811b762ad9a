"""
Numpy mirror of the single-precision compiled law (csrc/ehm_compiled32.hip, DESIGN.md 3.8c "single
precision"); test infrastructure, host only.

    arrays32 = narrow(arrays)                     # k_compiled_narrow; NarrowError where it refuses
    u, leaf, depth, levels = evaluate32(arrays32, X)
    mir = mirror32(arrays32, leaf_mode, plant, X0, T, ...)      # k_compiled_rollout<float, ..>

``arrays`` are in the layout of ``CompiledLaw.arrays()``.  The root is chosen by the double mirror
(``compiled_cpu._locate`` / ``_first_root``) on the double state; below it everything is numpy
float32, one rounding per product and per sum in the device's order, so on exported arrays the
results are bit-equal to the device's.

The two bounds of the contract between the single law and the double law it was narrowed from, with
u = 2^-24 the unit roundoff of a float:

``turn_bound`` = (p + 4) u (sum |a_i x_i| + |b|).  The single sum runs on a_i (1 + d), x_i (1 + d),
rounds each product and each of its p additions (the first, 0 + a_0 xs_0, is exact; + b is the
last): a term passes at most p + 3 roundings, b two, and gamma_(p+3) <= (p + 4) u.  So the single
law's s is within turn_bound of the exact a . x + b, and it can turn against the double law only
where |s64| is that small.

``u_bound`` = (p + 4) u (|u_0c| + sum_i |K_ci| (|d_i| + 2 (|x_i| + |v_0i|))), d = x - v_0: the same
count for the leaf's sum, with the error of d_i = xs_i - v32_0i, at most u (|x_i| + |v_0i|) from the
two narrowings plus one rounding of the difference, carried through K.
"""

import contextlib
from fractions import Fraction

import numpy as np

from tests import compiled_cpu as cc
from tests import compiled_rollout_cpu as cr
from tests import explicit_synth as es

U32 = 2. ** -24
EPS32 = np.float32(2. ** -23)
FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def node_stride32(p):
    return 8 if p <= 5 else 16


def leaf_stride32(p, n_u):
    return (p + n_u + n_u * p + 3) // 4 * 4


class NarrowError(ValueError):
    """What k_compiled_narrow refuses; ``reason`` in ('test nodes', 'overflow', 'underflow',
    'zero normal')."""

    def __init__(self, reason):
        super().__init__('no single-precision form: ' + reason)
        self.reason = reason


def _narrow_values(a):
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        f = a.astype(np.float32)
    if not np.isfinite(f).all():
        raise NarrowError('overflow')
    if ((a != 0.) & (np.abs(f) < FLT_MIN)).any():
        raise NarrowError('underflow')
    return f


def narrow(arrays):
    """The arrays of the single law of a double law's arrays: node[:, :p+1] and leaf_rec rounded to
    nearest float at the single strides, the child pair copied, everything else unchanged."""
    h = dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))
    if h['n_test'] > 0:
        raise NarrowError('test nodes')
    p, n_u = h['p'], h['n_u']
    ns, ls = node_stride32(p), leaf_stride32(p, n_u)
    node64 = np.ascontiguousarray(arrays['node'], dtype=np.float64).reshape(h['n_int'],
                                                                           h['node_stride'])
    leaf64 = np.ascontiguousarray(arrays['leaf_rec'], dtype=np.float64).reshape(h['n_leaf'],
                                                                               h['leaf_stride'])
    used = p + n_u + n_u * p
    leaf32 = np.zeros((h['n_leaf'], ls), dtype=np.float32)
    node32 = np.zeros((h['n_int'], ns), dtype=np.float32)
    node32[:, :p + 1] = _narrow_values(node64[:, :p + 1])
    leaf32[:, :used] = _narrow_values(leaf64[:, :used])
    if h['n_int'] and (node32[:, :p] == 0).all(axis=1).any():
        raise NarrowError('zero normal')
    node32.view(np.int32)[:, p + 1:p + 3] = \
        node64[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)
    out = {k: np.array(v, copy=True) for k, v in arrays.items()}
    out['header'][cc.HEADER.index('node_stride')] = ns
    out['header'][cc.HEADER.index('leaf_stride')] = ls
    out['node'], out['leaf_rec'] = node32, leaf32
    return out


def _header(arrays32):
    h = dict(zip(cc.HEADER, (int(v) for v in arrays32['header'])))
    assert h['n_test'] == 0 and h['node_stride'] == node_stride32(h['p'])
    assert arrays32['node'].dtype == np.float32 and arrays32['leaf_rec'].dtype == np.float32
    return h


def walk32_from(arrays32, h, root, X, levels=None):
    """The single walk and leaf map from the roots ``root`` for the double states X: (leaf index in
    the compiled arrays, u float64, levels walked).  ``levels`` (a list) receives per level
    (states, their nodes, s float32, went left)."""
    p, n_u = h['p'], h['n_u']
    n = X.shape[0]
    node = np.ascontiguousarray(arrays32['node']).reshape(h['n_int'], h['node_stride'])
    children = node.view(np.int32)[:, p + 1:p + 3]
    with np.errstate(over='ignore', invalid='ignore'):
        xs = X.astype(np.float32)
    k = np.asarray(arrays32['root_entry'])[root].astype(np.int64)
    walked = np.zeros(n, dtype=np.int64)
    live = np.nonzero(k >= 0)[0]
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        while live.size:
            rec = node[k[live]]
            walked[live] += 1
            s = np.zeros(live.size, dtype=np.float32)
            for c in range(p):
                s = s + rec[:, c] * xs[live, c]
            s = s + rec[:, p]
            go_left = s >= -EPS32
            if levels is not None:
                levels.append((live.copy(), k[live].copy(), s, go_left))
            k[live] = np.where(go_left, children[k[live], 0], children[k[live], 1])
            live = live[k[live] >= 0]
        l = ~k
        lr = np.ascontiguousarray(arrays32['leaf_rec']).reshape(h['n_leaf'], h['leaf_stride'])[l]
        d = xs - lr[:, :p]
        u = np.empty((n, n_u))
        for c in range(n_u):
            t = np.zeros(n, dtype=np.float32)
            for q in range(p):
                t = t + lr[:, p + n_u + c * p + q] * d[:, q]
            u[:, c] = (lr[:, p + c] + t).astype(np.float64)
    return l, u, walked


def choose_root(arrays, X, locate=True):
    """(root, decisions made) per state: the double law's rule on the double state, for the arrays
    of either precision."""
    h = dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))
    p, n = h['p'], X.shape[0]
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    root = np.full(n, -1, dtype=np.int64)
    depth = np.zeros(n, dtype=np.int64)
    if h['has_nbr'] and locate:
        root, depth = cc._locate(root_rec, np.asarray(arrays['nbr']), X, p)
        depth = np.where(root >= 0, depth, 0)
    todo = np.nonzero(root < 0)[0]
    root[todo], depth[todo] = cc._first_root(root_rec, X[todo], p)
    return root, depth


def evaluate32(arrays32, X, locate=True):
    """(u [n, n_u] float64, leaf [n] source node ids, depth [n], levels) of the states X under the
    single law, in the device's order of operations."""
    h = _header(arrays32)
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64).reshape(-1, h['p'])
    root, depth = choose_root(arrays32, X, locate)
    levels = []
    l, u, walked = walk32_from(arrays32, h, root, X, levels)
    leaf = np.asarray(arrays32['leaf_node'])[l].astype(np.int32)
    return u, leaf, (depth + walked).astype(np.int32), levels


def turn_bound(arrays, nodes, X):
    """(p + 4) 2^-24 (sum |a_i x_i| + |b|) for the double law's records ``nodes`` and the states X,
    and s64, the double mirror's sum there."""
    h = dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))
    p = h['p']
    rec = np.asarray(arrays['node'], dtype=np.float64).reshape(h['n_int'], h['node_stride'])[nodes]
    s = np.zeros(X.shape[0])
    mag = np.zeros(X.shape[0])
    for c in range(p):
        s = s + rec[:, c] * X[:, c]
        mag = mag + np.abs(rec[:, c] * X[:, c])
    s = s + rec[:, p]
    return (p + 4) * U32 * (mag + np.abs(rec[:, p])), s


def u_bound(arrays, leaves, X):
    """(p + 4) 2^-24 (|u_0c| + sum_i |K_ci| (|d_i| + 2 (|x_i| + |v_0i|))) [n, n_u] for the double
    law's leaf records ``leaves`` (indices in the compiled arrays) and the states X."""
    h = dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))
    p, n_u = h['p'], h['n_u']
    lr = np.asarray(arrays['leaf_rec'], dtype=np.float64).reshape(h['n_leaf'], h['leaf_stride'])[
        leaves]
    v0, u0 = lr[:, :p], lr[:, p:p + n_u]
    K = lr[:, p + n_u:p + n_u + n_u * p].reshape(-1, n_u, p)
    w = np.abs(X - v0) + 2. * (np.abs(X) + np.abs(v0))
    return (p + 4) * U32 * (np.abs(u0) + np.einsum('nci,ni->nc', np.abs(K), w))


def exact_sum(rec, x, p):
    """a . x + b of one record in rational arithmetic (the values as they are stored)."""
    return sum((Fraction(float(rec[c])) * Fraction(float(x[c])) for c in range(p)),
               Fraction(float(rec[p])))


# -- the closed loop ------------------------------------------------------------------------------
@contextlib.contextmanager
def _single_walk():
    """``compiled_rollout_cpu.mirror`` with the single walk in place of the double one: every other
    piece of the step -- the root, the exit test, the plant, the noise, the records -- is the
    double law's mirror itself."""
    keep = cr.walk_from

    def walk(arrays32, h, root, X):
        l, u, _ = walk32_from(arrays32, h, root, X)
        return l, u

    cr.walk_from = walk
    try:
        yield
    finally:
        cr.walk_from = keep


def mirror32(arrays32, leaf_mode, plant, X0, T, **kw):
    """``compiled_rollout_cpu.mirror`` for the arrays of a single law."""
    _header(arrays32)
    with _single_walk():
        return cr.mirror(arrays32, leaf_mode, plant, X0, T, **kw)


N_TRAJ, T_STEPS = 257, 12


def case32(kind, p, n_u, draw=0):
    """The law, plant, initial states and rollout arguments of one (kind, p, n_u) instance: the
    recipe of ``compiled_rollout_cpu.case`` at 257 trajectories (a partial block) x 12 steps.  Half
    the states are uniform in the box, half ``law.states`` (in and around the grown subtrees).
    ``draw`` numbers the draws of one instance: a law whose compiled records hold a value below
    the range of a float (elimination noise of an inverse) has no single form, and the caller
    draws again."""
    rng = np.random.default_rng([32, cr.KINDS.index(kind), p, n_u, draw])
    cost = 'inf' if (p + n_u + cr.KINDS.index(kind)) % 2 == 0 else 'quadratic'
    kw = dict(tol_exit=1e-9)
    if kind == 'guarded':
        n_modes = 2 + (p + n_u) % 7
        plant = es.random_guarded(rng, p, n_u, n_modes, cost, substeps=1 + (p * n_u) % 4,
                                  n_rows=1 + (p + 3 * n_u) % 16)
    else:
        n_modes = 1 + (p + 2 * n_u) % 4
        n_d = 8 if (p + n_u) % 2 else 0
        plant = es.random_plant(rng, p, n_u, n_modes, cost, n_d=n_d)
    law = es.SynthLaw(es.kuhn_forest(p), n_u, n_modes, rng)
    X0 = np.concatenate([rng.uniform(-0.9, 0.9, (N_TRAJ // 2, p)),
                         law.states(rng, N_TRAJ)[:N_TRAJ - N_TRAJ // 2]])
    assert X0.shape[0] == N_TRAJ
    if kind == 'noisy':
        kw.update(noise=es.random_noise(rng, p, n_u, plant.n_d), seed=int(rng.integers(1 << 40)),
                  traj0=int(rng.integers(1 << 20)))
    elif kind == 'nominal':
        kw['v'] = rng.normal(size=(T_STEPS, N_TRAJ, p)) * 1e-3
        if plant.n_d:
            kw['d'] = rng.normal(size=(T_STEPS, N_TRAJ, plant.n_d))
    return law, plant, X0, kw
