"""
Leaf cells of a compiled law and its certificate leaf by leaf (DESIGN.md 3.8f,
csrc/ehm_certify.hip):

    cells = law.cells()                 # LeafCells of every leaf; law.cells(leaves=[3, 7]) of some
    cells.vertices                      # [n, p+1, p] the simplex of each leaf
    cells.inputs                        # [n, p+1, n_u] the leaf's own map at its vertices
    cells.status                        # [n] 0 a cell, 1 no_cell (CELL_STATUS_NAMES)
    res = law.certify(oracle)           # CertificateResult: counts by status (STATUS_NAMES),
    res.certified_volume_fraction       # certified volume over the roots' volume, res.passed

A compiled law keeps no vertices.  Every split of the partition was a bisection, so the cell of a
leaf follows from the law's own arrays: the root's vertices (``applied.root_cells``) and, at every
plane node on the leaf's path, the two vertices the plane separates -- the one with a . v + b near
+1 and the one near -1, the ends of the bisected edge -- whose midpoint replaces the negative-side
vertex in the left child and the positive-side one in the right child.  The midpoint is the
partition engine's expression, (v + w) / 2, so below the root's vertices the cells are the
partition's own bit for bit; the root's vertices carry the error of recovering them from the root
records (inv(inv(E))).  ``inputs`` are u_0 + K (v - v_0) of THIS leaf's record at each vertex in the
law's own arithmetic (a single law: xs = (float) v, float sums, widened) -- not the tree walked
again: a vertex lies on several leaves, and a statement about a leaf is about its own map.

With the cells a law is certified leaf by leaf and not only audited at samples (``certify``): on a
leaf the law is affine, the cost V_d(x, u(x)) of its input under a fixed commutation d is convex in
x, so the costs W of the vertex inputs bound it from above on the whole cell, and the decision form
of the reference's bar_E_delta_R with Vbar = W (``ehm_bar_e_batch``) closing the cell proves
V_u(x) - V*(x) < max(eps_a, eps_r V*(x)) at every state of the leaf -- the contract of
``CompiledLaw.audit``.  ``uncertified`` is not a violation: the interpolation is an upper bound.
What the cells are and are not:
they are the cells the law's planes define for the piecewise-affine function its arrays define;
they say nothing about the rounding of a single law's evaluation (DESIGN.md 3.8c bounds it) nor
about a state within rounding of a split face being handed to the sibling leaf's map.

Works for double and single laws, compiled here or loaded.  A law with test nodes has no cells
(``EhmError``; ``compile(spine='roots')`` has none).  A leaf deeper than ``MAX_DEPTH`` levels below
its root, and a leaf whose path holds a node that is no bisection of the cell that reaches it, get
status ``no_cell`` and NaN rows; the law is not refused.
"""

import ctypes

import numpy as np

from . import _capi
from ._capi import ptr

CELL_STATUS_NAMES = ('cell', 'no_cell')
STATUS_NAMES = ('certified', 'uncertified', 'inadmissible', 'no_law', 'no_cell', 'stalled')
SECONDS = ('kernels', 'feasibility', 'costs', 'tests', 'volumes', 'rest')
MAX_DEPTH = _capi.EHM_CELL_MAX_DEPTH


_check = _capi.checker('ehm_certify_last_error')


class LeafCells:
    """What ``CompiledLaw.cells`` returns: ``leaves`` int32 [n] (rows of the law's leaf records),
    ``leaf_node`` int32 [n] (their source node ids), ``vertices`` [n, p+1, p], ``inputs``
    [n, p+1, n_u], ``status`` int32 [n] (index into CELL_STATUS_NAMES); rows without a cell are
    NaN.  ``counts``: leaves by status name."""

    def __init__(self, leaves, leaf_node, vertices, inputs, status):
        self.leaves, self.leaf_node = leaves, leaf_node
        self.vertices, self.inputs, self.status = vertices, inputs, status

    @property
    def counts(self):
        return {name: int((self.status == k).sum()) for k, name in enumerate(CELL_STATUS_NAMES)}

    def __len__(self):
        return self.status.size

    def __repr__(self):
        return 'LeafCells(n=%d, counts=%r)' % (len(self), self.counts)


def cells(law, leaves=None):
    """The cells of ``leaves`` (rows of the leaf records; None: all) of a ``CompiledLaw``."""
    from . import applied
    if not getattr(law, '_handle', None):
        raise ValueError('the law is closed')
    if law._h['n_test'] > 0:
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its cells do not '
                             "follow from its planes -- compile(spine='roots') has none" %
                             law._h['n_test'])
    ids = _leaf_ids(law, leaves)
    if law._root_cells is None:
        law._root_cells = applied.root_cells(law)
    roots = law._root_cells['vertices']
    n, p, n_u = ids.size, law.p, law.n_u
    vertices = np.empty((n, p + 1, p))
    inputs = np.empty((n, p + 1, n_u))
    status = np.empty(n, dtype=np.int32)
    _check(_capi.load().ehm_compiled_cells(law._handle, ptr(roots), n,
                                           None if leaves is None else ptr(ids), ptr(vertices),
                                           ptr(inputs), ptr(status)))
    return LeafCells(ids, law.leaf_node[ids], vertices, inputs, status)


def _leaf_ids(law, leaves):
    n_leaf = law._h['n_leaf']
    if leaves is None:
        return np.arange(n_leaf, dtype=np.int32)
    given = np.asarray(leaves)
    if given.ndim != 1 or (given.size and given.dtype.kind not in 'iu'):
        raise ValueError('leaves must be a 1-d array of leaf record indices')
    if given.size and (int(given.min()) < 0 or int(given.max()) >= n_leaf):
        raise ValueError('leaves must lie in 0 .. %d' % (n_leaf - 1))
    return np.ascontiguousarray(given, dtype=np.int32)


class CertificateResult:
    """
    What ``CompiledLaw.certify`` found: ``counts`` leaves by status name
    (STATUS_NAMES), ``certified_volume_fraction`` the certified cells' volume over the roots' (the
    reference's progress metric; over the roots of the whole law also when only some ``leaves``
    were asked for), ``cell_volume_fraction`` the same for every leaf that has a cell, ``worst`` the
    uncertified leaf with the largest ``tbest`` (dict of leaf, leaf_node, tbest; None if there is
    none), ``n_relaxed`` the leaves whose certificate is for an input within ``input_tol`` of the
    law's, ``seconds`` by stage (SECONDS), ``n``, ``input_tol``, ``max_tries``, and with
    ``return_leaves`` the per-leaf arrays ``leaves, leaf_node, status, delta_idx, tbest, tries,
    relaxed, n_candidates, volume, vertices, inputs, W``.  ``passed``: every leaf that has a law
    is certified.  ``uncertified`` is NOT a violation: the interpolation of a convex function over
    the cell is an upper bound of it, not the function; it says this test could not close the leaf.
    """

    def __init__(self, **kw):
        self.leaves = self.leaf_node = self.status = self.delta_idx = self.tbest = None
        self.tries = self.relaxed = self.n_candidates = self.volume = None
        self.vertices = self.inputs = self.W = None
        self.__dict__.update(kw)

    @property
    def passed(self):
        return self.counts['certified'] == self.n - self.counts['no_law']

    def __repr__(self):
        return 'CertificateResult(n=%d, passed=%s, counts=%r, certified_volume_fraction=%.6g, ' \
            'n_relaxed=%d)' % (self.n, self.passed, self.counts, self.certified_volume_fraction,
                               self.n_relaxed)


def certify(law, oracle, leaves=None, input_tol=None, max_tries=3, chunk=0,
            return_leaves=False):
    """The one path to ``ehm_compiled_certify``; see ``CompiledLaw.certify``."""
    from . import applied
    if not getattr(law, '_handle', None):
        raise ValueError('the law is closed')
    gp = applied.oracle_gpu(oracle)
    if law._h['n_test'] > 0:
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its roots do '
                             "not tile the set -- compile(spine='roots') has none" %
                             law._h['n_test'])
    p, n_u = law.p, law.n_u
    if gp.can.p != p or gp.can.n_u != n_u:
        raise ValueError('the oracle has p = %d, n_u = %d, the law %d, %d' % (
            gp.can.p, gp.can.n_u, p, n_u))
    max_tries, chunk = int(max_tries), int(chunk)
    if max_tries < 0 or chunk < 0:
        raise ValueError('max_tries and chunk must be >= 0')
    if input_tol is None:
        if law._input_scale is None:
            u0 = law.array('leaf_rec')[:, p:p + n_u]
            law._input_scale = applied.default_input_tol(u0)
        input_tol = law._input_scale
    input_tol = float(input_tol)
    ap = applied.applied_gpu(oracle, 0.)            # ValueError for p + n_u > EHM_MAX_P
    relaxed = applied.applied_gpu(oracle, input_tol) if input_tol > 0. else None
    ids = _leaf_ids(law, leaves)
    if law._root_cells is None:
        law._root_cells = applied.root_cells(law)
    roots = law._root_cells
    n = ids.size
    opts = _capi.CertifyOpts(n=n, leaf_ids=None if leaves is None else ptr(ids),
                             root_vertices=ptr(roots['vertices']), chunk=chunk,
                             relaxed=None if relaxed is None else relaxed._handle,
                             cost_u=ptr(ap.can.cost_u), p=p, n_u=n_u,
                             n_delta=int(gp.can.n_delta), max_tries=max_tries,
                             device=int(law.device))
    res = _capi.CertifyResult()
    arrays, lv = {}, None
    if return_leaves:
        i4 = lambda: np.empty(n, np.int32)
        arrays = dict(status=i4(), delta_idx=i4(), tbest=np.empty(n), tries=i4(), relaxed=i4(),
                      n_candidates=i4(), volume=np.empty(n), vertices=np.empty((n, p + 1, p)),
                      inputs=np.empty((n, p + 1, n_u)), W=np.empty((n, p + 1)))
        lv = ctypes.byref(_capi.CertifyLeaves(**{k: ptr(a) for k, a in arrays.items()}))
        arrays.update(leaves=ids, leaf_node=law.leaf_node[ids])
    _check(_capi.load().ehm_compiled_certify(law._handle, gp._handle, ap._handle,
                                             ctypes.byref(opts), ctypes.byref(res), lv))
    total = float(roots['volume'].sum())
    worst = None
    if res.worst_leaf >= 0:
        l = int(ids[res.worst_leaf])
        worst = dict(leaf=l, leaf_node=int(law.leaf_node[l]), tbest=float(res.worst_tbest))
    return CertificateResult(
        n=n, counts={name: int(res.counts[k]) for k, name in enumerate(STATUS_NAMES)},
        certified_volume_fraction=float(res.certified_volume) / total,
        cell_volume_fraction=float(res.cell_volume) / total, worst=worst,
        n_relaxed=int(res.relaxed), seconds=dict(zip(SECONDS, res.seconds[:])),
        input_tol=input_tol, max_tries=max_tries, **arrays)
