"""
One-step invariance of a compiled law leaf by leaf (csrc/ehm_invariance.hip), and the
leaves the closed loop never leaves (csrc/ehm_core.hip; ``invariant_core`` below), and
where the loop goes from a set of leaves (csrc/ehm_reach.hip; ``CoreResult.reach``,
``reach_relation`` and ``ReachResult`` at the end):

    res = law.successors()                      # SuccessorResult of every leaf, nominal successor
    res = law.successors(d_box=(lo, hi))        # under every disturbance of the box
    res.counts                                  # leaves by status name (STATUS_NAMES)
    res.status, res.margin, res.worst           # per leaf
    res.invariant_volume_fraction, res.set_convex, res.holds_on_set

The argument.  On a leaf the law is affine, u = u_0 + K (x - v_0).  In the leaf's step-0 mode m the
plant of ``rollout`` is x+ = A_m x + B_m u + w_m + E d, affine in (x, u, d).  So the successor map
(x, d) -> x+ is affine on cell x box, and the image of the leaf under every disturbance of the box is
the convex hull of its successors at the (p + 1) 2^n_d points (cell vertex, box corner).  If all of
them lie in a CONVEX set, so does every successor of every state of the leaf.  The set is the union
of the law's roots, where the law exists; ``roots_convex`` decides whether it is convex.

A leaf is ``invariant`` when every one of those successors, located as one step of ``rollout``
locates its state, passes the rollout's exit test on its root's weights (``tol_exit``), and every
vertex of the cell passes the region rows of the leaf's mode (the rollout's status 2; a region is
convex, so the whole cell lies in it).  ``exits``: some successor fails the exit test.  Where every
leaf is invariant and the set is convex (``holds_on_set``) no trajectory of the nominal plant under
disturbances of the box ever stops with status 1 or 2, whatever its length.

What the result covers: the piecewise-affine function the law's arrays define on the cells their
planes define (``cells``), and the nominal plant of ``simulate.Plant`` with a box disturbance.  It
does not cover: measurement error v or input error e (``robust.py``, DESIGN.md 3.8j, does: the
closed-form facet test and the core with a generator block per mode); the rounding of a single
law's evaluation at interior points (DESIGN.md 3.8c bounds it); a state within rounding of a split
face being handed to the sibling leaf's map; the recovery error of the root vertices the cells
carry.  Without a convex set ``invariant`` is a statement about the vertex successors only.
``margin`` is in units of the chosen root's barycentric weights: for a point outside it orders
leaves, it is not a distance.
"""

import ctypes

import numpy as np

from . import _capi
from ._capi import ptr

STATUS_NAMES = ('invariant', 'exits', 'mode_region', 'no_mode', 'no_cell')
MAX_D = 8                       # EHM_R_MAX_D: 2^8 corners
# ``CoreResult.status``: the one-step status, and ``unresolved`` for a leaf whose row was cut off
CORE_STATUS_NAMES = STATUS_NAMES + ('unresolved',)
CORE_COUNT_NAMES = ('core', 'transient') + CORE_STATUS_NAMES[1:]
CORE_ROWS = {'invariant': 0, 'all': 1}          # EHM_CORE_ROWS_*
# Resource caps of ``invariant_core``.  A row longer than MAX_FAN is cut off (its leaf is a seed);
# the relation takes 4 bytes per edge on the device, and as much on the host with return_edges:
# 512 MiB at MAX_EDGES.
MAX_FAN = 4096
MAX_EDGES = 1 << 27


_check = _capi.checker('ehm_invariance_last_error')
_check_core = _capi.checker('ehm_core_last_error')


def roots_convex(root_vertices, rtol=1e-9):
    """True iff the union of the simplices ``root_vertices`` [n_roots, p+1, p] is convex: the third
    return of ``boundary_facets``, which says how it is decided."""
    return boundary_facets(root_vertices, rtol)[2]


def boundary_facets(root_vertices, rtol=1e-9):
    """
    (normals [n_b, p], offsets [n_b], convex): the boundary facets of the union of the simplices
    ``root_vertices`` [n_roots, p+1, p] as half-spaces normal . x >= offset with unit normals, and
    whether the union is convex -- it is then the intersection of those half-spaces; host numpy.

    The vertices are deduplicated first: per coordinate, values closer than rtol max|v| are one
    value, so vertices that differ in their last bits between roots are one vertex.  The boundary
    facets are the facets (p vertices of a root) owned by exactly one root; each one's plane is
    oriented by the owning root's opposite vertex.  The union is reported convex iff every distinct
    vertex lies on the inner side of every boundary plane within rtol max|v| (unit normals).

    Why that decides it: a closed union of simplices that lies inside the intersection of its
    boundary facets' half-spaces and has nonempty interior IS that intersection -- a point of the
    intersection outside the union could be joined to an interior point of the union by a segment
    that leaves the union through a boundary facet, at whose plane it would change sides -- and an
    intersection of half-spaces is convex; the union lies inside iff its vertices do.  Conversely
    a convex union lies on one side of the plane of each of its boundary facets.  Limits: the roots
    must be a face-to-face triangulation (a facet that is a proper part of a neighbour's facet
    counts as boundary, and the answer is then False where it should be True, never the other way);
    roots of no volume have no side and are not supported; the test is within rtol, so a dent
    shallower than rtol max|v| is not seen.  The facet-by-vertex products are made in chunks of at
    most about 256 MB.
    """
    V = np.ascontiguousarray(root_vertices, dtype=np.float64)
    if V.ndim != 3 or V.shape[1] != V.shape[2] + 1:
        raise ValueError('root_vertices must be [n_roots, p+1, p]')
    R, nv, p = V.shape
    none = np.zeros((0, p)), np.zeros(0)
    if R == 0:
        return none + (True,)
    scale = float(np.abs(V).max())
    tol = float(rtol) * (scale if scale > 0. else 1.)
    flat = V.reshape(-1, p)
    key = np.empty(flat.shape, dtype=np.int64)
    for c in range(p):
        order = np.argsort(flat[:, c], kind='stable')
        step = np.concatenate([[0], (np.diff(flat[order, c]) > tol).astype(np.int64)])
        key[order, c] = np.cumsum(step)
    uniq, first, vid = np.unique(key, axis=0, return_index=True, return_inverse=True)
    points = flat[first]                                        # [n_points, p]
    vid = vid.reshape(R, nv)
    if p == 1:
        lo, hi = points.min(), points.max()
        covered = np.sort(V[:, :, 0], axis=1)
        order = np.argsort(covered[:, 0])
        reach = np.maximum.accumulate(covered[order, 1])
        return (np.array([[1.], [-1.]]), np.array([lo, -hi]),
                bool((covered[order, 0][1:] <= reach[:-1] + tol).all() and reach[-1] >= hi - tol
                     and covered[order, 0][0] <= lo + tol))
    # every facet: the root's vertices without the k-th, which is its opposite vertex
    keep = np.array([[j for j in range(nv) if j != k] for k in range(nv)])      # [nv, p]
    facets = np.sort(vid[:, keep], axis=2).reshape(-1, p)                       # [R nv, p]
    opposite = vid.reshape(-1)                                                  # facet r nv + k: k
    _, index, counts = np.unique(facets, axis=0, return_index=True, return_counts=True)
    boundary = index[counts == 1]
    if boundary.size == 0:
        return none + (True,)
    F = points[facets[boundary]]                                                # [nb, p, p]
    edges = F[:, 1:] - F[:, :1]                                                 # [nb, p-1, p]
    normal = np.linalg.svd(edges, full_matrices=True)[2][:, -1, :]              # unit, [nb, p]
    side = np.einsum('fc,fc->f', normal, points[opposite[boundary]] - F[:, 0])
    normal = normal * np.where(side < 0., -1., 1.)[:, None]
    offset = np.einsum('fc,fc->f', normal, F[:, 0])
    rows = max(1, (1 << 25) // max(1, points.shape[0]))
    for s in range(0, normal.shape[0], rows):
        d = normal[s:s + rows] @ points.T - offset[s:s + rows, None]
        if (d < -tol).any():
            return normal, offset, False
    return normal, offset, True


class SuccessorResult:
    """
    What ``CompiledLaw.successors`` found: ``n`` leaves asked for, ``counts`` by
    status name (STATUS_NAMES); per leaf ``leaves`` (rows of the leaf records), ``leaf_node``,
    ``status`` int32, ``margin`` (the smallest weight of any vertex successor in the root that
    holds it; NaN without a cell or mode), ``worst`` = i n_c + j, the (vertex, corner) pair that
    gives it, ``max_violation`` (of the plant's state rows at the successors);
    ``invariant_volume_fraction`` and ``cell_volume_fraction`` over the roots' volume (of the whole
    law also when only some ``leaves`` were asked for); ``worst_leaf`` (dict of leaf, leaf_node,
    margin; None) the leaf of status invariant or exits with the smallest margin, ``worst_margin``;
    ``seconds`` of the kernel; ``n_corners``; ``set_convex`` (``roots_convex`` of the law's roots);
    ``holds_on_set``: every requested leaf is invariant, every leaf was requested, and the set is
    convex.  With ``return_successors``: ``x_next`` [n, p+1, n_c, p], ``succ_root`` and
    ``succ_leaf`` [n, p+1, n_c] (-1 where the successor is outside).
    """

    x_next = succ_root = succ_leaf = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'SuccessorResult(n=%d, counts=%r, invariant_volume_fraction=%.6g, ' \
            'worst_margin=%.3g, set_convex=%s, holds_on_set=%s)' % (
                self.n, self.counts, self.invariant_volume_fraction, self.worst_margin,
                self.set_convex, self.holds_on_set)


def _box(plant, d_box):
    """(lo, hi) float64 [n_d] of ``d_box``, or (None, None) for the nominal successor."""
    if d_box is None:
        return None, None
    try:
        lo, hi = d_box
    except (TypeError, ValueError):
        raise ValueError('d_box must be (lo, hi)')
    lo = np.ascontiguousarray(np.atleast_1d(lo), dtype=np.float64)
    hi = np.ascontiguousarray(np.atleast_1d(hi), dtype=np.float64)
    if lo.shape != (plant.n_d,) or hi.shape != (plant.n_d,):
        raise ValueError('d_box must be two arrays [%d] (the plant\'s n_d)' % plant.n_d)
    if plant.n_d > MAX_D:
        raise ValueError('a box of %d disturbances has more than 2^%d corners' % (plant.n_d,
                                                                                 MAX_D))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError('d_box must be finite with lo <= hi')
    return lo, hi


class _Step:
    """What both entry points need of (law, plant, d_box, tol_exit), resolved once: ``plant``, the
    box ``lo`` / ``hi`` (None without one) and ``n_d`` (0 without one), ``tol_exit`` and ``chunk``,
    the plant's arrays as contiguous float64 (``A B w E H h Gx gx``; ``rows`` int32), the leaf
    ``modes`` int32, the law's root cells ``roots`` and ``set_convex``."""

    def __init__(self, law, plant, d_box, tol_exit, chunk=0):
        from . import applied, simulate
        if not getattr(law, '_handle', None):
            raise ValueError('the law is closed')
        if plant is None:
            plant = law._rollout_plant
        if plant is None and law.mpc is not None:
            plant = simulate.Plant.from_mpc(law.mpc)
        if plant is None:
            raise ValueError('successors needs a plant: the law has none and no mpc to make one '
                             'from')
        if plant.guarded:
            raise ValueError('a guarded plant chooses its mode per substep by its guards: the '
                             'successor is not affine on a leaf')
        if plant.n_x != law.p or plant.n_u != law.n_u:
            raise ValueError('plant (n_x %d, n_u %d) does not fit the law (p %d, n_u %d)' % (
                plant.n_x, plant.n_u, law.p, law.n_u))
        self.plant = plant
        self._set_box(d_box)
        self.tol_exit, self.chunk = float(tol_exit), int(chunk)
        if not self.tol_exit >= 0. or self.chunk < 0:
            raise ValueError('tol_exit and chunk must be >= 0')
        if law._h['n_test'] > 0:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its cells do '
                                 "not follow from its planes -- compile(spine='roots') has none" %
                                 law._h['n_test'])
        self.modes = np.ascontiguousarray(law._plant_modes(plant), dtype=np.int32)
        if law._root_cells is None:
            law._root_cells = applied.root_cells(law)
        self.roots = law._root_cells
        if getattr(law, '_set_facets', None) is None:
            law._set_facets = boundary_facets(self.roots['vertices'])
            law._set_convex = law._set_facets[2]
        self.facets = law._set_facets
        self.set_convex = bool(law._set_convex)
        rows, H, h = plant.region_arrays()
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        for k, a in dict(A=plant.A, B=plant.B, w=plant.w, E=plant.E, H=H, h=h, Gx=plant.Gx,
                         gx=plant.gx).items():
            setattr(self, k, np.ascontiguousarray(a, dtype=np.float64))

    def _set_box(self, d_box):
        """``lo`` / ``hi`` / ``n_d`` of the caller's box (``robust._RobustStep`` has three)."""
        self.lo, self.hi = _box(self.plant, d_box)
        self.n_d = 0 if self.lo is None else self.plant.n_d

    def opts(self, **kw):
        """The plant part of an ``InvarianceOpts`` (an empty array, or E without a box: NULL)."""
        opt = lambda a: ptr(a) if a.size else None
        box = lambda a: opt(a) if self.n_d else None
        return _capi.InvarianceOpts(
            root_vertices=ptr(self.roots['vertices']), A=ptr(self.A), B=ptr(self.B), w=ptr(self.w),
            E=box(self.E), leaf_mode=ptr(self.modes), d_lo=box(self.lo), d_hi=box(self.hi),
            tol_exit=self.tol_exit, n_modes=int(self.plant.n_modes), n_d=self.n_d, **kw)


def successors(law, plant=None, d_box=None, leaves=None, tol_exit=1e-9, return_successors=False,
               chunk=0):
    """The one path to ``ehm_compiled_successors``; see ``CompiledLaw.successors``."""
    return _successors(law, _Step(law, plant, d_box, tol_exit, chunk), leaves, return_successors)


def _successors(law, st, leaves, return_successors):
    from . import certify
    ids = certify._leaf_ids(law, leaves)
    n, p = ids.size, law.p
    n_c = 1 << st.n_d
    opt = lambda a: ptr(a) if a.size else None
    opts = st.opts(
        n=n, leaf_ids=None if leaves is None else ptr(ids), chunk=st.chunk,
        region_rows=ptr(st.rows), H=opt(st.H), h=opt(st.h), Gx=opt(st.Gx), gx=opt(st.gx),
        n_g=int(st.gx.size))
    arrays = dict(status=np.empty(n, np.int32), margin=np.empty(n), worst=np.empty(n, np.int32),
                  max_violation=np.empty(n))
    if return_successors:
        arrays.update(x_next=np.empty((n, p + 1, n_c, p)),
                      succ_root=np.empty((n, p + 1, n_c), np.int32),
                      succ_leaf=np.empty((n, p + 1, n_c), np.int32))
    lv = _capi.InvarianceLeaves(**{k: ptr(a) for k, a in arrays.items()})
    res = _capi.InvarianceResult()
    _check(_capi.load().ehm_compiled_successors(law._handle, ctypes.byref(opts),
                                                ctypes.byref(res), ctypes.byref(lv)))
    total = float(st.roots['volume'].sum())
    counts = {name: int(res.counts[k]) for k, name in enumerate(STATUS_NAMES)}
    worst = None
    if res.worst_leaf >= 0:
        l = int(ids[res.worst_leaf])
        worst = dict(leaf=l, leaf_node=int(law.leaf_node[l]), margin=float(res.worst_margin))
    every = n >= law._h['n_leaf'] and np.unique(ids).size == law._h['n_leaf']
    return SuccessorResult(
        n=n, counts=counts, leaves=ids, leaf_node=law.leaf_node[ids], n_corners=n_c,
        invariant_volume_fraction=float(res.invariant_volume) / total,
        cell_volume_fraction=float(res.cell_volume) / total, worst_leaf=worst,
        worst_margin=float(res.worst_margin), seconds=float(res.seconds),
        set_convex=st.set_convex, tol_exit=st.tol_exit,
        holds_on_set=bool(counts['invariant'] == n and every and st.set_convex), **arrays)


def _leaf_rows(law, leaf):
    """The rows of the leaf records with the source node ids ``leaf`` (what ``evaluate`` returns).
    In a refined law (``CompiledLaw.refine``, also one loaded from its file) the children of a split
    leaf share their source node, so a state does not name its leaf record this way: ``ValueError``."""
    unique = getattr(law, '_leaf_node_ascending', None)
    if unique is None:
        unique = law._leaf_node_ascending = bool((np.diff(law.leaf_node) > 0).all())
    if not unique:
        raise ValueError('the leaves of a refined law share source nodes: a state does not name its '
                         'leaf record; give leaf rows (start=, masks) instead of states')
    return np.searchsorted(law.leaf_node, leaf)


class CoreResult:
    """
    What ``CompiledLaw.invariant_core`` found.  Per leaf: ``level`` int32 (-1 for
    a core leaf, 0 for a seed, k >= 1 for a leaf whose every state has its first k successors in
    the set and in its mode's region), ``core`` bool, ``status`` int32 (the one-step status of
    ``successors``, CORE_STATUS_NAMES: ``unresolved`` where the leaf's row was longer than
    ``max_fan``).  ``counts`` by CORE_COUNT_NAMES (core, transient = level >= 1, then the seeds by
    status); ``core_volume_fraction`` and ``cell_volume_fraction`` over the roots' volume;
    ``n_sweeps`` = the largest level + 1; ``n_edges``; ``set_convex``; ``holds``: the set is convex
    and the core is not empty -- every state of a core leaf then stays in the set, in its mode's
    region and in the core for ever, under the assumptions of ``successors``.  ``seeds`` is the
    ``SuccessorResult`` the seeds came from.  With ``return_edges``: ``indptr`` int64 [n_leaf + 1]
    and ``indices`` int32, the may-reach relation as CSR (row order: roots ascending, left before
    right).  ``seconds_reach`` (device time of the relation), ``seconds_sweeps`` (wall time of the
    fixed point).
    """

    indptr = indices = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'CoreResult(counts=%r, core_volume_fraction=%.6g, n_sweeps=%d, n_edges=%d, ' \
            'set_convex=%s, holds=%s)' % (self.counts, self.core_volume_fraction, self.n_sweeps,
                                          self.n_edges, self.set_convex, self.holds)

    def contains(self, X):
        """bool [n]: the leaf the law evaluates X [n, p] in is a core leaf; False where the law has
        no input for the state.  ``evaluate`` answers for every state, so for one outside the set
        this is the answer for the leaf the walk from the last root ends in: ask ``rollout`` or
        the roots whether the state is in the set."""
        if getattr(self, '_law', None) is None or not getattr(self._law, '_handle', None):
            raise ValueError('contains needs the compiled law the result was made for, open')
        u, leaf, _, _ = self._law.evaluate(X, return_info=True)
        row = _leaf_rows(self._law, leaf)
        return self.core[row] & np.isfinite(u).all(axis=1)


def invariant_core(law, plant=None, d_box=None, tol_exit=1e-9, tol_side=None, rows='invariant',
                   return_edges=False, max_fan=MAX_FAN, max_edges=MAX_EDGES):
    """The one path to ``ehm_compiled_core``; see ``CompiledLaw.invariant_core``."""
    tol_side, max_fan, max_edges = _core_args(tol_exit, tol_side, rows, max_fan, max_edges)
    st = _Step(law, plant, d_box, tol_exit)
    seeds = _successors(law, st, None, False)
    return _core(law, st, seeds, tol_side, rows, return_edges, max_fan, max_edges,
                 lambda lib, po, co, res, lv: lib.ehm_compiled_core(law._handle, po, co, res, lv))


def _core_args(tol_exit, tol_side, rows, max_fan, max_edges):
    """(tol_side, max_fan, max_edges) checked, as both core calls take them."""
    if rows not in CORE_ROWS:
        raise ValueError("rows must be 'invariant' or 'all'")
    if not float(tol_exit) >= 0.:
        raise ValueError('tol_exit must be >= 0')
    tol_side = float(tol_exit) if tol_side is None else float(tol_side)
    max_fan, max_edges = int(max_fan), int(max_edges)
    if not tol_side >= 0.:
        raise ValueError('tol_side must be >= 0')
    if max_fan < 1 or not 1 <= max_edges < 2 ** 31:
        raise ValueError('max_fan must be >= 1 and max_edges in 1 .. 2^31 - 1')
    return tol_side, max_fan, max_edges


def _core(law, st, seeds, tol_side, rows, return_edges, max_fan, max_edges, call):
    """The relation and its fixed point from the one-step result ``seeds``; ``call(lib, plant opts,
    core opts, result, leaves)`` is the entry point (``ehm_compiled_core`` or its robust form)."""
    tol_exit = st.tol_exit
    n_leaf = law._h['n_leaf']
    po = st.opts(n=0, n_g=0)
    status_in = np.ascontiguousarray(seeds.status, dtype=np.int32)
    co = _capi.CoreOpts(status=ptr(status_in), n_status=status_in.size, max_edges=max_edges,
                        tol_side=tol_side, max_fan=max_fan, rows=CORE_ROWS[rows],
                        want_edges=int(bool(return_edges)))
    level, status = np.empty(n_leaf, np.int32), np.empty(n_leaf, np.int32)
    indptr = np.empty(n_leaf + 1, np.int64) if return_edges else None
    edges = ctypes.c_void_p(None)
    lv = _capi.CoreLeaves(level=ptr(level), status=ptr(status), indptr=ptr(indptr),
                          indices_out=ctypes.addressof(edges) if return_edges else None)
    res = _capi.CoreResult()
    lib = _capi.load()
    indices = None
    try:
        _check_core(call(lib, ctypes.byref(po), ctypes.byref(co), ctypes.byref(res),
                         ctypes.byref(lv)))
        if return_edges:
            n_e = int(res.n_edges)
            indices = np.empty(n_e, np.int32)
            if n_e:
                ctypes.memmove(indices.ctypes.data, edges.value, n_e * 4)
    finally:
        if edges.value:
            lib.ehm_host_free(edges)
    total = float(st.roots['volume'].sum())
    counts = {name: int(res.counts[k]) for k, name in enumerate(CORE_COUNT_NAMES)}
    core = level < 0
    return CoreResult(
        level=level, core=core, status=status, counts=counts, seeds=seeds,
        core_volume_fraction=float(res.core_volume) / total,
        cell_volume_fraction=float(res.cell_volume) / total, n_sweeps=int(res.n_sweeps),
        n_edges=int(res.n_edges), set_convex=st.set_convex,
        holds=bool(st.set_convex and core.any()), indptr=indptr, indices=indices,
        seconds_reach=float(res.seconds_reach), seconds_sweeps=float(res.seconds_sweeps),
        tol_exit=float(tol_exit), tol_side=tol_side, rows=rows, _law=law)


# -- the reach tube and the limit set of the closed loop (csrc/ehm_reach.hip) ---------

_check_reach = _capi.checker('ehm_reach_last_error')
MAX_STEP_BYTES = 1 << 28        # (horizon + 1) n_leaf of ``return_steps``
ROW_MAP = 'wave'                # the default row mapping: 4x to 10x faster


class ReachResult:
    """
    What ``CoreResult.reach`` / ``reach_relation`` found, all sets as masks or
    arrays over the leaf records.  Seeds (``level == 0``) are absorbing: nothing is claimed of a
    trajectory after it reaches one.

    Arrival: ``arrival`` int32 (the first step a leaf can be reached at from the start set, -1:
    never), ``closure`` bool, ``n_arrival``, ``leak_step`` (the first step a seed can be reached at,
    -1: never) and ``safe`` (``leak_step == -1``); ``tube_box`` [n_arrival + 1, 2, p] and
    ``tube_count``: the box (lo, hi) and size of the leaves reached within k steps.

    Limit set (only when ``safe``): ``limit`` bool, the fixed point of D_0 = closure,
    D_(j+1) = post(D_j) (None when a phase did not finish; ``limit_outer`` is then the last D_j,
    or None); ``depart`` int32, the first j >= 1 with the leaf not in D_j (-1 for limit leaves and
    outside the closure); ``settle``; ``settle_box`` [settle + 1, 2, p], ``settle_count``;
    ``limit_box`` = ``settle_box[-1]``.

    Step sets: ``step_box`` [H' + 1, 2, p] and ``step_count`` of R_k = post^k(start), H' the horizon
    cut at ``leak_step``; ``steps`` uint8 [H' + 1, n_leaf] with ``return_steps``.

    The box of an empty set, or of leaves without a cell, is NaN.  ``closure_volume_fraction`` and
    ``limit_volume_fraction`` over the roots' volume (None without a law's cells).  ``converged``:
    every phase that ran finished within ``max_sweeps``.  ``holds``: the core's set is convex, the
    run is ``safe`` and converged -- then a trajectory whose step-0 state is evaluated in a start
    leaf is, at every step k, evaluated in a leaf of the closure, of R_k and of D_min(k, settle).
    ``n_outside``: states of ``X0`` the law has no input for.  ``seconds_boxes``, ``seconds_arrival``,
    ``seconds_settle``, ``seconds_steps``: device time; ``seconds_upload``: wall time of checking and
    uploading the relation.
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'ReachResult(closure=%d, n_arrival=%d, leak_step=%d, limit=%s, settle=%s, ' \
            'converged=%s, holds=%s)' % (
                int(self.closure.sum()), self.n_arrival, self.leak_step,
                None if self.limit is None else int(self.limit.sum()), self.settle, self.converged,
                self.holds)

    def contains(self, X, k=None):
        """bool [n]: the leaf the law evaluates X [n, p] in lies in the limit set (``k`` None) or in
        D_min(k, settle); False where the law has no input for the state.  As ``CoreResult.contains``
        it answers for the leaf ``evaluate`` returns, also for a state outside the set."""
        if self.limit is None:
            raise ValueError('contains needs a limit set: the run leaks or did not converge')
        if getattr(self, '_law', None) is None or not getattr(self._law, '_handle', None):
            raise ValueError('contains needs the compiled law the result was made for, open')
        u, leaf, _, _ = self._law.evaluate(X, return_info=True)
        row = _leaf_rows(self._law, leaf)
        ok = np.isfinite(u).all(axis=1) & (row < self.limit.size)
        row = np.minimum(row, self.limit.size - 1)
        if k is None or int(k) >= self.settle:
            return self.limit[row] & ok
        if int(k) < 0:
            raise ValueError('k must be >= 0')
        # D_j holds the closure's leaves that have not departed by j
        return self.closure[row] & ((self.depart[row] < 0) | (self.depart[row] > int(k))) & ok


def _start_rows(n_leaf, start):
    """int32 rows of a start set given as a bool mask [n_leaf] or as int rows; nonempty."""
    s = np.asarray(start)
    if s.dtype == np.bool_:
        if s.shape != (n_leaf,):
            raise ValueError('a start mask must be [%d] (one entry per leaf)' % n_leaf)
        rows = np.nonzero(s)[0]
    else:
        if s.ndim != 1 or (s.size and s.dtype.kind not in 'iu'):
            raise ValueError('start must be a bool mask or a 1-d array of leaf rows')
        rows = s
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= n_leaf):
            raise ValueError('start rows must lie in 0 .. %d' % (n_leaf - 1))
    if rows.size == 0:
        raise ValueError('the start set is empty')
    return np.ascontiguousarray(rows, dtype=np.int32)


def reach_relation(law, indptr, indices, level, start, horizon=0, max_sweeps=None,
                   return_steps=False, row_map=None):
    """
    The one path to ``ehm_compiled_reach``: the reach tube, limit set and step sets (DESIGN.md
    3.8l) of any relation over the first ``n = len(indptr) - 1`` leaf records of ``law``, as CSR
    (``indptr`` [n + 1], ``indices``), with ``level`` [n] (0: a seed, absorbing) and ``start`` (a
    bool mask [n] or int rows).  ``horizon``: the step sets R_0 .. R_horizon (cut at the leak);
    ``max_sweeps`` (None: n) bounds each phase; ``return_steps``: the step sets as masks, needs
    (horizon + 1) n <= 2^28; ``row_map``: ``'thread'`` or ``'wave'`` (None: ``ROW_MAP``), how the
    device walks a row -- no result depends on it.  Returns a ``ReachResult`` whose ``holds`` is
    False and whose volume fractions are those of the law's cells: ``CoreResult.reach`` fills in
    what the core knows.
    """
    from . import applied
    if not getattr(law, '_handle', None):
        raise ValueError('the law is closed')
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    level = np.ascontiguousarray(level, dtype=np.int32)
    if indptr.ndim != 1 or indptr.size < 2 or indices.ndim != 1 or level.ndim != 1:
        raise ValueError('indptr [n + 1] with n >= 1, indices and level must be 1-d')
    n = indptr.size - 1
    if n > law._h['n_leaf']:
        raise ValueError('a relation over %d leaves, the law has %d' % (n, law._h['n_leaf']))
    if level.size != n:
        raise ValueError('level must be [%d] (one entry per leaf)' % n)
    rows = _start_rows(n, start)
    horizon = int(horizon)
    max_sweeps = n if max_sweeps is None else int(max_sweeps)
    if horizon < 0:
        raise ValueError('horizon must be >= 0')
    if max_sweeps < 1:
        raise ValueError('max_sweeps must be >= 1')
    if return_steps and (horizon + 1) * n > MAX_STEP_BYTES:
        raise ValueError('return_steps needs (horizon + 1) * n_leaf <= 2^28')
    row_map = ROW_MAP if row_map is None else row_map
    if row_map not in _capi.EHM_REACH_MAPS:
        raise ValueError("row_map must be 'thread' or 'wave'")
    if law._h['n_test'] > 0:
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its cells do '
                             "not follow from its planes -- compile(spine='roots') has none" %
                             law._h['n_test'])
    if law._root_cells is None:
        law._root_cells = applied.root_cells(law)
    roots = law._root_cells
    p = law.p
    cap = min(max_sweeps, n) + 1
    out = dict(arrival=np.empty(n, np.int32), depart=np.empty(n, np.int32),
               limit=np.empty(n, np.uint8),
               steps=np.empty((horizon + 1, n), np.uint8) if return_steps else None,
               leaf_box=np.empty((2, p, n)), tube_box=np.empty((cap, 2, p)),
               tube_count=np.empty(cap, np.int64), settle_box=np.empty((cap, 2, p)),
               settle_count=np.empty(cap, np.int64), step_box=np.empty((horizon + 1, 2, p)),
               step_count=np.empty(horizon + 1, np.int64))
    opts = _capi.ReachOpts(root_vertices=ptr(roots['vertices']), indptr=ptr(indptr),
                           indices=ptr(indices), level=ptr(level), start=ptr(rows), n_leaf=n,
                           n_edges=indices.size, n_level=level.size, n_start=rows.size,
                           max_sweeps=max_sweeps, horizon=horizon,
                           want_steps=int(bool(return_steps)),
                           row_map=_capi.EHM_REACH_MAPS[row_map])
    lv = _capi.ReachLeaves(**{k: ptr(a) for k, a in out.items()})
    res = _capi.ReachResult()
    _check_reach(_capi.load().ehm_compiled_reach(law._handle, ctypes.byref(opts),
                                                 ctypes.byref(res), ctypes.byref(lv)))
    n_arrival, settle, n_steps = int(res.n_arrival), int(res.settle), int(res.n_steps)
    leak = int(res.leak_step)
    ran_b = bool(res.arrival_done) and leak < 0
    done_b = ran_b and bool(res.settle_done)
    arrival = out['arrival']
    closure = arrival >= 0
    last = out['limit'].astype(bool)
    settle_box = out['settle_box'][:settle + 1].copy() if ran_b else None
    # the volumes: |det| of the cells' edge matrices over p!, against the roots'
    lo, hi = out['leaf_box']
    has = np.isfinite(lo).all(axis=0)
    frac = lambda mask: None
    total = float(roots['volume'].sum())
    if n == law._h['n_leaf']:
        V = law.cells().vertices
        det = np.zeros(n)
        det[has] = np.abs(np.linalg.det(V[has][:, 1:] - V[has][:, :1]))
        fact = float(np.prod(np.arange(1, p + 1)))
        frac = lambda mask: float(det[mask].sum()) / fact / total
    return ReachResult(
        arrival=arrival, closure=closure, n_arrival=n_arrival, leak_step=leak, safe=leak < 0,
        limit=last if done_b else None, limit_outer=last if ran_b and not done_b else None,
        depart=out['depart'], settle=settle if ran_b else None,
        tube_box=out['tube_box'][:n_arrival + 1].copy(),
        tube_count=out['tube_count'][:n_arrival + 1].copy(), settle_box=settle_box,
        settle_count=out['settle_count'][:settle + 1].copy() if ran_b else None,
        limit_box=settle_box[-1] if ran_b else None,
        step_box=out['step_box'][:n_steps].copy(), step_count=out['step_count'][:n_steps].copy(),
        steps=out['steps'][:n_steps].copy() if return_steps else None,
        leaf_box=np.ascontiguousarray(np.transpose(out['leaf_box'], (2, 0, 1))),
        closure_volume_fraction=frac(closure),
        limit_volume_fraction=frac(last) if done_b else None,
        converged=bool(res.arrival_done) and (done_b or not ran_b), holds=False,
        horizon=horizon, max_sweeps=max_sweeps, row_map=row_map, n_outside=0,
        sweeps_arrival=int(res.sweeps_arrival), sweeps_settle=int(res.sweeps_settle),
        seconds_boxes=float(res.seconds_boxes), seconds_arrival=float(res.seconds_arrival),
        seconds_settle=float(res.seconds_settle), seconds_steps=float(res.seconds_steps),
        seconds_upload=float(res.seconds_upload), _law=law)


def _core_reach(self, start=None, X0=None, horizon=0, max_sweeps=None, return_steps=False,
                row_map=None):
    """
    Where does the closed loop go from ``start``?  The forward analysis of the
    relation this result holds (it must have been made with ``return_edges=True``): the leaves
    reachable step by step with their bounding boxes, the first step a seed can be reached
    (``leak_step``), and, when none can, the limit set the loop settles into and its box.

    ``start``: a bool mask or int rows of the leaf records; or ``X0`` [n, p]: the leaves ``evaluate``
    returns for those states, located as ``contains`` locates them (states without an input are
    counted in ``n_outside`` and left out); neither: all core leaves.  ``horizon``, ``max_sweeps``,
    ``return_steps``, ``row_map`` as ``reach_relation``.  ``ValueError`` for both ``start`` and ``X0``,
    an empty start, a result without edges and a closed law.  Returns a ``ReachResult``; every
    statement holds under the assumptions and exclusions of the core that made the relation.
    """
    law = getattr(self, '_law', None)
    if self.indptr is None or self.indices is None:
        raise ValueError('reach needs the relation: make the core with return_edges=True')
    if start is not None and X0 is not None:
        raise ValueError('give start or X0, not both')
    if law is None or not getattr(law, '_handle', None):
        raise ValueError('reach needs the compiled law the result was made for: the law is closed')
    n_outside = 0
    if X0 is not None:
        X0 = np.ascontiguousarray(X0, dtype=np.float64)
        u, leaf, _, _ = law.evaluate(X0, return_info=True)
        ok = np.isfinite(u).all(axis=1)
        n_outside = int((~ok).sum())
        start = np.unique(_leaf_rows(law, leaf[ok])).astype(np.int32)
    elif start is None:
        start = self.core
    out = reach_relation(law, self.indptr, self.indices, self.level, start, horizon=horizon,
                         max_sweeps=max_sweeps, return_steps=return_steps, row_map=row_map)
    out.n_outside = n_outside
    out.set_convex = bool(self.set_convex)
    out.holds = bool(self.set_convex and out.safe and out.converged)
    return out


CoreResult.reach = _core_reach


# -- certified fuel bounds of the closed loop (csrc/ehm_cost.hip) ---------------------

_check_cost = _capi.checker('ehm_cost_last_error')
MAX_PATH_BYTES = 1 << 28        # horizon n_leaf 4 of ``return_paths``, per direction
COST_MAX_NU = 4                 # the inputs a rollout steps


class CostResult:
    """
    What ``CoreResult.cost`` / ``cost_relation`` found: bounds of the summed input
    2-norm (``u_norm_sum`` of a rollout) of every trajectory that stays in the domain D.

    Per leaf, NaN outside D: ``w_hi``, ``w_lo`` (the largest and smallest 2-norm of the commanded
    input on the leaf's cell, widened by ``pad``, the rounding of the law's evaluation), ``hi`` = U_H
    and ``lo`` = L_H, the bounds over ``horizon`` steps from the leaf.  Per step k = 0 .. H:
    ``max_hi``, ``min_lo`` over D, ``start_hi``, ``start_lo`` over the start set, ``rate_hi`` =
    ``max_hi[k] / k`` and ``rate_lo`` = ``min_lo[k] / k`` (NaN at k = 0).  ``best_rate_hi`` = min_k
    rate_hi at ``best_k_hi``, ``best_rate_lo`` = max_k rate_lo at ``best_k_lo``: every window of K
    steps spends at most K rate_hi[K], so the long-run spend per step lies in [best_rate_lo,
    best_rate_hi].  With ``return_paths``: ``path_hi``, ``path_lo`` int32 [H + 1], the leaves a
    worst and a best path visits (-1 after a leaf with an empty row).  ``holds``: the core's set
    is convex.  ``n_domain``, ``n_start``; ``seconds_weights``, ``seconds_sweeps`` (device time)
    and ``seconds_upload`` (wall time of checking and uploading the relation).
    """

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'CostResult(n_domain=%d, n_start=%d, horizon=%d, start=[%.6g, %.6g], ' \
            'rate=[%.6g (k=%d), %.6g (k=%d)], holds=%s)' % (
                self.n_domain, self.n_start, self.horizon, self.start_lo[-1], self.start_hi[-1],
                self.best_rate_lo, self.best_k_lo, self.best_rate_hi, self.best_k_hi, self.holds)


def _set_rows(n_leaf, rows, what):
    """``_start_rows`` for the set called ``what``."""
    try:
        return _start_rows(n_leaf, rows)
    except ValueError as e:
        raise ValueError(str(e).replace('start', what)) from None


def cost_relation(law, indptr, indices, level, domain, start=None, horizon=64, w_hi=None,
                  w_lo=None, return_paths=False):
    """
    The one path to ``ehm_compiled_cost``: certified bounds of the summed input 2-norm over k = 0 ..
    ``horizon`` steps on the relation over the first ``n = len(indptr) - 1`` leaf
    records of ``law``, as ``reach_relation`` takes it.  ``domain`` (a bool mask [n] or int rows)
    must hold no seed (``level == 0``) and be closed under the relation -- the device checks both and
    ``EhmError`` names the first row that fails --; ``start`` (None: the domain) lies in it.  The
    weights come from the law's cells and maps (a domain leaf without a cell is refused) unless
    ``w_hi`` and ``w_lo`` [n] are both given: any per-leaf cost, finite with ``w_lo <= w_hi`` on the
    domain.  ``return_paths`` needs horizon * n * 4 <= 2^28.  Returns a ``CostResult`` whose
    ``holds`` is False: ``CoreResult.cost`` fills in what the core knows.
    """
    from . import applied
    if not getattr(law, '_handle', None):
        raise ValueError('the law is closed')
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    level = np.ascontiguousarray(level, dtype=np.int32)
    if indptr.ndim != 1 or indptr.size < 2 or indices.ndim != 1 or level.ndim != 1:
        raise ValueError('indptr [n + 1] with n >= 1, indices and level must be 1-d')
    n = indptr.size - 1
    if n > law._h['n_leaf']:
        raise ValueError('a relation over %d leaves, the law has %d' % (n, law._h['n_leaf']))
    if level.size != n:
        raise ValueError('level must be [%d] (one entry per leaf)' % n)
    dom = _set_rows(n, domain, 'domain')
    rows = dom if start is None else _set_rows(n, start, 'start')
    if not np.isin(rows, dom).all():
        raise ValueError('the start set must lie in the domain: row %d does not'
                         % int(rows[~np.isin(rows, dom)][0]))
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError('horizon must be >= 1')
    if (w_hi is None) != (w_lo is None):
        raise ValueError('give both w_hi and w_lo, or neither')
    if return_paths and horizon * n * 4 > MAX_PATH_BYTES:
        raise ValueError('return_paths needs horizon * n_leaf * 4 <= 2^28')
    if w_hi is not None:
        w_hi = np.ascontiguousarray(w_hi, dtype=np.float64)
        w_lo = np.ascontiguousarray(w_lo, dtype=np.float64)
        if w_hi.shape != (n,) or w_lo.shape != (n,):
            raise ValueError('w_hi and w_lo must be [%d] (one entry per leaf)' % n)
        if not (np.isfinite(w_hi[dom]).all() and np.isfinite(w_lo[dom]).all()):
            raise ValueError('w_hi and w_lo must be finite on the domain')
        if (w_lo[dom] > w_hi[dom]).any():
            raise ValueError('w_lo <= w_hi must hold on the domain')
    if law._h['n_test'] > 0:
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its cells do '
                             "not follow from its planes -- compile(spine='roots') has none" %
                             law._h['n_test'])
    if law.n_u > COST_MAX_NU:
        raise ValueError('cost bounds at most %d inputs, the law has %d' % (COST_MAX_NU, law.n_u))
    if law._root_cells is None:
        law._root_cells = applied.root_cells(law)
    roots = law._root_cells
    out = dict(w_hi=np.empty(n), w_lo=np.empty(n), pad=np.empty(n), hi=np.empty(n),
               lo=np.empty(n), max_hi=np.empty(horizon + 1), min_lo=np.empty(horizon + 1),
               start_hi=np.empty(horizon + 1), start_lo=np.empty(horizon + 1),
               path_hi=np.empty(horizon + 1, np.int32) if return_paths else None,
               path_lo=np.empty(horizon + 1, np.int32) if return_paths else None)
    opts = _capi.CostOpts(root_vertices=ptr(roots['vertices']), indptr=ptr(indptr),
                          indices=ptr(indices), level=ptr(level), domain=ptr(dom),
                          start=ptr(rows), w_hi=ptr(w_hi), w_lo=ptr(w_lo), n_leaf=n,
                          n_edges=indices.size, n_level=level.size, n_domain=dom.size,
                          n_start=rows.size, horizon=horizon, want_paths=int(bool(return_paths)))
    lv = _capi.CostLeaves(**{k: ptr(a) for k, a in out.items()})
    res = _capi.CostResult()
    _check_cost(_capi.load().ehm_compiled_cost(law._handle, ctypes.byref(opts),
                                               ctypes.byref(res), ctypes.byref(lv)))
    k = np.arange(horizon + 1, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        rate_hi, rate_lo = out['max_hi'] / k, out['min_lo'] / k
    rate_hi[0] = rate_lo[0] = np.nan
    best_k_hi = 1 + int(np.argmin(rate_hi[1:]))
    best_k_lo = 1 + int(np.argmax(rate_lo[1:]))
    return CostResult(
        rate_hi=rate_hi, rate_lo=rate_lo, best_rate_hi=float(rate_hi[best_k_hi]),
        best_k_hi=best_k_hi, best_rate_lo=float(rate_lo[best_k_lo]), best_k_lo=best_k_lo,
        holds=False, horizon=horizon, n_domain=int(res.n_domain), n_start=int(res.n_start),
        domain=dom, start=rows, seconds_weights=float(res.seconds_weights),
        seconds_sweeps=float(res.seconds_sweeps), seconds_upload=float(res.seconds_upload),
        _law=law, **out)


def _core_cost(self, domain=None, start=None, X0=None, horizon=64, w_hi=None, w_lo=None,
               return_paths=False):
    """
    What can the closed loop spend while it stays in ``domain``?  Certified bounds
    of the summed input 2-norm over the relation this result holds (it must have been made with
    ``return_edges=True``).  ``domain``: a bool mask or int rows, a set without a seed that the
    relation does not leave (the core, a safe closure, every D_j and the limit set of ``reach``);
    None: the core.  ``start``: a subset of it, or ``X0`` [n, p], located as ``reach`` locates it;
    neither: the domain.  ``horizon``, ``w_hi``, ``w_lo``, ``return_paths`` as ``cost_relation``.
    ``ValueError`` for both ``start`` and ``X0``, an empty set, a start outside the domain, a result
    without edges and a closed law.  Returns a ``CostResult``; every statement holds under the
    assumptions and exclusions of the core that made the relation.
    """
    law = getattr(self, '_law', None)
    if self.indptr is None or self.indices is None:
        raise ValueError('cost needs the relation: make the core with return_edges=True')
    if start is not None and X0 is not None:
        raise ValueError('give start or X0, not both')
    if law is None or not getattr(law, '_handle', None):
        raise ValueError('cost needs the compiled law the result was made for: the law is closed')
    n_outside = 0
    if X0 is not None:
        X0 = np.ascontiguousarray(X0, dtype=np.float64)
        u, leaf, _, _ = law.evaluate(X0, return_info=True)
        ok = np.isfinite(u).all(axis=1)
        n_outside = int((~ok).sum())
        start = np.unique(_leaf_rows(law, leaf[ok])).astype(np.int32)
    out = cost_relation(law, self.indptr, self.indices, self.level,
                        self.core if domain is None else domain, start=start, horizon=horizon,
                        w_hi=w_hi, w_lo=w_lo, return_paths=return_paths)
    out.n_outside = n_outside
    out.set_convex = bool(self.set_convex)
    out.holds = bool(self.set_convex)
    return out


CoreResult.cost = _core_cost


def _reach_cost(self, core, which='limit', **kw):
    """``core.cost`` on a set this result found: ``which`` = ``'limit'`` (the limit set) or
    ``'closure'``; the run must be safe (and, for the limit set, converged).  ``core``: the
    ``CoreResult`` whose relation the reach was made over; the other arguments as
    ``CoreResult.cost``."""
    if which not in ('limit', 'closure'):
        raise ValueError("which must be 'limit' or 'closure'")
    if not self.safe:
        raise ValueError('the run leaks: the closure holds a seed')
    domain = self.limit if which == 'limit' else self.closure
    if domain is None:
        raise ValueError('no limit set: the run did not converge')
    return core.cost(domain=domain, **kw)


ReachResult.cost = _reach_cost
