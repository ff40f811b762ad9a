"""
Invariance of a compiled law under process, measurement and input error (DESIGN.md 3.8j,
csrc/ehm_robust.hip; the relation by csrc/ehm_core.hip):

    res = law.robust_successors(d_box=(lo, hi), v_box=(lo, hi), e_box=(lo, hi))
    res = law.robust_successors(noise=NoiseModel.from_mpc(mpc))     # boxes from the model
    res.status, res.margin, res.worst, res.counts, res.boxes, res.holds_on_set
    core = law.robust_core(noise=model)                             # an invariance.CoreResult
    res = law.robust_successors(noise=model, radii='leaf')          # a box per leaf (3.8k)
    res.leaf_boxes, res.x_abs_leaf, res.x_next_abs, res.u_abs_leaf

The argument.  The noisy closed loop (``rollout(..., noise=)``) evaluates the law at the measured
state z = x + v, tests the region of the leaf's mode m on the true state x = z - v and steps the plant
with u + e.  For z in the cell of a leaf the measured successor is

    z+ = [A_m z + B_m u(z) + w_m] + E d - A_m v + B_m e + v'         (v' the next step's error),

affine in (z, d, v, e, v'), so its image under every error of the boxes is hull{y_i} + G_m [g_lo, g_hi]
with the p + 1 nominal vertex successors y_i, G_m = [E | -A_m | B_m | I] and the box [d; v; e; v].
Where the set -- the union of the roots -- is convex it is the intersection of the half-spaces of its
boundary facets (``invariance.boundary_facets``), and the minimum of a facet's form over the image
is closed-form: no corner is enumerated, so 64 generators cost as much per facet as one.  A leaf is
``invariant`` when that minimum is >= -tol_set max|root vertex| for every facet and every region row
of its mode holds on cell - v box; ``margin`` is the smallest such minimum, a distance in state
units.  The v and e boxes must hold 0: v_0 = 0, and e = 0 where u = 0, are draws too.

What a core leaf promises, where the set is convex: every trajectory of the noisy closed loop from a
state of it has, for any errors of the boxes and at every length, every measured state in the set
and in a core leaf, every true state in its mode's region and within the v box of the set.  Not
covered: the rounding of a single law's evaluation at interior points, the hand-over within rounding
of a split face, the recovery error of the root vertices, guarded plants (refused).

Per-leaf radii (``radii='leaf'``).  With ``noise=`` the boxes above are
``noise.bounding_boxes`` at one global bound, so a state-dependent radius is taken at the set's corner
for every leaf.  The rollout draws v_t at the true state x_t and the last input u_(t-1), e_t and d_t at
x_t and u_t = u(z_t), v_(t+1) at x_(t+1) and u_t.  For z_t in the cell of leaf L: |x_t| <= a_L, found
by ``radius_iters`` steps of a <- min(a, c_L + vhalf(a, u_abs)) from the global x_abs (every iterate
is a valid bound by monotonicity alone); |u_t| <= ubar_L, the largest vertex input modulus of L;
|x_(t+1)| <= a'_L = min(x_abs, max_i |y_i| + |E| dmax_L + |A_m| vmax_L + |B_m| emax_L).  So
v_L = box_state(a_L, u_abs), e_L = box_input(a_L, ubar_L), d_L = box_process(a_L, ubar_L),
v'_L = box_state(a'_L, ubar_L), and the image of L is hull{y_i} + G_m [d_L; v_L; e_L; v'_L].  The device
makes the boxes from the packed model the rollout uses; statuses, margins and the core's promises are
the ones above, read leaf by leaf.
"""

import ctypes

import numpy as np

from . import _capi, invariance
from . import noise as noise_mod
from ._capi import ptr

MAX_G = 64                      # EHM_ROB_MAX_G: generators n_d + 2 p + n_u
RADII = ('global', 'leaf')
MAX_RADIUS_ITERS = 16           # EHM_RAD_MAX_ITERS

_check = _capi.checker('ehm_robust_last_error')


class RobustSuccessorResult:
    """
    What ``CompiledLaw.robust_successors`` found: ``n`` leaves asked for, ``counts``
    by status name (``invariance.STATUS_NAMES``); per leaf ``leaves``, ``leaf_node``, ``status``
    int32, ``margin`` (the smallest minimum of any boundary facet's form over the leaf's image, in
    state units, no threshold applied; NaN without a cell or mode), ``worst`` = f (p + 1) + i, the
    facet and the vertex that give it; ``invariant_volume_fraction`` and ``cell_volume_fraction``
    over the roots' volume; ``worst_leaf`` (dict of leaf, leaf_node, margin; None),
    ``worst_margin``; ``seconds`` of the kernel, ``seconds_slack`` of the facet-by-mode table;
    ``n_facets``, ``n_generators``; ``boxes``: the dict of (lo, hi) by kind that was certified
    ('process', 'state', 'input'; None for a kind without a box), and with ``noise=`` the global
    bounds they were made from, ``x_abs`` and ``u_abs`` (else None); ``radii`` ('global' or 'leaf');
    with ``radii='leaf'`` ``leaf_boxes``, a dict with 'process', 'state', 'input'
    and 'state_next', each [n, 2, dim] (lo, hi per requested leaf; None for a kind without terms; NaN
    for a leaf without a cell or mode), ``x_abs_leaf`` [n, p] (a_L), ``x_next_abs`` [n, p] (a'_L),
    ``u_abs_leaf`` [n, n_u] (ubar_L), ``radius_iters``, ``seconds_radii`` -- ``boxes``, ``x_abs`` and
    ``u_abs`` stay the global ones the iteration starts from -- else all None; ``set_convex``;
    ``holds_on_set``: every requested leaf is invariant, every leaf was requested, and the set is
    convex.  Without a convex set the facets bound nothing and ``invariant`` proves nothing.
    """

    radii = 'global'
    leaf_boxes = x_abs_leaf = x_next_abs = u_abs_leaf = radius_iters = seconds_radii = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return 'RobustSuccessorResult(n=%d, radii=%r, counts=%r, invariant_volume_fraction=%.6g, ' \
            'worst_margin=%.3g, n_generators=%d, set_convex=%s, holds_on_set=%s)' % (
                self.n, self.radii, self.counts, self.invariant_volume_fraction,
                self.worst_margin, self.n_generators, self.set_convex, self.holds_on_set)


def _pair(box, size, name, holds_zero):
    """(lo, hi) float64 [size] of ``box`` = (lo, hi), finite with lo <= hi (and lo <= 0 <= hi)."""
    try:
        lo, hi = box
    except (TypeError, ValueError):
        raise ValueError('%s must be (lo, hi)' % name)
    lo = np.ascontiguousarray(np.atleast_1d(lo), dtype=np.float64)
    hi = np.ascontiguousarray(np.atleast_1d(hi), dtype=np.float64)
    if lo.shape != (size,) or hi.shape != (size,):
        raise ValueError('%s must be two arrays [%d]' % (name, size))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise ValueError('%s must be finite with lo <= hi' % name)
    if holds_zero and not ((lo <= 0.).all() and (hi >= 0.).all()):
        raise ValueError('%s must hold 0: the first measurement has no error, and an input of 0 '
                         'has none' % name)
    return lo, hi


def _radii_args(radii, radius_iters, noise, d_box, v_box, e_box):
    """(radii, radius_iters) checked; what ``radii='leaf'`` refuses needs no law."""
    if radii not in RADII:
        raise ValueError("radii must be 'global' or 'leaf', not %r" % (radii,))
    try:
        iters = int(radius_iters)
        whole = iters == radius_iters
    except (TypeError, ValueError):
        whole = False
    if not whole or not 1 <= iters <= MAX_RADIUS_ITERS:
        raise ValueError('radius_iters must be an integer in 1..%d, not %r' % (MAX_RADIUS_ITERS,
                                                                               radius_iters))
    if radii == 'leaf':
        if noise is None:
            raise ValueError("radii='leaf' makes the boxes of every leaf from a model: give noise=")
        if not (d_box is None and v_box is None and e_box is None):
            raise ValueError("radii='leaf' makes the boxes of every leaf from the model: give no "
                             'boxes')
        const = noise_mod.bounding_boxes(noise, np.zeros(noise.n_x), np.zeros(noise.n_u))
        for kind, name in (('state', 'v'), ('input', 'e')):
            lo, hi = const[kind]
            if not ((lo <= 0.).all() and (hi >= 0.).all()):
                raise ValueError("radii='leaf': the constant part of the %s box must hold 0 (a "
                                 "leaf's box is a subset of the global one): [%s, %s]" % (name, lo,
                                                                                          hi))
    return radii, iters


class _RobustStep(invariance._Step):
    """``invariance._Step`` with the three boxes resolved: ``boxes`` (dict by kind of (lo, hi) or
    None), ``x_abs`` / ``u_abs`` (with ``noise=``), ``tol_set``, and ``robust_opts()``."""

    def __init__(self, law, plant, d_box, v_box, e_box, noise, tol_exit, tol_set, chunk=0,
                 radii='global', radius_iters=3):
        self.radii, self.radius_iters = _radii_args(radii, radius_iters, noise, d_box, v_box, e_box)
        self.noise = noise
        if noise is not None and not (d_box is None and v_box is None and e_box is None):
            raise ValueError('noise= fills all three boxes: give it or boxes, not both')
        self.tol_set = float(tol_set)
        if not self.tol_set >= 0.:
            raise ValueError('tol_set must be >= 0')
        self._given = (v_box, e_box)
        self.x_abs = self.u_abs = None
        super().__init__(law, plant, d_box, tol_exit, chunk)
        if noise is not None:
            plant, p, n_u = self.plant, law.p, law.n_u
            if (noise.n_x, noise.n_u, noise.n_d) != (p, n_u, plant.n_d):
                raise ValueError('the noise model (n_x %d, n_u %d, n_d %d) does not fit the plant '
                                 '(%d, %d, %d)' % (noise.n_x, noise.n_u, noise.n_d, p, n_u,
                                                   plant.n_d))
            # |u_c| is convex on a cell, so its maximum over the law is at a cell vertex
            inputs = law.cells().inputs
            self.u_abs = np.nanmax(np.abs(inputs.reshape(-1, n_u)), axis=0)
            set_abs = np.abs(self.roots['vertices'].reshape(-1, p)).max(axis=0)
            self.x_abs = noise_mod.state_bound(noise, set_abs, self.u_abs)
            bb = noise_mod.bounding_boxes(noise, self.x_abs, self.u_abs)
            self._given = (bb['state'], bb['input'])
            self._set_box(bb['process'] if plant.n_d else None)
        normals, offsets, _ = self.facets
        self.facet_rows = np.ascontiguousarray(np.hstack([normals, offsets[:, None]]),
                                               dtype=np.float64)

    def _set_box(self, d_box):
        """The three boxes checked: ``boxes``, ``lo`` / ``hi`` / ``n_d`` of d, ``n_g``."""
        plant, (v_box, e_box) = self.plant, self._given
        p, n_u = plant.n_x, plant.n_u
        self.boxes = dict(
            process=None if d_box is None else _pair(d_box, plant.n_d, 'd_box', False),
            state=None if v_box is None else _pair(v_box, p, 'v_box', True),
            input=None if e_box is None else _pair(e_box, n_u, 'e_box', True))
        self.lo, self.hi = self.boxes['process'] or (None, None)
        self.n_d = 0 if self.lo is None else plant.n_d
        self.n_g = self.n_d + (2 * p if v_box is not None else 0) + \
            (n_u if e_box is not None else 0)
        if self.n_g > MAX_G:
            raise ValueError('%d generators (n_d + 2 p + n_u), at most %d' % (self.n_g, MAX_G))

    def radii_opts(self):
        """The ``RobustRadii`` of ``radii='leaf'``: the packed model, the global bounds, the
        iterations.  The arrays live as long as this object."""
        desc, data = self.noise.pack()
        self._packed = (np.ascontiguousarray(desc, dtype=np.int32),
                        np.ascontiguousarray(data, dtype=np.float64),
                        np.ascontiguousarray(self.x_abs, dtype=np.float64),
                        np.ascontiguousarray(self.u_abs, dtype=np.float64))
        desc, data, x_abs, u_abs = self._packed
        return _capi.RobustRadii(
            desc=ptr(desc) if desc.size else None, data=ptr(data) if data.size else None,
            x_abs=ptr(x_abs), u_abs=ptr(u_abs), n_terms=int(desc.shape[0]), n_data=int(data.size),
            n_x=self.noise.n_x, n_u=self.noise.n_u, n_d=self.noise.n_d,
            radius_iters=self.radius_iters)

    def robust_opts(self):
        v, e = self.boxes['state'], self.boxes['input']
        return _capi.RobustOpts(
            facets=ptr(self.facet_rows) if self.facet_rows.size else None,
            n_facets=self.facet_rows.shape[0],
            v_lo=None if v is None else ptr(v[0]), v_hi=None if v is None else ptr(v[1]),
            e_lo=None if e is None else ptr(e[0]), e_hi=None if e is None else ptr(e[1]),
            tol_set=self.tol_set)


def robust_successors(law, plant=None, d_box=None, v_box=None, e_box=None, noise=None, leaves=None,
                      tol_exit=1e-9, tol_set=1e-9, chunk=0, radii='global', radius_iters=3):
    """The one path to ``ehm_compiled_robust_successors`` and its per-leaf form; see
    ``CompiledLaw.robust_successors``."""
    _radii_args(radii, radius_iters, noise, d_box, v_box, e_box)
    return _robust_successors(law, _RobustStep(law, plant, d_box, v_box, e_box, noise, tol_exit,
                                               tol_set, chunk, radii, radius_iters), leaves)


def _robust_successors(law, st, leaves):
    from . import certify
    ids = certify._leaf_ids(law, leaves)
    n = ids.size
    opt = lambda a: ptr(a) if a.size else None
    opts = st.opts(n=n, leaf_ids=None if leaves is None else ptr(ids), chunk=st.chunk,
                   region_rows=ptr(st.rows), H=opt(st.H), h=opt(st.h), n_g=0)
    ro = st.robust_opts()
    arrays = dict(status=np.empty(n, np.int32), margin=np.empty(n), worst=np.empty(n, np.int32))
    lv = _capi.RobustLeaves(**{k: ptr(a) for k, a in arrays.items()})
    res = _capi.RobustResult()
    leaf = {}
    if st.radii == 'leaf':
        p, n_u, model = law.p, law.n_u, st.noise
        has = {k: any(t.kind == k for t in model.terms) for k in noise_mod.KINDS}
        has['process'] = has['process'] and st.plant.n_d > 0
        boxes = dict(process=np.empty((n, 2, st.plant.n_d)) if has['process'] else None,
                     state=np.empty((n, 2, p)) if has['state'] else None,
                     input=np.empty((n, 2, n_u)) if has['input'] else None,
                     state_next=np.empty((n, 2, p)) if has['state'] else None)
        leaf = dict(leaf_boxes=boxes, x_abs_leaf=np.empty((n, p)), x_next_abs=np.empty((n, p)),
                    u_abs_leaf=np.empty((n, n_u)))
        lb = _capi.RobustLeafBoxes(
            d=ptr(boxes['process']), v=ptr(boxes['state']), e=ptr(boxes['input']),
            v_next=ptr(boxes['state_next']), x_abs_leaf=ptr(leaf['x_abs_leaf']),
            x_next_abs=ptr(leaf['x_next_abs']), u_abs_leaf=ptr(leaf['u_abs_leaf']))
        rr = st.radii_opts()
        _check(_capi.load().ehm_compiled_robust_successors_leaf(
            law._handle, ctypes.byref(opts), ctypes.byref(ro), ctypes.byref(rr), ctypes.byref(res),
            ctypes.byref(lv), ctypes.byref(lb)))
        leaf.update(radius_iters=st.radius_iters, seconds_radii=float(lb.seconds_radii))
    else:
        _check(_capi.load().ehm_compiled_robust_successors(
            law._handle, ctypes.byref(opts), ctypes.byref(ro), ctypes.byref(res),
            ctypes.byref(lv)))
    total = float(st.roots['volume'].sum())
    counts = {name: int(res.counts[k]) for k, name in enumerate(invariance.STATUS_NAMES)}
    worst = None
    if res.worst_leaf >= 0:
        l = int(ids[res.worst_leaf])
        worst = dict(leaf=l, leaf_node=int(law.leaf_node[l]), margin=float(res.worst_margin))
    every = n >= law._h['n_leaf'] and np.unique(ids).size == law._h['n_leaf']
    return RobustSuccessorResult(
        n=n, counts=counts, leaves=ids, leaf_node=law.leaf_node[ids],
        invariant_volume_fraction=float(res.invariant_volume) / total,
        cell_volume_fraction=float(res.cell_volume) / total, worst_leaf=worst,
        worst_margin=float(res.worst_margin), seconds=float(res.seconds),
        seconds_slack=float(res.seconds_slack), n_facets=int(st.facet_rows.shape[0]),
        n_generators=int(res.n_generators), boxes=st.boxes, x_abs=st.x_abs, u_abs=st.u_abs,
        set_convex=st.set_convex, tol_exit=st.tol_exit, tol_set=st.tol_set, radii=st.radii,
        holds_on_set=bool(counts['invariant'] == n and every and st.set_convex), **arrays, **leaf)


def robust_core(law, plant=None, d_box=None, v_box=None, e_box=None, noise=None, tol_exit=1e-9,
                tol_set=1e-9, tol_side=None, rows='invariant', return_edges=False,
                max_fan=invariance.MAX_FAN, max_edges=invariance.MAX_EDGES, radii='global',
                radius_iters=3):
    """The one path to ``ehm_compiled_robust_core`` and its per-leaf form; see
    ``CompiledLaw.robust_core``."""
    _radii_args(radii, radius_iters, noise, d_box, v_box, e_box)
    tol_side, max_fan, max_edges = invariance._core_args(tol_exit, tol_side, rows, max_fan,
                                                         max_edges)
    st = _RobustStep(law, plant, d_box, v_box, e_box, noise, tol_exit, tol_set, 0, radii,
                     radius_iters)
    seeds = _robust_successors(law, st, None)
    ro = st.robust_opts()
    if st.radii == 'leaf':
        rr = st.radii_opts()
        return invariance._core(
            law, st, seeds, tol_side, rows, return_edges, max_fan, max_edges,
            lambda lib, po, co, res, lv: lib.ehm_compiled_robust_core_leaf(
                law._handle, po, ctypes.byref(ro), ctypes.byref(rr), co, res, lv))
    return invariance._core(
        law, st, seeds, tol_side, rows, return_edges, max_fan, max_edges,
        lambda lib, po, co, res, lv: lib.ehm_compiled_robust_core(
            law._handle, po, ctypes.byref(ro), co, res, lv))
