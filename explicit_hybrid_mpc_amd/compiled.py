"""
The explicit law compiled for deployment (csrc/ehm_compiled.hip):

    law = ExplicitMPC(tree, oracle).compile()     # CompiledLaw, independent of its source
    u = law.evaluate(X)                           # as ExplicitMPC.evaluate
    res = law.rollout(X0, T, plant=plant)         # as ExplicitMPC.rollout, one kernel launch
    law.save('law.npz'); law = CompiledLaw.load('law.npz')

Every split of the partition is a bisection, so an internal node keeps one hyperplane (the split
face, p + 1 doubles) next to its two child indices instead of the child's p + p^2 record, and a
leaf keeps the affine map u = u_0 + K (x - v_0) instead of its vertex inputs.  Nodes whose
children are no bisection (the data-less spine of a nested reference tree) keep the reference's
containment test.

``rollout`` closes the loop around the compiled law on the device (k_compiled_rollout), also for a
law that was only ever loaded from a file.  A step measures z, chooses the root as ``evaluate``
does, stops with status 1 unless every barycentric weight of z in that root is >= -tol_exit,
walks the planes and applies the leaf's affine map -- (leaf, u) are ``evaluate(z)`` bit for bit --
and then steps the plant exactly as ``ExplicitMPC.rollout`` does.  Two differences from that
rollout: ``tol_exit`` is in units of the root's weights, not the leaf's (the statuses can differ
only for z within a tol_exit-wide band of the hull), and a state within rounding of a split face
may go to the sibling leaf, as it does in ``evaluate``.  The mode of a leaf comes from
``leaf_mode`` (``set_leaf_modes``; ``ExplicitMPC.compile`` attaches it, ``save`` / ``load`` keep
it): like the plant it is an attachment for rollouts, not part of the law.  Laws with test nodes
and laws with more than four inputs have no rollout.  No CPU fallback.

    single = law.to_single()                      # or ExplicitMPC.compile(dtype=np.float32)

is the same law with its internal and leaf records in single precision (``dtype`` np.float32), as a
flight computer holds it: a new, independent ``CompiledLaw`` with everything above.  The root is
still chosen in double on the double state (and the rollout's exit test made there), so both laws
choose the same root for every state; below it xs = (float) x, the plane sums and the leaf map run
in float, one rounding per product and per sum, left iff s >= -2^-23, and u is widened to double.
A turn can differ from the double law's only where |s| is within the rounding bound of the sum,
and in the same leaf the inputs differ by at most a like bound (DESIGN.md 3.8c states both).  Laws
with test nodes, and laws a value of which overflows or leaves the normal range of a float, have
no single form (``EhmError``, EHM_E_INVALID).  ``save`` marks the file with the key ``precision``.

Two options open both forms to the laws people hold (both off by default).  ``compile(spine='roots')``
turns the data-less right spine of a nested reference tree into the law's root table: the spine's
test nodes go, the simplices that hang off it become the roots (and get the locator from 128 on), so
the law has a rollout and a single form like one compiled from the flat forest, with the same
(u, leaf) as under the default.  ``to_single(flush=True)`` (``compile(dtype=np.float32, flush=True)``)
stores a value below the normal range of a float as +0.0 instead of refusing the law and counts
those in ``flushed``.

    res = law.audit(oracle, n=100000)             # applied.AppliedAuditResult

checks the law's contract at sampled states by what its input costs (applied.py): a
compiled law keeps no costs, so the input it applies is priced by P_theta with the first input
fixed to it, against P_theta itself.  For double and single laws, compiled here or only loaded.

    cells = law.cells()                           # certify.LeafCells

rebuilds the simplex of every leaf from the law's own arrays and gives the leaf's own map at its
vertices (certify.py): a compiled law keeps no vertices, and a statement that holds
on a whole leaf, where the audit speaks of samples, starts from them.

    res = law.certify(oracle)                     # certify.CertificateResult

is that statement: the contract of ``audit`` proved on every leaf the test can close, from the
costs of the vertex inputs (convexity of the fixed-commutation cost along the leaf's affine map).

    small = law.reduce()                          # or ExplicitMPC.compile(reduce=True)

merges the leaves that apply one affine map (csrc/ehm_reduce.hip): a new law of the
same precision and file format whose input is within ``tol`` of this law's at every state of
every cell of this law; ``small.reduction`` holds what it saved.

    fine = law.refine(levels=2, leaves=mask)      # or max_diameter=, max_spread=

goes the other way (csrc/ehm_refine.hip): the selected leaves are bisected as the
partitioner would have bisected their cells and both children keep the parent's record verbatim, so
the new law applies the same input bit for bit at every state while every leaf-by-leaf statement
(``certify``, ``successors``, ``invariant_core``, ``reach``, ``cost``) is made on smaller cells;
``fine.refinement`` holds what it did.
"""

import ctypes
import time

import numpy as np

from . import _capi
from ._capi import f64, ptr

FORMAT_VERSION = 1
HEADER = ('version', 'p', 'n_u', 'n_roots', 'n_int', 'n_leaf', 'n_test', 'node_stride',
          'leaf_stride', 'side_stride', 'has_nbr', 'n_source_nodes')
ARRAYS = ('node', 'leaf_rec', 'leaf_node', 'test_rec', 'root_rec', 'root_entry', 'nbr')
_INT_ARRAYS = ('leaf_node', 'root_entry', 'nbr')
_NARROWED = ('node', 'leaf_rec')        # float32 in a single law; everything else as in a double one


def node_stride32(p):
    """Floats of an internal record of a single law: [a (p) | b | left, right] rounded up to 32 B."""
    return 8 * ((p + 3 + 7) // 8)


def leaf_stride32(p, n_u):
    """Floats of a leaf record of a single law: [v_0 | u_0 | K] rounded up to 16 B."""
    return 4 * ((p + n_u + n_u * p + 3) // 4)


_check = _capi.checker('ehm_compiled_last_error')
_check_reduce = _capi.checker('ehm_reduce_last_error')
_check_refine = _capi.checker('ehm_refine_last_error')


def _shapes(h):
    """The shape of every array a header states."""
    return {'node': (h['n_int'], h['node_stride']), 'leaf_rec': (h['n_leaf'], h['leaf_stride']),
            'leaf_node': (h['n_leaf'],), 'test_rec': (h['n_test'], h['side_stride']),
            'root_rec': (h['n_roots'], h['side_stride']), 'root_entry': (h['n_roots'],),
            'nbr': (h['n_roots'] if h['has_nbr'] else 0, h['p'] + 1)}


def precision_of(arrays):
    """32 if ``arrays`` are a single law's (node and leaf_rec float32), else 64; ``EhmError`` if only
    one of the two is float32."""
    single = [np.asarray(arrays[k]).dtype == np.float32 for k in _NARROWED]
    if single[0] != single[1]:
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: node is %s, leaf_rec %s' % tuple(
            np.asarray(arrays[k]).dtype for k in _NARROWED))
    return 32 if single[0] else 64


def _marshal(arrays):
    """(header int64 [12], the seven arrays contiguous in their dtypes, precision); the arrays must
    have the sizes the header states -- the library reads that many elements."""
    precision = precision_of(arrays)
    real = {k: np.float32 if precision == 32 and k in _NARROWED else np.float64 for k in ARRAYS}
    header = np.ascontiguousarray(arrays['header'], dtype=np.int64).ravel()
    if header.size != len(HEADER) or (header[1:] < 0).any() or (header > 1 << 40).any():
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: bad header')
    h = dict(zip(HEADER, (int(v) for v in header)))
    out = []
    for name, shape in _shapes(h).items():
        a = np.ascontiguousarray(arrays[name],
                                 dtype=np.int32 if name in _INT_ARRAYS else real[name])
        if a.size != int(np.prod(shape)):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s has %d elements, the '
                                 'header states %s' % (name, a.size, shape))
        out.append(a.reshape(shape))
    if precision == 32:
        if out[3].size:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: a single-precision law has '
                                 'no test records')
        del out[3]              # the _single entry points take no test_rec
    return header, out, precision


def check_leaf_mode(leaf_mode, n_leaf):
    """int32 [n_leaf] of a file's (or a caller's) ``leaf_mode``; ``EhmError`` (EHM_E_INVALID) if
    its length is not n_leaf or a value is < -1.  Host only."""
    a = np.asarray(leaf_mode)
    if a.ndim != 1 or a.size != n_leaf or a.dtype.kind not in 'iu':
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: leaf_mode must be %d integers, '
                             'not %s %s' % (n_leaf, a.dtype, a.shape))
    if a.size and (int(a.min()) < -1 or int(a.max()) >= 1 << 31):
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: leaf_mode holds %d (a mode, or '
                             '-1 for none)' % int(a.min() if a.min() < -1 else a.max()))
    return np.ascontiguousarray(a, dtype=np.int32)


def refine_selection(n_leaf, levels, leaves):
    """(levels int32 [n_leaf], selected uint8 [n_leaf]) of ``CompiledLaw.refine``'s ``levels`` (an
    int or int [n_leaf], 0 .. 16) and ``leaves`` (None: all, a bool mask [n_leaf], or leaf ids);
    ``EhmError`` (EHM_E_INVALID) for anything else.  Host only."""
    lv = np.asarray(levels)
    if lv.dtype.kind not in 'iu' or lv.ndim > 1 or (lv.ndim == 1 and lv.size != n_leaf):
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: levels must be an integer or %d '
                             'integers, not %s %s' % (n_leaf, lv.dtype, lv.shape))
    if lv.size and (int(lv.min()) < 0 or int(lv.max()) > _capi.EHM_REFINE_MAX_LEVELS):
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: levels must be 0 .. %d, not %d' % (
            _capi.EHM_REFINE_MAX_LEVELS, int(lv.min() if lv.min() < 0 else lv.max())))
    lv = np.ascontiguousarray(np.broadcast_to(lv, (n_leaf,)), dtype=np.int32)
    if leaves is None:
        return lv, np.ones(n_leaf, dtype=np.uint8)
    sel = np.asarray(leaves)
    if sel.dtype == np.bool_:
        if sel.shape != (n_leaf,):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: a mask of %s for %d leaves' % (
                sel.shape, n_leaf))
        return lv, np.ascontiguousarray(sel, dtype=np.uint8)
    if sel.ndim != 1 or (sel.size and sel.dtype.kind not in 'iu'):
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: leaves must be a bool mask or leaf ids, '
                             'not %s %s' % (sel.dtype, sel.shape))
    if sel.size and (int(sel.min()) < 0 or int(sel.max()) >= n_leaf):
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: leaf %d of %d leaves' % (
            int(sel.min() if sel.min() < 0 else sel.max()), n_leaf))
    mask = np.zeros(n_leaf, dtype=np.uint8)
    mask[sel.astype(np.int64)] = 1
    return lv, mask


def refine_criteria(n_u, max_diameter, max_spread):
    """(max_diameter float64 [1] or None, max_spread float64 [n_u] or None) of ``CompiledLaw.refine``;
    ``EhmError`` (EHM_E_INVALID) for one that is negative or not finite.  Host only."""
    out = []
    for name, value, size in (('max_diameter', max_diameter, 1), ('max_spread', max_spread, n_u)):
        if value is None:
            out.append(None)
            continue
        a = np.asarray(value, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and (name == 'max_diameter' or a.size != size)):
            raise ValueError('%s must be a scalar%s' % (
                name, '' if name == 'max_diameter' else ' or [%d]' % size))
        a = np.ascontiguousarray(np.broadcast_to(a, (size,)))
        if not (np.isfinite(a).all() and (a >= 0.).all()):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: %s must be finite and >= 0, not '
                                 '%s' % (name, a))
        out.append(a)
    return tuple(out)


def read_file(path):
    """(arrays, leaf_mode or None) of a file ``save`` wrote, read and checked for its keys on the
    host; the arrays themselves are validated when they are imported (``validate_arrays``)."""
    with np.load(path, allow_pickle=False) as z:
        if 'format_version' not in z.files or int(z['format_version']) != FORMAT_VERSION:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s is not a format-%d '
                                 'file' % (path, FORMAT_VERSION))
        missing = [k for k in ('header',) + ARRAYS if k not in z.files]
        if missing:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s lacks %s' % (
                path, ', '.join(missing)))
        arrays = {k: z[k] for k in ('header',) + ARRAYS}
        leaf_mode = z['leaf_mode'] if 'leaf_mode' in z.files else None
        precision = int(z['precision']) if 'precision' in z.files else None
    if precision is None:
        # a file from before the key: a double law, whatever dtype its arrays were stored in
        for k in _NARROWED:
            arrays[k] = np.asarray(arrays[k], dtype=np.float64)
    else:
        if precision not in (32, 64):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s states precision %d (32 '
                                 'or 64)' % (path, precision))
        want = np.float32 if precision == 32 else np.float64
        for k in _NARROWED:
            if arrays[k].dtype != want:
                raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s states precision %d, '
                                     'its %s is %s' % (path, precision, k, arrays[k].dtype))
    if leaf_mode is not None:
        header = np.asarray(arrays['header']).ravel()
        if header.size != len(HEADER):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: bad header')
        leaf_mode = check_leaf_mode(leaf_mode, int(header[HEADER.index('n_leaf')]))
    return arrays, leaf_mode


def write_file(path, arrays, leaf_mode=None):
    """What ``CompiledLaw.save`` writes, from ``arrays`` on the host: the format version, the
    arrays, ``leaf_mode`` if given, and for a single law (``precision_of``) the key ``precision`` =
    32.  A double law's file carries no such key: it is the file every earlier version wrote."""
    extra = {} if leaf_mode is None else {'leaf_mode': leaf_mode}
    if precision_of(arrays) == 32:
        extra['precision'] = np.int64(32)
    with open(path, 'wb') as f:
        np.savez(f, format_version=np.int64(FORMAT_VERSION), **arrays, **extra)


def validate_arrays(arrays):
    """Raises ``EhmError`` (EHM_E_INVALID) unless ``arrays`` (``CompiledLaw.arrays()``) are a
    well-formed compiled law of their precision: the library's check of ehm_compiled_import /
    _import_single, on the host."""
    header, arrs, precision = _marshal(arrays)
    fn = _capi.load().ehm_compiled_validate_single if precision == 32 else \
        _capi.load().ehm_compiled_validate
    _check(fn(ptr(header), *[ptr(a) if a.size else None for a in arrs]))


class CompiledLaw:
    """A compiled explicit law on the device.  Made by ``ExplicitMPC.compile()``,
    ``CompiledLaw.load(path)`` or ``CompiledLaw.from_arrays(arrays)``."""

    # class defaults: rollout checks its arguments before it touches anything else
    mpc = None                  # the source's law (ExplicitMPC.compile): the default plant
    leaf_mode = None            # int32 [n_leaf]: step-0 mode of every leaf's commutation, -1 none
    _rollout_plant = None       # the plant the device holds (set_plant)
    _leaf_node = None
    flushed = None              # to_single(flush=True): the counts of the values set to zero
    reduction = None            # reduce(): what the reduction this law came from saved
    refinement = None           # refine(): what the refinement this law came from did
    _root_cells = None          # audit: the roots as the sampler's cells (built on first use)
    _input_scale = None         # audit: the default input_tol

    def __init__(self, handle, device, compile_seconds=0., dtype=np.float64):
        self._lib = _capi.load()
        self._handle = handle
        self.dtype = np.dtype(dtype).type       # np.float64, or np.float32 for a single law
        self.device = int(device)
        self.compile_seconds = float(compile_seconds)
        info = (ctypes.c_int64 * 14)()
        _check(self._lib.ehm_compiled_info(self._handle, ctypes.addressof(info)))
        self._h = dict(zip(HEADER, (int(v) for v in info[:12])))
        self.p, self.n_u = self._h['p'], self._h['n_u']
        self._bytes, self._source_bytes = int(info[12]), int(info[13])

    @classmethod
    def compile(cls, explicit, vertices, spine='tests'):
        """Compiles the law an ``ExplicitMPC`` holds; ``vertices`` [n_nodes, p+1, p] as it was
        set up from.  ``spine='roots'``: the data-less right spine of a nested tree -- the chain
        of test nodes from node 0 along the right children -- gets no records, and the simplices
        that hang off it become the law's roots (ehm_compiled_create_opts); a tree without such a
        chain, and a forest, compile as under the default ``'tests'``."""
        if spine not in ('tests', 'roots'):
            raise ValueError("spine must be 'tests' or 'roots'")
        vertices = f64(vertices)
        if vertices.shape != (explicit.n_nodes, explicit.p + 1, explicit.p):
            raise ValueError('vertices must be [%d, %d, %d]' % (explicit.n_nodes, explicit.p + 1,
                                                                explicit.p))
        handle, secs = ctypes.c_void_p(), ctypes.c_double(0.)
        flags = _capi.EHM_COMPILE_SPINE_ROOTS if spine == 'roots' else 0
        _check(_capi.load().ehm_compiled_create_opts(explicit._handle, ptr(vertices), flags,
                                                     ctypes.byref(handle), ctypes.addressof(secs)))
        return cls(handle, explicit.device, secs.value)

    @classmethod
    def from_arrays(cls, arrays, device=0):
        """A law from ``arrays()``.  ``ehm_compiled_import`` validates what it is given before
        anything reaches the device (``validate_arrays`` is the same check without a device)."""
        header, arrs, precision = _marshal(arrays)
        handle = ctypes.c_void_p()
        fn = _capi.load().ehm_compiled_import_single if precision == 32 else \
            _capi.load().ehm_compiled_import
        _check(fn(int(device), ptr(header), *[ptr(a) if a.size else None for a in arrs],
                  ctypes.byref(handle)))
        return cls(handle, device, dtype=np.float32 if precision == 32 else np.float64)

    def to_single(self, flush=False):
        """The law in single precision: a new, independent ``CompiledLaw`` (``dtype`` np.float32)
        whose internal and leaf records were rounded to nearest float on the device
        (ehm_compiled_narrow).  It keeps ``mpc`` and the leaf modes.  ``EhmError`` for a law with
        test nodes, or one a value of which overflows, becomes zero or subnormal, or whose plane
        loses its normal.  ``flush=True``: a nonzero value whose float is zero or subnormal (it is
        below 2^-126 in magnitude: elimination noise of an inverse) is stored as +0.0 instead of
        refused, and ``flushed`` of the new law counts them: {'a': plane coefficients, 'b': plane
        offsets, 'leaf': leaf values} (DESIGN.md 3.8c states what that adds to the two bounds)."""
        handle = ctypes.c_void_p()
        gone = (ctypes.c_int64 * 3)()
        _check(self._lib.ehm_compiled_narrow_opts(
            self._handle, _capi.EHM_NARROW_FLUSH if flush else 0, ctypes.addressof(gone),
            ctypes.byref(handle)))
        law = type(self)(handle, self.device, self.compile_seconds, dtype=np.float32)
        if flush:
            law.flushed = dict(zip(('a', 'b', 'leaf'), (int(v) for v in gone)))
        law.mpc = self.mpc
        if self.leaf_mode is not None:
            law.set_leaf_modes(self.leaf_mode)
        return law

    def reduce(self, tol=None, return_map=False):
        """
        The law with every subtree whose leaves all apply one affine map within ``tol`` replaced
        by one leaf: a new, independent ``CompiledLaw`` of the same precision and file format
        (ehm_compiled_reduce).  The representative of an internal record is its
        leftmost leaf; the record is mergeable iff every leaf below it has a cell (``cells``), the
        representative's ``leaf_mode`` (where the law holds leaf modes) and, at each vertex of its
        OWN cell and for each input c, an input within ``tol[c]`` of the representative's map
        there, both maps in the law's own arithmetic; a NaN never passes.  The topmost mergeable
        records become leaves.  Both maps are affine, so the new law's input is within ``tol`` of
        this law's at every state of every cell of this law -- against the original leaves, not
        against a merged neighbour, so the bound does not grow with the levels merged.  It is per
        call: a second ``reduce`` of the result may merge further, and its bound adds to the first.
        A merged leaf takes the record, the ``leaf_mode`` and the ``leaf_node`` of its
        representative: ``leaf_node`` of a merged leaf is the representative's source id, not the
        id of a source node that spans the merged cell.
        ``tol``: a scalar or [n_u], finite and >= 0; None: ``applied.default_input_tol`` of the
        leaf records' u_0, the relaxation ``audit`` and ``certify`` grant an input; 0 merges only
        where the computed difference is exactly zero.  A law in which nothing merges comes back
        as an equal, independent copy.  ``mpc``, the leaf modes and ``flushed`` carry over, as in
        ``to_single``.  The new law's ``reduction`` is a dict of n_leaf_before, n_leaf_after,
        n_int_before, n_int_after, bytes_before, bytes_after, tol, max_deviation (the largest
        difference that passed the test: an upper bound of the deviation at the cells' vertices)
        and seconds.  ``return_map=True``: returns (law, leaf_of), leaf_of int32 [n_leaf_before]
        the new leaf record of every original one.  ``EhmError`` (EHM_E_INVALID) for a law with
        test nodes (``compile(spine='roots')`` has none), a ``tol`` that is negative or not
        finite, a ``leaf_mode`` of the wrong length, and a law whose own arrays would not pass
        the import check (``validate_arrays``), which the new law goes through.  Certify before
        reducing: a certificate belongs to the function, and ``certify`` on the reduced law tests
        the larger cells.
        """
        from . import applied
        if not getattr(self, '_handle', None):
            raise ValueError('the law is closed')
        if self._h['n_test'] > 0:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its cells do not '
                                 "follow from its planes -- compile(spine='roots') has none" %
                                 self._h['n_test'])
        n_leaf = self._h['n_leaf']
        if tol is None:
            if self._input_scale is None:
                u0 = self.array('leaf_rec')[:, self.p:self.p + self.n_u]
                self._input_scale = applied.default_input_tol(u0)
            tol = self._input_scale
        tol = np.asarray(tol, dtype=np.float64)
        if tol.ndim > 1 or (tol.ndim == 1 and tol.size != self.n_u):
            raise ValueError('tol must be a scalar or [%d]' % self.n_u)
        tol = np.ascontiguousarray(np.broadcast_to(tol, (self.n_u,)))
        if not (np.isfinite(tol).all() and (tol >= 0.).all()):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'reduce: tol must be finite and >= 0, not '
                                 '%s' % tol)
        modes = None if self.leaf_mode is None else check_leaf_mode(self.leaf_mode, n_leaf)
        if self._root_cells is None:
            self._root_cells = applied.root_cells(self)
        roots = self._root_cells['vertices']
        handle = ctypes.c_void_p()
        modes_out = None if modes is None else np.empty(n_leaf, dtype=np.int32)
        leaf_of = np.empty(n_leaf, dtype=np.int32) if return_map else None
        counts = np.zeros(4, dtype=np.int64)
        stats = np.zeros(2)
        rc = self._lib.ehm_compiled_reduce(self._handle, ptr(roots), ptr(tol), ptr(modes),
                                           ctypes.byref(handle), ptr(modes_out), ptr(leaf_of),
                                           ptr(counts), ptr(stats))
        _check_reduce(rc)
        law = type(self)(handle, self.device, self.compile_seconds, dtype=self.dtype)
        law.flushed = self.flushed
        law.mpc = self.mpc
        if modes is not None:
            law.set_leaf_modes(modes_out[:int(counts[1])])
        law.reduction = dict(n_leaf_before=int(counts[0]), n_leaf_after=int(counts[1]),
                             n_int_before=int(counts[2]), n_int_after=int(counts[3]),
                             bytes_before=self._bytes, bytes_after=law._bytes, tol=tol.copy(),
                             max_deviation=float(stats[0]), seconds=float(stats[1]))
        return (law, leaf_of) if return_map else law

    def refine(self, levels=1, leaves=None, max_diameter=None, max_spread=None, max_leaves=None,
               return_map=False):
        """
        The law with the cells of its leaves bisected, the inverse of ``reduce``: a new, independent
        ``CompiledLaw`` of the same precision and file format (ehm_compiled_refine)
        that applies the same input, bit for bit, at every state.  A leaf is split as the
        partitioner would have split its cell (``cells``): along the first longest edge (i, j) in
        ``tools.split_along_longest_edge``'s arithmetic and order, by the plane that is +1 at v_j,
        -1 at v_i and 0 at the other vertices; the left child is the partitioner's S_1.  Both
        children carry the parent's leaf record, ``leaf_node`` and ``leaf_mode`` byte for byte, and
        a leaf record is anchored, so the audits and the certificate -- statements about the
        function -- carry over; what changes is the cells every leaf-by-leaf statement is made on.
        ``certify`` now tests smaller cells, and ``successors``, ``invariant_core``, the robust
        forms, ``reach`` and ``cost`` have to be computed again on the refined law.  The left child
        keeps the leaf's index, the right children and the new planes are appended in leaf order.

        ``leaves``: None for all, a bool mask [n_leaf], or leaf ids.  ``levels``: an int or int
        [n_leaf], 0 .. 16 passes over the leaves; both children of a split leaf inherit what is
        left.  With no criterion every selected leaf is split ``levels`` times.  With
        ``max_diameter`` (compared with the longest edge) or ``max_spread`` (a scalar or [n_u],
        compared per input c with max_i u_c(v_i) - min_i u_c(v_i) of the leaf's own map at its
        vertices, in the law's arithmetic) a leaf with levels left is split iff one of them is
        exceeded on its own cell; a NaN never splits.  ``max_leaves`` (default 2^24): a call that
        could make more leaves -- 2^levels per selected leaf -- is refused before anything is
        allocated.  A plane that, as stored, fails the test ``cells`` applies (a sliver in a single
        law) is not written: the leaf is kept whole and reported.

        ``mpc``, the leaf modes and ``flushed`` carry over, ``reduction`` is None, ``refinement`` is
        a dict of n_leaf_before, n_leaf_after, n_int_before, n_int_after, bytes_before,
        bytes_after, passes, n_split, max_plane_residual (the largest distance of an accepted
        plane's value at a vertex from +1, -1 or 0; measured, not gated), stops (final leaves by
        stop code: ``_capi.EHM_REFINE_STOPS``), seconds and plan_seconds.  ``return_map=True``:
        returns (law, origin, stop): origin int32 [n_leaf_after] the source leaf of every leaf, stop
        int8 the code of every leaf -- unselected, satisfied (levels done without a criterion, or
        every criterion met), levels (exhausted with a criterion exceeded), no_cell, unseparated,
        too_deep (at depth 256: its children would have no cell).  ``levels`` = 0 returns an equal,
        independent copy.  ``EhmError`` (EHM_E_INVALID) for a law with test nodes, ``levels``
        outside 0 .. 16, ``leaves`` of the wrong length or out of range, a criterion that is
        negative or not finite, a ``leaf_mode`` of the wrong length, ``max_leaves`` exceeded and
        a closed law.
        """
        from . import applied
        if not getattr(self, '_handle', None):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: the law is closed')
        if self._h['n_test'] > 0:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its cells do not '
                                 "follow from its planes -- compile(spine='roots') has none" %
                                 self._h['n_test'])
        n_leaf = self._h['n_leaf']
        levels, selected = refine_selection(n_leaf, levels, leaves)
        crit = refine_criteria(self.n_u, max_diameter, max_spread)
        max_leaves = 1 << 24 if max_leaves is None else int(max_leaves)
        worst = int((1 << levels.astype(np.int64))[selected != 0].sum() + (selected == 0).sum())
        if max_leaves < 1 or worst > max_leaves:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'refine: the call could make %d leaves, '
                                 'max_leaves is %d' % (worst, max_leaves))
        modes = None if self.leaf_mode is None else check_leaf_mode(self.leaf_mode, n_leaf)
        if self._root_cells is None:
            self._root_cells = applied.root_cells(self)
        roots = self._root_cells['vertices']
        handle = ctypes.c_void_p()
        modes_out = None if modes is None else np.empty(worst, dtype=np.int32)
        origin = np.empty(worst, dtype=np.int32)
        stop = np.empty(worst, dtype=np.int8)
        counts = np.zeros(12, dtype=np.int64)
        stats = np.zeros(3)
        rc = self._lib.ehm_compiled_refine(
            self._handle, ptr(roots), ptr(levels), ptr(selected), ptr(crit[0]), ptr(crit[1]),
            ptr(modes), max_leaves, worst, ctypes.byref(handle), ptr(modes_out), ptr(origin),
            ptr(stop), ptr(counts), ptr(stats))
        _check_refine(rc)
        law = type(self)(handle, self.device, self.compile_seconds, dtype=self.dtype)
        law.flushed = self.flushed
        law.mpc = self.mpc
        n_after = int(counts[1])
        if modes is not None:
            law.set_leaf_modes(modes_out[:n_after])
        law.refinement = dict(
            n_leaf_before=int(counts[0]), n_leaf_after=n_after, n_int_before=int(counts[2]),
            n_int_after=int(counts[3]), bytes_before=self._bytes, bytes_after=law._bytes,
            passes=int(counts[4]), n_split=int(counts[5]), max_plane_residual=float(stats[0]),
            stops=dict(zip(_capi.EHM_REFINE_STOPS, (int(v) for v in counts[6:12]))),
            seconds=float(stats[1]), plan_seconds=float(stats[2]))
        if return_map:
            return law, origin[:n_after].copy(), stop[:n_after].copy()
        return law

    @classmethod
    def load(cls, path, device=0):
        """The law ``save`` wrote (one .npz of plain arrays): a single law where the file says
        ``precision`` = 32."""
        arrays, leaf_mode = read_file(path)
        law = cls.from_arrays(arrays, device=device)
        if leaf_mode is not None:
            law.set_leaf_modes(leaf_mode)
        return law

    def save(self, path):
        """Writes the arrays and the format version to ``path`` (.npz); a law that holds leaf
        modes also writes the optional key ``leaf_mode``, a single law ``precision`` = 32 and its
        ``node`` and ``leaf_rec`` as float32."""
        write_file(path, self.arrays(), self.leaf_mode)

    def arrays(self):
        """dict: 'header' (int64 [12], ``HEADER``) and the arrays of ``ARRAYS`` (include/ehmpc.h),
        copied from the device; ``node`` and ``leaf_rec`` of a single law are float32."""
        out = {'header': np.array([self._h[k] for k in HEADER], dtype=np.int64)}
        single = self.dtype is np.float32
        for name, shape in _shapes(self._h).items():
            real = np.float32 if single and name in _NARROWED else np.float64
            out[name] = np.zeros(shape, dtype=np.int32 if name in _INT_ARRAYS else real)
        self._export(*[ptr(out[k]) if out[k].size else None for k in ARRAYS])
        return out

    def array(self, name):
        """One array of ``arrays()`` (a name of ``ARRAYS``), copied from the device alone."""
        single = self.dtype is np.float32
        real = np.float32 if single and name in _NARROWED else np.float64
        out = np.zeros(_shapes(self._h)[name], dtype=np.int32 if name in _INT_ARRAYS else real)
        if out.size:
            self._export(*[ptr(out) if k == name else None for k in ARRAYS])
        return out

    def _export(self, node, leaf_rec, leaf_node, test_rec, root_rec, root_entry, nbr):
        if self.dtype is np.float32:
            _check(self._lib.ehm_compiled_export_single(self._handle, node, leaf_rec, leaf_node,
                                                   root_rec, root_entry, nbr))
        else:
            _check(self._lib.ehm_compiled_export(self._handle, node, leaf_rec, leaf_node,
                                                 test_rec, root_rec, root_entry, nbr))

    @property
    def stats(self):
        """Record counts, strides in bytes, ``bytes`` the law holds on the device and
        ``source_bytes``, what the source evaluator holds for the same tree (0 for a loaded law).
        bytes = (n_plane + n_test) node_stride + n_leaf (leaf_stride + 4) + n_test side_stride
        + n_roots (side_stride + 4) + nbr_bytes.  A double law: node_stride = 64 (p <= 6) or 128,
        leaf_stride = 8 (p + n_u + n_u p) rounded up to 16.  A single law: node_stride =
        4 (p + 3) rounded up to 32 (32 for p <= 5, else 64), leaf_stride = 4 (p + n_u + n_u p)
        rounded up to 16, n_test = 0.  side_stride = 8 (p + p^2) rounded up to 16 in both."""
        h = self._h
        scalar = 4 if self.dtype is np.float32 else 8
        return {'n_plane': h['n_int'] - h['n_test'], 'n_test': h['n_test'], 'n_leaf': h['n_leaf'],
                'n_roots': h['n_roots'], 'node_stride': scalar * h['node_stride'],
                'leaf_stride': scalar * h['leaf_stride'], 'side_stride': 8 * h['side_stride'],
                'nbr_bytes': 4 * h['n_roots'] * (h['p'] + 1) if h['has_nbr'] else 0,
                'bytes': self._bytes, 'source_bytes': self._source_bytes}

    def close(self):
        if getattr(self, '_handle', None):
            self._lib.ehm_compiled_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, X, return_info=False):
        """u [n, n_u] for the states X [n, p]; with return_info also (leaf ids in the source
        tree, decisions made, seconds), as ``ExplicitMPC.evaluate``."""
        X = f64(np.atleast_2d(X))
        if X.shape[1] != self.p:
            raise ValueError('X must be [n, %d]' % self.p)
        n = X.shape[0]
        u = np.empty((n, self.n_u))
        leaf = np.empty(n, dtype=np.int32)
        depth = np.empty(n, dtype=np.int32)
        secs = ctypes.c_double(0.)
        _check(self._lib.ehm_compiled_eval_batch(self._handle, n, ptr(X), ptr(u), ptr(leaf),
                                                 ptr(depth), ctypes.addressof(secs)))
        if return_info:
            return u, leaf, depth, secs.value
        return u

    # -- closed loop ---------------------------------------------------------------------------
    @property
    def leaf_node(self):
        """int32 [n_leaf]: the source node id of every leaf (ascending; in a refined law the
        children of a split leaf share their parent's, so it is neither ascending nor unique)."""
        if self._leaf_node is None:
            out = np.zeros(self._h['n_leaf'], dtype=np.int32)
            self._export(None, None, ptr(out), None, None, None, None)
            self._leaf_node = out
        return self._leaf_node

    def set_leaf_modes(self, modes):
        """The step-0 mode of every leaf's commutation, int32 [n_leaf] in the order of the leaf
        records (-1: no commutation, a trajectory that reaches the leaf stops with status 3);
        None removes the table.  The next rollout hands it to the device with its plant."""
        self.leaf_mode = None if modes is None else check_leaf_mode(modes, self._h['n_leaf'])
        self._rollout_plant = None

    def _plant_modes(self, plant):
        if plant.n_modes == 1 and not plant.guarded:
            return np.zeros(self._h['n_leaf'], dtype=np.int32)
        if self.leaf_mode is None:
            raise ValueError('a hybrid or guarded plant needs the leaf modes (set_leaf_modes; '
                             'ExplicitMPC.compile attaches them when its oracle gives them)')
        return self.leaf_mode

    def set_plant(self, plant):
        """Hands the plant the rollout closes the loop around to the device (once per plant).  A
        single-mode nominal plant needs no ``leaf_mode`` (all zeros), any other plant does."""
        if plant.n_x != self.p or plant.n_u != self.n_u:
            raise ValueError('plant (n_x %d, n_u %d) does not fit the law (p %d, n_u %d)' % (
                plant.n_x, plant.n_u, self.p, self.n_u))
        modes = self._plant_modes(plant)
        opt = lambda a: ptr(a) if a.size else None
        A, B, w, Gx, gx, Q, R = (f64(a) for a in (plant.A, plant.B, plant.w, plant.Gx, plant.gx,
                                                  plant.Q, plant.R))
        if plant.guarded:
            gm, row0, ga, gb, gc, gt, st = plant.guard_arrays()
            ga, gb, gc, gt = f64(ga), f64(gb), f64(gc), f64(gt)
            fn = self._lib.ehm_compiled_set_plant_guarded
            own = (plant.substeps, len(gm), opt(gm), ptr(row0), opt(ga), opt(gb), opt(gc), opt(gt),
                   opt(st), plant.default_mode)
        else:
            rows, H, h = plant.region_arrays()
            E, H, h = f64(plant.E), f64(H), f64(h)
            fn = self._lib.ehm_compiled_set_plant
            own = (plant.n_d, opt(E), ptr(rows), opt(H), opt(h))
        self._rollout_plant = None
        _check(fn(self._handle, plant.n_modes, ptr(A), ptr(B), ptr(w), *own, plant.gx.size, opt(Gx),
                  opt(gx), ptr(modes), 0 if plant.cost == 'inf' else 1, ptr(Q), ptr(R)))
        self._plant_mode = modes
        self._rollout_plant = plant

    def set_noise(self, model, plant):
        """Hands the uncertainty model (``noise.NoiseModel``) to the device; a no-op when the
        device already holds the same packed model for the same n_d."""
        if (model.n_x, model.n_u, model.n_d) != (self.p, self.n_u, plant.n_d):
            raise ValueError('noise model (n_x %d, n_u %d, n_d %d) does not fit the law and plant '
                             '(%d, %d, %d)' % (model.n_x, model.n_u, model.n_d, self.p, self.n_u,
                                               plant.n_d))
        desc, data = model.pack()
        held = getattr(self, '_noise_packed', None)
        if held is not None and held[2] == plant.n_d and np.array_equal(held[0], desc) \
                and np.array_equal(held[1], data):
            return
        self._noise_packed = None
        _check(self._lib.ehm_compiled_set_noise(self._handle, desc.shape[0], ptr(desc),
                                                ptr(data) if data.size else None, data.size,
                                                plant.n_d))
        self._noise_packed = (desc, data, plant.n_d)

    def rollout(self, X0, T, d=None, v=None, record=True, tol_exit=1e-9, plant=None, noise=None,
                seed=0, traj0=0):
        """
        Closed loop from the states X0 [n, p] for T steps in ONE kernel launch
        (ehm_compiled_rollout, one device thread per trajectory), with the signature, status
        codes, records and conventions of ``ExplicitMPC.rollout`` (simulate.py; the step's
        contract and its two differences are in the module docstring).  ``plant`` defaults to the
        plant last set, else to ``Plant.from_mpc`` of the law this one was compiled from.
        Returns a ``simulate.ClosedLoop``: ``leaf`` holds source node ids, ``mode`` comes from
        ``leaf_mode`` (None for a guarded plant), ``commutation`` stays None.
        """
        from . import simulate
        X0 = f64(np.atleast_2d(X0))
        n, p = X0.shape
        T = int(T)
        if plant is None:
            plant = self._rollout_plant
        if plant is None and self.mpc is not None:
            plant = simulate.Plant.from_mpc(self.mpc)
        d, v = simulate._check_rollout_args(plant, noise, d, v, n, p, T)
        if p != self.p or T < 0:
            raise ValueError('X0 must be [n, %d] and T >= 0' % self.p)
        if plant is not self._rollout_plant:
            self.set_plant(plant)
        if noise is not None:
            self.set_noise(noise, plant)
        rec = lambda shape, dtype=np.float64: np.empty(shape, dtype) if record else None
        xs, us, leaf = rec((T + 1, n, p)), rec((T, n, self.n_u)), rec((T, n), np.int32)
        x_final = np.empty((n, p))
        steps = np.empty(n, dtype=np.int32)
        status = np.empty(n, dtype=np.int32)
        cost, unorm, maxv = np.empty(n), np.empty(n), np.empty(n)
        secs = ctypes.c_double(0.)
        if noise is None:
            vs = es = ws = None
            fn = self._lib.ehm_compiled_rollout
            head = (ptr(d), ptr(v), float(tol_exit), ptr(xs), ptr(us), ptr(leaf))
        else:
            vs, es, ws = rec((T, n, p)), rec((T, n, self.n_u)), rec((T, n, plant.n_d))
            fn = self._lib.ehm_compiled_rollout_noisy
            head = (int(seed), int(traj0), float(tol_exit), ptr(xs), ptr(us), ptr(leaf), ptr(vs),
                    ptr(es), ptr(ws))
        _check(fn(self._handle, n, T, ptr(X0), *head, ptr(x_final), ptr(steps), ptr(status),
                  ptr(cost), ptr(unorm), ptr(maxv), ctypes.addressof(secs)))
        out = simulate.ClosedLoop(x_final=x_final, steps=steps, status=status, cost=cost,
                                  u_norm_sum=unorm, max_violation=maxv, seconds=secs.value,
                                  x=xs, u=us, leaf=leaf, v=vs, e=es, w=ws)
        if record and not plant.guarded:
            live = leaf >= 0
            order = np.argsort(self.leaf_node, kind='stable')      # ascending for a compiled law
            at = np.searchsorted(self.leaf_node, np.maximum(leaf, 0), sorter=order)
            l = order[np.minimum(at, order.size - 1)]
            out.mode = np.where(live, self._plant_mode[l], -1).astype(np.int32)
        return out

    # -- audit by the cost of the applied input (applied.py) ----------------------
    def audit(self, oracle, n=None, X=None, seed=0, rtol=1e-7, input_tol=None,
              return_samples=False, first=0, chunk=0):
        """
        Checks the law's contract at sampled states by what its input costs:
        0 <= V_u(x) - V*(x) <= max(eps_a, eps_r V*(x)),  V_u the optimum of P_theta with the first
        input fixed to ``evaluate(x)`` (``applied.applied_input_problem``), V* the optimum of
        P_theta, both from the batched P_theta of ``oracle`` -- an argument, because a loaded law
        has none --, each side with the slack rtol (1 + |V*|).  Give ``n`` -- points drawn uniform
        in the law's roots (``applied.root_cells``) with the sampler, key and global ids
        ``first`` .. ``first + n - 1`` of ``ExplicitMPC.sample`` -- or the states ``X``, not both.
        ``input_tol``: by how much (infinity norm) the input may be moved to meet a row, a
        relaxation (None: 1e-7 max(1, largest |u_0| of the leaf records)); it is used only at a
        sample whose input is not admissible as it stands (``relaxed``, ``n_relaxed``), every
        other V_u is the exact substitution's.  ``chunk``: samples per
        pass; no result depends on it.  Works for double and single laws, compiled here or loaded.
        ``EhmError`` for a law with test nodes (``compile(spine='roots')`` has none) and for an
        oracle without a batched P_theta; ``ValueError`` for p + n_u > 8.  Returns an
        ``applied.AppliedAuditResult``.  A sampled check; ``certify`` gives the statement that
        holds at every state of a leaf.
        """
        from . import applied
        if not getattr(self, '_handle', None):
            raise ValueError('the law is closed')
        if (n is None) == (X is None):
            raise ValueError('give n (points drawn in the roots) or X, not both')
        applied.oracle_gpu(oracle)
        if self._h['n_test'] > 0:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'the law has %d test nodes: its roots do '
                                 "not tile the set -- compile(spine='roots') has none" %
                                 self._h['n_test'])
        if input_tol is None:
            if self._input_scale is None:
                u0 = self.array('leaf_rec')[:, self.p:self.p + self.n_u]
                self._input_scale = applied.default_input_tol(u0)
            input_tol = self._input_scale
        if X is None and self._root_cells is None:
            self._root_cells = applied.root_cells(self)
        return applied.run(oracle, self.p, self.n_u, self.device, input_tol, law=self._handle,
                           X=X, cells=self._root_cells, n=n, seed=seed, rtol=rtol,
                           return_samples=return_samples, first=first, chunk=chunk)

    # -- the leaf cells (certify.py) ------------------------------------------------
    def cells(self, leaves=None):
        """
        The simplex of every leaf (``leaves``: rows of the leaf records, None: all), rebuilt on the
        device from the root records, the root entries and the planes alone, and the input this
        leaf's own map gives at each of its vertices, in the law's own arithmetic.  Works for
        double and single laws, compiled here or loaded; the same law loaded from its file gives
        the same cells bit for bit.  A leaf more than 256 levels below its root, or one whose path
        holds a node that does not bisect the cell that reaches it, has status ``no_cell`` and NaN
        rows.  ``EhmError`` for a law with test nodes (``compile(spine='roots')`` has none).
        Returns a ``certify.LeafCells``.
        """
        from . import certify
        return certify.cells(self, leaves)

    def certify(self, oracle, leaves=None, input_tol=None, max_tries=3, chunk=0,
                return_leaves=False):
        """
        Certifies the law's contract leaf by leaf: a leaf is ``certified`` when
        V_u(x) - V*(x) < max(eps_a, eps_r V*(x)) is PROVED at every state x of its cell, V_u and V*
        as in ``audit``.  On a leaf the law is affine, so for a fixed commutation d the cost of its
        input is convex in x and lies below the interpolation of its values W at the cell's
        vertices; the decision form of the reference's bar_E_delta_R (``ehm_bar_e_batch``) with
        Vbar = W then closes the cell or not.  The candidates d are the commutations of the
        applied-input problem feasible at all p + 1 vertices (by convexity feasible on the cell),
        tried in the order of sum W, at most ``max_tries`` of them (0: all); any one that closes
        the cell proves the statement.  A leaf without a candidate is tried on the problem relaxed
        by ``input_tol`` (None: as ``audit``) and marked ``relaxed``: its certificate is for an
        input within input_tol of the law's.  ``leaves``: rows of the leaf records (None: all);
        ``chunk``: leaves per pass, no result depends on it.

        What it covers: the piecewise-affine function the arrays define on the cells their planes
        define (``cells``).  Not: the rounding of a single law's evaluation (DESIGN.md 3.8c bounds
        it), a state within rounding of a split face being handed to the sibling leaf's map, the
        recovery error of the root vertices the cells carry, nor the tolerances of the LP solves.
        ``uncertified`` is not a violation: the vertex interpolation of a convex function is an
        upper bound, not the function.  Refusals as ``audit``.  Returns a
        ``certify.CertificateResult``.
        """
        from . import certify
        return certify.certify(self, oracle, leaves=leaves, input_tol=input_tol,
                               max_tries=max_tries, chunk=chunk, return_leaves=return_leaves)

    # -- one-step invariance leaf by leaf (invariance.py) ---------------------------
    def successors(self, plant=None, d_box=None, leaves=None, tol_exit=1e-9,
                   return_successors=False, chunk=0):
        """
        Where the law's input sends the state, leaf by leaf: on a leaf the law is affine and in the
        leaf's step-0 mode the plant is affine, so the image of the leaf under every disturbance of
        the box ``d_box`` = (lo, hi) (arrays [plant.n_d]; None: the nominal successor, no E term)
        is the convex hull of its successors at the (p + 1) 2^n_d points (cell vertex, box corner).
        Each is computed bit for bit as ``rollout`` would compute it for that state, input, mode
        and disturbance, located as one rollout step locates its state, and judged by the
        rollout's exit test (``tol_exit``).  Status per leaf, the first that applies: ``no_cell``,
        ``no_mode`` (no step-0 mode: the rollout's status 3), ``mode_region`` (a vertex of the
        cell is outside the region of the leaf's mode: status 2 can occur on the leaf), ``exits``
        (a vertex successor leaves the partitioned set: status 1 can occur), ``invariant``.
        ``plant`` defaults as in ``rollout``; a guarded plant is refused (``ValueError``): its
        mode is chosen per substep by guards, so the successor is not affine on a leaf.
        ``leaves``: rows of the leaf records (None: all); ``chunk``: leaves per pass, no result
        depends on it.  ``return_successors``: also the successors, their roots and their leaves
        (the transition relation of the vertices).

        ``invariant`` for every leaf proves that no trajectory leaves the set only where the set
        -- the union of the roots -- is convex (``set_convex``, ``holds_on_set``); without that it
        is a statement about the vertex successors.  What it covers: the piecewise-affine function
        the arrays define on the cells their planes define, the nominal plant of ``Plant`` with a
        box disturbance.  Not: measurement error v or input error e, the rounding of a single
        law's evaluation at interior points, the sibling hand-over within rounding of a split
        face, the recovery error of the root vertices.  ``margin`` is in units of the chosen
        root's weights: for a point outside it orders leaves, it is not a distance.  ``EhmError``
        for a law with test nodes.  Returns an ``invariance.SuccessorResult``.
        """
        from . import invariance
        return invariance.successors(self, plant=plant, d_box=d_box, leaves=leaves,
                                     tol_exit=tol_exit, return_successors=return_successors,
                                     chunk=chunk)

    # -- the leaves the closed loop never leaves (invariance.py) -----------------
    def invariant_core(self, plant=None, d_box=None, tol_exit=1e-9, tol_side=None,
                       rows='invariant', return_edges=False, max_fan=None, max_edges=None):
        """
        From which leaves is it safe to start?  ``successors`` judges one step; this follows the
        steps after it.  The MAY-REACH relation lists, for every leaf, the leaves the image of
        that leaf -- under the law, the plant and every disturbance of ``d_box`` -- can land in;
        it is a superset of what the evaluator can return for any state of the leaf.  The CORE is
        the largest set of leaves that is closed under it and holds no leaf that fails the
        one-step test (``tol_exit``): where the set is convex (``set_convex``), every state of a
        core leaf stays in the set, in its mode's region and in a core leaf for ever.  A leaf
        outside the core has a ``level``: 0 for a leaf that fails the one-step test, k for one
        that can reach level k - 1, so its states have k safe steps.  The relation is a superset,
        so the core is an inner approximation: leaves next to a leaking leaf are lost
        conservatively.

        ``tol_side`` (default ``tol_exit``; keep it >= ``tol_exit``) is the slack of every side
        decision, in the units of the planes (half the bisected edge) and of the roots' weights;
        it has to cover the rounding of the sums the decisions are made on.  ``rows``:
        ``'invariant'`` builds the rows the fixed point needs, ``'all'`` those of every leaf with
        a cell and a mode (the transition graph of the whole law).  ``return_edges``: also the
        relation as CSR.  ``max_fan`` (default ``invariance.MAX_FAN``): a longer row is cut off
        and its leaf is a seed with status ``unresolved``; ``max_edges`` (``invariance.MAX_EDGES``):
        a relation with more edges is an ``EhmError`` that names the total.  Always the whole law:
        a fixed point over some of the leaves means nothing.  Covered and not covered: as
        ``successors``.  Refusals as ``successors``.  Returns an ``invariance.CoreResult``.
        """
        from . import invariance
        return invariance.invariant_core(
            self, plant=plant, d_box=d_box, tol_exit=tol_exit, tol_side=tol_side, rows=rows,
            return_edges=return_edges,
            max_fan=invariance.MAX_FAN if max_fan is None else max_fan,
            max_edges=invariance.MAX_EDGES if max_edges is None else max_edges)

    # -- the same two questions under measurement and input error (robust.py) -------
    def robust_successors(self, plant=None, d_box=None, v_box=None, e_box=None, noise=None,
                          leaves=None, tol_exit=1e-9, tol_set=1e-9, chunk=0, radii='global',
                          radius_iters=3):
        """
        ``successors`` for the closed loop ``rollout(..., noise=)`` runs: the law is evaluated at
        the measured state z = x + v, the region of the leaf's mode is tested on the true state,
        the plant steps with u + e and a disturbance d.  With d, v and e in the boxes ``d_box``,
        ``v_box``, ``e_box`` (each (lo, hi) or None for none; v and e must hold 0) the image of a
        leaf's measured states is the hull of its p + 1 nominal vertex successors plus
        G_m [box], G_m = [E | -A_m | B_m | I], box = [d; v; e; v] -- up to 64 generators, no corner
        enumerated.  A leaf is ``invariant`` when the minimum over that image of every boundary
        facet's form n_f . z - c_f (``invariance.boundary_facets``, unit normals) is
        >= -tol_set max|root vertex| and every region row of its mode holds on cell - v box
        (``tol_exit``); else ``exits`` / ``mode_region``; ``no_mode``, ``no_cell`` as
        ``successors``.  ``margin`` is the smallest facet minimum, a distance in state units with
        no threshold applied.  ``tol_set`` defaults to the tolerance within which the set is known
        to be convex at all.

        ``noise=`` (a ``NoiseModel``; not together with a box) fills the three boxes from the model:
        ``noise.bounding_boxes`` at ``u_abs``, the largest vertex input modulus of any leaf, and at
        ``x_abs``, a verified bound on every true state (``noise.state_bound`` from the set's
        largest vertex moduli); both are in the result with the boxes.  These boxes are global
        (``radii='global'``, the default).  With neither noise nor v / e boxes this is the
        closed-form test under ``d_box`` alone, for any n_d up to 64.

        ``radii='leaf'`` (needs ``noise=``, takes no boxes) bounds every error on
        leaf L at the states and inputs L itself can see: the true state by ``radius_iters`` (1..16)
        steps of a <- min(a, c_L + vhalf(a, u_abs)) from the global ``x_abs``, the input by the
        leaf's largest vertex input modulus, the next true state by the leaf's image.  The device
        makes one box per leaf from the packed model the rollout uses; the result then also holds
        ``leaf_boxes``, ``x_abs_leaf``, ``x_next_abs`` and ``u_abs_leaf``, and ``boxes``, ``x_abs``,
        ``u_abs`` stay the global ones.  ``ValueError`` without ``noise=``, with a box, for an
        unknown ``radii``, a ``radius_iters`` outside 1..16 and a model whose constant part of the
        v or e box does not hold 0.

        As with ``successors``, the result proves something only where the set is convex
        (``set_convex``, ``holds_on_set``); without that the facets bound nothing.  Not covered:
        the rounding of a single law's evaluation at interior points, the hand-over within
        rounding of a split face, the recovery error of the root vertices, guarded plants
        (``ValueError``).  ``EhmError`` for a law with test nodes.  Returns a
        ``robust.RobustSuccessorResult``.
        """
        from . import robust
        return robust.robust_successors(self, plant=plant, d_box=d_box, v_box=v_box, e_box=e_box,
                                        noise=noise, leaves=leaves, tol_exit=tol_exit,
                                        tol_set=tol_set, chunk=chunk, radii=radii,
                                        radius_iters=radius_iters)

    def robust_core(self, plant=None, d_box=None, v_box=None, e_box=None, noise=None,
                    tol_exit=1e-9, tol_set=1e-9, tol_side=None, rows='invariant',
                    return_edges=False, max_fan=None, max_edges=None, radii='global',
                    radius_iters=3):
        """
        ``invariant_core`` for the noisy closed loop: the may-reach relation of the images of
        ``robust_successors`` (boxes and ``noise=`` as there), seeded with the leaves its one-step
        test does not call invariant.  Where the set is convex, every trajectory of the noisy
        closed loop from a state of a core leaf has, for any errors in the boxes and at every
        length, every measured state in the set and in a core leaf, every true state in its mode's
        region and within the v box of the set; a leaf of level k has k safe steps.  ``tol_side``,
        ``rows``, ``return_edges``, ``max_fan``, ``max_edges`` as ``invariant_core``; ``radii`` and
        ``radius_iters`` as ``robust_successors`` (``'leaf'``: the image of a leaf is spanned by the
        leaf's own boxes, which the device makes for all leaves itself).  Returns an
        ``invariance.CoreResult`` whose ``seeds`` is the ``robust.RobustSuccessorResult``.
        """
        from . import invariance, robust
        return robust.robust_core(
            self, plant=plant, d_box=d_box, v_box=v_box, e_box=e_box, noise=noise,
            tol_exit=tol_exit, tol_set=tol_set, tol_side=tol_side, rows=rows,
            return_edges=return_edges,
            max_fan=invariance.MAX_FAN if max_fan is None else max_fan,
            max_edges=invariance.MAX_EDGES if max_edges is None else max_edges, radii=radii,
            radius_iters=radius_iters)

    # -- where the closed loop goes (invariance.py) -------------------------------
    def reach(self, core, start=None, X0=None, horizon=0, max_sweeps=None, return_steps=False,
              row_map=None):
        """
        The reach tube, the limit set and the step sets of the closed loop from ``start`` (or the
        leaves of the states ``X0``; neither: all core leaves), over the relation of ``core``, an
        ``invariance.CoreResult`` of this law made with ``return_edges=True`` by ``invariant_core``
        or ``robust_core``: ``core.reach(...)``, which documents the arguments.  Returns an
        ``invariance.ReachResult``.
        """
        if getattr(core, '_law', None) is not self:
            raise ValueError('the core was made for another law')
        return core.reach(start=start, X0=X0, horizon=horizon, max_sweeps=max_sweeps,
                          return_steps=return_steps, row_map=row_map)

    # -- what the closed loop spends (invariance.py) ------------------------------
    def cost(self, core, domain=None, start=None, X0=None, horizon=64, w_hi=None, w_lo=None,
             return_paths=False):
        """
        Certified bounds of the summed input 2-norm of every trajectory that stays in ``domain``
        (None: the core) over the relation of ``core``, an ``invariance.CoreResult`` of this law
        made with ``return_edges=True``: ``core.cost(...)``, which documents the arguments.
        Returns an ``invariance.CostResult``.
        """
        if getattr(core, '_law', None) is not self:
            raise ValueError('the core was made for another law')
        return core.cost(domain=domain, start=start, X0=X0, horizon=horizon, w_hi=w_hi,
                         w_lo=w_lo, return_paths=return_paths)

    def __call__(self, x):
        """(u, t): the input for state x and the evaluation time, as the reference's call."""
        tic = time.time()
        u = self.evaluate(np.asarray(x, dtype=np.float64)[None])[0]
        return u, time.time() - tic
