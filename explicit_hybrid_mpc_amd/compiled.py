"""
The explicit law compiled for deployment (csrc/ehm_compiled.hip):

    law = ExplicitMPC(tree, oracle).compile()     # CompiledLaw, independent of its source
    u = law.evaluate(X)                           # as ExplicitMPC.evaluate
    law.save('law.npz'); law = CompiledLaw.load('law.npz')

Every split of the partition is a bisection, so an internal node keeps one hyperplane (the split
face, p + 1 doubles) next to its two child indices instead of the child's p + p^2 record, and a
leaf keeps the affine map u = u_0 + K (x - v_0) instead of its vertex inputs.  Nodes whose
children are no bisection (the data-less spine of a nested reference tree) keep the reference's
containment test.  The compiled law has no exit test: rollouts stay on ``ExplicitMPC``.  No CPU
fallback.
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


def _check(rc):
    if rc != _capi.EHM_OK:
        raise _capi.EhmError(rc, _capi.load().ehm_compiled_last_error().decode('utf-8', 'replace'))


def _shapes(h):
    """The shape of every array a header states."""
    return {'node': (h['n_int'], h['node_stride']), 'leaf_rec': (h['n_leaf'], h['leaf_stride']),
            'leaf_node': (h['n_leaf'],), 'test_rec': (h['n_test'], h['side_stride']),
            'root_rec': (h['n_roots'], h['side_stride']), 'root_entry': (h['n_roots'],),
            'nbr': (h['n_roots'] if h['has_nbr'] else 0, h['p'] + 1)}


def _marshal(arrays):
    """(header int64 [12], the seven arrays contiguous in their dtypes); the arrays must have the
    sizes the header states -- the library reads that many elements."""
    header = np.ascontiguousarray(arrays['header'], dtype=np.int64).ravel()
    if header.size != len(HEADER) or (header[1:] < 0).any() or (header > 1 << 40).any():
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: bad header')
    h = dict(zip(HEADER, (int(v) for v in header)))
    out = []
    for name, shape in _shapes(h).items():
        a = np.ascontiguousarray(arrays[name],
                                 dtype=np.int32 if name in _INT_ARRAYS else np.float64)
        if a.size != int(np.prod(shape)):
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s has %d elements, the '
                                 'header states %s' % (name, a.size, shape))
        out.append(a.reshape(shape))
    return header, out


def validate_arrays(arrays):
    """Raises ``EhmError`` (EHM_E_INVALID) unless ``arrays`` (``CompiledLaw.arrays()``) are a
    well-formed compiled law: the library's check of ehm_compiled_import, on the host."""
    header, arrs = _marshal(arrays)
    _check(_capi.load().ehm_compiled_validate(ptr(header), *[ptr(a) if a.size else None
                                                             for a in arrs]))


class CompiledLaw:
    """A compiled explicit law on the device.  Made by ``ExplicitMPC.compile()``,
    ``CompiledLaw.load(path)`` or ``CompiledLaw.from_arrays(arrays)``."""

    def __init__(self, handle, device, compile_seconds=0.):
        self._lib = _capi.load()
        self._handle = handle
        self.device = int(device)
        self.compile_seconds = float(compile_seconds)
        info = (ctypes.c_int64 * 14)()
        _check(self._lib.ehm_compiled_info(self._handle, ctypes.addressof(info)))
        self._h = dict(zip(HEADER, (int(v) for v in info[:12])))
        self.p, self.n_u = self._h['p'], self._h['n_u']
        self._bytes, self._source_bytes = int(info[12]), int(info[13])

    @classmethod
    def compile(cls, explicit, vertices):
        """Compiles the law an ``ExplicitMPC`` holds; ``vertices`` [n_nodes, p+1, p] as it was
        set up from."""
        vertices = f64(vertices)
        if vertices.shape != (explicit.n_nodes, explicit.p + 1, explicit.p):
            raise ValueError('vertices must be [%d, %d, %d]' % (explicit.n_nodes, explicit.p + 1,
                                                                explicit.p))
        handle, secs = ctypes.c_void_p(), ctypes.c_double(0.)
        _check(_capi.load().ehm_compiled_create(explicit._handle, ptr(vertices),
                                                ctypes.byref(handle), ctypes.addressof(secs)))
        return cls(handle, explicit.device, secs.value)

    @classmethod
    def from_arrays(cls, arrays, device=0):
        """A law from ``arrays()``.  ``ehm_compiled_import`` validates what it is given before
        anything reaches the device (``validate_arrays`` is the same check without a device)."""
        header, arrs = _marshal(arrays)
        handle = ctypes.c_void_p()
        _check(_capi.load().ehm_compiled_import(int(device), ptr(header),
                                                *[ptr(a) if a.size else None for a in arrs],
                                                ctypes.byref(handle)))
        return cls(handle, device)

    @classmethod
    def load(cls, path, device=0):
        """The law ``save`` wrote (one .npz of plain arrays)."""
        with np.load(path, allow_pickle=False) as z:
            if 'format_version' not in z.files or int(z['format_version']) != FORMAT_VERSION:
                raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s is not a format-%d '
                                     'file' % (path, FORMAT_VERSION))
            missing = [k for k in ('header',) + ARRAYS if k not in z.files]
            if missing:
                raise _capi.EhmError(_capi.EHM_E_INVALID, 'compiled law: %s lacks %s' % (
                    path, ', '.join(missing)))
            arrays = {k: z[k] for k in ('header',) + ARRAYS}
        return cls.from_arrays(arrays, device=device)

    def save(self, path):
        """Writes the arrays and the format version to ``path`` (.npz)."""
        with open(path, 'wb') as f:
            np.savez(f, format_version=np.int64(FORMAT_VERSION), **self.arrays())

    def arrays(self):
        """dict: 'header' (int64 [12], ``HEADER``) and the arrays of ``ARRAYS`` (include/ehmpc.h),
        copied from the device."""
        out = {'header': np.array([self._h[k] for k in HEADER], dtype=np.int64)}
        for name, shape in _shapes(self._h).items():
            out[name] = np.zeros(shape, dtype=np.int32 if name in _INT_ARRAYS else np.float64)
        _check(self._lib.ehm_compiled_export(self._handle, *[ptr(out[k]) if out[k].size else None
                                                             for k in ARRAYS]))
        return out

    @property
    def stats(self):
        """Record counts, strides in bytes, ``bytes`` the law holds on the device and
        ``source_bytes``, what the source evaluator holds for the same tree (0 for a loaded law).
        bytes = (n_plane + n_test) node_stride + n_leaf (leaf_stride + 4) + n_test side_stride
        + n_roots (side_stride + 4) + nbr_bytes."""
        h = self._h
        return {'n_plane': h['n_int'] - h['n_test'], 'n_test': h['n_test'], 'n_leaf': h['n_leaf'],
                'n_roots': h['n_roots'], 'node_stride': 8 * h['node_stride'],
                'leaf_stride': 8 * h['leaf_stride'], 'side_stride': 8 * h['side_stride'],
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

    def __call__(self, x):
        """(u, t): the input for state x and the evaluation time, as the reference's call."""
        tic = time.time()
        u = self.evaluate(np.asarray(x, dtype=np.float64)[None])[0]
        return u, time.time() - tic
