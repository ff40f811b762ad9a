"""
Explicit MPC evaluation with the reference's interface (lib/mpc_library.py:662-792) on the GPU:

    ExplicitMPC(tree, oracle)(x)  ->  (u, t)            one state, like the reference
    ExplicitMPC(tree, oracle).evaluate(X)  ->  u [n, n_u]   a batch in one kernel launch

``tree`` is the partition as the reference stores it (nested ``tree.Tree`` with the Delaunay
right spine on top, e.g. loaded from a reference ``tree.pkl``) or the engine's ``FlatTree``.
Point location follows the reference exactly: at an internal node go left iff the state lies
in the left child's simplex (barycentric weights in [-eps, 1+eps]), else right; at the leaf
interpolate the vertex inputs.  The walk runs in ``ehm_explicit_eval_batch`` (one thread per
state); ``inv([v1-v0 .. vp-v0])`` of every simplex is computed on the device at set-up
(``compute_simplex_basis_inverse``, lib/mpc_library.py:685-712).  No CPU fallback.
"""

import ctypes
import time

import numpy as np

from . import _capi
from ._capi import f64, ptr
from .engine import FlatTree


_check = _capi.checker('ehm_explicit_last_error')


def node_commutation(nd):
    """The commutation a nested-tree node stores (NodeData.commutation), or None."""
    c = getattr(nd.data, 'commutation', None) if nd.data is not None else None
    return None if c is None else np.asarray(c, dtype=np.float64)


def flatten_tree(root, commutations=False, costs=False):
    """
    Nested ``tree.Tree`` (reference layout) -> flat arrays with node 0 = root, children after
    their parents: (vertices, vertex_inputs, left, right, nodes).  Data-less spine nodes and
    nodes without inputs get placeholders; they are never tested (only left children and final
    leaves are, lib/mpc_library.py:703-711) or never returned.  With ``commutations`` also the
    list of every node's commutation vector (None where the node has none).  With ``costs`` also
    a dict of what the audit reads: ``vertex_costs`` [K, p+1] (NaN where a node has none),
    ``flags`` uint8 [K] (bit 0: is_epsilon_suboptimal, as FlatTree.flags) and ``simplex`` bool [K]
    (the node's data holds a simplex, i.e. it is no spine node).
    """
    first, stack = None, [root]
    while stack:                        # any node with vertex inputs tells the shapes
        nd = stack.pop()
        if nd.data is not None and hasattr(nd.data, 'vertex_inputs'):
            first = nd
            break
        if not nd.is_leaf():
            stack += [nd.right, nd.left]
    if first is None:
        raise ValueError('the tree has no node with vertex inputs')
    p = np.asarray(first.data.vertices).shape[1]
    n_u = np.asarray(first.data.vertex_inputs).shape[1]
    unit = np.vstack([np.zeros(p), np.eye(p)])
    nodes, left, right = [root], [], []
    head = 0
    while head < len(nodes):
        nd = nodes[head]
        if nd.is_leaf():
            left.append(-1)
            right.append(-1)
        else:
            left.append(len(nodes))
            right.append(len(nodes) + 1)
            nodes += [nd.left, nd.right]
        head += 1
    K = len(nodes)
    vertices = np.empty((K, p + 1, p))
    vinput = np.zeros((K, p + 1, n_u))
    for k, nd in enumerate(nodes):
        d = nd.data
        ok = d is not None and np.asarray(d.vertices).shape == (p + 1, p)
        vertices[k] = np.asarray(d.vertices, dtype=np.float64) if ok else unit
        if d is not None and hasattr(d, 'vertex_inputs'):
            vinput[k] = np.asarray(d.vertex_inputs, dtype=np.float64)
    out = (vertices, vinput, np.array(left, dtype=np.int32), np.array(right, dtype=np.int32), nodes)
    if commutations:
        out = out + ([node_commutation(nd) for nd in nodes],)
    if costs:
        vcost = np.full((K, p + 1), np.nan)
        flags = np.zeros(K, dtype=np.uint8)
        simplex = np.zeros(K, dtype=bool)
        for k, nd in enumerate(nodes):
            d = nd.data
            if d is None:
                continue
            simplex[k] = np.asarray(d.vertices).shape == (p + 1, p)
            if hasattr(d, 'vertex_costs'):
                vcost[k] = np.asarray(d.vertex_costs, dtype=np.float64)
            flags[k] = 1 if getattr(d, 'is_epsilon_suboptimal', False) else 0
        out = out + (dict(vertex_costs=vcost, flags=flags, simplex=simplex),)
    return out


def forest_order(left, right, spine):
    """
    Node ids of a flattened nested tree in the numbering of the engine's flat export: the roots
    (the first nodes below the spine, in spine order), then breadth first over all of them, the
    left child before the right one.  ``spine`` [K] marks the nodes above the roots.
    """
    roots, stack = [], [0]
    while stack:
        k = stack.pop()
        if spine[k] and left[k] >= 0:
            stack += [int(right[k]), int(left[k])]
        else:
            roots.append(k)
    order, head = roots, 0
    while head < len(order):
        k = order[head]
        head += 1
        if left[k] >= 0:
            order += [int(left[k]), int(right[k])]
    return np.array(order, dtype=np.int64)


STATUS_NAMES = ('within', 'violation', 'negative', 'open', 'infeasible')    # by status value


class AuditResult:
    """
    What ``ExplicitMPC.audit`` found (a sampled check, not a certificate):
    ``counts`` samples by status name (STATUS_NAMES), ``relocated`` samples located in a leaf other
    than the cell they were drawn in, ``max_ratio`` the largest (Vbar - V*) / bound over statuses
    0-2 (-inf if there is none), ``worst`` that sample (id, x, cell, leaf, vbar, vstar, bound; None
    if there is none), ``histogram`` int64 [33] of the ratio (32 bins over [0, 1], one above),
    ``open_volume_fraction`` the volume of the leaves that are not closed over the volume of all
    leaves (exact, from flags and volumes, not sampled), ``seconds`` (sampling kernel, locate and
    reduce kernels, P_theta batches), ``n``, and with ``return_samples`` the arrays ``x, cell,
    leaf, vbar, wmin, vstar, delta_idx, status``.  ``passed``: no violation, no negative, no
    infeasible, and no open leaf unless ``allow_open``.
    """

    def __init__(self, **kw):
        self.x = self.cell = self.leaf = self.vbar = self.wmin = self.vstar = None
        self.delta_idx = self.status = None
        self.__dict__.update(kw)

    @property
    def passed(self):
        c = self.counts
        bad = c['violation'] + c['negative'] + c['infeasible']
        return bad == 0 and (self.allow_open or c['open'] == 0)

    def __repr__(self):
        return 'AuditResult(n=%d, passed=%s, counts=%r, max_ratio=%.6g, relocated=%d, ' \
            'open_volume_fraction=%.6g)' % (self.n, self.passed, self.counts, self.max_ratio,
                                            self.relocated, self.open_volume_fraction)


class ImplicitMPC:
    """
    The implicit law of lib/mpc_library.py:626-660 (same constructor and call signature): one
    mixed-integer oracle solve ``P_theta(x)`` per call, i.e. on the device one batched launch
    over the commutations.  ``evaluate`` is the batched form.
    """

    def __init__(self, oracle):
        mpc = oracle.mpc
        self.plant = getattr(mpc, 'plant', None)
        self.T_s = getattr(mpc, 'T_s', None)
        if hasattr(mpc, 'specs'):
            self.specs = mpc.specs
        self.__oracle = oracle
        self.mpc = mpc

    def __call__(self, x):
        """(u, t): epsilon-suboptimal (here: optimal) input and evaluation time."""
        u, _, _, t = self.__oracle.P_theta(x)
        return u, t

    def rollout(self, X0, T, d=None, v=None, record=True, tol_exit=1e-9, plant=None, noise=None,
                seed=0, traj0=0, on_device=False):
        """
        Closed loop from the states X0 [n, p] for T steps (simulate.py): per step one batched
        P_theta over the live trajectories, the plant (default ``Plant.from_mpc``) stepped in
        the step-0 mode of the returned commutation.  ``noise`` (a ``noise.NoiseModel``) draws
        v, e and d on the host with the counters of the device rollout (trajectory q has id
        traj0 + q).  ``on_device=True``: the whole loop runs on the device
        (``simulate.rollout_implicit``; the result also has ``stalled`` and ``n_stalled_pairs``).
        Returns a ``simulate.ClosedLoop``.
        """
        from . import simulate
        if plant is None:
            plant = simulate.Plant.from_mpc(self.__oracle.mpc)
        self._rollout_plant = plant
        return simulate.rollout_implicit(self.__oracle, plant, X0, T, d=d, v=v, record=record,
                                         tol_exit=tol_exit, noise=noise, seed=seed, traj0=traj0,
                                         on_device=on_device)

    def evaluate(self, X):
        """Inputs for a batch of states (n, p) -> (n, n_u); NaN rows where infeasible."""
        J, u0, didx = self.__oracle.gpu.solve_pt(np.asarray(X, dtype=np.float64))
        u0 = u0.copy()
        u0[didx < 0] = np.nan
        return u0


class ExplicitMPC:
    """GPU counterpart of lib/mpc_library.py:662-792 (same constructor and call signature)."""

    # class defaults: rollout checks its arguments before it touches anything else
    mpc = None
    _rollout_plant = None       # the plant the device holds (set_plant)
    _input_scale = None         # audit_applied: the default input_tol (built on first use)

    def __init__(self, tree, oracle=None, device=0):
        mpc = getattr(oracle, 'mpc', None)
        self.mpc = mpc
        self.plant = getattr(mpc, 'plant', None)
        self.T_s = getattr(mpc, 'T_s', None)
        if hasattr(mpc, 'specs'):
            self.specs = mpc.specs
        self.tree = tree
        self._oracle = oracle       # audit: P_theta of the oracle the law was built with
        self._cells = None          # audit, sample: the leaves as cells (built on first use)
        self._costs_set = False
        self.device = int(device)
        self._lib = _capi.load()
        self._handle = ctypes.c_void_p()
        self.setup()

    def setup(self):
        """Readies the evaluator: flat arrays + simplex basis inverses on the device."""
        if isinstance(self.tree, FlatTree):
            t = self.tree
            vertices, vinput = f64(t.vertices), f64(t.vertex_inputs)
            left = np.ascontiguousarray(t.left, dtype=np.int32)
            right = np.ascontiguousarray(t.right, dtype=np.int32)
            n_roots = int(t.info['n_roots'])
            self.nodes = None
        else:
            vertices, vinput, left, right, self.nodes, self._commutations = flatten_tree(
                self.tree, commutations=True)
            n_roots = 1
        self.n_nodes, self.p, self.n_u = vertices.shape[0], vertices.shape[2], vinput.shape[2]
        self.eps = np.finfo(np.float64).eps
        self._costs_set = False     # a new handle holds no costs yet
        _check(self._lib.ehm_explicit_create(self.device, self.n_nodes, n_roots, self.p, self.n_u,
                                             ptr(left), ptr(right), ptr(vertices), ptr(vinput),
                                             ctypes.byref(self._handle)))

    def compile(self, dtype=np.float64, spine='tests', flush=False, reduce=None):
        """The law as a ``compiled.CompiledLaw``: one hyperplane per internal node, one affine map
        per leaf, compiled on the device.  It holds its own arrays and outlives this object.  For
        its rollouts it remembers ``mpc`` (the default plant) and, where ``mpc`` tells the step-0
        mode of a commutation, the mode of every leaf (``CompiledLaw.leaf_mode``).
        ``dtype=np.float32``: the law in single precision (``CompiledLaw.to_single``), with
        ``flush=True`` its values below the normal range of a float set to zero instead of
        refused.  ``spine='roots'``: the data-less spine of a nested tree becomes the law's root
        table instead of test nodes (``CompiledLaw.compile``).  ``reduce``: a tolerance (a scalar
        or [n_u]), or True for the default one: the law with the leaves that apply one affine map
        within it merged (``CompiledLaw.reduce``), in the precision asked for."""
        from .compiled import CompiledLaw
        dtype = np.dtype(dtype).type
        if dtype not in (np.float64, np.float32):
            raise ValueError('dtype must be np.float64 or np.float32')
        if spine not in ('tests', 'roots'):
            raise ValueError("spine must be 'tests' or 'roots'")
        if flush and dtype is np.float64:
            raise ValueError('flush=True narrows the law: it needs dtype=np.float32')
        vertices = self.tree.vertices if isinstance(self.tree, FlatTree) else \
            flatten_tree(self.tree)[0]
        law = CompiledLaw.compile(self, vertices, spine=spine)
        law.mpc = self.mpc
        if self.mpc is not None and hasattr(self.mpc, 'step0_mode'):
            law.set_leaf_modes(self._step0_modes()[law.leaf_node])
        if dtype is np.float32:
            double = law
            try:
                law = double.to_single(flush=bool(flush))
            finally:
                double.close()
        if reduce is not None and reduce is not False:
            full = law
            try:
                law = full.reduce(tol=None if reduce is True else reduce)
            finally:
                full.close()
        return law

    def close(self):
        if getattr(self, '_handle', None):
            self._lib.ehm_explicit_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, X, return_info=False):
        """u [n, n_u] for the states X [n, p]; with return_info also (leaf ids, tests, seconds)."""
        X = f64(np.atleast_2d(X))
        n = X.shape[0]
        u = np.empty((n, self.n_u))
        leaf = np.empty(n, dtype=np.int32)
        visited = np.empty(n, dtype=np.int32)
        secs = ctypes.c_double(0.)
        _check(self._lib.ehm_explicit_eval_batch(self._handle, n, ptr(X), ptr(u), ptr(leaf),
                                                 ptr(visited), ctypes.addressof(secs)))
        if return_info:
            return u, leaf, visited, secs.value
        return u

    # -- uniform sampling and the audit of the epsilon-suboptimality contract --
    def cells(self):
        """
        The leaves as the sampler's cells: dict of ``node`` int32 [n_cells] (their node ids as
        ``evaluate`` reports leaves), ``vertices`` [n_cells, p+1, p], ``volume`` [n_cells]
        (``ehm_volume_batch``), ``cdf`` (its running sum), ``closed`` bool [n_cells], and the
        per-node ``vertex_costs`` [n_nodes, p+1] and ``flags`` uint8 [n_nodes].  A flat forest's
        cells are its leaves in ascending node id; a nested tree's are its leaves that hold a
        simplex, in the same order (``forest_order``), so both forms of one partition draw the
        same points.
        """
        if self._cells is not None:
            return self._cells
        from . import engine
        if isinstance(self.tree, FlatTree):
            t = self.tree
            vertices, vcost = f64(t.vertices), f64(t.vertex_costs)
            flags = np.ascontiguousarray(t.flags, dtype=np.uint8)
            node = np.nonzero(np.asarray(t.left) < 0)[0]
        else:
            vertices, _, left, right, _, extra = flatten_tree(self.tree, costs=True)
            vcost, flags = extra['vertex_costs'], extra['flags']
            order = forest_order(left, right, ~extra['simplex'])
            node = order[(left[order] < 0) & extra['simplex'][order]]
        node = np.ascontiguousarray(node, dtype=np.int32)
        if node.size == 0:
            raise ValueError('the tree has no leaf to sample')
        cv = f64(vertices[node])
        vol = engine.volume_batch(cv, device=self.device)
        self._cells = dict(node=node, vertices=cv, volume=vol, cdf=f64(np.cumsum(vol)),
                           closed=(flags[node] & 1).astype(bool), vertex_costs=f64(vcost),
                           flags=flags)
        return self._cells

    def _audit_opts(self, n, seed, mode, per_leaf, first, chunk):
        """(AuditOpts, n) for the sampler's arguments; the cells' arrays stay alive in cells()."""
        if not getattr(self, '_handle', None):
            raise ValueError('the law is closed')
        if mode is None:
            mode = 'uniform' if per_leaf is None else 'per_leaf'
        if mode not in _capi.EHM_AUDIT_MODES:
            raise ValueError("mode must be 'uniform' or 'per_leaf', not %r" % (mode,))
        first = int(first)
        if first < 0:
            raise ValueError('first must be >= 0')
        cells = self.cells()
        n_cells = cells['node'].size
        if mode == 'per_leaf':
            if per_leaf is None or int(per_leaf) < 1:
                raise ValueError("mode 'per_leaf' needs per_leaf >= 1")
            total = n_cells * int(per_leaf)
            if n is None:
                n = total - first
            if n < 0 or first + n > total:
                raise ValueError('per-leaf ids end at leaves x per_leaf = %d' % total)
        else:
            if per_leaf is not None:
                raise ValueError("per_leaf goes with mode 'per_leaf'")
            if n is None or int(n) < 0:
                raise ValueError("mode 'uniform' needs n >= 0")
        opts = _capi.AuditOpts(mode=_capi.EHM_AUDIT_MODES[mode], k=int(per_leaf or 0), n=int(n),
                               first=first, seed=int(seed) & ((1 << 64) - 1), n_cells=n_cells,
                               cell_vertices=ptr(cells['vertices']), cell_node=ptr(cells['node']),
                               cdf=ptr(cells['cdf']), chunk=int(chunk))
        return opts, int(n)

    def sample(self, n=None, seed=0, mode=None, per_leaf=None, first=0, chunk=0):
        """
        Points of the partitioned set drawn on the device (k_audit_sample): X [n, p] and the cell
        [n] (index into ``cells()``) each was drawn in.  ``mode='uniform'``: uniform in the set --
        a cell chosen by volume, a uniform point in it; ``mode='per_leaf'`` with ``per_leaf=k``:
        exactly k uniform points in every leaf, sample s in cell s // k (n defaults to all of them).
        Sample ids are global, ``first`` .. ``first + n - 1``: a point depends on (seed, id) only,
        not on n, ``chunk`` (samples per launch) or how a range of ids is split over calls.
        """
        opts, n = self._audit_opts(n, seed, mode, per_leaf, first, chunk)
        X = np.empty((n, self.p))
        cell = np.empty(n, dtype=np.int32)
        _check(self._lib.ehm_explicit_sample(self._handle, ctypes.byref(opts), ptr(X), ptr(cell)))
        return X, cell

    def records(self):
        """[n_nodes, p + p p]: [v_0 | inv([v_1 - v_0 .. v_p - v_0])] of every node as the device
        holds them (what a host mirror of the weights needs)."""
        rec = np.empty((self.n_nodes, self.p + self.p * self.p))
        _check(self._lib.ehm_explicit_records(self._handle, ptr(rec)))
        return rec

    def audit(self, n=None, seed=0, mode=None, per_leaf=None, rtol=1e-7, return_samples=False,
              oracle=None, allow_open=False, first=0, chunk=0):
        """
        Samples the partitioned set as ``sample`` does and checks the law's contract at every
        point:  0 <= Vbar(x) - V*(x) <= max(eps_a, eps_r V*(x)),  Vbar the interpolated vertex
        costs of the leaf the deployed walk ends in, V* the optimal cost ``P_theta(x)`` of
        ``oracle`` (default: the one the law was built with), each side with the slack
        rtol (1 + |V*|).  Give ``n`` (uniform) or ``per_leaf``, not both.  ``allow_open``: leaves
        left open by a depth limit do not fail ``passed``.  ``first``: id of the first sample (a
        shard audits its range of ids); ``chunk``: samples per pass (the length of the P_theta
        batches; no result depends on it).  ``return_samples``: the per-sample arrays too.
        Raises ValueError without an oracle and EhmError for an oracle without a batched P_theta
        (branch and bound over mode prefixes).  Returns an ``AuditResult``.  A sampled check, not
        a certificate.
        """
        oracle = self._oracle if oracle is None else oracle
        if oracle is None:
            raise ValueError('audit needs an oracle: the law was built without one')
        if n is not None and per_leaf is not None:
            raise ValueError('per_leaf fixes the number of samples (leaves x per_leaf): give n or '
                             'per_leaf, not both')
        opts, n = self._audit_opts(n, seed, mode, per_leaf, first, chunk)
        gp = getattr(oracle, 'gpu', None)
        if gp is None:
            raise _capi.EhmError(_capi.EHM_E_INVALID, 'audit needs the batched P_theta of an '
                                 'enumerating oracle; this one (branch and bound over mode '
                                 'prefixes) has none')
        if gp.can.p != self.p:
            raise ValueError('the oracle has parameter dimension %d, the law %d' % (gp.can.p,
                                                                                   self.p))
        cells = self.cells()
        if not self._costs_set:
            _check(self._lib.ehm_explicit_set_costs(self._handle, ptr(cells['vertex_costs']),
                                                    ptr(cells['flags'])))
            self._costs_set = True
        opts.rtol, opts.eps_a, opts.eps_r = float(rtol), float(oracle.eps_a), float(oracle.eps_r)
        res = _capi.AuditResult()
        arrays = {}
        smp = None
        if return_samples:
            arrays = dict(x=np.empty((n, self.p)), cell=np.empty(n, np.int32),
                          leaf=np.empty(n, np.int32), vbar=np.empty(n), wmin=np.empty(n),
                          vstar=np.empty(n), delta_idx=np.empty(n, np.int32),
                          status=np.empty(n, np.int32))
            smp = ctypes.byref(_capi.AuditSamples(**{k: ptr(a) for k, a in arrays.items()}))
        _check(self._lib.ehm_explicit_audit(self._handle, gp._handle, ctypes.byref(opts),
                                            ctypes.byref(res), smp))
        worst = None
        if res.worst_id >= 0:
            worst = dict(id=int(res.worst_id), x=np.array(res.worst_x[:self.p]),
                         cell=int(res.worst_cell), leaf=int(res.worst_leaf),
                         vbar=res.worst_vbar, vstar=res.worst_vstar, bound=res.worst_bound)
        vol = cells['volume']
        return AuditResult(n=n, counts={name: int(res.counts[k])
                                        for k, name in enumerate(STATUS_NAMES)},
                           relocated=int(res.relocated), max_ratio=float(res.max_ratio),
                           worst=worst, histogram=np.array(res.histogram[:], dtype=np.int64),
                           open_volume_fraction=float(vol[~cells['closed']].sum() / vol.sum()),
                           allow_open=bool(allow_open), rtol=float(rtol),
                           seconds=tuple(res.seconds[:]), **arrays)

    def audit_applied(self, n=None, seed=0, mode=None, per_leaf=None, rtol=1e-7, input_tol=None,
                      return_samples=False, oracle=None, first=0, chunk=0):
        """
        The judgement of ``CompiledLaw.audit`` (applied.py) for this law: at the
        points of ``sample`` (same arguments, so ``per_leaf`` works) the input of
        ``evaluate`` is priced by P_theta with the first input fixed to it, against V* =
        P_theta(x).  ``input_tol`` None: 1e-7 max(1, largest |u| of the leaves' vertex inputs).
        Returns an ``applied.AppliedAuditResult`` (``root`` is -1: the points were drawn in the
        leaves, ``sample`` tells in which).
        """
        from . import applied
        oracle = self._oracle if oracle is None else oracle
        if oracle is None:
            raise ValueError('audit_applied needs an oracle: the law was built without one')
        if n is not None and per_leaf is not None:
            raise ValueError('per_leaf fixes the number of samples (leaves x per_leaf): give n or '
                             'per_leaf, not both')
        applied.oracle_gpu(oracle)
        if self.p + self.n_u > _capi.EHM_MAX_P:
            raise ValueError('the applied-input problem adds one parameter per input: p + n_u = '
                             '%d exceeds EHM_MAX_P = %d' % (self.p + self.n_u, _capi.EHM_MAX_P))
        X, _ = self.sample(n=n, seed=seed, mode=mode, per_leaf=per_leaf, first=first, chunk=chunk)
        if input_tol is None:
            if self._input_scale is None:
                t = self.tree
                if isinstance(t, FlatTree):
                    vin = np.asarray(t.vertex_inputs)[np.asarray(t.left) < 0]
                else:
                    _, vin, left, _, _ = flatten_tree(t)
                    vin = vin[left < 0]
                self._input_scale = applied.default_input_tol(vin)
            input_tol = self._input_scale
        res = applied.run(oracle, self.p, self.n_u, self.device, input_tol, source=self._handle,
                          X=X, rtol=rtol, return_samples=return_samples, first=first, chunk=chunk)
        return res

    def certify_applied(self, oracle=None, spine='roots', dtype=np.float64, flush=False, **kw):
        """
        ``CompiledLaw.certify`` (certify.py) for this law: compiles it
        (``compile(spine=spine, dtype=dtype, flush=flush)``) and certifies the compiled law leaf
        by leaf against ``oracle`` (default: the one the law was built with); ``kw`` as
        ``CompiledLaw.certify``.  Returns its ``certify.CertificateResult``.
        """
        oracle = self._oracle if oracle is None else oracle
        if oracle is None:
            raise ValueError('certify_applied needs an oracle: the law was built without one')
        law = self.compile(dtype=dtype, spine=spine, flush=flush)
        try:
            return law.certify(oracle, **kw)
        finally:
            law.close()

    def successors(self, spine='roots', dtype=np.float64, flush=False, **kw):
        """
        ``CompiledLaw.successors`` (invariance.py) for this law: compiles it
        (``compile(spine=spine, dtype=dtype, flush=flush)``) and asks where its input sends every
        leaf; ``kw`` as ``CompiledLaw.successors``.  Returns its ``invariance.SuccessorResult``.
        """
        law = self.compile(dtype=dtype, spine=spine, flush=flush)
        try:
            return law.successors(**kw)
        finally:
            law.close()

    def invariant_core(self, spine='roots', dtype=np.float64, flush=False, **kw):
        """
        ``CompiledLaw.invariant_core`` (invariance.py) for this law: compiles it
        (``compile(spine=spine, dtype=dtype, flush=flush)``) and finds the leaves the closed loop
        never leaves; ``kw`` as ``CompiledLaw.invariant_core``.  Returns its
        ``invariance.CoreResult``, whose ``contains`` needs the compiled law and is not available
        here.
        """
        law = self.compile(dtype=dtype, spine=spine, flush=flush)
        try:
            res = law.invariant_core(**kw)
            res._law = None
            return res
        finally:
            law.close()

    def robust_successors(self, spine='roots', dtype=np.float64, flush=False, **kw):
        """
        ``CompiledLaw.robust_successors`` (robust.py) for this law: compiles it
        (``compile(spine=spine, dtype=dtype, flush=flush)``) and asks where its input sends every
        leaf under measurement and input error; ``kw`` as ``CompiledLaw.robust_successors``
        (``radii='leaf'``, ``radius_iters``: the per-leaf boxes of DESIGN.md 3.8k).
        Returns its ``robust.RobustSuccessorResult``.
        """
        law = self.compile(dtype=dtype, spine=spine, flush=flush)
        try:
            return law.robust_successors(**kw)
        finally:
            law.close()

    def robust_core(self, spine='roots', dtype=np.float64, flush=False, **kw):
        """
        ``CompiledLaw.robust_core`` (robust.py) for this law: compiles it
        (``compile(spine=spine, dtype=dtype, flush=flush)``) and finds the leaves the noisy closed
        loop never leaves; ``kw`` as ``CompiledLaw.robust_core`` (``radii``, ``radius_iters``
        included).  Returns its
        ``invariance.CoreResult``, whose ``contains`` needs the compiled law and is not available
        here.
        """
        law = self.compile(dtype=dtype, spine=spine, flush=flush)
        try:
            res = law.robust_core(**kw)
            res._law = None
            return res
        finally:
            law.close()

    def node_modes(self, plant):
        """int32 [n_nodes]: step-0 mode of every node's commutation (-1: none); all 0 for a
        single-mode plant."""
        if plant.n_modes == 1 and not plant.guarded:
            return np.zeros(self.n_nodes, dtype=np.int32)
        if self.mpc is None or not hasattr(self.mpc, 'step0_mode'):
            raise ValueError('the step-0 modes of a hybrid law need the oracle (its mpc)')
        return self._step0_modes()

    def _step0_modes(self):
        """int32 [n_nodes]: step-0 mode of every node's commutation (-1: none), from ``mpc``."""
        if isinstance(self.tree, FlatTree):
            modes = np.array([self.mpc.step0_mode(dl) for dl in self.tree.deltas] + [-1],
                             dtype=np.int32)
            didx = np.asarray(self.tree.delta_idx)
            return np.ascontiguousarray(np.where(didx >= 0, modes[didx], -1), dtype=np.int32)
        return np.array([-1 if c is None else self.mpc.step0_mode(c)
                         for c in self._commutations], dtype=np.int32)

    def set_plant(self, plant):
        """Hands the plant the rollout closes the loop around to the device (once per plant)."""
        if plant.n_x != self.p or plant.n_u != self.n_u:
            raise ValueError('plant (n_x %d, n_u %d) does not fit the law (p %d, n_u %d)' % (
                plant.n_x, plant.n_u, self.p, self.n_u))
        self._node_mode = self.node_modes(plant)
        opt = lambda a: ptr(a) if a.size else None
        A, B, w, Gx, gx, Q, R = (f64(a) for a in (plant.A, plant.B, plant.w, plant.Gx, plant.gx,
                                                  plant.Q, plant.R))
        if plant.guarded:
            gm, row0, ga, gb, gc, gt, st = plant.guard_arrays()
            ga, gb, gc, gt = f64(ga), f64(gb), f64(gc), f64(gt)
            fn = self._lib.ehm_explicit_set_plant_guarded
            own = (plant.substeps, len(gm), opt(gm), ptr(row0), opt(ga), opt(gb), opt(gc), opt(gt),
                   opt(st), plant.default_mode)
        else:
            rows, H, h = plant.region_arrays()
            E, H, h = f64(plant.E), f64(H), f64(h)
            fn = self._lib.ehm_explicit_set_plant
            own = (plant.n_d, opt(E), ptr(rows), opt(H), opt(h))
        _check(fn(self._handle, plant.n_modes, ptr(A), ptr(B), ptr(w), *own, plant.gx.size, opt(Gx),
                  opt(gx), ptr(self._node_mode), 0 if plant.cost == 'inf' else 1, ptr(Q), ptr(R)))
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
        _check(self._lib.ehm_explicit_set_noise(self._handle, desc.shape[0], ptr(desc),
                                                ptr(data) if data.size else None, data.size,
                                                plant.n_d))
        self._noise_packed = (desc, data, plant.n_d)

    def rollout(self, X0, T, d=None, v=None, record=True, tol_exit=1e-9, plant=None, noise=None,
                seed=0, traj0=0):
        """
        Closed loop from the states X0 [n, p] for T steps in ONE kernel launch
        (ehm_explicit_rollout, one device thread per trajectory; conventions in simulate.py).
        ``plant`` defaults to ``Plant.from_mpc`` of the oracle's law; d [T, n, n_d] and
        v [T, n, p] are optional.  With ``noise`` (a ``noise.NoiseModel``, not together with d
        or v) the kernel draws v, e and d itself (ehm_explicit_rollout_noisy, Philox key seed,
        trajectory q has id traj0 + q).  A ``simulate.GuardedPlant`` (the default for a law that
        has one, e.g. the pendulum) is held at u for its substeps per step and picks its own modes
        (its instantiation of the kernel); it takes neither noise nor d.  Returns a
        ``simulate.ClosedLoop`` (leaf, commutation, mode -- None for a guarded plant -- and v, e, w
        under noise, recorded with ``record``).
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
            fn = self._lib.ehm_explicit_rollout
            head = (ptr(d), ptr(v), float(tol_exit), ptr(xs), ptr(us), ptr(leaf))
        else:
            vs, es, ws = rec((T, n, p)), rec((T, n, self.n_u)), rec((T, n, plant.n_d))
            fn = self._lib.ehm_explicit_rollout_noisy
            head = (int(seed), int(traj0), float(tol_exit), ptr(xs), ptr(us), ptr(leaf), ptr(vs),
                    ptr(es), ptr(ws))
        _check(fn(self._handle, n, T, ptr(X0), *head, ptr(x_final), ptr(steps), ptr(status),
                  ptr(cost), ptr(unorm), ptr(maxv), ctypes.addressof(secs)))
        out = simulate.ClosedLoop(x_final=x_final, steps=steps, status=status, cost=cost,
                                  u_norm_sum=unorm, max_violation=maxv, seconds=secs.value,
                                  x=xs, u=us, leaf=leaf, v=vs, e=es, w=ws)
        if record:
            live = leaf >= 0
            if not plant.guarded:
                out.mode = np.where(live, self._node_mode[np.maximum(leaf, 0)],
                                    -1).astype(np.int32)
            if isinstance(self.tree, FlatTree):
                didx = np.asarray(self.tree.delta_idx, dtype=np.int32)
                out.commutation = np.where(live, didx[np.maximum(leaf, 0)], -1).astype(np.int32)
        return out

    def get_containing_cell(self, x):
        """NodeData of the leaf that contains x (nested trees), or its node index (FlatTree)."""
        _, leaf, _, _ = self.evaluate(np.asarray(x, dtype=np.float64)[None], return_info=True)
        k = int(leaf[0])
        return self.nodes[k].data if self.nodes is not None else k

    def __call__(self, x):
        """Epsilon-suboptimal input for state x and the evaluation time (lib/mpc_library.py:769)."""
        tic = time.time()
        u = self.evaluate(np.asarray(x, dtype=np.float64)[None])[0]
        return u, time.time() - tic
