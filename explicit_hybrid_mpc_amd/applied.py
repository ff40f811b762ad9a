"""
Audit of a law by the cost of the input it applies (csrc/ehm_applied.hip):

    res = law.audit(oracle, n=100000)             # CompiledLaw, double or single, also a loaded one
    res = explicit.audit_applied(n=100000)        # the same judgement for the source law

At a state x the law applies ubar = law(x).  What that input costs is the optimum of the
fixed-first-input problem, P_theta with u_0 = ubar:

    V_u(x) = min over commutations and the rest z_r of the decision  V([ubar ; z_r], x) .

Substituting u_0 = ubar into the canonical form gives again a canonical form
(``applied_input_problem``): n - n_u columns and p + n_u parameters theta' = (x, ubar), exactly, for
LP and for quadratic costs -- so the batched P_theta kernels solve it as they solve P_theta.
``input_tol`` is the distance (infinity norm) an input may be moved to be admitted: V_u comes from
the exact substitution wherever a commutation of it is feasible, and only where none is from the
problem relaxed by ``input_tol`` -- so the relaxation admits an input that overshoots a row by its
rounding (a single law) and never lowers the cost of an input that is admissible as it stands.  The
audit judges  0 <= V_u(x) - V*(x) <= max(eps_a, eps_r V*(x))  per point.  By convexity of V_delta
the interpolated input costs at most the interpolated vertex costs, V_u <= Vbar: this audit is the
tighter one, and the only one for a law that keeps no costs.  A sampled check;
``CompiledLaw.certify`` (certify.py) is the statement for every state of a leaf.
"""

import ctypes

import numpy as np

from . import _capi
from ._capi import f64, ptr
from .mpc_library import CanonicalLP

STATUS_NAMES = ('within', 'violation', 'negative', 'inadmissible', 'no_law', 'infeasible')
INPUT_TOL_FACTOR = 1e-7     # a hundred solver tolerances (lexicographic.TOL, audit's rtol)


_check = _capi.checker('ehm_applied_last_error')


def applied_input_problem(can, input_tol=0.):
    """
    The canonical form of P_theta with the first input fixed: with z = [u_0 ; z_r] and
    theta' = (theta, ubar) a ``CanonicalLP`` with n - n_u columns and p + n_u parameters,

        G' = G[:, :, n_u:],   S' = [S | -G[:, :, :n_u]],   w' = w + input_tol sum_j<n_u |G[:, :, j]|,
        c' = c[n_u:],

    and for a quadratic form (r the columns from n_u on, u those before; H symmetrised as the
    library does)  H' = H_rr, F' = [F_r | H_ru], f0' = f0_r, C' = [[C, F_u^T], [F_u, H_uu]],
    c1' = [c1 | f0_u + c_u], c0' = c0.  ``deltas``, ``N`` and ``delta_size`` stay.

    The cost of u_0 the form does not hold is ``cost_u`` [n_u] of the result: V([ubar ; z_r], theta)
    = V'(z_r, theta') + cost_u . ubar.  For an LP cost it is c[:n_u]; for a quadratic cost c[:n_u]
    is part of c1' and cost_u is zero.

    ``input_tol`` > 0 RELAXES the problem: every row is widened by what an input within input_tol
    of ubar (infinity norm) could gain on it, input_tol times the 1-norm of the row's u_0 part, so
    exactly the rows that touch u_0 move.  The optimum of the relaxed problem is at most that of
    the exact substitution (input_tol = 0), and an input it admits may violate a row by that
    much.

    Rows on u_0 alone, and on x_1 alone, have no entry left in G': they read 0 <= w'_i + S'_i
    theta'.  They stay in the problem -- every kernel family takes such rows, as it takes the
    rows 0 <= 1 that pad a commutation and the mode regions of step 0 of a hybrid form.

    ``n_u`` of the result is 1: the library returns z[:n_u] of a solve as its first input, which
    here is the first of the remaining columns and means nothing; nobody reads it.

    ``ValueError`` for p + n_u > EHM_MAX_P, and for a form that has no column besides u_0.
    """
    p, n_u = can.p, can.n_u
    if p + n_u > _capi.EHM_MAX_P:
        raise ValueError('the applied-input problem adds one parameter per input: p + n_u = %d '
                         'exceeds EHM_MAX_P = %d' % (p + n_u, _capi.EHM_MAX_P))
    if can.n <= n_u:
        raise ValueError('the form has no column besides u_0: nothing is left to solve for')
    input_tol = float(input_tol)
    if not input_tol >= 0.:
        raise ValueError('input_tol must be >= 0')
    Gu = can.G[:, :, :n_u]
    G = can.G[:, :, n_u:]
    S = np.concatenate([can.S, -Gu], axis=2)
    w = can.w + input_tol * np.abs(Gu).sum(axis=2)
    quad = None
    cost_u = np.array(can.c[:n_u])
    if getattr(can, 'quadratic', False):
        H = 0.5 * (can.H + np.transpose(can.H, (0, 2, 1)))
        Fu = can.F[:, :n_u]
        top = np.concatenate([can.C, np.transpose(Fu, (0, 2, 1))], axis=2)
        bottom = np.concatenate([Fu, H[:, :n_u, :n_u]], axis=2)
        quad = dict(H=H[:, n_u:, n_u:], F=np.concatenate([can.F[:, n_u:], H[:, n_u:, :n_u]], axis=2),
                    f0=can.f0[:, n_u:], C=np.concatenate([top, bottom], axis=1),
                    c1=np.concatenate([can.c1, can.f0[:, :n_u] + can.c[None, :n_u]], axis=1),
                    c0=can.c0)
        cost_u = np.zeros(n_u)
    out = CanonicalLP(G, w, S, can.c[n_u:], can.deltas, 1, can.N, can.delta_size, quad=quad)
    out.cost_u = f64(cost_u)
    out.input_tol = input_tol
    return out


def default_input_tol(U):
    """INPUT_TOL_FACTOR max(1, largest finite |u| in U)."""
    U = np.abs(np.asarray(U, dtype=np.float64))
    U = U[np.isfinite(U)]
    return INPUT_TOL_FACTOR * max(1., float(U.max()) if U.size else 0.)


def oracle_gpu(oracle):
    """The batched P_theta of an oracle; ``EhmError`` for an oracle without one."""
    gp = getattr(oracle, 'gpu', None)
    if gp is None:
        raise _capi.EhmError(_capi.EHM_E_INVALID, 'the audit needs the batched P_theta of an '
                             'enumerating oracle; this one (branch and bound over mode '
                             'prefixes) has none')
    return gp


def applied_gpu(oracle, input_tol):
    """The applied-input problem of ``oracle`` at ``input_tol`` on the oracle's device, an
    ``engine.GpuProblem``.  The oracle's ``GpuProblem`` owns it and closes it with itself; it
    keeps the exact substitution (input_tol = 0) and the relaxed problem last asked for -- another
    ``input_tol`` closes that one and takes its place."""
    from .engine import GpuProblem
    gp = oracle_gpu(oracle)
    if gp._applied is None:
        gp._applied = {}
    held = gp._applied
    key = float(input_tol)
    if key not in held:
        for other in [k for k in held if k != 0.]:
            held.pop(other).close()
        held[key] = GpuProblem(applied_input_problem(gp.can, key), gp.eps_a, gp.eps_r,
                               device=gp.device)
    return held[key]


def root_cells(law):
    """
    The roots of a compiled law as the sampler's cells: dict of ``vertices`` [n_roots, p+1, p],
    ``volume`` (``ehm_volume_batch``) and ``cdf`` (its running sum).  The vertices are recovered on
    the host from the law's root records [v_0 | inv(E)], E = [v_1 - v_0 .. v_p - v_0]: v_i = v_0 +
    column i of inv(inv(E)) -- from the arrays alone, so a law compiled in this process and the
    same law loaded from its file give the same cells bit for bit.
    """
    from . import engine
    p = law.p
    rec = f64(law.array('root_rec'))[:, :p + p * p]
    v0 = rec[:, :p]
    E = np.linalg.inv(rec[:, p:].reshape(-1, p, p))         # columns: v_i - v_0
    V = np.concatenate([v0[:, None, :], v0[:, None, :] + np.transpose(E, (0, 2, 1))], axis=1)
    V = f64(V)
    vol = engine.volume_batch(V, device=law.device)
    return dict(vertices=V, volume=vol, cdf=f64(np.cumsum(vol)))


class AppliedAuditResult:
    """
    What ``CompiledLaw.audit`` / ``ExplicitMPC.audit_applied`` found (a sampled
    check -- ``CompiledLaw.certify`` is the certificate): ``counts`` samples by status name
    (STATUS_NAMES), ``max_ratio`` the
    largest (V_u - V*) / bound over statuses 0-2 (-inf if there is none), ``worst`` that sample
    (id, x, leaf, u, vu, vstar, bound; None if there is none), ``histogram`` int64 [33] of the
    ratio (32 bins over [0, 1], one above), ``seconds`` (sampling kernel, evaluation kernel, pack
    and reduce kernels, the P_theta batches, the applied-input batches), ``n``, ``input_tol``,
    ``n_relaxed`` the samples whose input is admissible only within ``input_tol`` (their V_u is the
    relaxed problem's), and with ``return_samples`` the arrays ``x, root, leaf, u, vu, vstar,
    delta_idx, delta_idx_applied, status, relaxed``.  ``passed``: every sample is within the
    contract.
    """

    def __init__(self, **kw):
        self.x = self.root = self.leaf = self.u = self.vu = self.vstar = None
        self.delta_idx = self.delta_idx_applied = self.status = self.relaxed = None
        self.__dict__.update(kw)

    @property
    def passed(self):
        return self.counts['within'] == self.n

    def __repr__(self):
        return 'AppliedAuditResult(n=%d, passed=%s, counts=%r, max_ratio=%.6g, input_tol=%.3g, ' \
            'n_relaxed=%d)' % (self.n, self.passed, self.counts, self.max_ratio, self.input_tol,
                               self.n_relaxed)


def run(oracle, p, n_u, device, input_tol, law=None, source=None, X=None, U=None, cells=None,
        n=None, seed=0, rtol=1e-7, return_samples=False, first=0, chunk=0):
    """
    The one path to ``ehm_compiled_audit``.  The input comes from ``law`` (a compiled handle), else
    from ``source`` (an explicit handle), else from ``U`` [n, n_u]; the points are ``X`` [n, p] or n
    points drawn in ``cells`` (``root_cells``).  Returns an ``AppliedAuditResult``.
    """
    gp = oracle_gpu(oracle)
    if gp.can.p != p or gp.can.n_u != n_u:
        raise ValueError('the oracle has p = %d, n_u = %d, the law %d, %d' % (
            gp.can.p, gp.can.n_u, p, n_u))
    if (n is None) == (X is None):
        raise ValueError('give n (points drawn in the law\'s set) or X, not both')
    first = int(first)
    if first < 0:
        raise ValueError('first must be >= 0')
    input_tol = float(input_tol)
    ap = applied_gpu(oracle, 0.)
    relaxed = applied_gpu(oracle, input_tol) if input_tol > 0. else None
    opts = _capi.AppliedOpts(first=first, seed=int(seed) & ((1 << 64) - 1), chunk=int(chunk),
                             p=p, n_u=n_u, device=int(device), rtol=float(rtol),
                             eps_a=float(oracle.eps_a), eps_r=float(oracle.eps_r),
                             cost_u=ptr(ap.can.cost_u), source=source,
                             relaxed=None if relaxed is None else relaxed._handle)
    keep = []
    if X is not None:
        X = f64(np.atleast_2d(X))
        if X.shape[1] != p:
            raise ValueError('X must be [n, %d]' % p)
        n = X.shape[0]
        opts.x = ptr(X)
        keep.append(X)
    else:
        n = int(n)
        if n < 0:
            raise ValueError('n must be >= 0')
        opts.n_cells = cells['vertices'].shape[0]
        opts.cell_vertices, opts.cdf = ptr(cells['vertices']), ptr(cells['cdf'])
    if law is None and source is None:
        U = f64(np.atleast_2d(U))
        if U.shape != (n, n_u):
            raise ValueError('U must be [%d, %d]' % (n, n_u))
        opts.u = ptr(U)
        keep.append(U)
    opts.n = n
    res = _capi.AppliedResult()
    arrays, smp = {}, None
    if return_samples:
        i4 = lambda: np.empty(n, np.int32)
        arrays = dict(x=np.empty((n, p)), root=i4(), leaf=i4(), u=np.empty((n, n_u)),
                      vu=np.empty(n), vstar=np.empty(n), delta_idx=i4(), delta_idx_applied=i4(),
                      status=i4(), relaxed=i4())
        smp = ctypes.byref(_capi.AppliedSamples(**{k: ptr(a) for k, a in arrays.items()}))
    _check(_capi.load().ehm_compiled_audit(law, gp._handle, ap._handle, ctypes.byref(opts),
                                           ctypes.byref(res), smp))
    worst = None
    if res.worst_id >= 0:
        worst = dict(id=int(res.worst_id), x=np.array(res.worst_x[:p]), leaf=int(res.worst_leaf),
                     u=np.array(res.worst_u[:n_u]), vu=res.worst_vu, vstar=res.worst_vstar,
                     bound=res.worst_bound)
    return AppliedAuditResult(n=n, counts={name: int(res.counts[k])
                                           for k, name in enumerate(STATUS_NAMES)},
                              max_ratio=float(res.max_ratio), worst=worst,
                              n_relaxed=int(res.relaxed),
                              histogram=np.array(res.histogram[:], dtype=np.int64),
                              seconds=tuple(res.seconds[:]), rtol=float(rtol),
                              input_tol=float(input_tol), **arrays)


def audit_inputs(oracle, X, U, rtol=1e-7, input_tol=None, return_samples=False, chunk=0,
                 device=None):
    """The judgement for inputs of the caller's: U [n, n_u] applied at the states X [n, p]
    (``input_tol`` None: ``default_input_tol(U)``)."""
    gp = oracle_gpu(oracle)
    U = f64(np.atleast_2d(U))
    if input_tol is None:
        input_tol = default_input_tol(U)
    return run(oracle, gp.can.p, gp.can.n_u, gp.device if device is None else device, input_tol,
               X=X, U=U, rtol=rtol, return_samples=return_samples, chunk=chunk)
