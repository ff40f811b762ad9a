"""
The reference's uncertainty model (lib/uncertainty_sets.py ``UncertaintySet``) as data, sampled
by a counter-based generator so that the device rollout and the host agree draw for draw.

    model = NoiseModel.from_mpc(SatelliteZ(4))            # the six terms the law was tightened for
    v = model.sample('state', seed, traj_ids, t, x, u)    # [n, n_x], vectorised over trajectories

Terms, in model order, each of a kind 'process' (-> the plant's d), 'state' (-> the measurement
error v) or 'input' (-> the input error e):
  box   (addIndependentTerm): c + h * s, mapped by M [out, dim];
  ball  (addDependentTerm):   uniform in {||q||_norm <= radius}, mapped by L [out, dim];
        radius = sigma, sigma ||Fx x||_px (x the TRUE state) or sigma ||Fu u||_pu.
A kind's draw is the sum of its terms' draws in model order, from 0.0.

Random numbers: Philox4x64-10, key (seed, 0), counter (trajectory id, step t, term index j,
attempt a).  A box of dimension d uses blocks a = 0 .. ceil(d/4) - 1, word k % 4 of block k // 4
for component k; a ball of norm inf (or norm 1 in dimension 1) uses block 0; a 2-ball rejects
from the cube, one block per attempt a = 0, 1, .., accepting the first with sum s_k^2 <= 1, and
is zero after 64 attempts.  Words map to s = (r >> 11) 2^-52 - 1 in [-1, 1), exactly.  Every sum
and product below has the loop order of the kernel (csrc/ehm_explicit.hip, noise_kind) and no
fused multiply-add on either side, so host and device draws are bit-equal.
"""

import numpy as np

KINDS = ('process', 'state', 'input')
MAX_TERMS = 16          # must match EHM_N_MAX_TERMS in csrc/ehm_explicit.hip
MAX_BOX_DIM = 8
MAX_BALL_DIM = 3
MAX_F_ROWS = 8
MAX_ATTEMPTS = 64
DESC_WORDS = 8          # int32 per term descriptor, see NoiseModel.pack

_M64 = (1 << 64) - 1
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_PM0, _PM1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
_PW0, _PW1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def _mulhilo(a, b):
    """(hi, lo) of the 128-bit product of the constant a and the uint64 array b."""
    a0, a1 = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b0, b1 = b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    hi = p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)
    lo = (mid << _S32) | (p00 & _M32)
    return hi, lo


def philox4x64_10(c0, c1, c2, c3, k0, k1=0):
    """Philox4x64-10 of the counters (c0..c3, uint64 arrays or scalars, broadcast) under the key
    (k0, k1) (Python ints): the four words of the block, uint64 arrays."""
    c = np.broadcast_arrays(*[np.asarray(w, dtype=np.uint64) for w in (c0, c1, c2, c3)])
    c = [np.array(w, dtype=np.uint64) for w in c]
    k0, k1 = int(k0) & _M64, int(k1) & _M64
    for _ in range(10):
        hi0, lo0 = _mulhilo(_PM0, c[0])
        hi1, lo1 = _mulhilo(_PM1, c[2])
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _PW0) & _M64, (k1 + _PW1) & _M64
    return c


def uniform_pm1(r):
    """Raw uint64 words -> doubles in [-1, 1): (r >> 11) 2^-52 - 1 (exact)."""
    return (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def _norm_code(p):
    if p == np.inf or p == 'inf':
        return 0
    if p in (1, 2):
        return int(p)
    raise ValueError('norm must be 1, 2 or inf, not %r' % (p,))


def _norm_rows(Y, code):
    """||.||_code of the rows Y [k][n] (list of arrays), in loop order."""
    if code == 0:
        r = np.abs(Y[0])
        for y in Y[1:]:
            r = np.maximum(r, np.abs(y))
        return r
    if code == 1:
        r = 0.0 + np.abs(Y[0])
        for y in Y[1:]:
            r = r + np.abs(y)
        return r
    r = 0.0 + Y[0] * Y[0]
    for y in Y[1:]:
        r = r + y * y
    return np.sqrt(r)


def _matvec(M, X):
    """Rows of M [k][m] applied to X [n][m] column by column from 0.0: list of k arrays [n]."""
    out = []
    for i in range(M.shape[0]):
        s = np.zeros(X.shape[0])
        for c in range(M.shape[1]):
            s = s + M[i, c] * X[:, c]
        out.append(s)
    return out


class Term:
    """One term of a NoiseModel (see the module docstring)."""

    def __init__(self, kind, shape, dim, out_map, **kw):
        self.kind, self.shape, self.dim = kind, shape, int(dim)
        self.map = np.ascontiguousarray(out_map, dtype=np.float64)
        self.c = self.h = None
        self.norm, self.sigma, self.dep, self.F, self.p_dep = 2, 0., 'const', None, 2
        self.__dict__.update(kw)


class NoiseModel:
    """
    Ordered terms of process, state-estimation and input noise for a plant with n_x states, n_u
    inputs and n_d disturbance inputs (``addIndependentTerm`` / ``addDependentTerm`` follow the
    reference's ``UncertaintySet`` with the dependency given as numbers instead of a callable).
    """

    def __init__(self, n_x, n_u, n_d):
        self.n_x, self.n_u, self.n_d = int(n_x), int(n_u), int(n_d)
        self.terms = []

    def out_dim(self, kind):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, not %r" % (KINDS, kind))
        return {'process': self.n_d, 'state': self.n_x, 'input': self.n_u}[kind]

    def _add(self, term):
        if len(self.terms) >= MAX_TERMS:
            raise ValueError('at most %d terms' % MAX_TERMS)
        if term.map.shape != (self.out_dim(term.kind), term.dim):
            raise ValueError('the map of a %s term must be %d x %d, not %s' % (
                term.kind, self.out_dim(term.kind), term.dim, term.map.shape))
        self.terms.append(term)
        return self

    def addIndependentTerm(self, kind, lb, ub, M=None):
        """Uniform in the box lb <= w <= ub, mapped by M (identity by default)."""
        lb = np.atleast_1d(np.asarray(lb, dtype=np.float64))
        ub = np.atleast_1d(np.asarray(ub, dtype=np.float64))
        if lb.shape != ub.shape or lb.ndim != 1 or not np.all(lb <= ub):
            raise ValueError('lb and ub must be vectors of one size with lb <= ub')
        d = lb.size
        if d > MAX_BOX_DIM:
            raise ValueError('a box term has at most %d dimensions' % MAX_BOX_DIM)
        M = np.eye(d) if M is None else np.asarray(M, dtype=np.float64).reshape(-1, d)
        return self._add(Term(kind, 'box', d, M, c=(lb + ub) / 2., h=(ub - lb) / 2.))

    def addDependentTerm(self, kind, sigma, norm=2, dim=None, L=None, Fx=None, px=None, Fu=None,
                         pu=None):
        """
        Uniform in the ball {||q||_norm <= r}, mapped by L (identity of ``dim`` by default), with
        r = sigma (neither Fx/px nor Fu/pu given), sigma ||Fx x||_px or sigma ||Fu u||_pu
        (Fx / Fu default to the identity).
        """
        if L is None:
            if dim is None:
                raise ValueError('give dim or L')
            L = np.eye(int(dim))
        L = np.atleast_2d(np.asarray(L, dtype=np.float64))
        d = L.shape[1]
        code = _norm_code(norm)
        if d > MAX_BALL_DIM or (code == 1 and d > 1):
            raise ValueError('balls of norm 2 / inf up to dimension %d, norm 1 in dimension 1'
                             % MAX_BALL_DIM)
        if (px is not None or Fx is not None) and (pu is not None or Fu is not None):
            raise ValueError('the radius depends on the state or on the input, not on both')
        dep, F, p_dep = 'const', None, 2
        if px is not None or Fx is not None:
            dep, F, p_dep = 'state', np.eye(self.n_x) if Fx is None else Fx, 2 if px is None else px
        elif pu is not None or Fu is not None:
            dep, F, p_dep = 'input', np.eye(self.n_u) if Fu is None else Fu, 2 if pu is None else pu
        if F is not None:
            F = np.atleast_2d(np.asarray(F, dtype=np.float64))
            cols = self.n_x if dep == 'state' else self.n_u
            if F.shape[1] != cols or F.shape[0] > MAX_F_ROWS:
                raise ValueError('F must have %d columns and at most %d rows' % (cols, MAX_F_ROWS))
        return self._add(Term(kind, 'ball', d, L, norm=code, sigma=float(sigma), dep=dep, F=F,
                              p_dep=_norm_code(p_dep)))

    @classmethod
    def from_mpc(cls, mpc):
        """The uncertainty model a law was tightened against: the six terms of the reference's
        ``SatelliteZ`` (lib/mpc_library.py:236-255, in that order) for a ``SatelliteZ``; None for
        laws without one (``PWAMPC``)."""
        if not hasattr(mpc, 'u_pieces'):
            return None
        p = mpc.pars
        I, O = np.eye(1), np.zeros((1, 1))
        m = cls(mpc.n_x, mpc.n_u, mpc.E.shape[1])
        m.addIndependentTerm('process', lb=-p['w_max'] * np.ones(1), ub=p['w_max'] * np.ones(1))
        m.addIndependentTerm('state', lb=-np.array([p['p_max'], p['v_max']]),
                             ub=np.array([p['p_max'], p['v_max']]))
        m.addDependentTerm('input', p['sigma_fix'], norm=2, dim=1)
        m.addDependentTerm('state', p['sigma_pos'], norm=np.inf, L=np.vstack((I, O)),
                           Fx=np.hstack((I, O)), px=2)
        m.addDependentTerm('state', p['sigma_vel'], norm=np.inf, L=np.vstack((O, I)),
                           Fx=np.hstack((O, I)), px=2)
        m.addDependentTerm('input', p['sigma_rcs'], norm=2, dim=1, Fu=np.eye(1), pu=2)
        return m

    # -- sampling ------------------------------------------------------------------------------
    def _blocks(self, seed, ids, t, j, a):
        return philox4x64_10(ids, t, j, a, seed, 0)

    def _draw(self, j, term, seed, ids, t, X, U):
        """[n, dim] draw of term j before its map."""
        n = ids.size
        if term.shape == 'box':
            S = np.empty((n, term.dim))
            for b in range((term.dim + 3) // 4):
                w = self._blocks(seed, ids, t, j, b)
                for k in range(4 * b, min(term.dim, 4 * b + 4)):
                    S[:, k] = term.c[k] + term.h[k] * uniform_pm1(w[k % 4])
            return S
        if term.dep == 'const':
            r = np.full(n, term.sigma)
        else:
            Y = _matvec(term.F, X if term.dep == 'state' else U)
            r = term.sigma * _norm_rows(Y, term.p_dep)
        S = np.zeros((n, term.dim))
        if term.norm != 2:
            w = self._blocks(seed, ids, t, j, 0)
            for k in range(term.dim):
                S[:, k] = uniform_pm1(w[k])
        else:
            todo = np.arange(n)
            for a in range(MAX_ATTEMPTS):
                if todo.size == 0:
                    break
                w = self._blocks(seed, ids[todo], t, j, a)
                s = [uniform_pm1(w[k]) for k in range(term.dim)]
                ss = 0.0 + s[0] * s[0]
                for k in range(1, term.dim):
                    ss = ss + s[k] * s[k]
                ok = ss <= 1.0
                for k in range(term.dim):
                    S[todo[ok], k] = s[k][ok]
                todo = todo[~ok]
        for k in range(term.dim):
            S[:, k] = r * S[:, k]
        return S

    def sample(self, kind, seed, traj_ids, t, x, u):
        """
        Draw of ``kind`` [n, out_dim] for the trajectories traj_ids [n] at step t, at the true
        states x [n, n_x] and the inputs u [n, n_u] (the ones the radius depends on).  The
        input error is NOT zeroed here where u = 0; the rollouts do that.
        """
        ids = np.atleast_1d(np.asarray(traj_ids)).astype(np.uint64)
        X = np.asarray(x, dtype=np.float64).reshape(ids.size, self.n_x)
        U = np.asarray(u, dtype=np.float64).reshape(ids.size, self.n_u)
        out = np.zeros((ids.size, self.out_dim(kind)))
        for j, term in enumerate(self.terms):
            if term.kind != kind:
                continue
            Y = _matvec(term.map, self._draw(j, term, int(seed), ids, int(t), X, U))
            for i in range(out.shape[1]):
                out[:, i] = out[:, i] + Y[i]
        return out

    # -- the flat form of ehm_explicit_set_noise -----------------------------------------------
    def pack(self):
        """
        (desc int32 [n_terms, 8], data float64): per term (kind 0 process / 1 state / 2 input,
        shape 0 box / 1 ball, dim, ball norm code, radius dependency 0 const / 1 state / 2 input,
        its norm code, rows of F, offset of the term's doubles); norm codes 0 inf, 1, 2.  Doubles
        of a box: c [dim], h [dim], M [out][dim]; of a ball: sigma, F [rows][n_x or n_u],
        L [out][dim].
        """
        desc, data = [], []
        for term in self.terms:
            off = len(data)
            if term.shape == 'box':
                data += list(term.c) + list(term.h) + list(term.map.ravel())
                desc.append([KINDS.index(term.kind), 0, term.dim, 0, 0, 0, 0, off])
            else:
                rows = 0 if term.F is None else term.F.shape[0]
                data += [term.sigma] + ([] if term.F is None else list(term.F.ravel())) \
                    + list(term.map.ravel())
                desc.append([KINDS.index(term.kind), 1, term.dim, term.norm,
                             ('const', 'state', 'input').index(term.dep), term.p_dep, rows, off])
        return (np.ascontiguousarray(np.array(desc, dtype=np.int32).reshape(-1, DESC_WORDS)),
                np.ascontiguousarray(np.array(data, dtype=np.float64)))


def bounding_boxes(model, x_abs, u_abs):
    """
    {'process': (lo, hi), 'state': (lo, hi), 'input': (lo, hi)}: per kind an interval hull of every
    draw ``model.sample`` can make at true states with |x| <= x_abs and inputs with |u| <= u_abs
    (coordinate-wise), summed over the kind's terms; host numpy.  A box term M (c + h s), |s| <= 1,
    lies in M c -+ |M| h.  A ball term L q with ||q||_norm <= r has coordinate i within
    -+ r ||L_i||_*, the dual norm of the ball's (2 <-> 2, inf <-> 1, 1 <-> inf), and r is at most
    sigma, sigma || |F| x_abs ||_px or sigma || |F| u_abs ||_pu: the norms are monotone in the
    moduli and |F x| <= |F| |x|.  The bounds are in floating point: a draw may pass one by rounding.
    """
    x_abs = np.asarray(x_abs, dtype=np.float64).reshape(model.n_x)
    u_abs = np.asarray(u_abs, dtype=np.float64).reshape(model.n_u)
    out = {k: (np.zeros(model.out_dim(k)), np.zeros(model.out_dim(k))) for k in KINDS}
    for term in model.terms:
        lo, hi = out[term.kind]
        if term.shape == 'box':
            mid, rad = term.map @ term.c, np.abs(term.map) @ term.h
            out[term.kind] = (lo + (mid - rad), hi + (mid + rad))
            continue
        r = term.sigma
        if term.dep != 'const':
            y = np.abs(term.F) @ (x_abs if term.dep == 'state' else u_abs)
            r = r * _norm_rows([y[i:i + 1] for i in range(y.size)], term.p_dep)[0]
        L = np.abs(term.map)
        dual = np.sqrt((L * L).sum(axis=1)) if term.norm == 2 else \
            L.sum(axis=1) if term.norm == 0 else L.max(axis=1)
        out[term.kind] = (lo - r * dual, hi + r * dual)
    return out


def state_bound(model, set_abs, u_abs, grow=1e-6, iterations=100):
    """
    x_abs [n_x] with |x| <= x_abs for every true state x = z - v of a closed loop whose measured
    states z obey |z| <= set_abs, v drawn by ``model`` at x.  With v_half(a) the coordinate-wise
    largest modulus of the 'state' box of ``bounding_boxes(model, a, u_abs)``, every true state has
    |x| <= set_abs + v_half(|x|), and v_half is a constant plus a monotone, positively homogeneous
    function; so any a with set_abs + v_half(a) <= a bounds |x|.  a is found by
    iterating a <- set_abs + v_half(a) from set_abs, inflated by 1 + grow, and VERIFIED.
    ``ValueError`` where no iterate passes within ``iterations``: the relative error is 100 % or more.
    """
    set_abs = np.asarray(set_abs, dtype=np.float64).reshape(model.n_x)

    def v_half(a):
        with np.errstate(over='ignore', invalid='ignore'):      # a diverging iterate ends below
            lo, hi = bounding_boxes(model, a, u_abs)['state']
        return np.maximum(np.abs(lo), np.abs(hi))

    a = set_abs.copy()
    for _ in range(int(iterations)):
        a = set_abs + v_half(a)
        cand = a * (1. + grow)
        if not np.isfinite(cand).all():
            break
        if (set_abs + v_half(cand) <= cand).all():
            return cand
    raise ValueError('no bound on the true state within %d iterations: the state-dependent '
                     'measurement error does not contract (a relative error of 100 %% or more)'
                     % iterations)


def state_input_model(half, n_u):
    """
    A hand-built state / input model for a law without one of its own (``from_mpc`` gives None),
    for the set of half-widths ``half``: a measurement box of 1 % of the set, a 6-dimensional box
    of 0.1 % mapped onto the state (its draw takes two Philox blocks), a measurement 2-ball of
    radius 1 % ||x||_2, a fixed input box of 1e-3 and an input inf-ball of radius 5 % ||u||_inf.
    """
    half = np.asarray(half, dtype=np.float64)
    p = half.size
    m = NoiseModel(p, n_u, 0)
    m.addIndependentTerm('state', lb=-1e-2 * half, ub=1e-2 * half)
    m.addIndependentTerm('state', lb=-np.ones(6), ub=np.ones(6),
                         M=1e-3 * np.tile(np.diag(half), 6)[:, :6])
    m.addDependentTerm('state', 1e-2, norm=2, L=np.eye(p)[:, :min(3, p)], Fx=np.eye(p), px=2)
    m.addIndependentTerm('input', lb=-1e-3 * np.ones(n_u), ub=1e-3 * np.ones(n_u))
    k = min(3, n_u)
    m.addDependentTerm('input', 5e-2, norm=np.inf, L=np.eye(n_u)[:, :k], Fu=np.eye(n_u),
                       pu=np.inf)
    return m
