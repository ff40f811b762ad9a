"""
Synthetic explicit laws of any (p, n_u) and an exact restatement of what the device computes on
them (test infrastructure, host only; no partition and no oracle needed).

    forest = kuhn_forest(p, cells, lo, h)            # Kuhn roots of a grid of cubes
    law = SynthLaw(forest, n_u, n_modes, rng)         # bisection subtrees, inputs, modes
    ex = law.explicit()                               # ExplicitMPC over law.flat (public API)
    ref = law.locate(x)                               # exact leaf, weights, margins, kappas
    plant, model = random_plant(...), random_noise(...)
    mirror = replay(law, plant, res, X0, T, ...)      # the rollout in the device's order

Roots.  A Kuhn (Freudenthal) triangulation: grid cube c with corner g (integer grid coordinates,
side h, a power of two) is cut into p! simplices, one per permutation pi of the axes, vertices
v_0 = g, v_k = v_(k-1) + e_(pi(k-1)).  Inside the cube the simplex of pi is the set where the
fractional coordinates f satisfy f_pi(0) >= .. >= f_pi(p-1), and the barycentric weights of a
point are the gaps of that chain: l_0 = 1 - f_pi(0), l_k = f_pi(k-1) - f_pi(k), l_p = f_pi(p-1).
Every coordinate is dyadic, so the roots are exact in float64 and tile the box.  Roots are
numbered cube by cube (C order) and, in a cube, in itertools.permutations order.

Subtrees.  Bisection of the edge (i, j) at its midpoint m (asserted exact): the left child has
v_i replaced by m, the right child v_j.  The weights of a point in a child follow exactly from
the parent's: left mu_i = 2 l_i, mu_j = l_j - l_i; right mu_j = 2 l_j, mu_i = l_i - l_j.  So the
exact weights of x in every node on its path are integers over one power of two D (x and the
vertices are dyadic), and the reference's walk -- first root that contains x, else the last;
then left iff x is in the left child -- runs in Python integers.

Conditioning.  kappa(k) is the 2-norm condition number of node k's edge matrix
[v_1 - v_0 .. v_p - v_0]; sliver chains (the same edge bisected again and again) reach ~1e8.
"""

import itertools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from explicit_hybrid_mpc_amd import simulate
from explicit_hybrid_mpc_amd.engine import FlatTree
from explicit_hybrid_mpc_amd.noise import NoiseModel
from oracle.geometry import split_along_longest_edge

EPS = float(np.finfo(np.float64).eps)
LOCATE_MIN = 128        # EHM_X_LOCATE_MIN: spines this long get the root locator
LOCATE_STEPS = 96       # EHM_X_STEPS
MAX_ROOTS = 1 << 20     # roots the locator's packed index can name


class KuhnForest:
    """The Kuhn roots of a grid of ``cells`` cubes of side h (a power of two) from ``lo``; only
    the first ``n_keep`` roots are kept when given (a spine below LOCATE_MIN)."""

    def __init__(self, cells, lo, h, n_keep=None):
        self.cells = tuple(int(c) for c in cells)
        self.p = p = len(self.cells)
        self.lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (p,)).copy()
        self.h = float(h)
        if math.frexp(self.h)[0] != 0.5:
            raise ValueError('the side must be a power of two')
        self.perms = list(itertools.permutations(range(p)))
        self.perm_index = {pi: i for i, pi in enumerate(self.perms)}
        n_cells = int(np.prod(self.cells))
        full = n_cells * len(self.perms)
        self.n_roots = full if n_keep is None else min(int(n_keep), full)
        # integer grid coordinates of every root's vertices [n_roots, p+1, p]
        steps = np.zeros((len(self.perms), p + 1, p), dtype=np.int64)
        for a, pi in enumerate(self.perms):
            for k in range(1, p + 1):
                steps[a, k] = steps[a, k - 1]
                steps[a, k, pi[k - 1]] += 1
        corners = np.stack(np.unravel_index(np.arange(n_cells), self.cells), axis=1)
        n_c = -(-self.n_roots // len(self.perms))
        G = corners[:n_c, None, None, :] + steps[None]
        self.grid = G.reshape(-1, p + 1, p)[:self.n_roots]
        self.vertices = self.lo + self.grid * self.h

    def scaled(self, x):
        """Grid coordinates of x as integers Y over a power of two D: y = (x - lo) / h = Y / D."""
        ys = [(Fraction(float(x[c])) - Fraction(float(self.lo[c]))) / Fraction(self.h)
              for c in range(self.p)]
        D = max(y.denominator for y in ys)
        return [y.numerator * (D // y.denominator) for y in ys], D

    def root_weights(self, r, Y, D):
        """Exact weights of y = Y / D in root r, as integers over D."""
        cell, a = divmod(int(r), len(self.perms))
        g = np.unravel_index(cell, self.cells)
        pi = self.perms[a]
        f = [Y[c] - int(g[c]) * D for c in range(self.p)]
        lam = [D - f[pi[0]]]
        lam += [f[pi[k - 1]] - f[pi[k]] for k in range(1, self.p)]
        lam.append(f[pi[-1]])
        return lam

    def containing_roots(self, Y, D):
        """Every root index that holds y = Y / D (ties on faces give several), ascending."""
        opts = []
        for c in range(self.p):
            q, rem = divmod(Y[c], D)
            o = [q - 1, q] if rem == 0 else [q]
            o = [v for v in o if 0 <= v < self.cells[c]]
            if not o:
                return []
            opts.append(o)
        out = []
        for cell in itertools.product(*opts):
            f = [Y[c] - cell[c] * D for c in range(self.p)]
            order = sorted(range(self.p), key=lambda c: -f[c])
            groups = [list(g) for _, g in itertools.groupby(order, key=lambda c: f[c])]
            lin = int(np.ravel_multi_index(cell, self.cells))
            for parts in itertools.product(*[itertools.permutations(g) for g in groups]):
                pi = tuple(c for part in parts for c in part)
                r = lin * len(self.perms) + self.perm_index[pi]
                if r < self.n_roots:
                    out.append(r)
        return sorted(out)


def kuhn_forest(p, n_keep=None):
    """The forest the tests use per p: [-1, 1]^p in n^p cubes with at least LOCATE_MIN roots
    (p = 8: one cube, 40 320 roots), or its first ``n_keep`` roots."""
    n = {1: 128, 2: 8, 3: 4, 4: 2, 5: 2, 6: 1, 7: 1, 8: 1}[p]
    return KuhnForest([n] * p, -1., 2. / n, n_keep)


def _exact_midpoint(a, b):
    """(a + b) / 2, asserted exact (TwoSum error 0)."""
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    assert np.all(err == 0), 'a bisection midpoint is not exact'
    return s / 2.


class SynthLaw:
    """
    A law over ``forest``: subtrees grown under ``n_sub`` roots (mostly longest-edge bisection
    to depth 8..20, every third a sliver chain that bisects one edge to depth ``sliver_depth``),
    vertex inputs u_j(v) = sin(a_j.v + b_j) + 0.3 cos(c_j.v) ||v||^2 / p, and per node a
    commutation 0..n_modes-1 (``-1`` on about 4 % of the leaves: no law there).
    """

    def __init__(self, forest, n_u, n_modes, rng, n_sub=24, sliver_depth=26, no_law=0.04):
        self.forest = forest
        p, R = forest.p, forest.n_roots
        self.p, self.n_u, self.n_modes = p, int(n_u), int(n_modes)
        extra = []                          # nodes below the roots: vertices
        parent, split = [], []              # per extra node: parent, (i, j, side)
        left = np.full(R, -1, dtype=np.int64).tolist()
        right = list(left)
        self.sliver_leaves = []

        def vert(k):
            return forest.vertices[k] if k < R else extra[k - R]

        def add(k, S, i, j, side):
            extra.append(S)
            parent.append(k)
            split.append((i, j, side))
            left.append(-1)
            right.append(-1)
            return R + len(extra) - 1

        def bisect(k, edge=None):
            P = vert(k)
            if edge is None:
                _, _, (i, j) = split_along_longest_edge(P)
            else:
                i, j = edge
            m = _exact_midpoint(P[i], P[j])
            S1, S2 = P.copy(), P.copy()
            S1[i], S2[j] = m, m
            a, b = add(k, S1, i, j, 0), add(k, S2, i, j, 1)
            left[k], right[k] = a, b
            return a, b, (i, j)

        n_sub = min(n_sub, R)
        subs = rng.choice(R, n_sub, replace=False)
        for s, r in enumerate(subs):
            r = int(r)
            if s % 3 == 2:                  # sliver chain: one edge again and again
                a, b, edge = bisect(r)
                k = (a, b)[rng.integers(2)]
                for _ in range(sliver_depth - 1):
                    a, b, _ = bisect(k, edge)
                    k = (a, b)[rng.integers(2)]
                self.sliver_leaves += [a, b]
                continue
            stack = [(r, int(rng.integers(8, 21)))]
            while stack:
                k, dl = stack.pop()
                if dl == 0:
                    continue
                a, b, _ = bisect(k)
                c = rng.integers(2)
                stack.append(((a, b)[c], dl - 1))
                if rng.random() < 0.3:
                    stack.append(((a, b)[1 - c], min(dl - 1, int(rng.integers(1, 4)))))
        K = R + len(extra)
        self.n_nodes = K
        self.left = np.array(left, dtype=np.int32)
        self.right = np.array(right, dtype=np.int32)
        self.parent = np.array([-1] * R + parent, dtype=np.int64)
        self.split = [None] * R + split
        self.vertices = np.concatenate([forest.vertices, np.array(extra).reshape(-1, p + 1, p)])
        self.leaves = np.nonzero(self.left < 0)[0]
        # the law: smooth inputs at the vertices, commutations
        A = rng.normal(size=(self.n_u, p))
        bb = rng.uniform(-1, 1, self.n_u)
        C = rng.normal(size=(self.n_u, p))
        Vf = self.vertices.reshape(-1, p)
        U = np.sin(Vf @ A.T + bb) + 0.3 * np.cos(Vf @ C.T) * (Vf * Vf).sum(1)[:, None] / p
        self.vertex_inputs = np.ascontiguousarray(U.reshape(K, p + 1, self.n_u))
        self.u_max = float(np.abs(self.vertex_inputs).max())
        didx = rng.integers(0, self.n_modes, K).astype(np.int32)
        didx[self.leaves[rng.random(self.leaves.size) < no_law]] = -1
        self.delta_idx = didx
        self.flat = FlatTree(self.vertices, self.left, self.right, self.delta_idx,
                             np.zeros((K, p + 1)), self.vertex_inputs, np.zeros(K, np.uint8),
                             np.zeros(K), {'n_roots': R}, list(range(self.n_modes)))
        self._kappa = {}

    def explicit(self):
        """The device law (ExplicitMPC over the FlatTree; step-0 mode of commutation d is d)."""
        from explicit_hybrid_mpc_amd import explicit
        return explicit.ExplicitMPC(self.flat, SimpleNamespace(
            mpc=SimpleNamespace(step0_mode=lambda d: int(d))))

    def node_mode(self):
        return np.where(self.delta_idx >= 0, self.delta_idx, -1).astype(np.int32)

    def kappa(self, k):
        k = int(k)
        if k not in self._kappa:
            P = self.vertices[k]
            self._kappa[k] = float(np.linalg.cond((P[1:] - P[0]).T))
        return self._kappa[k]

    def depth(self, k):
        d = 0
        while self.parent[k] >= 0:
            k = self.parent[k]
            d += 1
        return d

    # -- exact point location ---------------------------------------------------------------
    @staticmethod
    def child_weights(lam, i, j, side):
        mu = list(lam)
        if side == 0:
            mu[i], mu[j] = 2 * lam[i], lam[j] - lam[i]
        else:
            mu[j], mu[i] = 2 * lam[j], lam[i] - lam[j]
        return mu

    def weights_in(self, k, Y, D):
        """Exact weights (integers over D) of y in node k, from its root down."""
        path = []
        while self.parent[k] >= 0:
            path.append(k)
            k = int(self.parent[k])
        lam = self.forest.root_weights(k, Y, D)
        for c in reversed(path):
            lam = self.child_weights(lam, *self.split[c])
        return lam

    def locate(self, x):
        """
        The reference's walk of x in exact arithmetic: SimpleNamespace(leaf, root, lam and D (the
        exact weights in the leaf are lam / D, integers over a power of two), margin (smallest decision margin on the path, in weight
        units; <= 0 on a tie), kappa (largest kappa on the path), tests (containment tests the
        serial walk makes), inside (some root holds x)).
        """
        F = self.forest
        Y, D = F.scaled(x)
        hold = F.containing_roots(Y, D)
        inside = bool(hold)
        r = hold[0] if hold else F.n_roots - 1
        lam = F.root_weights(r, Y, D)
        root_margin = Fraction(min(lam), D)
        tests = min(r + 1, F.n_roots - 1)
        if inside:      # the gaps of the Kuhn chain; any other root has a weight <= -gap / p
            margin = Fraction(min(lam), D * F.p)
        else:           # outside the box by delta grid units: every root has a weight <= -delta/p
            out = max(max(-Y[c], Y[c] - F.cells[c] * D) for c in range(F.p))
            margin = Fraction(max(out, 0), D * F.p)
        kappa = self.kappa(r)
        k = r
        while self.left[k] >= 0:
            tests += 1
            a = int(self.left[k])
            mu = self.child_weights(lam, *self.split[a])
            lo = min(mu)
            margin = min(margin, Fraction(abs(lo), D))
            kappa = max(kappa, self.kappa(a))
            if lo >= 0:
                k, lam = a, mu
            else:
                k = int(self.right[k])
                lam = self.child_weights(lam, *self.split[k])
        kappa = max(kappa, self.kappa(k))
        return SimpleNamespace(leaf=k, root=r, lam=lam, D=D, margin=margin, kappa=kappa,
                               tests=tests, inside=inside, Y=Y, root_margin=root_margin,
                               internal=tests - min(r + 1, F.n_roots - 1))

    def threshold(self, k):
        """The margin below which a containment decision about node k may go either way."""
        return Fraction(1e-10) * (1 + Fraction(self.kappa(k)))

    def check_path(self, k, ref):
        """
        Asserts that the walk to leaf k is the exact walk of ref's point up to decisions within
        ``threshold``: k's root holds the point within the threshold (and is the exact root when
        the spine's margin is above it), and at every node on the way down the turn taken is
        the exact one unless the left child's exact margin is within its threshold.  (After
        such a turn the walk goes on, right without a test, in a subtree that need not hold
        the point, so the leaf's weights can be far below 0: the reference's rule.)
        Returns the exact weights (integers over ref.D) in k.
        """
        path = [int(k)]
        while self.parent[path[-1]] >= 0:
            path.append(int(self.parent[path[-1]]))
        path.reverse()
        r = path[0]
        Y, D = ref.Y, ref.D
        lam = self.forest.root_weights(r, Y, D)
        if r != ref.root:
            assert ref.margin <= self.threshold(ref.root), ('root', r, ref.root)
            assert Fraction(min(lam), D) >= -self.threshold(r), ('root', r, ref.root)
        for a, b in zip(path[:-1], path[1:]):
            L = int(self.left[a])
            mu = self.child_weights(lam, *self.split[L])
            exact_left = min(mu) >= 0
            if (b == L) != exact_left:
                assert Fraction(abs(min(mu)), D) <= self.threshold(L), ('turn', a, b)
            lam = mu if b == L else self.child_weights(lam, *self.split[b])
        return lam

    def decisive(self, ref):
        """Every decision on the path has a margin above 1e-10 (1 + kappa)."""
        return ref.margin > Fraction(1e-10) * (1 + Fraction(ref.kappa))

    def u_exact(self, k, lam, D):
        """The input interpolated with the exact weights lam / D in node k, rounded once."""
        out = np.empty(self.n_u)
        for c in range(self.n_u):
            rat = [float(u).as_integer_ratio() for u in self.vertex_inputs[k, :, c]]
            den = max(b for _, b in rat)
            num = sum(l * a * (den // b) for l, (a, b) in zip(lam, rat))
            out[c] = num / (D * den)        # int / int: correctly rounded
        return out

    def u_tol(self, kappa, lam=None, D=1, c=32.):
        """|u_dev - u_exact| bound: c p kappa eps max|U| (c = 32), times max|weight| where the
        weights lam / D extrapolate beyond 1."""
        big = 1. if lam is None else max(1., max(abs(v) for v in lam) / D)
        return c * self.p * max(kappa, 1.) * EPS * self.u_max * big

    # -- states -----------------------------------------------------------------------------
    def states(self, rng, n, roots=None):
        """n states: a third uniform in random leaves, a sixth inside sliver leaves, the rest
        1e-12 on either side of a random face of a random node (hull faces from inside).
        ``roots``: draw only below these roots."""
        ok = np.ones(self.n_nodes, dtype=bool)
        if roots is not None:
            top = np.arange(self.n_nodes)
            for _ in range(64):
                up = np.where(self.parent[top] >= 0, self.parent[top], top)
                if np.array_equal(up, top):
                    break
                top = up
            ok = np.isin(top, roots)
        leaves = self.leaves[ok[self.leaves]]
        nodes = np.nonzero(ok)[0]
        slivers = np.array([k for k in self.sliver_leaves if ok[k]], dtype=np.int64)
        n_in = n // 3
        n_sl = n // 6 if slivers.size else 0
        pick = [rng.choice(leaves, n_in), rng.choice(slivers, n_sl) if n_sl else
                np.zeros(0, np.int64), rng.choice(nodes, n - n_in - n_sl)]
        X = []
        for part, kind in zip(pick, ('in', 'in', 'face')):
            for k in part:
                lam = rng.dirichlet(np.ones(self.p + 1))
                if kind == 'face':
                    f = rng.integers(self.p + 1)
                    lam[f] = 0.
                    lam *= 1. / lam.sum()
                    lam[f] = (1e-12 if rng.random() < 0.5 else -1e-12)
                X.append(lam @ self.vertices[k])
        X = np.array(X)
        hold = np.array([bool(self.forest.containing_roots(*self.forest.scaled(x))) for x in X])
        return X[hold]


# -- plants and noise models ----------------------------------------------------------------
def _spectral(rng, p, rho):
    A = rng.normal(size=(p, p))
    return A * (rho / max(abs(np.linalg.eigvals(A)).max(), 1e-12))


def random_plant(rng, p, n_u, n_modes, cost, n_d=0, n_g=None):
    """A ``simulate.Plant``: A_m of spectral radius 0.5..0.9, small B and w, mode regions (one
    or two rows that part of [-1, 1]^p violates; mode 0 everywhere), n_g state rows."""
    A = [_spectral(rng, p, rng.uniform(0.5, 0.9)) for _ in range(n_modes)]
    B = [rng.normal(size=(p, n_u)) * 0.1 for _ in range(n_modes)]
    w = [rng.normal(size=p) * 0.02 for _ in range(n_modes)]
    regions = [None]
    for m in range(1, n_modes):
        rows = int(rng.integers(1, 3))
        H = rng.normal(size=(rows, p))
        regions.append((H, np.abs(H).sum(1) * rng.uniform(0.3, 0.7, rows)))
    n_g = int(rng.integers(0, 40)) if n_g is None else n_g
    Gx = rng.normal(size=(n_g, p))
    gx = np.abs(Gx).sum(1) * 0.5
    E = rng.normal(size=(p, n_d)) * 0.01 if n_d else None
    Q = rng.normal(size=(p, p))
    R = rng.normal(size=(n_u, n_u))
    return simulate.Plant(A, B, w, E, regions, Gx if n_g else None, gx if n_g else None, Q, R,
                          cost)


def random_guarded(rng, p, n_u, n_modes, cost, substeps, n_rows, n_g=None):
    """A ``simulate.GuardedPlant``: n_modes modes (spectral radius <= 0.95 per plant step),
    guards of 1..3 rows, strict and non-strict, n_rows rows in all, the last mode the default."""
    A = [_spectral(rng, p, rng.uniform(0.6, 0.95) ** (1. / substeps)) for _ in range(n_modes)]
    B = [rng.normal(size=(p, n_u)) * 0.1 / substeps for _ in range(n_modes)]
    w = [rng.normal(size=p) * 0.02 / substeps for _ in range(n_modes)]
    guards, left = [], n_rows
    while left > 0:
        k = min(left, int(rng.integers(1, 4)))
        rows = [(rng.normal(size=p), rng.normal(size=n_u), float(rng.normal() * 0.1),
                 float(rng.uniform(-0.3, 0.5)), bool(rng.integers(2))) for _ in range(k)]
        guards.append((int(rng.integers(0, n_modes)), rows))
        left -= k
    n_g = int(rng.integers(0, 40)) if n_g is None else n_g
    Gx = rng.normal(size=(n_g, p))
    gx = np.abs(Gx).sum(1) * 0.5
    Q = rng.normal(size=(p, p))
    R = rng.normal(size=(n_u, n_u))
    return simulate.GuardedPlant(A, B, w, substeps, guards, n_modes - 1, Q, R, cost=cost,
                                 Gx=Gx if n_g else None, gx=gx if n_g else None)


def random_noise(rng, p, n_u, n_d):
    """A ``noise.NoiseModel`` with boxes of dimension up to 8 (two Philox blocks) and 2- / inf- /
    1-balls of dimension <= 3, constant and state / input dependent radii."""
    m = NoiseModel(p, n_u, n_d)
    d = int(rng.integers(5, 9))
    m.addIndependentTerm('state', lb=-np.ones(d), ub=np.ones(d) * rng.uniform(0.5, 1.),
                         M=rng.normal(size=(p, d)) * 2e-3)
    m.addDependentTerm('state', 1e-2, norm=2, L=rng.normal(size=(p, min(3, p))) * 0.3,
                       Fx=rng.normal(size=(int(rng.integers(1, 5)), p)), px=2)
    m.addDependentTerm('state', 5e-3, norm=np.inf, dim=min(3, p) if p <= 3 else None,
                       L=None if p <= 3 else rng.normal(size=(p, 3)) * 0.3)
    m.addIndependentTerm('input', lb=-1e-3 * np.ones(n_u), ub=1e-3 * np.ones(n_u))
    m.addDependentTerm('input', 5e-2, norm=1, L=rng.normal(size=(n_u, 1)), Fu=np.eye(n_u),
                       pu=np.inf)
    m.addDependentTerm('input', 1e-2, norm=2, L=rng.normal(size=(n_u, min(3, n_u))),
                       Fu=rng.normal(size=(2, n_u)), pu=1)
    if n_d:
        m.addIndependentTerm('process', lb=-np.ones(8), ub=np.ones(8),
                             M=rng.normal(size=(n_d, 8)))
        m.addDependentTerm('process', 0.5, norm=2, dim=None, L=rng.normal(size=(n_d, 2)),
                           Fx=np.eye(p)[:1], px=np.inf)
    return m


# -- the closed loop in the device's order ----------------------------------------------------
def dot_rows(M, X):
    return simulate._dot_rows(M, X)


def nominal_step(plant, X, U, m, D=None):
    """x+ = ((A_m x) + B_m u) + w_m (+ E d), one accumulator per row from 0.0, no FMA: the order
    of k_explicit_rollout (which differs from Plant.step's grouping)."""
    n, p = X.shape
    out = np.empty_like(X)
    A, B, w = plant.A[m], plant.B[m], plant.w[m]
    for i in range(p):
        s = np.zeros(n)
        for c in range(p):
            s = s + A[:, i, c] * X[:, c]
        for c in range(plant.n_u):
            s = s + B[:, i, c] * U[:, c]
        s = s + w[:, i]
        if D is not None:
            for j in range(plant.n_d):
                s = s + plant.E[i, j] * D[:, j]
        out[:, i] = s
    return out


def stage_cost(plant, X, U):
    """The stage cost of both kinds in the device's order (cost_kind 0: inf-norm, 1: quadratic)."""
    if plant.cost == 'inf':
        qx = np.zeros(X.shape[0])
        for y in dot_rows(plant.Q, X).T:
            qx = np.fmax(qx, np.abs(y))
        ru = np.zeros(X.shape[0])
        for y in dot_rows(plant.R, U).T:
            ru = np.fmax(ru, np.abs(y))
        return qx + ru
    s = np.zeros(X.shape[0])
    QX, RU = dot_rows(plant.Q, X), dot_rows(plant.R, U)
    for i in range(X.shape[1]):
        s = s + X[:, i] * QX[:, i]
    for i in range(U.shape[1]):
        s = s + U[:, i] * RU[:, i]
    return s


def u_norm(U):
    su = np.zeros(U.shape[0])
    for c in range(U.shape[1]):
        su = su + U[:, c] * U[:, c]
    return np.sqrt(su), su


def violation(plant, X):
    """max_j (Gx x - gx)_j in the device's order (-inf without rows)."""
    out = np.full(X.shape[0], -np.inf)
    if plant.gx.size:
        for j, y in enumerate(dot_rows(plant.Gx, X).T):
            out = np.fmax(out, y - plant.gx[j])
    return out


def in_region(plant, X, m, tol):
    """Mode m[i]'s region holds X[i]: every row sum_c H_c x_c <= h + tol (device order)."""
    ok = np.ones(X.shape[0], dtype=bool)
    for i in range(X.shape[0]):
        r = plant.regions[int(m[i])]
        if r is None:
            continue
        H = np.asarray(r[0], dtype=np.float64).reshape(-1, plant.n_x)
        h = np.asarray(r[1], dtype=np.float64).ravel()
        ok[i] = bool(np.all(dot_rows(H, X[i:i + 1])[0] <= h + tol))
    return ok


def replay(law, plant, res, X0, T, tol_exit, d=None, v=None, noise=None, seed=0, traj0=0,
           check_leaf=True):
    """
    Replays a recorded device rollout step by step from its own x_t and u_t: the draws (noisy),
    the exact leaf and input of z_t, the exit / mode / no-law tests, the plant step, cost,
    sum ||u|| and worst state row in the device's order.  Asserts what is bit-equal per step
    (x_{t+1}, v, e, w) and the leaf / input tolerances; returns the mirror's
    SimpleNamespace(x_final, steps, status, cost, u_norm_sum, max_violation, ambiguous) for the
    caller to compare.  A status is ``ambiguous`` (the device's own answer taken) only where
    the exact weights sit within kappa-sized rounding of the threshold.
    """
    n, p = X0.shape
    ids = np.arange(traj0, traj0 + n, dtype=np.uint64)
    node_mode = law.node_mode()
    if plant.n_modes == 1 and not plant.guarded:
        node_mode = np.zeros_like(node_mode)            # ExplicitMPC.node_modes: one mode
    x = X0.copy()
    steps = np.full(n, T, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    cost, unorm = np.zeros(n), np.zeros(n)
    maxv = np.full(n, -np.inf)
    u_prev = np.zeros((n, law.n_u))
    ambiguous = 0
    live = np.arange(n)
    assert np.array_equal(res.x[0], X0)
    for t in range(T):
        if live.size == 0:
            break
        xt = res.x[t, live]
        assert np.array_equal(xt, x[live])
        if noise is not None:
            vt = noise.sample('state', seed, ids[live], t, xt, u_prev[live])
            assert np.array_equal(res.v[t, live], vt)
            z = xt + vt if t > 0 else xt
        elif v is not None and t > 0:
            z = xt + v[t, live]
        else:
            z = xt
        dev_on = res.steps[live] > t
        go = np.zeros(live.size, dtype=bool)
        for a, q in enumerate(live):
            ref = law.locate(z[a])
            dec = law.decisive(ref)
            lo = Fraction(min(ref.lam), ref.D)
            slack = Fraction(64 * EPS) * (1 + Fraction(ref.kappa))
            if dev_on[a]:
                k = int(res.leaf[t, q])
                if check_leaf and dec:
                    assert k == ref.leaf, (t, q, k, ref.leaf, float(ref.margin))
                lam = law.check_path(k, ref)
                assert Fraction(min(lam), ref.D) >= -Fraction(tol_exit) - slack, (t, q)  # no exit
                if check_leaf:
                    ue = law.u_exact(k, lam, ref.D)
                    tol = law.u_tol(max(ref.kappa, law.kappa(k)), lam, ref.D)
                    assert np.all(np.abs(res.u[t, q] - ue) <= tol), (t, q, res.u[t, q], ue, tol)
                m = int(node_mode[k])
                assert m >= 0
                if not plant.guarded:
                    assert in_region(plant, xt[a:a + 1], [m], tol_exit)[0]
                go[a] = True
                continue
            # the device stopped this trajectory at t: the code must follow from the mirror
            code = int(res.status[q])
            exit_ = lo < -Fraction(tol_exit)
            near = abs(lo + Fraction(tol_exit)) <= slack or not dec
            if code == 1:
                if not exit_:
                    assert near, (t, q, float(lo))
                    ambiguous += 1
            else:
                if exit_:
                    assert near, (t, q, float(lo))
                    ambiguous += 1
                m = int(node_mode[ref.leaf])
                if code == 3:
                    assert m < 0 or not dec, (t, q)
                elif code == 2:
                    assert not plant.guarded and (m >= 0 or not dec)
                    if dec:
                        assert not in_region(plant, xt[a:a + 1], [m], tol_exit)[0]
                else:
                    raise AssertionError('trajectory %d stopped at %d with status %d' % (q, t, code))
            steps[q], status[q] = t, code
        live = live[go]
        if live.size == 0:
            break
        xl, ul = res.x[t, live], res.u[t, live]
        cost[live] = cost[live] + stage_cost(plant, xl, ul)
        nrm, su = u_norm(ul)
        unorm[live] = unorm[live] + nrm
        if noise is not None:
            e = noise.sample('input', seed, ids[live], t, xl, ul)
            e[su == 0.] = 0.
            w = noise.sample('process', seed, ids[live], t, xl, ul)
            assert np.array_equal(res.e[t, live], e)
            if plant.n_d:
                assert np.array_equal(res.w[t, live], w)
            u_prev[live] = ul
            xn = nominal_step(plant, xl, ul + e, node_mode[res.leaf[t, live]],
                              w if plant.n_d else None)
        elif plant.guarded:
            xn = plant.step(xl, ul)
        else:
            xn = nominal_step(plant, xl, ul, node_mode[res.leaf[t, live]],
                              None if d is None else d[t, live])
        assert np.array_equal(res.x[t + 1, live], xn), t
        maxv[live] = np.fmax(maxv[live], violation(plant, xn))
        x[live] = xn
    return SimpleNamespace(x_final=x, steps=steps, status=status, cost=cost, u_norm_sum=unorm,
                           max_violation=maxv, ambiguous=ambiguous)


def host_rollout(law, plant, X0, T, tol_exit, d=None, v=None, noise=None, seed=0, traj0=0):
    """The closed loop on the host with the exact walk and the exactly rounded input, recorded as
    the device records it (a ``simulate.ClosedLoop``): what ``replay`` must accept, on a CPU."""
    n, p = X0.shape
    ids = np.arange(traj0, traj0 + n, dtype=np.uint64)
    node_mode = law.node_mode()
    if plant.n_modes == 1 and not plant.guarded:
        node_mode = np.zeros_like(node_mode)
    xs = np.full((T + 1, n, p), np.nan)
    us = np.full((T, n, law.n_u), np.nan)
    leaf = np.full((T, n), -1, dtype=np.int32)
    vs = np.full((T, n, p), np.nan)
    es = np.full((T, n, law.n_u), np.nan)
    ws = np.full((T, n, plant.n_d), np.nan)
    xs[0] = X0
    x = X0.copy()
    steps = np.full(n, T, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    cost, unorm = np.zeros(n), np.zeros(n)
    maxv = np.full(n, -np.inf)
    u_prev = np.zeros((n, law.n_u))
    live = np.arange(n)
    for t in range(T):
        if live.size == 0:
            break
        xt = x[live]
        if noise is not None:
            vt = noise.sample('state', seed, ids[live], t, xt, u_prev[live])
            vs[t, live] = vt
            z = xt + vt if t > 0 else xt
        elif v is not None and t > 0:
            z = xt + v[t, live]
        else:
            z = xt
        go = np.zeros(live.size, dtype=bool)
        for a, q in enumerate(live):
            ref = law.locate(z[a])
            code = 0
            if Fraction(min(ref.lam), ref.D) < -Fraction(tol_exit):
                code = 1
            elif node_mode[ref.leaf] < 0:
                code = 3
            elif not plant.guarded and not in_region(plant, xt[a:a + 1], [node_mode[ref.leaf]],
                                                     tol_exit)[0]:
                code = 2
            if code:
                steps[q], status[q] = t, code
                continue
            go[a] = True
            leaf[t, q] = ref.leaf
            us[t, q] = law.u_exact(ref.leaf, ref.lam, ref.D)
        live = live[go]
        if live.size == 0:
            break
        xl, ul = x[live], us[t, live]
        cost[live] = cost[live] + stage_cost(plant, xl, ul)
        unorm[live] = unorm[live] + u_norm(ul)[0]
        m = node_mode[leaf[t, live]]
        if noise is not None:
            e = noise.sample('input', seed, ids[live], t, xl, ul)
            e[u_norm(ul)[1] == 0.] = 0.
            w = noise.sample('process', seed, ids[live], t, xl, ul)
            es[t, live], ws[t, live] = e, w
            u_prev[live] = ul
            xn = nominal_step(plant, xl, ul + e, m, w if plant.n_d else None)
        elif plant.guarded:
            xn = plant.step(xl, ul)
        else:
            xn = nominal_step(plant, xl, ul, m, None if d is None else d[t, live])
        maxv[live] = np.fmax(maxv[live], violation(plant, xn))
        x[live] = xn
        xs[t + 1, live] = xn
    out = simulate.ClosedLoop(x_final=x, steps=steps, status=status, cost=cost, u_norm_sum=unorm,
                              max_violation=maxv, x=xs, u=us, leaf=leaf)
    if noise is not None:
        out.v, out.e, out.w = vs, es, ws
    return out


def check_replay(mirror, res):
    """The rollout's per-trajectory outputs against the mirror: bit-equal, sum ||u|| to 1e-15."""
    assert np.array_equal(res.steps, mirror.steps)
    assert np.array_equal(res.status, mirror.status)
    assert np.array_equal(res.x_final, mirror.x_final)
    assert np.array_equal(res.cost, mirror.cost)
    assert np.array_equal(res.max_violation, mirror.max_violation)
    assert np.allclose(res.u_norm_sum, mirror.u_norm_sum, rtol=1e-15, atol=0)
