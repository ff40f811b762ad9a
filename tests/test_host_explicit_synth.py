"""
The test infrastructure of tests/test_gpu_explicit_widths.py on the host: the Kuhn roots tile
their box, the exact walk agrees with brute-force exact containment, and the order-faithful
mirror reproduces the plants' own steps and costs and accepts a host rollout while it catches
a one-ulp change of any recorded state.
"""

import math
from fractions import Fraction

import numpy as np
import pytest

from tests import explicit_synth as es


def _solve(M, b):
    """Exact solution of M y = b (Fractions, Gauss-Jordan)."""
    n = len(b)
    A = [[Fraction(M[r][c]) for c in range(n)] + [Fraction(b[r])] for r in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        for r in range(n):
            if r != c and A[r][c] != 0:
                f = A[r][c] / A[c][c]
                A[r] = [a - f * b for a, b in zip(A[r], A[c])]
    return [A[r][n] / A[r][r] for r in range(n)]


def _exact_weights(P, x):
    """Exact barycentric weights of x in the simplex P [(p+1), p] (float64 rows)."""
    p = P.shape[1]
    M = [[Fraction(float(P[c + 1][r])) - Fraction(float(P[0][r])) for c in range(p)]
         for r in range(p)]
    a = _solve(M, [Fraction(float(x[r])) - Fraction(float(P[0][r])) for r in range(p)])
    return [1 - sum(a)] + a


def _det(M):
    M = [[Fraction(v) for v in row] for row in M]
    n, d = len(M), Fraction(1)
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c] != 0), None)
        if piv is None:
            return Fraction(0)
        if piv != c:
            M[c], M[piv] = M[piv], M[c]
            d = -d
        d *= M[c][c]
        for r in range(c + 1, n):
            f = M[r][c] / M[c][c]
            M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return d


@pytest.mark.parametrize('cells', [(7,), (3, 2), (2, 2, 1), (1, 2, 1, 1)])
def test_kuhn_roots_tile_the_box(cells):
    F = es.KuhnForest(cells, -0.5, 0.25)
    p = len(cells)
    vol = sum(abs(_det((F.grid[r, 1:] - F.grid[r, 0]).T.tolist())) for r in range(F.n_roots))
    assert vol / math.factorial(p) == int(np.prod(cells))        # volumes h^p |det| / p!
    assert all(abs(_det((F.grid[r, 1:] - F.grid[r, 0]).T.tolist())) == 1 for r in range(F.n_roots))
    faces = {}
    for r in range(F.n_roots):
        for i in range(p + 1):
            key = tuple(sorted(tuple(v) for j, v in enumerate(F.grid[r].tolist()) if j != i))
            faces.setdefault(key, []).append(r)
    for key, owners in faces.items():
        assert len(owners) in (1, 2)
        on_hull = any(all(v[c] == 0 for v in key) or all(v[c] == cells[c] for v in key)
                      for c in range(p))
        assert (len(owners) == 1) == on_hull, key
    assert np.array_equal(F.vertices, -0.5 + 0.25 * F.grid)


@pytest.mark.parametrize('p', [1, 2, 3])
def test_exact_walk_matches_brute_force_containment(p):
    rng = np.random.default_rng(p)
    F = es.KuhnForest([3, 2, 2][:p] if p > 1 else [5], -1., 0.5)
    law = es.SynthLaw(F, 2, 2, rng, n_sub=F.n_roots, sliver_depth=10)
    X = law.states(rng, 150)
    # grid points and faces: ties between roots
    X = np.concatenate([X, -1. + 0.5 * rng.integers(0, 3, (20, p)),
                        rng.uniform(-1.5, 1.5, (20, p))])
    for x in X:
        ref = law.locate(x)
        w = [_exact_weights(F.vertices[r], x) for r in range(F.n_roots)]
        hold = [r for r in range(F.n_roots) if min(w[r]) >= 0]
        assert F.containing_roots(*F.scaled(x)) == hold
        r = hold[0] if hold else F.n_roots - 1
        assert ref.root == r and ref.inside == bool(hold)
        assert [Fraction(v, ref.D) for v in F.root_weights(r, ref.Y, ref.D)] == w[r]
        k = r
        while law.left[k] >= 0:
            a = int(law.left[k])
            k = a if min(_exact_weights(law.vertices[a], x)) >= 0 else int(law.right[k])
        assert ref.leaf == k
        assert [Fraction(v, ref.D) for v in ref.lam] == _exact_weights(law.vertices[k], x)
        if law.decisive(ref):
            assert ref.margin > 0
    assert p == 1 or max(law.kappa(k) for k in law.sliver_leaves) > 100.


def test_slivers_reach_kappa_1e8():
    law = es.SynthLaw(es.kuhn_forest(3), 1, 1, np.random.default_rng(3), n_sub=6)
    kap = max(law.kappa(k) for k in law.sliver_leaves)
    assert 1e7 < kap < 1e10


def test_mirror_reproduces_the_plants():
    rng = np.random.default_rng(4)
    for p, n_u in ((1, 1), (3, 2), (8, 4)):
        for cost in ('inf', 'quadratic'):
            pl = es.random_plant(rng, p, n_u, 3, cost, n_d=8)
            X, U, D = rng.normal(size=(50, p)), rng.normal(size=(50, n_u)), rng.normal(size=(50, 8))
            m = rng.integers(0, 3, 50)
            assert np.allclose(es.nominal_step(pl, X, U, m, D), pl.step(X, U, m, D),
                               rtol=1e-13, atol=1e-13)
            assert np.allclose(es.stage_cost(pl, X, U), pl.stage_cost(X, U), rtol=1e-13, atol=0)
            # one accumulator, from 0.0, in the device's order
            s = [[0.] * p for _ in range(50)]
            for q in range(50):
                for i in range(p):
                    a = 0.
                    for c in range(p):
                        a += pl.A[m[q], i, c] * X[q, c]
                    for c in range(n_u):
                        a += pl.B[m[q], i, c] * U[q, c]
                    a += pl.w[m[q], i]
                    for j in range(8):
                        a += pl.E[i, j] * D[q, j]
                    s[q][i] = a
            assert np.array_equal(es.nominal_step(pl, X, U, m, D), np.array(s))
            gp = es.random_guarded(rng, p, n_u, 5, cost, substeps=3, n_rows=6)
            assert np.array_equal(es.stage_cost(gp, X, U), gp.stage_cost(X, U))
            ok = es.in_region(pl, X, m, 0.)
            for q in range(50):
                r = pl.regions[m[q]]
                want = r is None or all(sum(r[0][j][c] * X[q, c] for c in range(p)) <= r[1][j]
                                        for j in range(len(r[1])))
                assert ok[q] == want


@pytest.mark.parametrize('kind', ['nominal', 'noisy', 'guarded'])
def test_mirror_accepts_a_host_rollout_and_catches_one_ulp(kind):
    rng = np.random.default_rng(5)
    p, n_u = 2, 2
    cost = 'inf' if kind != 'noisy' else 'quadratic'
    if kind == 'guarded':
        plant = es.random_guarded(rng, p, n_u, 4, cost, substeps=3, n_rows=5)
    else:
        plant = es.random_plant(rng, p, n_u, 3, cost, n_d=8 if kind == 'nominal' else 0)
    law = es.SynthLaw(es.kuhn_forest(p), n_u, plant.n_modes, rng, no_law=0.2)
    X0 = rng.uniform(-0.95, 0.95, (48, p))
    T = 10
    kw = dict(tol_exit=1e-9)
    if kind == 'noisy':
        kw.update(noise=es.random_noise(rng, p, n_u, plant.n_d), seed=3, traj0=7)
    elif kind == 'nominal':
        kw.update(d=rng.normal(size=(T, 48, 8)), v=rng.normal(size=(T, 48, p)) * 1e-3)
    res = es.host_rollout(law, plant, X0, T, **kw)
    mirror = es.replay(law, plant, res, X0, T, **kw)
    es.check_replay(mirror, res)
    assert (res.steps > 0).any()
    assert (res.status != 0).any()
    q = int(np.argmax(res.steps))
    t = int(res.steps[q]) // 2 + 1
    res.x[t, q, 0] = np.nextafter(res.x[t, q, 0], np.inf)
    with pytest.raises(AssertionError):
        es.replay(law, plant, res, X0, T, **kw)
