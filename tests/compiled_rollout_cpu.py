"""
Numpy mirror of the compiled law's closed loop (k_compiled_rollout) and its check
against exact arithmetic; test infrastructure, host only.

    mir = mirror(arrays, leaf_mode, plant, X0, T, tol_exit, ...)   # the device's order of operations
    skipped, applied = check_exact(law, res, mir.roots, mir.z, plant, leaf_mode, tol_exit)

``mirror`` runs on arrays in the layout of ``CompiledLaw.arrays()``: on exported arrays every
record it returns is bit-equal to the device's (``u_norm_sum`` to the last bit of a square root).
It is built from the pieces the other mirrors already pin: the containment sums, the serial root
rule and the plane walk of ``compiled_cpu``; the plant step, cost, norm, violation and region test
of ``explicit_synth``; ``GuardedPlant.step``; ``NoiseModel.sample``.
"""

from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from tests import compiled_cpu as cc
from tests import explicit_synth as es


def locate_warm(root_rec, nbr, X, p, start):
    """``compiled_cpu._locate`` started at the roots ``start``: the root the visibility walk
    accepts (strictly inside by STRICT), or -1."""
    n = X.shape[0]
    k = np.asarray(start, dtype=np.int64).copy()
    found = np.full(n, -1, dtype=np.int64)
    live = np.arange(n)
    for _ in range(cc.LOCATE_STEPS):
        if live.size == 0:
            break
        alpha, a0 = cc._weights(root_rec[k[live]], X[live], p)
        lo, at = a0.copy(), np.zeros(live.size, dtype=np.int64)
        for i in range(p):
            less = alpha[:, i] < lo
            lo = np.where(less, alpha[:, i], lo)
            at = np.where(less, i + 1, at)
        inside = lo > cc.STRICT
        found[live[inside]] = k[live[inside]]
        k2 = nbr[k[live], at]
        go = ~inside & ~(lo >= -cc.STRICT) & (k2 >= 0)
        k[live[go]] = k2[go]
        live = live[go]
    return found


def walk_from(arrays, h, root, X):
    """The plane walk and the leaf map of ``compiled_cpu.evaluate`` from the roots ``root``:
    (leaf index in the compiled arrays, u)."""
    p, n_u = h['p'], h['n_u']
    n = X.shape[0]
    node = np.ascontiguousarray(arrays['node'], dtype=np.float64).reshape(h['n_int'],
                                                                         h['node_stride'])
    children = node[:, p + 1:p + 2].copy().view(np.int32).reshape(-1, 2)
    k = np.asarray(arrays['root_entry'])[root].astype(np.int64)
    live = np.nonzero(k >= 0)[0]
    while live.size:
        rec = node[k[live]]
        s = np.zeros(live.size)
        for c in range(p):
            s = s + rec[:, c] * X[live, c]
        s = s + rec[:, p]
        k[live] = np.where(s >= -cc.EPS, children[k[live], 0], children[k[live], 1])
        live = live[k[live] >= 0]
    l = ~k
    lr = np.asarray(arrays['leaf_rec'], dtype=np.float64)[l]
    d = X - lr[:, :p]
    u = np.empty((n, n_u))
    for c in range(n_u):
        t = np.zeros(n)
        for q in range(p):
            t = t + lr[:, p + n_u + c * p + q] * d[:, q]
        u[:, c] = lr[:, p + c] + t
    return l, u


def plant_modes(leaf_mode, plant, n_leaf):
    """The table the device holds: zeros for a single-mode nominal plant (CompiledLaw.set_plant)."""
    if plant.n_modes == 1 and not plant.guarded:
        return np.zeros(n_leaf, dtype=np.int32)
    return np.asarray(leaf_mode, dtype=np.int32)


def mirror(arrays, leaf_mode, plant, X0, T, tol_exit=1e-9, d=None, v=None, noise=None, seed=0,
           traj0=0):
    """The rollout of the compiled law in numpy, in the device's order of operations.  Returns the
    records of a ``ClosedLoop`` (x, u, leaf, v, e, w, x_final, steps, status, cost, u_norm_sum,
    max_violation) and, per step, ``roots`` [T, n] (the root chosen, -1 where the trajectory was
    not measured) and ``z`` [T, n, p] (the measured state)."""
    h = dict(zip(cc.HEADER, (int(a) for a in arrays['header'])))
    assert h['n_test'] == 0, 'the rollout takes laws without test nodes'
    p, n_u, R = h['p'], h['n_u'], h['n_roots']
    X0 = np.ascontiguousarray(np.atleast_2d(X0), dtype=np.float64)
    n = X0.shape[0]
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    nbr = np.asarray(arrays['nbr']) if h['has_nbr'] else None
    leaf_node = np.asarray(arrays['leaf_node'])
    modes = plant_modes(leaf_mode, plant, h['n_leaf'])
    ids = np.arange(traj0, traj0 + n, dtype=np.uint64)
    xs = np.full((T + 1, n, p), np.nan)
    us = np.full((T, n, n_u), np.nan)
    leaf = np.full((T, n), -1, dtype=np.int32)
    vs = np.full((T, n, p), np.nan)
    ews = np.full((T, n, n_u), np.nan)
    ws = np.full((T, n, plant.n_d), np.nan)
    roots = np.full((T, n), -1, dtype=np.int64)
    zs = np.full((T, n, p), np.nan)
    xs[0] = X0
    x = X0.copy()
    steps = np.full(n, T, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    cost, unorm = np.zeros(n), np.zeros(n)
    maxv = np.full(n, -np.inf)
    u_prev = np.zeros((n, n_u))
    kr = (np.arange(n) % R).astype(np.int64)
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
        zs[t, live] = z
        # the root
        r = np.full(live.size, -1, dtype=np.int64)
        if nbr is not None:
            r = locate_warm(root_rec, nbr, z, p, kr[live])
        todo = np.nonzero(r < 0)[0]
        r[todo] = cc._first_root(root_rec, z[todo], p)[0]
        kr[live] = r
        roots[t, live] = r
        # the exit test on the root's weights: a conjunction of >=, so that NaN exits
        alpha, a0 = cc._weights(root_rec[r], z, p)
        inside = (a0 >= -tol_exit) & (alpha >= -tol_exit).all(axis=1)
        code = np.where(inside, 0, 1)
        l = np.zeros(live.size, dtype=np.int64)
        u = np.full((live.size, n_u), np.nan)
        w_in = np.nonzero(inside)[0]
        l[w_in], u[w_in] = walk_from(arrays, h, r[w_in], z[w_in])
        m = modes[l]
        no_law = inside & ((m < 0) | ((m >= plant.n_modes) & (not plant.guarded)))
        code[no_law] = 3
        if not plant.guarded:
            ask = np.nonzero(code == 0)[0]
            ok = es.in_region(plant, xt[ask], m[ask], tol_exit)
            code[ask[~ok]] = 2
        stop = code != 0
        steps[live[stop]], status[live[stop]] = t, code[stop]
        go = ~stop
        live, l, m = live[go], l[go], m[go]
        if live.size == 0:
            break
        xl, ul = x[live], u[go]
        us[t, live] = ul
        leaf[t, live] = leaf_node[l]
        cost[live] = cost[live] + es.stage_cost(plant, xl, ul)
        nrm, su = es.u_norm(ul)
        unorm[live] = unorm[live] + nrm
        if noise is not None:
            e = noise.sample('input', seed, ids[live], t, xl, ul)
            e[su == 0.] = 0.
            w = noise.sample('process', seed, ids[live], t, xl, ul)
            ews[t, live], ws[t, live] = e, w
            u_prev[live] = ul
            xn = es.nominal_step(plant, xl, ul + e, m, w if plant.n_d else None)
        elif plant.guarded:
            xn = plant.step(xl, ul)
        else:
            xn = es.nominal_step(plant, xl, ul, m, None if d is None else d[t, live])
        maxv[live] = np.fmax(maxv[live], es.violation(plant, xn))
        x[live] = xn
        xs[t + 1, live] = xn
    out = SimpleNamespace(x=xs, u=us, leaf=leaf, x_final=x, steps=steps, status=status, cost=cost,
                          u_norm_sum=unorm, max_violation=maxv, roots=roots, z=zs,
                          v=None, e=None, w=None)
    if noise is not None:
        out.v, out.e, out.w = vs, ews, ws
    return out


BIT_EQUAL = ('steps', 'status', 'x', 'u', 'leaf', 'v', 'e', 'w', 'x_final', 'cost',
             'max_violation')


def assert_same(res, mir, record=True):
    """A device result against the mirror: bit for bit, ``u_norm_sum`` to rtol 1e-15 (the
    allowance ``explicit_synth.check_replay`` makes)."""
    for f in BIT_EQUAL:
        a, b = getattr(res, f), getattr(mir, f)
        if not record and f in ('x', 'u', 'leaf', 'v', 'e', 'w'):
            assert a is None, f
            continue
        if b is None:
            assert a is None, f
            continue
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), f
    assert np.allclose(res.u_norm_sum, mir.u_norm_sum, rtol=1e-15, atol=0)


def check_exact(law, res, roots, z, plant, leaf_mode, tol_exit):
    """
    A rollout record (device or mirror) of the compiled ``SynthLaw`` against exact arithmetic, per
    applied step and at the step a trajectory stopped: the walk to the recorded leaf
    (``compiled_cpu.check_plane_path``, below the root the rollout chose), the exact leaf where
    the step is decisive, the input within ``u_tol`` (c = 64); the exit test on the exact weights
    of z in the chosen root with slack 64 eps (1 + kappa(root)); statuses 2 and 3 from the region
    and the mode of the exact leaf where the step is decisive.  Returns (skipped, applied): the
    applied steps skipped as non-decisive, of how many; at most a quarter may be.
    """
    T, n = roots.shape
    modes = plant_modes(leaf_mode, plant, law.leaves.size)
    mode_of = dict(zip((int(k) for k in law.leaves), (int(m) for m in modes)))
    tol = Fraction(tol_exit)
    skipped = applied = 0
    for q in range(n):
        for t in range(min(int(res.steps[q]) + 1, T)):
            on = t < res.steps[q]
            code = 0 if on else int(res.status[q])
            if not on and code == 0:
                break
            r = int(roots[t, q])
            if not np.all(np.isfinite(z[t, q])):
                assert code == 1, (t, q)
                continue
            ref = law.locate(z[t, q])
            lo = Fraction(min(law.forest.root_weights(r, ref.Y, ref.D)), ref.D)
            slack = Fraction(64 * es.EPS) * (1 + Fraction(law.kappa(r)))
            if code == 1:
                assert lo < -tol + slack, (t, q, float(lo))
                continue
            assert lo >= -tol - slack, (t, q, float(lo))
            dec = law.decisive(ref)
            if not on:
                if not dec:
                    continue
                m = mode_of[ref.leaf]
                if code == 3:
                    assert m < 0, (t, q)
                else:
                    assert code == 2 and not plant.guarded and m >= 0, (t, q, code)
                    assert not es.in_region(plant, res.x[t, q][None], [m], tol_exit)[0], (t, q)
                continue
            applied += 1
            k = int(res.leaf[t, q])
            top = k
            while law.parent[top] >= 0:
                top = int(law.parent[top])
            assert top == r, (t, q, top, r)
            lam = cc.check_plane_path(law, k, ref)
            ue = law.u_exact(k, lam, ref.D)
            bound = law.u_tol(max(ref.kappa, law.kappa(k)), lam, ref.D, c=64.)
            assert np.all(np.abs(res.u[t, q] - ue) <= bound), (t, q, res.u[t, q], ue, bound)
            if not dec:
                skipped += 1
                continue
            assert k == ref.leaf, (t, q, k, ref.leaf, float(ref.margin))
            m = mode_of[k]
            assert m >= 0, (t, q)
            if not plant.guarded:
                assert es.in_region(plant, res.x[t, q][None], [m], tol_exit)[0], (t, q)
    assert 4 * skipped <= applied, (skipped, applied)
    return skipped, applied


# -- the cases the host and the device tests share ----------------------------------------------
KINDS = ('nominal', 'noisy', 'guarded')       # PlantKind order
N_TRAJ, T_STEPS = 256, 16


def case(kind, p, n_u):
    """The law, plant, initial states and rollout arguments of one (kind, p, n_u): the recipe of
    tests/test_gpu_explicit_widths._case, restated."""
    rng = np.random.default_rng([KINDS.index(kind), p, n_u])
    cost = 'inf' if (p + n_u + KINDS.index(kind)) % 2 == 0 else 'quadratic'
    kw = dict(tol_exit=1e-9)
    if kind == 'guarded':
        n_modes = 2 + (p + n_u) % 7
        plant = es.random_guarded(rng, p, n_u, n_modes, cost, substeps=1 + (p * n_u) % 4,
                                  n_rows=1 + (p + 3 * n_u) % 16)
    else:
        n_modes = 1 + (p + 2 * n_u) % 4
        n_d = 8 if (p + n_u) % 2 else 0
        plant = es.random_plant(rng, p, n_u, n_modes, cost, n_d=n_d)
    law = es.SynthLaw(es.kuhn_forest(p), n_u, n_modes, rng)
    X0 = np.concatenate([rng.uniform(-0.9, 0.9, (N_TRAJ // 2, p)),
                         law.states(rng, N_TRAJ)[:N_TRAJ // 2]])
    if kind == 'noisy':
        kw.update(noise=es.random_noise(rng, p, n_u, plant.n_d), seed=int(rng.integers(1 << 40)),
                  traj0=int(rng.integers(1 << 20)))
    elif kind == 'nominal':
        kw['v'] = rng.normal(size=(T_STEPS, X0.shape[0], p)) * 1e-3
        if plant.n_d:
            kw['d'] = rng.normal(size=(T_STEPS, X0.shape[0], plant.n_d))
    return law, plant, X0, kw


def leaf_modes(law, arrays):
    """The law's modes in the order of the compiled leaves."""
    return np.ascontiguousarray(law.node_mode()[np.asarray(arrays['leaf_node'])], dtype=np.int32)
