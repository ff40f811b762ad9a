"""
Numpy mirror of the per-leaf error boxes of the noisy closed loop and of the two checks that read them
(csrc/ehm_noise_box_dev.h, csrc/ehm_radii_dev.h, the LEAF instances of csrc/ehm_robust.hip and
csrc/ehm_core.hip); test infrastructure, host only.

    bb = boxes_at(model, a, b)                      # {'process': (lo, hi), ..} at |x| <= a, |u| <= b
    rad = leaf_radii(model, plant, V, U, Y, modes, x_abs, u_abs, iters=3)
    rad.boxes, rad.x_abs_leaf, rad.x_next_abs, rad.u_abs_leaf, rad.lo, rad.hi, rad.iterates
    out = successors(arrays, leaf_mode, plant, model, x_abs, u_abs, iters=3, leaves=None, ...)
    out = core(arrays, leaf_mode, plant, model, x_abs, u_abs, iters=3, ...)

``boxes_at`` takes a [n, p] and b [n, n_u] (or one row each) and sums in the device's loop order:
terms in model order, every sum from 0.0.  The cells, the vertex inputs and the nominal vertex
successors are ``tests/invariance_cpu.successors``', the facets, the region rows and the beats rule
``tests/robust_cpu``'s, the relation ``tests/core_cpu``'s with the leaf's own box in its ``Image``.
"""

from types import SimpleNamespace

import numpy as np

from explicit_hybrid_mpc_amd import invariance
from explicit_hybrid_mpc_amd.noise import KINDS
from tests import certify_cpu as zc
from tests import core_cpu as kc
from tests import invariance_cpu as iv
from tests import robust_cpu as rb

INVARIANT, EXITS, MODE_REGION, NO_MODE, NO_CELL = range(5)


def boxes_at(model, a, b, kinds=KINDS):
    """{kind: (lo [n, out], hi [n, out])}: ``noise_box`` of every kind at the rows of a and b."""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    b = np.atleast_2d(np.asarray(b, dtype=np.float64))
    n = max(a.shape[0], b.shape[0])
    a = np.broadcast_to(a, (n, model.n_x))
    b = np.broadcast_to(b, (n, model.n_u))
    out = {}
    for kind in kinds:
        n_out = model.out_dim(kind)
        lo, hi = np.zeros((n, n_out)), np.zeros((n, n_out))
        for term in model.terms:
            if term.kind != kind:
                continue
            M, dim = term.map, term.dim
            if term.shape == 'box':
                for i in range(n_out):
                    mid, rad = 0., 0.
                    for k in range(dim):
                        mid = mid + M[i, k] * term.c[k]
                        rad = rad + abs(M[i, k]) * term.h[k]
                    lo[:, i] = lo[:, i] + (mid - rad)
                    hi[:, i] = hi[:, i] + (mid + rad)
                continue
            r = np.full(n, float(term.sigma))
            if term.dep != 'const':
                F = np.abs(np.asarray(term.F, dtype=np.float64))
                X = a if term.dep == 'state' else b
                nrm = np.zeros(n)
                with np.errstate(invalid='ignore', over='ignore'):
                    for i in range(F.shape[0]):
                        y = np.zeros(n)
                        for c in range(F.shape[1]):
                            y = y + F[i, c] * X[:, c]
                        if term.p_dep == 0:
                            nrm = np.fmax(nrm, np.abs(y))
                        elif term.p_dep == 1:
                            nrm = nrm + np.abs(y)
                        else:
                            nrm = nrm + y * y
                    if term.p_dep == 2:
                        nrm = np.sqrt(nrm)
                    r = r * nrm
            for i in range(n_out):
                dual = 0.
                for k in range(dim):
                    L = abs(float(M[i, k]))
                    if term.norm == 2:
                        dual = dual + L * L
                    elif term.norm == 0:
                        dual = dual + L
                    else:
                        dual = max(dual, L)
                if term.norm == 2:
                    dual = float(np.sqrt(dual))
                with np.errstate(invalid='ignore', over='ignore'):
                    w = r * dual
                    lo[:, i] = lo[:, i] - w
                    hi[:, i] = hi[:, i] + w
        out[kind] = (lo, hi)
    return out


def half_of(lo, hi):
    """The larger modulus of the two bounds (the first on ties: the same number)."""
    return np.where(np.abs(lo) > np.abs(hi), np.abs(lo), np.abs(hi))


def _max_abs(X):
    """max_i |X[:, i, c]| in vertex order: the first, then a strict >."""
    t = np.abs(X[:, 0])
    for i in range(1, X.shape[1]):
        s = np.abs(X[:, i])
        t = np.where(s > t, s, t)
    return t


def has_kinds(model, plant):
    """Which kinds have generator columns: those with terms (process: and a plant with n_d > 0)."""
    has = {k: any(t.kind == k for t in model.terms) for k in KINDS}
    has['process'] = has['process'] and plant.n_d > 0
    return has


def leaf_radii(model, plant, V, U, Y, modes, x_abs, u_abs, iters=3):
    """Steps 1 to 4 of DESIGN.md 3.8k for the live leaves: cells V [L, p+1, p], vertex inputs
    U [L, p+1, n_u], vertex successors Y [L, p+1, p], modes [L]."""
    L, nv, p = V.shape
    n_u, n_d = U.shape[2], plant.n_d
    x_abs = np.asarray(x_abs, dtype=np.float64).reshape(p)
    u_abs = np.asarray(u_abs, dtype=np.float64).reshape(n_u)
    has = has_kinds(model, plant)
    with np.errstate(invalid='ignore', over='ignore'):
        cL = _max_abs(V)
        ub = _max_abs(U)
        ug = np.broadcast_to(u_abs, (L, n_u))
        a = np.broadcast_to(x_abs, (L, p)).copy()
        iterates = [a.copy()]
        for _ in range(int(iters)):
            lo, hi = boxes_at(model, a, ug, ('state',))['state']
            t = cL + half_of(lo, hi)
            a = np.where(t < a, t, a)
            iterates.append(a.copy())
        v = boxes_at(model, a, ug, ('state',))['state']
        de = boxes_at(model, a, ub, ('process', 'input'))
        d, e = de['process'], de['input']
        xp = _max_abs(Y)
        A = np.abs(np.asarray(plant.A, dtype=np.float64).reshape(-1, p, p))[modes]
        B = np.abs(np.asarray(plant.B, dtype=np.float64).reshape(-1, p, n_u))[modes]
        if has['process']:
            E = np.abs(np.asarray(plant.E, dtype=np.float64).reshape(p, n_d))
            h = half_of(*d)
            for k in range(n_d):
                for c in range(p):
                    xp[:, c] = xp[:, c] + E[c, k] * h[:, k]
        h = half_of(*v)
        for k in range(p):
            for c in range(p):
                xp[:, c] = xp[:, c] + A[:, c, k] * h[:, k]
        h = half_of(*e)
        for k in range(n_u):
            for c in range(p):
                xp[:, c] = xp[:, c] + B[:, c, k] * h[:, k]
        a_next = np.where(xp < x_abs, xp, np.broadcast_to(x_abs, (L, p)))
        vn = boxes_at(model, a_next, ub, ('state',))['state']
    stack = lambda box: np.stack(box, axis=1)                   # [L, 2, dim]
    boxes = dict(process=stack(d) if has['process'] else None,
                 state=stack(v) if has['state'] else None,
                 input=stack(e) if has['input'] else None,
                 state_next=stack(vn) if has['state'] else None)
    cols = [boxes[k] for k in ('process', 'state', 'input', 'state_next') if boxes[k] is not None]
    both = np.concatenate(cols, axis=2) if cols else np.zeros((L, 2, 0))
    return SimpleNamespace(boxes=boxes, x_abs_leaf=a, x_next_abs=a_next, u_abs_leaf=ub,
                           lo=both[:, 0], hi=both[:, 1], iterates=iterates, c_leaf=cL,
                           v=v, has=has)


def facet_ng(normals, G):
    """nG [n_f, n_modes, n_g]: ((0 + n_0 G_0k) + ..), the sum of ``robust_cpu.facet_slack``."""
    n_f, p = normals.shape
    n_modes, _, n_g = G.shape
    out = np.zeros((n_f, n_modes, n_g))
    for m in range(n_modes):
        for k in range(n_g):
            ng = np.zeros(n_f)
            for c in range(p):
                ng = ng + normals[:, c] * G[m, c, k]
            out[:, m, k] = ng
    return out


def region_holds(plant, V, modes, v_lo, v_hi, tol_exit):
    """``robust_cpu.region_holds`` with a v box per leaf (v_lo, v_hi [L, p])."""
    L, nv, p = V.shape
    rows, H, h = plant.region_arrays()
    rows = np.asarray(rows, dtype=np.int64)
    H = np.asarray(H, dtype=np.float64).reshape(-1, p)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    row0 = np.concatenate([[0], np.cumsum(rows)])
    ok = np.ones(L, dtype=bool)
    for m in range(plant.n_modes):
        at = np.nonzero(modes == m)[0]
        if at.size == 0:
            continue
        for r in range(row0[m], row0[m + 1]):
            smax = None
            for i in range(nv):
                s = np.zeros(at.size)
                for c in range(p):
                    s = s + H[r, c] * V[at, i, c]
                smax = s if smax is None else np.where(s > smax, s, smax)
            rs = np.zeros(at.size)
            for c in range(p):
                g = 0. - H[r, c]
                a, b = g * v_lo[at, c], g * v_hi[at, c]
                rs = rs + np.where(a > b, a, b)
            ok[at] &= (smax + rs) <= h[r] + tol_exit
    return ok


def successors(arrays, leaf_mode, plant, model, x_abs, u_abs, iters=3, leaves=None, roots=None,
               tol_exit=1e-9, tol_set=1e-9, nominal=None):
    """``robust_cpu.successors`` with the box of every leaf its own.  The per-leaf arrays cover the
    requested leaves, NaN where a leaf has no cell or mode."""
    h = zc.header(arrays)
    p, n_u = h['p'], h['n_u']
    roots = zc.root_vertices(arrays) if roots is None else roots
    normals, offsets, convex = invariance.boundary_facets(roots)
    if nominal is None:
        nominal = iv.successors(arrays, leaf_mode, plant, leaves=leaves, roots=roots,
                                tol_exit=tol_exit)
    n = nominal.status.size
    has = has_kinds(model, plant)
    zero = lambda k: (np.zeros(k), np.zeros(k))
    G, _, _ = rb.generators(plant, p, n_u, zero(plant.n_d) if has['process'] else None,
                            zero(p) if has['state'] else None, zero(n_u) if has['input'] else None)
    n_g = G.shape[2]
    nG = facet_ng(normals, G)
    thr = float(tol_set) * float(np.abs(roots).max())
    status = np.where(nominal.status >= NO_MODE, nominal.status, INVARIANT).astype(np.int32)
    margin = np.full(n, np.nan)
    worst = np.full(n, -1, dtype=np.int32)
    Y = nominal.x_next[:, :, 0, :]
    live = np.nonzero(status == INVARIANT)[0]
    dims = dict(process=plant.n_d, state=p, input=n_u, state_next=p)
    kind_of = dict(process='process', state='state', input='input', state_next='state')
    boxes = {k: np.full((n, 2, d), np.nan) if has[kind_of[k]] else None for k, d in dims.items()}
    x_abs_leaf, x_next_abs = np.full((n, p), np.nan), np.full((n, p), np.nan)
    u_abs_leaf = np.full((n, n_u), np.nan)
    lo, hi = np.full((n, n_g), np.nan), np.full((n, n_g), np.nan)
    rad = None
    if live.size:
        L = live.size
        modes = nominal.modes[live]
        rad = leaf_radii(model, plant, nominal.vertices[live], nominal.inputs[live], Y[live], modes,
                         x_abs, u_abs, iters)
        for k in boxes:
            if boxes[k] is not None:
                boxes[k][live] = rad.boxes[k]
        x_abs_leaf[live], x_next_abs[live], u_abs_leaf[live] = \
            rad.x_abs_leaf, rad.x_next_abs, rad.u_abs_leaf
        lo[live], hi[live] = rad.lo, rad.hi
        v_lo, v_hi = rad.v if has['state'] else (np.zeros((L, p)), np.zeros((L, p)))
        in_region = region_holds(plant, nominal.vertices[live], modes, v_lo, v_hi, tol_exit)
        best, best_at = np.zeros(L), np.full(L, -1, dtype=np.int32)
        all_hold = np.ones(L, dtype=bool)
        with np.errstate(invalid='ignore', over='ignore'):
            for f in range(normals.shape[0]):
                mn, at = None, np.zeros(L, dtype=np.int32)
                for i in range(p + 1):
                    s = np.zeros(L)
                    for c in range(p):
                        s = s + normals[f, c] * Y[live, i, c]
                    if mn is None:
                        mn = s
                    else:
                        b = iv.beats(s, mn)
                        mn, at = np.where(b, s, mn), np.where(b, i, at).astype(np.int32)
                sl = np.zeros(L)
                for k in range(n_g):
                    a, b = nG[f, modes, k] * rad.lo[:, k], nG[f, modes, k] * rad.hi[:, k]
                    sl = sl + np.where(a < b, a, b)
                val = (mn - offsets[f]) + sl
                all_hold &= val >= -thr
                b = (best_at < 0) | iv.beats(val, best)
                best = np.where(b, val, best)
                best_at = np.where(b, f * (p + 1) + at, best_at).astype(np.int32)
        margin[live], worst[live] = best, best_at
        status[live] = np.where(~in_region, MODE_REGION, np.where(all_hold, INVARIANT, EXITS))
    counts = [int((status == k).sum()) for k in range(5)]
    worst_leaf, worst_margin = -1, np.nan
    for q in np.nonzero(((status == INVARIANT) | (status == EXITS)) & ~np.isnan(margin))[0]:
        if worst_leaf < 0 or margin[q] < worst_margin:
            worst_leaf, worst_margin = int(q), float(margin[q])
    return SimpleNamespace(status=status, margin=margin, worst=worst, counts=counts,
                           worst_leaf=worst_leaf, worst_margin=worst_margin, G=G, nG=nG, lo=lo, hi=hi,
                           leaf_boxes=boxes, x_abs_leaf=x_abs_leaf, x_next_abs=x_next_abs,
                           u_abs_leaf=u_abs_leaf, y=Y, vertices=nominal.vertices,
                           modes=nominal.modes, set_convex=convex, n_facets=normals.shape[0],
                           n_generators=n_g, nominal=nominal, normals=normals, offsets=offsets,
                           radii=rad)


def core(arrays, leaf_mode, plant, model, x_abs, u_abs, iters=3, tol_exit=1e-9, tol_set=1e-9,
         tol_side=None, rows='invariant', max_fan=4096, roots=None, seeds=None):
    """``robust_cpu.core`` with the image of leaf l spanned by G_m and the leaf's own box."""
    h = zc.header(arrays)
    assert h['n_test'] == 0
    n_leaf = h['n_leaf']
    tol_side = float(tol_exit) if tol_side is None else float(tol_side)
    single = zc.is_single(arrays)
    roots = zc.root_vertices(arrays) if roots is None else roots
    if seeds is None:
        seeds = successors(arrays, leaf_mode, plant, model, x_abs, u_abs, iters, roots=roots,
                           tol_exit=tol_exit, tol_set=tol_set)
    Y, G = seeds.y, seeds.G
    node = np.ascontiguousarray(arrays['node']).reshape(h['n_int'], h['node_stride'])
    ch = zc.children(arrays)
    entry = np.asarray(arrays['root_entry'])
    root_rec = np.asarray(arrays['root_rec'], dtype=np.float64)
    box_lo, box_hi = kc.root_boxes(roots)
    status = seeds.status.astype(np.int32).copy()
    wanted = status < NO_MODE
    if rows != 'all':
        wanted &= status == INVARIANT
    wanted &= np.isfinite(Y).all(axis=(1, 2))
    rows_out = [[] for _ in range(n_leaf)]
    for l in np.nonzero(wanted)[0]:
        E = G[seeds.modes[l]] if seeds.n_generators else None
        img = kc.Image(Y[l], E, seeds.lo[l], seeds.hi[l])
        out, ok = [], True
        for r in kc.candidate_roots(img, root_rec, box_lo, box_hi, tol_side):
            ok = kc.descend(img, node, ch, entry[r], single, tol_side, out, max_fan)
            if not ok:
                break
        if ok:
            rows_out[l] = out
        else:
            status[l] = kc.UNRESOLVED
    indptr = np.zeros(n_leaf + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows_out])
    indices = np.array([t for r in rows_out for t in r], dtype=np.int32)
    level = kc.fixed_point(status != INVARIANT, indptr, indices)
    counts = [int((level < 0).sum()), int((level > 0).sum())] + \
        [int(((level == 0) & (status == s)).sum()) for s in range(1, 6)]
    return SimpleNamespace(level=level, core=level < 0, status=status,
                           counts=dict(zip(kc.COUNT_NAMES, counts)), n_sweeps=int(level.max()) + 1,
                           indptr=indptr, indices=indices, n_edges=int(indices.size), seeds=seeds,
                           vertices=seeds.vertices, y=Y, tol_side=tol_side)


# -- the anisotropic cube the host and the device tests share (the exact case) ------
SIGMA = 5. / 64
ANISO_K = -np.diag([1. / 8, 1. / 2])


def aniso_model():
    """One state term on coordinate 0 whose radius is sigma |x_1|: L = e_0, Fx = e_1', px = inf."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    m = NoiseModel(2, 2, 0)
    m.addDependentTerm('state', SIGMA, norm=np.inf, L=np.array([[1.], [0.]]),
                       Fx=np.array([[0., 1.]]), px=np.inf)
    return m


def aniso_closed_form(V):
    """(margin, M0, c1) of every leaf with cell V [n, 3, 2] under per-leaf radii:
    z0+ = 7/8 z0 - v0 + v0', |v0| <= sigma c1, |v0'| <= sigma c1 / 2, z1+ = z1 / 2."""
    M0, c1 = np.abs(V[:, :, 0]).max(axis=1), np.abs(V[:, :, 1]).max(axis=1)
    return 1. - (7. / 8 * M0 + SIGMA * 1.5 * c1), M0, c1


def scaled_model(half, n_u, n_d, scale=1., rng=None):
    """``noise.state_input_model(half, n_u)`` with every half-width and every sigma times ``scale``,
    and with n_d > 0 a box and a state-dependent ball of kind process: a model with a fixed, a
    state-dependent and an input-dependent part in a plant with process inputs."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    base = state_input_model(half, n_u)
    m = NoiseModel(base.n_x, n_u, n_d)
    for t in base.terms:
        if t.shape == 'box':
            m.addIndependentTerm(t.kind, lb=scale * (t.c - t.h), ub=scale * (t.c + t.h), M=t.map)
        else:
            kw = {} if t.dep == 'const' else \
                (dict(Fx=t.F, px=(np.inf, 1, 2)[t.p_dep]) if t.dep == 'state' else
                 dict(Fu=t.F, pu=(np.inf, 1, 2)[t.p_dep]))
            m.addDependentTerm(t.kind, scale * t.sigma, norm=(np.inf, 1, 2)[t.norm], L=t.map, **kw)
    if n_d:
        rng = np.random.default_rng(0) if rng is None else rng
        m.addIndependentTerm('process', lb=-scale * np.ones(n_d), ub=scale * np.linspace(0.5, 1., n_d))
        m.addDependentTerm('process', 0.5 * scale, norm=2, dim=min(n_d, 3),
                           L=np.eye(n_d)[:, :min(n_d, 3)],
                           Fx=rng.uniform(-1., 1., (2, base.n_x)), px=1)
    return m
