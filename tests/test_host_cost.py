"""
Certified fuel bounds of a compiled law's closed loop (invariance.py) without a
device: the numpy mirror (tests/cost_cpu.py) on hand-made graphs with exact numbers, the properties
every result has on random graphs (against Karp's cycle means among them), the refusals ``cost``
makes before it uses the device, and the entry point's host checks (csrc/ehm_cost_host.h) under the
sanitizers.
"""

import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import cost_cpu as co
from tests.test_host_reach import csr, mask_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_properties(out, indptr, indices, domain, start=None):
    """What holds of every result with weights >= 0, whatever computed it."""
    start = domain if start is None else start
    H = out.horizon
    assert (out.lo[domain] <= out.hi[domain]).all()
    assert np.isnan(out.hi[~domain]).all() and np.isnan(out.lo[~domain]).all()
    assert (out.min_lo <= out.start_lo).all() and (out.start_lo <= out.start_hi).all()
    assert (out.start_hi <= out.max_hi).all()
    assert out.max_hi[0] == 0. and out.min_lo[0] == 0.
    assert out.max_hi[H] == out.hi[domain].max() and out.min_lo[H] == out.lo[domain].min()
    ends = bool(((np.diff(indptr) == 0) & domain).any())     # a walk that ends spends no more
    for a in range(H + 1):
        for b in range(H + 1 - a):
            assert out.max_hi[a + b] <= out.max_hi[a] + out.max_hi[b], (a, b)
            assert ends or out.min_lo[a + b] >= out.min_lo[a] + out.min_lo[b], (a, b)
    assert np.isnan(out.rate_hi[0]) and np.isnan(out.rate_lo[0])
    assert out.best_rate_hi == out.rate_hi[1:].min() == out.rate_hi[out.best_k_hi]
    assert out.best_rate_lo == out.rate_lo[1:].max() == out.rate_lo[out.best_k_lo]
    # each path is a path of the relation from the first start leaf that attains the bound, and its
    # right-nested weight sum is the bound bit for bit
    rows = np.nonzero(start)[0]
    for path, w, value, bound in ((out.path_hi, out.w_hi, out.hi, out.start_hi[H]),
                                  (out.path_lo, out.w_lo, out.lo, out.start_lo[H])):
        assert path.dtype == np.int32 and path.shape == (H + 1,)
        assert path[0] == rows[value[rows] == bound][0]
        for t in range(H):
            l, to = int(path[t]), int(path[t + 1])
            if l < 0:
                assert to == -1
                continue
            row = indices[indptr[l]:indptr[l + 1]]
            assert (to == -1 and row.size == 0) or to in row
        assert co.right_nested(w, path) == value[path[0]] == bound


def test_a_tail_of_four_into_a_three_cycle():
    # 0 -> 1 -> 2 -> 3 -> 4 -> 5 -> 6 -> 4; the tail weighs 1 a leaf, the cycle 1, 2, 3
    indptr, indices = csr([[1], [2], [3], [4], [5], [6], [4]])
    w = np.array([1., 1., 1., 1., 1., 2., 3.])
    D = np.ones(7, dtype=bool)
    out = co.bounds(indptr, indices, D, w, w, 12, start=mask_of(7, [0]))
    check_properties(out, indptr, indices, D, mask_of(7, [0]))
    assert np.array_equal(out.hi, out.lo)
    for k in (3, 6, 9, 12):
        assert out.rate_hi[k] == 2.
    assert (out.rate_hi[1:] >= 2.).all() and out.best_rate_hi == 2. and out.best_k_hi == 3
    assert out.max_hi.tolist() == [0., 3., 5., 6., 9., 11., 12., 15., 17., 18., 21., 23., 24.]
    # from the tail's head: 4 steps of 1, then 8 around the cycle from its lightest leaf
    assert out.hi[0] == 4. + (1. + 2. + 3.) * 2 + 1. + 2. == out.start_hi[12]
    assert out.path_hi.tolist() == [0, 1, 2, 3, 4, 5, 6, 4, 5, 6, 4, 5, 6]
    assert out.path_lo.tolist() == out.path_hi.tolist()
    assert out.start_hi[:6].tolist() == [0., 1., 2., 3., 4., 5.]
    assert co.cycle_mean(indptr, indices, D, w, True) == 2.
    assert co.cycle_mean(indptr, indices, D, w, False) == 2.
    # the cycle alone is a closed domain too
    cyc = mask_of(7, [4, 5, 6])
    sub = co.bounds(indptr, indices, cyc, w, w, 12)
    check_properties(sub, indptr, indices, cyc)
    assert np.array_equal(sub.max_hi, out.max_hi) and sub.min_lo[3] == 6. and sub.rate_lo[3] == 2.
    with pytest.raises(AssertionError, match='not closed'):
        co.bounds(indptr, indices, mask_of(7, [0, 1]), w, w, 3)


def test_a_self_loop():
    indptr, indices = csr([[0]])
    D = np.ones(1, dtype=bool)
    out = co.bounds(indptr, indices, D, [1.5], [0.25], 7)
    check_properties(out, indptr, indices, D)
    assert out.max_hi.tolist() == [1.5 * k for k in range(8)]
    assert out.min_lo.tolist() == [0.25 * k for k in range(8)]
    assert (out.rate_hi[1:] == 1.5).all() and (out.rate_lo[1:] == 0.25).all()
    assert out.best_k_hi == 1 and out.best_k_lo == 1
    assert (out.arg_hi == 0).all() and out.path_hi.tolist() == [0] * 8


def test_two_cycles_of_different_mean():
    # 0 <-> 1 weighs 1, 3 (mean 2); 2 -> 3 -> 4 -> 2 weighs 5, 5, 8 (mean 6); 5 feeds both
    indptr, indices = csr([[1], [0], [3], [4], [2], [0, 2]])
    w = np.array([1., 3., 5., 5., 8., 0.])
    D = np.ones(6, dtype=bool)
    out = co.bounds(indptr, indices, D, w, w, 12)
    check_properties(out, indptr, indices, D)
    assert out.best_rate_hi == 6. == co.cycle_mean(indptr, indices, D, w, True)
    assert out.best_k_hi == 3
    # the feeder's free step keeps min_lo below the small cycle's mean until it is dropped
    both = mask_of(6, [0, 1, 2, 3, 4])
    out = co.bounds(indptr, indices, both, w, w, 12)
    check_properties(out, indptr, indices, both)
    assert out.best_rate_hi == 6. and out.best_rate_lo == 2. and out.best_k_lo == 2
    assert co.cycle_mean(indptr, indices, both, w, False) == 2.
    # the worst path stays in the heavy cycle, the best in the light one; 12 steps are whole turns
    # of both, so every leaf of a cycle attains its bound and the smallest starts the path
    assert out.path_hi.tolist() == [2, 3, 4] * 4 + [2]
    assert out.path_lo.tolist() == [0, 1] * 6 + [0]
    assert out.hi[2:5].tolist() == [72.] * 3 and out.lo[:2].tolist() == [24.] * 2
    odd = co.bounds(indptr, indices, both, w, w, 10)         # ten steps: from the heaviest leaf    
    assert odd.path_hi.tolist() == [4, 2, 3] * 3 + [4, 2] and odd.hi[4] == 18. * 3 + 8.
    # ties: equal weights, so every leaf attains every bound and the smallest index decides
    flat = co.bounds(indptr, indices, D, np.ones(6), np.ones(6), 4)
    assert flat.path_hi.tolist() == [0, 1, 0, 1, 0] and flat.arg_hi[3].tolist() == [1, 0, 3, 4, 2, 0]


def test_a_leaf_with_an_empty_row():
    # 0 -> 1, 1 has no row: nothing is claimed past it; 2 -> {1, 2} can go on for ever
    indptr, indices = csr([[1], [], [1, 2]])
    w_hi, w_lo = np.array([2., 5., 1.]), np.array([1., 4., 1.])
    D = np.ones(3, dtype=bool)
    out = co.bounds(indptr, indices, D, w_hi, w_lo, 4)
    check_properties(out, indptr, indices, D)
    assert out.hi.tolist() == [7., 5., 8.] and out.lo.tolist() == [5., 4., 4.]
    assert (out.arg_hi[:, 1] == -1).all() and (out.arg_lo[:, 1] == -1).all()
    assert out.path_hi.tolist() == [2, 2, 2, 1, -1] and out.max_hi.tolist() == [0., 5., 7., 7., 8.]
    one = co.bounds(indptr, indices, D, w_hi, w_lo, 4, start=mask_of(3, [0]))
    assert one.path_hi.tolist() == [0, 1, -1, -1, -1] and one.start_hi.tolist() == [0., 2., 7., 7., 7.]
    # duplicates within a row change nothing
    again = co.bounds(*csr([[1, 1], [], [2, 1, 2, 1]]), D, w_hi, w_lo, 4)
    assert np.array_equal(again.hi, out.hi) and np.array_equal(again.arg_hi, out.arg_hi)


@pytest.mark.parametrize('seed', range(6))
def test_properties_on_random_graphs(seed):
    rng = np.random.default_rng([31, seed])
    n = int(rng.integers(2, 40))
    # every row nonempty (so a cycle exists), integer weights (so every sum is exact)
    rows = [rng.integers(0, n, rng.integers(1, 5)).tolist() for _ in range(n)]
    if seed % 2:
        rows[int(rng.integers(0, n))] = []
    indptr, indices = csr(rows)
    w_lo = rng.integers(0, 4 if seed < 4 else 2, n).astype(np.float64)
    w_hi = w_lo + rng.integers(0, 4 if seed < 4 else 1, n)
    # the closure of a few leaves is a closed domain; so is every leaf
    seen = mask_of(n, rng.integers(0, n, 2))
    while True:
        more = seen.copy()
        more[indices[np.repeat(seen, np.diff(indptr))]] = True
        if np.array_equal(more, seen):
            break
        seen = more
    for D in (np.ones(n, dtype=bool), seen):
        S = D & (rng.random(n) < 0.5)
        S[np.nonzero(D)[0][0]] = True
        out = co.bounds(indptr, indices, D, w_hi, w_lo, 2 * n, start=S)
        check_properties(out, indptr, indices, D, S)
        top = co.cycle_mean(indptr, indices, D, w_hi, True)
        low = co.cycle_mean(indptr, indices, D, w_lo, False)
        empty = (np.diff(indptr) == 0) & D
        if top is None:
            assert empty.any()
            continue
        assert (out.rate_hi[1:] >= top).all()
        assert top >= co.cycle_mean(indptr, indices, D, w_hi, False) >= low
        if not empty.any():                 # a walk that ends spends nothing more: no lower claim
            assert (out.rate_lo[1:] <= low).all()
            # U_K reaches K times the mean at a multiple of the critical cycle's length
            assert out.best_rate_hi == top or out.best_k_hi > n


@pytest.mark.parametrize('p', [2, 3])
def test_the_weights_of_a_cube_law(p):
    """The mirror's weights on the cube law u = K x + c of both precisions: the bounds hold the
    2-norm of the exact map at the vertices and at 200 points inside every cell, and the pad is the
    stated multiple of eps |R|."""
    from tests import certify_cpu as zc
    from tests import compiled_cpu as cc
    from tests import invariance_cpu as iv
    rng = np.random.default_rng([37, p])
    K = rng.uniform(-1., 1., (p, p))
    c = rng.uniform(-0.2, 0.2, p)
    arrays, _ = cc.compile_flat(iv.cube_law(p, K, c=c))
    for arr, eps in ((arrays, 2. ** -53), (zc.narrow_flushed(arrays), 2. ** -24)):
        V, st = zc.cells(arr)
        assert (st == zc.CELL).all()
        U = zc.vertex_inputs(arr, np.arange(V.shape[0]), V, st)
        w_hi, w_lo, pad = co.weights(arr, V, U)
        again = co.weights(arr)
        assert all(np.array_equal(a, b) for a, b in zip(again, (w_hi, w_lo, pad)))
        nrm = np.linalg.norm(U, axis=2)
        assert (w_hi >= nrm.max(axis=1)).all() and (w_lo <= nrm.min(axis=1)).all()
        assert (w_lo >= 0.).all() and (pad > 0.).all()
        assert (pad <= co.pad_constant(p, p) * eps * 8. * np.sqrt(p)).all()
        lam = rng.dirichlet(np.ones(p + 1), (V.shape[0], 200))             # [n, 200, p+1]
        X = lam @ V
        inside = np.linalg.norm(X @ K.T + c, axis=2)
        slack = 1e-6 if eps > 1e-10 else 1e-14      # the narrowed K and c against the exact ones
        assert (inside <= w_hi[:, None] + slack).all() and (inside >= w_lo[:, None] - slack).all()
        # a leaf that holds a zero of the map has no lower bound; one away from it has
        assert (w_lo > 0.).any()


def test_refusals_before_the_device():
    from explicit_hybrid_mpc_amd import compiled, invariance
    n = 6
    law = SimpleNamespace(_handle=1, _h=dict(n_leaf=n, n_test=0), p=2, n_u=1)
    indptr, indices = csr([[1], [2], [0], [], [5], [4]])
    level = np.full(n, -1, dtype=np.int32)
    core = invariance.CoreResult(indptr=indptr, indices=indices, level=level, core=level < 0,
                                 set_convex=True, _law=law)
    with pytest.raises(ValueError, match='return_edges=True'):
        invariance.CoreResult(indptr=None, indices=None, level=level, core=level < 0,
                              _law=law).cost()
    with pytest.raises(ValueError, match='not both'):
        core.cost(start=[0], X0=np.zeros((1, 2)))
    with pytest.raises(ValueError, match='closed'):
        invariance.CoreResult(indptr=indptr, indices=indices, level=level, core=level < 0,
                              _law=SimpleNamespace(_handle=None)).cost()
    with pytest.raises(ValueError, match='closed'):
        invariance.cost_relation(SimpleNamespace(_handle=None), indptr, indices, level, [0])
    for empty in (np.zeros(n, dtype=bool), np.zeros(0, dtype=np.int32)):
        with pytest.raises(ValueError, match='start set is empty'):
            core.cost(start=empty)
        with pytest.raises(ValueError, match='domain set is empty'):
            core.cost(domain=empty)
    none_core = invariance.CoreResult(indptr=indptr, indices=indices, level=np.zeros(n, np.int32),
                                      core=np.zeros(n, dtype=bool), set_convex=True, _law=law)
    with pytest.raises(ValueError, match='domain set is empty'):
        none_core.cost()                                    # no core leaf
    for bad in ([n], [-1], np.ones(n + 1, dtype=bool), [0.5]):
        with pytest.raises(ValueError, match='start'):
            core.cost(start=bad)
        with pytest.raises(ValueError, match='domain'):
            core.cost(domain=bad)
    with pytest.raises(ValueError, match='lie in the domain: row 4'):
        core.cost(domain=[0, 1, 2], start=[1, 4])
    for h in (0, -3):
        with pytest.raises(ValueError, match='horizon'):
            core.cost(horizon=h)
    w = np.ones(n)
    with pytest.raises(ValueError, match='both w_hi and w_lo'):
        core.cost(w_hi=w)
    with pytest.raises(ValueError, match='both w_hi and w_lo'):
        core.cost(w_lo=w)
    with pytest.raises(ValueError, match='one entry per leaf'):
        core.cost(w_hi=w[:-1], w_lo=w[:-1])
    with pytest.raises(ValueError, match='finite'):
        core.cost(w_hi=np.where(np.arange(n) == 3, np.inf, 1.), w_lo=w)
    with pytest.raises(ValueError, match='w_lo <= w_hi'):
        core.cost(w_hi=w, w_lo=w + (np.arange(n) == 2))
    with pytest.raises(ValueError, match='2\\^28'):
        core.cost(horizon=(1 << 26) // n + 1, return_paths=True)
    with pytest.raises(ValueError, match='level'):
        invariance.cost_relation(law, indptr, indices, level[:-1], [0])
    with pytest.raises(ValueError, match='the law has'):
        invariance.cost_relation(law, np.arange(n + 2), np.zeros(n + 1, np.int32),
                                 np.zeros(n + 1, np.int32), [0])
    with pytest.raises(ValueError, match='at most 4 inputs'):
        invariance.cost_relation(SimpleNamespace(_handle=1, _h=law._h, p=2, n_u=5), indptr,
                                 indices, level, [0, 1, 2])
    # through a reach result
    reach = invariance.ReachResult(safe=True, limit=mask_of(n, [0, 1, 2]), closure=level < 0)
    with pytest.raises(ValueError, match='which'):
        reach.cost(core, which='tube')
    with pytest.raises(ValueError, match='lie in the domain: row 4'):
        reach.cost(core, start=[4])
    with pytest.raises(ValueError, match='leaks'):
        invariance.ReachResult(safe=False, limit=None, closure=level < 0).cost(core)
    with pytest.raises(ValueError, match='no limit set'):
        invariance.ReachResult(safe=True, limit=None, closure=level < 0).cost(core)
    assert callable(compiled.CompiledLaw.cost)
    with pytest.raises(ValueError, match='another law'):
        compiled.CompiledLaw.cost(SimpleNamespace(), core)


def test_host_checks_under_the_sanitizers(tmp_path):
    """What csrc/ehm_cost_host.h checks of the options, the domain, the start set and the weights,
    the keys of the per-step reductions and the walk of the args, driven by a stand-alone program
    built with the address and undefined-behaviour sanitizers."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'cost_host_main')
    src = os.path.join(ROOT, 'tests', 'native', 'cost_host_main.cpp')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror', src, '-o', exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'cost host helpers: ok' in out.stdout
