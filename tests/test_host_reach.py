"""
The reach tube and the limit set of a compiled law's closed loop (invariance.py)
without a device: the numpy mirror (tests/reach_cpu.py) on hand-made graphs and on the exact cube and
two-mode cases of tests/test_host_core.py, the properties every result has, the refusals ``reach``
makes before it uses the device, and the entry point's host checks (csrc/ehm_reach_host.h) under the
sanitizers.
"""

import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tests import compiled_cpu as cc
from tests import core_cpu as kc
from tests import invariance_cpu as iv
from tests import reach_cpu as rh
from tests import reduce_cpu as rc
from tests.test_host_core import largest_coordinate, two_mode_case
from tests.test_host_invariance import cube_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def csr(rows):
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    indices = np.array([t for r in rows for t in r], dtype=np.int32)
    return indptr, indices


def mask_of(n, rows):
    m = np.zeros(n, dtype=bool)
    m[list(rows)] = True
    return m


def check_properties(out, indptr, indices, level, start):
    """What holds of every result, whatever computed it (``out.D``: the sets D_j, where made)."""
    core = level < 0
    assert np.array_equal(out.closure, out.arrival >= 0)
    assert (out.arrival[start] == 0).all() and out.n_arrival == out.arrival.max()
    assert (out.leak_step == -1) == bool(core[start].all())
    leaky = level[start][level[start] >= 0]
    if leaky.size:
        assert out.leak_step == leaky.min()
    assert out.safe == (out.leak_step == -1)
    if out.safe and out.converged:
        assert not (out.closure & ~core).any()                  # closed and free of seeds
        assert np.array_equal(rh.post(out.limit, indptr, indices, level), out.limit)
        assert not (out.limit & ~out.closure).any()
        assert out.settle == max(int(out.depart.max()), 0)
        assert np.array_equal(out.depart < 0, out.limit | ~out.closure)
        for a, b in zip(out.D[:-1], out.D[1:]):
            assert not (b & ~a).any()
        assert len(out.D) == out.settle + 1 and np.array_equal(out.D[-1], out.limit)
        for j, d in enumerate(out.D):
            assert np.array_equal(d, out.closure & ((out.depart < 0) | (out.depart > j)))
    else:
        assert out.limit is None
    # the step sets, and the tube as their running union
    seen = np.zeros(level.size, dtype=bool)
    for k, r in enumerate(out.steps.astype(bool)):
        seen |= r
        assert np.array_equal(seen, (out.arrival >= 0) & (out.arrival <= k))
        assert out.step_count[k] == r.sum()
    assert np.array_equal(out.tube_count,
                          np.cumsum(np.bincount(out.arrival[out.closure],
                                                minlength=out.n_arrival + 1)))


def test_a_tail_into_a_cycle():
    # 0 -> 1 -> 2 -> 3 -> 4 -> 5 -> 6 -> 4
    indptr, indices = csr([[1], [2], [3], [4], [5], [6], [4]])
    level = np.full(7, -1, dtype=np.int32)
    start = mask_of(7, [0])
    out = rh.reach(indptr, indices, level, start, horizon=12)
    check_properties(out, indptr, indices, level, start)
    assert out.closure.all() and out.arrival.tolist() == list(range(7)) and out.n_arrival == 6
    assert out.limit.tolist() == [False] * 4 + [True] * 3
    assert out.depart.tolist() == [1, 2, 3, 4, -1, -1, -1] and out.settle == 4
    assert out.settle_count.tolist() == [7, 6, 5, 4, 3]
    # R_k is one leaf: it walks the tail, then the cycle with period 3 -- it never converges
    assert out.steps.shape == (13, 7) and (out.steps.sum(axis=1) == 1).all()
    where = out.steps.argmax(axis=1)
    assert where.tolist() == [0, 1, 2, 3, 4, 5, 6, 4, 5, 6, 4, 5, 6]
    assert np.array_equal(out.steps[4:10], out.steps[7:13])
    assert np.isnan(out.tube_box).all() and out.tube_box.shape == (7, 2, 1)


def test_a_seed_at_distance_two_and_rows_of_seeds():
    rows = [[1], [2, 0], [], [3]]
    level = np.array([2, 1, 0, -1], dtype=np.int32)
    start = mask_of(4, [0])
    indptr, indices = csr(rows)
    out = rh.reach(indptr, indices, level, start, horizon=5)
    check_properties(out, indptr, indices, level, start)
    assert out.leak_step == 2 and not out.safe and out.limit is None and out.settle is None
    assert out.steps.shape == (3, 4) and out.step_count.tolist() == [1, 1, 2]
    assert out.arrival.tolist() == [0, 1, 2, -1] and out.converged
    # arbitrary rows for the seed: nothing changes, 3 stays out of reach
    rows[2] = [3, 3, 0, 1]
    again = rh.reach(*csr(rows), level, start, horizon=5)
    for k in ('arrival', 'depart', 'steps', 'step_count', 'tube_count'):
        assert np.array_equal(getattr(out, k), getattr(again, k)), k
    assert again.leak_step == 2 and again.limit is None


def test_a_self_loop_an_unreachable_part_and_an_empty_limit():
    # 0 -> 0; 1 -> 2 -> 1 is never reached; 3 -> 4, and 4 has no row and is no seed
    indptr, indices = csr([[0], [2], [1], [4], []])
    level = np.full(5, -1, dtype=np.int32)
    out = rh.reach(indptr, indices, level, mask_of(5, [0]), horizon=3)
    check_properties(out, indptr, indices, level, mask_of(5, [0]))
    assert out.closure.tolist() == [True, False, False, False, False]
    assert out.limit.tolist() == out.closure.tolist() and out.settle == 0 and out.n_arrival == 0
    assert out.arrival[1:].tolist() == [-1] * 4 and (out.depart == -1).all()
    assert (out.steps == out.steps[0]).all()
    # from 3 the loop runs out of rows: the limit set is empty after two steps
    out = rh.reach(indptr, indices, level, mask_of(5, [3]), horizon=3)
    check_properties(out, indptr, indices, level, mask_of(5, [3]))
    assert out.closure.tolist() == [False, False, False, True, True] and out.converged
    assert not out.limit.any() and out.settle == 2 and out.depart.tolist() == [-1, -1, -1, 1, 2]
    assert out.settle_count.tolist() == [2, 1, 0] and out.step_count.tolist() == [1, 1, 0, 0]


def test_max_sweeps_cuts_each_phase():
    indptr, indices = csr([[1], [2], [3], [4], [5], [6], [4]])
    level = np.full(7, -1, dtype=np.int32)
    start = mask_of(7, [0])
    full = rh.reach(indptr, indices, level, start)
    for m in (1, full.n_arrival - 1, full.n_arrival):
        cut = rh.reach(indptr, indices, level, start, max_sweeps=m, horizon=9)
        assert not cut.converged and cut.limit is None and cut.limit_outer is None
        assert np.array_equal(cut.arrival, np.where(full.arrival <= m, full.arrival, -1))
        assert cut.n_arrival == m and cut.steps.shape[0] == m + 1
    # five leaves in a chain: 5 sweeps are enough for either phase
    indptr, indices = csr([[1], [2], [3], [4], [4]])
    level = np.full(5, -1, dtype=np.int32)
    start = mask_of(5, [0])
    full = rh.reach(indptr, indices, level, start)
    assert full.n_arrival == 4 and full.settle == 4 and full.converged
    cut = rh.reach(indptr, indices, level, start, max_sweeps=5)
    assert cut.converged and cut.settle == 4
    # enough for phase A (4 sweeps that reach a leaf and one that does not), short of phase B (8)
    indptr, indices = csr([[1], [2], [3], [4], [5], [6], [7], [7]] + [[]] * 4)
    level = np.full(12, -1, dtype=np.int32)
    start = mask_of(12, [0, 3])
    full = rh.reach(indptr, indices, level, start)
    assert full.n_arrival == 4 and full.settle == 7
    cut = rh.reach(indptr, indices, level, start, max_sweeps=5)
    assert not cut.converged and cut.limit is None and cut.settle == 5
    assert np.array_equal(cut.limit_outer, full.D[5]) and not (full.limit & ~cut.limit_outer).any()
    assert np.array_equal(cut.arrival, full.arrival)


def _cube_relation(name, p, rows='all'):
    for case in cube_cases(p):
        if case[0] == name:
            _, K, E, d_box, _, _ = case
            flat = iv.cube_law(p, K)
            arrays, _ = cc.compile_flat(flat)
            plant = iv.identity_plant(p, E=E)
            core = kc.core(arrays, None, plant, d_box=d_box, tol_exit=0., tol_side=0., rows=rows)
            return arrays, core, flat.vertices[arrays['leaf_node']]
    raise KeyError(name)


def _two_mode_relation(p, rows='all'):
    flat, plant = two_mode_case(p)
    arrays, _ = cc.compile_flat(flat)
    modes = rc.leaf_modes(flat, arrays)
    core = kc.core(arrays, modes, plant, tol_exit=0., tol_side=0., rows=rows)
    return arrays, core, flat.vertices[arrays['leaf_node']]


# (case, p, start: None = all core leaves, 'all', 'far' = the leaf at argmax M) -> what the
# prototype of the definitions gave (n leaves, closure, n_arrival, limit, settle; inner: the
# limit leaves have M <= that)
CUBE_TABLE = [
    ('contraction', 2, None, dict(n=168, closure=168, limit=28, settle=3, inner=0.5)),
    ('contraction', 2, 'far', dict(closure=24, n_arrival=4, limit=19, settle=2)),
    ('contraction', 3, None, dict(n=424, limit=260, settle=2)),
    ('contraction_quarter_box', 2, None, dict(limit=152, settle=2)),
    ('contraction_quarter_box', 3, None, dict(limit=423, settle=1)),
    ('two_mode', 2, None, dict(closure=42, limit=28, settle=2)),
    ('two_mode', 3, None, dict(closure=56, limit=52, settle=1)),
    ('expansion', 2, 'all', dict(leak_step=0)),
    ('expansion', 3, 'all', dict(leak_step=0)),
    ('contraction_box', 2, 'all', dict(leak_step=0)),
    ('contraction_box', 3, 'all', dict(leak_step=0)),
]


def cube_start(core, V, start):
    if start is None:
        return core.core.copy()
    if start == 'all':
        return np.ones(core.level.size, dtype=bool)
    return mask_of(core.level.size, [int(np.argmax(largest_coordinate(V)))])


def check_cube_numbers(out, name, V, core, want):
    if 'n' in want:
        assert out.arrival.size == want['n']
    if 'closure' in want:
        assert out.closure.sum() == want['closure']
    if 'n_arrival' in want:
        assert out.n_arrival == want['n_arrival']
    if 'leak_step' in want:
        assert out.leak_step == want['leak_step'] and out.limit is None
    if 'limit' in want:
        assert out.safe and out.limit.sum() == want['limit'] and out.settle == want['settle']
        assert out.settle_count[-1] == want['limit']
    if name == 'two_mode':
        assert np.array_equal(out.closure, core.core)
    if 'inner' in want:
        assert (largest_coordinate(V)[out.limit] <= want['inner']).all()


@pytest.mark.parametrize('name,p,start,want', CUBE_TABLE)
def test_the_cube_and_two_mode_numbers(name, p, start, want):
    make = (lambda rows: _two_mode_relation(p, rows)) if name == 'two_mode' else \
        (lambda rows: _cube_relation(name, p, rows))
    arrays, core, V = make('all')
    S = cube_start(core, V, start)
    out = rh.reach(core.indptr, core.indices, core.level, S, V=V, horizon=6)
    check_properties(out, core.indptr, core.indices, core.level, S)
    check_cube_numbers(out, name, V, core, want)
    # the boxes are those of the cells
    boxes = rh.leaf_boxes(V)
    assert np.array_equal(out.tube_box[-1], rh.set_box(out.closure, boxes))
    assert np.array_equal(out.tube_box[0], np.stack([V[S].min(axis=(0, 1)), V[S].max(axis=(0, 1))]))
    if out.limit is not None:
        assert np.array_equal(out.limit_box, rh.set_box(out.limit, boxes))
        assert np.array_equal(out.settle_box[0], out.tube_box[-1])
    if name in ('contraction', 'contraction_quarter_box'):
        origin = np.searchsorted(arrays['leaf_node'], cc.evaluate(arrays, np.zeros((1, p)))[1])[0]
        assert out.limit[origin]
    # the rows of seeds change nothing
    _, inv, _ = make('invariant')
    assert np.array_equal(inv.level, core.level)
    again = rh.reach(inv.indptr, inv.indices, inv.level, S, V=V, horizon=6)
    for k in ('arrival', 'depart', 'steps', 'tube_box', 'tube_count', 'step_box', 'step_count'):
        assert np.array_equal(getattr(out, k), getattr(again, k), equal_nan=k.endswith('box')), k
    assert (out.limit is None) == (again.limit is None)
    if out.limit is not None:
        assert np.array_equal(out.limit, again.limit) and out.settle == again.settle
        assert np.array_equal(out.settle_box, again.settle_box, equal_nan=True)


def test_refusals_before_the_device():
    from explicit_hybrid_mpc_amd import invariance
    n = 6
    law = SimpleNamespace(_handle=1, _h=dict(n_leaf=n, n_test=0), p=2, n_u=1)
    indptr, indices = csr([[1], [2], [0], [], [5], [4]])
    level = np.full(n, -1, dtype=np.int32)
    core = invariance.CoreResult(indptr=indptr, indices=indices, level=level, core=level < 0,
                                 set_convex=True, _law=law)
    with pytest.raises(ValueError, match='return_edges=True'):
        invariance.CoreResult(indptr=None, indices=None, level=level, core=level < 0,
                              _law=law).reach()
    with pytest.raises(ValueError, match='not both'):
        core.reach(start=[0], X0=np.zeros((1, 2)))
    with pytest.raises(ValueError, match='closed'):
        invariance.CoreResult(indptr=indptr, indices=indices, level=level, core=level < 0,
                              _law=SimpleNamespace(_handle=None)).reach()
    with pytest.raises(ValueError, match='closed'):
        invariance.reach_relation(SimpleNamespace(_handle=None), indptr, indices, level, [0])
    for empty in (np.zeros(n, dtype=bool), np.zeros(0, dtype=np.int32)):
        with pytest.raises(ValueError, match='empty'):
            core.reach(start=empty)
    none_core = invariance.CoreResult(indptr=indptr, indices=indices, level=np.zeros(n, np.int32),
                                      core=np.zeros(n, dtype=bool), set_convex=True, _law=law)
    with pytest.raises(ValueError, match='empty'):
        none_core.reach()                                   # no core leaf to start from
    for bad in ([n], [-1], np.ones(n + 1, dtype=bool), [0.5], np.zeros((2, 2), dtype=int)):
        with pytest.raises(ValueError, match='start'):
            core.reach(start=bad)
    with pytest.raises(ValueError, match='horizon'):
        core.reach(start=[0], horizon=-1)
    with pytest.raises(ValueError, match='max_sweeps'):
        core.reach(start=[0], max_sweeps=0)
    with pytest.raises(ValueError, match='2\\^28'):
        core.reach(start=[0], horizon=(1 << 28) // n, return_steps=True)
    with pytest.raises(ValueError, match='row_map'):
        core.reach(start=[0], row_map='block')
    with pytest.raises(ValueError, match='level'):
        invariance.reach_relation(law, indptr, indices, level[:-1], [0])
    with pytest.raises(ValueError, match='the law has'):
        invariance.reach_relation(law, np.arange(n + 2), np.zeros(n + 1, np.int32),
                                  np.zeros(n + 1, np.int32), [0])
    from explicit_hybrid_mpc_amd import compiled
    assert callable(compiled.CompiledLaw.reach)
    with pytest.raises(ValueError, match='another law'):
        compiled.CompiledLaw.reach(SimpleNamespace(), core)


def test_host_checks_under_the_sanitizers(tmp_path):
    """What csrc/ehm_reach_host.h checks of a relation, a start set and the options, the narrowing
    of indptr and what it reads off the per-step counters, driven by a stand-alone program built
    with the address and undefined-behaviour sanitizers."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'reach_host_main')
    src = os.path.join(ROOT, 'tests', 'native', 'reach_host_main.cpp')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror', src, '-o', exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'reach host helpers: ok' in out.stdout
