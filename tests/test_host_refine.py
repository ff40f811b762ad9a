"""
The refinement of a compiled law on the host (tests/refine_cpu.py, the numpy mirror of
csrc/ehm_refine.hip): the mirror against the definition -- every accepted plane is
+1, -1 and 0 at the right vertices, the children's cells are the partitioner's recursive bisection
--, the index rules, the import check on what it writes, the refusals made in Python, and the
device code's host-side rules under the sanitizers and against the mirror bit for bit.  No GPU.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled
from explicit_hybrid_mpc_amd.engine import FlatTree
from oracle.geometry import split_along_longest_edge
from tests import certify_cpu as zc
from tests import compiled_cpu as cc
from tests import reduce_cpu as rc
from tests import refine_cpu as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (2, 1), (3, 2), (7, 2), (8, 1)]


def small_law(p, n_u, single, kind='affine', seed=0, n_split=50):
    """(arrays, leaf_mode, kink frame) of a Kuhn tree of 4 roots and at most 60 leaves."""
    rng = np.random.default_rng([17, p, n_u, seed])
    K, c = rc.integer_gain(p, n_u, rng)
    frame = rc.kink_frame(p, 4, K)
    inputs = rc.affine_inputs(K, c) if kind == 'affine' else rc.clipped_inputs(K, *frame)
    modes = lambda X: (X @ K[0] > np.median(X @ K[0])).astype(np.int32)
    flat = rc.kuhn_tree(p, 4, n_split, rng, inputs, n_u, modes)
    arrays, _ = cc.compile_flat(flat)
    mode = rc.leaf_modes(flat, arrays)
    return (zc.narrow_flushed(arrays) if single else arrays), mode, (K,) + frame


def shifted_chain(p, depth, shift, scale):
    """``certify_cpu.chain_tree`` on a root that is not dyadic: the planes of its slivers are not
    exact in a float."""
    root = np.concatenate([np.zeros((1, p)), np.eye(p)]) * scale + np.asarray(shift)[:p]
    V, left, right = [root], [-1], [-1]
    k = 0
    for _ in range(depth):
        S1, S2 = V[k].copy(), V[k].copy()
        S1[0] = S2[1] = (V[k][0] + V[k][1]) / 2.
        left[k], right[k] = len(V), len(V) + 1
        V += [S1, S2]
        left += [-1, -1]
        right += [-1, -1]
        k = right[k]
    n = len(V)
    V = np.array(V)
    return FlatTree(V, np.array(left, np.int32), np.array(right, np.int32), np.zeros(n, np.int32),
                    np.zeros((n, p + 1)), V.sum(axis=2, keepdims=True) + 1., np.zeros(n, np.uint8),
                    np.zeros(n), {'n_roots': 1}, [0])


def recursive_split(V, levels):
    """The cells of ``levels`` bisections of V [p+1, p] by the pinned split_along_longest_edge, in
    the order the refined law numbers them: the left child keeps the slot, the right children of
    a pass are appended in leaf order."""
    cells = [V]
    for _ in range(levels):
        pairs = [split_along_longest_edge(c)[:2] for c in cells]
        cells = [s1 for s1, _ in pairs] + [s2 for _, s2 in pairs]
    return cells


@pytest.mark.parametrize('single', [False, True], ids=['double', 'single'])
@pytest.mark.parametrize('p,n_u', SHAPES)
def test_mirror_is_the_definition(p, n_u, single):
    arrays, mode, _ = small_law(p, n_u, single)
    h = zc.header(arrays)
    n_leaf, n_int = h['n_leaf'], h['n_int']
    assert n_leaf <= 300
    V0, st0 = zc.cells(arrays)
    assert (st0 == zc.CELL).all()
    levels = 2
    out = fc.refine(arrays, levels=levels, leaf_mode=mode)
    new = out.arrays
    compiled.validate_arrays(new)
    hn = zc.header(new)
    assert hn['n_leaf'] == 4 * n_leaf and hn['n_int'] == n_int + 3 * n_leaf
    assert out.passes == levels and out.n_split == 3 * n_leaf
    assert out.stops['satisfied'] == 4 * n_leaf and (out.stop == fc.SATISFIED).all()
    assert new['node'].dtype == arrays['node'].dtype and new['leaf_rec'].dtype == arrays['leaf_rec'].dtype
    # every accepted plane is +1, -1, 0 at the right vertices to the reported residual
    worst = 0.
    for ids, (i, j), planes, par in out.trace:
        assert (np.diff(ids) > 0).all()
    cur = arrays
    for ids, (i, j), planes, par in out.trace:
        V, st = zc.cells(cur, ids)
        s = fc.plane_at_vertices(planes, V)
        target = np.zeros(s.shape)
        target[np.arange(ids.size), j], target[np.arange(ids.size), i] = 1., -1.
        assert (i < j).all()
        worst = max(worst, float(np.abs(s - target).max()))
        cur = fc.refine(cur, levels=1, leaves=ids).arrays
    assert worst == out.max_plane_residual
    assert out.max_plane_residual <= (1e-5 if single else 1e-12)
    for k in new:
        assert new[k].tobytes() == cur[k].tobytes(), k          # pass by pass is the same law
    # the children's cells are the recursive split of the parent's cell
    V1, st1 = zc.cells(new)
    assert (st1 == zc.CELL).all()
    for l in range(n_leaf):
        kids = np.nonzero(out.origin == l)[0]
        assert kids[0] == l and kids.size == 2 ** levels
        want = recursive_split(V0[l], levels)
        assert np.array_equal(V1[kids], np.array(want)), l
    # records of the children: the parent's, byte for byte
    assert new['leaf_rec'].tobytes() == arrays['leaf_rec'][out.origin].tobytes()
    assert np.array_equal(new['leaf_node'], arrays['leaf_node'][out.origin])
    assert np.array_equal(out.leaf_mode, mode[out.origin])
    # the index rules: old records keep their index and their plane, children come after parents
    assert new['node'][:n_int, :p + 1].tobytes() == arrays['node'][:, :p + 1].tobytes()
    ch = zc.children(new)
    assert (ch[ch >= 0] > np.repeat(np.arange(ch.shape[0]), 2)[(ch >= 0).ravel()]).all()
    assert rc.is_forest(new, zc.parents(new))
    for k in ('root_rec', 'nbr', 'test_rec'):
        assert new[k].tobytes() == arrays[k].tobytes()


@pytest.mark.parametrize('single', [False, True], ids=['double', 'single'])
def test_index_rules_of_one_pass(single):
    arrays, _, _ = small_law(3, 2, single)
    h = zc.header(arrays)
    n_leaf, n_int, p = h['n_leaf'], h['n_int'], h['p']
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(n_leaf, n_leaf // 3, replace=False))
    entry_leaf = [~int(e) for e in arrays['root_entry'] if e < 0]
    out = fc.refine(arrays, levels=1, leaves=ids)
    new = out.arrays
    compiled.validate_arrays(new)
    assert np.array_equal(out.stop[:n_leaf], np.where(np.isin(np.arange(n_leaf), ids),
                                                      fc.SATISFIED, fc.UNSELECTED))
    # the left child keeps the slot, the appended ones follow in leaf order
    assert np.array_equal(out.origin[:n_leaf], np.arange(n_leaf))
    assert np.array_equal(out.origin[n_leaf:], ids)
    ch0, ch1 = zc.children(arrays), zc.children(new)
    assert np.array_equal(ch1[n_int:, 0], ~ids) and np.array_equal(
        ch1[n_int:, 1], ~(n_leaf + np.arange(ids.size)))
    # exactly one reference per split leaf is re-pointed, nothing else moves
    moved = np.argwhere(ch1[:n_int] != ch0)
    moved_roots = np.nonzero(new['root_entry'] != arrays['root_entry'])[0]
    assert moved.shape[0] + moved_roots.size == ids.size
    for k, side in moved:
        l = ~int(ch0[k, side])
        assert l in ids and ch1[k, side] == n_int + np.searchsorted(ids, l)
    for r in moved_roots:
        l = ~int(arrays['root_entry'][r])
        assert l in ids and l in entry_leaf
        assert new['root_entry'][r] == n_int + np.searchsorted(ids, l)
    # untouched leaves keep their cells bit for bit
    V0, _ = zc.cells(arrays)
    V1, _ = zc.cells(new)
    rest = np.setdiff1d(np.arange(n_leaf), ids)
    assert V1[rest].tobytes() == V0[rest].tobytes()
    # a one-leaf law: the root entry becomes the plane
    one, _ = cc.compile_flat(rc.kuhn_tree(p, 1, 0, rng, rc.affine_inputs(*rc.integer_gain(p, 2, rng)),
                                          2))
    one = zc.narrow_flushed(one) if single else one
    assert zc.header(one)['n_int'] == 0 and one['root_entry'][0] == -1
    two = fc.refine(one, levels=1)
    compiled.validate_arrays(two.arrays)
    assert zc.header(two.arrays)['n_int'] == 1 and two.arrays['root_entry'][0] == 0
    assert zc.children(two.arrays).tolist() == [[-1, -2]]
    # levels = 0: an equal copy
    same = fc.refine(arrays, levels=0)
    assert same.passes == 0 and (same.stop == fc.SATISFIED).all()
    for k in arrays:
        assert same.arrays[k].tobytes() == arrays[k].tobytes(), k


def test_geometry_against_the_golden_fixtures():
    """The mirror's longest edge and bisection on the reference's recorded splits (random cells and
    the tie cells, where the FIRST longest edge decides), and the plane of each of those cells."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'geometry_golden.npz'))
    sets = sorted(k[:-2] for k in z.files if k.endswith('_R') and k[:-2] + '_ij' in z.files)
    assert len(sets) >= 6
    for name in sets:
        R, ij = z[name + '_R'], z[name + '_ij']
        i, j, _ = fc.longest_edge(R)
        assert np.array_equal(i, ij[:, 0]) and np.array_equal(j, ij[:, 1]), name
        S1, S2 = fc.split_cells(R)
        assert S1.tobytes() == z[name + '_S1'].tobytes() and S2.tobytes() == z[name + '_S2'].tobytes()
        a, b = fc.solve_plane(R, i, j)
        rec, storable = fc.store_plane(a, b, False)
        ok, res = fc.accept_plane(rec, R, i, j)
        good = np.linalg.cond(R[:, 1:] - R[:, :1]) < 1e6        # residual ~ cond * 2^-53
        assert good.sum() >= 0.5 * good.size, name
        assert (ok & storable)[good].all() and res[good].max() < 1e-6, name
        # the plane is zero on the shared face: both children see the midpoint on it
        mid = S1[np.arange(R.shape[0]), i]
        s = fc.plane_at_vertices(rec, mid[:, None, :])[:, 0]
        assert np.abs(s[good]).max() < 1e-6


def test_criteria_and_stop_codes():
    # max_diameter: satisfied leaves are at or below the bound, `levels` leaves above it
    arrays, _, _ = small_law(2, 1, False)
    V0, _ = zc.cells(arrays)
    d0 = fc.longest_edge(V0)[2]
    bound = float(np.median(d0)) / 2.
    out = fc.refine(arrays, levels=2, max_diameter=bound)
    V1, _ = zc.cells(out.arrays)
    d1 = fc.longest_edge(V1)[2]
    assert set(np.unique(out.stop)) == {fc.SATISFIED, fc.LEVELS}
    assert (d1[out.stop == fc.SATISFIED] <= bound).all() and (d1[out.stop == fc.LEVELS] > bound).all()
    assert np.bincount(out.origin)[d0 <= bound].max() == 1          # never split below the bound
    # max_spread on a clipped law: leaves away from the kink are flat beyond the first criterion
    arrays, _, (K, centre, width) = small_law(2, 1, False, kind='clip')
    V0, _ = zc.cells(arrays)
    U0 = zc.vertex_inputs(arrays, np.arange(V0.shape[0]), V0, np.zeros(V0.shape[0], np.int32))
    spread0 = (U0.max(axis=1) - U0.min(axis=1)).max(axis=1)
    out = fc.refine(arrays, levels=3, max_spread=0.)
    assert (np.bincount(out.origin)[spread0 == 0.] == 1).all() and (spread0 == 0.).any()
    assert (np.bincount(out.origin)[spread0 > 0.] > 1).all()
    # per-leaf levels with 0, and a NaN input never splits
    lv = np.arange(V0.shape[0]) % 3
    out = fc.refine(arrays, levels=lv)
    assert np.array_equal(np.bincount(out.origin), 2 ** lv)
    # an input that overflows exceeds every bound, a NaN input never splits
    big = {k: np.array(v, copy=True) for k, v in arrays.items()}
    l = int(np.argmin(spread0))
    rc.make_leaf_overflow(big, l, V0[l])
    out = fc.refine(big, levels=1, leaves=[l], max_spread=1e300)
    assert (out.origin == l).sum() == 2
    nan = fc.nan_law()
    Un = zc.vertex_inputs(nan, np.zeros(1, np.int64), *zc.cells(nan))[0, :, 0]
    assert Un[0] == 0. and np.isposinf(Un[1]) and np.isnan(Un[2])
    out = fc.refine(nan, levels=3, max_spread=0.)
    assert out.passes == 0 and out.stop.tolist() == [fc.SATISFIED]
    out = fc.refine(nan, levels=1, max_spread=0., max_diameter=1.)
    assert out.stop.tolist() == [fc.LEVELS] * 2
    # a broken plane: the leaves below it have no cell and are kept
    below = rc.leaves_below(arrays)
    bad = next(k for k in range(len(below)) if 2 <= len(below[k]) <= 8)
    broken = {k: np.array(v, copy=True) for k, v in arrays.items()}
    broken['node'][bad, :3] *= 0.25
    out = fc.refine(broken, levels=1)
    assert (out.stop[below[bad]] == fc.NO_CELL).all() and out.stops['no_cell'] == len(below[bad])
    assert np.bincount(out.origin)[below[bad]].max() == 1
    compiled.validate_arrays(out.arrays)
    # a chain of 300 levels: too_deep at depth 256, no_cell below, the shallower leaves split
    deep, _ = cc.compile_flat(zc.chain_tree(2, 300))
    out = fc.refine(deep, levels=1)
    depth = np.minimum(np.arange(301) + 1, 300)
    assert np.array_equal(np.nonzero(out.stop[:301] == fc.TOO_DEEP)[0], np.nonzero(depth == 256)[0])
    assert (out.stop[:301][depth > 256] == fc.NO_CELL).all()
    assert np.array_equal(np.bincount(out.origin), np.where(depth < 256, 2, 1))
    compiled.validate_arrays(out.arrays)
    assert (zc.cells(out.arrays)[1] == zc.CELL).sum() == 2 * 255 + 1
    # a sliver chain in single precision: where the float plane no longer separates the leaf stays
    flat = shifted_chain(2, 30, [1. / 3., 0.7], 0.9)
    double, _ = cc.compile_flat(flat)
    single = zc.narrow_flushed(double)
    out64, out32 = fc.refine(double, levels=1), fc.refine(single, levels=1)
    assert out64.stops['satisfied'] == 62 and out64.max_plane_residual < 1e-6
    assert out32.stops['unseparated'] >= 1
    kept = np.nonzero(out32.stop == fc.UNSEPARATED)[0]
    assert (np.bincount(out32.origin)[kept] == 1).all()
    compiled.validate_arrays(out32.arrays)
    st = zc.cells(out32.arrays)[1]
    assert (st[out32.stop == fc.SATISFIED] == zc.CELL).all()


def test_refusals_made_in_python():
    E = _capi.EhmError
    lv, sel = compiled.refine_selection(5, 2, None)
    assert lv.tolist() == [2] * 5 and sel.tolist() == [1] * 5 and lv.dtype == np.int32
    lv, sel = compiled.refine_selection(5, [0, 1, 2, 3, 16], [4, 0])
    assert lv.tolist() == [0, 1, 2, 3, 16] and sel.tolist() == [1, 0, 0, 0, 1]
    assert compiled.refine_selection(3, 1, np.array([True, False, True]))[1].tolist() == [1, 0, 1]
    assert compiled.refine_selection(3, 1, np.zeros(0, dtype=np.int64))[1].tolist() == [0, 0, 0]
    for levels, leaves in ((-1, None), (17, None), ([1, 2], None), (1.5, None), ([0, 0, 17], None),
                           (1, [3]), (1, [-1]), (1, np.array([True, False])), (1, [0.5]),
                           (1, np.zeros((2, 2), dtype=np.int64))):
        with pytest.raises(E) as err:
            compiled.refine_selection(3, levels, leaves)
        assert err.value.code == _capi.EHM_E_INVALID
    d, s = compiled.refine_criteria(2, 0.5, None)
    assert d.tolist() == [0.5] and s is None
    d, s = compiled.refine_criteria(2, None, 0.25)
    assert d is None and s.tolist() == [0.25, 0.25]
    assert compiled.refine_criteria(2, None, [1., 0.])[1].tolist() == [1., 0.]
    for d, s in ((-1., None), (np.nan, None), (np.inf, None), (None, -1e-9), (None, [1., np.nan])):
        with pytest.raises(E) as err:
            compiled.refine_criteria(2, d, s)
        assert err.value.code == _capi.EHM_E_INVALID
    for d, s in (([1., 2.], None), (None, [1., 2., 3.])):
        with pytest.raises(ValueError):
            compiled.refine_criteria(2, d, s)
    assert fc.worst_case(np.array([0, 3, 16]), np.array([True, True, False])) == 1 + 8 + 1
    with pytest.raises(E):
        compiled.check_leaf_mode(np.zeros(4, np.int32), 5)
    # a closed law, before anything else is looked at
    closed = type('Closed', (), {'_handle': None})()
    with pytest.raises(E) as err:
        compiled.CompiledLaw.refine(closed, levels=-1)
    assert err.value.code == _capi.EHM_E_INVALID and 'closed' in str(err.value)


def _host_program(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'refine_host_main')
    src = os.path.join(ROOT, 'tests', 'native', 'refine_host_main.cpp')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror', src, '-o', exe],
                   check=True, capture_output=True, text=True)
    return exe


def test_host_rules_under_the_sanitizers(tmp_path):
    """The longest edge, the solve, the rounding, the acceptance test, the criteria, the worst case,
    the depth and the re-pointing of csrc/ehm_refine_host.h, driven by a stand-alone program built
    with the address and undefined-behaviour sanitizers; then the same program on the cells of the
    golden fixtures and of a sliver chain against the numpy mirror, bit for bit."""
    exe = _host_program(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'refine host helpers: ok' in out.stdout
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'geometry_golden.npz'))
    cases = {int(k.split('_p')[1][0]): z[k] for k in z.files if k.startswith('rand_p') and
             k.endswith('_R')}
    chain, _ = cc.compile_flat(shifted_chain(2, 30, [1. / 3., 0.7], 0.9))
    cases[2] = np.concatenate([cases[2], z['tie_p2_R'][:200], zc.cells(chain)[0]])
    rng = np.random.default_rng(3)
    for p in (1, 5, 7):
        cases[p] = rng.normal(size=(100, p + 1, p))
    for p, R in sorted(cases.items()):
        src, dst = str(tmp_path / ('cells%d.bin' % p)), str(tmp_path / ('planes%d.bin' % p))
        np.ascontiguousarray(R, dtype=np.float64).tofile(src)
        out = subprocess.run([exe, str(p), src, dst], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        got = np.fromfile(dst).reshape(R.shape[0], p + 8)
        i, j, length = fc.longest_edge(R)
        a, b = fc.solve_plane(R, i, j)
        want = [i.astype(np.float64), j.astype(np.float64), length] + list(a.T) + [b]
        for single in (False, True):
            rec, storable = fc.store_plane(a, b, single)
            ok, res = fc.accept_plane(rec, R, i, j)
            want += [(ok & storable).astype(np.float64), np.where(storable, res, 0.)]
        want = np.stack(want, axis=1)
        assert want.tobytes() == got.tobytes(), p
