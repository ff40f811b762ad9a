"""
The reduction of a compiled law on the host (tests/reduce_cpu.py, the numpy mirror of
csrc/ehm_reduce.hip): the mirror against the definition by brute force, the bound
it promises at every vertex of every original cell, and the device code's host-side bookkeeping
under the sanitizers.  No GPU.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import compiled_cpu as cc
from tests import reduce_cpu as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1), (3, 2), (7, 1), (7, 2)]


def small_law(p, n_u, kind, single, seed=0, n_split=60):
    """(arrays, leaf_mode, tol, (K, centre, width) of the kinks, FlatTree) of a tree of at most 200
    leaves with prescribed vertex inputs."""
    rng = np.random.default_rng([91, p, n_u, seed])
    K, c = rc.integer_gain(p, n_u, rng)
    modes = None
    frame = rc.kink_frame(p, 3, K)
    if kind == 'exact':
        inputs, tol = rc.affine_inputs(K, c), 0.
    elif kind == 'clip':
        inputs, tol = rc.clipped_inputs(K, *frame), 1e-9
    elif kind == 'curved':
        inputs, tol = rc.curved_inputs(p, n_u, 1e-3), None
    else:
        inputs, tol = rc.affine_inputs(K, c), 0.
        modes = lambda X: (X @ K[0] > np.median(X @ K[0])).astype(np.int32)
    flat = rc.kuhn_tree(p, 3, n_split, rng, inputs, n_u, modes)
    arrays, _ = cc.compile_flat(flat)
    mode = rc.leaf_modes(flat, arrays)
    if single:
        arrays = zc.narrow_flushed(arrays)
    if tol is None:
        # about 0.6 tol between the two children of the deepest splits
        V, st = zc.cells(arrays)
        U = zc.vertex_inputs(arrays, np.arange(st.size), V, st)
        ch = zc.children(arrays)
        both = ch[(ch < 0).all(axis=1)]
        d = np.abs(rc.map_at(arrays, ~both[:, 0], V[~both[:, 1]]) - U[~both[:, 1]])
        tol = float(np.median(d.max(axis=(1, 2)))) / 0.6
    return arrays, mode, tol, (K,) + frame, flat


def brute_force_mergeable(arrays, tol, mode, V, U, status):
    """Per internal record: every leaf below it passes the direct test against the leftmost one."""
    ch = zc.children(arrays)
    below = rc.leaves_below(arrays)
    out = np.zeros(ch.shape[0], dtype=bool)
    for a in range(ch.shape[0]):
        c = a
        while c >= 0:
            c = int(ch[c, 0])
        rep = ~c
        assert below[a][0] == rep
        ok = True
        for l in below[a]:
            if status[l] != zc.CELL or (mode is not None and mode[l] != mode[rep]):
                ok = False
                break
            ur = rc.map_at(arrays, [rep], V[l:l + 1])[0]
            with np.errstate(invalid='ignore'):
                if (~(np.abs(ur - U[l]) <= tol)).any():
                    ok = False
                    break
        out[a] = ok
    return out


@pytest.mark.parametrize('single', [False, True], ids=['double', 'single'])
@pytest.mark.parametrize('kind', ['exact', 'clip', 'curved', 'modes'])
@pytest.mark.parametrize('p,n_u', SHAPES)
def test_mirror_is_the_definition_and_keeps_its_bound(p, n_u, kind, single):
    arrays, mode, tol, K, flat = small_law(p, n_u, kind, single)
    h = zc.header(arrays)
    assert h['n_leaf'] <= 200
    use_mode = mode if kind == 'modes' else None
    out = rc.reduce(arrays, tol, use_mode)
    V, status, U = out.cells, out.cell_status, out.inputs
    want = brute_force_mergeable(arrays, tol, use_mode, V, U, status)
    assert np.array_equal(out.open == 0, want)
    # the new leaves are the topmost mergeable records on each root path
    ch = zc.children(arrays)
    kept_int, kept_leaf = [], []
    stack = [int(e) for e in arrays['root_entry']][::-1]
    while stack:
        c = stack.pop()
        if c < 0:
            kept_leaf.append(~c)
        elif want[c]:
            kept_leaf.append(int(out.rep[c]))
        else:
            kept_int.append(c)
            stack += [int(ch[c, 1]), int(ch[c, 0])]
    assert sorted(kept_int) == np.nonzero(out.keep_int)[0].tolist()
    assert sorted(kept_leaf) == np.nonzero(out.keep_leaf)[0].tolist()
    new = out.arrays
    cc_h = zc.header(new)
    assert cc_h['n_leaf'] == len(kept_leaf) and cc_h['n_int'] == len(kept_int)
    # a merged leaf is its representative's record
    assert np.array_equal(new['leaf_rec'], arrays['leaf_rec'][out.keep_leaf])
    assert np.array_equal(new['leaf_node'], arrays['leaf_node'][out.keep_leaf])
    assert new['leaf_rec'].dtype == arrays['leaf_rec'].dtype
    # the bound, in the rule's own arithmetic: at every vertex of every original cell
    live = status == zc.CELL
    Unew = rc.map_at(new, out.leaf_of[live], V[live])
    assert (np.abs(Unew - U[live]) <= tol).all()
    assert out.max_deviation <= (tol if np.ndim(tol) == 0 else max(tol))
    # the reduced law is a law: children after parents, the same cells for what was kept, the
    # merged cells tile what they replace
    par = zc.parents(new)
    assert rc.is_forest(new, par)
    nch = zc.children(new)
    assert (nch[nch >= 0] > np.repeat(np.arange(nch.shape[0]), 2)[(nch >= 0).ravel()]).all()
    V2, st2 = zc.cells(new)
    assert (st2 == zc.CELL).all()
    same = out.keep_leaf & (out.target == np.arange(h['n_leaf']))
    untouched = np.array([(out.target == l).sum() == 1 for l in np.nonzero(same)[0]])
    ids = np.nonzero(same)[0][untouched]
    assert np.array_equal(V2[out.leaf_of[ids]], V[ids])
    if kind == 'exact':
        assert cc_h['n_int'] == 0 and cc_h['n_leaf'] == h['n_roots']
        assert (new['root_entry'] < 0).all() and out.max_deviation == 0.
    if kind == 'clip':
        assert cc_h['n_leaf'] < h['n_leaf']
        # A leaf whose cell straddles a kink applies the interpolant of clipped values, which is
        # neither of the two affine pieces: it never shares a leaf with a cell that lies on one
        # side.  (Two straddling siblings split along an edge that lies on one side of the kink
        # apply the same interpolant exactly, their parent's, and do merge: the rule asks for it.)
        strad = rc.straddles_kink(*K, V)
        assert strad.any()
        assert strad[out.target[strad]].all()
        for t in np.unique(out.target[strad]):
            assert strad[out.target == t].all()
        alone = np.bincount(out.target, minlength=h['n_leaf'])[strad] == 1
        assert (out.keep_leaf[strad] & alone).sum() >= 0.5 * strad.sum()
    if kind == 'modes':
        assert 0 < cc_h['n_int'] and cc_h['n_leaf'] > h['n_roots']
        again = rc.reduce(arrays, tol, None)
        assert zc.header(again.arrays)['n_int'] == 0
        assert np.array_equal(out.leaf_mode, mode[out.keep_leaf])
        assert (mode[out.target] == mode).all()


def test_the_bound_does_not_accumulate():
    """Neighbouring leaves of a slowly curving input differ by about 0.6 tol: sibling pairs that
    pass on their own stay apart where a deeper leaf fails against the representative, and every
    original leaf is within tol of the leaf that stands for it."""
    arrays, _, tol, _, _ = small_law(2, 1, 'curved', False, n_split=90)
    out = rc.reduce(arrays, tol)
    h = zc.header(arrays)
    V, U, status = out.cells, out.inputs, out.cell_status
    assert 1 < zc.header(out.arrays)['n_leaf'] < h['n_leaf']
    Unew = rc.map_at(out.arrays, out.leaf_of, V)
    assert (np.abs(Unew - U) <= tol).all()
    # an open record whose two children are each mergeable (or leaves), one of them a subtree, and
    # whose right representative agrees with the left one on its own cell: the pair looks
    # mergeable neighbour to neighbour, and stays apart because a deeper leaf fails against the
    # record's representative
    ch = zc.children(arrays)
    looks = 0
    for a in np.nonzero(out.open)[0]:
        l, r = (int(c) for c in ch[a])
        sub = [c < 0 or not out.open[c] for c in (l, r)]
        if not all(sub):
            continue
        rl = ~l if l < 0 else int(out.rep[l])
        rr = ~r if r < 0 else int(out.rep[r])
        d = np.abs(rc.map_at(arrays, [rl], V[rr:rr + 1]) - U[rr])
        if (d <= tol).all() and (l >= 0 or r >= 0):
            looks += 1
    assert looks >= 1


def test_no_cell_nan_and_unreached_records_keep_their_ancestors():
    arrays, _, tol, _, _ = small_law(3, 1, 'exact', False)
    h = zc.header(arrays)
    p, n_u = h['p'], h['n_u']
    below = rc.leaves_below(arrays)
    full = rc.reduce(arrays, 0.)
    assert zc.header(full.arrays)['n_int'] == 0

    def ancestors(par, l):
        out, up = [], int(par[2][l])
        while up >= 0:
            out.append(up)
            up = int(par[0][up])
        return out

    # a plane that is no bisection: the leaves below it have no cell, exactly their ancestors stay
    bad = next(k for k in range(h['n_int']) if 3 <= len(below[k]) <= 12)
    broken = {k: np.array(v, copy=True) for k, v in arrays.items()}
    broken['node'][bad, :p + 1] *= 0.25
    out = rc.reduce(broken, 0.)
    want = set()
    for l in below[bad]:
        want |= set(ancestors(out.par, l))
    assert set(np.nonzero(out.open)[0].tolist()) == want
    assert (out.cell_status[below[bad]] == zc.NO_CELL).all()
    assert out.keep_leaf[below[bad]].all()
    # a leaf whose map overflows: the difference with itself is NaN, it never merges
    nan = {k: np.array(v, copy=True) for k, v in arrays.items()}
    l = below[bad][1]
    rc.make_leaf_overflow(nan, l, full.cells[l])
    out = rc.reduce(nan, 0.)
    assert not np.isfinite(out.inputs[l]).all()
    assert set(np.nonzero(out.open)[0].tolist()) == set(ancestors(out.par, l))
    assert out.keep_leaf[l] and (out.target == l).sum() == 1
    # a chain of 300 levels: the 45 leaves without a cell keep every record of the chain
    deep, _ = cc.compile_flat(zc.chain_tree(2, 300))
    out = rc.reduce(deep, 1e300)
    assert (out.cell_status == zc.NO_CELL).sum() == 45
    assert out.open.all() and out.keep_leaf.all() and out.keep_int.all()
    for k in ('header', 'node', 'leaf_rec', 'leaf_node', 'root_rec', 'root_entry'):
        assert out.arrays[k].tobytes() == deep[k].tobytes(), k
    assert np.array_equal(out.leaf_of, np.arange(301))


def test_host_rules_under_the_sanitizers(tmp_path):
    """The forest check, the representative walk, the topmost-ancestor rule, the survivors and the
    renumbering of csrc/ehm_reduce_host.h, driven by a stand-alone program built with the address
    and undefined-behaviour sanitizers."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'reduce_host_main')
    src = os.path.join(ROOT, 'tests', 'native', 'reduce_host_main.cpp')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror', src, '-o', exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'reduce host helpers: ok' in out.stdout
