"""
The host mirror of the sampled audit (tests/audit_cpu.py) checked against what it must be by
construction, on a hand-made two-leaf tree, and the status logic on hand-made rows -- the mirror is
what tests/test_gpu_audit.py holds the device to.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import applied_cpu as apc
from tests import audit_cpu as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the unit square cut along its diagonal: two leaves of volume 1/2
CELLS = np.array([[[0., 0.], [1., 0.], [1., 1.]],
                  [[0., 0.], [1., 1.], [0., 1.]]])
CDF = np.cumsum([0.5, 0.5])


def test_spacings_are_barycentric_weights():
    for p in (1, 2, 4, 8):
        w = ac.words(np.arange(5000), 3, p)
        assert w.shape == (5000, p + 1) and w.dtype == np.uint64
        U = ac.uniform01(w[:, 1:])
        assert (U >= 0.).all() and (U < 1.).all()
        W = ac.spacings(U)
        assert W.shape == (5000, p + 1)
        assert (W >= 0.).all()
        assert np.abs(W.sum(axis=1) - 1.).max() <= 2.0 ** -52
    # the extremes of a word: 0 and the largest uniform, 1 - 2^-53
    assert ac.uniform01(np.uint64(0)) == 0.
    assert ac.uniform01(np.uint64(2 ** 64 - 1)) == 1. - 2.0 ** -53
    W = ac.spacings(np.array([[0., 1. - 2.0 ** -53], [0., 0.]]))
    assert (W >= 0.).all() and (W.sum(axis=1) == 1.).all()


def test_words_follow_the_counter_layout():
    """Word k of sample s is word k % 4 of block (s, k // 4, 0, 0), key (seed, 1): a sample's words
    depend on its id alone, and the key differs from the noise model's (seed, 0)."""
    from explicit_hybrid_mpc_amd.noise import philox4x64_10
    ids = np.array([0, 1, 77, 2 ** 40 + 5], dtype=np.uint64)
    w = ac.words(ids, 9, 6)                 # words 0..6: blocks 0 and 1
    b0 = philox4x64_10(ids, 0, 0, 0, 9, 1)
    b1 = philox4x64_10(ids, 1, 0, 0, 9, 1)
    for k in range(7):
        assert np.array_equal(w[:, k], (b0 if k < 4 else b1)[k % 4])
    assert np.array_equal(ac.words(ids[2:3], 9, 6), w[2:3])
    assert not np.array_equal(b0[0], philox4x64_10(ids, 0, 0, 0, 9, 0)[0])


def test_points_lie_in_their_cells_and_per_leaf_deals_k_ids_each():
    ids = np.arange(4000)
    X, cell = ac.sample(CELLS, CDF, ids, 1, ac.UNIFORM)
    assert set(cell) == {0, 1}
    assert abs(np.mean(cell == 0) - 0.5) < 0.05
    lower = X[:, 1] <= X[:, 0]
    assert (lower[cell == 0]).all() and (~lower[cell == 1] | (X[cell == 1, 0] == X[cell == 1, 1])).all()
    assert (X >= 0.).all() and (X <= 1.).all()
    Xp, cp = ac.sample(CELLS, CDF, np.arange(14), 1, ac.PER_LEAF, k=7)
    assert np.array_equal(cp, np.repeat([0, 1], 7))
    assert np.array_equal(np.bincount(cp), [7, 7])
    # global ids: a range drawn alone equals its rows of the whole
    Xs, cs = ac.sample(CELLS, CDF, ids[1000:1096], 1, ac.UNIFORM)
    assert np.array_equal(Xs, X[1000:1096]) and np.array_equal(cs, cell[1000:1096])


def test_cdf_choice_stays_in_range():
    cdf = np.cumsum([0.25, 0., 0.5, 0.25])
    u = np.array([0., 0.25 - 2.0 ** -54, 0.25, 0.75, 1. - 2.0 ** -53])
    assert np.array_equal(ac.choose_uniform(u, cdf), [0, 0, 2, 3, 3])   # the empty cell 1: never
    # a running sum whose last entries round below u * total: clamped to the last cell
    assert ac.choose_uniform(np.array([1. - 2.0 ** -53]), np.array([1e-300, 1e-300]))[0] <= 1
    assert ac.choose_uniform(np.array([0.]), np.array([3.]))[0] == 0


def test_status_logic_and_its_boundaries():
    eps_a, eps_r, rtol = 0.5, 0.1, 2.0 ** -10
    vstar = np.array([1., 1., 1., 1., 1., 1., 1., 10., 10., np.inf, 1., 1.])
    slack = rtol * (1. + np.abs(vstar))
    bound = np.maximum(eps_a, eps_r * vstar)
    gap = np.array([0.25,                       # within
                    bound[1] + slack[1],        # == bound + slack: within
                    bound[2] + 2 * slack[2],    # violation
                    -slack[3],                  # == -slack: within
                    -2 * slack[4],              # negative
                    0.25,                       # open leaf
                    5.,                         # open wins over violation
                    0.9,                        # relative bound 1.0: within
                    1.5,                        # violation of the relative bound
                    0.,                         # infeasible
                    0.25,                       # infeasible wins over open
                    np.nan])                    # a cost that is no number is no pass
    vbar = vstar + gap
    vbar[1] = vstar[1] + (bound[1] + slack[1])
    closed = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1], dtype=bool)
    didx = np.array([0, 0, 3, 0, 0, 0, 0, 0, 0, -1, -1, 0])
    st, ratio = ac.statuses(vbar, vstar, closed, didx, eps_a, eps_r, rtol)
    assert st.tolist() == [0, 0, 1, 0, 2, 3, 3, 0, 1, 4, 4, 2]
    counts, hist, best, worst = ac.summary(np.arange(100, 112), st, ratio)
    assert counts.tolist() == [4, 2, 2, 2, 2]
    assert hist.sum() == counts[:3].sum() and hist.shape == (33,)
    assert hist[32] == 3                    # rows 1, 2 and 8 lie above 1
    assert hist[0] == 3                     # the two negative gaps and the NaN
    assert best == ratio[8] == 1.5 and worst == 108
    # ties go to the smaller id
    st2, r2 = np.zeros(3, dtype=np.int32), np.array([0.5, 0.75, 0.75])
    assert ac.summary(np.array([9, 8, 7]), st2, r2)[2:] == (0.75, 7)
    assert ac.summary(np.arange(2), np.array([3, 4], dtype=np.int32), np.zeros(2))[2:] == (-np.inf, -1)


def test_flatten_tree_costs_are_optional_and_leave_the_rest_alone():
    from explicit_hybrid_mpc_amd import explicit
    from explicit_hybrid_mpc_amd.tree import NodeData, Tree
    root = Tree(NodeData(vertices=np.array([[0., 0.], [1., 0.], [1., 1.], [0., 1.]])))
    a = NodeData(CELLS[0], commutation=np.array([1, 0]), vertex_costs=np.array([1., 2., 3.]),
                 vertex_inputs=np.zeros((3, 1)))
    a.is_epsilon_suboptimal = True
    b = NodeData(CELLS[1], commutation=np.array([1, 0]), vertex_costs=np.array([1., 3., 4.]),
                 vertex_inputs=np.ones((3, 1)))
    root.grow(a, b)
    plain = explicit.flatten_tree(root)
    assert len(plain) == 5
    with_c = explicit.flatten_tree(root, commutations=True)
    assert len(with_c) == 6
    full = explicit.flatten_tree(root, commutations=True, costs=True)
    assert len(full) == 7
    for x, y in zip(plain[:4], full[:4]):
        assert np.array_equal(x, y)
    extra = full[6]
    assert np.isnan(extra['vertex_costs'][0]).all()
    assert np.array_equal(extra['vertex_costs'][1:], [[1., 2., 3.], [1., 3., 4.]])
    assert extra['flags'].tolist() == [0, 1, 0] and extra['flags'].dtype == np.uint8
    assert extra['simplex'].tolist() == [False, True, True]
    order = explicit.forest_order(full[2], full[3], ~extra['simplex'])
    assert order.tolist() == [1, 2]


def test_forest_order_numbers_the_roots_first_then_breadth_first():
    from explicit_hybrid_mpc_amd import explicit
    # spine 0 -> (1, 2), 2 -> (3, 4): roots 1, 3, 4; root 1 splits into (5, 6), root 4 into (7, 8),
    # 5 into (9, 10)
    left = np.array([1, 5, 3, -1, 7, 9, -1, -1, -1, -1, -1])
    right = np.array([2, 6, 4, -1, 8, 10, -1, -1, -1, -1, -1])
    spine = np.zeros(11, dtype=bool)
    spine[[0, 2]] = True
    assert explicit.forest_order(left, right, spine).tolist() == [1, 3, 4, 5, 6, 7, 8, 9, 10]


def test_verdict_rules_under_the_sanitizers_match_the_mirrors(tmp_path):
    """csrc/ehm_verdict.h and csrc/ehm_err.h driven by a stand-alone program built with the address
    and undefined-behaviour sanitizers: its own checks (the ladder at its thresholds, the bins, the
    host merge, a message longer than the channel's buffer), and its ladder and bins on rows that
    the two numpy mirrors judge too -- the C++ rules pinned to tests/audit_cpu.py and
    tests/applied_cpu.py."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'verdict_host_main')
    src = os.path.join(ROOT, 'tests', 'native', 'verdict_host_main.cpp')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Wextra',
                    '-Werror', src, '-o', exe], check=True, capture_output=True, text=True)
    # the ladder: V* = 0 makes bound = eps_a and slack = rtol, so the gaps are the thresholds
    # themselves and their neighbours; then rows whose gap rounds
    eps_a, eps_r, rtol = 0.25, 0.5, 1e-7
    inf = np.inf
    gaps = [-rtol, np.nextafter(-rtol, 0.), np.nextafter(-rtol, -inf), eps_a + rtol,
            np.nextafter(eps_a + rtol, 0.), np.nextafter(eps_a + rtol, inf), 0., -0., np.nan, inf,
            -inf, eps_a]
    rows = [(g, 0., eps_a, eps_r, rtol) for g in gaps]
    rng = np.random.default_rng(7)
    vs = rng.uniform(0.1, 4., 64)
    rows += [(v + g, v, eps_a, eps_r, rtol) for v, g in zip(vs, rng.uniform(-0.5, 3., 64))]
    rows += [(1., 1., 0., 0., rtol), (2., 1., 0., 0., rtol)]      # 0 / 0 and 1 / 0 at eps = 0
    ratios = [-0., 0., 1. / 32., 31. / 32., np.nextafter(1., 0.), 1., np.nextafter(1., 2.), inf,
              -inf, np.nan, 0.5, np.nextafter(0.5, 0.)]
    text = ''.join('j ' + ' '.join(float(x).hex() for x in r) + '\n' for r in rows)
    text += ''.join('b %s\n' % float(r).hex() for r in ratios)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split('\n')
    assert lines[len(rows) + len(ratios)] == 'verdict host rules: ok'
    vbar, vstar = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    n = len(rows)
    for k in range(n):
        e_a, e_r = rows[k][2], rows[k][3]
        st, ratio = ac.statuses(vbar[k:k + 1], vstar[k:k + 1], [True], [0], e_a, e_r, rtol)
        _, st_u, ratio_u = apc.statuses(vbar[k:k + 1], np.zeros(1), vstar[k:k + 1], [0], [0], [0],
                                        e_a, e_r, rtol)
        got_st, got_bin, got_r = lines[k].split()
        assert int(got_st) == st[0] == st_u[0], (rows[k], lines[k])
        assert np.array_equal(np.array([float.fromhex(got_r)]), ratio, equal_nan=True)
        assert np.array_equal(ratio, ratio_u, equal_nan=True)
        hist = ac.summary([0], np.zeros(1, dtype=np.int32), ratio)[1]
        hist_u = apc.summary([0], np.zeros(1, dtype=np.int32), ratio_u)[1]
        assert hist[int(got_bin)] == 1 == hist_u[int(got_bin)], (rows[k], lines[k])
    for k, r in enumerate(ratios):
        hist = ac.summary([0], np.zeros(1, dtype=np.int32), np.array([r]))[1]
        assert hist[int(lines[n + k])] == 1, (r, lines[n + k])
    assert [int(v) for v in lines[n:n + 10]] == [0, 0, 1, 31, 31, 31, 32, 32, 0, 0]
