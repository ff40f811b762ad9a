"""
The single-precision compiled law on the host (no GPU): the numpy mirror tests/compiled32_cpu.py
against the double mirror tests/compiled_cpu.py under the two bounds of the contract (DESIGN.md
3.8c, "single precision"; derived in compiled32_cpu's docstring), the refusals of the narrowing,
the library's validator of float arrays (ehm_compiled_validate_single, host code) and the file.

The trees are those of test_host_compiled (``kuhn_forest(p, 100)``, subtrees to depth 8..20, sliver
chains to depth 26); the states are uniform inside uniformly chosen leaves.  Share of the 2000
states per p that end in the double law's leaf, measured with these seeds: p = 1: 0.89, 2: 0.93,
3: 0.93, 4: 0.95, 5: 0.95, 6: 0.96, 7: 0.94, 8: 0.94 (the rest sit in leaves of the deep chains
that a float cannot resolve); the test asks for three quarters, so the bounds cannot carry it.
"""

from fractions import Fraction

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled
from tests import compiled32_cpu as c32
from tests import compiled_cpu as cc
from tests import explicit_synth as es

N_STATES, N_EXACT = 2000, 1500


def _law(p):
    rng = np.random.default_rng(500 + p)
    law = es.SynthLaw(es.kuhn_forest(p, 100), p % 4 + 1, 2, rng)
    return law, rng


def _states_in_leaves(law, rng, n):
    """Uniform in uniformly chosen leaves: barycentric weights Dirichlet(1, .., 1)."""
    k = rng.choice(law.leaves, n)
    w = rng.dirichlet(np.ones(law.p + 1), n)
    return np.einsum('nv,nvc->nc', w, law.vertices[k])


@pytest.mark.parametrize('p', range(1, 9), ids=lambda p: 'p%d' % p)
def test_turns_and_inputs_within_the_bounds(p):
    law, rng = _law(p)
    arrays, _ = cc.compile_flat(law.flat)
    a32 = c32.narrow(arrays)
    compiled.validate_arrays(a32)
    h = dict(zip(cc.HEADER, (int(v) for v in a32['header'])))
    assert 4 * h['node_stride'] == (32 if p <= 5 else 64) == 4 * compiled.node_stride32(p)
    assert h['leaf_stride'] == compiled.leaf_stride32(p, h['n_u']) and h['leaf_stride'] % 4 == 0
    for k in ('leaf_node', 'root_rec', 'root_entry', 'nbr', 'test_rec'):
        assert a32[k].tobytes() == arrays[k].tobytes() and a32[k].dtype == arrays[k].dtype, k
    X = _states_in_leaves(law, rng, N_STATES)
    u64, leaf64, depth64, _ = cc.evaluate(arrays, X)
    u32, leaf32, depth32, levels = c32.evaluate32(a32, X)
    same = leaf64 == leaf32
    print('p %d: share in the double law\'s leaf %.4f' % (p, same.mean()))
    assert 4 * same.sum() >= 3 * N_STATES, same.mean()
    assert np.array_equal(depth32[same], depth64[same])
    # turns: every turn on the single path is the double mirror's, or |s64| <= turn_bound
    node64 = arrays['node']
    xs = X.astype(np.float32)
    pairs, against = [], 0
    for live, nodes, s32, left in levels:
        bound, s64 = c32.turn_bound(arrays, nodes, X[live])
        differs = left != (s64 >= -cc.EPS)
        assert (~differs | (np.abs(s64) <= bound)).all(), (p, np.abs(s64[differs]), bound[differs])
        against += int(differs.sum())
        pairs += [(int(q), int(k), float(s), float(b), bool(d))
                  for q, k, s, b, d in zip(live, nodes, s32, bound, differs)]
    print('p %d: %d turns, %d against the double law' % (p, len(pairs), against))
    # the bound itself, in rational arithmetic: the single sum is within turn_bound of the exact
    # a . x + b of the double record, and of the narrowed record at the narrowed state
    pick = [t for t in pairs if t[4]]
    rest = [t for t in pairs if not t[4]]
    pick += [rest[i] for i in rng.choice(len(rest), min(N_EXACT, len(rest)), replace=False)]
    for q, k, s, b, _ in pick:
        assert abs(Fraction(s) - c32.exact_sum(node64[k], X[q], p)) <= Fraction(b), (p, q, k)
        assert abs(Fraction(s) - c32.exact_sum(a32['node'][k], xs[q], p)) <= Fraction(b), (p, q, k)
    # inputs: in the same leaf within u_bound
    l = np.searchsorted(arrays['leaf_node'], leaf64[same])
    assert np.array_equal(arrays['leaf_node'][l], leaf64[same])
    ub = c32.u_bound(arrays, l, X[same])
    assert (np.abs(u32[same] - u64[same]) <= ub).all()
    assert (u32[same] != u64[same]).any()         # it is another arithmetic
    assert (u32 == u32.astype(np.float32)).all()  # every input is a widened float


def test_narrowing_refusals():
    law, rng = _law(2)
    arrays, _ = cc.compile_flat(law.flat)
    c32.narrow(arrays)

    def variant(name, row, col, value):
        out = {k: np.array(v, copy=True) for k, v in arrays.items()}
        out[name][row, col] = value
        return out

    with pytest.raises(c32.NarrowError) as err:
        c32.narrow(cc.compile_flat(cc.two_point_tree())[0])
    assert err.value.reason == 'test nodes'
    cases = [('overflow', variant('node', 3, 1, 1e39)),
             ('overflow', variant('leaf_rec', 0, 4, -3.5e38)),
             ('underflow', variant('leaf_rec', 5, 0, 1e-46)),           # becomes zero
             ('underflow', variant('node', 1, 2, -1e-40)),              # becomes subnormal
             ('zero normal', variant('node', 2, slice(0, 2), 0.))]
    for reason, bad in cases:
        with pytest.raises(c32.NarrowError) as err:
            c32.narrow(bad)
        assert err.value.reason == reason
    # the largest double below FLT_MIN that still rounds to a normal float is kept
    edge = variant('leaf_rec', 5, 0, float(np.nextafter(np.float64(2. ** -126), 0.)))
    assert c32.narrow(edge)['leaf_rec'][5, 0] == np.float32(2. ** -126)


def test_validator_refuses_malformed_single_arrays():
    law, _ = _law(3)
    arrays, _ = cc.compile_flat(law.flat)
    a32 = c32.narrow(arrays)
    compiled.validate_arrays(a32)
    p = 3

    def variant(**kw):
        out = {k: np.array(v, copy=True) for k, v in a32.items()}
        for k, fn in kw.items():
            fn(out[k])
        return out

    def set_at(row, col, value):
        def fn(a):
            a[row, col] = value
        return fn

    def child(value):
        def fn(node):
            node.view(np.int32)[0, p + 1] = value
        return fn

    def header(i, value):
        def fn(hd):
            hd[i] = value
        return fn

    n_int, n_leaf = int(a32['header'][4]), int(a32['header'][5])
    bad = [('child out of range', variant(node=child(n_int))),
           ('leaf child out of range', variant(node=child(~n_leaf))),
           ('child not after its parent', variant(node=child(0))),
           ('inf plane', variant(node=set_at(0, 0, np.inf))),
           ('NaN leaf record', variant(leaf_rec=set_at(0, 1, np.nan))),
           ('subnormal plane', variant(node=set_at(1, p, 1e-40))),
           ('subnormal leaf record', variant(leaf_rec=set_at(2, 0, -1e-44))),
           ('zero normal', variant(node=set_at(1, slice(0, p), 0.))),
           ('test nodes', variant(header=header(6, 1))),
           ('wrong node stride', variant(header=header(7, 16))),
           ('wrong leaf stride', variant(header=header(8, int(a32['header'][8]) + 2))),
           ('wrong version', variant(header=header(0, 2)))]
    for name, arrs in bad:
        with pytest.raises(_capi.EhmError) as err:
            compiled.validate_arrays(arrs)
        assert err.value.code == _capi.EHM_E_INVALID, name
    # one narrowed array and one double array are no law of either precision
    with pytest.raises(_capi.EhmError):
        compiled.validate_arrays(dict(a32, leaf_rec=arrays['leaf_rec']))


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k         # (child pairs: by bytes)


def test_file_round_trip_of_both_precisions(tmp_path):
    law, _ = _law(2)
    arrays, _ = cc.compile_flat(law.flat)
    a32 = c32.narrow(arrays)
    modes = np.arange(int(arrays['header'][5]), dtype=np.int32) % 3 - 1
    path = str(tmp_path / 'law.npz')
    # single: the key, float32 arrays, the same 12-word header layout and format version
    compiled.write_file(path, a32, modes)
    with np.load(path) as z:
        assert int(z['precision']) == 32 and int(z['format_version']) == compiled.FORMAT_VERSION
        assert z['node'].dtype == np.float32 and z['leaf_rec'].dtype == np.float32
        assert z['header'].shape == (12,) and z['root_rec'].dtype == np.float64
    got, lm = compiled.read_file(path)
    _same(got, a32)
    assert np.array_equal(lm, modes) and compiled.precision_of(got) == 32
    compiled.validate_arrays(got)
    # double: no key, the file every earlier version wrote; and such a file loads unchanged
    compiled.write_file(path, arrays, modes)
    old = str(tmp_path / 'old.npz')
    with open(old, 'wb') as f:
        np.savez(f, format_version=np.int64(1), **arrays, leaf_mode=modes)
    with np.load(path) as z, np.load(old) as zo:
        assert 'precision' not in z.files and sorted(z.files) == sorted(zo.files)
        for k in z.files:
            assert z[k].tobytes() == zo[k].tobytes() and z[k].dtype == zo[k].dtype, k
    for file in (path, old):
        got, lm = compiled.read_file(file)
        _same(got, arrays)
        assert np.array_equal(lm, modes) and compiled.precision_of(got) == 64
        compiled.validate_arrays(got)

    def write(arrs, **extra):
        with open(path, 'wb') as f:
            np.savez(f, format_version=np.int64(1), **arrs, **extra)

    # a double file may state its precision
    write(arrays, precision=np.int64(64))
    _same(compiled.read_file(path)[0], arrays)
    # another precision, and dtypes that contradict the key
    refused = [(arrays, 16), (a32, 16), (arrays, 32), (a32, 64), (dict(a32, node=arrays['node']), 32),
               (dict(arrays, leaf_rec=a32['leaf_rec']), 64)]
    for arrs, precision in refused:
        write(arrs, precision=np.int64(precision))
        with pytest.raises(_capi.EhmError) as err:
            compiled.read_file(path)
        assert err.value.code == _capi.EHM_E_INVALID, precision
