"""
The compiled explicit law on the host (no GPU): the numpy mirror tests/compiled_cpu.py -- its
classification, records and walk -- against the exact arithmetic of tests/explicit_synth.py at
every width, and the library's validator of imported arrays (ehm_compiled_validate, host code).

Tolerances: the mirror's leaf must be the exact one wherever every decision's exact margin exceeds
1e-10 (1 + kappa) (``SynthLaw.decisive``); the input must be within ``SynthLaw.u_tol`` with c = 64
(the project's bound for an interpolated input, c doubled from 32 because the gain is built from
differences u_i - u_0 of magnitude up to 2 max|U|) of the exact interpolation in that leaf.
"""

from fractions import Fraction

import numpy as np
import pytest

from explicit_hybrid_mpc_amd import _capi, compiled
from tests import compiled_cpu as cc
from tests import explicit_synth as es


def test_fma_is_exact():
    """The mirror's fused multiply-add against rational arithmetic, cancellation included."""
    rng = np.random.default_rng(1)
    a = rng.normal(size=4000) * 10. ** rng.integers(-8, 9, 4000)
    b = rng.normal(size=4000) * 10. ** rng.integers(-8, 9, 4000)
    c = np.where(rng.random(4000) < 0.5, -a * b * (1 + rng.integers(-4, 5, 4000) * cc.EPS),
                 rng.normal(size=4000))
    # half-way cases: a b + c with the product's low part exactly at a rounding boundary
    a[:8], b[:8] = 1. + 2. ** -30, 1. + 2. ** -23
    c[:8] = np.array([1., -1., 2. ** -53, -2. ** -53, 2. ** 52, -2. ** 52, 3., 2. ** -60])
    got = cc.fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        assert g == float(Fraction(x) * Fraction(y) + Fraction(z)), (x, y, z)


@pytest.mark.parametrize('p', range(1, 9), ids=lambda p: 'p%d' % p)
def test_mirror_against_exact_walk(p):
    rng = np.random.default_rng(300 + p)
    law = es.SynthLaw(es.kuhn_forest(p, 100), p % 6 + 1, 2, rng)
    arrays, split = cc.compile_flat(law.flat)
    compiled.validate_arrays(arrays)
    h = dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))
    internal = np.nonzero(law.left >= 0)[0]
    assert h['n_test'] == 0 and h['n_int'] == internal.size and h['n_leaf'] == law.leaves.size
    for k in internal:
        assert split[k] == law.split[law.left[k]][:2], k
    X = law.states(rng, 2400)
    u, leaf, depth, smin = cc.evaluate(arrays, X)
    decisive = 0
    for q, x in enumerate(X):
        ref = law.locate(x)
        k = int(leaf[q])
        if law.decisive(ref):
            decisive += 1
            assert k == ref.leaf, (q, k, ref.leaf, float(ref.margin))
            assert depth[q] == ref.tests
        lam = cc.check_plane_path(law, k, ref)
        ue = law.u_exact(k, lam, ref.D)
        tol = law.u_tol(max(ref.kappa, law.kappa(k)), lam, ref.D, c=64.)
        assert np.all(np.abs(u[q] - ue) <= tol), (q, u[q], ue, tol)
    assert decisive >= X.shape[0] // 4


def test_children_with_different_split_points_become_test_nodes():
    arrays, split = cc.compile_flat(cc.two_point_tree())
    h = dict(zip(cc.HEADER, (int(v) for v in arrays['header'])))
    assert h['n_test'] == 1 and h['n_int'] == 1 and split[0] is None
    assert (arrays['node'][0, :1] == 0.).all() and arrays['node'][0, 1] == 0.
    compiled.validate_arrays(arrays)
    u, leaf, depth, smin = cc.evaluate(arrays, np.array([[0.25], [0.5], [0.55], [0.9]]))
    assert leaf.tolist() == [1, 1, 2, 2] and (depth == 1).all() and np.isinf(smin).all()
    assert np.allclose(u[:, 0], [0.25, 0.5, 0.55, 0.9], rtol=0, atol=1e-15)


def test_validator_refuses_malformed_arrays():
    law = es.SynthLaw(es.kuhn_forest(2, 100), 2, 1, np.random.default_rng(5))
    arrays, _ = cc.compile_flat(law.flat)
    compiled.validate_arrays(arrays)
    for name, bad in cc.malformed(arrays):
        with pytest.raises(_capi.EhmError) as err:
            compiled.validate_arrays(bad)
        assert err.value.code == _capi.EHM_E_INVALID, name
    short = dict(arrays, node=arrays['node'][:-1])
    with pytest.raises(_capi.EhmError):
        compiled.validate_arrays(short)
