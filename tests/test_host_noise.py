"""
The uncertainty model of the noisy rollout, the host side (explicit_hybrid_mpc_amd/noise.py): the
vectorised Philox4x64-10 against numpy's, the uniform mapping, the reference's cwh_z model, the
sets and distributions of the draws, the counter scheme, and the C entry points without a CPU
fallback.
"""

import numpy as np
import pytest
from scipy import stats

from explicit_hybrid_mpc_amd import _capi, noise
from explicit_hybrid_mpc_amd.mpc_library import SatelliteZ, satellite_parameters
from explicit_hybrid_mpc_amd.noise import NoiseModel

M64 = (1 << 64) - 1


def _numpy_block(ctr, key):
    """numpy's block of counter ctr: random_raw returns the block of its counter + 1."""
    c = sum(int(w) << (64 * i) for i, w in enumerate(ctr))
    c = (c - 1) % (1 << 256)
    prev = np.array([(c >> (64 * i)) & M64 for i in range(4)], dtype=np.uint64)
    return np.random.Philox(counter=prev, key=np.array(key, dtype=np.uint64)).random_raw(4)


def test_philox_matches_numpy():
    # the stated convention: counter [5, 0, 0, 0], key [7, 9] -> the block of [6, 0, 0, 0]
    assert int(np.random.Philox(counter=np.array([5, 0, 0, 0], dtype=np.uint64),
                                key=np.array([7, 9], dtype=np.uint64)).random_raw(4)[0]) \
        == 0xca3338aabc68b165
    assert int(noise.philox4x64_10(6, 0, 0, 0, 7, 9)[0]) == 0xca3338aabc68b165
    rng = np.random.default_rng(0)
    C = rng.integers(0, 1 << 63, (200, 4), dtype=np.uint64) * np.uint64(2) \
        + rng.integers(0, 2, (200, 4), dtype=np.uint64)
    keys = rng.integers(0, 1 << 63, (200, 2), dtype=np.uint64)
    # word-carry edges of numpy's increment
    edges = [[M64, 0, 0, 0], [0, M64, 0, 0], [M64, M64, M64, 3], [0, 0, 0, 1], [1, 0, 0, 0],
             [0, 0, 0, M64], [M64, M64, M64, M64]]
    C = np.vstack([C, np.array(edges, dtype=np.uint64)])
    keys = np.vstack([keys, np.array([[11, 0], [M64, M64]] * 4, dtype=np.uint64)[:len(edges)]])
    for k in (0, M64):                       # one key for the whole vectorised batch
        got = noise.philox4x64_10(C[:, 0], C[:, 1], C[:, 2], C[:, 3], k, 0)
        for i in range(0, C.shape[0], 9):
            assert [int(g[i]) for g in got] == [int(w) for w in _numpy_block(C[i], [k, 0])]
    for i in range(C.shape[0]):
        got = noise.philox4x64_10(*C[i], int(keys[i, 0]), int(keys[i, 1]))
        assert [int(g) for g in got] == [int(w) for w in _numpy_block(C[i], keys[i])], i


def test_uniform_mapping_is_exact():
    r = np.array([0, 1 << 11, (1 << 63) - 1, 1 << 63, M64, 0x1234567890abcdef], dtype=np.uint64)
    s = noise.uniform_pm1(r)
    assert s[0] == -1. and s[1] == -1. + 2. ** -52 and s[3] == 0. and s[4] == 1. - 2. ** -52
    # exact: (s + 1) 2^52 is the integer r >> 11
    for ri, si in zip(r, s):
        assert (si + 1.) * 2. ** 52 == float(int(ri) >> 11)
    assert np.all(s >= -1.) and np.all(s < 1.)


def test_from_mpc_restates_the_reference_model():
    mpc = SatelliteZ(4)
    m = NoiseModel.from_mpc(mpc)
    p = satellite_parameters()
    # lib/mpc_library.py:236-255, in that order
    want = [('process', 'box', 1), ('state', 'box', 2), ('input', 'ball', 1),
            ('state', 'ball', 1), ('state', 'ball', 1), ('input', 'ball', 1)]
    assert [(t.kind, t.shape, t.dim) for t in m.terms] == want
    assert (m.n_x, m.n_u, m.n_d) == (2, 1, 1)
    assert np.array_equal(m.terms[0].h, [p['w_max']]) and np.array_equal(m.terms[0].c, [0.])
    assert np.array_equal(m.terms[1].h, [p['p_max'], p['v_max']])
    assert np.array_equal(m.terms[1].c, [0., 0.])
    t2, t3, t4, t5 = m.terms[2:]
    assert (t2.sigma, t2.norm, t2.dep) == (p['sigma_fix'], 2, 'const')
    assert (t3.sigma, t3.norm, t3.dep, t3.p_dep) == (p['sigma_pos'], 0, 'state', 2)
    assert np.array_equal(t3.F, [[1., 0.]]) and np.array_equal(t3.map, [[1.], [0.]])
    assert (t4.sigma, t4.norm, t4.dep, t4.p_dep) == (p['sigma_vel'], 0, 'state', 2)
    assert np.array_equal(t4.F, [[0., 1.]]) and np.array_equal(t4.map, [[0.], [1.]])
    assert (t5.sigma, t5.norm, t5.dep, t5.p_dep) == (p['sigma_rcs'], 2, 'input', 2)
    assert np.array_equal(t5.F, [[1.]])
    # the bounds _tightening uses: ub of the boxes, sigma of the balls, the columns of D
    assert np.array_equal(np.concatenate([m.terms[0].h, m.terms[1].h]),
                          [p['w_max'], p['p_max'], p['v_max']])
    assert np.array_equal([t.sigma for t in m.terms[2:]], mpc.sigma)
    gain = {'process': mpc.E, 'state': -mpc.A, 'input': mpc.B}
    D = np.hstack([gain[t.kind] @ t.map for t in m.terms])
    assert np.array_equal(D, np.hstack([mpc.E, -mpc.A, mpc.B, -mpc.A[:, :1], -mpc.A[:, 1:],
                                        mpc.B]))
    assert np.array_equal(D[:, [0, 1, 2]], np.hstack([mpc.E, -mpc.A]))
    # laws without an uncertainty model
    from explicit_hybrid_mpc_amd import examples
    assert NoiseModel.from_mpc(examples.pwa_mpc(0)) is None


def _mixed_model():
    m = NoiseModel(3, 2, 2)
    m.addIndependentTerm('process', lb=[-1., 0.5], ub=[2., 0.75])
    m.addIndependentTerm('state', lb=-np.arange(1., 7.), ub=np.arange(1., 7.),
                         M=np.arange(18.).reshape(3, 6) / 10.)
    m.addDependentTerm('state', 0.3, norm=2, dim=3)
    m.addDependentTerm('state', 0.2, norm=2, L=np.array([[1., 0.], [0., 2.], [1., 1.]]),
                       Fx=np.array([[1., 2., 0.], [0., 0., 1.]]), px=1)
    m.addDependentTerm('input', 0.1, norm=np.inf, dim=2, Fu=np.eye(2), pu=np.inf)
    m.addDependentTerm('input', 0.05, norm=1, L=np.array([[1.], [-1.]]))
    m.addDependentTerm('process', 0.5, norm=2, dim=2, Fx=np.eye(3), px=2)
    return m


def test_samples_lie_in_their_sets():
    rng = np.random.default_rng(1)
    n = 4000
    ids = np.arange(n)
    x, u = rng.normal(size=(n, 3)), rng.normal(size=(n, 2))
    m = _mixed_model()
    for j, term in enumerate(m.terms):
        if term.shape == 'box':
            S = m._draw(j, term, 5, ids.astype(np.uint64), 3, x, u)
            assert np.all(S >= term.c - term.h) and np.all(S <= term.c + term.h)
        else:
            S = m._draw(j, term, 5, ids.astype(np.uint64), 3, x, u)
            if term.dep == 'const':
                r = np.full(n, term.sigma)
            elif term.dep == 'state':
                r = term.sigma * np.linalg.norm(x @ term.F.T, ord=[np.inf, 1, 2][term.p_dep],
                                                axis=1)
            else:
                r = term.sigma * np.linalg.norm(u @ term.F.T, ord=[np.inf, 1, 2][term.p_dep],
                                                axis=1)
            nrm = np.linalg.norm(S, ord=[np.inf, 1, 2][term.norm], axis=1)
            assert np.all(nrm <= r * (1 + 1e-15))
            assert np.mean(nrm > 0.5 * r) > 0.5
    # the sums of the kinds are the mapped draws
    for kind in noise.KINDS:
        tot = m.sample(kind, 5, ids, 3, x, u)
        ref = sum(m._draw(j, t, 5, ids.astype(np.uint64), 3, x, u) @ t.map.T
                  for j, t in enumerate(m.terms) if t.kind == kind)
        assert np.allclose(tot, ref, rtol=1e-12, atol=1e-12)


def test_box_draws_are_uniform():
    m = NoiseModel(6, 1, 0)
    m.addIndependentTerm('state', lb=-np.ones(6), ub=np.ones(6) * 3.)
    V = m.sample('state', 2024, np.arange(20000), 0, np.zeros((20000, 6)), np.zeros((20000, 1)))
    for k in range(6):                       # two Philox blocks, both words of each
        assert stats.kstest(V[:, k], stats.uniform(loc=-1., scale=4.).cdf).pvalue > 1e-3, k
    assert abs(np.corrcoef(V.T)[0, 5]) < 0.05


@pytest.mark.parametrize('dim', [2, 3])
def test_two_ball_radius_has_cdf_r_to_the_d(dim):
    m = NoiseModel(3, 1, 0)
    m.addDependentTerm('state', 2.0, norm=2, dim=dim, L=np.eye(3)[:, :dim])
    n = 20000
    V = m.sample('state', 7, np.arange(n), 11, np.zeros((n, 3)), np.zeros((n, 1)))
    r = np.linalg.norm(V, axis=1) / 2.0
    assert r.max() <= 1.
    assert stats.kstest(r, lambda q: np.clip(q, 0, 1) ** dim).pvalue > 1e-3
    # directions: uniform on the sphere (mean ~ 0)
    assert np.all(np.abs(V[:, :dim].mean(axis=0)) < 0.05)


def test_input_error_is_zero_without_input():
    """lib/simulator.py:172-174: no rogue input error while the input is off."""
    from explicit_hybrid_mpc_amd import simulate
    mpc = SatelliteZ(4)
    m = NoiseModel.from_mpc(mpc)
    plant = simulate.Plant.from_mpc(mpc)

    class Oracle:
        """An oracle whose law never acts (commutation 0: input off)."""
        canonical = type('C', (), {'deltas': [np.zeros(8)]})()

        def __init__(self):
            self.mpc = mpc
            self.gpu = self

        def solve_pt(self, z):
            return np.zeros(len(z)), np.zeros((len(z), 1)), np.zeros(len(z), dtype=np.int64)

    X0 = np.random.default_rng(3).uniform(-1, 1, (32, 2)) * [1e-2, 1e-4]
    res = simulate.rollout_implicit(Oracle(), plant, X0, 6, noise=m, seed=4)
    assert np.all(res.e == 0.) and np.all(res.u == 0.) and np.all(res.u_norm_sum == 0.)
    assert np.all(res.w != 0.) and np.all(res.v != 0.)
    # the fixed input error is drawn (it is not zero where u != 0)
    e = m.sample('input', 4, np.arange(32), 0, X0, np.full((32, 1), 1e-3))
    assert np.all(e != 0.) and np.all(np.abs(e) <= 1e-6 + np.tan(np.deg2rad(1.)) * 1e-3)
    # the plant stepped with E w only: x+ = A x + E w
    x1 = X0 @ mpc.A.T + res.w[0] @ mpc.E.T
    assert np.allclose(res.x[1], x1, rtol=1e-13, atol=1e-20)


def test_splitting_the_trajectories_gives_the_same_draws():
    m = _mixed_model()
    rng = np.random.default_rng(9)
    n = 300
    x, u = rng.normal(size=(n, 3)), rng.normal(size=(n, 2))
    for kind in noise.KINDS:
        whole = m.sample(kind, 77, np.arange(n), 5, x, u)
        a = m.sample(kind, 77, np.arange(0, 120), 5, x[:120], u[:120])
        b = m.sample(kind, 77, np.arange(120, n), 5, x[120:], u[120:])
        assert np.array_equal(whole, np.vstack([a, b]))
        # the draw of a trajectory does not depend on its position in the batch
        perm = rng.permutation(n)
        assert np.array_equal(m.sample(kind, 77, perm, 5, x[perm], u[perm]), whole[perm])
        # another seed or step changes it
        assert not np.array_equal(m.sample(kind, 78, np.arange(n), 5, x, u), whole)
        assert not np.array_equal(m.sample(kind, 77, np.arange(n), 6, x, u), whole)


def test_model_limits_are_checked():
    m = NoiseModel(2, 1, 1)
    with pytest.raises(ValueError):
        m.addDependentTerm('state', 1., norm=2, dim=4)
    with pytest.raises(ValueError):
        m.addDependentTerm('state', 1., norm=1, dim=2)
    with pytest.raises(ValueError):
        m.addIndependentTerm('state', lb=[0.], ub=[1.])         # map 2 x 1 needed
    with pytest.raises(ValueError):
        m.addIndependentTerm('bogus', lb=[0.], ub=[1.], M=np.ones((1, 1)))
    desc, data = NoiseModel.from_mpc(SatelliteZ(4)).pack()
    assert desc.shape == (6, noise.DESC_WORDS) and desc.dtype == np.int32
    assert desc[-1, 7] + 1 + 1 + 1 == data.size           # sigma, F [1x1], L [1x1]


def test_noise_with_d_or_v_is_refused():
    from explicit_hybrid_mpc_amd import explicit, simulate
    mpc = SatelliteZ(4)
    m = NoiseModel.from_mpc(mpc)
    X0 = np.zeros((2, 2))
    d, v = np.zeros((3, 2, 1)), np.zeros((3, 2, 2))
    plant = simulate.Plant.from_mpc(mpc)
    for kw in (dict(d=d), dict(v=v), dict(d=d, v=v)):
        with pytest.raises(ValueError):
            simulate.rollout_implicit(None, plant, X0, 3, noise=m, **kw)
        law = explicit.ExplicitMPC.__new__(explicit.ExplicitMPC)
        with pytest.raises(ValueError):
            law.rollout(X0, 3, noise=m, **kw)


def test_noise_entry_points_have_no_cpu_fallback():
    lib = _capi.load()
    desc, data = NoiseModel.from_mpc(SatelliteZ(4)).pack()
    assert lib.ehm_explicit_set_noise(None, desc.shape[0], desc.ctypes.data, data.ctypes.data,
                                      data.size, 1) == _capi.EHM_E_INVALID
    out = [np.zeros(4), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32),
           np.zeros(2), np.zeros(2), np.zeros(2)]
    rc = lib.ehm_explicit_rollout_noisy(None, 2, 3, np.zeros(4).ctypes.data, 1, 0, 1e-9,
                                        None, None, None, None, None, None,
                                        *[a.ctypes.data for a in out], None)
    assert rc == _capi.EHM_E_INVALID
    assert lib.ehm_philox_batch(4, None, None, None) == _capi.EHM_E_INVALID
    ctr = np.zeros((1, 4), dtype=np.uint64)
    key = np.zeros(2, dtype=np.uint64)
    blk = np.zeros((1, 4), dtype=np.uint64)
    rc = lib.ehm_philox_batch(1, ctr.ctypes.data, key.ctypes.data, blk.ctypes.data)
    if rc != _capi.EHM_OK:                     # no device: refused, not computed on the host
        assert rc in (_capi.EHM_E_NO_DEVICE, _capi.EHM_E_HIP) and not blk.any()
