"""
The closed loop under an uncertainty model on the device (ehm_explicit_rollout_noisy, noise.py):
the device Philox against numpy's, every recorded step of noisy rollouts against the host sampler,
the one-step evaluator and a numpy plant step, the counter scheme (record, split batches, seeds),
common random numbers with the implicit law, and the reference's experiment from x0 = 0.
"""

import numpy as np
import pytest

from tests import noise_cpu
from tests.test_gpu_rollout import _lin, _law, _pwa_small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cwh():
    """cwh_z job 1 (abs_frac 0.5, rel_err 2): its partition and its oracle."""
    from explicit_hybrid_mpc_amd import examples
    from oracle import geometry
    full_set, _, oracle = examples.example('cwh_z', abs_frac=0.5, rel_err=2.0)
    roots, _ = geometry.delaunay_simplices(full_set)
    flat = oracle.gpu.partition(np.array(roots), action='ecc')
    yield oracle, flat
    oracle.close()


def test_device_philox_matches_numpy():
    from explicit_hybrid_mpc_amd import _capi, noise
    lib = _capi.load()
    rng = np.random.default_rng(11)
    n = 100000
    C = rng.integers(0, 1 << 62, (n, 4), dtype=np.uint64) * np.uint64(4)
    C[:4] = np.array([[2 ** 64 - 1, 0, 0, 0], [0, 2 ** 64 - 1, 2 ** 64 - 1, 0], [0, 0, 0, 0],
                      [2 ** 64 - 1] * 4], dtype=np.uint64)
    key = np.array([0xdeadbeefcafe, 0], dtype=np.uint64)
    out = np.zeros((n, 4), dtype=np.uint64)
    assert lib.ehm_philox_batch(n, C.ctypes.data, key.ctypes.data, out.ctypes.data) == 0
    host = np.stack(noise.philox4x64_10(C[:, 0], C[:, 1], C[:, 2], C[:, 3], int(key[0])), axis=1)
    assert np.array_equal(out, host)
    M = (1 << 64) - 1
    for i in list(range(4)) + list(range(4, n, 997)):
        c = (sum(int(w) << (64 * j) for j, w in enumerate(C[i])) - 1) % (1 << 256)
        prev = np.array([(c >> (64 * j)) & M for j in range(4)], dtype=np.uint64)
        assert np.array_equal(out[i], np.random.Philox(counter=prev, key=key).random_raw(4)), i


def _setup(kind, cwh):
    from explicit_hybrid_mpc_amd import examples
    from explicit_hybrid_mpc_amd.noise import NoiseModel, state_input_model
    if kind == 'cwh_z':
        oracle, flat = cwh
        mpc = oracle.mpc
        model = NoiseModel.from_mpc(mpc)
        half = examples.theta_box(mpc)
    else:
        mpc, flat = _lin() if kind == 'lin' else _pwa_small()
        half = examples.theta_box(mpc)
        model = state_input_model(half, mpc.B[0].shape[1])
        assert max(t.dim for t in model.terms if t.shape == 'box') > 4     # two Philox blocks
    return mpc, flat, model, half


@pytest.mark.parametrize('kind', ['cwh_z', 'lin', 'pwa_small'])
def test_noisy_rollout_matches_the_host_sampler(kind, cwh):
    mpc, flat, model, half = _setup(kind, cwh)
    ex = _law(mpc, flat)
    rng = np.random.default_rng(21)
    n, T = 2048, 40
    X0 = rng.uniform(-1, 1, (n, half.size)) * half * 0.8
    res = ex.rollout(X0, T, noise=model, seed=5, traj0=3)
    assert noise_cpu.check_noisy_steps(ex, res, X0, T, model, 5, traj0=3) > n
    assert np.any(res.e[np.isfinite(res.e)] != 0.)
    # record=False gives the same figures
    res2 = ex.rollout(X0, T, noise=model, seed=5, traj0=3, record=False)
    assert res2.v is None and res2.e is None and res2.w is None
    for f in ('x_final', 'steps', 'status', 'cost', 'u_norm_sum', 'max_violation'):
        assert np.array_equal(getattr(res2, f), getattr(res, f)), f
    # one batch of 2m = two batches of m with traj0 = 3, 3 + m
    m = n // 2
    a = ex.rollout(X0[:m], T, noise=model, seed=5, traj0=3)
    b = ex.rollout(X0[m:], T, noise=model, seed=5, traj0=3 + m)
    for f in ('x', 'u', 'v', 'e', 'w'):
        assert np.array_equal(np.concatenate([getattr(a, f), getattr(b, f)], axis=1),
                              getattr(res, f), equal_nan=True), f
    for f in ('x_final', 'steps', 'status', 'cost', 'u_norm_sum'):
        assert np.array_equal(np.concatenate([getattr(a, f), getattr(b, f)]), getattr(res, f))
    # the same seed reproduces, another seed changes the draws
    again = ex.rollout(X0, T, noise=model, seed=5, traj0=3)
    assert np.array_equal(again.x, res.x, equal_nan=True)
    other = ex.rollout(X0, T, noise=model, seed=6, traj0=3)
    assert not np.array_equal(other.v, res.v, equal_nan=True)
    # the device copy of the model follows the model's content, not its identity
    h0 = model.terms[1].h
    model.terms[1].h = 2. * h0
    changed = ex.rollout(X0, T, noise=model, seed=5, traj0=3)
    model.terms[1].h = h0
    assert not np.array_equal(changed.v, res.v, equal_nan=True)
    noise_cpu.check_noisy_steps(ex, ex.rollout(X0[:256], T, noise=model, seed=5, traj0=3),
                                X0[:256], T, model, 5, traj0=3)
    # nominal rollouts are untouched by a model set before
    nom = ex.rollout(X0, T)
    assert nom.v is None and np.all(np.isfinite(nom.x_final[nom.status == 0]))
    ex.close()


def test_implicit_law_sees_common_random_numbers(cwh):
    from explicit_hybrid_mpc_amd import examples, explicit
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    oracle, flat = cwh
    mpc = oracle.mpc
    model = NoiseModel.from_mpc(mpc)
    ex = explicit.ExplicitMPC(flat, oracle)
    im = explicit.ImplicitMPC(oracle)
    X0 = np.random.default_rng(8).uniform(-1, 1, (48, 2)) * examples.theta_box(mpc) * 0.5
    T = 15
    a = ex.rollout(X0, T, noise=model, seed=9)
    b = im.rollout(X0, T, noise=model, seed=9)
    # the implicit law's draws are the host sampler's at its own states and inputs
    ids = np.arange(48)
    u_prev = np.zeros((48, 1))
    both_steps = 0
    for t in range(T):
        on = np.nonzero(b.steps > t)[0]
        if on.size == 0:
            break
        assert np.array_equal(b.v[t, on], model.sample('state', 9, ids[on], t, b.x[t, on],
                                                       u_prev[on]))
        u_prev[on] = b.u[t, on]
        # the process draw is independent of the state: bit-equal between the laws
        both = np.nonzero((a.steps > t) & (b.steps > t))[0]
        assert np.array_equal(a.w[t, both], b.w[t, both])
        both_steps += both.size
    assert both_steps > 48 * T // 2
    # with only the independent terms, v, e and w are bit-equal wherever both laws are alive
    ind = NoiseModel(2, 1, 1)
    for term in model.terms[:2]:
        ind.addIndependentTerm(term.kind, lb=term.c - term.h, ub=term.c + term.h)
    a = ex.rollout(X0, T, noise=ind, seed=9)
    b = im.rollout(X0, T, noise=ind, seed=9)
    for t in range(T):
        both = np.nonzero((a.steps > t) & (b.steps > t))[0]
        for f in ('v', 'w'):
            assert np.array_equal(getattr(a, f)[t, both], getattr(b, f)[t, both]), (f, t)
    ex.close()


def test_cwh_z_from_the_origin_acts_and_stays_in_the_box(cwh):
    """The reference's experiment (lib/post_process.py:553-568): from x0 = 0 for 20 orbits
    (1 115 steps at T_s = 100 s).  Every trajectory stays millimetres from the origin inside the
    10 cm box, and the law acts: without noise the state never leaves 0 and u_norm_sum is 0."""
    from explicit_hybrid_mpc_amd.noise import NoiseModel
    from explicit_hybrid_mpc_amd.simulate import Simulator
    oracle, flat = cwh
    mpc = oracle.mpc
    ex = _law(mpc, flat)
    T = len(np.linspace(0, 20 * 2 * np.pi / mpc.pars['wo'],
                        int(20 * 2 * np.pi / mpc.pars['wo'] / mpc.T_s + 1)))
    assert T == 1115
    res = ex.rollout(np.zeros((1024, 2)), T, noise=NoiseModel.from_mpc(mpc), seed=1,
                     record=False)
    assert (res.status == 0).all(), np.bincount(res.status)
    assert (res.steps == T).all()
    assert res.max_violation.max() <= 0.
    assert np.abs(res.x_final[:, 0]).max() < 2e-2
    assert (res.u_norm_sum > 0).all()
    # the reference's Simulator signature with its noise
    sim = Simulator(ex, 20 * 2 * np.pi / mpc.pars['wo'], noise='reference', seed=1).run(
        np.zeros(2))
    assert sim.x.shape == (2, T) and sim.w.shape == (1, T) and sim.e.shape == (1, T)
    assert np.any(sim.v != 0.) and np.any(sim.w != 0.)
    one = ex.rollout(np.zeros((1, 2)), T, noise=NoiseModel.from_mpc(mpc), seed=1)
    assert np.array_equal(sim.x, one.x[:T, 0].T) and np.array_equal(sim.v, one.v[:, 0].T)
    ex.close()
