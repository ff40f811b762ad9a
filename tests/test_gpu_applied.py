"""
The audit of a law by the cost of the input it applies (csrc/ehm_applied.hip, applied.py, DESIGN.md
3.8e) on the device: exact at the optimal input, every reported array bit for bit what the public
entry points give, the sampler the one of the existing audit on the law's roots, sound laws
passing, a leaf with an inadmissible input found, single laws judged, and the refusals.

The trees are those of tests/test_gpu_audit.py (tens to hundreds of leaves), built once per module.
"""

import numpy as np
import pytest

from tests import applied_cpu as apc
from tests import audit_cpu as ac
from tests.test_gpu_audit import _Case, _oracle

pytestmark = pytest.mark.gpu

N = 3000
RTOL = 1e-7
NAMES = ('within', 'violation', 'negative', 'inadmissible', 'no_law', 'infeasible')


class _Applied(_Case):
    def __init__(self, kind):
        super().__init__(kind)
        self.compiled = self.law.compile()

    def close(self):
        self.compiled.close()
        super().close()


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Applied(kind)
        return made[kind]
    yield get
    for c in made.values():
        c.close()


def _check_against_the_entry_points(law, orc, res, ids):
    """Everything ``res`` reports, from the public entry points and the mirror."""
    from explicit_hybrid_mpc_amd import applied, engine
    n = res.n
    u, leaf, _, _ = law.evaluate(res.x, return_info=True)
    assert res.u.tobytes() == u.tobytes() and np.array_equal(res.leaf, leaf)
    J, _, didx = orc.gpu.solve_pt(res.x)
    assert res.vstar.tobytes() == J.tobytes() and np.array_equal(res.delta_idx, didx)
    red = applied.applied_input_problem(orc.gpu.can)
    theta, konst, no_law = apc.pack(res.x, res.u, red.cost_u)
    gp = engine.GpuProblem(red, orc.eps_a, orc.eps_r)
    Ju, _, didx_u = gp.solve_pt(theta)
    gp.close()
    if res.input_tol > 0.:
        wide = engine.GpuProblem(applied.applied_input_problem(orc.gpu.can, res.input_tol),
                                 orc.eps_a, orc.eps_r)

        def solve_relaxed(idx):
            J, _, d = wide.solve_pt(theta[idx])
            return J, d
        Ju, didx_u, relaxed = apc.fall_back(didx, Ju, didx_u, solve_relaxed)
        wide.close()
    else:
        relaxed = np.zeros(n, dtype=np.int32)
    assert np.array_equal(res.relaxed, relaxed) and res.n_relaxed == relaxed.sum()
    assert np.array_equal(res.delta_idx_applied, didx_u)
    vu, st, ratio = apc.statuses(Ju, konst, res.vstar, didx, didx_u, no_law, orc.eps_a, orc.eps_r,
                                 res.rtol)
    assert res.vu.tobytes() == vu.tobytes()
    assert np.array_equal(res.status, st)
    counts, hist, best, worst = apc.summary(ids, st, ratio)
    assert [res.counts[k] for k in NAMES] == counts.tolist() and counts.sum() == n
    assert np.array_equal(res.histogram, hist)
    assert res.max_ratio == best
    if worst < 0:
        assert res.worst is None
    else:
        q = int(np.nonzero(ids == worst)[0][0])
        w = res.worst
        assert w['id'] == worst and w['leaf'] == res.leaf[q]
        assert w['vu'] == res.vu[q] and w['vstar'] == res.vstar[q]
        assert np.array_equal(w['x'], res.x[q]) and np.array_equal(w['u'], res.u[q])
        assert w['bound'] == max(orc.eps_a, orc.eps_r * res.vstar[q])
    return st, ratio


@pytest.mark.parametrize('kind', ['lin', 'lin_quadratic', 'pwa_small'])
def test_exact_at_the_optimal_input(cases, kind):
    """With ubar = u* the fixed-input optimum is the optimum: |V_u - V*| <= rtol (1 + |V*|), under
    the exact substitution (input_tol = 0; a relaxation may only lower V_u)."""
    from explicit_hybrid_mpc_amd import applied
    c = cases(kind)
    X, _ = c.law.sample(n=96, seed=21)
    J, U, didx = c.orc.gpu.solve_pt(X)
    X, U, J = X[didx >= 0][:64], U[didx >= 0][:64], J[didx >= 0][:64]
    assert X.shape[0] == 64
    res = applied.audit_inputs(c.orc, X, U, rtol=RTOL, input_tol=0., return_samples=True)
    slack = RTOL * (1. + np.abs(J))
    print(kind, res, 'largest |V_u - V*| / slack %.3e' % np.max(np.abs(res.vu - J) / slack))
    assert res.vstar.tobytes() == J.tobytes()
    assert (res.delta_idx_applied >= 0).all()
    assert (res.vu >= J - slack).all() and (res.vu <= J + slack).all()
    assert res.counts['within'] == 64 and res.passed
    assert (res.root == -1).all() and (res.leaf == -1).all()


@pytest.mark.parametrize('kind', ['lin', 'lin_quadratic', 'pwa_small'])
def test_every_array_is_what_the_entry_points_give(cases, kind):
    c = cases(kind)
    law = c.compiled
    res = law.audit(c.orc, n=N, seed=5, return_samples=True)
    ids = np.arange(N)
    _check_against_the_entry_points(law, c.orc, res, ids)
    if kind == 'pwa_small':
        assert c.orc.gpu.can.n_delta == 8 and np.unique(res.delta_idx).size > 1
    # one chunk, several chunks and a range of ids split over two calls report the same
    many = law.audit(c.orc, n=N, seed=5, return_samples=True, chunk=700)
    a = law.audit(c.orc, n=1000, seed=5, return_samples=True)
    b = law.audit(c.orc, n=N - 1000, seed=5, return_samples=True, first=1000, chunk=1100)
    for key in ('x', 'root', 'leaf', 'u', 'vu', 'vstar', 'delta_idx', 'delta_idx_applied',
                'status', 'relaxed'):
        whole = getattr(res, key)
        assert getattr(many, key).tobytes() == whole.tobytes(), key
        assert np.concatenate([getattr(a, key), getattr(b, key)]).tobytes() == whole.tobytes(), key
    assert many.counts == res.counts and np.array_equal(many.histogram, res.histogram)
    assert many.max_ratio == res.max_ratio and many.worst['id'] == res.worst['id']
    assert {k: a.counts[k] + b.counts[k] for k in NAMES} == res.counts
    assert np.array_equal(a.histogram + b.histogram, res.histogram)
    assert max(a.max_ratio, b.max_ratio) == res.max_ratio
    assert res.worst['id'] in (a.worst['id'], b.worst['id'])
    bare = law.audit(c.orc, n=N, seed=5)
    assert bare.x is None and bare.counts == res.counts and bare.max_ratio == res.max_ratio
    # the caller's points instead of drawn ones
    mine = law.audit(c.orc, X=res.x[:500], return_samples=True)
    assert mine.vu.tobytes() == res.vu[:500].tobytes() and (mine.root == -1).all()
    assert np.array_equal(mine.status, res.status[:500])


@pytest.mark.parametrize('kind', ['di', 'lin'])
def test_the_points_are_the_samplers_on_the_roots(cases, kind, tmp_path):
    from explicit_hybrid_mpc_amd import applied
    from explicit_hybrid_mpc_amd.compiled import CompiledLaw
    c = cases(kind)
    law = c.compiled
    cells = applied.root_cells(law)
    assert cells['vertices'].shape == (c.roots.shape[0], law.p + 1, law.p)
    # the recovered vertices are the roots' up to the rounding of two inversions
    assert np.abs(cells['vertices'] - c.roots).max() <= 1e-9 * np.abs(c.roots).max()
    res = law.audit(c.orc, n=N, seed=11, return_samples=True)
    Xm, cm = ac.sample(cells['vertices'], cells['cdf'], np.arange(N), 11, ac.UNIFORM)
    assert res.x.tobytes() == Xm.tobytes() and np.array_equal(res.root, cm)
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = CompiledLaw.load(path)
    again = loaded.audit(c.orc, n=N, seed=11, return_samples=True)
    loaded.close()
    assert again.x.tobytes() == res.x.tobytes() and np.array_equal(again.root, res.root)
    assert again.vu.tobytes() == res.vu.tobytes() and again.counts == res.counts
    if kind == 'lin':
        assert c.roots.shape[0] == 22 and np.unique(res.root).size == 22
    # every point lies in the root it was drawn in, so in the set
    R = c.roots[res.root]
    beta = np.linalg.solve(np.transpose(R[:, 1:] - R[:, :1], (0, 2, 1)),
                           (res.x - R[:, 0])[:, :, None])[:, :, 0]
    assert min(beta.min(), (1. - beta.sum(axis=1)).min()) >= -1e-12
    assert not np.array_equal(law.audit(c.orc, n=8, seed=12, return_samples=True).x, res.x[:8])


@pytest.mark.parametrize('kind', ['lin', 'lin_quadratic', 'pwa_small'])
def test_a_sound_law_passes(cases, kind):
    """n = 2000 at the default tolerances (rtol = 1e-7, input_tol = 1e-7 max(1, U)).  V_u comes
    from the exact substitution wherever the input is admissible as it stands, so the relaxation
    does not lower it: with V_u from the relaxed problem throughout, 42 of 2000 samples of 'lin' and
    3 of 'pwa_small' were `negative` by up to 3.0 slacks."""
    c = cases(kind)
    res = c.compiled.audit(c.orc, n=2000, seed=2, return_samples=True)
    src = c.law.audit_applied(n=2000, seed=2, return_samples=True)
    print(kind, res, src)
    judged = res.status <= 2
    print(kind, 'smallest (V_u - V*) / slack %.3e' % np.min(
        ((res.vu - res.vstar) / (RTOL * (1. + np.abs(res.vstar))))[judged]))
    assert res.n == 2000 and sum(res.counts.values()) == 2000
    assert res.counts['inadmissible'] == 0 and res.counts['violation'] == 0
    assert res.passed, res
    assert src.counts == res.counts and src.passed
    assert res.n_relaxed == 0 and src.n_relaxed == 0


@pytest.mark.parametrize('kind', ['lin', 'lin_quadratic', 'pwa_small'])
def test_a_sound_law_passes_under_the_exact_substitution(cases, kind):
    """input_tol = 0 is the exact substitution, for which V_u >= V* holds in exact arithmetic and
    V_u <= Vbar by convexity: sound laws pass, the compiled law and its source alike."""
    c = cases(kind)
    res = c.compiled.audit(c.orc, n=2000, seed=2, input_tol=0., return_samples=True)
    src = c.law.audit_applied(n=2000, seed=2, input_tol=0., return_samples=True)
    print(kind, res, src)
    print(kind, 'seconds (sample, evaluate, pack + reduce, P_theta, applied)', res.seconds)
    assert res.n == 2000 and res.counts['within'] == 2000 and res.passed
    assert res.histogram.sum() == 2000 and res.max_ratio > 0.
    w = res.worst
    assert res.max_ratio <= 1. + RTOL * (1. + abs(w['vstar'])) / w['bound']
    assert src.counts == res.counts and src.passed
    # the source law at its own points: its evaluator's (u, leaf), the same judgement
    u, leaf, _, _ = c.law.evaluate(src.x, return_info=True)
    assert src.u.tobytes() == u.tobytes() and np.array_equal(src.leaf, leaf)
    assert src.x.tobytes() == c.law.sample(n=2000, seed=2)[0].tobytes()
    assert (src.root == -1).all()
    # the interpolated input costs no more than the interpolated vertex costs (convexity)
    vbar = c.law.audit(n=2000, seed=2, return_samples=True).vbar
    assert (src.vu <= vbar + RTOL * (1. + np.abs(vbar))).all()
    per_leaf = c.law.audit_applied(per_leaf=2, seed=2, input_tol=0.)
    assert per_leaf.n == 2 * c.law.cells()['node'].size and per_leaf.passed


def test_the_relaxation_admits_an_overshoot_and_lowers_no_admissible_cost(cases):
    """Half the inputs are u* (admissible as they stand), half have their first component moved
    1e-5 past the bound u_max = 1 (a thousand feasibility tolerances of the solver, 1e-8): with
    input_tol = 1e-4 the first keep the exact problem's V_u bit for bit, the second are judged
    on the relaxed problem where that admits them and stay inadmissible where it does not."""
    from explicit_hybrid_mpc_amd import applied, engine
    c = cases('lin')
    assert np.abs(c.orc.mpc.gu).max() == 1. and np.abs(c.orc.mpc.Gu).max() == 1.   # u_max = 1
    X, _ = c.law.sample(n=256, seed=31)
    J, U, didx = c.orc.gpu.solve_pt(X)
    assert (didx >= 0).all()
    U = U.copy()
    over = np.arange(256) % 2 == 1
    U[over, 0] = 1. + 1e-5
    exact = applied.audit_inputs(c.orc, X, U, input_tol=0., return_samples=True)
    res = applied.audit_inputs(c.orc, X, U, input_tol=1e-4, return_samples=True)
    print(exact, res)
    assert exact.n_relaxed == 0 and (exact.relaxed == 0).all()
    assert (exact.status[over] == 3).all() and (exact.status[~over] == 0).all()
    assert (res.relaxed[~over] == 0).all()
    assert res.vu[~over].tobytes() == exact.vu[~over].tobytes()
    assert np.array_equal(res.status[~over], exact.status[~over])
    took = res.relaxed == 1
    assert took.sum() == res.n_relaxed > 0 and (res.status[took] <= 2).all()
    assert (res.status[over & ~took] == 3).all() and (res.delta_idx_applied[over & ~took] < 0).all()
    red = applied.applied_input_problem(c.orc.gpu.can, 1e-4)
    theta, konst, _ = apc.pack(X, U, red.cost_u)
    wide = engine.GpuProblem(red, c.orc.eps_a, c.orc.eps_r)
    Jw, _, dw = wide.solve_pt(theta[over])
    wide.close()
    assert np.array_equal(dw >= 0, took[over])
    assert res.vu[took].tobytes() == (Jw + konst[over])[dw >= 0].tobytes()
    assert np.array_equal(res.delta_idx_applied[took], dw[dw >= 0])


def test_a_leaf_with_an_inadmissible_input_is_found(cases):
    """Leaf L of the 'lin' law set to the constant input 2 u_max (K = 0): the input rows of u_0
    read 0 <= 1 - 2 + input_tol for every commutation, so exactly the samples located in L are
    inadmissible; the others keep status and V_u bit for bit."""
    from explicit_hybrid_mpc_amd.compiled import CompiledLaw
    c = cases('lin')
    law = c.compiled
    p, n_u = law.p, law.n_u
    assert np.abs(c.orc.mpc.gu).max() == 1. and np.abs(c.orc.mpc.Gu).max() == 1.   # u_max = 1
    ref = law.audit(c.orc, n=N, seed=8, return_samples=True)
    assert ref.counts['inadmissible'] == 0
    node = int(np.bincount(ref.leaf).argmax())
    arrays = law.arrays()
    L = int(np.nonzero(arrays['leaf_node'] == node)[0][0])
    arrays['leaf_rec'][L, p:p + n_u] = 2.
    arrays['leaf_rec'][L, p + n_u:p + n_u + n_u * p] = 0.
    broken = CompiledLaw.from_arrays(arrays)
    res = broken.audit(c.orc, n=N, seed=8, return_samples=True, input_tol=ref.input_tol)
    hit = res.leaf == node
    assert np.array_equal(res.leaf, ref.leaf) and res.x.tobytes() == ref.x.tobytes()
    assert hit.sum() >= 10 and (res.u[hit] == 2.).all()
    assert (res.status[hit] == 3).all() and np.array_equal(res.status[~hit], ref.status[~hit])
    assert res.vu[~hit].tobytes() == ref.vu[~hit].tobytes()
    assert res.counts['inadmissible'] == hit.sum() and not res.passed
    # a leaf without a law: status 4
    st, _ = _statuses_of_inputs(c, res.x, np.where(hit[:, None], np.nan, res.u), ref.input_tol)
    assert (st[hit] == 4).all() and np.array_equal(st[~hit], ref.status[~hit])
    broken.close()

    # an oracle a thousand times tighter than the build's: violations, the mirror's count
    class Tight:
        gpu, mpc = c.orc.gpu, c.orc.mpc
        eps_a, eps_r = c.orc.eps_a / 1000., c.orc.eps_r / 1000.
    tight = law.audit(Tight, n=N, seed=8, return_samples=True)
    st, _ = _check_against_the_entry_points(law, Tight, tight, np.arange(N))
    print('tight oracle:', tight)
    assert tight.counts['violation'] == (st == 1).sum() > 0 and not tight.passed
    assert tight.vu.tobytes() == ref.vu.tobytes()


def _statuses_of_inputs(c, X, U, input_tol):
    from explicit_hybrid_mpc_amd import applied
    res = applied.audit_inputs(c.orc, X, U, input_tol=input_tol, return_samples=True)
    return res.status, res


@pytest.mark.parametrize('kind,flush', [('lin_quadratic', False), ('lin', True)])
def test_single_precision_laws_are_judged(cases, kind, flush):
    c = cases(kind)
    single = c.compiled.to_single(flush=flush)
    assert single.dtype is np.float32
    double = c.compiled.audit(c.orc, n=N, seed=5, return_samples=True)
    res = single.audit(c.orc, n=N, seed=5, return_samples=True)
    print(kind, 'single, flush' if flush else 'single', res, 'double:', double)
    assert res.x.tobytes() == double.x.tobytes() and np.array_equal(res.root, double.root)
    assert sum(res.counts.values()) == N
    _check_against_the_entry_points(single, c.orc, res, np.arange(N))
    # the float law's input is the double law's up to the rounding of a float
    same = res.leaf == double.leaf
    assert same.mean() > 0.99
    assert np.abs(res.u[same] - double.u[same]).max() <= 1e-4
    single.close()


def test_arguments(cases):
    from explicit_hybrid_mpc_amd import _capi, explicit, partition
    c = cases('di')
    law = c.compiled
    res = law.audit(c.orc, n=0, return_samples=True)
    assert res.passed and res.n == 0 and res.x.shape == (0, 2) and res.status.shape == (0,)
    assert sum(res.counts.values()) == 0 and res.worst is None and res.max_ratio == -np.inf
    with pytest.raises(ValueError):
        law.audit(c.orc)
    with pytest.raises(ValueError):
        law.audit(c.orc, n=4, X=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        law.audit(c.orc, X=np.zeros((4, 3)))
    with pytest.raises(ValueError):
        law.audit(c.orc, n=4, first=-1)
    with pytest.raises(ValueError):
        c.law.audit_applied(n=10, per_leaf=2)

    class NoBatch:                  # an oracle without the batched P_theta (bnb.PrefixOracle)
        eps_a, eps_r = c.orc.eps_a, c.orc.eps_r
    with pytest.raises(_capi.EhmError):
        law.audit(NoBatch(), n=10)
    with pytest.raises(_capi.EhmError):
        c.law.audit_applied(n=10, oracle=NoBatch())
    bare = explicit.ExplicitMPC(c.flat)
    with pytest.raises(ValueError):
        bare.audit_applied(n=10)
    assert bare.audit_applied(n=50, oracle=c.orc).n == 50
    bare.close()
    # an oracle of another law
    with pytest.raises(ValueError):
        law.audit(cases('lin').orc, n=10)
    # a law with test nodes has no root cells: refused, as for the rollout
    orc, V = _oracle('di')
    root, _ = partition.partition_set(orc, V)
    nested = explicit.ExplicitMPC(root, orc)
    with_tests = nested.compile()
    assert with_tests.stats['n_test'] > 0
    with pytest.raises(_capi.EhmError):
        with_tests.audit(orc, n=10)
    as_roots = nested.compile(spine='roots')
    assert as_roots.stats['n_test'] == 0 and as_roots.audit(orc, n=200).n == 200
    # the C entry point refuses what the Python layer would not send
    lib = _capi.load()
    opts = _capi.AppliedOpts(n=4, p=2, n_u=1)
    out = _capi.AppliedResult()
    assert lib.ehm_compiled_audit(None, None, None, opts, out, None) == _capi.EHM_E_INVALID
    gp = c.orc.gpu._handle
    assert lib.ehm_compiled_audit(None, gp, gp, opts, out, None) == _capi.EHM_E_INVALID
    assert b'cost_u' in lib.ehm_applied_last_error()
    cost = np.zeros(1)
    opts.cost_u = cost.ctypes.data
    assert lib.ehm_compiled_audit(None, gp, gp, opts, out, None) == _capi.EHM_E_INVALID
    assert b'no inputs' in lib.ehm_applied_last_error()
    assert lib.ehm_compiled_audit(with_tests._handle, gp, gp, opts, out, None) == \
        _capi.EHM_E_INVALID
    assert b'test nodes' in lib.ehm_applied_last_error()
    opts.p = 7
    opts.n_u = 2
    assert lib.ehm_compiled_audit(None, gp, gp, opts, out, None) == _capi.EHM_E_INVALID
    for l in (with_tests, as_roots):
        l.close()
    nested.close()
    orc.close()
    gone = c.law.compile()
    gone.close()
    with pytest.raises(ValueError):
        gone.audit(c.orc, n=10)
