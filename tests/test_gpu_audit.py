"""
The sampled audit of a law's epsilon-suboptimality (csrc/ehm_audit.hip) on the
device: the sampler and the cost kernel bit for bit against the numpy mirror (tests/audit_cpu.py),
V* against GpuProblem.solve_pt, sound partitions passing, and -- what shows that the audit
discriminates -- a leaf whose costs are off by a derivable amount found, and open leaves counted.

The trees are small (tens to hundreds of leaves), built once per module.
"""

import copy

import numpy as np
import pytest

from tests import audit_cpu as ac
from tests import helpers

pytestmark = pytest.mark.gpu

ABS_FRAC, REL_ERR = 0.3, 0.5
N_SAMPLER = 4096


def _oracle(kind):
    from explicit_hybrid_mpc_amd import examples
    from explicit_hybrid_mpc_amd.oracle import Oracle
    if kind in ('lin', 'lin_quadratic'):
        mpc = helpers.make_instance('lin', 0) if kind == 'lin' else \
            examples.linear_mpc(0, cost='quadratic')
        V = examples.box_vertices(examples.theta_box(mpc))
        return examples.create_oracle(mpc, V, abs_frac=ABS_FRAC, abs_err=None, rel_err=REL_ERR), V
    mpc = helpers.make_instance(kind, 0)
    V = examples.box_vertices(examples.theta_box(mpc))
    return Oracle(mpc, helpers.eps_a_rule(mpc, ABS_FRAC), REL_ERR), V


class _Case:
    def __init__(self, kind):
        from explicit_hybrid_mpc_amd import explicit, partition
        from explicit_hybrid_mpc_amd import tools as ehm_tools
        self.kind = kind
        self.orc, self.V = _oracle(kind)
        roots, _ = ehm_tools.delaunay_roots(self.V)
        self.roots = np.array(roots)
        self.flat = partition.run_engine(self.orc, self.roots, action='ecc')
        self.law = explicit.ExplicitMPC(self.flat, self.orc)

    def close(self):
        self.law.close()
        self.orc.close()


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Case(kind)
        return made[kind]
    yield get
    for c in made.values():
        c.close()


def _per_leaf_k(law, n):
    return n // law.cells()['node'].size + 1


@pytest.mark.parametrize('mode', ['uniform', 'per_leaf'])
@pytest.mark.parametrize('kind', ['di', 'lin'])
def test_sampler_is_bit_equal_to_the_mirror(cases, kind, mode):
    c = cases(kind)
    law, flat = c.law, c.flat
    cells = law.cells()
    leaves = np.nonzero(flat.left < 0)[0]
    assert np.array_equal(cells['node'], leaves)
    if kind == 'di':
        assert law.p == 2 and 4 <= leaves.size <= 400      # (6 leaves at these tolerances)
    else:
        assert law.p == 4 and law.n_u == 2 and leaves.size >= 200
    k = _per_leaf_k(law, N_SAMPLER) if mode == 'per_leaf' else None
    X, cell = law.sample(n=N_SAMPLER, seed=11, mode=mode, per_leaf=k)
    Xm, cm = ac.sample(cells['vertices'], cells['cdf'], np.arange(N_SAMPLER), 11,
                       ac.PER_LEAF if mode == 'per_leaf' else ac.UNIFORM, k or 0)
    assert cell.dtype == np.int32 and np.array_equal(cell, cm)
    assert X.tobytes() == Xm.tobytes()
    if mode == 'per_leaf':
        assert np.array_equal(cell, np.arange(N_SAMPLER) // k)
    else:
        assert np.unique(cell).size > 2
    # every point lies in its cell
    R = cells['vertices'][cell]
    beta = np.linalg.solve(np.transpose(R[:, 1:] - R[:, :1], (0, 2, 1)),
                           (X - R[:, 0])[:, :, None])[:, :, 0]
    assert min(beta.min(), (1. - beta.sum(axis=1)).min()) >= -1e-12
    # neither the chunk size nor a split of the ids changes a point
    Xc, cc = law.sample(n=N_SAMPLER, seed=11, mode=mode, per_leaf=k, chunk=1000)
    assert Xc.tobytes() == X.tobytes() and np.array_equal(cc, cell)
    Xs, cs = law.sample(n=96, seed=11, mode=mode, per_leaf=k, first=1000)
    assert Xs.tobytes() == X[1000:1096].tobytes() and np.array_equal(cs, cell[1000:1096])
    # another seed, other points
    assert not np.array_equal(law.sample(n=8, seed=12, mode=mode, per_leaf=k)[0], X[:8])


@pytest.mark.parametrize('mode', ['uniform', 'per_leaf'])
@pytest.mark.parametrize('kind', ['di', 'lin'])
def test_cost_kernel_prices_the_law_as_deployed(cases, kind, mode):
    from tests.test_gpu_explicit import _interpolated_cost
    c = cases(kind)
    law, flat = c.law, c.flat
    k = _per_leaf_k(law, N_SAMPLER) if mode == 'per_leaf' else None
    X, cell = law.sample(n=N_SAMPLER, seed=11, mode=mode, per_leaf=k)
    if mode == 'per_leaf':
        res = law.audit(per_leaf=k, seed=11, return_samples=True)
        assert res.n == k * law.cells()['node'].size
    else:
        res = law.audit(n=N_SAMPLER, seed=11, return_samples=True)
    n = N_SAMPLER
    assert res.x[:n].tobytes() == X.tobytes() and np.array_equal(res.cell[:n], cell)
    _, leaf, _, _ = law.evaluate(res.x, return_info=True)
    assert np.array_equal(res.leaf, leaf)
    vbar, wmin = ac.interpolated_cost(law.records(), flat.vertex_costs, res.leaf, res.x)
    assert res.vbar.tobytes() == vbar.tobytes()
    assert res.wmin.tobytes() == wmin.tobytes()
    ref, _ = _interpolated_cost(flat, res.leaf, res.x)
    assert (np.abs(res.vbar - ref) <= 1e-10 * (1. + np.abs(ref))).all()


@pytest.mark.parametrize('kind', ['lin', 'lin_quadratic', 'pwa_small'])
def test_vstar_is_the_batched_p_theta_bit_for_bit(cases, kind):
    c = cases(kind)
    res = c.law.audit(n=N_SAMPLER, seed=5, return_samples=True, chunk=1500)
    J, _, didx = c.orc.gpu.solve_pt(res.x)
    assert res.vstar.tobytes() == J.tobytes()
    assert np.array_equal(res.delta_idx, didx)
    if kind == 'pwa_small':
        assert c.orc.gpu.can.n_delta == 8 and np.unique(didx).size > 1
    # the statuses and the summary are the mirror's on these arrays
    closed = (c.flat.flags[res.leaf] & 1).astype(bool)
    st, ratio = ac.statuses(res.vbar, res.vstar, closed, res.delta_idx, c.orc.eps_a, c.orc.eps_r,
                            1e-7)
    assert np.array_equal(res.status, st)
    counts, hist, best, worst = ac.summary(np.arange(N_SAMPLER), st, ratio)
    assert [res.counts[name] for name in
            ('within', 'violation', 'negative', 'open', 'infeasible')] == counts.tolist()
    assert np.array_equal(res.histogram, hist)
    assert res.max_ratio == best and res.worst['id'] == worst
    w = res.worst
    assert w['leaf'] == res.leaf[worst] and w['cell'] == res.cell[worst]
    assert w['vbar'] == res.vbar[worst] and w['vstar'] == res.vstar[worst]
    assert np.array_equal(w['x'], res.x[worst])
    assert w['bound'] == max(c.orc.eps_a, c.orc.eps_r * res.vstar[worst])
    # the chunk size changes nothing that is reported
    one = c.law.audit(n=N_SAMPLER, seed=5)
    assert one.counts == res.counts and np.array_equal(one.histogram, res.histogram)
    assert one.max_ratio == res.max_ratio and one.worst['id'] == res.worst['id']
    assert one.relocated == res.relocated and one.x is None


@pytest.mark.parametrize('mode', ['uniform', 'per_leaf'])
@pytest.mark.parametrize('kind', ['lin', 'lin_quadratic', 'pwa_small'])
def test_a_sound_partition_passes(cases, kind, mode):
    c = cases(kind)
    rtol = 1e-7
    if mode == 'uniform':
        res = c.law.audit(n=20000, seed=2, return_samples=True)
        assert res.n == 20000
    else:
        res = c.law.audit(per_leaf=4, seed=2, return_samples=True)
        assert res.n == 4 * c.law.cells()['node'].size
        assert np.array_equal(res.cell, np.arange(res.n) // 4)
    print(kind, mode, res, 'smallest weight %.3e' % res.wmin.min())
    assert res.passed, res
    assert res.counts['within'] == res.n and sum(res.counts.values()) == res.n
    assert res.histogram.sum() == res.n and res.histogram[32] <= res.n
    w = res.worst
    assert res.max_ratio <= 1. + rtol * (1. + abs(w['vstar'])) / w['bound']
    assert res.max_ratio > 0.
    assert res.open_volume_fraction == 0.
    # samples are interior to their cells almost surely, and for this seed they are: the smallest
    # spacing drawn is 6.9e-6 (1.1e-5 per leaf on 'lin', 1.9e-3 on 'pwa_small'), far above the
    # 1e-9 within which a face may hand a point to the neighbour -- the deployed walk must find
    # every sample's own cell
    assert res.wmin.min() > 1e-9
    assert res.relocated == 0
    assert np.array_equal(res.leaf, c.law.cells()['node'][res.cell])


def _with_costs(case, vertex_costs):
    from explicit_hybrid_mpc_amd import explicit
    flat = copy.copy(case.flat)
    flat.vertex_costs = vertex_costs
    return explicit.ExplicitMPC(flat, case.orc)


@pytest.mark.parametrize('kind', ['lin', 'pwa_small'])
def test_a_broken_leaf_is_found(cases, kind):
    """Leaf L's vertex costs raised by 3 B, B = max(eps_a, eps_r max vertex cost of L): since
    V* <= Vbar <= max vertex cost on L, B >= bound(x) there, so Vbar - V* >= 3 B > bound + slack at
    every point of L -- status 1 exactly on the samples located in L; lowered by 3 B instead,
    Vbar - V* <= bound - 3 B <= -2 B < -slack: status 2 on the same samples."""
    c = cases(kind)
    flat = c.flat
    closed_leaves = np.nonzero((flat.left < 0) & ((flat.flags & 1) != 0))[0]
    L = int(closed_leaves[closed_leaves.size // 2])
    B = max(c.orc.eps_a, c.orc.eps_r * float(np.max(flat.vertex_costs[L])))
    assert B > 1e-3
    for sign, status, name in ((+1., 1, 'violation'), (-1., 2, 'negative')):
        costs = np.array(flat.vertex_costs)
        costs[L] += sign * 3. * B
        law = _with_costs(c, costs)
        res = law.audit(per_leaf=4, seed=3, return_samples=True)
        law.close()
        hit = res.leaf == L
        assert hit.sum() >= 1
        assert (res.status[hit] == status).all() and (res.status[~hit] == 0).all()
        assert res.counts[name] == hit.sum() and not res.passed
        assert res.counts['within'] == res.n - hit.sum()
        if sign > 0:
            assert res.worst['leaf'] == L and res.max_ratio >= 3.
            assert res.histogram[32] >= hit.sum()
        else:
            assert res.worst['leaf'] != L and res.histogram[0] >= hit.sum()


def test_a_nan_ratio_is_binned_and_never_the_worst(cases):
    """Leaf L_nan (cell 0) has NaN vertex costs, leaf L_bad (cell 30) is raised by 3 B as in
    test_a_broken_leaf_is_found.  With 4 samples per leaf, sample 0 -- slot 0 of the first
    256-sample workgroup, which also holds L_bad's samples 120 .. 123 -- has a NaN ratio: it is
    status 2 and counted in bin 0, and the worst sample is the mirror's (np.nanmax, the smallest
    id), a sample of L_bad, whatever the chunk."""
    c = cases('lin')
    flat = c.flat
    node = c.law.cells()['node']
    assert node.size >= 64 and (flat.flags[node[[0, 30]]] & 1).all()
    L_nan, L_bad = int(node[0]), int(node[30])
    B = max(c.orc.eps_a, c.orc.eps_r * float(np.max(flat.vertex_costs[L_bad])))
    costs = np.array(flat.vertex_costs)
    costs[L_nan] = np.nan
    costs[L_bad] += 3. * B
    law = _with_costs(c, costs)
    runs = [law.audit(per_leaf=4, seed=3, return_samples=True, chunk=chunk)
            for chunk in (0, 256, 100)]
    law.close()
    res = runs[0]
    print('samples', res.n, 'worst', res.worst['id'], res.worst['leaf'], res.max_ratio)
    nan = res.leaf == L_nan
    assert res.cell[0] == 0 and nan[0] and np.isnan(res.vbar[nan]).all()
    assert (res.status[nan] == 2).all() and res.counts['negative'] == nan.sum()
    closed = (flat.flags[res.leaf] & 1).astype(bool)
    st, ratio = ac.statuses(res.vbar, res.vstar, closed, res.delta_idx, c.orc.eps_a, c.orc.eps_r,
                            1e-7)
    assert np.array_equal(res.status, st) and np.isnan(ratio[nan]).all()
    counts, hist, best, worst = ac.summary(np.arange(res.n), st, ratio)
    assert np.array_equal(res.histogram, hist)
    # bin 0 holds the NaN ratios
    assert res.histogram[0] >= nan.sum()
    assert res.worst['id'] == worst and res.max_ratio == best and best >= 3.
    assert res.worst['leaf'] == res.leaf[worst] == L_bad
    for other in runs[1:]:
        assert other.counts == res.counts and np.array_equal(other.histogram, res.histogram)
        assert other.worst['id'] == res.worst['id'] and other.max_ratio == res.max_ratio
        assert other.worst['leaf'] == res.worst['leaf']
        assert np.array_equal(other.status, res.status)


def test_open_leaves_are_counted_not_passed(cases):
    from explicit_hybrid_mpc_amd import engine, explicit, partition
    c = cases('lin')
    depth = int(c.flat.info['max_depth'])
    assert depth >= 4
    flat = partition.run_engine(c.orc, c.roots, action='ecc', max_depth=depth - 2)
    leaves = np.nonzero(flat.left < 0)[0]
    is_open = (flat.flags[leaves] & 1) == 0
    assert 0 < is_open.sum() < leaves.size
    law = explicit.ExplicitMPC(flat, c.orc)
    res = law.audit(n=8000, seed=4, return_samples=True)
    located_open = (flat.flags[res.leaf] & 1) == 0
    assert res.counts['open'] == located_open.sum() > 0
    assert (res.status[located_open] == 3).all() and (res.status[~located_open] != 3).all()
    assert not res.passed
    lenient = law.audit(n=8000, seed=4, allow_open=True)
    assert lenient.counts == res.counts
    assert lenient.passed == (res.counts['violation'] + res.counts['negative'] +
                              res.counts['infeasible'] == 0)
    assert lenient.passed
    vol = engine.volume_batch(flat.vertices[leaves])
    assert abs(res.open_volume_fraction - vol[is_open].sum() / vol.sum()) <= 1e-12
    # the sampled share of open volume agrees with the exact one (binomial, 6 sigma)
    f = res.open_volume_fraction
    assert abs(res.counts['open'] / res.n - f) <= 6. * np.sqrt(f * (1. - f) / res.n) + 1e-3
    law.close()


def test_nested_tree_and_flat_forest_of_one_partition_agree():
    from explicit_hybrid_mpc_amd import explicit, partition
    orc, V = _oracle('lin')
    root, flat = partition.partition_set(orc, V)
    nested = explicit.ExplicitMPC(root, orc)
    forest = explicit.ExplicitMPC(flat, orc)
    cn, cf = nested.cells(), forest.cells()
    assert np.array_equal(cn['vertices'], cf['vertices'])
    assert np.array_equal(cn['closed'], cf['closed'])
    for kw in (dict(n=5000), dict(per_leaf=2)):
        a = nested.audit(seed=6, return_samples=True, **kw)
        b = forest.audit(seed=6, return_samples=True, **kw)
        assert a.x.tobytes() == b.x.tobytes() and np.array_equal(a.cell, b.cell)
        assert a.vbar.tobytes() == b.vbar.tobytes()
        assert np.array_equal(a.status, b.status)
        assert a.counts == b.counts and a.passed and b.passed
        assert np.array_equal(a.histogram, b.histogram) and a.max_ratio == b.max_ratio
        # the located leaves are the same simplices under the two numberings
        assert np.array_equal(cn['node'][a.cell] == a.leaf, cf['node'][b.cell] == b.leaf)
        for q in range(0, a.n, 211):
            assert np.array_equal(nested.nodes[a.leaf[q]].data.vertices, flat.vertices[b.leaf[q]])
    Xn, _ = nested.sample(n=64, seed=1)
    Xf, _ = forest.sample(n=64, seed=1)
    assert Xn.tobytes() == Xf.tobytes()
    nested.close()
    forest.close()
    orc.close()


def test_arguments(cases):
    from explicit_hybrid_mpc_amd import _capi, explicit
    c = cases('di')
    law = c.law
    res = law.audit(n=0, return_samples=True)
    assert res.passed and res.n == 0 and res.x.shape == (0, 2) and res.status.shape == (0,)
    assert sum(res.counts.values()) == 0 and res.worst is None and res.max_ratio == -np.inf
    X, cell = law.sample(n=0)
    assert X.shape == (0, 2) and cell.shape == (0,)
    with pytest.raises(ValueError):
        law.audit(n=10, mode='stratified')
    with pytest.raises(ValueError):
        law.sample(n=10, mode='stratified')
    with pytest.raises(ValueError):
        law.audit(n=10, per_leaf=2)
    with pytest.raises(ValueError):
        law.audit(mode='per_leaf')
    with pytest.raises(ValueError):
        law.audit()
    with pytest.raises(ValueError):
        law.sample(per_leaf=2, first=2 * law.cells()['node'].size + 1)
    bare = explicit.ExplicitMPC(c.flat)
    with pytest.raises(ValueError):
        bare.audit(n=10)
    # ... but an oracle may be passed, and sampling needs none
    assert bare.audit(n=200, oracle=c.orc).passed
    assert bare.sample(n=5, seed=11)[0].tobytes() == law.sample(n=5, seed=11)[0].tobytes()

    class NoBatch:                  # an oracle without the batched P_theta (bnb.PrefixOracle)
        eps_a, eps_r = c.orc.eps_a, c.orc.eps_r
    with pytest.raises(_capi.EhmError):
        bare.audit(n=10, oracle=NoBatch())
    bare.close()
    with pytest.raises(ValueError):
        bare.audit(n=10, oracle=c.orc)
    with pytest.raises(ValueError):
        bare.sample(n=10)
    # the C entry points refuse what the Python layer would not send
    lib = _capi.load()
    opts = _capi.AuditOpts(mode=7, n=4)
    assert lib.ehm_explicit_sample(law._handle, opts, None, None) == _capi.EHM_E_INVALID
    assert b'mode' in lib.ehm_explicit_last_error()
    assert lib.ehm_explicit_audit(None, None, opts, None, None) == _capi.EHM_E_INVALID
