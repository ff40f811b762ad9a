"""
The leaf cells of a compiled law on the device (csrc/ehm_certify.hip, certify.py)
against the numpy mirror (tests/certify_cpu.py), bit for bit, and against the vertices of the
partitions the laws were compiled from.
"""

import numpy as np
import pytest

from tests import certify_cpu as zc
from tests import compiled_cpu as cc
from tests import explicit_synth as es
from tests.test_host_certify import C_ROOT, EPS, root_of

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def _mirror(arrays, leaves=None):
    n_leaf = zc.header(arrays)['n_leaf']
    leaves = np.arange(n_leaf) if leaves is None else np.asarray(leaves)
    V, status = zc.cells(arrays, leaves)
    return V, zc.vertex_inputs(arrays, leaves, V, status), status


def _check(law, arrays=None, leaves=None):
    """``law.cells(leaves)`` against the mirror on the law's own exported arrays."""
    arrays = law.arrays() if arrays is None else arrays
    got = law.cells(leaves)
    V, U, status = _mirror(arrays, leaves)
    assert np.array_equal(got.status, status) and got.status.dtype == np.int32
    # NaN rows compare by their bytes too: both sides write the same quiet NaN
    assert np.array_equal(got.vertices, V, equal_nan=True)
    assert np.array_equal(got.inputs, U, equal_nan=True)
    live = status == zc.CELL
    _same(got.vertices[live], V[live])
    _same(got.inputs[live], U[live])
    ids = np.arange(status.size) if leaves is None else np.asarray(leaves)
    assert np.array_equal(got.leaves, ids)
    assert np.array_equal(got.leaf_node, arrays['leaf_node'][ids])
    return got


# p = 2, 3: the 64-byte record (32 in single), 7: the 128-byte one (64 in single)
@pytest.mark.parametrize('p,n_u', [(2, 1), (3, 2), (7, 1), (7, 2)])
def test_cells_are_the_mirrors_bit_for_bit(p, n_u, tmp_path):
    from explicit_hybrid_mpc_amd import _capi, applied, compiled
    rng = np.random.default_rng([81, p, n_u])
    synth = es.SynthLaw(es.kuhn_forest(p, 100), n_u, 2, rng, n_sub=12)
    ex = synth.explicit()
    law = ex.compile()
    ex.close()
    arrays = law.arrays()
    n_leaf = zc.header(arrays)['n_leaf']
    assert n_leaf > 256                                         # more than one block of 64
    assert np.array_equal(applied.root_cells(law)['vertices'], zc.root_vertices(arrays))
    full = _check(law, arrays)
    assert (full.status == zc.CELL).all() and full.counts == {'cell': n_leaf, 'no_cell': 0}
    # Kuhn roots are dyadic: the recovery is exact, and so are the midpoints below them
    _same(full.vertices, synth.vertices[arrays['leaf_node']])
    # a subset, in the caller's order and with a leaf named twice, is the rows of the full call
    pick = np.concatenate([rng.permutation(n_leaf)[:77], [0, n_leaf - 1, 0]]).astype(np.int64)
    part = _check(law, arrays, pick)
    _same(part.vertices, full.vertices[pick])
    _same(part.inputs, full.inputs[pick])
    none = law.cells(np.zeros(0, dtype=np.int32))
    assert len(none) == 0 and none.vertices.shape == (0, p + 1, p)
    for bad in ([-1], [n_leaf], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            law.cells(bad)
    # the same law after save / load
    path = str(tmp_path / 'law.npz')
    law.save(path)
    loaded = compiled.CompiledLaw.load(path)
    again = loaded.cells()
    _same(again.vertices, full.vertices)
    _same(again.inputs, full.inputs)
    loaded.close()
    # its single form: the float planes choose the same vertices wherever their rounding leaves the
    # choice certain (tests/test_host_certify.py), the inputs are the float map's
    single = law.to_single(flush=True)
    a32 = single.arrays()
    s32 = _check(single, a32)
    live = s32.status == zc.CELL
    assert live.sum() >= 0.8 * n_leaf
    _same(s32.vertices[live], full.vertices[live])
    assert not np.array_equal(s32.inputs[live], full.inputs[live])
    scale = np.abs(a32['leaf_rec']).max() * (p + 1)
    ordinary = ~np.isin(arrays['leaf_node'], _sliver_nodes(synth))
    assert (np.abs(s32.inputs - full.inputs)[live & ordinary] <= 1e-3 * scale).all()
    single.save(path)
    loaded = compiled.CompiledLaw.load(path)
    again = loaded.cells(pick)
    assert np.array_equal(again.vertices, s32.vertices[pick], equal_nan=True)
    assert np.array_equal(again.inputs, s32.inputs[pick], equal_nan=True)
    loaded.close()
    single.close()
    # the C entry point refuses what the Python layer would not send
    lib = _capi.load()
    roots = zc.root_vertices(arrays)
    V = np.empty((2, p + 1, p))
    st = np.empty(2, dtype=np.int32)
    ids = np.array([0, n_leaf], dtype=np.int32)
    call = lambda n, i: lib.ehm_compiled_cells(law._handle, roots.ctypes.data, n, i,
                                               V.ctypes.data, None, st.ctypes.data)
    assert call(2, ids.ctypes.data) == _capi.EHM_E_INVALID
    assert b'leaf_ids[1]' in lib.ehm_certify_last_error()
    assert call(n_leaf + 1, None) == _capi.EHM_E_INVALID
    assert call(-1, None) == _capi.EHM_E_INVALID
    assert lib.ehm_compiled_cells(None, roots.ctypes.data, 2, None, V.ctypes.data, None,
                                  st.ctypes.data) == _capi.EHM_E_INVALID
    assert call(2, None) == _capi.EHM_OK                    # no inputs asked for
    _same(V, full.vertices[:2])
    law.close()


def _sliver_nodes(synth):
    """Every node below the first bisection of a sliver chain (their ends are sliver_leaves)."""
    out = set()
    for k in synth.sliver_leaves:
        while synth.parent[k] >= 0:
            out.add(int(k))
            k = int(synth.parent[k])
    return np.array(sorted(out))


def test_no_cell_on_exactly_the_leaves_concerned():
    """A node that does not bisect the cell that reaches it and a chain deeper than the 256 turns
    kept: ``no_cell`` there, every other leaf keeps its cell."""
    from explicit_hybrid_mpc_amd import compiled
    from tests.test_host_certify import split_tree
    flat, _ = split_tree(3, 2, 1, n_split=60, sliver=30)
    arrays, _ = cc.compile_flat(flat)
    h = zc.header(arrays)
    good = compiled.CompiledLaw.from_arrays(arrays)
    want = _check(good, arrays)
    assert (want.status == zc.CELL).all()
    good.close()
    broken = {k: np.array(v, copy=True) for k, v in arrays.items()}
    bad = h['n_int'] // 2
    broken['node'][bad, :h['p'] + 1] *= 0.25
    law = compiled.CompiledLaw.from_arrays(broken)
    got = _check(law, broken)
    assert 0 < (got.status == zc.NO_CELL).sum() < h['n_leaf'] // 2
    live = got.status == zc.CELL
    _same(got.vertices[live], want.vertices[live])
    law.close()
    # 300 levels: the 44 side leaves below level 256 and the chain's end have no cell
    chain = zc.chain_tree(2, 300)
    deep, _ = cc.compile_flat(chain)
    law = compiled.CompiledLaw.from_arrays(deep)
    got = _check(law, deep)
    assert got.counts == {'cell': 256, 'no_cell': 45}
    live = got.status == zc.CELL
    _same(got.vertices[live], chain.vertices[deep['leaf_node']][live])
    law.close()


@pytest.mark.parametrize('kind', ['di', 'lin'])
def test_cells_of_a_partition_are_its_leaves(kind):
    """A law compiled from a partition the engine made: from the exact roots the cells are the
    partition's vertices bit for bit (the midpoint is ehm_split_batch's expression), from the
    recovered roots within the recovery bound, and the leaf's map gives back the vertex inputs."""
    from explicit_hybrid_mpc_amd import _capi, explicit, partition
    from tests.test_gpu_audit import _Case, _oracle
    c = _Case(kind)
    flat = c.flat
    law = c.law.compile()
    arrays = law.arrays()
    got = _check(law, arrays)
    assert (got.status == zc.CELL).all()
    p, n_roots = law.p, flat.info['n_roots']
    src = flat.vertices[got.leaf_node]
    R = flat.vertices[root_of(flat)[got.leaf_node]]
    kappa = np.linalg.cond(np.transpose(R[:, 1:] - R[:, :1], (0, 2, 1)))
    bound = C_ROOT * p * kappa * EPS * np.abs(R).max(axis=(1, 2))
    assert (np.abs(got.vertices - src).max(axis=(1, 2)) <= bound).all()
    exact = np.ascontiguousarray(flat.vertices[:n_roots], dtype=np.float64)
    V = np.empty_like(got.vertices)
    st = np.empty(len(got), dtype=np.int32)
    lib = _capi.load()
    assert lib.ehm_compiled_cells(law._handle, exact.ctypes.data, len(got), None, V.ctypes.data,
                                  None, st.ctypes.data) == _capi.EHM_OK
    assert (st == zc.CELL).all()
    _same(V, src)
    usrc = flat.vertex_inputs[got.leaf_node]
    kleaf = np.linalg.cond(np.transpose(src[:, 1:] - src[:, :1], (0, 2, 1)))
    tol = 32. * p * kleaf * EPS * max(1., np.abs(usrc).max()) + bound.max() * \
        np.abs(arrays['leaf_rec']).max() * p
    assert (np.abs(got.inputs - usrc).max(axis=(1, 2)) <= tol).all()
    law.close()
    c.close()
    if kind != 'di':
        return
    # a nested tree: its spine as test nodes is refused, as the root table it has cells
    orc, Vs = _oracle('di')
    root, _ = partition.partition_set(orc, Vs)
    nested = explicit.ExplicitMPC(root, orc)
    with_tests = nested.compile()
    assert with_tests.stats['n_test'] > 0
    with pytest.raises(_capi.EhmError) as err:
        with_tests.cells()
    assert err.value.code == _capi.EHM_E_INVALID and 'test nodes' in str(err.value)
    roots = np.zeros((with_tests.stats['n_roots'], 3, 2))
    one = np.empty((1, 3, 2))
    st = np.empty(1, dtype=np.int32)
    assert lib.ehm_compiled_cells(with_tests._handle, roots.ctypes.data, 1, None,
                                  one.ctypes.data, None, st.ctypes.data) == _capi.EHM_E_INVALID
    assert b'test nodes' in lib.ehm_certify_last_error()
    as_roots = nested.compile(spine='roots')
    got = _check(as_roots)
    assert (got.status == zc.CELL).all()
    for l in (with_tests, as_roots):
        l.close()
    nested.close()
    orc.close()


# ---- the certificate (CompiledLaw.certify, ehm_compiled_certify) ---------------------------------

KINDS = ['lin', 'lin_quadratic', 'pwa_small']
ARRAYS = ('status', 'delta_idx', 'tbest', 'tries', 'relaxed', 'n_candidates', 'volume', 'W')


class _Certified:
    """A partition of test_gpu_audit, its compiled law, and an oracle at twice its tolerances."""

    def __init__(self, kind):
        from explicit_hybrid_mpc_amd import explicit, partition
        from explicit_hybrid_mpc_amd.oracle import Oracle
        from tests.test_gpu_audit import _Case
        self.case = _Case(kind)
        self.orc, self.flat, self.source = self.case.orc, self.case.flat, self.case.law
        if kind == 'lin_quadratic':
            # the quadratic cost vanishes at the origin, where only eps_a closes a leaf: four times
            # the absolute tolerance of test_gpu_audit keeps the partition at a few hundred leaves
            self.orc = Oracle(self.orc.mpc, 4. * self.orc.eps_a, self.orc.eps_r)
            self.flat = partition.run_engine(self.orc, self.case.roots, action='ecc')
            self.source = explicit.ExplicitMPC(self.flat, self.orc)
        self.law = self.source.compile()
        self.loose = Oracle(self.orc.mpc, 2. * self.orc.eps_a, 2. * self.orc.eps_r)
        self.tight = Oracle(self.orc.mpc, self.orc.eps_a / 50., self.orc.eps_r / 50.)

    def close(self):
        self.law.close()
        self.loose.close()
        self.tight.close()
        if self.source is not self.case.law:
            self.source.close()
            self.orc.close()
        self.case.close()


@pytest.fixture(scope='module')
def certified():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _Certified(kind)
        return made[kind]
    yield get
    for c in made.values():
        c.close()


def _mirror_certificate(law, orc, res, max_tries):
    """The mirror fed the batched oracles through ``GpuProblem``, on the device's own cells."""
    from explicit_hybrid_mpc_amd import applied, engine
    ap = applied.applied_gpu(orc, 0.)
    rl = applied.applied_gpu(orc, res.input_tol) if res.input_tol > 0. else None
    cells = law.cells(res.leaves)
    assert np.array_equal(cells.vertices, res.vertices, equal_nan=True)
    assert np.array_equal(cells.inputs, res.inputs, equal_nan=True)
    return zc.certify(cells.vertices, cells.inputs, cells.status, ap.can.cost_u,
                      int(orc.gpu.can.n_delta), ap.point_idx,
                      None if rl is None else rl.point_idx, orc.gpu.bar_e,
                      lambda R: engine.volume_batch(R, device=law.device), max_tries)


def _same_leaves(a, b):
    for k in ARRAYS + ('vertices', 'inputs'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), k
    assert a.counts == b.counts and a.worst == b.worst and a.n_relaxed == b.n_relaxed
    assert a.certified_volume_fraction == b.certified_volume_fraction
    assert a.cell_volume_fraction == b.cell_volume_fraction


@pytest.mark.parametrize('kind', KINDS)
def test_the_pipeline_is_its_parts(certified, kind):
    """Every per-leaf array is what the mirror gives from ``point_idx`` and ``bar_e`` called from
    Python; chunked, and on a subset of the leaves, the same bit for bit."""
    from explicit_hybrid_mpc_amd import applied, certify
    c = certified(kind)
    law, orc = c.law, c.orc
    n_leaf = law.stats['n_leaf']
    assert 10 <= n_leaf <= 1000
    res = law.certify(orc, max_tries=3, return_leaves=True)
    want = _mirror_certificate(law, orc, res, 3)
    for k in ARRAYS:
        got = getattr(res, k)
        assert np.array_equal(got, want[k], equal_nan=got.dtype.kind == 'f'), k
    names = certify.STATUS_NAMES
    assert res.counts == {name: int((want['status'] == k).sum()) for k, name in enumerate(names)}
    assert sum(res.counts.values()) == res.n == n_leaf
    total = applied.root_cells(law)['volume'].sum()
    assert res.certified_volume_fraction == want['certified_volume'] / total
    assert abs(res.cell_volume_fraction - 1.) <= 1e-12
    if want['worst'] is None:
        assert res.worst is None
    else:
        assert (res.worst['leaf'], res.worst['tbest']) == want['worst']
        assert res.worst['leaf_node'] == law.leaf_node[res.worst['leaf']]
    assert res.passed == (res.counts['certified'] == n_leaf - res.counts['no_law'])
    print(kind, res, res.seconds)
    chunked = law.certify(orc, max_tries=3, return_leaves=True, chunk=37)
    _same_leaves(chunked, res)
    pick = np.random.default_rng(3).permutation(n_leaf)[:50]
    part = law.certify(orc, leaves=pick, max_tries=3, return_leaves=True, chunk=16)
    for k in ARRAYS + ('vertices', 'inputs'):
        assert np.array_equal(getattr(part, k), getattr(res, k)[pick], equal_nan=True), k
    assert np.array_equal(part.leaves, pick) and part.n == pick.size
    # one try only: a prefix of the tries above
    once = law.certify(orc, max_tries=1, return_leaves=True)
    assert (once.tries <= 1).all() and np.array_equal(once.tries == 1, res.tries >= 1)
    first = (res.tries == 1) & (res.status == 0)
    assert np.array_equal(once.status == 0, first)
    bare = law.certify(orc, max_tries=3)
    assert bare.counts == res.counts and bare.status is None
    # an oracle fifty times tighter than the build's: leaves stay open, every candidate is tried
    tight = law.certify(c.tight, max_tries=3, return_leaves=True, chunk=64)
    want = _mirror_certificate(law, c.tight, tight, 3)
    for k in ARRAYS:
        got = getattr(tight, k)
        assert np.array_equal(got, want[k], equal_nan=got.dtype.kind == 'f'), k
    print(kind, 'tight:', tight, 'candidates up to', tight.n_candidates.max())
    stay = tight.status == 1
    assert stay.sum() > 0 and not tight.passed
    assert np.array_equal(tight.tries[stay], np.minimum(tight.n_candidates[stay], 3))
    assert (tight.tbest[stay] >= 0.).all() and (tight.delta_idx[stay] == -1).all()
    assert tight.worst['tbest'] == tight.tbest[stay].max()
    assert tight.worst['leaf'] == np.nonzero(stay & (tight.tbest == tight.worst['tbest']))[0][0]


@pytest.mark.parametrize('kind', KINDS)
def test_every_leaf_the_partition_closed_is_certified(certified, kind):
    """Partitioned at (eps_a, eps_r), certified at (2 eps_a, 2 eps_r) with every candidate tried:
    the leaf's own commutation is a candidate, its W the vertex costs up to solver tolerance, and
    the factor 2 covers that -- so every closed leaf is certified."""
    from explicit_hybrid_mpc_amd import explicit, partition
    c = certified(kind)
    res = c.law.certify(c.loose, max_tries=0, return_leaves=True)
    closed = (c.flat.flags[res.leaf_node] & 1) == 1
    assert closed.all()
    print(kind, res)
    assert (res.status == 0).all() and res.passed
    assert abs(res.certified_volume_fraction - 1.) <= 1e-12 and res.worst is None
    assert (res.delta_idx >= 0).all() and (res.tbest < 0.).all()
    via = c.source.certify_applied(oracle=c.loose, max_tries=0)
    assert via.counts == res.counts
    if kind != 'pwa_small':
        return
    # cut two levels short: the open leaves without data have no law, the closed ones a certificate
    depth = int(c.flat.info['max_depth'])
    flat = partition.run_engine(c.orc, c.case.roots, action='ecc', max_depth=depth - 2)
    src = explicit.ExplicitMPC(flat, c.orc)
    law = src.compile()
    src.close()
    cut = law.certify(c.loose, max_tries=0, return_leaves=True)
    is_closed = (flat.flags[cut.leaf_node] & 1) == 1
    no_data = ~np.isfinite(flat.vertex_inputs[cut.leaf_node]).all(axis=(1, 2))
    assert 0 < (~is_closed).sum() < is_closed.size
    assert (cut.status[is_closed] == 0).all()
    assert (cut.status[no_data] == 3).all() and (cut.status[~no_data] != 3).all()
    assert cut.passed == ((cut.status == 0) | (cut.status == 3)).all()
    law.close()


def _points_in(res, which, per_leaf, seed):
    """Seeded points inside the cells ``which`` (positions), by barycentric weights."""
    rng = np.random.default_rng(seed)
    p = res.vertices.shape[2]
    w = rng.dirichlet(np.ones(p + 1), (which.size, per_leaf))
    return np.einsum('nkv,nvc->nkc', w, res.vertices[which]).reshape(-1, p)


def _violating_nodes(law, orc, res, X, input_tol):
    """(source nodes of the leaves in which the audit finds a violation, the audit)."""
    a = law.audit(orc, X=X, return_samples=True, input_tol=input_tol)
    return set(a.leaf[a.status == 1].tolist()), a


@pytest.mark.parametrize('single', [False, True], ids=['double', 'single'])
def test_no_audited_violation_in_a_certified_leaf(certified, single):
    from explicit_hybrid_mpc_amd.compiled import CompiledLaw
    c = certified('lin')
    law = c.law.to_single(flush=True) if single else c.law
    orc = c.orc
    p, n_u = law.p, law.n_u
    res = law.certify(orc, max_tries=0, return_leaves=True)
    sure = np.nonzero(res.status == 0)[0]
    assert sure.size >= 20
    X = _points_in(res, sure, 12, 21)
    _, leaf, _, _ = law.evaluate(X, return_info=True)
    certified_nodes = set(res.leaf_node[sure].tolist())
    keep = np.isin(leaf, res.leaf_node[sure])
    assert keep.mean() > 0.9
    a = law.audit(orc, X=X[keep], return_samples=True, input_tol=res.input_tol)
    assert a.counts['violation'] == 0
    # a third of the leaves tampered with: u_0 shifted by seeded amounts of several sizes
    rng = np.random.default_rng(22)
    arrays = law.arrays()
    n_leaf = res.n
    hit = rng.permutation(n_leaf)[:n_leaf // 3]
    sizes = rng.choice([0.02, 0.1, 0.3, 0.6], hit.size)
    shift = sizes[:, None] * rng.choice([-1., 1.], (hit.size, n_u))
    arrays['leaf_rec'][hit, p:p + n_u] += shift.astype(arrays['leaf_rec'].dtype)
    over = int(hit[0])                                   # one leaf far outside the input set
    arrays['leaf_rec'][over, p:p + n_u] = 2.
    arrays['leaf_rec'][over, p + n_u:p + n_u + n_u * p] = 0.
    broken = CompiledLaw.from_arrays(arrays)
    bad = broken.certify(orc, max_tries=0, return_leaves=True, input_tol=res.input_tol)
    assert bad.status[over] == 2 and bad.n_candidates[over] == 0
    same = np.ones(n_leaf, dtype=bool)
    same[hit] = False
    for k in ARRAYS + ('vertices', 'inputs'):
        assert np.array_equal(getattr(bad, k)[same], getattr(res, k)[same], equal_nan=True), k
    every = np.nonzero(bad.status != 4)[0]
    Xb = _points_in(bad, every, 8, 23)
    violating, audit = _violating_nodes(broken, orc, bad, Xb, res.input_tol)
    print('tampered: %r; audit %r; leaves with a violation %d' % (bad, audit, len(violating)))
    assert len(violating) > 0
    assert not (violating & set(bad.leaf_node[bad.status == 0].tolist()))
    assert violating <= set(bad.leaf_node[hit].tolist())
    assert certified_nodes >= set(bad.leaf_node[same & (bad.status == 0)].tolist())
    broken.close()
    if single:
        law.close()


def test_certify_refusals(certified):
    from types import SimpleNamespace
    from explicit_hybrid_mpc_amd import _capi
    c = certified('lin')
    law = c.law

    class NoBatch:                  # an oracle without the batched P_theta (bnb.PrefixOracle)
        eps_a, eps_r = c.orc.eps_a, c.orc.eps_r
    with pytest.raises(_capi.EhmError):
        law.certify(NoBatch())
    with pytest.raises(ValueError):
        law.certify(c.orc, max_tries=-1)
    with pytest.raises(ValueError):
        law.certify(c.orc, leaves=[law.stats['n_leaf']])
    # p + n_u > 8: refused before anything is solved
    rng = np.random.default_rng(5)
    synth = es.SynthLaw(es.kuhn_forest(7, 20), 2, 1, rng, n_sub=2)
    ex = synth.explicit()
    wide = ex.compile()
    ex.close()
    can = SimpleNamespace(p=7, n_u=2, n=12, n_delta=1)
    fake = SimpleNamespace(gpu=SimpleNamespace(can=can, _applied=None, eps_a=1., eps_r=1.,
                                                device=0), eps_a=1., eps_r=1.)
    with pytest.raises(ValueError) as err:
        wide.certify(fake)
    assert 'EHM_MAX_P' in str(err.value)
    with pytest.raises(ValueError):
        wide.certify(c.orc)                             # an oracle of another (p, n_u)
    wide.close()
    lib = _capi.load()
    gp = c.orc.gpu._handle
    opts = _capi.CertifyOpts(n=1, p=7, n_u=2, n_delta=1)
    out = _capi.CertifyResult()
    assert lib.ehm_compiled_certify(law._handle, gp, gp, opts, out, None) == _capi.EHM_E_INVALID
    assert b'p + n_u' in lib.ehm_certify_last_error()
    opts = _capi.CertifyOpts(n=1, p=law.p, n_u=law.n_u, n_delta=1)
    assert lib.ehm_compiled_certify(law._handle, gp, gp, opts, out, None) == _capi.EHM_E_INVALID
    assert b'cost_u' in lib.ehm_certify_last_error()
    assert lib.ehm_compiled_certify(None, gp, gp, opts, out, None) == _capi.EHM_E_INVALID
    empty = law.certify(c.orc, leaves=np.zeros(0, dtype=np.int32), return_leaves=True)
    assert empty.n == 0 and empty.passed and empty.status.shape == (0,) and empty.worst is None
