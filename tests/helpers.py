"""Shared helpers for the parity tests (test infrastructure)."""

import numpy as np

from explicit_hybrid_mpc_amd import examples
from oracle.oracle_cpu import OracleCPU
from oracle import geometry


CHAIN_SMALL_SCALE = 0.6      # x_max = (1, 1), T = 0.1, N = 8: every vertex feasible (tested)
PWA_SMALL_SCALE = 0.367     # 0.9 x max feasible scale (0.408, tools/calibrate_configs.py)


def make_instance(kind, seed=0):
    if kind == 'di':
        return examples.double_integrator(3)
    if kind == 'lin':
        return examples.linear_mpc(seed)
    if kind == 'pwa':
        return examples.pwa_mpc(seed)
    if kind == 'chain':
        # config 4 (n_x = 6, n_u = 3, N = 10, box constraints): LPs of 50..57 columns, 360..369
        # rows -- the LDS-resident wide kernels (ehm_k4.hip); the streaming ones (ehm_k3.hip) when
        # the handle eliminates nothing (STREAMING_CHAIN)
        return examples.integrator_chain_mpc()
    if kind == 'chain_small':
        # same family, n_x = 4, n_u = 2, N = 8: 32 + 4 + 1 = 37 columns, 21 of them factorised (a
        # shared-block case, ehm_k2.hip)
        mpc = examples.integrator_chain_mpc(n_axes=2, N=8)
        examples.THETA_SCALE.setdefault(mpc.name, CHAIN_SMALL_SCALE)
        return mpc
    if kind == 'pwa_small':
        # 2 states, 1 input, N=3: 8 commutations -- a hybrid instance whose whole partition
        # the CPU oracle finishes in seconds
        mpc = examples.pwa_mpc(seed=seed, n_x=2, n_u=1, N=3, n_random=4, overlap=0.3)
        examples.THETA_SCALE.setdefault(mpc.name, PWA_SMALL_SCALE)
        return mpc
    raise ValueError(kind)


def eps_a_rule(mpc, abs_frac):
    """examples.create_oracle's eps_a rule (lib/examples.py:42-46) with the CPU oracle."""
    orc = OracleCPU(mpc, 1., 1.)
    V = examples.box_vertices(examples.theta_box(mpc))
    return max(orc.P_theta(abs_frac * v)[2] for v in V)


def roots_of(mpc):
    V = examples.box_vertices(examples.theta_box(mpc))
    return geometry.delaunay_simplices(V)


def random_simplices(mpc, rng, n, scale_lo=-2., scale_hi=0.):
    half = examples.theta_box(mpc)
    p = half.size
    out = []
    for _ in range(n):
        scale = 10 ** rng.uniform(scale_lo, scale_hi)
        ctr = rng.uniform(-1, 1, p) * half * (1 - scale)
        R = ctr + scale * rng.uniform(-1, 1, (p + 1, p)) * half
        out.append(np.clip(R, -half, half))
    return np.array(out)


# ---- one single-commutation instance per persistent frontier kernel ------------------------------
# Members of examples.linear_mpc(seed=0, n_x, n_u, N, n_random), each routed by persistent_run
# (csrc/ehm_capi.hip) to one compiled persistent kernel: the two-width pairs kp / kpm
# (decide width, expand width, row slots; EHM_KP_ALL), the single-width k2 instances (np, slots)
# and the LDS-resident family k4.  Widths are factorised columns; s0 = created with EHM_SPARSE=0
# (no column eliminated, so the widths are n + p + 1 and n).  Scales: 0.9 x
# tools/calibrate_configs.max_feasible_scale (persistent_width_scale recomputes them).
#   (family, np_decide, np_expand, slots, n_x, n_u, N, n_random, s0, theta scale)
PERSISTENT_WIDTH_ROWS = (
    ('kp', 12, 8, 2, 2, 3, 2, 16, False, 0.7081),
    ('kp', 12, 8, 3, 2, 2, 4, 16, False, 0.8711),
    ('kp', 16, 8, 2, 4, 2, 4, 4, False, 0.596),
    ('kp', 16, 8, 3, 4, 2, 4, 8, False, 0.5063),
    ('kp', 16, 12, 2, 2, 3, 4, 4, False, 0.7054),
    ('kp', 16, 12, 3, 2, 3, 4, 16, False, 0.7081),
    ('kp', 16, 12, 4, 2, 2, 5, 24, False, 0.8764),
    ('kp', 20, 12, 2, 4, 2, 3, 4, True, 0.596),
    ('kp', 20, 12, 3, 4, 3, 4, 4, False, 0.485),
    ('kp', 20, 16, 2, 2, 3, 5, 4, False, 0.7054),
    ('kp', 20, 16, 3, 2, 3, 5, 8, False, 0.7533),
    ('kp', 24, 16, 2, 4, 2, 4, 4, True, 0.596),
    ('kp', 24, 16, 3, 5, 3, 5, 4, False, 0.7877),
    ('kp', 24, 20, 2, 2, 1, 6, 4, True, 0.3507),
    ('kp', 24, 20, 3, 2, 1, 6, 16, True, 0.3661),
    ('kp', 28, 20, 2, 4, 3, 4, 2, True, 0.6328),
    ('kp', 28, 20, 3, 4, 3, 4, 4, True, 0.485),
    ('kp', 28, 20, 4, 4, 2, 5, 16, True, 0.5365),
    ('kp', 28, 24, 2, 2, 2, 6, 4, True, 0.9),
    ('kp', 28, 24, 3, 2, 1, 8, 4, True, 0.3507),
    ('kp', 32, 24, 2, 4, 6, 3, 0, True, 0.9),
    ('kp', 32, 24, 3, 4, 2, 6, 4, True, 0.596),
    ('kp', 32, 24, 4, 4, 1, 8, 4, True, 0.573),
    ('kp', 32, 28, 2, 2, 2, 7, 1, True, 0.9),
    ('kp', 32, 28, 3, 2, 2, 7, 4, True, 0.9),
    ('k2', 8, 8, 1, 2, 1, 2, 4, False, 0.3507),
    ('k2', 8, 8, 2, 2, 1, 2, 24, False, 0.3421),
    ('k2', 8, 8, 3, 2, 1, 4, 24, False, 0.3408),
    ('k2', 12, 12, 1, 2, 3, 2, 4, False, 0.7054),
    ('k2', 12, 12, 2, 2, 3, 3, 4, False, 0.7054),
    ('k2', 12, 12, 3, 2, 3, 3, 24, False, 0.6668),
    ('k2', 12, 12, 4, 2, 1, 6, 24, False, 0.3407),
    ('k2', 16, 16, 1, 2, 3, 2, 4, True, 0.7054),
    ('k2', 16, 16, 4, 4, 2, 4, 24, False, 0.5162),
    ('k2', 20, 20, 4, 2, 3, 5, 24, False, 0.6668),
    ('k2', 24, 24, 4, 5, 3, 5, 8, False, 0.7924),
    ('k2', 24, 24, 2, 2, 1, 7, 4, True, 0.3507),
    ('k2', 24, 24, 3, 2, 1, 7, 8, True, 0.3965),
    ('k2', 28, 28, 2, 2, 3, 5, 4, True, 0.7054),
    ('k2', 28, 28, 3, 2, 3, 5, 8, True, 0.7533),
    ('k4', 24, 24, 4, 2, 1, 7, 16, True, 0.3661),
    ('k4', 24, 24, 4, 5, 1, 6, 8, True, 0.5934),
)
def persistent_width_name(row):
    fam, d, e, sl, n_x, n_u, N, n_random, s0 = row[:9]
    return '%s_%d_%d_%d-nx%d_nu%d_N%d_r%d%s' % (fam, d, e, sl, n_x, n_u, N, n_random,
                                               '_s0' if s0 else '')


def persistent_width_instance(row):
    """The row's MPC, its theta scale registered under a name that carries n_random too."""
    n_x, n_u, N, n_random, s0, scale = row[4:]
    mpc = examples.linear_mpc(seed=0, n_x=n_x, n_u=n_u, N=N, n_random=n_random)
    mpc.name = 'linear_nx%d_nu%d_N%d_r%d_seed0' % (n_x, n_u, N, n_random)
    if scale > 0:
        examples.THETA_SCALE.setdefault(mpc.name, scale)
    return mpc


def persistent_width_scale(row, tol=1e-4):
    """The row's theta scale as recorded: 0.9 x the largest centred box with feasible vertices,
    rounded down to four digits (tools/calibrate_configs.py)."""
    import math
    from tools.calibrate_configs import max_feasible_scale
    s = max_feasible_scale(persistent_width_instance(row[:9] + (0.0,)), tol=tol)
    return math.floor(1e4 * s * examples.THETA_SAFETY) / 1e4


def make_gp(row, can, eps_a, eps_r):
    """GpuProblem of the row; EHM_SPARSE=0 while the handle is created for the s0 rows."""
    import os
    from explicit_hybrid_mpc_amd import engine
    old = os.environ.get('EHM_SPARSE')
    if row[8]:
        os.environ['EHM_SPARSE'] = '0'
    try:
        gp = engine.GpuProblem(can, eps_a, eps_r)
    finally:
        if old is None:
            os.environ.pop('EHM_SPARSE', None)
        else:
            os.environ['EHM_SPARSE'] = old
    if row[8]:
        assert gp.layout()['nE'] == 0
    return gp


# ---- one quadratic-cost law per quadratic shared-block instance, and the edges of the row layout --
# Members of examples.linear_mpc(seed=0, n_x, n_u, N, n_random, cost='quadratic'): n = n_u N
# columns, m = N (2 n_x + n_random + 2 n_u) rows, p = n_x, nothing eliminated.  The instance named
# is the one of the suboptimality-test programme, n + p + 1 columns and lp_slots(m, p + 3) row slots
# (csrc/ehm_k2.h), among the -DEHM2_QUAD=1 instances of csrc/ehm_k2.hip (build.K2Q_NPS x K2_SLOTS);
# each row is the smallest member reaching its instance over n_x 2..4, n_u <= min(n_x, 3), N <= 30.
#   (capacity, slots, n_x, n_u, N, n_random, what the row is there for)
QUADRATIC_WIDTH_ROWS = (
    (8, 1, 2, 1, 1, 0, ''),
    (8, 2, 2, 1, 2, 24, ''),
    (8, 3, 4, 1, 3, 32, ''),
    (8, 4, 3, 1, 4, 40, ''),
    (16, 1, 4, 2, 2, 0, ''),
    (16, 2, 4, 1, 4, 8, ''),
    (16, 3, 4, 1, 4, 24, ''),
    (16, 4, 4, 1, 4, 40, ''),
    (24, 1, 4, 3, 4, 0, ''),
    (24, 2, 4, 3, 4, 2, ''),
    (24, 3, 3, 1, 13, 2, ''),
    (24, 4, 4, 1, 12, 8, ''),
    (32, 2, 3, 3, 7, 0, ''),
    (32, 3, 4, 3, 7, 4, ''),
    (32, 4, 4, 1, 20, 0, ''),
    # (32, 4) again with a short horizon and p = 3: the law of the persistent-kernel tests, whose
    # CPU partition solves the uncondensed programmes (N = 20 takes ten times as long)
    (32, 4, 3, 3, 7, 16, 'short'),
    # n + p + 1 = the capacity: the last factorised column, t, sits in lane NP - 1
    (8, 1, 4, 3, 1, 0, 'full'),
    (16, 1, 3, 3, 4, 0, 'full'),
    (24, 2, 3, 2, 10, 0, 'full'),
    (32, 3, 4, 3, 9, 0, 'full'),
    # m + p + 3 = 256 (m = 250): the second quadratic row is lane 63 of slot 4, and the law is at
    # the row limit of the generation-1 kernels
    (16, 4, 3, 1, 5, 42, 'rows256'),
    # m = 64: the extra rows open a slot of their own
    (8, 2, 2, 1, 1, 58, 'm64'),
    # (m mod 64) + (p + 3) = 64: the extras just fit behind the rows; = 65: lp_xbase moves them to
    # the next slot and leaves a gap of invalid rows
    (8, 1, 4, 1, 1, 47, 'fit64'),
    (8, 2, 4, 1, 1, 48, 'gap65'),
)
# the rows whose whole partition the persistent frontier kernel grows, and their theta scales:
# 0.999 x tools/calibrate_configs.max_feasible_scale (quadratic_width_scale recomputes them), so
# that the corner regions of the box are constrained
QUADRATIC_PERSISTENT_ROWS = {(24, 1, 4, 3, 4, 0, ''): 0.704, (24, 4, 4, 1, 12, 8, ''): 0.6369,
                             (32, 2, 3, 3, 7, 0, ''): 0.7827, (32, 4, 3, 3, 7, 16, 'short'): 0.7197}


def quadratic_width_name(row):
    cap, sl, n_x, n_u, N, n_random, tag = row
    return 'k2q_%d_%d-nx%d_nu%d_N%d_r%d%s' % (cap, sl, n_x, n_u, N, n_random,
                                             '_' + tag if tag else '')


def quadratic_width_instance(row, scale=None):
    """The row's MPC; with ``scale`` its theta scale is registered under a name of the row's own."""
    n_x, n_u, N, n_random = row[2:6]
    mpc = examples.linear_mpc(seed=0, n_x=n_x, n_u=n_u, N=N, n_random=n_random, cost='quadratic')
    mpc.name = 'quadratic_nx%d_nu%d_N%d_r%d_seed0' % (n_x, n_u, N, n_random)
    if scale is not None:
        examples.THETA_SCALE.setdefault(mpc.name, scale)
    return mpc


def quadratic_width_scale(row, tol=1e-4):
    """0.999 x the largest centred box with feasible vertices, rounded down to four digits."""
    import math
    from tools.calibrate_configs import max_feasible_scale
    return math.floor(1e4 * 0.999 * max_feasible_scale(quadratic_width_instance(row), tol=tol)) / 1e4


# ---- laws the LDS-resident wide family refuses: the streaming wide kernels (ehm_k3.hip) ----------
# Rows in the format above (family, np, np, slots, n_x, n_u, N, n_random, s0, theta scale); k3's two
# instances hold 64 columns x 8 or 16 row slots.  What k4 refuses them for (K2Api::fits):
#   B   30 x 520, p 4 (35 columns): more than 512 rows -- the 16-slot instance; 3-tile normal
#       matrix, on a handle WITH eliminated columns (k3 ignores DevProblem::Wc4)
#   C   50 x 520, p 4 (55 columns, all of which k3 factorises): more than 512 rows; 4 tiles
#   D   40 x 440, p 4 (45 columns), s0: the reduced block does not fit the LDS budget; 3 tiles
#   D4  the same law on a default handle (20 of 40 columns factorised): k4 takes it -- D's partner
# ('chain' with s0 -- 57 factorised columns, 8 slots, 4 tiles -- is the fifth, see STREAMING_CHAIN)
STREAMING_WIDE_ROWS = {
    'B': ('k3', 64, 64, 16, 4, 1, 10, 32, False, 0.5378),
    'C': ('k3', 64, 64, 16, 4, 3, 10, 24, False, 0.4582),
    'D': ('k3', 64, 64, 8, 4, 2, 10, 20, True, 0.4962),
    'D4': ('k4', 48, 48, 8, 4, 2, 10, 20, False, 0.4962),
}
STREAMING_CHAIN = ('k3', 64, 64, 8, None, None, None, None, True, 0.)     # make_instance('chain')
# multi-commutation law on the 16-slot instance: 15 x 515, p 2, 32 commutations
STREAMING_PWA = dict(n_x=2, n_u=1, N=5, n_random=90)
STREAMING_PWA_SCALE = 0.2309     # 0.9 x max feasible scale (tools/calibrate_configs.py)


def streaming_pwa_instance():
    mpc = examples.pwa_mpc(seed=0, **STREAMING_PWA)
    mpc.name = 'pwa_nx2_nu1_N5_r90_seed0'
    examples.THETA_SCALE.setdefault(mpc.name, STREAMING_PWA_SCALE)
    return mpc


# ---- shared assertions of the sharded persistent runs (GPU tests) --------------------------------
def check_dealt_shares(gp, roots, locs, world=3, per_rank=32, one_launch=True):
    """
    ehm_run_opts.deal_depth: one persistent launch per rank from the roots, dealt at a tree depth
    by the nodes' path codes.  The shares of ``world`` ranks (run one after the other on gp's
    GPU) tile the tree one unsharded run grows.  one_launch: each share is one launch, no sweeps
    (False for the wide-image problems, which sweep).  Returns (full tree, shares).
    """
    from explicit_hybrid_mpc_amd import distributed
    full = gp.partition(np.array(roots))
    depth = distributed.deal_depth_for(len(roots), world, per_rank=per_rank)
    parts = [gp.partition(np.array(roots), shard=(r, world, 0), deal_depth=depth)
             for r in range(world)]
    full_loc = full.locations(locs)
    full_leaves = {full_loc[k] for k in range(full.n_nodes) if full.is_leaf(k)}
    got = set()
    for part in parts:
        if one_launch:
            assert part.info['decide_launches'] == 1            # no sweeps at all
        loc = part.locations(locs)
        below = node_depths(part)
        mine = {loc[k]: below[k] for k in range(part.n_nodes)
                if part.is_leaf(k) and not (part.flags[k] & 4)}
        # the replicated top's closed leaves appear in every share; everything else once
        assert all(mine[name] <= depth for name in set(mine) & got)
        got |= set(mine)
        remote = [k for k in range(part.n_nodes) if part.flags[k] & 4]
        assert remote and all(part.is_leaf(k) for k in remote)
    assert got == full_leaves
    own_closed = [p_.info['n_closed'] - (p_.info['replicated_closed'] if r else 0)
                  for r, p_ in enumerate(parts)]
    assert sum(own_closed) == full.info['n_closed']
    own_nodes = [p_.info['n_nodes'] - (p_.info['replicated_nodes'] if r else 0)
                 for r, p_ in enumerate(parts)]
    assert sum(own_nodes) == full.n_nodes
    return full, parts


def node_depths(tree):
    """Depth of every node below its root."""
    out = np.zeros(tree.n_nodes, dtype=np.int64)
    for k in range(tree.n_nodes):          # children always have larger indices
        if tree.left[k] >= 0:
            out[tree.left[k]] = out[tree.right[k]] = out[k] + 1
    return out


def check_budgeted_rounds(gps, roots, locs, first_budget=64):
    """
    ehm_partition_advance: rounds of the PERSISTENT frontier kernel with a pop budget; what is
    left of its device queue is the frontier the ranks rebalance.  gps: three handles with the
    same problem and tolerances -- gps[0] and gps[1] play two ranks, rank 0 owns the roots, rank 1
    starts empty (shard_min_frontier < 0) and is fed by the first rounds; gps[2] grows the
    reference tree in one run.  The merged shares are that tree node for node.
    first_budget: pops of the first round, doubled every round (trees of under 2000 nodes need a
    smaller one to last the three rounds asked for below).
    Returns (reference tree, finished shares).
    """
    from explicit_hybrid_mpc_amd import distributed
    ref = gps[2].partition(roots, action='ecc')
    world = 2
    runs = [gps[r].begin(roots, shard=(r, world, -1)) for r in range(world)]
    assert runs[1].advance(10) == 0                     # nothing to do yet
    logs = [[] for _ in range(world)]
    rnd, moved, budget = 0, 0, int(first_budget)
    while True:
        counts = [run.advance(budget) for run in runs]
        budget = min(2 * budget, 4096)
        if sum(counts) == 0:
            break
        for donor, receiver, n in distributed.balance_plan(counts, tolerance=0.02, min_move=4):
            ids, rec, meta = runs[donor].take(n)
            first = runs[receiver].give(rec, meta)
            logs[donor].append(dict(kind='give', round=rnd, peer=receiver, ids=ids))
            logs[receiver].append(dict(kind='recv', round=rnd, peer=donor, first=first, count=n))
            moved += n
        rnd += 1
    parts = [run.finish(export=True) for run in runs]
    assert moved > 0 and rnd >= 3
    assert parts[1].info['n_closed'] > 0.2 * ref.info['n_closed']      # rank 1 really worked
    received = distributed.resolve_received(parts, logs, locs)
    merged = distributed.merge_flat(parts, locs, received)
    assert merged.n_nodes == ref.n_nodes
    rloc, mloc = ref.locations(locs), merged.locations(locs)
    ridx = {n: k for k, n in enumerate(rloc)}
    assert set(rloc) == set(mloc)
    for k, name in enumerate(mloc):
        j = ridx[name]
        assert np.array_equal(merged.vertices[k], ref.vertices[j])
        assert merged.is_leaf(k) == ref.is_leaf(j)
        assert (merged.flags[k] & 1) == (ref.flags[j] & 1)
        assert not (merged.flags[k] & 4)
        assert np.allclose(merged.vertex_costs[k], ref.vertex_costs[j], rtol=1e-9, atol=1e-12)
    assert sum(int(p.info['n_closed']) for p in parts) == int(np.sum((ref.flags & 1) > 0))
    return ref, parts
