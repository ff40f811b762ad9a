/*
 * ehmpc.h -- C-ABI of libehmpc.so, the MI355X (gfx950) implementation of the offline
 * parameter-space partitioning hot path of dmalyuta/explicit_hybrid_mpc.
 *
 * The reference is pure Python and has no FFI/plugin interface of its own
 * (SURVEY.md section 8b): its seam for this path is the Python `Oracle` object
 * (lib/oracle.py:18-474), the geometry helpers (lib/tools.py:134-257), the node types
 * (lib/tree.py:12-95) and the partition entry `alg_call(which_alg, branch, location)`
 * (lib/worker.py:180-185, 241-417).  Every entry point below states which of those it
 * replaces.  The Python package `explicit_hybrid_mpc_amd` binds this header with ctypes
 * and re-exposes the reference's Python signatures; INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions: plain C, every function returns 0 on success or a negative EHM_E_* code
 * (message via ehm_last_error(), thread-local).  All arrays are C-contiguous, caller
 * owned, float64 / int32 / uint8.  "host" entry points take host pointers and copy;
 * "_dev" entry points take device pointers valid on the problem's GPU and enqueue on
 * the problem's HIP stream without synchronising (use ehm_sync()).  A handle is bound to
 * one GPU and is not thread-safe (the reference's Oracle is not re-entrant either,
 * lib/oracle.py:271-280).  There is no CPU fallback: without a usable GPU
 * ehm_problem_create fails with EHM_E_NO_DEVICE.
 */
#ifndef EHMPC_H
#define EHMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libehmpc.so is built with -fvisibility=hidden: the entry points declared in this header (and
 * in the other two public headers) are its whole exported surface. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define EHM_OK              0
#define EHM_E_INVALID      -1   /* bad argument / unsupported dimension */
#define EHM_E_NO_DEVICE    -2   /* no HIP device, or HIP runtime error at setup */
#define EHM_E_HIP          -3   /* HIP runtime error during execution */
#define EHM_E_CAPACITY     -4   /* node pool exhausted (raise max_nodes) */
#define EHM_E_INFEASIBLE   -5   /* Theta contains infeasible regions (lib/worker.py:266) */
#define EHM_E_NUMERIC      -6   /* a vertex solve failed (lib/oracle.py:440-442) */

/* Limits of this build.  Up to 32 columns / 256 rows an LP is solved by one wavefront
 * (several LPs per workgroup around one LDS copy of the commutation's constant block);
 * wider LPs by one workgroup each, with the normal matrix formed on the matrix cores. */
#define EHM_MAX_N   64          /* LP columns incl. simplex weights and slack */
#define EHM_MAX_M   1024        /* LP rows   incl. simplex / cost rows */
#define EHM_MAX_P   8           /* parameter dimension */

/* Per-instance solve status (status arrays). */
#define EHM_ST_OPTIMAL  0       /* all relative optimality criteria met */
#define EHM_ST_STALLED  1       /* best iterate returned; merit > 1 */

/*
 * Canonical data of one MPC instance: for commutation index d (0..n_delta-1)
 *     J*(theta,d) = min_z c^T z   s.t.  G[d] z <= w[d] + S[d] theta ,   u0 = z[0:n_u].
 * Built on the host by explicit_hybrid_mpc_amd.mpc_library.PWAMPC.compile(); it carries
 * what the reference's Oracle.__init__ (lib/oracle.py:23-102) extracts from
 * mpc.make_constraints / mpc.cost.
 */
typedef struct ehm_problem_desc {
    int32_t n;          /* decision variables of P_theta_delta                       */
    int32_t m;          /* inequality rows                                           */
    int32_t p;          /* parameter dimension (= n_x; simplices have p+1 vertices)  */
    int32_t n_u;        /* inputs returned as u0                                     */
    int32_t n_delta;    /* admissible commutations                                   */
    int32_t delta_len;  /* length of one commutation vector (delta_size * N)         */
    const double*  G;       /* [n_delta][m][n] row-major                              */
    const double*  w;       /* [n_delta][m]                                           */
    const double*  S;       /* [n_delta][m][p]                                        */
    const double*  c;       /* [n]                                                    */
    const uint8_t* deltas;  /* [n_delta][delta_len] 0/1, enumeration order           */
    double eps_a;       /* absolute suboptimality tolerance (lib/oracle.py:38)       */
    double eps_r;       /* relative suboptimality tolerance (lib/oracle.py:39)       */
} ehm_problem_desc;

typedef struct ehm_problem ehm_problem;   /* opaque: device copies + stream + scratch */
typedef struct ehm_tree    ehm_tree;      /* opaque: grown partition, device resident */

/* Oracle.__init__ (lib/oracle.py:23-102). device = HIP ordinal. */
int ehm_problem_create(const ehm_problem_desc* desc, int device, ehm_problem** out);
int ehm_problem_destroy(ehm_problem* prob);
/* Quadratic part of the cost.  Every MPC law of the reference has a cvx.quad_form cost
 * (lib/mpc_library.py:180-183, :515-517): per commutation d
 *     V(z,theta) = c^T z + 1/2 z^T H[d] z + (f0[d] + F[d] theta)^T z
 *                  + 1/2 theta^T C[d] theta + c1[d]^T theta + c0[d]
 * H [n_delta][n][n], F [n_delta][n][p], f0 [n_delta][n], C [n_delta][p][p], c1 [n_delta][p],
 * c0 [n_delta]; H and C symmetric positive semidefinite (symmetrised on entry).  After this
 * call P_theta_delta is a convex QP, the suboptimality test (lib/oracle.py:89-97) a convex
 * QCQP with two quadratic rows, and every entry point below works on them (n+p+1 <= 32,
 * m+p+3 <= 256).  Both kernel generations carry the quadratic block; generation 2 is the
 * default, ehm_problem_set_solver(prob, 1) selects the one-wavefront kernels. */
int ehm_problem_set_quadratic(ehm_problem* prob, const double* H, const double* F,
                              const double* f0, const double* C, const double* c1,
                              const double* c0);
/* Re-set eps_a / eps_r (examples.create_oracle builds a second Oracle, lib/examples.py:43-46). */
int ehm_problem_set_eps(ehm_problem* prob, double eps_a, double eps_r);
/* Replaces the constant blocks of commutation slots [first, first + count) (G [count][m][n],
 * w [count][m], S [count][m][p], row-major like ehm_problem_desc) and rebuilds every image the
 * kernels read for them.  With it the commutation table is a cache of problems generated on the
 * fly: the prefix relaxations of a search over mode sequences -- what the reference leaves to the
 * MICP solver's branch-and-bound (lib/oracle.py:42-46, 89-102, lib/global_vars.py:25) --
 * explicit_hybrid_mpc_amd/sequences.py.  Not while a partition run is active. */
int ehm_problem_update_blocks(ehm_problem* prob, int32_t first, int32_t count, const double* G,
                              const double* w, const double* S);
/* Batched problems with the commutation given as a slot index of the table (not as a 0/1
 * vector): problems over a simplex (mode 0 = min, 1 = suboptimality-test slack, 2 = phase one;
 * the a5 / a7' problems of lib/oracle.py:74-79, 89-97) and P_theta_delta / its phase-one form
 * (lib/oracle.py:141-173). */
int ehm_simplex_idx_batch(ehm_problem* prob, int64_t n_inst, const double* R, const double* Vbar,
                          const int32_t* slot, int32_t mode, double* obj, double* alpha,
                          int32_t* status);
int ehm_point_idx_batch(ehm_problem* prob, int64_t n_inst, const double* theta,
                        const int32_t* slot, int32_t feas, double* J, double* u0,
                        int32_t* status);
/* Kernel generation used by this handle's launches: 2 (default) = one copy of the
 * commutation's constant LP block in LDS per workgroup, several wavefronts per workgroup;
 * 1 = one wavefront per workgroup with a private copy of the LP (first build, kept as an
 * on-device cross-check).  Environment override at create time: EHM_SOLVER=1|2. */
int ehm_problem_set_solver(ehm_problem* prob, int generation);
/* Named options: "solver" (1|2, as above); "decide_full" (0|1): by default the
 * suboptimality-test sweep of ehm_partition_run stops each LP as soon as the SIGN of its
 * optimum t* is certain (the reference's bar_E is a feasibility problem,
 * lib/oracle.py:285-309) and records a lower bound of |t*|; 1 = solve every test LP to full
 * accuracy (EHM_DECIDE_FULL=1 at create time does the same); "mid_first" (0|1, default 1): the
 * persistent frontier kernel solves a node's midpoint problem before its suboptimality test and
 * skips the test when the midpoint already proves the node open (42 % of the open nodes of the
 * bench tree; identical tree, tests/test_gpu_kernel_generations.py; EHM_MID_FIRST=0|1);
 * "inherit_witness" (0|1, default 1): a node the suboptimality-test LP finds open hands the
 * point that proved it (the LP iterate's parameter, with the cost of its decision vector as an
 * upper bound of the optimal cost there) to the child that contains it; the child is open
 * without an LP of its own while that point still beats its interpolated vertex costs by the
 * tolerance plus a safety margin (EHM_NO_WITNESS=1 disables);
 * "share_midpoints" (0|1, default 1): the persistent frontier kernel keeps a table of midpoint
 * optima in device memory -- the simplices around an edge all bisect it at the same point and,
 * with one commutation, solve the same problem there; the first to ask solves and publishes,
 * the others take the entry (csrc/ehm_midtable.h; identical tree, ehm_tree_info.midpoints_shared
 * counts the problems saved; EHM_NO_MIDTABLE=1 disables).  The same switch covers the table's
 * other uses: the level-synchronous wide kernels share their midpoint solves through it, the
 * persistent kernel looks up the midpoints of a node's OTHER edges as witnesses of openness
 * (ehm_tree_info.witness_table) and puts a node whose midpoint is being solved elsewhere back
 * into its queue instead of waiting, and the multi-commutation engine shares the results of its
 * point problems by (parameter, commutation, kind).  With the table on, WHICH valid witness a
 * node records (its own midpoint's, another edge's that a neighbour happened to have published,
 * an LP's) depends on the order wavefronts reach the table, so ehm_tree_info's solve and witness
 * counters, min_margin and the stored witnesses vary by a fraction of a percent between runs;
 * every verdict is taken with the same margin rule, and the tree (structure, vertices, vertex
 * costs, flags) does not vary.  "share_midpoints" = 0 gives run-to-run identical counters;
 * "any_admissible" (seed + 1, default 0 = off; multi-commutation handles): V_R and bar_D return a
 * draw among the ADMISSIBLE commutations -- feasible at every vertex; with t* >= 0 -- instead of
 * the canonical one (first in enumeration order; largest slack).  The reference poses both as
 * Minimize(0) (lib/oracle.py:201, 347): which admissible commutation comes back is its solver's
 * choice, and its published cwh_z tree sizes (lib/post_process.py:489, 526) carry that choice.
 * The draw is a hash of (seed, oracle, path code of the node), so a run repeats bit for bit and
 * the CPU oracle (oracle/oracle_cpu.py, rule 'hash') takes the same draws; values 2^30 + m are
 * deterministic extremes instead of draws (m bit 0: V_R returns the LAST commutation feasible at
 * every vertex, bit 1: bar_D the admissible commutation with the SMALLEST slack): the envelope of
 * what the choice can do to a tree (tools/cwh_jobs.py).  Not to be set while a run is active, and
 * ehm_partition_take / _give refuse to move nodes of a multi-commutation run under it (the
 * hand-over does not carry the path codes the draws read);
 * "budget_keep" (0|1, default 0): budgeted launches (ehm_partition_advance) let a wavefront keep
 * one child like unbudgeted ones.  Off by default: measured, the frontier such a launch leaves
 * costs the rebalancing rounds more than the kept children save.
 * "check_witness" (0|1, default 0): cross-check of the persistent kernel's two LP-free verdicts --
 * the tangent-plane bound is evaluated also for the nodes the inherited witness proves open; a
 * node it would close at the same time counts in ehm_tree_info.errors (a test option: it costs
 * the bound for every such node);
 * "work_first" (0|1, default 1): a wavefront of the persistent kernel that splits a node goes on
 * with one of the two children itself and queues the other (EHM_NO_WORKFIRST=1 disables);
 * "eager_children" (0|1, default 1): that wavefront runs both children's LP-free tests (inherited
 * witness, tangent-plane bound) on the copies it has in LDS when it creates them: a child the
 * bound closes is written closed and is never queued, the wavefront keeps a child that still
 * needs work (child 1 if both do), and a node the inherited witness proves open allocates its
 * children before its midpoint solve.  0 = every child is decided by a visit of its own.
 * Identical tree (tests/test_gpu_eager_children.py); ehm_tree_info.persist_ticks[9] counts the
 * children closed at creation, persist_pushes the queue pushes;
 * "requeue_undecided" (0|1, default 1): a node that finds its midpoint being solved by another
 * wavefront goes back into the queue once whether or not its fate is known (0: only the nodes the
 * inherited witness has opened, the others sleep through the solve); never in budgeted launches.
 * Identical tree (tests/test_gpu_persist_idle.py); persist_ticks[8] counts the nodes put back;
 * "timing" (0|1, default 0): multi-commutation runs record an event pair and a counter snapshot
 * around every batched launch, so that ehm_tree_info carries kernel seconds and solves by problem
 * kind (bench.py sets it; ~25 extra stream commands per sweep otherwise spared). */
int ehm_problem_set_option(ehm_problem* prob, const char* name, double value);
/* Environment switches read by the library (experiments and A/B measurements; none is needed):
 *   EHM_SOLVER=1|2, EHM_DECIDE_FULL=1   at ehm_problem_create, as the options above;
 *   EHM_ENGINE=0|1     overrides ehm_run_opts.engine (1 = persistent frontier kernel);
 *   EHM_NO_KP=1        persistent kernel at one solver width even where a two-width instance
 *                      (ehm_kp.hip, same kernel source) is compiled;
 *   EHM_NO_CUTS=1      no vertex gradients: every leaf is closed by its suboptimality-test LP
 *                      (the tangent-plane bound is also off under decide_full = 1);
 *   EHM_KEEP_GOING=1   a run whose oracle solves failed returns its tree instead of
 *                      EHM_E_NUMERIC;  EHM_DUMP_FAIL=path  writes the failing instance there. */
int ehm_sync(ehm_problem* prob);
/* HIP stream the handle enqueues on (a hipStream_t), for event timing by the caller. */
void* ehm_stream(ehm_problem* prob);

/* ---- batched oracles (host buffers) ------------------------------------------------ */

/* Oracle.P_theta_delta(theta, delta) (lib/oracle.py:141-173) for n_inst instances.
 * delta: [n_inst][delta_len] 0/1.  Outputs J [n_inst], u0 [n_inst][n_u],
 * status/iters [n_inst] (may be NULL).  An infeasible instance reports EHM_ST_STALLED. */
int ehm_solve_ptd_batch(ehm_problem* prob, int64_t n_inst, const double* theta,
                        const uint8_t* delta, double* J, double* u0,
                        int32_t* status, int32_t* iters);

/* Oracle.P_theta_delta(theta, delta, check_feasibility=True) (lib/oracle.py:164-167):
 * feasible[k] = 1 iff the constraint set is non-empty; tau[k] (may be NULL) is the
 * optimal worst-row violation (<= 0 iff feasible). */
int ehm_feas_ptd_batch(ehm_problem* prob, int64_t n_inst, const double* theta,
                       const uint8_t* delta, uint8_t* feasible, double* tau);

/* Oracle.P_theta(theta) (lib/oracle.py:104-139): minimum over all commutations, lowest
 * index on ties.  delta_idx[k] = -1 and J = +inf when no commutation is feasible. */
int ehm_solve_pt_batch(ehm_problem* prob, int64_t n_inst, const double* theta,
                       double* J, double* u0, int32_t* delta_idx);

/* Oracle.V_R(R) (lib/oracle.py:175-218): first commutation feasible at every vertex of
 * R [n_inst][p+1][p]; delta_idx = -1 if none.  vJ [n_inst][p+1], vu0 [n_inst][p+1][n_u]. */
int ehm_vr_batch(ehm_problem* prob, int64_t n_inst, const double* R,
                 int32_t* delta_idx, double* vJ, double* vu0);

/* Slack of the epsilon-suboptimality test for ONE commutation per instance: the decision
 * form of Oracle.bar_E_delta_R's constraints (lib/oracle.py:89-97)
 *     t* = max t  s.t. MPC constraints at theta = sum alpha_i v_i,
 *                      sum alpha_i Vbar_i - V - eps_a >= t,  sum alpha_i Vbar_i - (1+eps_r) V >= t.
 * alpha [n_inst][p+1] (may be NULL) is the maximiser's simplex weights. */
int ehm_slack_batch(ehm_problem* prob, int64_t n_inst, const double* R, const double* Vbar,
                    const uint8_t* delta, double* tstar, double* alpha, int32_t* status);

/* Oracle.bar_E_delta_R(R, V_delta_R) (lib/oracle.py:285-309): closed[k] = 1 iff no
 * commutation has t* >= 0 (epsilon-suboptimal => close the leaf).  tbest = max_d t*(d). */
int ehm_bar_e_batch(ehm_problem* prob, int64_t n_inst, const double* R, const double* Vbar,
                    uint8_t* closed, double* tbest);

/* min over the simplex for a fixed commutation (lib/oracle.py:74-79, used by
 * in_variability_ball :276). */
int ehm_min_simplex_batch(ehm_problem* prob, int64_t n_inst, const double* R,
                          const uint8_t* delta, double* Jmin, int32_t* status);

/* Oracle.bar_D_delta_R(R, V_delta_R, delta_ref) incl. in_variability_ball
 * (lib/oracle.py:311-414, 220-283).  delta_idx = -1 when there is no better commutation
 * (the reference's (None,None,None,None)); otherwise theta_star [p], vJ [p+1],
 * vu0 [p+1][n_u], var_small. */
int ehm_bar_d_batch(ehm_problem* prob, int64_t n_inst, const double* R, const double* Vbar,
                    const uint8_t* delta_ref, int32_t* delta_idx, double* theta_star,
                    double* vJ, double* vu0, uint8_t* var_small);

/* Oracle.P_theta_delta(theta, d, check_feasibility=True) for EVERY commutation d:
 * feasible [n_inst][n_delta]. */
int ehm_feas_all_batch(ehm_problem* prob, int64_t n_inst, const double* theta, uint8_t* feasible);

/* One visit of Worker.lcss for a batch of nodes (lib/worker.py:367-401): bar_E_delta_R and, for
 * the nodes that stay open, bar_D_delta_R, sharing the slacks the two oracles have in common and
 * what the caller already knows:
 *   vfeas [n_inst][p+1][n_delta]  feasibility of every commutation at every vertex (a child
 *         inherits p of its p+1 vertices; ehm_feas_all_batch on the new midpoints only),
 *   cand  [n_inst][n_delta] or NULL  commutations feasible somewhere on the PARENT simplex.
 * Feasible at a vertex => feasible on the simplex; infeasible on the parent => infeasible on the
 * child; only the rest gets a phase-one problem.  Outputs: closed / tbest as ehm_bar_e_batch,
 * cand_out [n_inst][n_delta] (feasible on this simplex: the children's `cand`), and for open
 * nodes delta_idx / theta_star / vJ / vu0 / var_small as ehm_bar_d_batch (delta_idx = -1 for
 * closed nodes).  Same verdicts and optima as the two calls, ~2.5x fewer sub-problems. */
int ehm_lcss_batch(ehm_problem* prob, int64_t n_inst, const double* R, const double* Vbar,
                   const uint8_t* delta_ref, const uint8_t* vfeas, const uint8_t* cand,
                   uint8_t* closed, double* tbest, uint8_t* cand_out, int32_t* delta_idx,
                   double* theta_star, double* vJ, double* vu0, uint8_t* var_small);


/* ---- geometry ------------------------------------------------------------------------ */

/* tools.split_along_longest_edge (lib/tools.py:224-257), bit-exact incl. the first-max
 * tie rule.  R,S1,S2: [n][p+1][p]; ij: [n][2].  device = HIP ordinal. */
int ehm_split_batch(int device, int64_t n, int32_t p, const double* R,
                    double* S1, double* S2, int32_t* ij);
/* tools.simplex_volume (lib/tools.py:134-150). */
int ehm_volume_batch(int device, int64_t n, int32_t p, const double* R, double* vol);

/* ---- partition engine ---------------------------------------------------------------- */

typedef struct ehm_run_opts {
    int64_t max_nodes;      /* node pool capacity (0 = default)                          */
    int32_t max_depth;      /* stop splitting below this depth relative to roots (0 = none) */
    int32_t action;         /* 0 = 'ecc' then 'lcss' (lib/worker.py:241-291), 1 = 'lcss'   */
    int32_t engine;         /* 0 = level-synchronous sweeps (decide / scan / expand launches per
                             * tree level); 1 = persistent frontier kernel: ONE launch, every
                             * wavefront pops nodes from a device queue, tests them and pushes
                             * the children of the ones it splits -- used when the run goes to
                             * completion on one rank with the shared-block kernels, otherwise
                             * the sweeps run.  Node ids in device memory then follow the
                             * allocation order; ehm_tree_export relabels them breadth first,
                             * i.e. to the numbering of engine 0 (same tree either way). */
    /* Multi-GPU sharding of the live frontier: every rank grows the same top of the tree
     * until a sweep's frontier holds >= shard_min_frontier nodes, then keeps only the
     * frontier nodes whose position k satisfies k % shard_world == shard_rank (the rest are
     * flagged bit2 = "owned by another rank").  shard_world <= 1 disables it. */
    int32_t shard_rank;
    int32_t shard_world;
    int32_t skip_volume;    /* 1 = do not compute volume_closed in ehm_tree_info_get       */
    int64_t shard_min_frontier;
    /* > 0 (with shard_world > 1, engine 1): the whole run is ONE launch of the persistent
     * frontier kernel on every rank, from the roots; the tree above this depth is grown
     * identically everywhere (replicated), a node created AT this depth is pursued by rank
     * (path code % shard_world) only -- no sweeps, no host round trip, no collective.
     * 0 = deal the frontier of a sweep (shard_min_frontier), then one launch per share. */
    int32_t deal_depth;
    int32_t reserved0;
} ehm_run_opts;

/* Optional initial node data for action 1 ('lcss' roots already carry a commutation,
 * lib/scheduler.py:633-639). */
typedef struct ehm_node_init {
    const uint8_t* delta;   /* [n_roots][delta_len]   */
    const double*  vcost;   /* [n_roots][p+1]         */
    const double*  vinput;  /* [n_roots][p+1][n_u]    */
} ehm_node_init;

/* alg_call(which_alg, branch, location) (lib/worker.py:180-185) for a batch of root
 * simplices: grows every root until all leaves are epsilon-suboptimal.
 * root_vertices: [n_roots][p+1][p] host. */
int ehm_partition_run(ehm_problem* prob, int64_t n_roots, const double* root_vertices,
                      const ehm_node_init* init, const ehm_run_opts* opts, ehm_tree** out);

/* The same run in resumable pieces, for the multi-GPU driver (one process per GPU): every rank
 * runs a few sweeps, the ranks all-gather their frontier sizes (RCCL) and move node records
 * from the longest frontiers to the shortest.  The reference rebalances through its MPI
 * master/worker star (lib/scheduler.py:498-599); here only counts and the moved records travel.
 *   begin  : uploads the roots (and runs the 'ecc' vertex solves);
 *   step   : up to max_sweeps frontier sweeps (<= 0: until the frontier is empty);
 *            *frontier_size = live frontier nodes afterwards;
 *   take   : removes count frontier nodes -- every s-th entry of the frontier, s = size / count,
 *            a sample of all its depths (single-commutation runs; the newest count entries if
 *            s < 2, on multi-commutation runs, or with EHM_TAKE_NEWEST=1): node_ids [count], records
 *            [count][(p+1)p + (p+1) + (p+1)n_u] (vertices | vertex costs | vertex inputs),
 *            meta [count][2] = (commutation index, depth); the nodes get flag bit2;
 *   give   : appends count nodes produced by another rank's take to the pool (flag bit5)
 *            and to the live frontier; *first_id = node id of the first one;
 *   finish : totals for ehm_tree_info_get / ehm_tree_export (required before either).
 * The buffers of take (node_ids, records, meta) and give (records, meta) may be HOST or DEVICE
 * pointers (hipMemcpyDefault): the multi-GPU driver hands device-resident blocks -- torch tensors --
 * straight to ncclSend / ncclRecv, no staging through the host. */
int ehm_partition_begin(ehm_problem* prob, int64_t n_roots, const double* root_vertices,
                        const ehm_node_init* init, const ehm_run_opts* opts, ehm_tree** out);
int ehm_partition_step(ehm_tree* tree, int32_t max_sweeps, int64_t* frontier_size);
int ehm_partition_take(ehm_tree* tree, int64_t count, int32_t* node_ids, double* records,
                       int32_t* meta);
int ehm_partition_give(ehm_tree* tree, int64_t count, const double* records,
                       const int32_t* meta, int32_t* first_id);
int ehm_partition_finish(ehm_tree* tree);

/* Progress of a run in flight, between two ehm_partition_step calls: what the reference's
 * WorkerStatusPublisher accumulates per closed leaf (lib/worker.py:19-116, 374-375) -- volume
 * filled, simplex count -- read from the device node pool (one reduction kernel). */
typedef struct ehm_progress {
    int64_t n_nodes;        /* simplices generated so far (multi-GPU: the replicated top */
    int64_t n_closed;       /* of the tree is reported by rank 0 only); closed leaves    */
    int64_t frontier;       /* live frontier size                                       */
    int64_t sweeps;
    int64_t lp_solves;
    int64_t ipm_iters;
    int32_t depth;
    int32_t reserved;
    double  volume_closed;  /* sum of the closed leaves' volumes                        */
    int64_t n_splits;       /* splits performed by this rank: what the reference's status
                               publisher counts (simplex_count += 1 per split,
                               lib/worker.py:274,327,107-109)                           */
} ehm_progress;
/* Up to max_pops node visits of the persistent frontier kernel (<= 0: to completion); the
 * unprocessed part of its device queue -- a contiguous slice, the queue is consumed in order --
 * becomes the live frontier again, so ehm_partition_take / _give can move nodes between ranks
 * before the next call.  Single-commutation problems on the shared-block kernels.
 * Dynamic multi-GPU runs: ehm_run_opts.shard_min_frontier < 0 makes every rank but 0 start with
 * an EMPTY frontier (rank 0 owns the roots); the rebalancing rounds feed them. */
int ehm_partition_advance(ehm_tree* tree, int64_t max_pops, int64_t* frontier_size);
/* Pool occupancy of a run in progress, without touching the device: nodes allocated so far and
 * the capacity of this run (max_nodes).  The multi-GPU driver checks a receiver's free pool
 * before it plans a transfer (explicit_hybrid_mpc_amd/distributed.py). */
int ehm_partition_counts(const ehm_tree* tree, int64_t* n_nodes, int64_t* max_nodes);
/* What ehm_partition_take can hand over right now, and the width of one record in doubles:
 * single-commutation runs move any frontier node ([vertices | costs | inputs]); multi-commutation
 * runs move lcss nodes only, each with the engine's bit rows appended (feasibility per vertex,
 * candidates, inherited verdicts, blacklist: csrc/ehm_hybrid.h).  records of take / give are
 * [count][record_doubles]. */
int ehm_partition_movable(const ehm_tree* tree, int64_t* movable, int32_t* record_doubles);
int ehm_partition_progress(ehm_tree* tree, ehm_progress* out);

typedef struct ehm_tree_info {
    int64_t n_nodes;
    int64_t n_leaves;
    int64_t n_roots;
    int64_t n_closed;       /* leaves with is_epsilon_suboptimal                        */
    int64_t lp_solves;      /* LP sub-problems solved on the device                     */
    int64_t ref_solves;     /* reference-equivalent oracle calls (one MICP = 1)         */
    int64_t ipm_iters;      /* interior-point iterations summed over all solves         */
    int64_t sweeps;         /* frontier sweeps (levels)                                 */
    int32_t max_depth;
    int32_t truncated;      /* 1 if max_depth / capacity stopped the growth             */
    double  volume_closed;  /* sum of closed leaf volumes (lib/worker.py:374-375)       */
    double  min_margin;     /* min |t*| over all close/split decisions                  */
    double  device_seconds; /* GPU time of the whole run (HIP events on the stream)     */
    double  decide_seconds; /* summed duration of the suboptimality-test sweep kernel   */
    double  expand_seconds; /* summed duration of the split + midpoint-solve kernel     */
    int64_t decide_launches;
    int64_t expand_launches;
    int64_t decide_solves;  /* LPs solved by the decide kernel                          */
    int64_t decide_iters;   /* their interior-point iterations                          */
    /* multi-GPU sharding: work done before the frontier was dealt is identical on every rank */
    int64_t replicated_closed;
    int64_t replicated_nodes;
    int64_t replicated_solves;
    int64_t cert_closed;    /* leaves closed by the tangent-plane bound of t* (gradients of the
                               optimal cost at the vertices, from the multipliers of the vertex
                               solves) without solving their suboptimality-test LP            */
    int64_t witness_open;   /* nodes proved open by their midpoint solve (option "mid_first") */
    /* multi-commutation runs */
    int64_t swaps;          /* nodes that took a better commutation in place (lib/worker.py:396-401) */
    int64_t blacklisted;    /* commutations blacklisted after a failed vertex solve
                               (lib/oracle.py:198-218, 406-414) */
    /* solves / interior-point iterations by problem kind: [0] P_theta_delta, [1] its phase-one
     * form, [2] min over a simplex, [3] suboptimality test (slack), [4] phase one over a simplex.
     * Multi-commutation runs: decide_* / decide_seconds cover the simplex kinds (2-4),
     * expand_seconds the point kinds (0-1). */
    int64_t kind_solves[5];
    int64_t kind_iters[5];
    /* near-threshold routing: decisions whose |t*| is below 1e-6 (1 + |V_0|); each of them was
     * taken by the suboptimality-test problem solved to full accuracy, never by a shortcut
     * (sign-only stop, tangent-plane bound, midpoint witness, inherited verdict) */
    int64_t near_threshold;
    int64_t witness_inherited;  /* nodes proved open by the witness of an ancestor's
                                   suboptimality test (option "inherit_witness"), no LP     */
    int64_t midpoints_shared;   /* splits whose midpoint optimum another simplex around the same
                                   edge had solved already (option "share_midpoints"), no LP */
    /* persistent frontier kernel: where its wavefronts spent their time, in ticks of the 100 MHz
     * wall clock summed over all of them: [0] resident, [1] waiting for a queue slot to be filled
     * (starved), [2] waiting for a midpoint optimum another wavefront was solving, [3] in midpoint
     * solves, [4] in suboptimality-test solves; [5] = number of waits of kind [2]; [6] from the
     * pop of a node to its midpoint claim (record load, tangent-plane bound, inherited witness,
     * longest edge), [7] child records and queue pushes; [8] = nodes put back into the queue
     * because another wavefront was solving their midpoint; [9] = children closed by the
     * tangent-plane bound when they were created (option "eager_children"): leaves that never
     * entered the queue, a part of cert_closed */
    int64_t persist_ticks[10];
    int64_t witness_table;      /* nodes proved open by the optimum at the midpoint of one of their
                                   OTHER edges, left in the table of midpoint optima by a
                                   neighbouring simplex that had bisected that edge, no LP */
    int64_t persist_pushes;     /* persistent frontier kernel: children pushed into its queue (the
                                   kept child of a split and a child closed at its creation are
                                   not; neither are the nodes put back, persist_ticks[8]) */
} ehm_tree_info;

int ehm_tree_info_get(const ehm_tree* tree, ehm_tree_info* out);
/* Flat export, node k: vertices [k][p+1][p], left[k] / right[k] child index or -1,
 * delta_idx[k] (-1 = none), vcost [k][p+1], vinput [k][p+1][n_u],
 * flags[k] bit0 = is_epsilon_suboptimal, bit1 = has commutation data,
 * bit2 = subtree owned by another rank (multi-GPU sharding / ehm_partition_take),
 * bit5 = node received from another rank (ehm_partition_give; it is a root of this part).
 * Nodes 0..n_roots-1 are the roots in input order.  Any pointer may be NULL. */
int ehm_tree_export(const ehm_tree* tree, double* vertices, int32_t* left, int32_t* right,
                    int32_t* delta_idx, double* vcost, double* vinput, uint8_t* flags,
                    double* tstar);
int ehm_tree_destroy(ehm_tree* tree);
/* Page-locked host memory for the arrays ehm_tree_export fills (the export then runs at the speed
 * of the host link; the branch is the worker's output, lib/worker.py:456-458).  Free with
 * ehm_host_free. */
int ehm_host_alloc(size_t bytes, void** out);
int ehm_host_free(void* ptr);


/* ---- batched evaluation of the explicit control law (the partition's consumer) --------- */

/* ExplicitMPC.setup + __call__ (lib/mpc_library.py:677-792) for batches of states.  The
 * partition comes as the flat export of ehm_tree_export (or any binary forest in that form):
 * nodes 0..n_roots-1 are the root simplices in tools.delaunay order (they hang off the
 * reference's right spine, lib/tools.py:152-189), left/right = child index or -1,
 * vertices [n_nodes][p+1][p], vinput [n_nodes][p+1][n_u].  create computes
 * inv([v1-v0 .. vp-v0]) for every node on the device (compute_simplex_basis_inverse, :685-712). */
typedef struct ehm_explicit ehm_explicit;
int ehm_explicit_create(int device, int64_t n_nodes, int32_t n_roots, int32_t p, int32_t n_u,
                        const int32_t* left, const int32_t* right, const double* vertices,
                        const double* vinput, ehm_explicit** out);
/* x [n][p] -> u [n][n_u] (barycentric interpolation in the containing leaf, :786-789);
 * leaf [n] = node id of that leaf, visited [n] = containment tests on the way (both may be
 * NULL); kernel_seconds (may be NULL) = device time of the evaluation kernel. */
int ehm_explicit_eval_batch(ehm_explicit* ex, int64_t n, const double* x, double* u,
                            int32_t* leaf, int32_t* visited, double* kernel_seconds);
int ehm_explicit_destroy(ehm_explicit* ex);
const char* ehm_explicit_last_error(void);

/* ---- the explicit law compiled into a hyperplane tree with affine leaf gains ------------------
 *
 * Every split of the partition is a bisection, so inside a parent "left child" is the sign of one
 * affine function (the split face), and the interpolation over a leaf is u = u_0 + K (x - v_0).
 * A compiled law holds, in arrays it owns (it outlives the handle it was compiled from):
 *   node       [n_int][node_stride]   [a (p) | b | (left, right) int32 pair]; a child >= 0 is an
 *                                     internal node, < 0 is ~leaf; children come after parents.
 *                                     Plane node: left iff ((0 + a_0 x_0) + ..) + b >= -eps.
 *                                     Test node (children that are no bisection): a = +0.0, b = its
 *                                     row of test_rec; left iff the left child's simplex holds x.
 *   leaf_rec   [n_leaf][leaf_stride]  [v_0 (p) | u_0 (n_u) | K (n_u x p, row-major)]
 *   leaf_node  [n_leaf]               node id of the leaf in the source tree
 *   test_rec   [n_test][side_stride]  [v_0 | inv(E)] of a test node's left child
 *   root_rec   [n_roots][side_stride] [v_0 | inv(E)] of the roots;  root_entry [n_roots]: a root's
 *                                     index (internal, or ~leaf);  nbr [n_roots][p+1] (header
 *                                     entry has_nbr): the roots' face adjacency
 * (strides in doubles) and the header, int64 [12]: version, p, n_u, n_roots, n_int, n_leaf, n_test,
 * node_stride, leaf_stride, side_stride, has_nbr, nodes of the source tree.
 *
 * create compiles the law of `src` on its device; vertices [n_nodes][p+1][p] are the ones `src`
 * was created from (it keeps only their inverses); compile_seconds may be NULL. */
typedef struct ehm_compiled ehm_compiled;
int ehm_compiled_create(ehm_explicit* src, const double* vertices, ehm_compiled** out,
                        double* compile_seconds);
/* create with a flags word (create is flags = 0).  EHM_COMPILE_SPINE_ROOTS: where `src` has one
 * root and the chain s_0 = 0, s_(i+1) = right(s_i) of internal test nodes has m > 0 nodes (the
 * data-less spine of a nested tree), those nodes get no record and the law gets the m + 1 roots
 * left(s_0), .., left(s_(m-1)), right(s_(m-1)) instead: root_rec their [v_0 | inv(E)] records,
 * root_entry their indices, nbr their face adjacency (from `vertices`) from 128 roots on.  Without
 * such a chain, or with more than one root, the flag changes nothing. */
#define EHM_COMPILE_SPINE_ROOTS 1
int ehm_compiled_create_opts(ehm_explicit* src, const double* vertices, int32_t flags,
                             ehm_compiled** out, double* compile_seconds);
/* As ehm_explicit_eval_batch: leaf [n] = source node id of the leaf, depth [n] = decisions made
 * (root tests or locator steps, then one per level); both and kernel_seconds may be NULL. */
int ehm_compiled_eval_batch(ehm_compiled* law, int64_t n, const double* x, double* u,
                            int32_t* leaf, int32_t* depth, double* kernel_seconds);
/* info [14]: the header, then the device bytes of the arrays and of the source evaluator's arrays
 * for the same tree (0 for an imported law). */
int ehm_compiled_info(const ehm_compiled* law, int64_t* info);
/* The arrays to host memory (sizes from the header; an array may be NULL to skip it). */
int ehm_compiled_export(ehm_compiled* law, double* node, double* leaf_rec, int32_t* leaf_node,
                        double* test_rec, double* root_rec, int32_t* root_entry, int32_t* nbr);
/* Checks arrays of the sizes the header states (host only, no device needed): version, p <= 8,
 * strides, every child / leaf / root / adjacency index in range, children after their parents
 * (so no cycle), finite records.  EHM_E_INVALID otherwise: a file is untrusted input. */
int ehm_compiled_validate(const int64_t* header, const double* node, const double* leaf_rec,
                          const int32_t* leaf_node, const double* test_rec,
                          const double* root_rec, const int32_t* root_entry, const int32_t* nbr);
/* A new law from exported arrays, validated as above before anything reaches the device. */
int ehm_compiled_import(int device, const int64_t* header, const double* node,
                        const double* leaf_rec, const int32_t* leaf_node, const double* test_rec,
                        const double* root_rec, const int32_t* root_entry, const int32_t* nbr,
                        ehm_compiled** out);

/* ---- the compiled law in single precision ------------------------------------------------------
 *
 * The law a flight computer runs: the reference sizes it for an on-board computer
 * (get_opt_memreq, lib/post_process.py:99-142).  Only node and leaf_rec become floats, at strides of
 * their own (in floats): node [a (p) | b | left, right int32], 8 floats (p <= 5) or 16; leaf_rec
 * [v_0 | u_0 | K] rounded up to a multiple of 4.  leaf_node, root_rec, root_entry and nbr stay as
 * they are, and so does the choice of the root, made in double on the double state.  Below the root
 * xs = (float) x; s = ((0 + a_0 xs_0) + .. + a_(p-1) xs_(p-1)) + b, left iff s >= -2^-23; at the
 * leaf u_c = u_0c + ((0 + K_c0 d_0) + ..) with d = xs - v_0, widened to double; every product and
 * every sum rounded once to float.  ehm_compiled_eval_batch, the plant and noise setters and the two
 * rollouts take a handle of either precision.
 *
 * narrow: a new, independent single law from a double one, its records rounded to nearest on the
 * device.  EHM_E_INVALID for a law with test nodes, a value that overflows, a nonzero value that
 * becomes zero or subnormal, a plane whose normal becomes zero. */
int ehm_compiled_narrow(ehm_compiled* law, ehm_compiled** out);
/* narrow with a flags word (narrow is flags = 0).  EHM_NARROW_FLUSH: a nonzero value whose float
 * is zero or subnormal (every such value is below 2^-126 in magnitude) is stored as +0.0f instead
 * of being refused; flushed [3] (may be NULL) receives how many plane coefficients, plane offsets
 * and leaf values were set to zero (all 0 without the flag).  Still EHM_E_INVALID: test nodes, an
 * overflow, a plane whose normal is zero after narrowing and flushing. */
#define EHM_NARROW_FLUSH 1
int ehm_compiled_narrow_opts(ehm_compiled* law, int32_t flags, int64_t* flushed,
                             ehm_compiled** out);
/* ehm_compiled_export for a single law (EHM_E_INVALID for a double one, as ehm_compiled_export is
 * for a single one); a single law has no test_rec. */
int ehm_compiled_export_single(ehm_compiled* law, float* node, float* leaf_rec, int32_t* leaf_node,
                          double* root_rec, int32_t* root_entry, int32_t* nbr);
/* ehm_compiled_validate / _import for the arrays of a single law: the same checks at the single
 * strides, and no test node, no zero normal, every float of node and leaf_rec zero or normal. */
int ehm_compiled_validate_single(const int64_t* header, const float* node, const float* leaf_rec,
                            const int32_t* leaf_node, const double* root_rec,
                            const int32_t* root_entry, const int32_t* nbr);
int ehm_compiled_import_single(int device, const int64_t* header, const float* node,
                          const float* leaf_rec, const int32_t* leaf_node, const double* root_rec,
                          const int32_t* root_entry, const int32_t* nbr, ehm_compiled** out);
int ehm_compiled_destroy(ehm_compiled* law);
const char* ehm_compiled_last_error(void);

/* ---- closed-loop simulation under the explicit law (lib/simulator.py, lib/post_process.py) ---
 *
 * The plant the law is closed around (Simulator.__init__, lib/simulator.py:73-122, with the
 * plant period equal to the controller's T_s):
 *     x+ = A_m x + B_m u + w_m + E d      m = step-0 mode of the leaf's commutation,
 * n_modes <= 4 modes, A [n_modes][p][p], B [n_modes][p][n_u], w [n_modes][p]; E [p][n_d] with
 * n_d <= 8 (n_d = 0: no disturbance input, E may be NULL); mode m holds where
 * H_m x <= h_m: region_rows [n_modes] rows each (NULL: no region), H [rows][p], h [rows] stacked
 * by mode; Gx [n_g][p], gx [n_g] (n_g <= 256) the state constraints whose worst value the
 * rollout reports; node_mode [n_nodes] the mode of every node (-1: no commutation, a
 * trajectory that reaches such a leaf stops with status 3); stage cost cost_kind 0:
 * ||Q x||_inf + ||R u||_inf, 1: x'Qx + u'Ru, Q [p][p], R [n_u][n_u].  The law's n_u must be
 * <= 4.  Replaces an earlier plant. */
int ehm_explicit_set_plant(ehm_explicit* ex, int32_t n_modes, const double* A, const double* B,
                           const double* w, int32_t n_d, const double* E,
                           const int32_t* region_rows, const double* H, const double* h,
                           int32_t n_g, const double* Gx, const double* gx,
                           const int32_t* node_mode, int32_t cost_kind, const double* Q,
                           const double* R);
/* A guarded multi-rate plant instead (simulate.GuardedPlant; lib/simulator.py:124-188 with a
 * plant period T_s / substeps, lib/mpc_library.py:588-626): per controller step the law's u is
 * held over substeps (1..64) plant steps x+ = A_m x + B_m u + w_m, n_modes <= 8, where before
 * each plant step m is guard_mode[g] of the first guard g (n_guards of them) whose rows
 * guard_row0[g] .. guard_row0[g+1]-1 all hold, else default_mode.  Row r holds iff
 *     ((sum_c ga[r][c] x_c) + sum_c gb[r][c] u_c) + gc[r]  <=  gt[r]     (< if strict[r]),
 * summed in that order without FMA (at most 16 rows; ga [rows][p], gb [rows][n_u]).  No
 * mode-region check (status 2 does not occur) and no disturbance; node_mode only marks leaves
 * without commutation (-1, status 3).  Stage cost, u_norm_sum and the Gx rows are taken at
 * controller steps, the records of ehm_explicit_rollout too.  ehm_explicit_rollout_noisy
 * refuses a guarded plant.  Replaces an earlier plant. */
int ehm_explicit_set_plant_guarded(ehm_explicit* ex, int32_t n_modes, const double* A,
                                   const double* B, const double* w, int32_t substeps,
                                   int32_t n_guards, const int32_t* guard_mode,
                                   const int32_t* guard_row0, const double* ga, const double* gb,
                                   const double* gc, const double* gt, const int32_t* strict,
                                   int32_t default_mode, int32_t n_g, const double* Gx,
                                   const double* gx, const int32_t* node_mode, int32_t cost_kind,
                                   const double* Q, const double* R);
/* n trajectories of T steps from x0 [n][p], one device thread each (Simulator.run,
 * lib/simulator.py:124-188).  Step t: measure z = x + v[t] (v [T][n][p] or NULL; no error at
 * t = 0, :168), locate z with the walk of ehm_explicit_eval_batch (same leaf, bit-equal u),
 * stop if z is outside the leaf (a barycentric weight < -tol_exit: status 1, no input applied),
 * stop if the mode's region does not hold x (status 2), else apply u and step the plant with
 * d[t] (d [T][n][n_d] or NULL).  Time-major records, each may be NULL: x_traj [T+1][n][p],
 * u_traj [T][n][n_u], leaf_traj [T][n]; after a stop NaN states / inputs and leaf -1.  Always:
 * x_final [n][p], steps [n] (T if never stopped), status [n] (0 ok, 1 left the set, 2 mode
 * region violated, 3 leaf without commutation), cost [n] (summed stage cost), u_norm_sum [n]
 * (sum of ||u_t||_2, the delta-v usage of total_delta_v_usage, lib/post_process.py:242-266),
 * max_violation [n] (max over steps and rows of Gx x_{t+1} - gx; -inf if no step was taken).
 * kernel_seconds (may be NULL) = device time of the rollout kernel. */
int ehm_explicit_rollout(ehm_explicit* ex, int64_t n, int32_t T, const double* x0,
                         const double* d, const double* v, double tol_exit, double* x_traj,
                         double* u_traj, int32_t* leaf_traj, double* x_final, int32_t* steps,
                         int32_t* status, double* cost, double* u_norm_sum,
                         double* max_violation, double* kernel_seconds);

/* ---- the closed loop under the reference's noise model (lib/uncertainty_sets.py, noise.py) ----
 *
 * The model as flat arrays (NoiseModel.pack): n_terms <= 16 terms in model order, desc
 * [n_terms][8] int32 per term: kind (0 process -> d, 1 state -> v, 2 input -> e), shape (0 box,
 * 1 ball), dim (box <= 8, ball <= 3), ball norm (0 inf, 1 (dim 1 only), 2), radius dependency
 * (0 constant, 1 ||F x||, 2 ||F u||), its norm (0 inf, 1, 2), rows of F (<= 8), offset into data;
 * data [n_data] the terms' doubles: box c [dim], h [dim], M [out][dim] (draw M (c + h s));
 * ball sigma, F [rows][p or n_u], L [out][dim] (draw L q, q uniform in the ball of radius sigma,
 * sigma ||F x|| or sigma ||F u||).  out = n_d (must equal the plant's), p or n_u.  Replaces an
 * earlier model. */
int ehm_explicit_set_noise(ehm_explicit* ex, int32_t n_terms, const int32_t* desc,
                           const double* data, int32_t n_data, int32_t n_d);
/* ehm_explicit_rollout with v, e and d drawn from the model (lib/simulator.py:160-180): at step t
 * v at the true state and the last commanded input (0 at t = 0), applied from t = 1; e and the
 * plant's d at the true state and the commanded input u, e = 0 where ||u||_2 = 0; the plant
 * steps with B (u + e) and E d; cost, u_norm_sum and u_traj stay the commanded input's.
 * Random numbers: Philox4x64-10, key (seed, 0), counter (traj0 + q, t, term, attempt) for
 * trajectory q.  Extra records (may be NULL): v_traj [T][n][p] (NaN after the step a trajectory
 * stopped at), e_traj [T][n][n_u], w_traj [T][n][n_d] (NaN from that step on). */
int ehm_explicit_rollout_noisy(ehm_explicit* ex, int64_t n, int32_t T, const double* x0,
                               uint64_t seed, uint64_t traj0, double tol_exit, double* x_traj,
                               double* u_traj, int32_t* leaf_traj, double* v_traj,
                               double* e_traj, double* w_traj, double* x_final, int32_t* steps,
                               int32_t* status, double* cost, double* u_norm_sum,
                               double* max_violation, double* kernel_seconds);
/* Raw Philox4x64-10 blocks on the current device: out[i] = philox(counters[i], key), counters
 * and out [n][4], key [2] (numpy: np.random.Philox(counter=c - 1, key=key).random_raw(4)). */
int ehm_philox_batch(int64_t n, const uint64_t* counters, const uint64_t* key, uint64_t* out);

/* ---- sampled audit of a law's epsilon-suboptimality (csrc/ehm_audit.hip) --------
 *
 * What the reference's PostProcessor asks of invariant_set.randomPoint after a partition: points
 * uniform in the partitioned set, the law as deployed priced at each of them against the implicit
 * law's optimal cost, and the contract  0 <= Vbar(x) - V*(x) <= max(eps_a, eps_r V*(x))  judged
 * per point.  A sampled check, not a certificate.
 *
 * The cells are the leaves the caller lists, in the order it lists them (for a flat export: the
 * leaves in ascending node id): cell_vertices [n_cells][p+1][p] (the handle keeps only their
 * inverses), cell_node [n_cells] their node ids.  Sample s -- a GLOBAL id, first + q for the q-th
 * sample of a call, so that neither the chunk size nor a split of the ids over calls or devices
 * changes a point -- takes its random words from Philox4x64-10 under the key (seed, 1) (the noise
 * model owns (seed, 0)): word k is word k % 4 of the block with counter (s, k / 4, 0, 0).  Word 0
 * chooses the cell, words 1..p become the uniforms g = (r >> 11) * 2^-53 in [0, 1).
 *   mode EHM_AUDIT_UNIFORM:  cdf [n_cells] = running sum of the cells' volumes; with
 *        t = u * cdf[n_cells - 1], u the uniform of word 0, the cell is the first i with
 *        cdf[i] > t (binary search), at most the last cell;
 *   mode EHM_AUDIT_PER_LEAF: the cell is s / k; every cell gets exactly k samples
 *        (first + n <= n_cells * k).
 * The point: the p uniforms sorted ascending (insertion sort) g_1 <= .. <= g_p, their spacings
 * w_0 = g_1, w_i = g_(i+1) - g_i, w_p = 1 - g_p as barycentric weights,
 * x_c = w_0 v_0c, then + w_i v_ic for i = 1..p in that order; every product and sum rounded once. */
#define EHM_AUDIT_UNIFORM  0
#define EHM_AUDIT_PER_LEAF 1
typedef struct ehm_audit_opts {
    int32_t mode;           /* EHM_AUDIT_UNIFORM | EHM_AUDIT_PER_LEAF                          */
    int32_t k;              /* samples per cell (per-leaf mode)                                */
    int64_t n;              /* samples of this call                                            */
    uint64_t first;         /* global id of its first sample                                   */
    uint64_t seed;
    int64_t n_cells;
    const double*  cell_vertices;   /* [n_cells][p+1][p]                                       */
    const int32_t* cell_node;       /* [n_cells] (the sampler alone does not read it)          */
    const double*  cdf;             /* [n_cells], uniform mode                                 */
    double rtol;            /* slack = rtol (1 + |V*|) on both sides of the contract           */
    double eps_a, eps_r;    /* the tolerances the law was built with                           */
    int64_t chunk;          /* samples per pass (0: 65536); the LP batches are this long       */
} ehm_audit_opts;
/* Statuses, the first that applies: 4 infeasible (no commutation feasible at x), 3 open (the
 * located leaf is not closed), 2 negative (not gap >= -slack), 1 violation (gap > bound + slack),
 * 0 within contract; gap = Vbar - V*, bound = max(eps_a, eps_r V*). */
typedef struct ehm_audit_result {
    int64_t counts[5];      /* samples by status                                               */
    int64_t relocated;      /* samples located in a leaf other than their cell                 */
    int64_t histogram[33];  /* of gap / bound over statuses 0-2: 32 bins over [0, 1] (negative
                               ratios in bin 0, ratio 1 in bin 31), bin 32 = above 1           */
    int64_t worst_id;       /* the sample with the largest gap / bound among statuses 0-2, the
                               smallest id on ties; -1: no such sample                         */
    int32_t worst_leaf;
    int32_t worst_cell;
    double  max_ratio;      /* its gap / bound (-inf: no such sample)                          */
    double  worst_vbar, worst_vstar, worst_bound;
    double  worst_x[8];
    double  seconds[3];     /* [0] sampling kernel, [1] locate + cost + reduce kernels (device
                               time), [2] the P_theta batches (host wall time)                 */
} ehm_audit_result;
/* Per-sample outputs of an audit, each [n] ([n][p] for x) or NULL. */
typedef struct ehm_audit_samples {
    double*  x;
    int32_t* cell;
    int32_t* leaf;          /* the located leaf                                                */
    double*  vbar;
    double*  wmin;          /* smallest barycentric weight of x in the located leaf            */
    double*  vstar;
    int32_t* delta_idx;
    int32_t* status;
} ehm_audit_samples;
/* The per-node data the audit prices the law with: vcost [n_nodes][p+1] and flags [n_nodes] (bit 0:
 * the node is closed) of the tree the handle was created from.  Replaces an earlier pair. */
int ehm_explicit_set_costs(ehm_explicit* ex, const double* vcost, const uint8_t* flags);
/* The sampler alone: x [n][p], cell [n] (either may be NULL).  Reads mode, k, n, first, seed, the
 * cells and chunk of opts. */
int ehm_explicit_sample(ehm_explicit* ex, const ehm_audit_opts* opts, double* x, int32_t* cell);
/* The audit: samples as ehm_explicit_sample draws them; each located with the walk of
 * ehm_explicit_eval_batch (root locator included), weights alpha in the located leaf, priced as
 * Vbar = alpha_0 c_0, then + c_(i+1) alpha_(i+1) in order (one rounding per operation, the order
 * of the input interpolation); V* and delta_idx from ehm_solve_pt_batch on `prob` (the points of
 * a chunk make one round trip through the host; prob must have the law's parameter dimension),
 * bit for bit what that entry point returns for the same points; statuses, counts and histogram
 * by integer atomics, the worst sample by a reduction with ties to the smaller id: no result
 * depends on the launch shape or the chunk size.  samples may be NULL.  Needs
 * ehm_explicit_set_costs.  Errors of the LP batches are reported through
 * ehm_explicit_last_error like the others. */
int ehm_explicit_audit(ehm_explicit* ex, ehm_problem* prob, const ehm_audit_opts* opts,
                       ehm_audit_result* result, const ehm_audit_samples* samples);
/* [v_0 (p) | inv([v_1 - v_0 .. v_p - v_0]) (p x p, row-major)] of every node as the handle holds
 * them: rec [n_nodes][p + p p].  What a host mirror needs to repeat the device's weights. */
int ehm_explicit_records(ehm_explicit* ex, double* rec);
/* ehm_abi_sizes for the structs of this section, in this order: ehm_audit_opts, ehm_audit_result,
 * ehm_audit_samples.  A list of its own: ehm_abi_sizes keeps returning the six it always has. */
int ehm_audit_abi_sizes(int64_t* sizes, int32_t n);

/* ---- audit of a law by the cost of the input it applies (csrc/ehm_applied.hip) ---
 *
 * At every point x the law's input ubar is priced by the fixed-first-input problem: V_u(x) = the
 * optimum of P_theta with u_0 = ubar, against V*(x) = P_theta(x).  `applied` holds that problem
 * (applied.applied_input_problem: the canonical form with the columns of u_0 moved to the
 * parameters, theta' = (x, ubar), p + n_u <= EHM_MAX_P), `oracle` the problem the law was built
 * for.  Both optima come from ehm_solve_pt_batch, bit for bit what it returns for the same points.
 *
 * Points: x [n][p] of the caller, or (x NULL) drawn as ehm_explicit_sample draws them in uniform
 * mode from the cells listed -- for a compiled law its roots -- with the same key (seed, 1) and the
 * same global ids first .. first + n - 1.
 * Input: of `law` (ehm_compiled_eval_batch: u and leaf are that entry point's, for a double and a
 * single law), else of `source` (ehm_explicit_eval_batch), else the caller's u [n][n_u].
 * Per sample (k_applied_pack): theta' = (x, ubar), with 0 in place of a component of ubar that is
 * not finite and the sample flagged; constant = 0 + cost_u[0] ubar_0 + cost_u[1] ubar_1 + .., one
 * rounding per operation; V_u = (optimum of `applied` at theta') + constant.
 * `applied` is the exact substitution.  opts->relaxed (may be NULL) is the same problem with its
 * rows widened by input_tol (applied_input_problem(can, input_tol)): a sample at which x is feasible
 * and no commutation of `applied` is, is solved again there, and if a commutation of `relaxed` is
 * feasible its optimum and commutation take the place of `applied`'s (the sample counts in
 * result->relaxed).  So the cost of an input that is admissible as it stands is never lowered by
 * the relaxation, and V_u >= V* holds for it in exact arithmetic. */
typedef struct ehm_applied_opts {
    int64_t n;              /* samples of this call                                            */
    uint64_t first;         /* global id of its first sample                                   */
    uint64_t seed;
    int64_t chunk;          /* samples per pass (0: 65536); the LP batches are this long       */
    int64_t n_cells;        /* drawn points: the cells                                         */
    const double* cell_vertices;    /* [n_cells][p+1][p]                                       */
    const double* cdf;              /* [n_cells] running sum of their volumes                  */
    const double* x;        /* the caller's points [n][p], or NULL: draw them                  */
    const double* u;        /* the caller's inputs [n][n_u] (law and source NULL)              */
    ehm_explicit* source;   /* the evaluator when law is NULL                                  */
    ehm_problem* relaxed;   /* the applied problem widened by input_tol, or NULL               */
    const double* cost_u;   /* [n_u] cost of u_0 that `applied` does not hold                  */
    int32_t p, n_u;         /* of the law; applied has p + n_u parameters                      */
    int32_t device;
    int32_t reserved;
    double rtol;            /* slack = rtol (1 + |V*|)                                         */
    double eps_a, eps_r;
} ehm_applied_opts;
/* Statuses, the first that applies: 5 infeasible (no commutation feasible at x), 4 no_law (an
 * input that is not finite), 3 inadmissible (x feasible, no commutation feasible with ubar
 * applied), 2 negative (not gap >= -slack), 1 violation (gap > bound + slack), 0 within;
 * gap = V_u - V*, bound = max(eps_a, eps_r V*). */
typedef struct ehm_applied_result {
    int64_t counts[6];      /* samples by status                                               */
    int64_t histogram[33];  /* of gap / bound over statuses 0-2, binned as ehm_audit_result's  */
    int64_t worst_id;       /* largest gap / bound among statuses 0-2, the smallest id on ties;
                               -1: no such sample                                              */
    int32_t worst_leaf;
    int32_t reserved;
    int64_t relaxed;        /* samples whose V_u comes from opts->relaxed                      */
    double  max_ratio;      /* -inf: no such sample                                            */
    double  worst_vu, worst_vstar, worst_bound;
    double  worst_x[8];
    double  worst_u[8];
    double  seconds[5];     /* [0] sampling kernel, [1] evaluation kernel, [2] pack + reduce
                               kernels (device time), [3] the P_theta batches of `oracle`,
                               [4] those of `applied` and `relaxed` (host wall time)           */
} ehm_applied_result;
/* Per-sample outputs, each [n] ([n][p] for x, [n][n_u] for u) or NULL.  root: the cell a drawn
 * point was drawn in, -1 for a caller's point; leaf: -1 for a caller's input. */
typedef struct ehm_applied_samples {
    double*  x;
    int32_t* root;
    int32_t* leaf;
    double*  u;
    double*  vu;
    double*  vstar;
    int32_t* delta_idx;
    int32_t* delta_idx_applied;
    int32_t* status;
    int32_t* relaxed;       /* 1 where V_u comes from opts->relaxed, else 0                    */
} ehm_applied_samples;
/* Statuses and counts by integer atomics, the worst sample by a reduction with ties to the smaller
 * id, no floating-point sum across samples: nothing reported depends on the launch shape or the
 * chunk size.  A law with test nodes is refused (EHM_E_INVALID).  samples may be NULL.  Errors,
 * those of the evaluators and of the LP batches included, are reported through
 * ehm_applied_last_error. */
int ehm_compiled_audit(ehm_compiled* law, ehm_problem* oracle, ehm_problem* applied,
                       const ehm_applied_opts* opts, ehm_applied_result* result,
                       const ehm_applied_samples* samples);
const char* ehm_applied_last_error(void);
/* ehm_abi_sizes for ehm_applied_opts, ehm_applied_result, ehm_applied_samples, in this order. */
int ehm_applied_abi_sizes(int64_t* sizes, int32_t n);

/* ---- leaf cells of a compiled law (csrc/ehm_certify.hip) --------------------------
 *
 * The simplex of every requested leaf, rebuilt from the law's own arrays (root_rec, root_entry,
 * node), and the input the leaf's own affine map gives at each of its vertices: what a certificate
 * of the law leaf by leaf starts from.  For double and single laws, compiled or imported.
 * leaf_ids [n]: rows of leaf_rec (0 .. n_leaf - 1; EHM_E_INVALID outside), or NULL: leaves 0 .. n - 1
 * (n <= n_leaf).  root_vertices [n_roots][p+1][p]: the roots' vertices, which the caller recovers
 * from root_rec (applied.root_cells: v_i = v_0 + column i of inv(inv(E))).
 * A leaf is walked up to its root through a parent table made on the device (the turns kept in a
 * set of EHM_CELL_MAX_DEPTH bits) and then down from the root's vertices: at a plane node
 * s_i = ((0 + a_0 v_i0) + .. + a_(p-1) v_i(p-1)) + b in double (float coefficients widened), exactly
 * one s_i > 0.5 and exactly one s_i < -0.5 are required -- the two ends of the bisected edge --, their
 * midpoint is (v + w) / 2 as ehm_split_batch computes it and replaces the negative-side vertex in
 * the left child, the positive-side one in the right child.
 * Outputs: vertices [n][p+1][p]; ubar [n][p+1][n_u] (may be NULL): the leaf map at every vertex in
 * the law's own arithmetic -- a double law u_0 + K (v - v_0) as ehm_compiled_eval_batch sums it, a
 * single law xs = (float) v and float sums, one rounding per product and per sum, widened;
 * status [n]: 0 a cell, 1 no_cell (a leaf deeper than EHM_CELL_MAX_DEPTH, a node that is no
 * bisection of the cell that reaches it, a leaf no root reaches), whose vertices and ubar are NaN.
 * A law with test nodes is refused (EHM_E_INVALID).  Errors through ehm_certify_last_error. */
#define EHM_CELL_MAX_DEPTH 256
#define EHM_CELL_OK        0
#define EHM_CELL_NO_CELL   1
int ehm_compiled_cells(ehm_compiled* law, const double* root_vertices, int64_t n,
                       const int32_t* leaf_ids, double* vertices, double* ubar, int32_t* status);
const char* ehm_certify_last_error(void);

/* ---- certificate of a compiled law leaf by leaf (csrc/ehm_certify.hip) ----------
 *
 * On a leaf the law is affine, and for a fixed commutation d the cost V_d(x, u(x)) of its input --
 * the optimum of the applied-input problem of section 3.8e with the commutation fixed -- is convex in
 * x.  With W_i its values at the p + 1 vertices of the leaf's cell,
 *     V_u(x) <= V_d(x, u(x)) <= sum_i alpha_i(x) W_i      on the cell,
 * so ehm_bar_e_batch(oracle, cell, Vbar = W) closing the cell proves
 *     V_u(x) - V*(x) < max(eps_a, eps_r V*(x))            at every state x of the leaf.
 * Per leaf: the cell and the vertex inputs (ehm_compiled_cells); theta' = (v_i, ubar_i) and the
 * constant 0 + cost_u[0] ubar_0 + .. packed on the device, a component of ubar that is not finite
 * replaced by 0 and the leaf flagged no_law; every (vertex, commutation) pair tested for feasibility
 * on `applied` (ehm_point_idx_batch, feas = 1, feasible iff tau <= 1e-8 as in the batched oracles);
 * a commutation feasible at all p + 1 vertices is a CANDIDATE (feasible on the cell by convexity of
 * the feasible set in (theta, u_0)); the candidates' vertex problems solved (feas = 0),
 * W_i = J_i + constant_i; a leaf without a candidate repeats both steps on opts->relaxed (may be
 * NULL) and is marked relaxed if that gives one: its certificate is for an input within input_tol
 * of the law's.  A candidate one of whose solves reports EHM_ST_STALLED is not tried.  The others
 * are ordered by ((0 + W_0) + .. ) + W_p ascending, the lowest index on ties, and tried in that
 * order, at most max_tries of them (0: all), until ehm_bar_e_batch closes the cell.  Any candidate
 * that closes it proves the statement: the order affects cost only.
 * Statuses, the first that applies: 4 no_cell, 3 no_law, 0 certified, 2 inadmissible (no
 * candidate, not even relaxed, and none set aside), 5 stalled (not certified, and a candidate was
 * set aside for a stalled solve), 1 uncertified (every try had t* >= 0: NOT a violation -- the
 * interpolation of a convex function is an upper bound, not the function). */
typedef struct ehm_certify_opts {
    int64_t n;                      /* leaves of this call                                     */
    const int32_t* leaf_ids;        /* [n] rows of leaf_rec, or NULL: leaves 0 .. n - 1        */
    const double* root_vertices;    /* [n_roots][p+1][p], as for ehm_compiled_cells            */
    int64_t chunk;                  /* leaves per pass (0: 8192); no result depends on it      */
    ehm_problem* relaxed;           /* the applied problem widened by input_tol, or NULL       */
    const double* cost_u;           /* [n_u] cost of u_0 that `applied` does not hold          */
    int32_t p, n_u;                 /* of the law; applied has p + n_u parameters              */
    int32_t n_delta;                /* commutations of oracle, applied and relaxed             */
    int32_t max_tries;              /* candidates tried per leaf (0: all)                      */
    int32_t device;
    int32_t reserved;
} ehm_certify_opts;
typedef struct ehm_certify_result {
    int64_t counts[6];              /* leaves by status                                        */
    int64_t relaxed;                /* leaves whose candidates come from opts->relaxed         */
    int64_t worst_leaf;             /* position in the call (0 .. n - 1) of the uncertified leaf
                                       with the largest tbest, the first on ties; -1: none     */
    double  worst_tbest;            /* NaN: none                                               */
    double  certified_volume;       /* sum of the certified cells' volumes, in leaf order      */
    double  cell_volume;            /* the same over every leaf that has a cell                */
    double  seconds[6];             /* [0] cell, pack and judge kernels (device time), then host
                                       wall time of [1] the feasibility batches, [2] the cost
                                       batches, [3] the tests, [4] the volumes, [5] the rest    */
} ehm_certify_result;
/* Per-leaf outputs, each [n] or NULL: delta_idx the closing commutation (-1: none), tbest of the
 * last try (NaN: none), tries made, relaxed 0 / 1, n_candidates (those set aside included),
 * volume of the cell (NaN: none); vertices [n][p+1][p], inputs [n][p+1][n_u], and W [n][p+1] the
 * vertex costs of the last candidate tried (NaN: none). */
typedef struct ehm_certify_leaves {
    int32_t* status;
    int32_t* delta_idx;
    double*  tbest;
    int32_t* tries;
    int32_t* relaxed;
    int32_t* n_candidates;
    double*  volume;
    double*  vertices;
    double*  inputs;
    double*  W;
} ehm_certify_leaves;
/* `oracle` is the problem the law was built for, `applied` the exact substitution
 * (applied.applied_input_problem).  Refusals as ehm_compiled_cells and ehm_compiled_audit (test
 * nodes, p + n_u > EHM_MAX_P, a law of another (p, n_u)).  leaves may be NULL. */
int ehm_compiled_certify(ehm_compiled* law, ehm_problem* oracle, ehm_problem* applied,
                         const ehm_certify_opts* opts, ehm_certify_result* result,
                         const ehm_certify_leaves* leaves);
/* ehm_abi_sizes for ehm_certify_opts, ehm_certify_result, ehm_certify_leaves, in this order. */
int ehm_certify_abi_sizes(int64_t* sizes, int32_t n);

/* ---- merging the leaves that apply one affine map (csrc/ehm_reduce.hip) ----------
 *
 * A new, independent law of the same precision and format in which every subtree whose leaves all
 * apply one affine map within tol is one leaf.  The REPRESENTATIVE of an internal record is its
 * leftmost leaf.  An internal record is MERGEABLE iff every leaf l below it has a cell
 * (ehm_compiled_cells: EHM_CELL_OK), the leaf mode of the representative (when leaf_mode is given)
 * and, at each of the p + 1 vertices v_i of l's OWN cell and for each input c,
 * !(|u_rep(v_i)_c - u_l(v_i)_c| <= tol[c]) false -- both maps in the law's own arithmetic as ubar of
 * ehm_compiled_cells, the difference in double; a difference that is NaN never passes.  Both maps are
 * affine, so the reduced law is within tol of the original at every state of every original cell;
 * the comparison is with the original leaves, so the bound does not grow with the levels merged.
 * The new leaves are the topmost mergeable records on each root path (a root entry may become a
 * leaf); a merged leaf takes the record, the leaf_node and the leaf_mode of its representative.
 * Surviving records keep their order (children still come after their parents); records no root
 * reaches are kept as they are; root_rec and nbr are copied.  The new law is checked as
 * ehm_compiled_import checks a file's arrays before it is returned.
 * root_vertices as for ehm_compiled_cells; tol [n_u], finite and >= 0 (0 merges only where the
 * computed difference is exactly zero); leaf_mode [n_leaf] or NULL.  Outputs: *out; leaf_mode_out
 * [n_leaf of the new law, at most n_leaf] (may be NULL; written only with leaf_mode); leaf_of [n_leaf]
 * (may be NULL) the new leaf record of every original one; counts [4] = leaves before and after,
 * internal records before and after; stats [2] = the largest difference that passed the test at any
 * record (an upper bound of the reduced law's deviation at the cells' vertices, <= tol), seconds.
 * EHM_E_INVALID for a law with test nodes, a tol that is negative or not finite, and a law whose
 * records form no forest (a record named by two parents or roots).  Errors through
 * ehm_reduce_last_error. */
int ehm_compiled_reduce(ehm_compiled* law, const double* root_vertices, const double* tol,
                        const int32_t* leaf_mode, ehm_compiled** out, int32_t* leaf_mode_out,
                        int32_t* leaf_of, int64_t* counts, double* stats);
const char* ehm_reduce_last_error(void);

/* ---- splitting the leaves of a compiled law (csrc/ehm_refine.hip) -----------------
 *
 * The inverse of ehm_compiled_reduce: a new, independent law of the same precision and format whose
 * selected leaves are bisected as the partitioner would have bisected their cells.  Both children of
 * a split leaf keep its leaf record, leaf_node and leaf_mode byte for byte, and a leaf record is
 * anchored (u = u_0 + K (x - v_0)), so the new law applies the same input, bit for bit, at every
 * state; only the cells get smaller.
 * One split: the cell as ehm_compiled_cells rebuilds it; its first longest edge (i, j), i < j, in
 * ehm_split_batch's arithmetic and order; the plane s = a . x + b with s(v_j) = +1, s(v_i) = -1 and
 * s = 0 at the other vertices from a p x p solve in double (rows v_k - v_i, k != i ascending; right-
 * hand side 2 for k = j, else 1; partial pivoting, the first largest modulus on ties; b = -1 - a . v_i;
 * one rounding per product and per sum), rounded to the law's scalar.  Left iff s >= -eps: the left
 * child is the partitioner's S_1 (the midpoint replaces v_i), the right child S_2.  The stored plane,
 * widened, must be finite (a single law: normal or zero) and at the cell's vertices pass the test of
 * ehm_compiled_cells with its positive end at j and its negative end at i; else the leaf is kept
 * whole (EHM_REFINE_UNSEPARATED).
 * The left child keeps the leaf's index l; with offset[l] the number of split leaves before l, the
 * right child is leaf n_leaf + offset[l] and the plane internal record n_int + offset[l]; the one
 * reference that named ~l (a child slot or a root entry) names the new record.  root_rec and nbr are
 * copied.  A level is one pass over the current leaves; a leaf's remaining levels go to both
 * children, minus one; passes are made until one splits nothing.
 * levels [n_leaf], each 0 .. EHM_REFINE_MAX_LEVELS; selected [n_leaf] (0 / 1) or NULL: all;
 * max_diameter (one number) and max_spread [n_u], each NULL or finite and >= 0: with neither, a
 * selected leaf is split while it has levels left; else only while one of them is exceeded on its own
 * cell -- the longest edge > *max_diameter, or for an input c max_i u_c(v_i) - min_i u_c(v_i) >
 * max_spread[c], the leaf map as ubar of ehm_compiled_cells; a NaN never splits.  root_vertices and
 * leaf_mode as for ehm_compiled_reduce.  The call could make at most worst = sum over the leaves of
 * 2^levels (selected) or 1 leaves: worst > max_leaves is refused before anything is allocated, and
 * the per-leaf outputs, each of `capacity` >= worst elements or NULL, are leaf_mode_out (written only
 * with leaf_mode), origin (the source leaf of every new leaf) and stop (EHM_REFINE_*, one per new
 * leaf).  counts [12] = leaves before and after, internal records before and after, passes that
 * split, leaves split, then the new leaves by stop code; stats [3] = the largest |s(v_k) - target_k|
 * of an accepted plane (measured, not gated), seconds, seconds of the plan kernels on the device.
 * EHM_E_INVALID for a law with test nodes, levels outside their range, a criterion that is negative
 * or not finite, and max_leaves exceeded.  Errors through ehm_refine_last_error. */
#define EHM_REFINE_MAX_LEVELS  16
#define EHM_REFINE_UNSELECTED  0   /* the leaf was not selected                                    */
#define EHM_REFINE_SATISFIED   1   /* levels done with no criterion, or every criterion met        */
#define EHM_REFINE_LEVELS      2   /* levels exhausted with a criterion still exceeded             */
#define EHM_REFINE_NO_CELL     3   /* the leaf has no cell                                         */
#define EHM_REFINE_UNSEPARATED 4   /* the stored plane failed the acceptance test                  */
#define EHM_REFINE_TOO_DEEP    5   /* at depth EHM_CELL_MAX_DEPTH: its children would have no cell */
#define EHM_REFINE_STOPS       6
int ehm_compiled_refine(ehm_compiled* law, const double* root_vertices, const int32_t* levels,
                        const uint8_t* selected, const double* max_diameter,
                        const double* max_spread, const int32_t* leaf_mode, int64_t max_leaves,
                        int64_t capacity, ehm_compiled** out, int32_t* leaf_mode_out,
                        int32_t* origin, int8_t* stop, int64_t* counts, double* stats);
const char* ehm_refine_last_error(void);

/* ---- one-step invariance leaf by leaf (csrc/ehm_invariance.hip) -------------------
 *
 * On a leaf the law is affine and in the leaf's step-0 mode the plant x+ = A_m x + B_m u + w_m + E d
 * is affine in (x, u, d), so (x, d) -> x+ is affine on cell x box: the image of the leaf under every
 * disturbance of the box [d_lo, d_hi] is the convex hull of the successors at the (p + 1) n_c points
 * (cell vertex i, box corner j), n_c = 2^n_d (n_d = 0: no box, no E term, n_c = 1).  The entry takes
 * its own copies of the plant; it does not read the handle's rollout attachment.
 * Per requested leaf l (leaf_ids and root_vertices as for ehm_compiled_cells), one device thread:
 *  1. the cell V and u_i, the leaf's own map at v_i: vertices and ubar of ehm_compiled_cells;
 *  2. m = leaf_mode[l];
 *  3. for every vertex i and region row r of mode m (region_rows [n_modes], H and h stacked by mode):
 *     s = ((0 + H_r0 v_0) + ..); the vertex is in the region iff s <= h_r + tol_exit;
 *  4. y_i[k] = (((0 + A_k0 v_0 + ..) + B_k0 u_0 + ..) + w_k);
 *  5. corner j takes d_b = d_hi[b] where bit b of j is set, else d_lo[b];
 *     x+_ij[k] = y_i[k] + E_k0 d_0 + .. in that order -- bit for bit what ehm_compiled_rollout
 *     writes for the state v_i, the input u_i, mode m and the disturbance d_j;
 *  6. x+_ij is located as one rollout step locates its state: with an adjacency table the visibility
 *     walk started at the leaf's own root, else (or when the walk does not accept a root) the first
 *     root that contains it, else the last; its weights (a0, alpha) are taken in that root;
 *  7. margin_ij = min(a0, alpha_*) (a weight that is NaN is taken); x+_ij is INSIDE iff every weight
 *     is >= -tol_exit (a NaN fails);
 *  8. viol_ij = max_r (Gx_r . x+_ij - gx_r) from -inf, rows summed as in step 3 (n_g = 0: -inf).
 * Status, the first that applies: 4 no_cell; 3 no_mode (m < 0 or m >= n_modes); 2 mode_region (a
 * cell vertex fails a region row of m); 1 exits (some x+_ij is not inside); 0 invariant.
 * Per-leaf outputs (required): status; margin, the minimum of margin_ij in (i, j) order, the first on
 * ties, a NaN before any number (NaN without a cell or mode); worst = i n_c + j of that pair (-1);
 * max_violation, the maximum of viol_ij (NaN without a cell or mode).  Optional, each may be NULL:
 * x_next [n][p+1][n_c][p]; succ_root [n][p+1][n_c], the root of step 6 (-1 where x+_ij is not
 * inside); succ_leaf, the row of leaf_rec the law's walk from that root ends in for x+_ij (-1
 * likewise): the transition relation of the vertices.  Rows of a leaf without a cell or mode are NaN
 * and -1.  margin is in units of the chosen root's weights: for a point outside it orders leaves, it
 * is no distance.
 * Result: counts by status (integer atomics on the device); worst_leaf, the position in the call of
 * the leaf of status 0 or 1 with the smallest margin, the first on ties (-1, NaN: none);
 * invariant_volume and cell_volume, the volumes (ehm_volume_batch) of the invariant leaves and of
 * every leaf with a cell summed in leaf order; seconds, the device time of the kernel.  The leaves
 * are processed chunk at a time (0: as many as keep x_next of a pass within 128 MiB); no result
 * depends on the chunk.
 * EHM_E_INVALID for a law with test nodes, n_u > 4, n_d > 8, n_modes > 4, more than 256 region rows
 * or constraint rows, d_lo > d_hi or a bound that is not finite, a box without E, a leaf_ids entry
 * outside the law (named in the message), a required array that is NULL, tol_exit negative or NaN.
 * Errors through ehm_invariance_last_error. */
typedef struct ehm_invariance_opts {
    int64_t n;                      /* leaves of this call                                     */
    const int32_t* leaf_ids;        /* [n] rows of leaf_rec, or NULL: leaves 0 .. n - 1        */
    const double* root_vertices;    /* [n_roots][p+1][p], as for ehm_compiled_cells            */
    int64_t chunk;                  /* leaves per pass (0: see above)                          */
    const double* A;                /* [n_modes][p][p]                                         */
    const double* B;                /* [n_modes][p][n_u]                                       */
    const double* w;                /* [n_modes][p]                                            */
    const double* E;                /* [p][n_d], NULL with n_d = 0                             */
    const int32_t* region_rows;     /* [n_modes] rows of every mode's region, NULL: none       */
    const double* H;                /* [rows][p] stacked by mode                               */
    const double* h;                /* [rows]                                                  */
    const double* Gx;               /* [n_g][p]                                                */
    const double* gx;               /* [n_g]                                                   */
    const int32_t* leaf_mode;       /* [n_leaf] step-0 mode of every leaf, -1: none            */
    const double* d_lo;             /* [n_d]                                                   */
    const double* d_hi;             /* [n_d]                                                   */
    double tol_exit;
    int32_t n_modes, n_d, n_g, reserved;
} ehm_invariance_opts;
typedef struct ehm_invariance_result {
    int64_t counts[5];
    int64_t worst_leaf;
    double  worst_margin;
    double  invariant_volume;
    double  cell_volume;
    double  seconds;
} ehm_invariance_result;
typedef struct ehm_invariance_leaves {
    int32_t* status;
    double*  margin;
    int32_t* worst;
    double*  max_violation;
    double*  x_next;
    int32_t* succ_root;
    int32_t* succ_leaf;
} ehm_invariance_leaves;
int ehm_compiled_successors(ehm_compiled* law, const ehm_invariance_opts* opts,
                            ehm_invariance_result* result, const ehm_invariance_leaves* leaves);
const char* ehm_invariance_last_error(void);
/* ehm_abi_sizes for ehm_invariance_opts, ehm_invariance_result, ehm_invariance_leaves, in this
 * order. */
int ehm_invariance_abi_sizes(int64_t* sizes, int32_t n);

/* ---- the invariant core of a compiled law (csrc/ehm_core.hip) ---------------------
 * (no counterpart in the reference)
 *
 * The may-reach relation between the leaves and its fixed point.  On a leaf L with mode m the image
 * under every disturbance of the box is I(L) = hull{y_i} + E [d_lo, d_hi], y_i the p + 1 vertex
 * successors of ehm_compiled_successors before the disturbance (its step 4, bit for bit).  An affine
 * f = g . x + h has over I(L) the maximum max_i f(y_i) + sum_k max(gE_k d_lo_k, gE_k d_hi_k),
 * gE_k = ((0 + g_0 E_0k) + ..), and the minimum with min in both places.
 * `plant` is an ehm_invariance_opts of which root_vertices, A, B, w, E, leaf_mode, d_lo, d_hi,
 * n_modes, n_d and chunk are read (n_d up to 64 here: no corner is enumerated; chunk: the leaves
 * whose cells go to the host at a time for their volumes, 0: 65536, and no result depends on it);
 * the rest is ignored.
 * The row of leaf l -- built when l has a cell and a mode and (rows = EHM_CORE_ROWS_ALL or
 * status[l] = 0) -- lists, roots ascending and below a root left before right, every leaf reached by:
 *  1. root r is a candidate iff its bounding box, widened per coordinate by (p + 1) tol_side times
 *     its extent, meets the image's, and no barycentric weight of r (the sums of the [v0 | inv(E)]
 *     record at the y_i, the rows of inv(E) as g) has its maximum over I(L) below -tol_side;
 *  2. from the entry of a candidate: at a plane node with s = a . x + b visit the left child iff
 *     smax >= -eps_T - tol_side - w, the right child iff smin < -eps_T + tol_side + w; eps_T is 2^-52
 *     for a double law and 2^-23 for a single law, w = 0 for a double law and
 *     (p + 3) 2^-24 ((0 + |a_0| X_0 + ..) + |b|) + 2^-126 for a single law, X_c the largest |x_c| of
 *     the image's bounding box.
 * A row longer than max_fan is cut off: it is empty and the leaf's status is 5 (unresolved).  If the
 * rows together hold more than max_edges (at most 2^31 - 1) the call fails with EHM_E_CAPACITY and
 * the message names the total.
 * level [n_leaf]: 0 for a seed (status other than 0 after the above), k >= 1 for a leaf not of a
 * lower level whose row names a leaf of level k - 1, -1 for the core, the leaves never reached.
 * status [n_leaf]: the caller's with 5 where a row was cut off.  counts: core, level >= 1, then the
 * seeds by status 1 .. 5.  n_sweeps = the largest level + 1.  core_volume and cell_volume through
 * ehm_volume_batch, summed in leaf order.  seconds_reach: device time of the two passes of the
 * relation; seconds_sweeps: wall time of the fixed point.  With want_edges: indptr [n_leaf + 1]
 * (caller's) and *indices_out, the rows' leaves in page-locked memory the caller releases with
 * ehm_host_free.
 * EHM_E_INVALID as ehm_compiled_successors for the law, the plant and the box; for n_status other
 * than the law's leaves, a status outside 0 .. 4, tol_side negative or NaN, max_fan < 1, a negative
 * chunk.  Errors through ehm_core_last_error. */
#define EHM_CORE_ROWS_INVARIANT 0
#define EHM_CORE_ROWS_ALL 1
typedef struct ehm_core_opts {
    const int32_t* status;          /* [n_status] the one-step status of every leaf            */
    int64_t n_status;               /* must be the law's n_leaf                                */
    int64_t max_edges;
    double  tol_side;
    int32_t max_fan, rows, want_edges, reserved;
} ehm_core_opts;
typedef struct ehm_core_result {
    int64_t counts[7];
    int64_t n_edges;
    int64_t n_sweeps;
    double  core_volume;
    double  cell_volume;
    double  seconds_reach;
    double  seconds_sweeps;
} ehm_core_result;
typedef struct ehm_core_leaves {
    int32_t*  level;                /* [n_leaf]                                                */
    int32_t*  status;               /* [n_leaf]                                                */
    int64_t*  indptr;               /* [n_leaf + 1], with want_edges                           */
    int32_t** indices_out;          /* with want_edges                                         */
} ehm_core_leaves;
int ehm_compiled_core(ehm_compiled* law, const ehm_invariance_opts* plant,
                      const ehm_core_opts* opts, ehm_core_result* result,
                      const ehm_core_leaves* leaves);
const char* ehm_core_last_error(void);
/* ehm_abi_sizes for ehm_core_opts, ehm_core_result, ehm_core_leaves, in this order. */
int ehm_core_abi_sizes(int64_t* sizes, int32_t n);

/* ---- one-step invariance and the core under measurement and input error (csrc/ehm_robust.hip,
 * csrc/ehm_core.hip) -------------------------------------------------------------
 * (no counterpart in the reference)
 *
 * The closed loop of ehm_compiled_rollout_noisy evaluates the law at the measured state z = x + v,
 * tests the mode's region rows on the true state x = z - v and steps the plant with u + e.  With d, v
 * and e in boxes the measured state's successor on leaf L of mode m is
 *     z+ = [A_m z + B_m u(z) + w_m] + E d - A_m v + B_m e + v'          (v' in the box of v),
 * so its image is I(L) = hull{y_i} + G_m [g_lo, g_hi]: y_i the p + 1 vertex successors of
 * ehm_compiled_successors before the disturbance (its step 4, bit for bit), G_m = [E | -A_m | B_m | I]
 * [p][n_g], n_g = n_d + 2 p + n_u, the box [d; v; e; v].  The columns of v (both blocks) and of e are
 * there only where the box is given (v_lo / v_hi, e_lo / e_hi: both NULL for none), so n_g shrinks
 * accordingly; n_g <= 64.  The v and e boxes must hold 0.
 * `plant` is an ehm_invariance_opts of which n, leaf_ids, root_vertices, chunk, A, B, w, E,
 * region_rows, H, h, leaf_mode, d_lo, d_hi, tol_exit, n_modes and n_d (up to 64) are read.
 *
 * ehm_compiled_robust_successors: facets [n_facets][p+1] are the boundary facets of the roots' union,
 * row f = [n_f | c_f], n_f a unit normal, the inner side n_f . x >= c_f.  A small kernel first fills
 * slack[f][m] = sum_k min(nG_k g_lo_k, nG_k g_hi_k) from 0, nG_k = ((0 + n_f0 G_m[0][k]) + ..).  Per
 * requested leaf, one device thread:
 *  1. the cell and m as ehm_compiled_successors;
 *  2. region row r of mode m holds iff  max_i ((0 + H_r0 v_i0) + ..) + rs_r <= h_r + tol_exit,
 *     rs_r = sum_c max((-H_rc) v_lo_c, (-H_rc) v_hi_c) from 0 (0 without a v box), the maximum taken
 *     in vertex order;
 *  3. y_i as step 4 of ehm_compiled_successors;
 *  4. for every facet f in order: mn_f = min_i ((0 + n_f0 y_i0) + ..), the first on ties, a NaN before
 *     any number; val_f = (mn_f - c_f) + slack[f][m]; the facet holds iff
 *     val_f >= -(tol_set * max|root_vertices|) (a NaN fails).
 * Status, the first that applies: 4 no_cell; 3 no_mode; 2 mode_region (a region row fails); 1 exits (a
 * facet fails); 0 invariant.  margin: the minimum of val_f in facet order, the first on ties, a NaN
 * before any number (NaN without a cell or mode) -- a distance in state units, no threshold applied;
 * worst = f (p + 1) + i of the facet and the vertex that give it (-1).  Result: counts, worst_leaf,
 * worst_margin, the volumes and seconds as ehm_compiled_successors; seconds_slack, the device time
 * of the slack kernel; n_generators.  No result depends on the chunk (0: 65536 leaves per pass).
 * Where the union is not convex the facets bound nothing: the caller says so, the call is the same.
 *
 * ehm_compiled_robust_core: ehm_compiled_core with G_m of the leaf's mode in the place of E and the
 * stacked box in the place of [d_lo, d_hi]; everything else -- the candidate roots, the traversal,
 * tol_side, the single law's widening, max_fan, max_edges, the fixed point, the outputs -- is
 * ehm_compiled_core's.  `opts->status` is the one-step status of ehm_compiled_robust_successors.
 *
 * EHM_E_INVALID, before the device is touched: as ehm_compiled_successors for the law and the plant;
 * n_g > 64; a box with lo > hi or a bound that is not finite; a v or e box without 0 or with one
 * bound NULL; n_facets < 1 or n_facets (p + 1) >= 2^31 (robust_successors); tol_set negative or NaN;
 * a required array that is NULL.  Errors through ehm_robust_last_error (robust_successors) and
 * ehm_core_last_error (robust_core). */
typedef struct ehm_robust_opts {
    const double* facets;           /* [n_facets][p+1]; not read by ehm_compiled_robust_core   */
    int64_t n_facets;
    const double* v_lo;             /* [p] or NULL                                             */
    const double* v_hi;
    const double* e_lo;             /* [n_u] or NULL                                           */
    const double* e_hi;
    double tol_set;
} ehm_robust_opts;
typedef struct ehm_robust_result {
    int64_t counts[5];
    int64_t worst_leaf;
    double  worst_margin;
    double  invariant_volume;
    double  cell_volume;
    double  seconds;
    double  seconds_slack;
    int32_t n_generators, reserved;
} ehm_robust_result;
typedef struct ehm_robust_leaves {
    int32_t* status;
    double*  margin;
    int32_t* worst;
} ehm_robust_leaves;
int ehm_compiled_robust_successors(ehm_compiled* law, const ehm_invariance_opts* plant,
                                   const ehm_robust_opts* opts, ehm_robust_result* result,
                                   const ehm_robust_leaves* leaves);
int ehm_compiled_robust_core(ehm_compiled* law, const ehm_invariance_opts* plant,
                             const ehm_robust_opts* robust, const ehm_core_opts* opts,
                             ehm_core_result* result, const ehm_core_leaves* leaves);
const char* ehm_robust_last_error(void);
/* ehm_abi_sizes for ehm_robust_opts, ehm_robust_result, ehm_robust_leaves, in this order. */
int ehm_robust_abi_sizes(int64_t* sizes, int32_t n);

/* ---- the same two checks with per-leaf error boxes (csrc/ehm_radii_dev.h, csrc/ehm_robust.hip,
 * csrc/ehm_core.hip) ---------------------------------------------------------------
 * (no counterpart in the reference)
 *
 * The boxes of d, v, e and v' are no longer one per call but one per leaf, made on the device from
 * the packed uncertainty model that ehm_compiled_set_noise takes (desc [n_terms][8], data [n_data]):
 * on leaf L every error is bounded at the states and inputs L itself can see.  box_K(a, b) is the
 * interval hull of kind K over every draw at |x| <= a, |u| <= b: terms in model order, sums from 0.0,
 * a box term adds mid -+ rad (mid = sum_k M_ik c_k, rad = sum_k |M_ik| h_k), a ball term -+ r dual_i
 * with r the sampler's radius at |F| and a or b, dual_i the dual norm of row i of L.  Per leaf, one
 * device thread (k_leaf_radii):
 *  1. c_L[c] = max_i |V_ic| over the cell's vertices, ubar_L[k] = max_i |u_k(V_i)| (the leaf's map in
 *     the law's arithmetic), the y_i as ehm_compiled_successors' step 4;
 *  2. a = x_abs; radius_iters times a <- min(a, c_L + vhalf(a, u_abs)), vhalf the larger modulus of
 *     the two bounds of box_state: a_L;
 *  3. v_L = box_state(a_L, u_abs), e_L = box_input(a_L, ubar_L), d_L = box_process(a_L, ubar_L);
 *  4. xplus_L = max_i |y_i| + |E| dmax_L + |A_m| vmax_L + |B_m| emax_L (in that order, column by
 *     column), a'_L = min(x_abs, xplus_L), v'_L = box_state(a'_L, ubar_L).
 * x_abs and u_abs are the caller's global bounds on every true state and every commanded input; they
 * must be valid (the Python layer verifies x_abs), the iteration only ever lowers them.  The image is
 * I(L) = hull{y_i} + G_m [d_L; v_L; e_L; v'_L]; a kind without terms has no columns in G_m.  A facet's
 * value is (mn_f - c_f) + sum_k min(nG[f][m][k] lo_k(L), nG[f][m][k] hi_k(L)) from 0 in k order,
 * nG[f][m][k] = ((0 + n_f0 G_m[0][k]) + ..) from a small kernel; the region rows are tested on
 * cell - v_L.  Statuses, margin, worst, counts, volumes and the core are those of the entry points
 * above, read leaf by leaf.  d_lo / d_hi of `plant` and the v / e bounds of `robust` are not read.
 *
 * ehm_compiled_robust_successors_leaf: `leaf_boxes` (may be NULL) takes, per requested leaf, the boxes
 * and bounds; an array that is NULL, or whose kind has no terms, is not written; seconds_radii is the
 * device time of k_leaf_radii, result->seconds_slack that of the nG table.
 * ehm_compiled_robust_core_leaf: makes the boxes of all leaves on the device itself (their time is part
 * of seconds_reach) and reads them in a third set of the relation's kernels.
 *
 * EHM_E_INVALID, before the device is touched: everything the entry points above refuse; more than 16
 * terms or a bad descriptor (the message names the term); model dimensions that are not the plant's;
 * n_d > 8; radius_iters outside 1..16; x_abs or u_abs NULL, negative or not finite; a model whose
 * constant part of the v or e box (box_K(0, 0)) does not hold 0; n_g > 64; plant, generators, bounds
 * and model together above 8192 doubles of LDS.  Errors through ehm_robust_last_error
 * (robust_successors_leaf) and ehm_core_last_error (robust_core_leaf). */
typedef struct ehm_robust_radii {
    const int32_t* desc;            /* [n_terms][8]                                            */
    const double*  data;            /* [n_data]                                                */
    const double*  x_abs;           /* [p]                                                     */
    const double*  u_abs;           /* [n_u]                                                   */
    int32_t n_terms, n_data;
    int32_t n_x, n_u, n_d;          /* the model's dimensions                                  */
    int32_t radius_iters;
} ehm_robust_radii;
typedef struct ehm_robust_leaf_boxes {
    double* d;                      /* [n][2][n_d]: lo, hi                                     */
    double* v;                      /* [n][2][p]                                               */
    double* e;                      /* [n][2][n_u]                                             */
    double* v_next;                 /* [n][2][p]                                               */
    double* x_abs_leaf;             /* [n][p]    a_L                                           */
    double* x_next_abs;             /* [n][p]    a'_L                                          */
    double* u_abs_leaf;             /* [n][n_u]  ubar_L                                        */
    double  seconds_radii;          /* written by the call                                     */
} ehm_robust_leaf_boxes;
int ehm_compiled_robust_successors_leaf(ehm_compiled* law, const ehm_invariance_opts* plant,
                                        const ehm_robust_opts* robust,
                                        const ehm_robust_radii* radii, ehm_robust_result* result,
                                        const ehm_robust_leaves* leaves,
                                        ehm_robust_leaf_boxes* leaf_boxes);
int ehm_compiled_robust_core_leaf(ehm_compiled* law, const ehm_invariance_opts* plant,
                                  const ehm_robust_opts* robust, const ehm_robust_radii* radii,
                                  const ehm_core_opts* opts, ehm_core_result* result,
                                  const ehm_core_leaves* leaves);
/* ehm_abi_sizes for ehm_robust_radii, ehm_robust_leaf_boxes, in this order. */
int ehm_robust_radii_abi_sizes(int64_t* sizes, int32_t n);

/* ---- reach tube and limit set of the closed loop (csrc/ehm_reach.hip) -------------
 * (no counterpart in the reference)
 *
 * The forward analysis of a may-reach relation between the first n_leaf leaf records of a law
 * (n_leaf at most the law's), given as host CSR (indptr, indices: what ehm_compiled_core returns with
 * want_edges, or any other relation), with `level` [n_leaf] (0: a seed) and the start rows.  A seed is
 * absorbing: F(l) is the row of l for a non-seed and empty for a seed, whether or not the relation
 * has a row for it; post(X) is the union of F over X.
 *  A. arrival [n_leaf]: the smallest k >= 0 with l in post^k(S), -1 if there is none, by sweeps
 *     k = 1, 2, .. (a row with arrival k - 1 writes k into every target without an arrival) until a
 *     sweep reaches nothing new or max_sweeps sweeps were made (arrival_done = 0).  n_arrival: the
 *     largest arrival.  leak_step: the smallest arrival of a seed, -1 without one.
 *  B. only with arrival_done and leak_step = -1: D_0 = {arrival >= 0}, D_(j+1) = post(D_j), until
 *     D_(j+1) = D_j or D_(j+1) is empty (settle_done = 1; settle = j resp. j + 1) or max_sweeps sweeps
 *     were made (settle_done = 0, settle = the sweeps made).  depart [n_leaf]: the first j >= 1 with l
 *     not in D_j, -1 for the leaves of the last set and those outside D_0.  limit [n_leaf]: the last
 *     D_j (all 0 when phase B did not run).
 *  C. R_0 = S, R_(k+1) = post(R_k) for k = 0 .. n_steps - 1, n_steps - 1 = horizon, cut at leak_step
 *     where there is one and at max_sweeps where phase A did not finish.  steps [n_steps][n_leaf]
 *     with want_steps.
 * Boxes: leaf_box [2][p][n_leaf] (lo then hi, leaf-fastest; may be NULL) holds per coordinate the
 * smallest and largest vertex coordinate of the leaf's cell (ehm_compiled_cells), NaN without a cell;
 * the box of a set takes the minimum and maximum over its leaves that have a cell, NaN for none, and
 * adds 0.0 to each bound (a zero is +0).  tube_box [n_arrival + 1][2][p]: of {0 <= arrival <= k};
 * settle_box [settle + 1][2][p]: of D_j; step_box [n_steps][2][p]: of R_k; the counts beside them are
 * the sets' sizes.  The caller's tube and settle arrays hold min(max_sweeps, n_leaf) + 1 rows, the
 * step arrays horizon + 1.
 * row_map: how the rows are walked, one thread per row (EHM_REACH_MAP_THREAD) or one wavefront per
 * row, the lanes striding it (EHM_REACH_MAP_WAVE); no result depends on it.
 * seconds_boxes / _arrival / _settle / _steps: device time of the phases; seconds_upload: wall time of
 * checking, narrowing and uploading the relation.
 * EHM_E_INVALID, before the device is touched: a NULL argument or required array; a law with test
 * nodes; n_leaf < 1 or above the law's; indptr[0] != 0, a decreasing indptr, indptr[n_leaf] other
 * than n_edges, n_edges >= 2^31; an index outside 0 .. n_leaf - 1; n_level other than n_leaf; an
 * empty start or a start row out of range; horizon < 0; max_sweeps < 1; a row_map that is neither;
 * want_steps with (horizon + 1) n_leaf > 2^28.  Errors through ehm_reach_last_error. */
#define EHM_REACH_MAP_THREAD 0
#define EHM_REACH_MAP_WAVE 1
typedef struct ehm_reach_opts {
    const double*  root_vertices;   /* [n_roots][p+1][p], as for ehm_compiled_cells            */
    const int64_t* indptr;          /* [n_leaf + 1]                                            */
    const int32_t* indices;         /* [n_edges]                                               */
    const int32_t* level;           /* [n_level]                                               */
    const int32_t* start;           /* [n_start] rows of the leaf records                      */
    int64_t n_leaf, n_edges, n_level, n_start;
    int64_t max_sweeps;
    int32_t horizon, want_steps, row_map, reserved;
} ehm_reach_opts;
typedef struct ehm_reach_result {
    int64_t n_arrival, leak_step, settle, n_steps;
    int64_t sweeps_arrival, sweeps_settle;
    int32_t arrival_done, settle_done;
    double  seconds_boxes, seconds_arrival, seconds_settle, seconds_steps, seconds_upload;
} ehm_reach_result;
typedef struct ehm_reach_leaves {
    int32_t* arrival;               /* [n_leaf]                                                */
    int32_t* depart;                /* [n_leaf]                                                */
    uint8_t* limit;                 /* [n_leaf]                                                */
    uint8_t* steps;                 /* [horizon + 1][n_leaf], with want_steps                  */
    double*  leaf_box;              /* [2][p][n_leaf] or NULL                                  */
    double*  tube_box;
    int64_t* tube_count;
    double*  settle_box;
    int64_t* settle_count;
    double*  step_box;
    int64_t* step_count;
} ehm_reach_leaves;
int ehm_compiled_reach(ehm_compiled* law, const ehm_reach_opts* opts, ehm_reach_result* result,
                       const ehm_reach_leaves* leaves);
const char* ehm_reach_last_error(void);
/* ehm_abi_sizes for ehm_reach_opts, ehm_reach_result, ehm_reach_leaves, in this order. */
int ehm_reach_abi_sizes(int64_t* sizes, int32_t n);

/* ---- certified fuel bounds of the closed loop (csrc/ehm_cost.hip) ----------------
 * (no counterpart in the reference)
 *
 * Upper and lower bounds of the summed input 2-norm of every trajectory over k = 0 .. horizon steps,
 * by a max-plus and a min-plus dynamic program over a relation between the first n_leaf leaf records
 * of a law, given as for ehm_compiled_reach.  domain [n_domain] and start [n_start] are rows of the
 * leaf records (a row named twice is one row); the start set lies in the domain.  The domain D holds
 * no seed (level 0) and is closed under the relation; the device checks both and the call is
 * refused with "row r is a seed" or "row r of the domain reaches leaf t outside it", r the smallest
 * such row and t its smallest such target.
 * Weights, per leaf of D, by the device unless w_hi and w_lo [n_leaf] are both given (then they are
 * read on D, must be finite with w_lo <= w_hi there, and pad is 0): with u(v) the leaf's own map at
 * the p + 1 vertices of its cell in the law's arithmetic (ehm_compiled_cells' ubar) and |.| the
 * 2-norm as the rollout takes it (squares summed in ascending component order, sqrt, in double),
 *   w_hi = max_v |u(v)| + pad,  w_lo = max(0, |g| - pad),  g_c = max(0, min_v u_c(v), -max_v u_c(v)),
 *   pad = (2 p + n_u + 8) eps_T |R|,  R_c = |u0_c| + sum_j |K_cj| (max_v |v_j - v0_j| + x_j),
 * eps_T = 2^-53 and x_j = 0 for a double law, eps_T = 2^-24 and x_j = max_v |v_j| for a single one
 * (whose state is narrowed before the offset is taken).  A leaf of D without a cell is refused by
 * name.
 * Recurrence on D: U_0 = L_0 = 0; U_(k+1)(l) = w_hi[l] + max over t in row(l) of U_k(t);
 * L_(k+1)(l) = w_lo[l] + min over the row of L_k(t); an empty row contributes 0.  The leaves'
 * arrays are NaN outside D: w_hi, w_lo, pad, hi = U_horizon, lo = L_horizon.  max_hi, min_lo
 * [horizon + 1]: over D for every k; start_hi, start_lo: over the start set.  With want_paths
 * (horizon n_leaf 4 <= 2^28 bytes per direction): path_hi / path_lo int32 [horizon + 1] start at
 * the smallest leaf of the start set that attains start_hi[horizon] / start_lo[horizon] and follow
 * the smallest leaf that attains the max / min of each row, -1 after an empty row.
 * seconds_weights, seconds_sweeps: device time; seconds_upload: wall time of checking, narrowing
 * and uploading the relation.
 * EHM_E_INVALID, before the device is touched: what ehm_compiled_reach refuses of a law and of a
 * relation; n_u > 4; horizon < 1; an empty domain or start set, a row of either out of range, a
 * start row outside the domain; only one of w_hi, w_lo; a weight on D that is not finite or
 * w_lo > w_hi; the bytes of the paths.  Errors through ehm_cost_last_error. */
typedef struct ehm_cost_opts {
    const double*  root_vertices;   /* [n_roots][p+1][p], as for ehm_compiled_cells            */
    const int64_t* indptr;          /* [n_leaf + 1]                                            */
    const int32_t* indices;         /* [n_edges]                                               */
    const int32_t* level;           /* [n_level]                                               */
    const int32_t* domain;          /* [n_domain] rows of the leaf records                     */
    const int32_t* start;           /* [n_start] rows of the leaf records                      */
    const double*  w_hi;            /* [n_leaf] or NULL: both or neither                       */
    const double*  w_lo;
    int64_t n_leaf, n_edges, n_level, n_domain, n_start;
    int32_t horizon, want_paths;
} ehm_cost_opts;
typedef struct ehm_cost_result {
    int64_t n_domain, n_start;      /* distinct rows                                           */
    double  seconds_weights, seconds_sweeps, seconds_upload;
} ehm_cost_result;
typedef struct ehm_cost_leaves {
    double*  w_hi;                  /* [n_leaf]                                                */
    double*  w_lo;
    double*  pad;
    double*  hi;
    double*  lo;
    double*  max_hi;                /* [horizon + 1]                                           */
    double*  min_lo;
    double*  start_hi;
    double*  start_lo;
    int32_t* path_hi;               /* [horizon + 1], with want_paths                          */
    int32_t* path_lo;
} ehm_cost_leaves;
int ehm_compiled_cost(ehm_compiled* law, const ehm_cost_opts* opts, ehm_cost_result* result,
                      const ehm_cost_leaves* leaves);
const char* ehm_cost_last_error(void);
/* ehm_abi_sizes for ehm_cost_opts, ehm_cost_result, ehm_cost_leaves, in this order. */
int ehm_cost_abi_sizes(int64_t* sizes, int32_t n);

/* ---- closed-loop simulation under the COMPILED law (csrc/ehm_compiled.hip) -------
 *
 * The entry points of the explicit law's rollout, argument for argument, on a compiled law -- also
 * one that was only ever imported.  leaf_mode [n_leaf] (the order of leaf_rec) takes the place of
 * node_mode [n_nodes]: the step-0 mode of every leaf's commutation, -1: none (status 3).  The mode
 * table, the plant and the model are attachments of the handle for its rollouts: they are not part
 * of the law (ehm_compiled_info's bytes, ehm_compiled_export).  Refusals as the explicit law's
 * (NULL arrays, limits, n_u <= 4, a mode >= n_modes for the nominal plant, the LDS cap, a noisy
 * guarded plant, d without E), and a law with test nodes (header n_test > 0) is refused by both
 * plant setters with EHM_E_INVALID.
 * A step: measure z = x + v (none at t = 0); choose the root as ehm_compiled_eval_batch does -- with
 * an adjacency table the visibility walk, started at the previous step's root (q mod n_roots at
 * t = 0), else the first root that contains z, else the last; stop with status 1 unless every
 * barycentric weight of z in THAT ROOT is >= -tol_exit (a NaN state stops); walk the planes and
 * apply the leaf's affine map -- (leaf, u) are ehm_compiled_eval_batch's for z, bit for bit;
 * then the step of ehm_explicit_rollout for the plant kind, bit for bit.  leaf_traj records the
 * source node id of the leaf. */
int ehm_compiled_set_plant(ehm_compiled* law, int32_t n_modes, const double* A, const double* B,
                           const double* w, int32_t n_d, const double* E,
                           const int32_t* region_rows, const double* H, const double* h,
                           int32_t n_g, const double* Gx, const double* gx,
                           const int32_t* leaf_mode, int32_t cost_kind, const double* Q,
                           const double* R);
int ehm_compiled_set_plant_guarded(ehm_compiled* law, int32_t n_modes, const double* A,
                                   const double* B, const double* w, int32_t substeps,
                                   int32_t n_guards, const int32_t* guard_mode,
                                   const int32_t* guard_row0, const double* ga, const double* gb,
                                   const double* gc, const double* gt, const int32_t* strict,
                                   int32_t default_mode, int32_t n_g, const double* Gx,
                                   const double* gx, const int32_t* leaf_mode, int32_t cost_kind,
                                   const double* Q, const double* R);
int ehm_compiled_set_noise(ehm_compiled* law, int32_t n_terms, const int32_t* desc,
                           const double* data, int32_t n_data, int32_t n_d);
int ehm_compiled_rollout(ehm_compiled* law, int64_t n, int32_t T, const double* x0,
                         const double* d, const double* v, double tol_exit, double* x_traj,
                         double* u_traj, int32_t* leaf_traj, double* x_final, int32_t* steps,
                         int32_t* status, double* cost, double* u_norm_sum,
                         double* max_violation, double* kernel_seconds);
int ehm_compiled_rollout_noisy(ehm_compiled* law, int64_t n, int32_t T, const double* x0,
                               uint64_t seed, uint64_t traj0, double tol_exit, double* x_traj,
                               double* u_traj, int32_t* leaf_traj, double* v_traj,
                               double* e_traj, double* w_traj, double* x_final, int32_t* steps,
                               int32_t* status, double* cost, double* u_norm_sum,
                               double* max_violation, double* kernel_seconds);

/* ---- the closed loop around the IMPLICIT law on the device (csrc/ehm_implicit.hip) ------------
 *
 * simulate.rollout_implicit without its host loop: per step one mixed-integer P_theta for every
 * running trajectory (phase one for the n * n_delta (trajectory, commutation) pairs, the point
 * solve for the feasible ones, the minimum with the tie rule of ehm_solve_pt_batch), the plant step
 * and the noise draws, all on the stream of the solver handle with no copy and no synchronisation
 * between steps.  The handle borrows `prob` (generation-2 solver, p <= 8, n_u <= 4): destroy it
 * before the problem, and do not use the problem from another thread while a rollout runs.  Errors:
 * ehm_implicit_last_error. */
typedef struct ehm_implicit ehm_implicit;
int ehm_implicit_create(ehm_problem* prob, ehm_implicit** out);
int ehm_implicit_destroy(ehm_implicit* im);
const char* ehm_implicit_last_error(void);
/* The plant, as ehm_explicit_set_plant / ehm_explicit_set_plant_guarded take it (the same flat
 * arrays), with mode_of [n_delta] = the step-0 mode of every commutation of the problem in place of
 * node_mode (each in [0, n_modes); a guarded plant only records it). */
int ehm_implicit_set_plant(ehm_implicit* im, int32_t n_modes, const double* A, const double* B,
                           const double* w, int32_t n_d, const double* E,
                           const int32_t* region_rows, const double* H, const double* h,
                           int32_t n_g, const double* Gx, const double* gx,
                           const int32_t* mode_of, int32_t cost_kind, const double* Q,
                           const double* R);
int ehm_implicit_set_plant_guarded(ehm_implicit* im, int32_t n_modes, const double* A,
                                   const double* B, const double* w, int32_t substeps,
                                   int32_t n_guards, const int32_t* guard_mode,
                                   const int32_t* guard_row0, const double* ga, const double* gb,
                                   const double* gc, const double* gt, const int32_t* strict,
                                   int32_t default_mode, int32_t n_g, const double* Gx,
                                   const double* gx, const int32_t* mode_of, int32_t cost_kind,
                                   const double* Q, const double* R);
/* The uncertainty model, as ehm_explicit_set_noise takes it (NoiseModel.pack). */
int ehm_implicit_set_noise(ehm_implicit* im, int32_t n_terms, const int32_t* desc,
                           const double* data, int32_t n_data, int32_t n_d);
/* n trajectories of T steps from x0 [n][p].  noisy = 0: the caller's d [T][n][n_d] and v [T][n][p]
 * (each may be NULL; v applies from t = 1); noisy = 1: d and v NULL, v, e and d drawn with the
 * counters of ehm_explicit_rollout_noisy (key (seed, 0), trajectory q has id traj0 + q; not with a
 * guarded plant).  Step t: z = x + v; P_theta at z; no feasible commutation, or none whose point
 * solve converged: status 3; the region of the commutation's step-0 mode does not hold the TRUE
 * state (within tol_exit): status 2; else stage cost and ||u||_2 of the commanded u, the plant step
 * with u + e (a guarded plant: its substeps with u held, no status 2), the worst Gx x+ - gx.
 * Arithmetic of the step: sums in a fixed order from 0.0, no FMA -- x+ = ((A x) + (B u)) + w, then
 * + (E d), each product summed over its columns; a guarded plant steps as in
 * ehm_explicit_set_plant_guarded.  Outputs and time-major records (may be NULL) as
 * ehm_explicit_rollout_noisy, with commutation_traj [T][n] (index of the commutation, -1 after a
 * stop) in place of leaf_traj, and mode_traj [T][n] (its step-0 mode).
 * Stalled solves (the host path repeats them on the generation-1 kernels, this loop cannot): a
 * phase-one solve that ends with a non-zero status keeps the tau it reached, so its verdict may
 * differ from the host's; a feasible pair whose point solve ends with one is left out of the
 * minimum.  Both are counted, and stalled [n] flags the trajectories this happened to -- they may
 * differ from simulate.rollout_implicit's.
 * counts [5]: stalled pairs (both solves), phase-one LPs, point LPs, launches of the fixed
 * sequence (1 + 7 T), stalled pairs of phase one alone.  device_seconds (may be
 * NULL): device time from the first to the last launch. */
int ehm_implicit_rollout(ehm_implicit* im, int64_t n, int32_t T, const double* x0,
                         const double* d, const double* v, int32_t noisy, uint64_t seed,
                         uint64_t traj0, double tol_exit, double* x_traj, double* u_traj,
                         int32_t* commutation_traj, int32_t* mode_traj, double* v_traj,
                         double* e_traj, double* w_traj, double* x_final, int32_t* steps,
                         int32_t* status, double* cost, double* u_norm_sum,
                         double* max_violation, int32_t* stalled, int64_t* counts,
                         double* device_seconds);

/* Cumulative counters of a problem handle (SURVEY.md section 5 "tracing"). */
typedef struct ehm_counters {
    int64_t lp_solves;
    int64_t ipm_iters;
    int64_t kernel_launches;
    int64_t stalled;
    int64_t fallbacks;      /* batch LPs the generation-2 kernels handed to generation 1 */
    int64_t slivers;        /* (simplex, commutation) pairs of the mixed-integer oracles whose
                               phase-one optimum is within 1e-7 of zero AND whose slack problem
                               found no interior: treated as infeasible on that simplex */
    /* batched oracles on the shared-block / wide kernels: device seconds of their kernels (HIP
     * events on the handle's stream around each launch) and launches; [0] problems at a point
     * (ehm_solve_ptd_batch, ehm_point_idx_batch, ...), [1] problems over a simplex */
    double  batch_seconds[2];
    int64_t batch_launches[2];
} ehm_counters;
int ehm_stats(ehm_problem* prob, ehm_counters* out);

/* sizeof of the public structs, in this order: ehm_problem_desc, ehm_run_opts, ehm_node_init,
 * ehm_progress, ehm_tree_info, ehm_counters.  A binding that mirrors the structs (the ctypes
 * classes of explicit_hybrid_mpc_amd/_capi.py) checks itself against the library it loaded: a
 * mirror that is too small would be overrun by the library's writes.  Returns the number of
 * sizes it knows; writes at most n of them.  Needs no device. */
int ehm_abi_sizes(int64_t* sizes, int32_t n);

/* Diagnostics of the shared-block solver (csrc/ehm_ipm2.h): shader-clock cycles spent in each
 * phase of the interior-point iteration, lane 0 of every wavefront, summed over all solves since
 * the handle was created; out[23] = the number of solves.  All zero unless the library was built
 * with -DEHM2_PROF=1 (an experimental build, tools/solver_phases.py).  No reference counterpart:
 * the reference times whole oracle calls (lib/worker.py:60-116). */
int ehm_solver_phase_ticks(ehm_problem* prob, int64_t out[24]);

/* What the shared-block solver eliminates from the Newton systems of this handle (csrc/ehm_ipm2.h,
 * DESIGN.md section 3.2b): out = { nd0, nE, LE, lda } -- the z-columns [nd0, nd0 + nE) are the
 * trailing range of which every MPC row holds at most one entry (the epigraph variables of the
 * infinity-norm cost, lib/mpc_library.py:530-560), LE = rows per such column (padded), lda = column
 * stride of the LDS image.  nE = 0: nothing is eliminated (no such range, a quadratic cost, or
 * EHM_SPARSE=0 in the environment when the handle was created).  Reporting only (bench.py prices
 * the executed flops with it); no reference counterpart. */
int ehm_problem_layout(ehm_problem* prob, int32_t out[4]);

/* The persistent frontier kernel the last persistent launch of this tree ran: out = { family,
 * decide width, expand width, row slots } (widths in factorised columns; the single-width
 * families report theirs twice).  family: EHM_PERSIST_NONE (the run only swept), _K2 (the
 * single-width kernel of ehm_k2.hip), _KP / _KPM (the two-width pair, suboptimality test or
 * midpoint solve first), _K4 (the LDS-resident wide family, ehm_k4.hip: single-rank runs to
 * completion only -- dealt, budgeted and witness-checking launches take the single-width kernel
 * of the same size instead).  Reporting only; no reference counterpart. */
#define EHM_PERSIST_NONE 0
#define EHM_PERSIST_K2   1
#define EHM_PERSIST_KP   2
#define EHM_PERSIST_KPM  3
#define EHM_PERSIST_K4   4
int ehm_tree_persist_kernel(const ehm_tree* tree, int32_t out[4]);

/* The kernel instance a batched solve of LP kind `kind` would run on this handle now: 0 = point,
 * 1 = point feasibility, 2 = minimum over a simplex, 3 = slack (suboptimality test), 4 = simplex
 * feasibility.  out = { family, column capacity (factorised columns), row slots of 64 rows,
 * threads per LP }.  family: EHM_BATCH_K1 (the generation-1 kernels, ehm_problem_set_solver; sized
 * at run time, they report their column limit and the LP's own slots), _K2 (shared-block
 * instances of ehm_k2.hip, one wavefront per LP), _K3 (streaming wide kernels, ehm_k3.hip: 8 or
 * 16 slots), _K4 (LDS-resident wide family, ehm_k4.hip).  The sweeps of a partition (decide,
 * expand, vertex solves) take the instance of the same kinds.  Follows the handle's solver
 * generation, its eliminated columns and the EHM_K4* environment exactly as the launches do.
 * Reporting only; no reference counterpart. */
#define EHM_BATCH_K1 1
#define EHM_BATCH_K2 2
#define EHM_BATCH_K3 3
#define EHM_BATCH_K4 4
int ehm_problem_batch_kernel(ehm_problem* prob, int32_t kind, int32_t out[4]);

/* Device self test of the wave-level primitives (DPP reductions, reciprocal) of every
 * compiled kernel instance: out[5*k .. 5*k+4] for instance k, expected
 * {1072, 99, 25, 1/3, -1}.  Test hook, not part of the reference's surface. */
int ehm_selftest(int device, double* out, int32_t max_instances, int32_t* n_instances);

const char* ehm_last_error(void);
const char* ehm_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* EHMPC_H */
