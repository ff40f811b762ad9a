// The invariant core of a compiled law: the may-reach relation between the
// leaves and the greatest set of one-step invariant leaves that is closed under it.  On a leaf L in
// mode m the successor map (x, d) -> A_m x + B_m u(x) + w_m + E d is affine, so the image of L under
// every disturbance of the box is I(L) = hull{y_i} + E [d_lo, d_hi] with y_i the p + 1 vertex
// successors before the disturbance, and an affine f = g . x + h has over I(L) the extrema
// max_i f(y_i) + sum_k max(gE_k d_lo_k, gE_k d_hi_k) (min likewise), gE_k = g . E[:, k]: no corner of
// the box is enumerated.  A second set of k_reach instances (PER_MODE) reads the generator block of
// the leaf's mode, the blocks p n_g doubles apart: the robust step's G_m = [E | -A_m | B_m | I]
// (ehm_compiled_robust_core), whose box is [d; v; e; v]; the instances of this
// section's entry point read the shared E and compile to the code they had before there was a
// second set.  A third set (k_reach_leaf, ehm_compiled_robust_core_leaf) reads a box
// per leaf: k_leaf_radii (ehm_radii_dev.h) makes the boxes of all leaves, leaf-fastest, and every lane
// copies its leaf's into a slice of LDS of its own, so the traversal reads it through the same
// pointers and the other two sets keep their code.
//
//   k_root_boxes   one thread per root: the bounding box of its vertices
//   k_reach        one thread per leaf, templated on the law's scalar and on P, run twice (count, then
//                  fill): the cell (leaf_cell), the inputs (leaf_map_at) and the y_i in the order of
//                  k_successors (a copy of its step: DESIGN.md 3.8i, Kernels, says why), kept where
//                  the cell was; the image's box; the roots scanned serially
//                  in ascending order, a root a candidate iff its box meets the image's and none of
//                  its p + 1 weights has its maximum over I(L) below -tol_side; below a candidate a
//                  stackless depth-first traversal, left where the plane's maximum allows the walk to
//                  go left, right where its minimum allows it to go right, up through the parent
//                  table, the decision of a node recomputed on the way back from its left child
//   k_core_seed    level 0 for the leaves that fail the one-step test or have no row they asked for
//   k_core_sweep   one thread per leaf without a level: level s if its row names a level < s
//   k_core_counts  the leaves by outcome, through the LDS counters of ehm_verdict.h
//
// The plant and the box sit in LDS (plant_load).  Every operation a decision depends on runs under
// fp contract(off) in a fixed order (tests/core_cpu.py is the numpy mirror); decisions are
// comparisons, so the relation and the levels are the mirror's bit for bit.  The volumes are summed
// on the host in leaf order; the chunk of the count pass, which sends the cells there, changes no
// result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_radii_dev.h"
#include "ehm_scan_dev.h"
#include "ehm_verdict.h"

#define EHM_CORE_BLOCK 64
#define EHM_CORE_OUTCOMES 7
#define EHM_CORE_MAX_D 64           // columns of E the box may have
#define EHM_CORE_CHUNK 65536        // leaves per count pass (plant->chunk = 0)
#define EHM_CORE_POLL 8             // sweeps between two reads of the change flag
#define EHM_CORE_U32 5.9604644775390625e-08      // 2^-24: the single law's widening is (P + 3) of it
#define EHM_CORE_TINY 1.1754943508222875e-38    // 2^-126: what underflow can add to it

namespace {

enum { CORE_INVARIANT = 0, CORE_NO_MODE = 3, CORE_NO_CELL = 4, CORE_UNRESOLVED = 5 };

struct ReachArgs {
    long long n, first;             // leaves first .. first + n - 1
    long long budget;               // node visits one root's traversal may take (3 n_int + 3)
    const void* node;               // of the law's scalar, as leaf_rec
    const void* leaf_rec;
    const int32_t* root_entry;
    const double* root_rec;         // [n_roots][side_stride]
    const double* root_vertices;    // [n_roots][P+1][P]
    const double* root_box;         // [n_roots][2][P]: lo, hi
    ehm_cert::Parents par;
    const int32_t* leaf_mode;       // [n_leaf]
    const int32_t* status;          // [n_leaf] the one-step status
    int n_u, leaf_stride, side_stride, n_roots;
    int n_d, o_lo, o_hi;
    int rows_all, max_fan;
    double tol_side;
    double* vertices;               // [n][P+1][P] or nullptr
    int32_t* count;                 // [n_leaf]: written by the count pass, read by the fill pass
    int32_t* over;                  // [n_leaf]: 1 where the row was cut off
    const int32_t* indptr;          // [n_leaf + 1], nullptr in the count pass
    int32_t* indices;
    unsigned long long* total;      // the count pass: the sum of the counts
};

// The per-leaf boxes of DESIGN.md 3.8k, for the PER_LEAF instances alone: their own kernel argument,
// so that the other instances keep theirs.  Every lane copies its leaf's box, read leaf-fastest from
// `box`, into a slice of LDS of its own, 2 n_d + 1 doubles apart (an odd stride), at o_box.
struct LeafBoxes {
    const double* box;              // [2][n_d][box_n] (k_leaf_radii)
    long long box_n;
    int o_box;
};

// row i of Y [(P+1) P] into v [P] by selects, so Y stays in registers
template <int P>
__device__ __forceinline__ void pick_row(const double (&Y)[(P + 1) * P], int i, double* v) {
#pragma unroll
    for (int c = 0; c < P; ++c) {
        double t = 0.0;
#pragma unroll
        for (int ii = 0; ii <= P; ++ii) t = ii == i ? Y[ii * P + c] : t;
        v[c] = t;
    }
}

// what the box adds to the maximum and to the minimum of g . x over the image
template <int P>
__device__ __forceinline__ void box_range(const double* g, const double* sE, int n_d,
                                          const double* lo_d, const double* hi_d, double& dmax,
                                          double& dmin) {
#pragma clang fp contract(off)
    dmax = 0.0;
    dmin = 0.0;
    for (int k = 0; k < n_d; ++k) {
        double ge = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) ge = ge + g[c] * sE[c * n_d + k];
        const double a = ge * lo_d[k], b = ge * hi_d[k];
        dmax = dmax + (a > b ? a : b);
        dmin = dmin + (a < b ? a : b);
    }
}

// The decision of plane node k for the image: may the walk go left, may it go right.
template <class T, int P>
__device__ __forceinline__ void node_decision(const T* __restrict__ node, int k,
                                              const double (&Y)[(P + 1) * P], const double* X,
                                              const double* sE, int n_d, const double* lo_d,
                                              const double* hi_d, double tol_side, bool& go_left,
                                              bool& go_right, int32_t& left, int32_t& right) {
#pragma clang fp contract(off)
    constexpr bool SINGLE = std::is_same<T, float>::value;
    constexpr int NS = SINGLE ? (P <= 5 ? 8 : 16) : (P <= 6 ? 8 : 16);
    const T* rec = node + (size_t)k * NS;
    double a[P + 1];
#pragma unroll
    for (int c = 0; c <= P; ++c) a[c] = (double)rec[c];
    ehm_cert::children_of(rec, P, left, right);
    double smax = 0.0, smin = 0.0;
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) s = s + a[c] * Y[i * P + c];
        s = s + a[P];
        smax = (i == 0 || s > smax) ? s : smax;
        smin = (i == 0 || s < smin) ? s : smin;
    }
    double dmax, dmin;
    box_range<P>(a, sE, n_d, lo_d, hi_d, dmax, dmin);
    smax = smax + dmax;
    smin = smin + dmin;
    double slack = tol_side;
    if (SINGLE) {
        // |s as walk32 sums it - s| over the image's box
        double m = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) m = m + fabs(a[c]) * X[c];
        m = m + fabs(a[P]);
        slack = slack + (((double)(P + 3) * EHM_CORE_U32) * m + EHM_CORE_TINY);
    }
    const double eps = SINGLE ? (double)EHM_C_EPS32 : EHM_C_EPS;
    go_left = smax >= -eps - slack;
    go_right = smin < -eps + slack;
}

// Everything of one leaf in one pass.  PER_MODE: the generator block is G_m of the leaf's mode, the
// blocks P n_d doubles apart; else the shared E, and the code is that of 3.8i.
// PER_LEAF (with PER_MODE): the box is the leaf's own, copied from LB into the lane's slice of LDS
// (3.8k); the traversal reads it through the same pointers.
template <class T, int P, bool PER_MODE, bool PER_LEAF>
__device__ __forceinline__ void leaf_reach(const ReachArgs& A, const DevPlant& PL,
                                           const double* sh, long long q,
                                           const LeafBoxes* LB = nullptr) {
#pragma clang fp contract(off)
    const int32_t l = (int32_t)(A.first + q);
    const bool fill = A.indptr != nullptr;
    const int n_u = A.n_u, n_d = A.n_d;
    if (fill && A.count[l] == 0) return;
    const T* node = static_cast<const T*>(A.node);
    double Y[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, node, A.root_entry, A.root_vertices, l, Y);
    if (A.vertices) {
        double* vout = A.vertices + (size_t)q * (P + 1) * P;
#pragma unroll
        for (int e = 0; e < (P + 1) * P; ++e) vout[e] = ok ? Y[e] : NAN;
    }
    const int m = A.leaf_mode[l];
    const bool wanted = ok && m >= 0 && m < PL.n_modes &&
                        (A.rows_all || A.status[l] == CORE_INVARIANT);
    if (!wanted) {
        if (!fill) {
            A.count[l] = 0;
            A.over[l] = 0;
        }
        return;
    }
    const T* lr = static_cast<const T*>(A.leaf_rec) + (size_t)l * A.leaf_stride;
    const double* sA = sh + PL.oA + m * P * P;
    const double* sB = sh + PL.oB + m * P * n_u;
    const double* sw = sh + PL.ow + m * P;
    const double* sE = sh + PL.oE + (PER_MODE ? m * (P * n_d) : 0);
    const double* lo_d = sh + A.o_lo;
    const double* hi_d = sh + A.o_hi;
    if constexpr (PER_LEAF) {
        double* mine = const_cast<double*>(sh) + LB->o_box + (int)threadIdx.x * (2 * n_d + 1);
        for (int k = 0; k < 2 * n_d; ++k) mine[k] = LB->box[(size_t)k * LB->box_n + l];
        lo_d = mine;
        hi_d = mine + n_d;
    }
    // the vertex successors before the disturbance, in place of the cell
    for (int i = 0; i <= P; ++i) {
        double v[P];
        pick_row<P>(Y, i, v);
        double u[EHM_R_MAX_NU];
#pragma unroll
        for (int c = 0; c < EHM_R_MAX_NU; ++c)
            u[c] = c < n_u ? leaf_map_at<P>(lr, n_u, c, v) : 0.0;
        double y[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s = s + sA[k * P + c] * v[c];
#pragma unroll
            for (int c = 0; c < EHM_R_MAX_NU; ++c)
                if (c < n_u) s = s + sB[k * n_u + c] * u[c];
            y[k] = s + sw[k];
        }
#pragma unroll
        for (int c = 0; c < P; ++c)
#pragma unroll
            for (int ii = 0; ii <= P; ++ii) Y[ii * P + c] = ii == i ? y[c] : Y[ii * P + c];
    }
    // successors that are not finite (a leaf without a law) span no image: the row stays empty
    bool finite = true;
#pragma unroll
    for (int e = 0; e < (P + 1) * P; ++e) finite = finite && fabs(Y[e]) <= 1.7976931348623157e308;
    if (!finite) {
        if (!fill) {
            A.count[l] = 0;
            A.over[l] = 0;
        }
        return;
    }
    // the image's box, and the largest modulus of every coordinate over it
    double ilo[P], ihi[P], X[P];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        double hi = Y[c], lo = Y[c];
#pragma unroll
        for (int i = 1; i <= P; ++i) {
            hi = Y[i * P + c] > hi ? Y[i * P + c] : hi;
            lo = Y[i * P + c] < lo ? Y[i * P + c] : lo;
        }
        double dmax = 0.0, dmin = 0.0;
        for (int k = 0; k < n_d; ++k) {
            const double a = sE[c * n_d + k] * lo_d[k], b = sE[c * n_d + k] * hi_d[k];
            dmax = dmax + (a > b ? a : b);
            dmin = dmin + (a < b ? a : b);
        }
        ihi[c] = hi + dmax;
        ilo[c] = lo + dmin;
        X[c] = fabs(ihi[c]) > fabs(ilo[c]) ? fabs(ihi[c]) : fabs(ilo[c]);
    }
    const double pad = (double)(P + 1) * A.tol_side;
    const int expect = fill ? A.count[l] : 0;
    int32_t* row = fill ? A.indices + A.indptr[l] : nullptr;
    int cnt = 0;
    bool over = false;
    for (int r = 0; r < A.n_roots && !over; ++r) {
        // the boxes: a root whose box, widened by what a weight of -tol_side reaches, misses the
        // image's holds no point of it
        const double* rb = A.root_box + (size_t)r * 2 * P;
        bool apart = false;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double w = pad * (rb[P + c] - rb[c]);
            apart = apart || (rb[c] - w > ihi[c]) || (rb[P + c] + w < ilo[c]);
        }
        if (apart) continue;
        // the weights: the maximum of each over the image
        const double* rec = A.root_rec + (size_t)r * A.side_stride;
        // (the sums of c_weights, one weight at a time so that few of them are live at once)
        bool holds = true;
        double ssum[P + 1];
#pragma unroll
        for (int i = 0; i <= P; ++i) ssum[i] = 0.0;
#pragma unroll 1
        for (int qq = 0; qq < P; ++qq) {
            const double* g = rec + P + qq * P;
            double wmax = 0.0;
#pragma unroll
            for (int i = 0; i <= P; ++i) {
                double al = 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) al = fma(g[c], Y[i * P + c] - rec[c], al);
                ssum[i] += al;
                wmax = (i == 0 || al > wmax) ? al : wmax;
            }
            double dmax, dmin;
            box_range<P>(g, sE, n_d, lo_d, hi_d, dmax, dmin);
            holds = holds && !(wmax + dmax < -A.tol_side);
        }
        {
            double w0max = 0.0;
#pragma unroll
            for (int i = 0; i <= P; ++i) {
                const double a0 = 1.0 - ssum[i];
                w0max = (i == 0 || a0 > w0max) ? a0 : w0max;
            }
            // the weight of v_0 has the gradient -(sum of the rows)
            double d0 = 0.0;
            for (int k = 0; k < n_d; ++k) {
                double sg = 0.0;
#pragma unroll 1
                for (int qq = 0; qq < P; ++qq) {
                    double ge = 0.0;
#pragma unroll
                    for (int c = 0; c < P; ++c) ge = ge + rec[P + qq * P + c] * sE[c * n_d + k];
                    sg = sg + ge;
                }
                const double g0 = 0.0 - sg;
                const double a = g0 * lo_d[k], b = g0 * hi_d[k];
                d0 = d0 + (a > b ? a : b);
            }
            holds = holds && !(w0max + d0 < -A.tol_side);
        }
        if (!holds) continue;
        // below the root: depth first without a stack.  phase 0: the node is entered from above,
        // 1: from its left child, 2: from its right child.
        int32_t cur = A.root_entry[r];
        if (cur < 0) {
            if (fill && cnt < expect) row[cnt] = ~cur;
            ++cnt;
            over = cnt > A.max_fan;
            continue;
        }
        int phase = 0;
        long long budget = A.budget;
        while (!over) {
            if (--budget < 0) {
                over = true;
                break;
            }
            bool go_left = false, go_right = false;
            int32_t left = 0, right = 0;
            if (phase < 2)
                node_decision<T, P>(node, cur, Y, X, sE, n_d, lo_d, hi_d, A.tol_side, go_left,
                                    go_right, left, right);
            int32_t child;
            int side;
            if (phase == 0 && go_left) {
                child = left;
                side = 0;
            } else if (phase < 2 && go_right) {
                child = right;
                side = 1;
            } else {
                const int32_t up = A.par.node[cur];
                if (up < 0) break;
                phase = A.par.node_side[cur] ? 2 : 1;
                cur = up;
                continue;
            }
            if (child < 0) {
                if (fill && cnt < expect) row[cnt] = ~child;
                ++cnt;
                over = cnt > A.max_fan;
                phase = side ? 2 : 1;
            } else {
                cur = child;
                phase = 0;
            }
        }
    }
    if (!fill) {
        A.count[l] = over ? 0 : cnt;
        A.over[l] = over ? 1 : 0;
    }
}

template <class T, int P, bool PER_MODE>
__global__ __launch_bounds__(EHM_CORE_BLOCK) void k_reach(ReachArgs A, DevPlant PL) {
    // all of the block's LDS is dynamic: the plant and the box (PL.total doubles), the block's edge
    // count after them
    extern __shared__ __attribute__((aligned(16))) double sh[];
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(sh + PL.total);
    const int t = threadIdx.x;
    plant_load(PL, sh);
    if (t == 0) *sum = 0ull;
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + t;
    if (q < A.n) {
        leaf_reach<T, P, PER_MODE, false>(A, PL, sh, q);
        if (!A.indptr) {
            const int c = A.count[A.first + q];
            if (c) atomicAdd(sum, (unsigned long long)c);
        }
    }
    __syncthreads();
    if (t == 0 && !A.indptr && *sum) atomicAdd(A.total, *sum);
}

// k_reach with the leaf's own box: the same block, the lanes' slices after the edge count
template <class T, int P>
__global__ __launch_bounds__(EHM_CORE_BLOCK) void k_reach_leaf(ReachArgs A, DevPlant PL,
                                                               LeafBoxes LB) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(sh + PL.total);
    const int t = threadIdx.x;
    plant_load(PL, sh);
    if (t == 0) *sum = 0ull;
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + t;
    if (q < A.n) {
        leaf_reach<T, P, true, true>(A, PL, sh, q, &LB);
        if (!A.indptr) {
            const int c = A.count[A.first + q];
            if (c) atomicAdd(sum, (unsigned long long)c);
        }
    }
    __syncthreads();
    if (t == 0 && !A.indptr && *sum) atomicAdd(A.total, *sum);
}

__global__ void k_root_boxes(long long n_roots, int p, const double* __restrict__ root_vertices,
                             double* __restrict__ box) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_roots) return;
    const double* v = root_vertices + (size_t)r * (p + 1) * p;
    for (int c = 0; c < p; ++c) {
        double lo = v[c], hi = v[c];
        for (int i = 1; i <= p; ++i) {
            const double x = v[i * p + c];
            lo = x < lo ? x : lo;
            hi = x > hi ? x : hi;
        }
        box[(size_t)r * 2 * p + c] = lo;
        box[(size_t)r * 2 * p + p + c] = hi;
    }
}

// level 0 for the seeds, -1 for the rest; the status with `unresolved` in it
__global__ void k_core_seed(long long n_leaf, const int32_t* __restrict__ status,
                            const int32_t* __restrict__ over, int32_t* __restrict__ level,
                            int32_t* __restrict__ status_out) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_leaf) return;
    const int s = over[l] ? CORE_UNRESOLVED : status[l];
    status_out[l] = s;
    level[l] = s == CORE_INVARIANT ? -1 : 0;
}

// Sweep s >= 1.  What it writes is s, what it reads for is < s: one array is enough.
__global__ void k_core_sweep(long long n_leaf, int s, const int32_t* __restrict__ indptr,
                             const int32_t* __restrict__ indices, int32_t* level,
                             int32_t* __restrict__ changed) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_leaf || level[l] >= 0) return;
    for (int32_t e = indptr[l]; e < indptr[l + 1]; ++e) {
        const int32_t lv = level[indices[e]];
        if (lv >= 0 && lv < s) {
            level[l] = s;
            *changed = 1;
            return;
        }
    }
}

// outcome 0 core, 1 a level above 0, 1 + status for a seed (2 exits .. 6 unresolved)
__global__ __launch_bounds__(256) void k_core_counts(long long n_leaf,
                                                     const int32_t* __restrict__ level,
                                                     const int32_t* __restrict__ status,
                                                     unsigned long long* __restrict__ counters) {
    __shared__ unsigned int cnt[EHM_CORE_OUTCOMES];
    ehm_verdict::counters_zero<256, EHM_CORE_OUTCOMES>(cnt);
    __syncthreads();
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < n_leaf) {
        const int lv = level[l];
        atomicAdd(&cnt[lv < 0 ? 0 : lv > 0 ? 1 : 1 + status[l]], 1u);
    }
    __syncthreads();
    ehm_verdict::counters_flush<256, EHM_CORE_OUTCOMES>(cnt, counters);
}

typedef void (*reach_fn)(ReachArgs, DevPlant);
#define EHM_CORE_ALL(T, M) {&k_reach<T, 1, M>, &k_reach<T, 2, M>, &k_reach<T, 3, M>, \
                            &k_reach<T, 4, M>, &k_reach<T, 5, M>, &k_reach<T, 6, M>, \
                            &k_reach<T, 7, M>, &k_reach<T, 8, M>}
// [0]: the shared E (ehm_compiled_core); [1]: a generator block per mode (ehm_compiled_robust_core)
const reach_fn k_reach64[2][EHM_CP] = {EHM_CORE_ALL(double, false), EHM_CORE_ALL(double, true)};
const reach_fn k_reach32[2][EHM_CP] = {EHM_CORE_ALL(float, false), EHM_CORE_ALL(float, true)};
#undef EHM_CORE_ALL
// the leaf's own box (ehm_compiled_robust_core_leaf)
typedef void (*reach_leaf_fn)(ReachArgs, DevPlant, LeafBoxes);
#define EHM_CORE_ALL(T) {&k_reach_leaf<T, 1>, &k_reach_leaf<T, 2>, &k_reach_leaf<T, 3>, \
                         &k_reach_leaf<T, 4>, &k_reach_leaf<T, 5>, &k_reach_leaf<T, 6>, \
                         &k_reach_leaf<T, 7>, &k_reach_leaf<T, 8>}
const reach_leaf_fn k_reachl64[EHM_CP] = EHM_CORE_ALL(double);
const reach_leaf_fn k_reachl32[EHM_CP] = EHM_CORE_ALL(float);
#undef EHM_CORE_ALL

thread_local ehm_err_channel c_err;

}  // namespace

extern "C" {

const char* ehm_core_last_error(void) { return c_err.c_str(); }

int ehm_core_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_core_opts), (int64_t)sizeof(ehm_core_result),
                           (int64_t)sizeof(ehm_core_leaves)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

}  // extern "C"

namespace {

// Both entry points.  ro: the robust step's boxes (the generator block of a leaf is then G_m of its
// mode), nullptr: the shared E and the box of `o`.
// rr (with ro): the box is the leaf's own, made here from the model for all leaves (3.8k).
int core_run(ehm_compiled* law, const ehm_invariance_opts* o, const ehm_robust_opts* ro,
             const ehm_robust_radii* rr, const ehm_core_opts* co, ehm_core_result* res,
             const ehm_core_leaves* lv) {
    if (!law || !o || !co || !res || !lv) return c_err.fail(EHM_E_INVALID, "core: bad argument");
    if (o->chunk < 0) return c_err.fail(EHM_E_INVALID, "core: chunk < 0");
    if (!o->root_vertices || !o->A || !o->B || !o->w || !o->leaf_mode || !co->status)
        return c_err.fail(EHM_E_INVALID, "core: a required array is NULL");
    if (!lv->level || !lv->status)
        return c_err.fail(EHM_E_INVALID, "core: a required output is NULL");
    if (!(co->tol_side >= 0.0)) return c_err.fail(EHM_E_INVALID, "core: tol_side must be >= 0");
    if (co->rows != EHM_CORE_ROWS_INVARIANT && co->rows != EHM_CORE_ROWS_ALL)
        return c_err.fail(EHM_E_INVALID, "core: rows = %d", (int)co->rows);
    if (co->max_fan < 1 || co->max_edges < 1 || co->max_edges > 0x7fffffffLL)
        return c_err.fail(EHM_E_INVALID, "core: max_fan %d, max_edges %lld (1 .. 2^31 - 1)",
                          (int)co->max_fan, (long long)co->max_edges);
    if (co->want_edges && (!lv->indptr || !lv->indices_out))
        return c_err.fail(EHM_E_INVALID, "core: a required output is NULL");
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    int rc = check_law_shape(c_err, v, "core");
    if (rc) return rc;
    const int p = v.p, n_u = v.n_u;
    RadiiPlan rp;
    if (rr) {
        rc = radii_plan(c_err, o, ro, rr, p, n_u, EHM_CORE_MAX_D, "robust_core_leaf", rp);
        if (rc) return rc;
        o = &rp.og;
        ro = &rp.rg;
    }
    rc = check_step_plant(c_err, o, n_u, EHM_CORE_MAX_D, "core");
    if (rc) return rc;
    RobustGen gen;
    ehm_invariance_opts og = *o;
    if (ro) {
        rc = robust_generators(c_err, o, ro, p, n_u, EHM_CORE_MAX_D, "robust_core", gen);
        if (rc) return rc;
        og.E = gen.G.data();
        og.d_lo = gen.lo.data();
        og.d_hi = gen.hi.data();
        og.n_d = gen.n_g;
        o = &og;
    }
    const long long n_leaf = v.n_leaf;
    if (co->n_status != n_leaf)
        return c_err.fail(EHM_E_INVALID, "core: a status array of %lld for %lld leaves",
                          (long long)co->n_status, n_leaf);
    for (long long l = 0; l < n_leaf; ++l)
        if (co->status[l] < CORE_INVARIANT || co->status[l] > CORE_NO_CELL)
            return c_err.fail(EHM_E_INVALID, "core: status[%lld] = %d (0..4)", l,
                              (int)co->status[l]);
    std::memset(res, 0, sizeof *res);
    if (lv->indices_out) *lv->indices_out = nullptr;
    if (n_leaf == 0) return EHM_OK;
    // the plant's doubles, the box after them
    DevPlant pl{};
    ReachArgs A{};
    Pack pk;
    pack_step_plant(pk, pl, o, p, n_u, A.o_lo, A.o_hi, ro ? o->n_modes : 1);
    const int o_xabs = rr ? pk.put(rr->x_abs, (size_t)p) : 0;
    const int o_uabs = rr ? pk.put(rr->u_abs, (size_t)n_u) : 0;
    pl.total = (int)pk.buf.size();
    const size_t plant_bytes = (size_t)pl.total * sizeof(double);
    // the per-leaf instances: a slice of 2 n_g + 1 doubles per lane after the plant and the count
    const int n_g = o->n_d;
    const size_t slices = rr ? (size_t)EHM_CORE_BLOCK * (2 * n_g + 1) : 0;
    const size_t lds = plant_bytes + slices * sizeof(double) + sizeof(unsigned long long);
    if (rr && pl.total + rr->n_data > EHM_N_MAX_LDS)
        return c_err.fail(EHM_E_INVALID,
                          "robust_core_leaf: plant and model need %d doubles of LDS (%d)",
                          pl.total + (int)rr->n_data, EHM_N_MAX_LDS);
    if (rr && lds > (size_t)EHM_N_MAX_LDS * sizeof(double))
        return c_err.fail(EHM_E_INVALID,
                          "robust_core_leaf: plant and the lanes' boxes need %zu bytes of LDS (%zu)",
                          lds, (size_t)EHM_N_MAX_LDS * sizeof(double));
    EHM_HIP_TRY(c_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(c_err, stream.create());
    const size_t cell = (size_t)(p + 1) * p;
    ParentTable T;
    EHM_HIP_TRY(c_err, make_parents(v, stream, T));
    DevBuf d_plant, d_mode, d_roots, d_box, d_status, d_vert, d_count, d_over, d_ptr, d_idx, d_total,
        d_level, d_status_out, d_flag, d_cnt;
    EHM_HIP_TRY(c_err, d_plant.upload(pk.buf.data(), plant_bytes));
    pl.data = d_plant.as<const double>();
    EHM_HIP_TRY(c_err, d_mode.upload(o->leaf_mode, (size_t)n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_status.upload(co->status, (size_t)n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_roots.upload(o->root_vertices, (size_t)v.n_roots * cell * sizeof(double)));
    EHM_HIP_TRY(c_err, d_box.alloc((size_t)v.n_roots * 2 * p * sizeof(double)));
    const long long chunk = o->chunk > 0 ? o->chunk : EHM_CORE_CHUNK;
    const size_t cap = (size_t)std::min<long long>(chunk, n_leaf);
    EHM_HIP_TRY(c_err, d_vert.alloc(cap * cell * sizeof(double)));
    EHM_HIP_TRY(c_err, d_count.alloc((size_t)(n_leaf + 1) * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_over.alloc((size_t)n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_ptr.alloc((size_t)(n_leaf + 1) * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_total.alloc(sizeof(unsigned long long)));
    EHM_HIP_TRY(c_err, hipMemsetAsync(d_total.ptr, 0, sizeof(unsigned long long), stream));
    EHM_HIP_TRY(c_err, hipMemsetAsync(d_count.ptr, 0, (size_t)(n_leaf + 1) * sizeof(int32_t),
                                      stream));
    hipLaunchKernelGGL(k_root_boxes, dim3(blocks_of(v.n_roots, 256)), dim3(256), 0, stream,
                       v.n_roots, p, d_roots.as<const double>(), d_box.as<double>());
    EHM_HIP_TRY(c_err, hipGetLastError());
    // the boxes of all leaves, leaf-fastest, by the kernel of the one-step test
    DevBuf d_model, d_lbox, d_xl, d_xn, d_ul;
    LeafBoxes LB{};
    double seconds_radii = 0.0;
    if (rr) {
        EHM_HIP_TRY(c_err, d_model.upload(rr->data, (size_t)rr->n_data * sizeof(double)));
        EHM_HIP_TRY(c_err, d_lbox.alloc(2 * (size_t)n_g * n_leaf * sizeof(double)));
        EHM_HIP_TRY(c_err, d_xl.alloc((size_t)n_leaf * p * sizeof(double)));
        EHM_HIP_TRY(c_err, d_xn.alloc((size_t)n_leaf * p * sizeof(double)));
        EHM_HIP_TRY(c_err, d_ul.alloc((size_t)n_leaf * n_u * sizeof(double)));
        rp.nz.data = d_model.as<const double>();
        RadiiArgs RA{};
        RA.n = n_leaf;
        RA.node = v.node;
        RA.leaf_rec = v.leaf_rec;
        RA.root_entry = v.root_entry;
        RA.root_vertices = d_roots.as<const double>();
        RA.par = T.view();
        RA.leaf_mode = d_mode.as<const int32_t>();
        RA.n_u = n_u;
        RA.leaf_stride = v.leaf_stride;
        RA.n_dd = rp.n_dd;
        RA.n_v = rp.n_v;
        RA.n_e = rp.n_e;
        RA.n_g = n_g;
        RA.iters = rr->radius_iters;
        RA.o_xabs = o_xabs;
        RA.o_uabs = o_uabs;
        RA.box_n = n_leaf;
        RA.box = d_lbox.as<double>();
        RA.x_abs_leaf = d_xl.as<double>();
        RA.x_next_abs = d_xn.as<double>();
        RA.u_abs_leaf = d_ul.as<double>();
        EventPair evr;
        (void)hipEventRecord(evr.e0, stream);
        hipLaunchKernelGGL((v.single ? k_rad32 : k_rad64)[p - 1],
                           dim3(blocks_of(n_leaf, EHM_RAD_BLOCK)), dim3(EHM_RAD_BLOCK),
                           plant_bytes + (size_t)rr->n_data * sizeof(double), stream, RA, pl,
                           rp.nz);
        (void)hipEventRecord(evr.e1, stream);
        EHM_HIP_TRY(c_err, hipGetLastError());
        EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
        evr.seconds(&seconds_radii);
        LB.box = d_lbox.as<const double>();
        LB.box_n = n_leaf;
        LB.o_box = pl.total + 1;         // after the block's edge count
    }
    A.budget = 3 * v.n_int + 3;
    A.node = v.node;
    A.leaf_rec = v.leaf_rec;
    A.root_entry = v.root_entry;
    A.root_rec = v.root_rec;
    A.root_vertices = d_roots.as<const double>();
    A.root_box = d_box.as<const double>();
    A.par = T.view();
    A.leaf_mode = d_mode.as<const int32_t>();
    A.status = d_status.as<const int32_t>();
    A.n_u = n_u;
    A.leaf_stride = v.leaf_stride;
    A.side_stride = v.side_stride;
    A.n_roots = (int)v.n_roots;
    A.n_d = o->n_d;
    A.rows_all = co->rows == EHM_CORE_ROWS_ALL;
    A.max_fan = co->max_fan;
    A.tol_side = co->tol_side;
    A.count = d_count.as<int32_t>();
    A.over = d_over.as<int32_t>();
    A.total = d_total.as<unsigned long long>();
    auto launch = [&](long long first, long long n) {
        A.first = first;
        A.n = n;
        const dim3 grid(blocks_of(n, EHM_CORE_BLOCK)), block(EHM_CORE_BLOCK);
        if (rr)
            hipLaunchKernelGGL((v.single ? k_reachl32 : k_reachl64)[p - 1], grid, block, lds, stream,
                               A, pl, LB);
        else
            hipLaunchKernelGGL((v.single ? k_reach32 : k_reach64)[ro ? 1 : 0][p - 1], grid, block,
                               lds, stream, A, pl);
    };
    // the count pass, chunk by chunk: the cells go to the host for their volumes
    std::vector<double> hvert(cap * cell), vsub, volume((size_t)n_leaf, 0.0);
    std::vector<long long> has;
    EventPair ev;
    for (long long off = 0; off < n_leaf; off += chunk) {
        const long long nc = std::min<long long>(chunk, n_leaf - off);
        A.vertices = d_vert.as<double>();
        (void)hipEventRecord(ev.e0, stream);
        launch(off, nc);
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(c_err, hipGetLastError());
        EHM_HIP_TRY(c_err, hipMemcpyAsync(hvert.data(), d_vert.ptr,
                                          (size_t)nc * cell * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
        double s = 0.0;
        ev.seconds(&s);
        res->seconds_reach += s;
        has.clear();
        for (long long q = 0; q < nc; ++q)
            if (hvert[(size_t)q * cell] == hvert[(size_t)q * cell]) has.push_back(q);
        rc = cell_volumes(c_err, "core", v.device, p, hvert.data(), has, vsub);
        if (rc) return rc;
        for (size_t a = 0; a < has.size(); ++a) volume[(size_t)(off + has[a])] = vsub[a];
    }
    res->seconds_reach += seconds_radii;
    unsigned long long total = 0;
    EHM_HIP_TRY(c_err, hipMemcpy(&total, d_total.ptr, sizeof total, hipMemcpyDeviceToHost));
    if (total > (unsigned long long)co->max_edges)
        return c_err.fail(EHM_E_CAPACITY, "core: the relation has %llu edges, max_edges is %lld",
                          total, (long long)co->max_edges);
    res->n_edges = (int64_t)total;
    rc = exclusive_scan(c_err, stream, d_count.as<const int32_t>(), d_ptr.as<int32_t>(),
                        n_leaf + 1);
    if (rc) return rc;
    EHM_HIP_TRY(c_err, d_idx.alloc((size_t)total * sizeof(int32_t)));
    // the fill pass
    A.vertices = nullptr;
    A.indptr = d_ptr.as<const int32_t>();
    A.indices = d_idx.as<int32_t>();
    (void)hipEventRecord(ev.e0, stream);
    launch(0, n_leaf);
    (void)hipEventRecord(ev.e1, stream);
    EHM_HIP_TRY(c_err, hipGetLastError());
    EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
    {
        double s = 0.0;
        ev.seconds(&s);
        res->seconds_reach += s;
    }
    // the fixed point
    EHM_HIP_TRY(c_err, d_level.alloc((size_t)n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_status_out.alloc((size_t)n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_flag.alloc(sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_cnt.alloc(EHM_CORE_OUTCOMES * sizeof(unsigned long long)));
    const dim3 lgrid(blocks_of(n_leaf, 256)), lblock(256);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_core_seed, lgrid, lblock, 0, stream, n_leaf, d_status.as<const int32_t>(),
                       d_over.as<const int32_t>(), d_level.as<int32_t>(),
                       d_status_out.as<int32_t>());
    EHM_HIP_TRY(c_err, hipGetLastError());
    for (long long s = 1; s <= n_leaf;) {
        EHM_HIP_TRY(c_err, hipMemsetAsync(d_flag.ptr, 0, sizeof(int32_t), stream));
        for (int j = 0; j < EHM_CORE_POLL && s <= n_leaf; ++j, ++s)
            hipLaunchKernelGGL(k_core_sweep, lgrid, lblock, 0, stream, n_leaf, (int)s,
                               d_ptr.as<const int32_t>(), d_idx.as<const int32_t>(),
                               d_level.as<int32_t>(), d_flag.as<int32_t>());
        EHM_HIP_TRY(c_err, hipGetLastError());
        int32_t changed = 0;
        EHM_HIP_TRY(c_err, hipMemcpyAsync(&changed, d_flag.ptr, sizeof changed,
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
        if (!changed) break;
    }
    res->seconds_sweeps = wall_since(t0);
    EHM_HIP_TRY(c_err, hipMemsetAsync(d_cnt.ptr, 0, EHM_CORE_OUTCOMES * sizeof(unsigned long long),
                                      stream));
    hipLaunchKernelGGL(k_core_counts, lgrid, lblock, 0, stream, n_leaf,
                       d_level.as<const int32_t>(), d_status_out.as<const int32_t>(),
                       d_cnt.as<unsigned long long>());
    EHM_HIP_TRY(c_err, hipGetLastError());
    unsigned long long cnt[EHM_CORE_OUTCOMES];
    EHM_HIP_TRY(c_err, hipMemcpyAsync(cnt, d_cnt.ptr, sizeof cnt, hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->level, d_level.ptr, (size_t)n_leaf * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->status, d_status_out.ptr,
                                      (size_t)n_leaf * sizeof(int32_t), hipMemcpyDeviceToHost,
                                      stream));
    EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
    for (int i = 0; i < EHM_CORE_OUTCOMES; ++i) res->counts[i] = (int64_t)cnt[i];
    int32_t top = -1;
    for (long long l = 0; l < n_leaf; ++l) {
        top = std::max(top, lv->level[l]);
        res->cell_volume += volume[(size_t)l];
        if (lv->level[l] < 0) res->core_volume += volume[(size_t)l];
    }
    res->n_sweeps = (int64_t)top + 1;
    if (co->want_edges) {
        std::vector<int32_t> hptr((size_t)n_leaf + 1);
        EHM_HIP_TRY(c_err, hipMemcpy(hptr.data(), d_ptr.ptr, hptr.size() * sizeof(int32_t),
                                     hipMemcpyDeviceToHost));
        for (long long l = 0; l <= n_leaf; ++l) lv->indptr[l] = hptr[(size_t)l];
        {
            void* host = nullptr;
            rc = ehm_host_alloc((size_t)std::max<unsigned long long>(total, 1) * sizeof(int32_t),
                                &host);
            if (rc) return c_err.fail(rc, "core: ehm_host_alloc: %s", ehm_last_error());
            const hipError_t e = hipMemcpy(host, d_idx.ptr, (size_t)total * sizeof(int32_t),
                                           hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                (void)ehm_host_free(host);
                return c_err.fail(EHM_E_HIP, "core: copying the edges: %s", hipGetErrorString(e));
            }
            *lv->indices_out = static_cast<int32_t*>(host);
        }
    }
    return EHM_OK;
}

}  // namespace

extern "C" {

int ehm_compiled_core(ehm_compiled* law, const ehm_invariance_opts* o, const ehm_core_opts* co,
                      ehm_core_result* res, const ehm_core_leaves* lv) {
    return core_run(law, o, nullptr, nullptr, co, res, lv);
}

int ehm_compiled_robust_core(ehm_compiled* law, const ehm_invariance_opts* o,
                             const ehm_robust_opts* ro, const ehm_core_opts* co,
                             ehm_core_result* res, const ehm_core_leaves* lv) {
    if (!ro) return c_err.fail(EHM_E_INVALID, "robust_core: bad argument");
    return core_run(law, o, ro, nullptr, co, res, lv);
}

int ehm_compiled_robust_core_leaf(ehm_compiled* law, const ehm_invariance_opts* o,
                                  const ehm_robust_opts* ro, const ehm_robust_radii* rr,
                                  const ehm_core_opts* co, ehm_core_result* res,
                                  const ehm_core_leaves* lv) {
    if (!ro || !rr || !o) return c_err.fail(EHM_E_INVALID, "robust_core_leaf: bad argument");
    return core_run(law, o, ro, rr, co, res, lv);
}

}  // extern "C"
