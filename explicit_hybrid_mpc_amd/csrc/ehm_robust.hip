// One-step invariance of a compiled law under process, measurement and input error (DESIGN.md
// section 3.8j).  The closed loop of the noisy rollout evaluates the law at the measured state
// z = x + v, tests the mode's region on the true state x = z - v and steps the plant with u + e, so on
// a leaf L of mode m the measured state's successor is
//     z+ = [A_m z + B_m u(z) + w_m] + E d - A_m v + B_m e + v',
// affine in (z, d, v, e, v'): its image is I(L) = hull{y_i} + G_m [g_lo, g_hi],
// G_m = [E | -A_m | B_m | I].
// Where the roots' union is convex it is the intersection of the half-spaces n_f . x >= c_f of its
// boundary facets, and the minimum of n_f . y - c_f over I(L) is
// min_i n_f . y_i - c_f + sum_k min(nG_k g_lo_k, nG_k g_hi_k), nG_k = n_f . G_m[:, k]: no corner of the
// box is enumerated.
//
//   k_robust_slack   one thread per (facet, mode): the sum over the generators, which no leaf changes
//   k_robust_step    one thread per requested leaf, templated on the law's scalar and on P: the cell
//                    and the leaf's map at its vertices (ehm_cells_dev.h), the region rows of the
//                    leaf's mode at the vertices with what the v box adds, the y_i in the order of
//                    k_successors (ehm_invariance.hip), kept where the cell was, then every facet in
//                    order: the row [n_f | c_f] is the same for all lanes (a wave-uniform load), the
//                    slack is read at [f][m]; the counts by the LDS counters of ehm_verdict.h
//
// With per-leaf error boxes (ehm_compiled_robust_successors_leaf) the box differs from
// leaf to leaf, so no table holds the sum over the generators:
//   k_leaf_radii        (ehm_radii_dev.h) one thread per requested leaf: the leaf's box, leaf-fastest
//   k_robust_ng         one thread per (facet, mode): nG[f][m][k] = n_f . G_m[:, k], k_robust_slack's sum
//   k_robust_step_leaf  k_robust_step over the same body (LEAF): the v box of the region rows is the
//                       leaf's, the facet value (mn_f - c_f) + sum_k min(nG_k lo_k(L), nG_k hi_k(L))
//                       from 0 in k order -- with constant boxes k_robust_slack's value bit for bit
// The new arguments travel in a struct of their own (LeafBox), so k_robust_step compiles to the code it
// had.
//
// The plant, G, the boxes and the region rows sit in LDS (plant_load).  Every operation a result
// depends on runs under fp contract(off) in a fixed order (tests/robust_cpu.py is the numpy mirror).
// The worst leaf and the volumes are taken on the host in leaf order, so no result depends on the
// chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_radii_dev.h"
#include "ehm_verdict.h"

#define EHM_ROB_BLOCK 64
#define EHM_ROB_STATUSES 5
#define EHM_ROB_MAX_G 64            // generators: n_d + 2 p + n_u
#define EHM_ROB_CHUNK 65536         // leaves per pass (plant->chunk = 0)

namespace {

enum { ROB_INVARIANT = 0, ROB_EXITS = 1, ROB_MODE_REGION = 2, ROB_NO_MODE = 3, ROB_NO_CELL = 4 };

struct RobustArgs {
    long long n;
    const int32_t* leaf_ids;        // or nullptr: leaves first .. first + n - 1
    long long first;
    const void* node;               // of the law's scalar, as leaf_rec
    const void* leaf_rec;
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    ehm_cert::Parents par;
    const int32_t* leaf_mode;       // [n_leaf]
    const double* facets;           // [n_facets][P+1]: n_f, c_f
    const double* slack;            // [n_facets][n_modes]
    long long n_facets;
    int n_u, leaf_stride;
    int o_vlo, o_vhi;               // the v box at sh + o_vlo, sh + o_vhi (zeros without one)
    double tol_exit, thr;           // a facet holds iff its value is >= -thr
    double* vertices;               // [n][P+1][P]
    int32_t* status;                // [n]
    double* margin;                 // [n]
    int32_t* worst;                 // [n]
    unsigned long long* counters;   // [EHM_ROB_STATUSES]
};

// The per-leaf boxes of DESIGN.md 3.8k, for the LEAF instances alone: their own kernel argument, so
// that the other instances keep theirs.
struct LeafBox {
    const double* box;              // [2][n_g][box_n], leaf-fastest (k_leaf_radii)
    long long box_n;
    const double* nG;               // [n_facets][n_modes][n_g]
    int n_g, n_dd, n_v;
};

// a beats b as the smaller value: the smaller number, a NaN before any number; the earlier stays on
// ties
__device__ __forceinline__ bool value_beats(double a, double b) {
    return a < b || (a != a && b == b);
}

// slack[f][m] = sum_k min(nG_k lo_k, nG_k hi_k); G [n_modes][p][n_g]
__global__ void k_robust_slack(long long n_facets, int n_modes, int p, int n_g,
                               const double* __restrict__ facets, const double* __restrict__ G,
                               const double* __restrict__ lo, const double* __restrict__ hi,
                               double* __restrict__ slack) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_facets * n_modes) return;
    const long long f = t / n_modes;
    const int m = (int)(t - f * n_modes);
    const double* nf = facets + (size_t)f * (p + 1);
    const double* Gm = G + (size_t)m * p * n_g;
    double s = 0.0;
    for (int k = 0; k < n_g; ++k) {
        double ng = 0.0;
        for (int c = 0; c < p; ++c) ng = ng + nf[c] * Gm[c * n_g + k];
        const double a = ng * lo[k], b = ng * hi[k];
        s = s + (a < b ? a : b);
    }
    slack[t] = s;
}

// nG[f][m][k] = ((0 + n_f0 G_m[0][k]) + ..): the sum of k_robust_slack, kept per generator for the
// boxes that differ from leaf to leaf
__global__ void k_robust_ng(long long n_facets, int n_modes, int p, int n_g,
                            const double* __restrict__ facets, const double* __restrict__ G,
                            double* __restrict__ nG) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_facets * n_modes) return;
    const long long f = t / n_modes;
    const int m = (int)(t - f * n_modes);
    const double* nf = facets + (size_t)f * (p + 1);
    const double* Gm = G + (size_t)m * p * n_g;
    for (int k = 0; k < n_g; ++k) {
        double ng = 0.0;
        for (int c = 0; c < p; ++c) ng = ng + nf[c] * Gm[c * n_g + k];
        nG[(size_t)t * n_g + k] = ng;
    }
}

// Everything of one leaf; returns its status.  LEAF: the v box of the region rows and the box of the
// facet sums are the leaf's own (LB); else LB is not read and the code is that of
// 3.8j.
template <class T, int P, bool LEAF>
__device__ __forceinline__ int leaf_robust(const RobustArgs& A, const DevPlant& PL,
                                           const double* sh, long long q, const LeafBox* LB) {
#pragma clang fp contract(off)
    const int32_t l = A.leaf_ids ? A.leaf_ids[q] : (int32_t)(A.first + q);
    const int n_u = A.n_u;
    const T* node = static_cast<const T*>(A.node);
    double Y[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, node, A.root_entry, A.root_vertices, l, Y);
    double* vout = A.vertices + (size_t)q * (P + 1) * P;
#pragma unroll
    for (int e = 0; e < (P + 1) * P; ++e) vout[e] = ok ? Y[e] : NAN;
    const int m = A.leaf_mode[l];
    if (!ok || m < 0 || m >= PL.n_modes) {
        A.margin[q] = NAN;
        A.worst[q] = -1;
        return ok ? ROB_NO_MODE : ROB_NO_CELL;
    }
    // the region rows of the leaf's mode on the true state z - v: the largest row sum over the
    // vertices and what the v box adds to it
    const double* v_lo = sh + A.o_vlo;
    const double* v_hi = sh + A.o_vhi;
    bool in_region = true;
    double vl[P], vh[P];
    if constexpr (LEAF) {
#pragma unroll
        for (int c = 0; c < P; ++c) {
            vl[c] = LB->n_v ? LB->box[(size_t)(LB->n_dd + c) * LB->box_n + q] : 0.0;
            vh[c] = LB->n_v ? LB->box[(size_t)(LB->n_g + LB->n_dd + c) * LB->box_n + q] : 0.0;
        }
    }
    for (int r = PL.row0[m]; r < PL.row0[m + 1]; ++r) {
        double H[P];
#pragma unroll
        for (int c = 0; c < P; ++c) H[c] = sh[PL.oH + r * P + c];
        double smax = 0.0;
#pragma unroll
        for (int i = 0; i <= P; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s = s + H[c] * Y[i * P + c];
            smax = (i == 0 || s > smax) ? s : smax;
        }
        double rs = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double g = 0.0 - H[c];
            double lo_c, hi_c;
            if constexpr (LEAF) {
                lo_c = vl[c];
                hi_c = vh[c];
            } else {
                lo_c = v_lo[c];
                hi_c = v_hi[c];
            }
            const double a = g * lo_c, b = g * hi_c;
            rs = rs + (a > b ? a : b);
        }
        in_region = in_region && (smax + rs <= sh[PL.oh + r] + A.tol_exit);
    }
    // the vertex successors before the errors, in place of the cell: the step of k_successors
    const T* lr = static_cast<const T*>(A.leaf_rec) + (size_t)l * A.leaf_stride;
    const double* sA = sh + PL.oA + m * P * P;
    const double* sB = sh + PL.oB + m * P * n_u;
    const double* sw = sh + PL.ow + m * P;
    for (int i = 0; i <= P; ++i) {
        double v[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double t = 0.0;
#pragma unroll
            for (int ii = 0; ii <= P; ++ii) t = ii == i ? Y[ii * P + c] : t;
            v[c] = t;
        }
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
    // the facets: f is the same for every lane, so the row comes by a wave-uniform load
    const double* __restrict__ slack = A.slack + m;
    bool all_hold = true;
    double best = 0.0;
    int best_at = -1;
    for (long long f = 0; f < A.n_facets; ++f) {
        const double* __restrict__ nf = A.facets + (size_t)f * (P + 1);
        double mn = 0.0;
        int at = 0;
#pragma unroll
        for (int i = 0; i <= P; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s = s + nf[c] * Y[i * P + c];
            const bool b = i == 0 || value_beats(s, mn);
            mn = b ? s : mn;
            at = b ? i : at;
        }
        double sl;
        if constexpr (LEAF) {
            const double* __restrict__ ng = LB->nG + ((size_t)f * PL.n_modes + m) * LB->n_g;
            const double* __restrict__ bl = LB->box + q;
            const double* __restrict__ bh = LB->box + (size_t)LB->n_g * LB->box_n + q;
            sl = 0.0;
            for (int k = 0; k < LB->n_g; ++k) {
                const double a = ng[k] * bl[(size_t)k * LB->box_n];
                const double b = ng[k] * bh[(size_t)k * LB->box_n];
                sl = sl + (a < b ? a : b);
            }
        } else {
            sl = slack[(size_t)f * PL.n_modes];
        }
        const double val = (mn - nf[P]) + sl;
        all_hold = all_hold && (val >= -A.thr);
        if (best_at < 0 || value_beats(val, best)) {
            best = val;
            best_at = (int)f * (P + 1) + at;
        }
    }
    A.margin[q] = best;
    A.worst[q] = best_at;
    return !in_region ? ROB_MODE_REGION : all_hold ? ROB_INVARIANT : ROB_EXITS;
}

template <class T, int P, bool LEAF>
__device__ __forceinline__ void robust_block(const RobustArgs& A, const DevPlant& PL,
                                             const LeafBox* LB) {
    // all of the block's LDS is dynamic: the plant, G, the boxes and the region rows (PL.total
    // doubles), the status counters after them
    extern __shared__ __attribute__((aligned(16))) double sh[];
    unsigned int* cnt = reinterpret_cast<unsigned int*>(sh + PL.total);
    plant_load(PL, sh);
    ehm_verdict::counters_zero<EHM_ROB_BLOCK, EHM_ROB_STATUSES>(cnt);
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < A.n) {
        const int s = leaf_robust<T, P, LEAF>(A, PL, sh, q, LB);
        A.status[q] = s;
        atomicAdd(&cnt[s], 1u);
    }
    __syncthreads();
    ehm_verdict::counters_flush<EHM_ROB_BLOCK, EHM_ROB_STATUSES>(cnt, A.counters);
}

template <class T, int P>
__global__ __launch_bounds__(EHM_ROB_BLOCK) void k_robust_step(RobustArgs A, DevPlant PL) {
    robust_block<T, P, false>(A, PL, nullptr);
}

template <class T, int P>
__global__ __launch_bounds__(EHM_ROB_BLOCK) void k_robust_step_leaf(RobustArgs A, DevPlant PL,
                                                                    LeafBox LB) {
    robust_block<T, P, true>(A, PL, &LB);
}

typedef void (*robust_fn)(RobustArgs, DevPlant);
typedef void (*robust_leaf_fn)(RobustArgs, DevPlant, LeafBox);
#define EHM_ROB_ALL(T) {&k_robust_step<T, 1>, &k_robust_step<T, 2>, &k_robust_step<T, 3>, \
                        &k_robust_step<T, 4>, &k_robust_step<T, 5>, &k_robust_step<T, 6>, \
                        &k_robust_step<T, 7>, &k_robust_step<T, 8>}
const robust_fn k_rob64[EHM_CP] = EHM_ROB_ALL(double);
const robust_fn k_rob32[EHM_CP] = EHM_ROB_ALL(float);
#undef EHM_ROB_ALL
#define EHM_ROB_ALL(T) {&k_robust_step_leaf<T, 1>, &k_robust_step_leaf<T, 2>, \
                        &k_robust_step_leaf<T, 3>, &k_robust_step_leaf<T, 4>, \
                        &k_robust_step_leaf<T, 5>, &k_robust_step_leaf<T, 6>, \
                        &k_robust_step_leaf<T, 7>, &k_robust_step_leaf<T, 8>}
const robust_leaf_fn k_robl64[EHM_CP] = EHM_ROB_ALL(double);
const robust_leaf_fn k_robl32[EHM_CP] = EHM_ROB_ALL(float);
#undef EHM_ROB_ALL

thread_local ehm_err_channel b_err;

}  // namespace

extern "C" {

const char* ehm_robust_last_error(void) { return b_err.c_str(); }

int ehm_robust_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_robust_opts), (int64_t)sizeof(ehm_robust_result),
                           (int64_t)sizeof(ehm_robust_leaves)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_robust_radii_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_robust_radii),
                           (int64_t)sizeof(ehm_robust_leaf_boxes)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

}  // extern "C"

namespace {

// Both entry points.  rr: the boxes are the leaf's own, made from the model (lb takes
// them, or is nullptr); nullptr: the boxes of `o` and `ro` (3.8j).
int robust_run(ehm_compiled* law, const ehm_invariance_opts* o, const ehm_robust_opts* ro,
               const ehm_robust_radii* rr, ehm_robust_result* res, const ehm_robust_leaves* lv,
               ehm_robust_leaf_boxes* lb, const char* who) {
    if (!law || !o || !ro || !res || !lv) return b_err.fail(EHM_E_INVALID, "%s: bad argument", who);
    if (o->n < 0 || o->chunk < 0) return b_err.fail(EHM_E_INVALID, "%s: n or chunk < 0", who);
    if (!o->root_vertices || !o->A || !o->B || !o->w || !o->leaf_mode || !ro->facets)
        return b_err.fail(EHM_E_INVALID, "%s: a required array is NULL", who);
    if (o->n > 0 && (!lv->status || !lv->margin || !lv->worst))
        return b_err.fail(EHM_E_INVALID, "%s: a required output is NULL", who);
    if (!(o->tol_exit >= 0.0) || !(ro->tol_set >= 0.0))
        return b_err.fail(EHM_E_INVALID, "%s: tol_exit and tol_set must be >= 0", who);
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    int rc = check_law_shape(b_err, v, who);
    if (rc) return rc;
    const int p = v.p, n_u = v.n_u;
    if (ro->n_facets < 1 || ro->n_facets * (p + 1) >= 0x7fffffffLL)
        return b_err.fail(EHM_E_INVALID, "%s: %lld facets (1 .. (2^31 - 1) / (p + 1))", who,
                          (long long)ro->n_facets);
    RadiiPlan rp;
    RobustGen gen0;
    if (rr) {
        rc = radii_plan(b_err, o, ro, rr, p, n_u, EHM_ROB_MAX_G, who, rp);
        if (rc) return rc;
        o = &rp.og;
        ro = &rp.rg;
    } else {
        rc = check_step_plant(b_err, o, n_u, EHM_ROB_MAX_G, who);
        if (rc) return rc;
        rc = robust_generators(b_err, o, ro, p, n_u, EHM_ROB_MAX_G, who, gen0);
        if (rc) return rc;
    }
    const RobustGen& gen = rr ? rp.gen : gen0;
    DevPlant pl{};
    int rows = 0;
    for (int m = 0; m < o->n_modes; ++m) {
        const int r = o->region_rows ? o->region_rows[m] : 0;
        if (r < 0) return b_err.fail(EHM_E_INVALID, "%s: mode %d has %d region rows", who, m, r);
        pl.row0[m] = rows;
        rows += r;
    }
    if (rows > EHM_R_MAX_ROWS || (rows > 0 && (!o->H || !o->h)))
        return b_err.fail(EHM_E_INVALID, "%s: %d mode-region rows (0..%d)", who, rows,
                          EHM_R_MAX_ROWS);
    for (int m = o->n_modes; m <= EHM_R_MAX_MODES; ++m) pl.row0[m] = rows;
    rc = check_law_leaves(b_err, v, o->n, o->leaf_ids, who);
    if (rc) return rc;
    std::memset(res, 0, sizeof *res);
    res->worst_leaf = -1;
    res->worst_margin = NAN;
    res->n_generators = gen.n_g;
    if (lb) lb->seconds_radii = 0.0;
    if (o->n == 0) return EHM_OK;
    const size_t cell = (size_t)(p + 1) * p;
    double scale = 0.0;
    for (size_t e = 0; e < (size_t)v.n_roots * cell; ++e)
        scale = std::max(scale, std::fabs(o->root_vertices[e]));
    // the plant's doubles with G_m of every mode and the stacked box, the region rows and the v box
    // after them
    ehm_invariance_opts og = *o;
    og.E = gen.G.data();
    og.d_lo = gen.lo.data();
    og.d_hi = gen.hi.data();
    og.n_d = gen.n_g;
    Pack pk;
    int o_lo, o_hi;
    pack_step_plant(pk, pl, &og, p, n_u, o_lo, o_hi, o->n_modes);
    pl.oH = pk.put(o->H, (size_t)rows * p);
    pl.oh = pk.put(o->h, (size_t)rows);
    const int o_vlo = pk.put(ro->v_lo, (size_t)p), o_vhi = pk.put(ro->v_hi, (size_t)p);
    const int o_xabs = rr ? pk.put(rr->x_abs, (size_t)p) : 0;
    const int o_uabs = rr ? pk.put(rr->u_abs, (size_t)n_u) : 0;
    pl.total = (int)pk.buf.size();
    const size_t plant_bytes = (size_t)pl.total * sizeof(double);
    const size_t lds = plant_bytes + EHM_ROB_STATUSES * sizeof(unsigned int);
    if (rr && pl.total + rr->n_data > EHM_N_MAX_LDS)
        return b_err.fail(EHM_E_INVALID, "%s: plant and model need %d doubles of LDS (%d)", who,
                          pl.total + (int)rr->n_data, EHM_N_MAX_LDS);
    EHM_HIP_TRY(b_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(b_err, stream.create());
    ParentTable T;
    EHM_HIP_TRY(b_err, make_parents(v, stream, T));
    const long long chunk = o->chunk > 0 ? o->chunk : EHM_ROB_CHUNK;
    const size_t cap = (size_t)std::min<long long>(chunk, o->n);
    DevBuf d_plant, d_mode, d_roots, d_ids, d_cnt, d_facets, d_slack;
    EHM_HIP_TRY(b_err, d_plant.upload(pk.buf.data(), plant_bytes));
    pl.data = d_plant.as<const double>();
    EHM_HIP_TRY(b_err, d_mode.upload(o->leaf_mode, (size_t)v.n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(b_err, d_roots.upload(o->root_vertices, (size_t)v.n_roots * cell * sizeof(double)));
    EHM_HIP_TRY(b_err, d_facets.upload(ro->facets,
                                       (size_t)ro->n_facets * (p + 1) * sizeof(double)));
    EHM_HIP_TRY(b_err, d_slack.alloc((size_t)ro->n_facets * o->n_modes * sizeof(double)));
    if (o->leaf_ids) EHM_HIP_TRY(b_err, d_ids.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(b_err, d_cnt.alloc(EHM_ROB_STATUSES * sizeof(unsigned long long)));
    EHM_HIP_TRY(b_err, hipMemsetAsync(d_cnt.ptr, 0, EHM_ROB_STATUSES * sizeof(unsigned long long),
                                      stream));
    // the per-leaf boxes: the model, the box of a chunk, the bounds, the table nG
    const int n_g = gen.n_g;
    DevBuf d_model, d_box, d_xl, d_xn, d_ul, d_ng;
    RadiiArgs RA{};
    LeafBox LB{};
    if (rr) {
        EHM_HIP_TRY(b_err, d_model.upload(rr->data, (size_t)rr->n_data * sizeof(double)));
        EHM_HIP_TRY(b_err, d_box.alloc(2 * (size_t)n_g * cap * sizeof(double)));
        EHM_HIP_TRY(b_err, d_xl.alloc(cap * p * sizeof(double)));
        EHM_HIP_TRY(b_err, d_xn.alloc(cap * p * sizeof(double)));
        EHM_HIP_TRY(b_err, d_ul.alloc(cap * n_u * sizeof(double)));
        EHM_HIP_TRY(b_err, d_ng.alloc((size_t)ro->n_facets * o->n_modes * n_g * sizeof(double)));
        rp.nz.data = d_model.as<const double>();
    }
    EventPair ev, ev_radii;
    (void)hipEventRecord(ev.e0, stream);
    if (rr)
        hipLaunchKernelGGL(k_robust_ng, dim3(blocks_of(ro->n_facets * o->n_modes, 256)), dim3(256),
                           0, stream, (long long)ro->n_facets, (int)o->n_modes, p, n_g,
                           d_facets.as<const double>(), pl.data + pl.oE, d_ng.as<double>());
    else
        hipLaunchKernelGGL(k_robust_slack, dim3(blocks_of(ro->n_facets * o->n_modes, 256)),
                           dim3(256), 0, stream, (long long)ro->n_facets, (int)o->n_modes, p,
                           gen.n_g, d_facets.as<const double>(), pl.data + pl.oE, pl.data + o_lo,
                           pl.data + o_hi, d_slack.as<double>());
    (void)hipEventRecord(ev.e1, stream);
    EHM_HIP_TRY(b_err, hipGetLastError());
    EHM_HIP_TRY(b_err, hipStreamSynchronize(stream));
    ev.seconds(&res->seconds_slack);
    RobustArgs A{};
    A.leaf_ids = d_ids.as<const int32_t>();
    A.node = v.node;
    A.leaf_rec = v.leaf_rec;
    A.root_entry = v.root_entry;
    A.root_vertices = d_roots.as<const double>();
    A.par = T.view();
    A.leaf_mode = d_mode.as<const int32_t>();
    A.facets = d_facets.as<const double>();
    A.slack = d_slack.as<const double>();
    A.n_facets = ro->n_facets;
    A.n_u = n_u;
    A.leaf_stride = v.leaf_stride;
    A.o_vlo = o_vlo;
    A.o_vhi = o_vhi;
    A.tol_exit = o->tol_exit;
    A.thr = ro->tol_set * scale;
    A.counters = d_cnt.as<unsigned long long>();
    DevBuf d_vert, d_status, d_margin, d_worst;
    EHM_HIP_TRY(b_err, d_vert.alloc(cap * cell * sizeof(double)));
    EHM_HIP_TRY(b_err, d_status.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(b_err, d_margin.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(b_err, d_worst.alloc(cap * sizeof(int32_t)));
    A.vertices = d_vert.as<double>();
    A.status = d_status.as<int32_t>();
    A.margin = d_margin.as<double>();
    A.worst = d_worst.as<int32_t>();
    if (rr) {
        RA.leaf_ids = A.leaf_ids;
        RA.node = A.node;
        RA.leaf_rec = A.leaf_rec;
        RA.root_entry = A.root_entry;
        RA.root_vertices = A.root_vertices;
        RA.par = A.par;
        RA.leaf_mode = A.leaf_mode;
        RA.n_u = n_u;
        RA.leaf_stride = v.leaf_stride;
        RA.n_dd = rp.n_dd;
        RA.n_v = rp.n_v;
        RA.n_e = rp.n_e;
        RA.n_g = n_g;
        RA.iters = rr->radius_iters;
        RA.o_xabs = o_xabs;
        RA.o_uabs = o_uabs;
        RA.box_n = (long long)cap;
        RA.box = d_box.as<double>();
        RA.x_abs_leaf = d_xl.as<double>();
        RA.x_next_abs = d_xn.as<double>();
        RA.u_abs_leaf = d_ul.as<double>();
        LB.box = d_box.as<const double>();
        LB.box_n = (long long)cap;
        LB.nG = d_ng.as<const double>();
        LB.n_g = n_g;
        LB.n_dd = rp.n_dd;
        LB.n_v = rp.n_v;
    }
    const size_t lds_radii = rr ? plant_bytes + (size_t)rr->n_data * sizeof(double) : 0;
    std::vector<double> hbox(lb ? 2 * (size_t)n_g * cap : 0);
    std::vector<double> hvert(cap * cell), vsub;
    std::vector<long long> has;
    bool have_worst = false;
    for (long long off = 0; off < o->n; off += chunk) {
        const long long nc = std::min<long long>(chunk, o->n - off);
        if (o->leaf_ids)
            EHM_HIP_TRY(b_err, hipMemcpyAsync(d_ids.ptr, o->leaf_ids + off,
                                              (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice,
                                              stream));
        A.n = nc;
        A.first = off;
        const dim3 grid(blocks_of(nc, EHM_ROB_BLOCK)), block(EHM_ROB_BLOCK);
        if (rr) {
            RA.n = nc;
            RA.first = off;
            (void)hipEventRecord(ev_radii.e0, stream);
            hipLaunchKernelGGL((v.single ? k_rad32 : k_rad64)[p - 1], grid, dim3(EHM_RAD_BLOCK),
                               lds_radii, stream, RA, pl, rp.nz);
            (void)hipEventRecord(ev_radii.e1, stream);
            EHM_HIP_TRY(b_err, hipGetLastError());
        }
        (void)hipEventRecord(ev.e0, stream);
        if (rr)
            hipLaunchKernelGGL((v.single ? k_robl32 : k_robl64)[p - 1], grid, block, lds, stream, A,
                               pl, LB);
        else
            hipLaunchKernelGGL((v.single ? k_rob32 : k_rob64)[p - 1], grid, block, lds, stream, A,
                               pl);
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(b_err, hipGetLastError());
        if (lb) {
            if (!hbox.empty())
                EHM_HIP_TRY(b_err, hipMemcpyAsync(hbox.data(), d_box.ptr,
                                                  hbox.size() * sizeof(double),
                                                  hipMemcpyDeviceToHost, stream));
            if (lb->x_abs_leaf)
                EHM_HIP_TRY(b_err, hipMemcpyAsync(lb->x_abs_leaf + off * p, d_xl.ptr,
                                                  (size_t)nc * p * sizeof(double),
                                                  hipMemcpyDeviceToHost, stream));
            if (lb->x_next_abs)
                EHM_HIP_TRY(b_err, hipMemcpyAsync(lb->x_next_abs + off * p, d_xn.ptr,
                                                  (size_t)nc * p * sizeof(double),
                                                  hipMemcpyDeviceToHost, stream));
            if (lb->u_abs_leaf)
                EHM_HIP_TRY(b_err, hipMemcpyAsync(lb->u_abs_leaf + off * n_u, d_ul.ptr,
                                                  (size_t)nc * n_u * sizeof(double),
                                                  hipMemcpyDeviceToHost, stream));
        }
        EHM_HIP_TRY(b_err, hipMemcpyAsync(hvert.data(), d_vert.ptr,
                                          (size_t)nc * cell * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(b_err, hipMemcpyAsync(lv->status + off, d_status.ptr,
                                          (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(b_err, hipMemcpyAsync(lv->margin + off, d_margin.ptr,
                                          (size_t)nc * sizeof(double), hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(b_err, hipMemcpyAsync(lv->worst + off, d_worst.ptr,
                                          (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(b_err, hipStreamSynchronize(stream));
        double s = 0.0;
        ev.seconds(&s);
        res->seconds += s;
        if (rr && lb) {
            ev_radii.seconds(&s);
            lb->seconds_radii += s;
            // the chunk's box, leaf-fastest, into the caller's arrays by kind: [n][2][dim]
            struct { double* out; int col0, dim; } kinds[4] = {
                {lb->d, 0, rp.n_dd}, {lb->v, rp.n_dd, rp.n_v},
                {lb->e, rp.n_dd + rp.n_v, rp.n_e}, {lb->v_next, rp.n_dd + rp.n_v + rp.n_e, rp.n_v}};
            for (const auto& kd : kinds) {
                if (!kd.out) continue;
                for (long long q = 0; q < nc; ++q)
                    for (int side = 0; side < 2; ++side)
                        for (int k = 0; k < kd.dim; ++k)
                            kd.out[((size_t)(off + q) * 2 + side) * kd.dim + k] =
                                hbox[((size_t)side * n_g + kd.col0 + k) * cap + (size_t)q];
            }
        }
        // the worst leaf and the volumes, in leaf order
        has.clear();
        for (long long q = 0; q < nc; ++q) {
            const int st = lv->status[off + q];
            const double mg = lv->margin[off + q];
            if ((st == ROB_INVARIANT || st == ROB_EXITS) && mg == mg &&
                (!have_worst || mg < res->worst_margin)) {
                have_worst = true;
                res->worst_margin = mg;
                res->worst_leaf = off + q;
            }
            if (st != ROB_NO_CELL) has.push_back(q);
        }
        rc = cell_volumes(b_err, who, v.device, p, hvert.data(), has, vsub);
        if (rc) return rc;
        for (size_t a = 0; a < has.size(); ++a) {
            res->cell_volume += vsub[a];
            if (lv->status[off + has[a]] == ROB_INVARIANT) res->invariant_volume += vsub[a];
        }
    }
    unsigned long long cnt[EHM_ROB_STATUSES];
    EHM_HIP_TRY(b_err, hipMemcpy(cnt, d_cnt.ptr, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < EHM_ROB_STATUSES; ++i) res->counts[i] = (int64_t)cnt[i];
    return EHM_OK;
}

}  // namespace

extern "C" {

int ehm_compiled_robust_successors(ehm_compiled* law, const ehm_invariance_opts* o,
                                   const ehm_robust_opts* ro, ehm_robust_result* res,
                                   const ehm_robust_leaves* lv) {
    return robust_run(law, o, ro, nullptr, res, lv, nullptr, "robust_successors");
}

int ehm_compiled_robust_successors_leaf(ehm_compiled* law, const ehm_invariance_opts* o,
                                        const ehm_robust_opts* ro, const ehm_robust_radii* rr,
                                        ehm_robust_result* res, const ehm_robust_leaves* lv,
                                        ehm_robust_leaf_boxes* lb) {
    if (!rr) return b_err.fail(EHM_E_INVALID, "robust_successors_leaf: bad argument");
    return robust_run(law, o, ro, rr, res, lv, lb, "robust_successors_leaf");
}

}  // extern "C"
