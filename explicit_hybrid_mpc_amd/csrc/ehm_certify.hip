// Leaf cells of a compiled law, rebuilt from its own arrays, the input the leaf's own map gives at
// each of their vertices, and the certificate of the law leaf by leaf that starts from them
// (DESIGN.md section 3.8f).  A compiled law keeps no vertices; every split was a bisection, so the
// cell of a leaf follows from its root's vertices and the turns of its path.  On a leaf the law is
// affine, so for a fixed commutation the cost of its input is convex along the leaf and lies below
// the interpolation of its values at the cell's vertices: ehm_bar_e_batch closing the cell with
// those values as Vbar proves the contract of the applied audit (3.8e) at every state of the leaf.
//
//   k_certify_roots    one thread per root: its entry's parent is ~root
//   k_certify_parents  one thread per internal record: the parent and the side of its two children
//                      (children come after their parents, so no record is written twice by a law
//                      whose records form a forest)
//   k_certify_cells    one thread per requested leaf, templated on the law's scalar and on P: up to
//                      the root through the parent table, the turns in a set of 256 bits; down from
//                      the root's vertices, at every plane node s_i = a . v_i + b in double, the one
//                      vertex above 0.5 and the one below -0.5 the ends of the bisected edge, their
//                      midpoint (v + w) / 2 in place of the negative-side vertex in the left child
//                      and of the positive-side one in the right child; then the leaf's affine map
//                      at the p + 1 vertices in the law's own arithmetic
//   k_certify_pack     one thread per (leaf, vertex): theta' = (v, ubar) of the applied-input problem,
//                      the cost constant, the flag of an input that is not finite
//                      (pack_applied_row of ehm_verdict.h)
//   k_certify_judge    one thread per leaf: its status from what the host's batches found, the
//                      counts by integer atomics, the worst uncertified leaf per workgroup (the
//                      counters and the tree of ehm_verdict.h)
//
// ehm_compiled_certify runs the batched oracles between them (ehm_point_idx_batch on the applied
// problem, ehm_bar_e_batch on the oracle's): host-orchestrated over the batched kernels like every
// multi-commutation oracle of ehm_capi.hip; a chunk's rows make their round trips through the host,
// which the LP batches dwarf.
//
// The parent table, the cell of a leaf and the leaf's map at a vertex are ehm_cells_dev.h's, which
// ehm_reduce.hip shares.  The cell lives in registers: (P + 1) P <= 72 doubles, indexed statically
// throughout.  Every
// operation a result depends on runs under fp contract(off) in a fixed order
// (tests/certify_cpu.py is the numpy mirror).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_verdict.h"

#define EHM_CERT_BLOCK 64
#define EHM_CERT_CHUNK 65536        // leaves per pass of ehm_compiled_cells
#define EHM_CERT_PASS 8192          // leaves per pass of ehm_compiled_certify (opts->chunk = 0)
#define EHM_CERT_JUDGE_BLOCK 256
#define EHM_CERT_FEAS_TOL 1e-8      // EHM_FEAS_TOL of the batched oracles: feasible iff tau <= this

static_assert(EHM_CERT_MAX_DEPTH == EHM_CELL_MAX_DEPTH, "the turn set holds EHM_CELL_MAX_DEPTH bits");

namespace {

using ehm_cert::Parents;
using ehm_cert::TurnSet;

template <class T>
struct CellArgs {
    long long n;
    const int32_t* leaf_ids;        // or nullptr: leaves first .. first + n - 1
    long long first;
    const T* node;
    const T* leaf_rec;
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    Parents par;
    int n_u, leaf_stride;
    double* vertices;               // [n][P+1][P]
    double* ubar;                   // [n][P+1][n_u] or nullptr
    int32_t* status;                // [n]
};

template <class T, int P>
__global__ __launch_bounds__(EHM_CERT_BLOCK) void k_certify_cells(CellArgs<T> A) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n) return;
    const int32_t l = A.leaf_ids ? A.leaf_ids[q] : (int32_t)(A.first + q);
    double V[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, A.node, A.root_entry, A.root_vertices, l, V);
    double* out = A.vertices + (size_t)q * (P + 1) * P;
#pragma unroll
    for (int e = 0; e < (P + 1) * P; ++e) out[e] = ok ? V[e] : NAN;
    A.status[q] = ok ? EHM_CELL_OK : EHM_CELL_NO_CELL;
    if (!A.ubar) return;
    // the leaf's own map at every vertex: the leaf-map part of law_input (ehm_compiled_dev.h)
    const int n_u = A.n_u;
    double* ub = A.ubar + (size_t)q * (P + 1) * n_u;
    if (!ok) {
        for (int e = 0; e < (P + 1) * n_u; ++e) ub[e] = NAN;
        return;
    }
    const T* lr = A.leaf_rec + (size_t)l * A.leaf_stride;
#pragma unroll
    for (int i = 0; i <= P; ++i)
        for (int c = 0; c < n_u; ++c) ub[i * n_u + c] = leaf_map_at<P>(lr, n_u, c, &V[i * P]);
}

// theta' = (v_i, ubar_i) and konst_i of every (leaf, vertex) pair; a pair without a cell enters as
// zeros, a component that is not finite flags the leaf
__global__ void k_certify_pack(long long n_pairs, int p, int n_u, const double* __restrict__ V,
                               const double* __restrict__ U, const int32_t* __restrict__ cell,
                               const double* __restrict__ cost_u, double* __restrict__ theta,
                               double* __restrict__ konst, int32_t* __restrict__ no_law) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    const long long leaf = q / (p + 1);
    const bool has = cell[leaf] == EHM_CELL_OK;
    const bool bad = ehm_verdict::pack_applied_row(
        p, n_u, [&](int c) { return has ? V[q * p + c] : 0.0; },
        [&](int j) { return has ? U[q * n_u + j] : 0.0; }, cost_u, theta + (size_t)q * (p + n_u),
        &konst[q]);
    if (bad) atomicOr(&no_law[leaf], 1);
}

__global__ __launch_bounds__(EHM_CERT_JUDGE_BLOCK) void k_certify_judge(
    long long n, long long first, const int32_t* __restrict__ cell,
    const int32_t* __restrict__ no_law, const int32_t* __restrict__ n_cand,
    const int32_t* __restrict__ n_aside, const int32_t* __restrict__ closed_d,
    const double* __restrict__ tbest, int32_t* __restrict__ status,
    unsigned long long* __restrict__ counters, double* __restrict__ blk_t,
    long long* __restrict__ blk_i) {
    __shared__ unsigned int cnt[ehm_cert::CERT_STATUSES];
    ehm_verdict::counters_zero<EHM_CERT_JUDGE_BLOCK, ehm_cert::CERT_STATUSES>(cnt);
    __syncthreads();
    const long long q = (long long)blockIdx.x * EHM_CERT_JUDGE_BLOCK + threadIdx.x;
    double tb = -INFINITY;
    long long id = -1;
    if (q < n) {
        const int s = ehm_cert::certify_status(cell[q] == EHM_CELL_OK, no_law[q], n_cand[q],
                                               n_aside[q], closed_d[q] >= 0);
        status[q] = s;
        atomicAdd(&cnt[s], 1u);
        if (s == ehm_cert::CERT_UNCERTIFIED && tbest[q] == tbest[q]) {
            tb = tbest[q];
            id = first + q;
        }
    }
    ehm_verdict::block_worst<EHM_CERT_JUDGE_BLOCK>(
        tb, id,
        [](double ta, long long ia, double tb_, long long ib) {
            return ehm_cert::worst_beats(ta, ia, tb_, ib);
        },
        [](long long i) { return i >= 0; });
    if (threadIdx.x == 0) {
        blk_t[blockIdx.x] = tb;
        blk_i[blockIdx.x] = id;
    }
    ehm_verdict::counters_flush<EHM_CERT_JUDGE_BLOCK, ehm_cert::CERT_STATUSES>(cnt, counters);
}

typedef void (*cells64_fn)(CellArgs<double>);
typedef void (*cells32_fn)(CellArgs<float>);
#define EHM_CERT_ALL(T) {&k_certify_cells<T, 1>, &k_certify_cells<T, 2>, &k_certify_cells<T, 3>, \
                         &k_certify_cells<T, 4>, &k_certify_cells<T, 5>, &k_certify_cells<T, 6>, \
                         &k_certify_cells<T, 7>, &k_certify_cells<T, 8>}
const cells64_fn k_cells64[EHM_CP] = EHM_CERT_ALL(double);
const cells32_fn k_cells32[EHM_CP] = EHM_CERT_ALL(float);
#undef EHM_CERT_ALL

thread_local ehm_err_channel z_err;

// what both entry points check of a law and of the caller's leaves
int check_law(const ehm_compiled_view& v, int64_t n, const int32_t* leaf_ids, const char* who) {
    const int rc = check_law_shape(z_err, v, who);
    return rc ? rc : check_law_leaves(z_err, v, n, leaf_ids, who);
}

// k_certify_cells for the leaves ids[0 .. nc - 1] (device; nullptr: first .. first + nc - 1)
void launch_cells(const ehm_compiled_view& v, hipStream_t stream, const ParentTable& T,
                  const double* roots, const int32_t* ids, long long first, long long nc,
                  double* vert, double* ubar, int32_t* status) {
    const dim3 grid(blocks_of(nc, EHM_CERT_BLOCK)), block(EHM_CERT_BLOCK);
    if (v.single) {
        CellArgs<float> A{nc, ids, first, static_cast<const float*>(v.node),
                          static_cast<const float*>(v.leaf_rec), v.root_entry, roots, T.view(),
                          v.n_u, v.leaf_stride, vert, ubar, status};
        hipLaunchKernelGGL(k_cells32[v.p - 1], grid, block, 0, stream, A);
    } else {
        CellArgs<double> A{nc, ids, first, static_cast<const double*>(v.node),
                           static_cast<const double*>(v.leaf_rec), v.root_entry, roots, T.view(),
                           v.n_u, v.leaf_stride, vert, ubar, status};
        hipLaunchKernelGGL(k_cells64[v.p - 1], grid, block, 0, stream, A);
    }
}

// one candidate commutation of a leaf
struct Candidate {
    int32_t d;
    bool aside;                 // a vertex solve stalled: not tried
    double key;
    double W[EHM_CP + 1];
};

// The candidates of the leaves `todo` (positions in the chunk) on problem P: the commutations
// feasible at all nv vertices, by index ascending, with their vertex costs.
int find_candidates(ehm_problem* P, const std::vector<long long>& todo, int nv, int pp, int nd,
                    const double* theta, const double* konst,
                    std::vector<std::vector<Candidate>>& cand, double* t_feas, double* t_cost) {
    if (todo.empty()) return EHM_OK;
    auto t0 = std::chrono::steady_clock::now();
    const size_t pairs = todo.size() * (size_t)nv * nd;
    std::vector<double> th(pairs * pp), tau(pairs);
    std::vector<int32_t> slot(pairs);
    size_t r = 0;
    for (long long q : todo)
        for (int i = 0; i < nv; ++i)
            for (int d = 0; d < nd; ++d, ++r) {
                std::memcpy(&th[r * pp], theta + ((size_t)q * nv + i) * pp, pp * sizeof(double));
                slot[r] = d;
            }
    int rc = ehm_point_idx_batch(P, (int64_t)pairs, th.data(), slot.data(), 1, tau.data(), nullptr,
                                 nullptr);
    if (rc) return z_err.fail(rc, "certify: ehm_point_idx_batch (feasibility): %s",
                              ehm_last_error());
    *t_feas += wall_since(t0);
    t0 = std::chrono::steady_clock::now();
    std::vector<long long> who;         // (leaf position, commutation) of every candidate
    std::vector<int32_t> which;
    for (size_t a = 0; a < todo.size(); ++a)
        for (int d = 0; d < nd; ++d) {
            bool all = true;
            for (int i = 0; i < nv; ++i)
                all = all && tau[(a * nv + i) * nd + d] <= EHM_CERT_FEAS_TOL;
            if (all) {
                who.push_back(todo[a]);
                which.push_back(d);
            }
        }
    if (who.empty()) return EHM_OK;
    const size_t rows = who.size() * (size_t)nv;
    th.resize(rows * pp);
    slot.resize(rows);
    std::vector<double> J(rows);
    std::vector<int32_t> st(rows);
    for (size_t a = 0; a < who.size(); ++a)
        for (int i = 0; i < nv; ++i) {
            std::memcpy(&th[(a * nv + i) * pp], theta + ((size_t)who[a] * nv + i) * pp,
                        pp * sizeof(double));
            slot[a * nv + i] = which[a];
        }
    rc = ehm_point_idx_batch(P, (int64_t)rows, th.data(), slot.data(), 0, J.data(), nullptr,
                             st.data());
    if (rc) return z_err.fail(rc, "certify: ehm_point_idx_batch (costs): %s", ehm_last_error());
    for (size_t a = 0; a < who.size(); ++a) {
        Candidate c{};
        c.d = which[a];
        for (int i = 0; i < nv; ++i) {
            c.W[i] = J[a * nv + i] + konst[(size_t)who[a] * nv + i];
            c.aside = c.aside || st[a * nv + i] != EHM_ST_OPTIMAL;
        }
        c.key = ehm_cert::candidate_key(c.W, nv);
        cand[(size_t)who[a]].push_back(c);
    }
    *t_cost += wall_since(t0);
    return EHM_OK;
}

}  // namespace

extern "C" {

const char* ehm_certify_last_error(void) { return z_err.c_str(); }

int ehm_certify_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_certify_opts), (int64_t)sizeof(ehm_certify_result),
                           (int64_t)sizeof(ehm_certify_leaves)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_compiled_cells(ehm_compiled* law, const double* root_vertices, int64_t n,
                       const int32_t* leaf_ids, double* vertices, double* ubar, int32_t* status) {
    if (!law || !root_vertices || n < 0 || (n > 0 && (!vertices || !status)))
        return z_err.fail(EHM_E_INVALID, "cells: bad argument");
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    int rc = check_law(v, n, leaf_ids, "cells");
    if (rc) return rc;
    if (n == 0) return EHM_OK;
    EHM_HIP_TRY(z_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(z_err, stream.create());
    const int p = v.p, n_u = v.n_u;
    const size_t cell = (size_t)(p + 1) * p;
    ParentTable T;
    EHM_HIP_TRY(z_err, make_parents(v, stream, T));
    DevBuf droots, dids, dvert, dubar, dstatus;
    EHM_HIP_TRY(z_err, droots.upload(root_vertices, (size_t)v.n_roots * cell * sizeof(double)));
    const size_t cap = (size_t)std::min<int64_t>(n, EHM_CERT_CHUNK);
    if (leaf_ids) EHM_HIP_TRY(z_err, dids.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dvert.alloc(cap * cell * sizeof(double)));
    if (ubar) EHM_HIP_TRY(z_err, dubar.alloc(cap * (size_t)(p + 1) * n_u * sizeof(double)));
    EHM_HIP_TRY(z_err, dstatus.alloc(cap * sizeof(int32_t)));
    for (int64_t off = 0; off < n; off += EHM_CERT_CHUNK) {
        const int64_t nc = std::min<int64_t>(EHM_CERT_CHUNK, n - off);
        if (leaf_ids)
            EHM_HIP_TRY(z_err, hipMemcpyAsync(dids.ptr, leaf_ids + off,
                                              (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice,
                                              stream));
        launch_cells(v, stream, T, droots.as<const double>(),
                     leaf_ids ? dids.as<const int32_t>() : nullptr, off, nc, dvert.as<double>(),
                     ubar ? dubar.as<double>() : nullptr, dstatus.as<int32_t>());
        EHM_HIP_TRY(z_err, hipGetLastError());
        EHM_HIP_TRY(z_err, hipMemcpyAsync(vertices + (size_t)off * cell, dvert.ptr,
                                          (size_t)nc * cell * sizeof(double), hipMemcpyDeviceToHost,
                                          stream));
        if (ubar)
            EHM_HIP_TRY(z_err, hipMemcpyAsync(ubar + (size_t)off * (p + 1) * n_u, dubar.ptr,
                                              (size_t)nc * (p + 1) * n_u * sizeof(double),
                                              hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(status + off, dstatus.ptr, (size_t)nc * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipStreamSynchronize(stream));
    }
    return EHM_OK;
}

int ehm_compiled_certify(ehm_compiled* law, ehm_problem* oracle, ehm_problem* applied,
                         const ehm_certify_opts* o, ehm_certify_result* res,
                         const ehm_certify_leaves* lv) {
    if (!law || !oracle || !applied || !o || !res)
        return z_err.fail(EHM_E_INVALID, "certify: bad argument");
    if (o->n < 0 || o->chunk < 0 || o->max_tries < 0 || o->n_delta < 1)
        return z_err.fail(EHM_E_INVALID, "certify: n, chunk, max_tries < 0 or n_delta < 1");
    if (o->p < 1 || o->n_u < 1 || o->p + o->n_u > EHM_MAX_P)
        return z_err.fail(EHM_E_INVALID, "certify: p = %d, n_u = %d: p + n_u must be <= %d",
                          (int)o->p, (int)o->n_u, EHM_MAX_P);
    if (!o->cost_u || !o->root_vertices)
        return z_err.fail(EHM_E_INVALID, "certify: no cost_u or no root vertices");
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    if (v.p != o->p || v.n_u != o->n_u)
        return z_err.fail(EHM_E_INVALID, "certify: the law has p = %d, n_u = %d, the options %d, "
                          "%d", v.p, v.n_u, (int)o->p, (int)o->n_u);
    int rc = check_law(v, o->n, o->leaf_ids, "certify");
    if (rc) return rc;
    std::memset(res, 0, sizeof *res);
    res->worst_leaf = -1;
    res->worst_tbest = NAN;
    if (o->n == 0) return EHM_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || o->device < 0 || o->device >= ndev)
        return z_err.fail(EHM_E_NO_DEVICE, "no HIP device %d (libehmpc has no CPU fallback)",
                          (int)o->device);
    EHM_HIP_TRY(z_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(z_err, stream.create());
    const int p = v.p, n_u = v.n_u, nv = p + 1, pp = p + n_u, nd = o->n_delta;
    const size_t cell = (size_t)nv * p;
    ParentTable T;
    EHM_HIP_TRY(z_err, make_parents(v, stream, T));
    const long long chunk = o->chunk > 0 ? o->chunk : EHM_CERT_PASS;
    const size_t cap = (size_t)std::min<long long>(chunk, o->n);
    const unsigned max_blocks = blocks_of((long long)cap, EHM_CERT_JUDGE_BLOCK);
    DevBuf droots, dcost, dids, dvert, dubar, dcell, dtheta, dkonst, dnolaw, dncand, dnaside,
        dclosed, dtbest, dstatus, dcnt, dbt, dbi;
    EHM_HIP_TRY(z_err, droots.upload(o->root_vertices, (size_t)v.n_roots * cell * sizeof(double)));
    EHM_HIP_TRY(z_err, dcost.upload(o->cost_u, (size_t)n_u * sizeof(double)));
    if (o->leaf_ids) EHM_HIP_TRY(z_err, dids.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dvert.alloc(cap * cell * sizeof(double)));
    EHM_HIP_TRY(z_err, dubar.alloc(cap * nv * n_u * sizeof(double)));
    EHM_HIP_TRY(z_err, dcell.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dtheta.alloc(cap * nv * pp * sizeof(double)));
    EHM_HIP_TRY(z_err, dkonst.alloc(cap * nv * sizeof(double)));
    EHM_HIP_TRY(z_err, dnolaw.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dncand.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dnaside.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dclosed.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dtbest.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(z_err, dstatus.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(z_err, dcnt.alloc(ehm_cert::CERT_STATUSES * sizeof(unsigned long long)));
    EHM_HIP_TRY(z_err, dbt.alloc(max_blocks * sizeof(double)));
    EHM_HIP_TRY(z_err, dbi.alloc(max_blocks * sizeof(long long)));
    EHM_HIP_TRY(z_err, hipMemsetAsync(dcnt.ptr, 0,
                                      ehm_cert::CERT_STATUSES * sizeof(unsigned long long),
                                      stream));
    std::vector<double> hvert(cap * cell), hubar(cap * nv * n_u), htheta(cap * nv * pp),
        hkonst(cap * nv), htbest(cap), hvol(cap), hW(cap * nv), hbt(max_blocks), R, Vb, tb, vsub;
    std::vector<int32_t> hcell(cap), hnolaw(cap), hncand(cap), hnaside(cap), hclosed(cap),
        htries(cap), hrelaxed(cap), hstatus(cap);
    std::vector<long long> hbi(max_blocks), todo, open, next;
    std::vector<uint8_t> closed;
    std::vector<std::vector<Candidate>> cand(cap);
    std::vector<std::vector<int32_t>> order(cap);
    std::vector<double> keys;
    EventPair ev_c, ev_j;
    long long worst_leaf = -1;
    double worst_tbest = NAN;
    for (long long off = 0; off < o->n; off += chunk) {
        const long long nc = std::min<long long>(chunk, o->n - off);
        auto t_pass = std::chrono::steady_clock::now();
        const double before = res->seconds[1] + res->seconds[2] + res->seconds[3] + res->seconds[4];
        // the cells, the vertex inputs and the rows of the applied problem
        if (o->leaf_ids)
            EHM_HIP_TRY(z_err, hipMemcpyAsync(dids.ptr, o->leaf_ids + off,
                                              (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice,
                                              stream));
        EHM_HIP_TRY(z_err, hipMemsetAsync(dnolaw.ptr, 0, (size_t)nc * sizeof(int32_t), stream));
        (void)hipEventRecord(ev_c.e0, stream);
        launch_cells(v, stream, T, droots.as<const double>(),
                     o->leaf_ids ? dids.as<const int32_t>() : nullptr, off, nc, dvert.as<double>(),
                     dubar.as<double>(), dcell.as<int32_t>());
        hipLaunchKernelGGL(k_certify_pack, dim3(blocks_of(nc * nv, 256)), dim3(256), 0, stream,
                           nc * nv, p, n_u, dvert.as<const double>(), dubar.as<const double>(),
                           dcell.as<const int32_t>(), dcost.as<const double>(),
                           dtheta.as<double>(), dkonst.as<double>(), dnolaw.as<int32_t>());
        (void)hipEventRecord(ev_c.e1, stream);
        EHM_HIP_TRY(z_err, hipGetLastError());
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hvert.data(), dvert.ptr,
                                          (size_t)nc * cell * sizeof(double), hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hubar.data(), dubar.ptr,
                                          (size_t)nc * nv * n_u * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hcell.data(), dcell.ptr, (size_t)nc * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(htheta.data(), dtheta.ptr,
                                          (size_t)nc * nv * pp * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hkonst.data(), dkonst.ptr,
                                          (size_t)nc * nv * sizeof(double), hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hnolaw.data(), dnolaw.ptr, (size_t)nc * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipStreamSynchronize(stream));
        // candidates: on the exact substitution, and where it gives none on the relaxed problem
        todo.clear();
        for (long long q = 0; q < nc; ++q) {
            cand[q].clear();
            order[q].clear();
            hrelaxed[q] = 0;
            htries[q] = 0;
            hclosed[q] = -1;
            htbest[q] = NAN;
            hvol[q] = NAN;
            for (int i = 0; i < nv; ++i) hW[(size_t)q * nv + i] = NAN;
            if (hcell[q] == EHM_CELL_OK && !hnolaw[q]) todo.push_back(q);
        }
        rc = find_candidates(applied, todo, nv, pp, nd, htheta.data(), hkonst.data(), cand,
                             &res->seconds[1], &res->seconds[2]);
        if (rc) return rc;
        if (o->relaxed) {
            next.clear();
            for (long long q : todo)
                if (cand[q].empty()) next.push_back(q);
            rc = find_candidates(o->relaxed, next, nv, pp, nd, htheta.data(), hkonst.data(), cand,
                                 &res->seconds[1], &res->seconds[2]);
            if (rc) return rc;
            for (long long q : next)
                if (!cand[q].empty()) {
                    hrelaxed[q] = 1;
                    res->relaxed += 1;
                }
        }
        // the order of the tries
        open.clear();
        for (long long q : todo) {
            std::vector<int32_t> live;
            keys.clear();
            for (size_t a = 0; a < cand[q].size(); ++a)
                if (!cand[q][a].aside) {
                    live.push_back((int32_t)a);
                    keys.push_back(cand[q][a].key);
                }
            std::vector<int32_t> rank(live.size());
            ehm_cert::order_candidates((int)live.size(), keys.data(), rank.data());
            for (int32_t r : rank) order[q].push_back(live[(size_t)r]);
            if (!order[q].empty()) open.push_back(q);
        }
        for (long long q = 0; q < nc; ++q) {
            hncand[q] = (int32_t)cand[q].size();
            hnaside[q] = hncand[q] - (int32_t)order[q].size();
        }
        // the tests: every open leaf with its next candidate, until it closes or runs out
        auto t0 = std::chrono::steady_clock::now();
        for (int t = 0; !open.empty() && (o->max_tries == 0 || t < o->max_tries); ++t) {
            const size_t nb = open.size();
            R.resize(nb * cell);
            Vb.resize(nb * nv);
            closed.resize(nb);
            tb.resize(nb);
            for (size_t a = 0; a < nb; ++a) {
                const long long q = open[a];
                const Candidate& c = cand[q][(size_t)order[q][(size_t)t]];
                std::memcpy(&R[a * cell], &hvert[(size_t)q * cell], cell * sizeof(double));
                std::memcpy(&Vb[a * nv], c.W, nv * sizeof(double));
            }
            rc = ehm_bar_e_batch(oracle, (int64_t)nb, R.data(), Vb.data(), closed.data(),
                                 tb.data());
            if (rc) return z_err.fail(rc, "certify: ehm_bar_e_batch: %s", ehm_last_error());
            next.clear();
            for (size_t a = 0; a < nb; ++a) {
                const long long q = open[a];
                const Candidate& c = cand[q][(size_t)order[q][(size_t)t]];
                htries[q] = t + 1;
                htbest[q] = tb[a];
                std::memcpy(&hW[(size_t)q * nv], c.W, nv * sizeof(double));
                if (closed[a]) hclosed[q] = c.d;
                else if ((size_t)t + 1 < order[q].size()) next.push_back(q);
            }
            open.swap(next);
        }
        res->seconds[3] += wall_since(t0);
        // the volumes of the cells
        t0 = std::chrono::steady_clock::now();
        todo.clear();
        for (long long q = 0; q < nc; ++q)
            if (hcell[q] == EHM_CELL_OK) todo.push_back(q);
        rc = cell_volumes(z_err, "certify", v.device, p, hvert.data(), todo, vsub);
        if (rc) return rc;
        for (size_t a = 0; a < todo.size(); ++a) hvol[(size_t)todo[a]] = vsub[a];
        res->seconds[4] += wall_since(t0);
        // the judgement (the oracles above may have left another device current)
        EHM_HIP_TRY(z_err, hipSetDevice(v.device));
        const unsigned nblk = blocks_of(nc, EHM_CERT_JUDGE_BLOCK);
        EHM_HIP_TRY(z_err, hipMemcpyAsync(dncand.ptr, hncand.data(), (size_t)nc * sizeof(int32_t),
                                          hipMemcpyHostToDevice, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(dnaside.ptr, hnaside.data(), (size_t)nc * sizeof(int32_t),
                                          hipMemcpyHostToDevice, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(dclosed.ptr, hclosed.data(), (size_t)nc * sizeof(int32_t),
                                          hipMemcpyHostToDevice, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(dtbest.ptr, htbest.data(), (size_t)nc * sizeof(double),
                                          hipMemcpyHostToDevice, stream));
        (void)hipEventRecord(ev_j.e0, stream);
        hipLaunchKernelGGL(k_certify_judge, dim3(nblk), dim3(EHM_CERT_JUDGE_BLOCK), 0, stream, nc,
                           off, dcell.as<const int32_t>(), dnolaw.as<const int32_t>(),
                           dncand.as<const int32_t>(), dnaside.as<const int32_t>(),
                           dclosed.as<const int32_t>(), dtbest.as<const double>(),
                           dstatus.as<int32_t>(), dcnt.as<unsigned long long>(), dbt.as<double>(),
                           dbi.as<long long>());
        (void)hipEventRecord(ev_j.e1, stream);
        EHM_HIP_TRY(z_err, hipGetLastError());
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hstatus.data(), dstatus.ptr, (size_t)nc * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hbt.data(), dbt.ptr, nblk * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipMemcpyAsync(hbi.data(), dbi.ptr, nblk * sizeof(long long),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(z_err, hipStreamSynchronize(stream));
        double s = 0.0;
        ev_c.seconds(&s);
        res->seconds[0] += s;
        ev_j.seconds(&s);
        res->seconds[0] += s;
        if (ehm_verdict::merge_block_worst(hbt.data(), hbi.data(), nblk, -1LL,
                                           ehm_cert::worst_beats, worst_tbest, worst_leaf)) {
            res->worst_tbest = worst_tbest;
            res->worst_leaf = worst_leaf;
        }
        for (long long q = 0; q < nc; ++q) {
            if (hcell[q] == EHM_CELL_OK) res->cell_volume += hvol[q];
            if (hstatus[q] == ehm_cert::CERT_CERTIFIED) res->certified_volume += hvol[q];
        }
        if (lv) {
            const size_t n4 = (size_t)nc * sizeof(int32_t), n8 = (size_t)nc * sizeof(double);
            if (lv->status) std::memcpy(lv->status + off, hstatus.data(), n4);
            if (lv->delta_idx) std::memcpy(lv->delta_idx + off, hclosed.data(), n4);
            if (lv->tbest) std::memcpy(lv->tbest + off, htbest.data(), n8);
            if (lv->tries) std::memcpy(lv->tries + off, htries.data(), n4);
            if (lv->relaxed) std::memcpy(lv->relaxed + off, hrelaxed.data(), n4);
            if (lv->n_candidates) std::memcpy(lv->n_candidates + off, hncand.data(), n4);
            if (lv->volume) std::memcpy(lv->volume + off, hvol.data(), n8);
            if (lv->vertices) std::memcpy(lv->vertices + (size_t)off * cell, hvert.data(), n8 * cell);
            if (lv->inputs)
                std::memcpy(lv->inputs + (size_t)off * nv * n_u, hubar.data(), n8 * nv * n_u);
            if (lv->W) std::memcpy(lv->W + (size_t)off * nv, hW.data(), n8 * nv);
        }
        const double batches = res->seconds[1] + res->seconds[2] + res->seconds[3] +
                               res->seconds[4] - before;
        res->seconds[5] += wall_since(t_pass) - batches;
    }
    unsigned long long cnt[ehm_cert::CERT_STATUSES];
    EHM_HIP_TRY(z_err, hipMemcpy(cnt, dcnt.ptr, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < ehm_cert::CERT_STATUSES; ++i) res->counts[i] = (int64_t)cnt[i];
    return EHM_OK;
}

}  // extern "C"
