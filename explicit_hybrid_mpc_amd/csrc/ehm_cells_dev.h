// What ehm_certify.hip, ehm_reduce.hip, ehm_invariance.hip and ehm_core.hip share (DESIGN.md 3.8f
// to 3.8i): the parent table of a compiled law, the cell of a leaf rebuilt from the law's own
// arrays with the cell in registers, the leaf's affine map at a vertex in the law's own arithmetic
// and the volumes of a chunk's cells; for the last two what they refuse of the plant they step a
// leaf's vertices through and how they pack it.  The rules of the cells are plain C++ in
// ehm_certify_host.h.  Every translation unit that includes this gets its own copy (unnamed
// namespace), as of ehm_compiled_dev.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "ehm_certify_host.h"
#include "ehm_compiled_dev.h"
#include "ehm_compiled_view.h"
#include "ehm_host.h"

namespace {

__global__ void k_certify_roots(long long n_roots, const int32_t* __restrict__ root_entry,
                                ehm_cert::Parents P) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_roots) return;
    ehm_cert::link_root(P, (int32_t)r, root_entry[r]);
}

template <class T>
__global__ void k_certify_parents(long long n_int, int p, int node_stride,
                                  const T* __restrict__ node, ehm_cert::Parents P) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_int) return;
    int32_t left, right;
    ehm_cert::children_of(node + (size_t)k * node_stride, p, left, right);
    ehm_cert::link_children(P, (int32_t)k, left, right);
}

// the parent table of a law on the device
struct ParentTable {
    DevBuf node, node_side, leaf, leaf_side;
    ehm_cert::Parents view() const {
        return ehm_cert::Parents{node.as<int32_t>(), node_side.as<uint8_t>(), leaf.as<int32_t>(),
                                 leaf_side.as<uint8_t>()};
    }
};

inline hipError_t make_parents(const ehm_compiled_view& v, hipStream_t stream, ParentTable& T) {
#define EHM_CELLS_TRY(expr)                \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return e_;   \
    } while (0)
    EHM_CELLS_TRY(T.node.alloc((size_t)v.n_int * sizeof(int32_t)));
    EHM_CELLS_TRY(T.node_side.alloc((size_t)v.n_int));
    EHM_CELLS_TRY(T.leaf.alloc((size_t)v.n_leaf * sizeof(int32_t)));
    EHM_CELLS_TRY(T.leaf_side.alloc((size_t)v.n_leaf));
    if (v.n_int) {
        EHM_CELLS_TRY(hipMemsetD32Async((hipDeviceptr_t)T.node.ptr, EHM_CERT_UNREACHED,
                                        (size_t)v.n_int, stream));
        EHM_CELLS_TRY(hipMemsetAsync(T.node_side.ptr, 0, (size_t)v.n_int, stream));
    }
    EHM_CELLS_TRY(hipMemsetD32Async((hipDeviceptr_t)T.leaf.ptr, EHM_CERT_UNREACHED,
                                    (size_t)v.n_leaf, stream));
    EHM_CELLS_TRY(hipMemsetAsync(T.leaf_side.ptr, 0, (size_t)v.n_leaf, stream));
    const ehm_cert::Parents P = T.view();
    if (v.n_int) {
        if (v.single)
            hipLaunchKernelGGL(k_certify_parents<float>, dim3(blocks_of(v.n_int, 256)),
                               dim3(256), 0, stream, v.n_int, v.p, v.node_stride,
                               static_cast<const float*>(v.node), P);
        else
            hipLaunchKernelGGL(k_certify_parents<double>, dim3(blocks_of(v.n_int, 256)),
                               dim3(256), 0, stream, v.n_int, v.p, v.node_stride,
                               static_cast<const double*>(v.node), P);
        EHM_CELLS_TRY(hipGetLastError());
    }
    // the roots last: an entry is a root whatever else names it
    hipLaunchKernelGGL(k_certify_roots, dim3(blocks_of(v.n_roots, 256)), dim3(256), 0,
                       stream, v.n_roots, v.root_entry, P);
    EHM_CELLS_TRY(hipGetLastError());
#undef EHM_CELLS_TRY
    return hipSuccess;
}

// What every entry point that rebuilds cells refuses of a law (`who` names the entry point) ...
inline int check_law_shape(ehm_err_channel& err, const ehm_compiled_view& v, const char* who) {
    if (v.n_test > 0)
        return err.fail(EHM_E_INVALID,
                        "%s: the law has %lld test nodes (children that are no bisection); its "
                        "cells do not follow from its planes -- compile it with the spine as its "
                        "root table",
                        who, v.n_test);
    if (v.p < 1 || v.p > EHM_CP) return err.fail(EHM_E_INVALID, "%s: p = %d", who, v.p);
    if (v.n_roots >= 0x7fffffffLL) return err.fail(EHM_E_INVALID, "%s: too many roots", who);
    return EHM_OK;
}

// ... and of the caller's n leaves (leaf_ids nullptr: the first n)
inline int check_law_leaves(ehm_err_channel& err, const ehm_compiled_view& v, int64_t n,
                            const int32_t* leaf_ids, const char* who) {
    if (!leaf_ids && n > v.n_leaf)
        return err.fail(EHM_E_INVALID, "%s: n = %lld of %lld leaves", who, (long long)n, v.n_leaf);
    if (leaf_ids) {
        const int64_t bad = ehm_cert::first_bad_leaf(leaf_ids, n, v.n_leaf);
        if (bad >= 0)
            return err.fail(EHM_E_INVALID, "%s: leaf_ids[%lld] = %d of %lld leaves", who,
                            (long long)bad, (int)leaf_ids[bad], v.n_leaf);
    }
    return EHM_OK;
}

// The cell of leaf record l into V [(P+1) P], statically indexed throughout: up to the root through
// the parent table, the turns in a set of 256 bits; down from the root's vertices, at every plane
// node s_i = a . v_i + b in double, the one vertex above 0.5 and the one below -0.5 the ends of the
// bisected edge, their midpoint (v + w) / 2 in place of the negative-side vertex in the left child
// and of the positive-side one in the right child.  False (V is then not a cell) for a leaf no root
// reaches, one deeper than the set holds and one whose path holds a node that is no bisection.
template <class T, int P>
__device__ __forceinline__ bool leaf_cell(const ehm_cert::Parents& par, const T* __restrict__ node,
                                          const int32_t* __restrict__ root_entry,
                                          const double* __restrict__ root_vertices, int32_t l,
                                          double (&V)[(P + 1) * P]) {
#pragma clang fp contract(off)
    constexpr bool SINGLE = std::is_same<T, float>::value;
    constexpr int NS = SINGLE ? (P <= 5 ? 8 : 16) : (P <= 6 ? 8 : 16);
    ehm_cert::TurnSet turns;
    int32_t root = 0;
    bool ok = ehm_cert::walk_up(par, l, turns, root);
#pragma unroll
    for (int e = 0; e < (P + 1) * P; ++e) V[e] = NAN;
    if (ok) {
        const double* rv = root_vertices + (size_t)root * (P + 1) * P;
#pragma unroll
        for (int e = 0; e < (P + 1) * P; ++e) V[e] = rv[e];
        int32_t k = root_entry[root];
        while (turns.depth > 0) {
            if (k < 0) {
                ok = false;
                break;
            }
            const T* rec = node + (size_t)k * NS;
            double a[P + 1];
#pragma unroll
            for (int c = 0; c <= P; ++c) a[c] = (double)rec[c];
            double s[P + 1];
#pragma unroll
            for (int i = 0; i <= P; ++i) {
                double t = 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) t = t + a[c] * V[i * P + c];
                s[i] = t + a[P];
            }
            int pos, neg;
            if (!ehm_cert::bisected_edge<P + 1>(s, pos, neg)) {
                ok = false;
                break;
            }
            int32_t left, right;
            ehm_cert::children_of(rec, P, left, right);
            const int turn = turns.pop();
            const int gone = turn ? pos : neg;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                double vp = 0.0, vn = 0.0;
#pragma unroll
                for (int i = 0; i <= P; ++i) {
                    vp = i == pos ? V[i * P + c] : vp;
                    vn = i == neg ? V[i * P + c] : vn;
                }
                const double mid = (vn + vp) / 2.0;
#pragma unroll
                for (int i = 0; i <= P; ++i) V[i * P + c] = i == gone ? mid : V[i * P + c];
            }
            k = turn ? right : left;
        }
        ok = ok && k == ~l;
    }
    return ok;
}

// Component c of the map of leaf record lr at the point v [P] in the law's own arithmetic: the
// leaf-map part of law_input (ehm_compiled_dev.h).  A double law: d = v - v_0,
// u_c = u_0c + ((0 + K_c0 d_0) + .. + K_c(P-1) d_(P-1)) in double; a single law: xs = (float) v and
// leaf_offset32 / leaf_input32, widened.
template <int P>
__device__ __forceinline__ double leaf_map_at(const double* __restrict__ lr, int n_u, int c,
                                              const double* v) {
#pragma clang fp contract(off)
    double d[P];
#pragma unroll
    for (int j = 0; j < P; ++j) d[j] = v[j] - lr[j];
    const double* Kc = lr + P + n_u;
    double w = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) w = w + Kc[c * P + j] * d[j];
    return lr[P + c] + w;
}

template <int P>
__device__ __forceinline__ double leaf_map_at(const float* __restrict__ lr, int n_u, int c,
                                              const double* v) {
#pragma clang fp contract(off)
    float xs[P], d[P];
#pragma unroll
    for (int j = 0; j < P; ++j) xs[j] = (float)v[j];
    leaf_offset32<P>(lr, xs, d);
    return leaf_input32<P>(lr, n_u, c, d);
}

// What both entry points refuse of the plant of the step, the plant part of an
// ehm_invariance_opts: the inputs, the modes, the box of at most max_d disturbances and its E.
inline int check_step_plant(ehm_err_channel& err, const ehm_invariance_opts* o, int n_u, int max_d,
                            const char* who) {
    if (n_u > EHM_R_MAX_NU)
        return err.fail(EHM_E_INVALID, "%s: n_u = %d, at most %d inputs", who, n_u,
                        EHM_R_MAX_NU);
    if (o->n_modes < 1 || o->n_modes > EHM_R_MAX_MODES)
        return err.fail(EHM_E_INVALID, "%s: %d modes (1..%d)", who, (int)o->n_modes,
                        EHM_R_MAX_MODES);
    if (o->n_d < 0 || o->n_d > max_d)
        return err.fail(EHM_E_INVALID, "%s: n_d = %d (0..%d)", who, (int)o->n_d, max_d);
    if (o->n_d > 0 && !o->E)
        return err.fail(EHM_E_INVALID, "%s: a box of %d disturbances but no E", who, (int)o->n_d);
    if (o->n_d > 0 && (!o->d_lo || !o->d_hi))
        return err.fail(EHM_E_INVALID, "%s: a required array is NULL", who);
    for (int b = 0; b < o->n_d; ++b)
        if (!std::isfinite(o->d_lo[b]) || !std::isfinite(o->d_hi[b]) || o->d_lo[b] > o->d_hi[b])
            return err.fail(EHM_E_INVALID, "%s: the box is [%g, %g] on axis %d", who, o->d_lo[b],
                            o->d_hi[b], b);
    return EHM_OK;
}

// The generators of the robust step: per mode G_m = [E | -A_m | B_m | I] [p][n_g]
// and the box [d; v; e; v] stacked in that order; the v columns (both blocks) and the e columns are
// there only where the caller gives the box.  Every entry is a copy or a negation, so G is exact.
// `o` has passed check_step_plant.  Refused: a v or e box of which one bound is NULL, one without 0
// (v_0 = 0, and e = 0 where u = 0, are draws too), n_g > max_g.
struct RobustGen {
    std::vector<double> G, lo, hi;
    int n_g = 0;
};

inline int robust_generators(ehm_err_channel& err, const ehm_invariance_opts* o,
                             const ehm_robust_opts* ro, int p, int n_u, int max_g, const char* who,
                             RobustGen& g) {
    if ((!ro->v_lo) != (!ro->v_hi) || (!ro->e_lo) != (!ro->e_hi))
        return err.fail(EHM_E_INVALID, "%s: a box with one bound NULL", who);
    const int n_d = o->n_d, n_v = ro->v_lo ? p : 0, n_e = ro->e_lo ? n_u : 0;
    g.n_g = n_d + 2 * n_v + n_e;
    if (g.n_g > max_g)
        return err.fail(EHM_E_INVALID, "%s: n_g = %d generators (n_d + 2 p + n_u), at most %d", who,
                        g.n_g, max_g);
    for (int c = 0; c < n_v; ++c)
        if (!(ro->v_lo[c] <= 0.0 && ro->v_hi[c] >= 0.0))
            return err.fail(EHM_E_INVALID, "%s: the v box [%g, %g] on axis %d does not hold 0", who,
                            ro->v_lo[c], ro->v_hi[c], c);
    for (int c = 0; c < n_e; ++c)
        if (!(ro->e_lo[c] <= 0.0 && ro->e_hi[c] >= 0.0))
            return err.fail(EHM_E_INVALID, "%s: the e box [%g, %g] on axis %d does not hold 0", who,
                            ro->e_lo[c], ro->e_hi[c], c);
    const int n_g = g.n_g;
    g.G.assign((size_t)o->n_modes * p * n_g, 0.0);
    for (int m = 0; m < o->n_modes; ++m)
        for (int k = 0; k < p; ++k) {
            double* row = &g.G[((size_t)m * p + k) * n_g];
            for (int b = 0; b < n_d; ++b) row[b] = o->E[k * n_d + b];
            for (int c = 0; c < n_v; ++c) row[n_d + c] = -o->A[((size_t)m * p + k) * p + c];
            for (int c = 0; c < n_e; ++c) row[n_d + n_v + c] = o->B[((size_t)m * p + k) * n_u + c];
            if (n_v) row[n_d + n_v + n_e + k] = 1.0;
        }
    g.lo.clear();
    g.hi.clear();
    g.lo.insert(g.lo.end(), o->d_lo, o->d_lo + n_d);
    g.hi.insert(g.hi.end(), o->d_hi, o->d_hi + n_d);
    for (int rep = 0; rep < 2; ++rep) {
        g.lo.insert(g.lo.end(), ro->v_lo, ro->v_lo + n_v);
        g.hi.insert(g.hi.end(), ro->v_hi, ro->v_hi + n_v);
        if (rep == 0) {
            g.lo.insert(g.lo.end(), ro->e_lo, ro->e_lo + n_e);
            g.hi.insert(g.hi.end(), ro->e_hi, ro->e_hi + n_e);
        }
    }
    for (int k = 0; k < n_g; ++k)
        if (!std::isfinite(g.lo[k]) || !std::isfinite(g.hi[k]) || g.lo[k] > g.hi[k])
            return err.fail(EHM_E_INVALID, "%s: the box is [%g, %g] on generator %d", who, g.lo[k],
                            g.hi[k], k);
    return EHM_OK;
}

// That plant's doubles into pk: A, B, w and E at pl's offsets, the box after them at o_lo, o_hi.
// e_modes: the blocks [p][n_d] that E holds (1: the shared E; n_modes: the generators of every mode).
inline void pack_step_plant(Pack& pk, DevPlant& pl, const ehm_invariance_opts* o, int p, int n_u,
                            int& o_lo, int& o_hi, int e_modes = 1) {
    pl.n_modes = o->n_modes;
    pl.n_d = o->n_d;
    pl.oA = pk.put(o->A, (size_t)o->n_modes * p * p);
    pl.oB = pk.put(o->B, (size_t)o->n_modes * p * n_u);
    pl.ow = pk.put(o->w, (size_t)o->n_modes * p);
    pl.oE = pk.put(o->E, (size_t)e_modes * p * o->n_d);
    o_lo = pk.put(o->d_lo, (size_t)o->n_d);
    o_hi = pk.put(o->d_hi, (size_t)o->n_d);
}

// The volumes of the cells a chunk's positions `has` hold (cells [..][(p+1) p] by position):
// vol[a] is that of position has[a].  ehm_volume_batch may leave another device current, so the
// caller's is set again.
inline int cell_volumes(ehm_err_channel& err, const char* who, int device, int p,
                        const double* cells, const std::vector<long long>& has,
                        std::vector<double>& vol) {
    const size_t cell = (size_t)(p + 1) * p;
    vol.resize(has.size());
    if (has.empty()) return EHM_OK;
    std::vector<double> packed(has.size() * cell);
    for (size_t a = 0; a < has.size(); ++a)
        std::memcpy(&packed[a * cell], cells + (size_t)has[a] * cell, cell * sizeof(double));
    const int rc = ehm_volume_batch(device, (int64_t)has.size(), p, packed.data(), vol.data());
    if (rc) return err.fail(rc, "%s: ehm_volume_batch: %s", who, ehm_last_error());
    EHM_HIP_TRY(err, hipSetDevice(device));
    return EHM_OK;
}

}  // namespace
