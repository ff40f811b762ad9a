// Merging the leaves of a compiled law that apply one affine map.  The
// partition is split by what the optimal cost does; where the first input is one affine function
// on both sides of a split, every leaf below carries the same u = u_0 + K (x - v_0) up to solver
// noise.  An internal record is MERGEABLE iff every leaf below it has a cell, the leaf mode of the
// record's representative (its leftmost leaf) and, at each vertex of its OWN cell, an input within
// tol of the representative's map there; the topmost mergeable records become leaves that take
// their representative's record.  Both maps are affine, so the reduced law is within tol of the
// original at every state of every original cell, and the bound does not grow with the levels.
//
//   make_parents       the parent table, as ehm_compiled_cells builds it (ehm_cells_dev.h)
//   k_reduce_forest    one thread per internal record and per root: the table names it as the parent
//                      of what it names (else the records form no forest and the law is refused)
//   k_reduce_rep       one thread per leaf: up while it hangs on the left side, itself as `rep`
//   k_reduce_flags     the hot kernel, one thread per leaf, templated on the law's scalar and on P:
//                      the cell in registers (leaf_cell), the leaf's own map at its vertices, then
//                      up the parent table once per input: rep's map at the same vertices,
//                      open[a] = 1 where !(|u_rep - u_l| <= tol); plain byte stores, every writer
//                      writes the same value; the largest accepted deviation per workgroup
//   k_reduce_max       the largest of the workgroups' deviations
//   k_reduce_survive   one thread per record: the internal records and leaves that survive, the
//                      leaf that stands for every leaf
//   k_reduce_scan      order-preserving compaction: exclusive sums of the survivors (blocks of 1024,
//   k_reduce_scan_add  the block sums scanned the same way), so children still follow their parents
//                      (ehm_scan_dev.h)
//   k_reduce_rewrite   renumbers children and root entries, gathers the leaf records, leaf_node and
//                      leaf_mode, and writes the new leaf of every original leaf
//
// The differences are taken in double under fp contract(off) in a fixed order
// (tests/reduce_cpu.py is the numpy mirror); the rules are ehm_reduce_host.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_reduce_host.h"
#include "ehm_scan_dev.h"

#define EHM_RED_BLOCK 64            // k_reduce_flags: the cell of P = 8 takes 144 registers

namespace {

using ehm_cert::Parents;

template <class T>
__global__ void k_reduce_forest(long long n_int, long long n_roots, int p, int node_stride,
                                const T* __restrict__ node,
                                const int32_t* __restrict__ root_entry, Parents P,
                                int32_t* __restrict__ bad) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = true;
    if (q < n_int) {
        int32_t left, right;
        ehm_cert::children_of(node + (size_t)q * node_stride, p, left, right);
        ok = ehm_red::names_its_children(P, (int32_t)q, left, right);
    } else if (q < n_int + n_roots) {
        const int32_t r = (int32_t)(q - n_int);
        ok = ehm_red::root_names_entry(P, r, root_entry[r]);
    }
    if (!ok) *bad = 1;
}

__global__ void k_reduce_rep(long long n_leaf, Parents P, int32_t* __restrict__ rep) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_leaf) return;
    ehm_red::mark_representative(P, (int32_t)l, rep);
}

template <class T>
struct FlagArgs {
    long long n_leaf;
    const T* node;
    const T* leaf_rec;
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    Parents par;
    const int32_t* rep;             // [n_int]
    const int32_t* leaf_mode;       // [n_leaf] or nullptr
    const double* tol;              // [n_u]
    int n_u, leaf_stride;
    uint8_t* open;                  // [n_int], zero on entry
    double* blk_dev;                // [blocks]
};

template <class T, int P>
__global__ __launch_bounds__(EHM_RED_BLOCK) void k_reduce_flags(FlagArgs<T> A) {
#pragma clang fp contract(off)
    __shared__ double sdev[EHM_RED_BLOCK];
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double dev = 0.0;
    if (q < A.n_leaf) {
        const int32_t l = (int32_t)q;
        double V[(P + 1) * P];
        const bool ok = leaf_cell<T, P>(A.par, A.node, A.root_entry, A.root_vertices, l, V);
        if (!ok) {
            // no cell: nothing above this leaf merges
            for (int32_t a = A.par.leaf[l]; a >= 0; a = A.par.node[a]) A.open[a] = 1;
        } else {
            if (A.leaf_mode) {
                const int32_t m = A.leaf_mode[l];
                for (int32_t a = A.par.leaf[l]; a >= 0; a = A.par.node[a]) {
                    const int32_t r = A.rep[a];
                    if (r < 0 || A.leaf_mode[r] != m) A.open[a] = 1;
                }
            }
            const T* lr = A.leaf_rec + (size_t)l * A.leaf_stride;
            for (int c = 0; c < A.n_u; ++c) {
                const double tol = A.tol[c];
                double w[P + 1];
#pragma unroll
                for (int i = 0; i <= P; ++i) w[i] = leaf_map_at<P>(lr, A.n_u, c, &V[i * P]);
                for (int32_t a = A.par.leaf[l]; a >= 0; a = A.par.node[a]) {
                    const int32_t r = A.rep[a];
                    if (r < 0) {
                        A.open[a] = 1;
                        continue;
                    }
                    const T* rr = A.leaf_rec + (size_t)r * A.leaf_stride;
                    bool pass = true;
#pragma unroll
                    for (int i = 0; i <= P; ++i) {
                        const double diff = fabs(leaf_map_at<P>(rr, A.n_u, c, &V[i * P]) - w[i]);
                        if (diff <= tol) dev = fmax(dev, diff);
                        else pass = false;          // a NaN difference too
                    }
                    if (!pass) A.open[a] = 1;
                }
            }
        }
    }
    sdev[threadIdx.x] = dev;
    __syncthreads();
    for (int h = EHM_RED_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sdev[threadIdx.x] = fmax(sdev[threadIdx.x], sdev[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) A.blk_dev[blockIdx.x] = sdev[0];
}

__global__ __launch_bounds__(256) void k_reduce_max(long long n, const double* __restrict__ in,
                                                    double* __restrict__ out) {
    __shared__ double sh[256];
    double m = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) m = fmax(m, in[i]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

__global__ void k_reduce_survive(long long n_int, long long n_leaf, Parents P,
                                 const uint8_t* __restrict__ open,
                                 const int32_t* __restrict__ rep, int32_t* __restrict__ keep_int,
                                 int32_t* __restrict__ keep_leaf, int32_t* __restrict__ target) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n_int) {
        keep_int[q] = ehm_red::internal_survives(P, (int32_t)q, open) ? 1 : 0;
    } else if (q < n_int + n_leaf) {
        const int32_t l = (int32_t)(q - n_int);
        const int32_t t = ehm_red::leaf_target(P, l, open, rep);
        target[l] = t;
        keep_leaf[l] = t == l ? 1 : 0;
    }
}

template <class T>
struct RewriteArgs {
    long long n_int, n_leaf, n_roots;
    int p, node_stride, leaf_stride;
    const T* node;
    const T* leaf_rec;
    const int32_t* leaf_node;
    const int32_t* leaf_mode;       // or nullptr
    const int32_t* root_entry;
    const uint8_t* open;
    const int32_t* rep;
    const int32_t* keep_int;
    const int32_t* keep_leaf;
    const int32_t* new_int;
    const int32_t* new_leaf;
    const int32_t* target;
    T* node_out;
    T* leaf_out;
    int32_t* leaf_node_out;
    int32_t* leaf_mode_out;         // or nullptr
    int32_t* root_entry_out;
    int32_t* leaf_of;               // [n_leaf]
};

template <class T>
__global__ void k_reduce_rewrite(RewriteArgs<T> A) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < A.n_int) {
        if (!A.keep_int[q]) return;
        const T* src = A.node + (size_t)q * A.node_stride;
        T* dst = A.node_out + (size_t)A.new_int[q] * A.node_stride;
        for (int e = 0; e < A.node_stride; ++e) dst[e] = src[e];
        int32_t ch[2];
        ehm_cert::children_of(src, A.p, ch[0], ch[1]);
        for (int s = 0; s < 2; ++s)
            ch[s] = ehm_red::renumber(ch[s], A.open, A.rep, A.new_int, A.new_leaf);
        __builtin_memcpy(dst + A.p + 1, ch, sizeof ch);
    } else if (q < A.n_int + A.n_leaf) {
        const long long l = q - A.n_int;
        A.leaf_of[l] = A.new_leaf[A.target[l]];
        if (!A.keep_leaf[l]) return;
        const int32_t at = A.new_leaf[l];
        const T* src = A.leaf_rec + (size_t)l * A.leaf_stride;
        T* dst = A.leaf_out + (size_t)at * A.leaf_stride;
        for (int e = 0; e < A.leaf_stride; ++e) dst[e] = src[e];
        A.leaf_node_out[at] = A.leaf_node[l];
        if (A.leaf_mode_out) A.leaf_mode_out[at] = A.leaf_mode[l];
    } else if (q < A.n_int + A.n_leaf + A.n_roots) {
        const long long r = q - A.n_int - A.n_leaf;
        A.root_entry_out[r] =
            ehm_red::renumber(A.root_entry[r], A.open, A.rep, A.new_int, A.new_leaf);
    }
}

typedef void (*flags64_fn)(FlagArgs<double>);
typedef void (*flags32_fn)(FlagArgs<float>);
#define EHM_RED_ALL(T) {&k_reduce_flags<T, 1>, &k_reduce_flags<T, 2>, &k_reduce_flags<T, 3>, \
                        &k_reduce_flags<T, 4>, &k_reduce_flags<T, 5>, &k_reduce_flags<T, 6>, \
                        &k_reduce_flags<T, 7>, &k_reduce_flags<T, 8>}
const flags64_fn k_flags64[EHM_CP] = EHM_RED_ALL(double);
const flags32_fn k_flags32[EHM_CP] = EHM_RED_ALL(float);
#undef EHM_RED_ALL

thread_local ehm_err_channel r_err;

template <class T>
int reduce_law(ehm_compiled* law, const ehm_compiled_view& v, hipStream_t stream,
               const double* root_vertices, const double* tol, const int32_t* leaf_mode,
               ehm_compiled** out, int32_t* leaf_mode_out, int32_t* leaf_of, int64_t* counts,
               double* max_deviation) {
    const int p = v.p, n_u = v.n_u;
    const long long n_int = v.n_int, n_leaf = v.n_leaf, n_roots = v.n_roots;
    const T* node = static_cast<const T*>(v.node);
    const T* leaf_rec = static_cast<const T*>(v.leaf_rec);
    const int32_t* leaf_node = v.leaf_node;
    ParentTable tab;
    EHM_HIP_TRY(r_err, make_parents(v, stream, tab));
    const Parents par = tab.view();
    DevBuf d_bad, d_rep, d_open, d_roots, d_tol, d_mode, d_blk, d_dev;
    EHM_HIP_TRY(r_err, d_bad.alloc(sizeof(int32_t)));
    EHM_HIP_TRY(r_err, hipMemsetAsync(d_bad.ptr, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_reduce_forest<T>, dim3(blocks_of(n_int + n_roots, 256)), dim3(256),
                       0, stream, n_int, n_roots, p, v.node_stride, node, v.root_entry, par,
                       d_bad.as<int32_t>());
    EHM_HIP_TRY(r_err, hipGetLastError());
    int32_t bad = 0;
    EHM_HIP_TRY(r_err, hipMemcpyAsync(&bad, d_bad.ptr, sizeof bad, hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(r_err, hipStreamSynchronize(stream));
    if (bad)
        return r_err.fail(EHM_E_INVALID, "reduce: the law's records form no forest (a record is "
                          "named by two parents or roots)");
    EHM_HIP_TRY(r_err, d_rep.alloc((size_t)n_int * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, d_open.alloc((size_t)n_int));
    if (n_int) {
        EHM_HIP_TRY(r_err, hipMemsetD32Async((hipDeviceptr_t)d_rep.ptr, -1, (size_t)n_int, stream));
        EHM_HIP_TRY(r_err, hipMemsetAsync(d_open.ptr, 0, (size_t)n_int, stream));
    }
    hipLaunchKernelGGL(k_reduce_rep, dim3(blocks_of(n_leaf, 256)), dim3(256), 0, stream,
                       n_leaf, par, d_rep.as<int32_t>());
    EHM_HIP_TRY(r_err, hipGetLastError());
    // the flags
    const size_t cell = (size_t)(p + 1) * p;
    EHM_HIP_TRY(r_err, d_roots.upload(root_vertices, (size_t)n_roots * cell * sizeof(double)));
    EHM_HIP_TRY(r_err, d_tol.upload(tol, (size_t)n_u * sizeof(double)));
    if (leaf_mode) EHM_HIP_TRY(r_err, d_mode.upload(leaf_mode, (size_t)n_leaf * sizeof(int32_t)));
    const unsigned nblk = blocks_of(n_leaf, EHM_RED_BLOCK);
    EHM_HIP_TRY(r_err, d_blk.alloc((size_t)nblk * sizeof(double)));
    EHM_HIP_TRY(r_err, d_dev.alloc(sizeof(double)));
    FlagArgs<T> F{n_leaf, node, leaf_rec, v.root_entry, d_roots.as<const double>(), par,
                  d_rep.as<const int32_t>(), leaf_mode ? d_mode.as<const int32_t>() : nullptr,
                  d_tol.as<const double>(), n_u, v.leaf_stride, d_open.as<uint8_t>(),
                  d_blk.as<double>()};
    if constexpr (std::is_same<T, float>::value)
        hipLaunchKernelGGL(k_flags32[p - 1], dim3(nblk), dim3(EHM_RED_BLOCK), 0, stream, F);
    else
        hipLaunchKernelGGL(k_flags64[p - 1], dim3(nblk), dim3(EHM_RED_BLOCK), 0, stream, F);
    EHM_HIP_TRY(r_err, hipGetLastError());
    hipLaunchKernelGGL(k_reduce_max, dim3(1), dim3(256), 0, stream, (long long)nblk,
                       d_blk.as<const double>(), d_dev.as<double>());
    EHM_HIP_TRY(r_err, hipGetLastError());
    // survivors and their new places; element n of each scan is the number of survivors
    DevBuf d_keep_int, d_keep_leaf, d_new_int, d_new_leaf, d_target;
    EHM_HIP_TRY(r_err, d_keep_int.alloc((size_t)(n_int + 1) * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, d_keep_leaf.alloc((size_t)(n_leaf + 1) * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, d_new_int.alloc((size_t)(n_int + 1) * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, d_new_leaf.alloc((size_t)(n_leaf + 1) * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, d_target.alloc((size_t)n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, hipMemsetAsync(d_keep_int.ptr, 0, (size_t)(n_int + 1) * sizeof(int32_t),
                                      stream));
    EHM_HIP_TRY(r_err, hipMemsetAsync(d_keep_leaf.ptr, 0, (size_t)(n_leaf + 1) * sizeof(int32_t),
                                      stream));
    hipLaunchKernelGGL(k_reduce_survive, dim3(blocks_of(n_int + n_leaf, 256)), dim3(256), 0,
                       stream, n_int, n_leaf, par, d_open.as<const uint8_t>(),
                       d_rep.as<const int32_t>(), d_keep_int.as<int32_t>(),
                       d_keep_leaf.as<int32_t>(), d_target.as<int32_t>());
    EHM_HIP_TRY(r_err, hipGetLastError());
    int rc = exclusive_scan(r_err, stream, d_keep_int.as<const int32_t>(), d_new_int.as<int32_t>(),
                            n_int + 1);
    if (rc) return rc;
    rc = exclusive_scan(r_err, stream, d_keep_leaf.as<const int32_t>(), d_new_leaf.as<int32_t>(),
                        n_leaf + 1);
    if (rc) return rc;
    int32_t m_int = 0, m_leaf = 0;
    EHM_HIP_TRY(r_err, hipMemcpyAsync(&m_int, d_new_int.as<int32_t>() + n_int, sizeof m_int,
                                      hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(r_err, hipMemcpyAsync(&m_leaf, d_new_leaf.as<int32_t>() + n_leaf, sizeof m_leaf,
                                      hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(r_err, hipMemcpyAsync(max_deviation, d_dev.ptr, sizeof(double),
                                      hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(r_err, hipStreamSynchronize(stream));
    if (m_int < 0 || m_int > n_int || m_leaf < 1 || m_leaf > n_leaf)
        return r_err.fail(EHM_E_NUMERIC, "reduce: %d of %lld internal records and %d of %lld "
                          "leaves survive", (int)m_int, n_int, (int)m_leaf, n_leaf);
    // the new arrays
    DevBuf node_out, leaf_out, leaf_node_out, mode_out, entry_out, d_leaf_of;
    EHM_HIP_TRY(r_err, node_out.alloc((size_t)m_int * v.node_stride * sizeof(T)));
    EHM_HIP_TRY(r_err, leaf_out.alloc((size_t)m_leaf * v.leaf_stride * sizeof(T)));
    EHM_HIP_TRY(r_err, leaf_node_out.alloc((size_t)m_leaf * sizeof(int32_t)));
    if (leaf_mode) EHM_HIP_TRY(r_err, mode_out.alloc((size_t)m_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, entry_out.alloc((size_t)n_roots * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, d_leaf_of.alloc((size_t)n_leaf * sizeof(int32_t)));
    RewriteArgs<T> W{n_int, n_leaf, n_roots, p, v.node_stride, v.leaf_stride, node, leaf_rec,
                     leaf_node, leaf_mode ? d_mode.as<const int32_t>() : nullptr, v.root_entry,
                     d_open.as<const uint8_t>(), d_rep.as<const int32_t>(),
                     d_keep_int.as<const int32_t>(), d_keep_leaf.as<const int32_t>(),
                     d_new_int.as<const int32_t>(), d_new_leaf.as<const int32_t>(),
                     d_target.as<const int32_t>(), node_out.as<T>(), leaf_out.as<T>(),
                     leaf_node_out.as<int32_t>(), leaf_mode ? mode_out.as<int32_t>() : nullptr,
                     entry_out.as<int32_t>(), d_leaf_of.as<int32_t>()};
    hipLaunchKernelGGL(k_reduce_rewrite<T>, dim3(blocks_of(n_int + n_leaf + n_roots, 256)),
                       dim3(256), 0, stream, W);
    EHM_HIP_TRY(r_err, hipGetLastError());
    if (leaf_of)
        EHM_HIP_TRY(r_err, hipMemcpyAsync(leaf_of, d_leaf_of.ptr, (size_t)n_leaf * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
    if (leaf_mode && leaf_mode_out)
        EHM_HIP_TRY(r_err, hipMemcpyAsync(leaf_mode_out, mode_out.ptr,
                                          (size_t)m_leaf * sizeof(int32_t), hipMemcpyDeviceToHost,
                                          stream));
    EHM_HIP_TRY(r_err, hipStreamSynchronize(stream));
    counts[0] = n_leaf;
    counts[1] = m_leaf;
    counts[2] = n_int;
    counts[3] = m_int;
    rc = ehm_compiled_adopt(law, m_int, m_leaf, node_out, leaf_out, leaf_node_out, entry_out, out);
    if (rc) return r_err.fail(rc, "reduce: the reduced law is refused: %s",
                              ehm_compiled_last_error());
    return EHM_OK;
}

}  // namespace

extern "C" {

const char* ehm_reduce_last_error(void) { return r_err.c_str(); }

int ehm_compiled_reduce(ehm_compiled* law, const double* root_vertices, const double* tol,
                        const int32_t* leaf_mode, ehm_compiled** out, int32_t* leaf_mode_out,
                        int32_t* leaf_of, int64_t* counts, double* stats) {
    if (out) *out = nullptr;
    if (!law || !root_vertices || !tol || !out || !counts || !stats)
        return r_err.fail(EHM_E_INVALID, "reduce: bad argument");
    const auto t0 = std::chrono::steady_clock::now();
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    if (const int rc = check_law_shape(r_err, v, "reduce")) return rc;
    for (int c = 0; c < v.n_u; ++c)
        if (!(tol[c] >= 0.0) || !std::isfinite(tol[c]))
            return r_err.fail(EHM_E_INVALID, "reduce: tol[%d] = %g (a finite number >= 0)", c,
                              tol[c]);
    EHM_HIP_TRY(r_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(r_err, stream.create());
    // the law's arrays were written on its own stream (create) or by blocking copies (import)
    EHM_HIP_TRY(r_err, hipStreamSynchronize(v.stream));
    stats[0] = 0.0;
    const int rc = v.single
        ? reduce_law<float>(law, v, stream, root_vertices, tol, leaf_mode, out, leaf_mode_out,
                            leaf_of, counts, &stats[0])
        : reduce_law<double>(law, v, stream, root_vertices, tol, leaf_mode, out, leaf_mode_out,
                             leaf_of, counts, &stats[0]);
    stats[1] = wall_since(t0);
    return rc;
}

}  // extern "C"
