// Splitting the leaves of a compiled law, the inverse of ehm_reduce.hip.
// A leaf carries u = u_0 + K (x - v_0), anchored: when a leaf's cell is bisected as the partitioner
// would have bisected it and both children keep the parent's record verbatim, the refined law applies
// the same input, bit for bit, at every state.  Only the cells get smaller, and with them every
// statement the project makes leaf by leaf.
//
// A level is one pass over the current leaves:
//   make_parents       the parent table of the current arrays (ehm_cells_dev.h)
//   k_refine_plan      the hot kernel, one thread per leaf, templated on the law's scalar and on P:
//                      the cell in registers (leaf_cell), the first longest edge (i, j) in the
//                      partition engine's arithmetic, the criteria, the plane with s(v_j) = +1,
//                      s(v_i) = -1, s = 0 at the other vertices by a P x P solve in double, rounded
//                      to the law's scalar, the acceptance test (bisected_edge on the stored plane:
//                      what leaf_cell will apply to the children) and the residual, the largest
//                      per workgroup
//   k_refine_max       the largest residual so far
//   k_reduce_scan ..   the exclusive sums of the split flags (ehm_scan_dev.h)
//   k_refine_rewrite   copies the records; the left child keeps the leaf's index l, the right child
//                      is leaf n_leaf + offset[l], the plane is internal record n_int + offset[l] (so
//                      children still come after their parents), and the one reference that named ~l
//                      is re-pointed through the parent table
// until a pass splits nothing.  The arrays stay on the device between the passes; the import check
// of ehm_compiled_adopt runs once, on the final arrays.  The solve is in double under
// fp contract(off) in the fixed order of ehm_refine_host.h (tests/refine_cpu.py is the numpy mirror).
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
#include "ehm_refine_host.h"
#include "ehm_scan_dev.h"

#define EHM_REF_BLOCK 64            // k_refine_plan: one wavefront
#ifndef EHM_REF_STASH_P
#define EHM_REF_STASH_P 6
#endif

static_assert(EHM_REF_MAX_LEVELS == EHM_REFINE_MAX_LEVELS, "ehm_refine_host.h and ehmpc.h");
static_assert(ehm_ref::STOP_UNSELECTED == EHM_REFINE_UNSELECTED &&
              ehm_ref::STOP_SATISFIED == EHM_REFINE_SATISFIED &&
              ehm_ref::STOP_LEVELS == EHM_REFINE_LEVELS &&
              ehm_ref::STOP_NO_CELL == EHM_REFINE_NO_CELL &&
              ehm_ref::STOP_UNSEPARATED == EHM_REFINE_UNSEPARATED &&
              ehm_ref::STOP_TOO_DEEP == EHM_REFINE_TOO_DEEP &&
              ehm_ref::STOP_CODES == EHM_REFINE_STOPS, "ehm_refine_host.h and ehmpc.h");
static_assert(EHM_CERT_MAX_DEPTH == EHM_CELL_MAX_DEPTH, "ehm_certify_host.h and ehmpc.h");

namespace {

using ehm_cert::Parents;

template <class T>
struct PlanArgs {
    long long n_leaf;
    const T* node;
    const T* leaf_rec;
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    Parents par;
    const int32_t* rem;             // [n_leaf] levels remaining
    const double* max_spread;       // [n_u] or nullptr
    double max_diameter;            // read only with has_diameter
    int has_diameter;
    int n_u, leaf_stride;
    int8_t* stop;                   // [n_leaf]: PENDING on entry where the leaf is still open
    int32_t* split;                 // [n_leaf + 1]
    T* plane;                       // [n_leaf][P+1], written where split
    double* blk_res;                // [blocks]
};

template <class T, int P>
__global__ __launch_bounds__(EHM_REF_BLOCK) void k_refine_plan(PlanArgs<T> A) {
#pragma clang fp contract(off)
    // From P = EHM_REF_STASH_P on the cell waits in LDS while the solve runs (one column per thread,
    // nothing shared): the cell and the matrix together do not fit the register file.
    constexpr bool STASH = P >= EHM_REF_STASH_P;
    __shared__ double sres[EHM_REF_BLOCK];
    __shared__ double scell[STASH ? (P + 1) * P : 1][EHM_REF_BLOCK];
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double res = 0.0;
    if (q < A.n_leaf && A.stop[q] == ehm_ref::STOP_PENDING) {
        const int32_t l = (int32_t)q;
        double V[(P + 1) * P];
        int code = ehm_ref::STOP_NO_CELL;
        int split = 0;
        if (leaf_cell<T, P>(A.par, A.node, A.root_entry, A.root_vertices, l, V)) {
            int i, j;
            const double len = ehm_ref::longest_edge_of<P>(V, i, j);
            const int rem = A.rem[l];
            bool want = rem > 0;
            code = ehm_ref::STOP_SATISFIED;
            if (A.has_diameter || A.max_spread) {
                bool over = A.has_diameter && ehm_ref::exceeds(len, A.max_diameter);
                if (A.max_spread) {
                    const T* lr = A.leaf_rec + (size_t)l * A.leaf_stride;
                    for (int c = 0; c < A.n_u; ++c) {
                        double w[P + 1];
#pragma unroll
                        for (int k = 0; k <= P; ++k)
                            w[k] = leaf_map_at<P>(lr, A.n_u, c, &V[k * P]);
                        over = over || ehm_ref::exceeds(ehm_ref::spread_of<P + 1>(w),
                                                        A.max_spread[c]);
                    }
                }
                code = over ? ehm_ref::STOP_LEVELS : ehm_ref::STOP_SATISFIED;
                want = want && over;
            }
            if (want) {
                if (ehm_ref::depth_of(A.par, l) >= EHM_CERT_MAX_DEPTH) {
                    code = ehm_ref::STOP_TOO_DEEP;
                } else {
                    double a[P], b;
                    if constexpr (STASH) {
#pragma unroll
                        for (int e = 0; e < (P + 1) * P; ++e) scell[e][threadIdx.x] = V[e];
                    }
                    ehm_ref::solve_plane<P>(V, i, j, a, b);
                    if constexpr (STASH) {
                        asm volatile("" ::: "memory");      // the loads are not the stored values
#pragma unroll
                        for (int e = 0; e < (P + 1) * P; ++e) V[e] = scell[e][threadIdx.x];
                    }
                    T rec[P + 1];
                    double r = 0.0;
                    if (ehm_ref::store_plane<T, P>(a, b, rec) &&
                        ehm_ref::accept_plane<T, P>(V, rec, i, j, r)) {
                        split = 1;
                        res = r;
                        code = ehm_ref::STOP_PENDING;   // its children are open
                        T* out = A.plane + (size_t)l * (P + 1);
#pragma unroll
                        for (int c = 0; c <= P; ++c) out[c] = rec[c];
                    } else {
                        code = ehm_ref::STOP_UNSEPARATED;
                    }
                }
            }
        }
        A.stop[l] = (int8_t)code;
        A.split[l] = split;
    }
    sres[threadIdx.x] = res;
    __syncthreads();
    for (int h = EHM_REF_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sres[threadIdx.x] = fmax(sres[threadIdx.x], sres[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) A.blk_res[blockIdx.x] = sres[0];
}

// *out = max(*out, in[0 .. n - 1])
__global__ __launch_bounds__(256) void k_refine_max(long long n, const double* __restrict__ in,
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
    if (threadIdx.x == 0) *out = fmax(*out, sh[0]);
}

// the arrays of a law between the passes, with what a pass carries per leaf
struct Work {
    DevBuf node, leaf_rec, leaf_node, leaf_mode, root_entry, rem, stop, origin;
    long long n_int = 0, n_leaf = 0;
};

template <class T>
struct RewriteArgs {
    long long n_int, n_leaf, n_roots;
    int p, node_stride, leaf_stride;
    const T* node;
    const T* leaf_rec;
    const int32_t* leaf_node;
    const int32_t* leaf_mode;       // or nullptr
    const int32_t* root_entry;
    const int32_t* rem;
    const int8_t* stop;
    const int32_t* origin;
    Parents par;
    const int32_t* split;
    const int32_t* offset;
    const T* plane;
    T* node_out;
    T* leaf_out;
    int32_t* leaf_node_out;
    int32_t* leaf_mode_out;         // or nullptr
    int32_t* root_entry_out;
    int32_t* rem_out;
    int8_t* stop_out;
    int32_t* origin_out;
};

template <class T>
__global__ void k_refine_rewrite(RewriteArgs<T> A) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < A.n_int) {
        const T* src = A.node + (size_t)q * A.node_stride;
        T* dst = A.node_out + (size_t)q * A.node_stride;
        for (int e = 0; e < A.node_stride; ++e) dst[e] = src[e];
        int32_t ch[2];
        ehm_cert::children_of(src, A.p, ch[0], ch[1]);
        for (int s = 0; s < 2; ++s)
            ch[s] = ehm_ref::repoint_child(A.par, (int32_t)q, s, ch[s], A.split, A.offset, A.n_int);
        __builtin_memcpy(dst + A.p + 1, ch, sizeof ch);
    } else if (q < A.n_int + A.n_leaf) {
        const long long l = q - A.n_int;
        const bool split = A.split[l] != 0;
        const long long twin = A.n_leaf + A.offset[l];
        const T* src = A.leaf_rec + (size_t)l * A.leaf_stride;
        for (int side = 0; side < (split ? 2 : 1); ++side) {
            const long long at = side ? twin : l;
            T* dst = A.leaf_out + (size_t)at * A.leaf_stride;
            for (int e = 0; e < A.leaf_stride; ++e) dst[e] = src[e];
            A.leaf_node_out[at] = A.leaf_node[l];
            if (A.leaf_mode_out) A.leaf_mode_out[at] = A.leaf_mode[l];
            A.origin_out[at] = A.origin[l];
            A.rem_out[at] = split ? A.rem[l] - 1 : A.rem[l];
            A.stop_out[at] = A.stop[l];         // PENDING where split
        }
        if (split) {
            T* dst = A.node_out + (size_t)(A.n_int + A.offset[l]) * A.node_stride;
            const T* pl = A.plane + (size_t)l * (A.p + 1);
            for (int e = 0; e < A.node_stride; ++e) dst[e] = e <= A.p ? pl[e] : (T)0;
            const int32_t ch[2] = {~(int32_t)l, ~(int32_t)twin};
            __builtin_memcpy(dst + A.p + 1, ch, sizeof ch);
        }
    } else if (q < A.n_int + A.n_leaf + A.n_roots) {
        const long long r = q - A.n_int - A.n_leaf;
        A.root_entry_out[r] = ehm_ref::repoint_entry(A.par, (int32_t)r, A.root_entry[r], A.split,
                                                     A.offset, A.n_int);
    }
}

typedef void (*plan64_fn)(PlanArgs<double>);
typedef void (*plan32_fn)(PlanArgs<float>);
#define EHM_REF_ALL(T) {&k_refine_plan<T, 1>, &k_refine_plan<T, 2>, &k_refine_plan<T, 3>, \
                        &k_refine_plan<T, 4>, &k_refine_plan<T, 5>, &k_refine_plan<T, 6>, \
                        &k_refine_plan<T, 7>, &k_refine_plan<T, 8>}
const plan64_fn k_plan64[EHM_CP] = EHM_REF_ALL(double);
const plan32_fn k_plan32[EHM_CP] = EHM_REF_ALL(float);
#undef EHM_REF_ALL

thread_local ehm_err_channel f_err;

struct RefineCall {
    const double* root_vertices;
    const int32_t* levels;
    const uint8_t* selected;
    const double* max_diameter;
    const double* max_spread;
    const int32_t* leaf_mode;
    int64_t worst;
    int32_t* leaf_mode_out;
    int32_t* origin;
    int8_t* stop;
    int64_t* counts;
    double* stats;
};

template <class T>
int refine_law(ehm_compiled* law, const ehm_compiled_view& v, hipStream_t stream,
               const RefineCall& c, ehm_compiled** out) {
    const int p = v.p, n_u = v.n_u;
    const long long n_roots = v.n_roots;
    const size_t ns = (size_t)v.node_stride * sizeof(T), ls = (size_t)v.leaf_stride * sizeof(T);
    // the working copy: the law's arrays, every leaf its own origin
    Work cur;
    cur.n_int = v.n_int;
    cur.n_leaf = v.n_leaf;
    EHM_HIP_TRY(f_err, cur.node.alloc((size_t)v.n_int * ns));
    EHM_HIP_TRY(f_err, cur.leaf_rec.alloc((size_t)v.n_leaf * ls));
    EHM_HIP_TRY(f_err, cur.leaf_node.alloc((size_t)v.n_leaf * sizeof(int32_t)));
    EHM_HIP_TRY(f_err, cur.root_entry.alloc((size_t)n_roots * sizeof(int32_t)));
    if (v.n_int)
        EHM_HIP_TRY(f_err, hipMemcpyAsync(cur.node.ptr, v.node, (size_t)v.n_int * ns,
                                          hipMemcpyDeviceToDevice, stream));
    EHM_HIP_TRY(f_err, hipMemcpyAsync(cur.leaf_rec.ptr, v.leaf_rec, (size_t)v.n_leaf * ls,
                                      hipMemcpyDeviceToDevice, stream));
    EHM_HIP_TRY(f_err, hipMemcpyAsync(cur.leaf_node.ptr, v.leaf_node,
                                      (size_t)v.n_leaf * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                      stream));
    EHM_HIP_TRY(f_err, hipMemcpyAsync(cur.root_entry.ptr, v.root_entry,
                                      (size_t)n_roots * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                      stream));
    EHM_HIP_TRY(f_err, hipStreamSynchronize(stream));
    {
        std::vector<int32_t> origin((size_t)v.n_leaf);
        std::vector<int8_t> stop((size_t)v.n_leaf);
        for (long long l = 0; l < v.n_leaf; ++l) {
            origin[(size_t)l] = (int32_t)l;
            stop[(size_t)l] = (!c.selected || c.selected[l]) ? ehm_ref::STOP_PENDING
                                                             : ehm_ref::STOP_UNSELECTED;
        }
        EHM_HIP_TRY(f_err, cur.origin.upload(origin.data(), origin.size() * sizeof(int32_t)));
        EHM_HIP_TRY(f_err, cur.stop.upload(stop.data(), stop.size()));
        EHM_HIP_TRY(f_err, cur.rem.upload(c.levels, (size_t)v.n_leaf * sizeof(int32_t)));
        if (c.leaf_mode)
            EHM_HIP_TRY(f_err, cur.leaf_mode.upload(c.leaf_mode,
                                                    (size_t)v.n_leaf * sizeof(int32_t)));
    }
    DevBuf d_roots, d_spread, d_res;
    const size_t cell = (size_t)(p + 1) * p;
    EHM_HIP_TRY(f_err, d_roots.upload(c.root_vertices, (size_t)n_roots * cell * sizeof(double)));
    if (c.max_spread)
        EHM_HIP_TRY(f_err, d_spread.upload(c.max_spread, (size_t)n_u * sizeof(double)));
    EHM_HIP_TRY(f_err, d_res.alloc(sizeof(double)));
    EHM_HIP_TRY(f_err, hipMemsetAsync(d_res.ptr, 0, sizeof(double), stream));
    long long passes = 0, n_split = 0;
    double plan_seconds = 0.0;
    for (;;) {
        const long long n_int = cur.n_int, n_leaf = cur.n_leaf;
        ehm_compiled_view w = v;
        w.node = cur.node.ptr;
        w.leaf_rec = cur.leaf_rec.ptr;
        w.leaf_node = cur.leaf_node.as<const int32_t>();
        w.root_entry = cur.root_entry.as<const int32_t>();
        w.n_int = n_int;
        w.n_leaf = n_leaf;
        ParentTable tab;
        EHM_HIP_TRY(f_err, make_parents(w, stream, tab));
        const Parents par = tab.view();
        DevBuf d_split, d_offset, d_plane, d_blk;
        EHM_HIP_TRY(f_err, d_split.alloc((size_t)(n_leaf + 1) * sizeof(int32_t)));
        EHM_HIP_TRY(f_err, d_offset.alloc((size_t)(n_leaf + 1) * sizeof(int32_t)));
        EHM_HIP_TRY(f_err, d_plane.alloc((size_t)n_leaf * (p + 1) * sizeof(T)));
        const unsigned nblk = blocks_of(n_leaf, EHM_REF_BLOCK);
        EHM_HIP_TRY(f_err, d_blk.alloc((size_t)nblk * sizeof(double)));
        EHM_HIP_TRY(f_err, hipMemsetAsync(d_split.ptr, 0, (size_t)(n_leaf + 1) * sizeof(int32_t),
                                          stream));
        PlanArgs<T> F{n_leaf, cur.node.as<const T>(), cur.leaf_rec.as<const T>(),
                      cur.root_entry.as<const int32_t>(), d_roots.as<const double>(), par,
                      cur.rem.as<const int32_t>(),
                      c.max_spread ? d_spread.as<const double>() : nullptr,
                      c.max_diameter ? *c.max_diameter : 0.0, c.max_diameter ? 1 : 0, n_u,
                      v.leaf_stride, cur.stop.as<int8_t>(), d_split.as<int32_t>(), d_plane.as<T>(),
                      d_blk.as<double>()};
        EventPair ev;
        EHM_HIP_TRY(f_err, hipEventRecord(ev.e0, stream));
        if constexpr (std::is_same<T, float>::value)
            hipLaunchKernelGGL(k_plan32[p - 1], dim3(nblk), dim3(EHM_REF_BLOCK), 0, stream, F);
        else
            hipLaunchKernelGGL(k_plan64[p - 1], dim3(nblk), dim3(EHM_REF_BLOCK), 0, stream, F);
        EHM_HIP_TRY(f_err, hipGetLastError());
        EHM_HIP_TRY(f_err, hipEventRecord(ev.e1, stream));
        hipLaunchKernelGGL(k_refine_max, dim3(1), dim3(256), 0, stream, (long long)nblk,
                           d_blk.as<const double>(), d_res.as<double>());
        EHM_HIP_TRY(f_err, hipGetLastError());
        // element n_leaf of the scan is the number of leaves this pass splits
        const int rc = exclusive_scan(f_err, stream, d_split.as<const int32_t>(),
                                      d_offset.as<int32_t>(), n_leaf + 1);
        if (rc) return rc;
        int32_t m = 0;
        EHM_HIP_TRY(f_err, hipMemcpyAsync(&m, d_offset.as<int32_t>() + n_leaf, sizeof m,
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(f_err, hipStreamSynchronize(stream));
        double secs = 0.0;
        ev.seconds(&secs);
        plan_seconds += secs;
        if (m < 0 || m > n_leaf || n_leaf + m > c.worst)
            return f_err.fail(EHM_E_NUMERIC, "refine: a pass splits %d of %lld leaves (at most "
                              "%lld leaves in all)", (int)m, n_leaf, (long long)c.worst);
        if (m == 0) break;
        Work nxt;
        nxt.n_int = n_int + m;
        nxt.n_leaf = n_leaf + m;
        EHM_HIP_TRY(f_err, nxt.node.alloc((size_t)nxt.n_int * ns));
        EHM_HIP_TRY(f_err, nxt.leaf_rec.alloc((size_t)nxt.n_leaf * ls));
        EHM_HIP_TRY(f_err, nxt.leaf_node.alloc((size_t)nxt.n_leaf * sizeof(int32_t)));
        if (c.leaf_mode)
            EHM_HIP_TRY(f_err, nxt.leaf_mode.alloc((size_t)nxt.n_leaf * sizeof(int32_t)));
        EHM_HIP_TRY(f_err, nxt.root_entry.alloc((size_t)n_roots * sizeof(int32_t)));
        EHM_HIP_TRY(f_err, nxt.rem.alloc((size_t)nxt.n_leaf * sizeof(int32_t)));
        EHM_HIP_TRY(f_err, nxt.stop.alloc((size_t)nxt.n_leaf));
        EHM_HIP_TRY(f_err, nxt.origin.alloc((size_t)nxt.n_leaf * sizeof(int32_t)));
        RewriteArgs<T> W{n_int, n_leaf, n_roots, p, v.node_stride, v.leaf_stride,
                         cur.node.as<const T>(), cur.leaf_rec.as<const T>(),
                         cur.leaf_node.as<const int32_t>(),
                         c.leaf_mode ? cur.leaf_mode.as<const int32_t>() : nullptr,
                         cur.root_entry.as<const int32_t>(), cur.rem.as<const int32_t>(),
                         cur.stop.as<const int8_t>(), cur.origin.as<const int32_t>(), par,
                         d_split.as<const int32_t>(), d_offset.as<const int32_t>(),
                         d_plane.as<const T>(), nxt.node.as<T>(), nxt.leaf_rec.as<T>(),
                         nxt.leaf_node.as<int32_t>(),
                         c.leaf_mode ? nxt.leaf_mode.as<int32_t>() : nullptr,
                         nxt.root_entry.as<int32_t>(), nxt.rem.as<int32_t>(),
                         nxt.stop.as<int8_t>(), nxt.origin.as<int32_t>()};
        hipLaunchKernelGGL(k_refine_rewrite<T>, dim3(blocks_of(n_int + n_leaf + n_roots, 256)),
                           dim3(256), 0, stream, W);
        EHM_HIP_TRY(f_err, hipGetLastError());
        // the buffers of this pass are freed when they go: hipFree waits for the work that uses them
        EHM_HIP_TRY(f_err, hipStreamSynchronize(stream));
        cur = std::move(nxt);
        ++passes;
        n_split += m;
    }
    // what the caller gets back
    const size_t n_out = (size_t)cur.n_leaf;
    std::vector<int8_t> stop(n_out);
    EHM_HIP_TRY(f_err, hipMemcpyAsync(stop.data(), cur.stop.ptr, n_out, hipMemcpyDeviceToHost,
                                      stream));
    if (c.origin)
        EHM_HIP_TRY(f_err, hipMemcpyAsync(c.origin, cur.origin.ptr, n_out * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
    if (c.leaf_mode && c.leaf_mode_out)
        EHM_HIP_TRY(f_err, hipMemcpyAsync(c.leaf_mode_out, cur.leaf_mode.ptr,
                                          n_out * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(f_err, hipMemcpyAsync(&c.stats[0], d_res.ptr, sizeof(double),
                                      hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(f_err, hipStreamSynchronize(stream));
    c.counts[0] = v.n_leaf;
    c.counts[1] = cur.n_leaf;
    c.counts[2] = v.n_int;
    c.counts[3] = cur.n_int;
    c.counts[4] = passes;
    c.counts[5] = n_split;
    for (int k = 0; k < ehm_ref::STOP_CODES; ++k) c.counts[6 + k] = 0;
    for (size_t l = 0; l < n_out; ++l) {
        if (stop[l] < 0 || stop[l] >= ehm_ref::STOP_CODES)
            return f_err.fail(EHM_E_NUMERIC, "refine: leaf %lld ends with stop code %d",
                              (long long)l, (int)stop[l]);
        ++c.counts[6 + stop[l]];
        if (c.stop) c.stop[l] = stop[l];
    }
    c.stats[2] = plan_seconds;
    const int rc = ehm_compiled_adopt(law, cur.n_int, cur.n_leaf, cur.node, cur.leaf_rec,
                                      cur.leaf_node, cur.root_entry, out);
    if (rc) return f_err.fail(rc, "refine: the refined law is refused: %s",
                              ehm_compiled_last_error());
    return EHM_OK;
}

}  // namespace

extern "C" {

const char* ehm_refine_last_error(void) { return f_err.c_str(); }

int ehm_compiled_refine(ehm_compiled* law, const double* root_vertices, const int32_t* levels,
                        const uint8_t* selected, const double* max_diameter,
                        const double* max_spread, const int32_t* leaf_mode, int64_t max_leaves,
                        int64_t capacity, ehm_compiled** out, int32_t* leaf_mode_out,
                        int32_t* origin, int8_t* stop, int64_t* counts, double* stats) {
    if (out) *out = nullptr;
    if (!law || !root_vertices || !levels || !out || !counts || !stats)
        return f_err.fail(EHM_E_INVALID, "refine: bad argument");
    const auto t0 = std::chrono::steady_clock::now();
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    if (const int rc = check_law_shape(f_err, v, "refine")) return rc;
    if (max_diameter && (!(*max_diameter >= 0.0) || !std::isfinite(*max_diameter)))
        return f_err.fail(EHM_E_INVALID, "refine: max_diameter = %g (a finite number >= 0)",
                          *max_diameter);
    for (int c = 0; max_spread && c < v.n_u; ++c)
        if (!(max_spread[c] >= 0.0) || !std::isfinite(max_spread[c]))
            return f_err.fail(EHM_E_INVALID, "refine: max_spread[%d] = %g (a finite number >= 0)",
                              c, max_spread[c]);
    const int64_t worst = ehm_ref::worst_case_leaves(v.n_leaf, levels, selected);
    if (worst < 0)
        return f_err.fail(EHM_E_INVALID, "refine: levels[%lld] = %d (0..%d)",
                          (long long)(-1 - worst), (int)levels[-1 - worst], EHM_REF_MAX_LEVELS);
    if (max_leaves < 1 || worst > max_leaves || worst >= ((int64_t)1 << 31))
        return f_err.fail(EHM_E_INVALID, "refine: the call could make %lld leaves, max_leaves is "
                          "%lld", (long long)worst, (long long)max_leaves);
    if ((origin || stop || (leaf_mode && leaf_mode_out)) && capacity < worst)
        return f_err.fail(EHM_E_INVALID, "refine: the per-leaf outputs hold %lld leaves, the call "
                          "could make %lld", (long long)capacity, (long long)worst);
    EHM_HIP_TRY(f_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(f_err, stream.create());
    // the law's arrays were written on its own stream (create) or by blocking copies (import)
    EHM_HIP_TRY(f_err, hipStreamSynchronize(v.stream));
    stats[0] = stats[1] = stats[2] = 0.0;
    const RefineCall c{root_vertices, levels, selected, max_diameter, max_spread, leaf_mode, worst,
                       leaf_mode_out, origin, stop, counts, stats};
    const int rc = v.single ? refine_law<float>(law, v, stream, c, out)
                            : refine_law<double>(law, v, stream, c, out);
    stats[1] = wall_since(t0);
    return rc;
}

}  // extern "C"
