// The reach tube and the limit set of a compiled law's closed loop: the
// forward analysis of the may-reach relation ehm_core.hip builds, handed over as host CSR, and the
// bounding boxes of the leaf sets it produces.  Seeds (level 0) are absorbing: their rows are never
// read.  Three phases over one set of kernels:
//   A  arrival: sweep k writes k into every target without an arrival of a row whose arrival is k - 1
//   B  D_0 = the closure, D_(j+1) = post(D_j) down to the fixed point; depart, the first set a leaf
//      is missing from
//   C  R_0 = the start set, R_(k+1) = post(R_k) for the horizon
//
//   k_reach_leaf_boxes  one thread per leaf, templated on the law's scalar and on P, once per call:
//                       the cell (leaf_cell through the parent table, as k_certify_cells), its lo and
//                       hi per coordinate, leaf-fastest; NaN without a cell
//   k_reach_push        phase A.  What a sweep writes is k, what it tests for is k - 1 and "no arrival
//                       yet": one array is enough and the sweep is Jacobi (k_core_sweep's argument)
//   k_reach_post        phases B and C: every row of the current set marks its targets in a cleared
//                       array; many lanes storing the same byte is the only race
//   k_reach_book        one pass over the leaves per sweep: depart, the set's size, what left it, and
//                       the set's box as per-block partials (wavefront shuffles, then LDS)
//   k_reach_final       one block: the partials into the box of step k (phase A: joined with the box
//                       of step k - 1, the tube is cumulative)
// k_reach_push and k_reach_post exist in two row mappings: one thread per row, and one wavefront per
// row with the lanes striding it so that the loads of `indices` coalesce.  Sizes and boxes go into
// device arrays indexed by the step and are read once at the end; the host reads one counter every
// EHM_REACH_POLL sweeps, and a sweep after convergence rewrites the same set.  Minimum and maximum
// do not depend on the order, so every box is numpy's over the same cells (tests/reach_cpu.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_reach_host.h"
#include "ehm_relation_dev.h"

#define EHM_REACH_CELL_BLOCK 64
#define EHM_REACH_BLOCK 256
#define EHM_REACH_WAVE 64
#define EHM_REACH_POLL 8            // sweeps between two reads of a counter

namespace {

struct LeafBoxArgs {
    long long n;
    const void* node;               // of the law's scalar
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    ehm_cert::Parents par;
    double* box;                    // [2][P][n]: lo, hi; leaf-fastest
};

template <class T, int P>
__global__ __launch_bounds__(EHM_REACH_CELL_BLOCK) void k_reach_leaf_boxes(LeafBoxArgs A) {
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= A.n) return;
    double V[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, static_cast<const T*>(A.node), A.root_entry,
                                    A.root_vertices, (int32_t)l, V);
#pragma unroll
    for (int c = 0; c < P; ++c) {
        double lo = V[c], hi = V[c];
#pragma unroll
        for (int i = 1; i <= P; ++i) {
            lo = V[i * P + c] < lo ? V[i * P + c] : lo;
            hi = V[i * P + c] > hi ? V[i * P + c] : hi;
        }
        A.box[(size_t)c * A.n + l] = ok ? lo : NAN;
        A.box[(size_t)(P + c) * A.n + l] = ok ? hi : NAN;
    }
}

// the row of a thread and its first edge and stride in it
template <bool WAVE>
__device__ __forceinline__ void row_of(long long& row, int& lane, int& stride) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    row = WAVE ? g / EHM_REACH_WAVE : g;
    lane = WAVE ? (int)(threadIdx.x % EHM_REACH_WAVE) : 0;
    stride = WAVE ? EHM_REACH_WAVE : 1;
}

// Sweep k >= 1 of phase A.
template <bool WAVE>
__global__ __launch_bounds__(EHM_REACH_BLOCK) void k_reach_push(
    long long n, int k, const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const int32_t* __restrict__ level, int32_t* arrival) {
    long long row;
    int lane, stride;
    row_of<WAVE>(row, lane, stride);
    if (row >= n || arrival[row] != k - 1 || level[row] == 0) return;
    const int32_t end = indptr[row + 1];
    for (int32_t e = indptr[row] + lane; e < end; e += stride) {
        const int32_t t = indices[e];
        if (arrival[t] < 0) arrival[t] = k;
    }
}

// next |= post(cur); next was cleared
template <bool WAVE>
__global__ __launch_bounds__(EHM_REACH_BLOCK) void k_reach_post(
    long long n, const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const int32_t* __restrict__ level, const uint8_t* __restrict__ cur, uint8_t* next) {
    long long row;
    int lane, stride;
    row_of<WAVE>(row, lane, stride);
    if (row >= n || !cur[row] || level[row] == 0) return;
    const int32_t end = indptr[row + 1];
    for (int32_t e = indptr[row] + lane; e < end; e += stride) next[indices[e]] = 1;
}

struct BookArgs {
    long long n;
    int k, p;
    const int32_t* arrival;         // phase A: the set is {arrival == k}; else nullptr
    const uint8_t* set;             // phases B, C: the set
    const uint8_t* prev;            // phase B: D_(k-1); else nullptr
    int32_t* depart;                // phase B
    const double* leaf_box;         // [2][p][n]
    unsigned long long* size;       // [steps]
    unsigned long long* gone;       // [steps], phase B
    double* partial;                // [blocks][2 p]: +inf / -inf where the block adds nothing
};

__global__ __launch_bounds__(EHM_REACH_BLOCK) void k_reach_book(BookArgs A) {
    constexpr int WAVES = EHM_REACH_BLOCK / EHM_REACH_WAVE;
    __shared__ unsigned int cnt[2];
    __shared__ double red[2 * EHM_CP][WAVES];
    const int t = threadIdx.x, lane = t % EHM_REACH_WAVE, wave = t / EHM_REACH_WAVE;
    const long long l = (long long)blockIdx.x * EHM_REACH_BLOCK + t;
    if (t < 2) cnt[t] = 0u;
    __syncthreads();
    bool in = false, out = false;
    if (l < A.n) {
        in = A.arrival ? A.arrival[l] == A.k : A.set[l] != 0;
        out = A.prev && A.prev[l] && !in;
        if (out) A.depart[l] = A.k;
    }
    const unsigned n_in = (unsigned)__popcll(__ballot(in));
    const unsigned n_out = (unsigned)__popcll(__ballot(out));
    if (lane == 0) {
        if (n_in) atomicAdd(&cnt[0], n_in);
        if (n_out) atomicAdd(&cnt[1], n_out);
    }
    __syncthreads();
    const unsigned members = cnt[0];
    if (t == 0) {
        if (members) atomicAdd(A.size + A.k, (unsigned long long)members);
        if (cnt[1]) atomicAdd(A.gone + A.k, (unsigned long long)cnt[1]);
    }
    const int p2 = 2 * A.p;
    double* part = A.partial + (size_t)blockIdx.x * p2;
    if (members == 0) {                 // the whole block: nothing to reduce
        if (t < p2) part[t] = t < A.p ? INFINITY : -INFINITY;
        return;
    }
    for (int j = 0; j < p2; ++j) {
        const bool low = j < A.p;
        double v = low ? INFINITY : -INFINITY;
        if (in) {
            const double b = A.leaf_box[(size_t)j * A.n + l];
            v = b == b ? b : v;         // a leaf without a cell adds nothing
        }
#pragma unroll
        for (int s = EHM_REACH_WAVE / 2; s > 0; s >>= 1) {
            const double o = __shfl_xor(v, s, EHM_REACH_WAVE);
            v = low ? (o < v ? o : v) : (o > v ? o : v);
        }
        if (lane == 0) red[j][wave] = v;
    }
    __syncthreads();
    if (t < p2) {
        const bool low = t < A.p;
        double v = red[t][0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const double o = red[t][w];
            v = low ? (o < v ? o : v) : (o > v ? o : v);
        }
        part[t] = v;
    }
}

// box[k] [2 p] from the partials of `blocks` blocks; join: with box[k - 1] (k >= 1).  One block.
__global__ __launch_bounds__(EHM_REACH_BLOCK) void k_reach_final(long long blocks, int p, int k,
                                                                 int join,
                                                                 const double* __restrict__ partial,
                                                                 double* box) {
    __shared__ double red[EHM_REACH_BLOCK];
    const int t = threadIdx.x, p2 = 2 * p;
    for (int j = 0; j < p2; ++j) {
        const bool low = j < p;
        double v = low ? INFINITY : -INFINITY;
        for (long long b = t; b < blocks; b += EHM_REACH_BLOCK) {
            const double o = partial[(size_t)b * p2 + j];
            v = low ? (o < v ? o : v) : (o > v ? o : v);
        }
        red[t] = v;
        __syncthreads();
        for (int s = EHM_REACH_BLOCK / 2; s > 0; s >>= 1) {
            if (t < s) {
                const double o = red[t + s];
                red[t] = low ? (o < red[t] ? o : red[t]) : (o > red[t] ? o : red[t]);
            }
            __syncthreads();
        }
        if (t == 0) {
            v = red[0];
            if (join && k > 0) {
                const double o = box[(size_t)(k - 1) * p2 + j];
                if (o == o) v = low ? (o < v ? o : v) : (o > v ? o : v);
            }
            // no leaf with a cell: NaN; else + 0.0, so that a zero bound is +0 whatever the order
            box[(size_t)k * p2 + j] = (v == INFINITY || v == -INFINITY) ? NAN : v + 0.0;
        }
        __syncthreads();
    }
}

typedef void (*leaf_boxes_fn)(LeafBoxArgs);
#define EHM_REACH_ALL(T) {&k_reach_leaf_boxes<T, 1>, &k_reach_leaf_boxes<T, 2>,     \
                          &k_reach_leaf_boxes<T, 3>, &k_reach_leaf_boxes<T, 4>,     \
                          &k_reach_leaf_boxes<T, 5>, &k_reach_leaf_boxes<T, 6>,     \
                          &k_reach_leaf_boxes<T, 7>, &k_reach_leaf_boxes<T, 8>}
const leaf_boxes_fn k_boxes64[EHM_CP] = EHM_REACH_ALL(double);
const leaf_boxes_fn k_boxes32[EHM_CP] = EHM_REACH_ALL(float);
#undef EHM_REACH_ALL

thread_local ehm_err_channel r_err;

}  // namespace

extern "C" {

const char* ehm_reach_last_error(void) { return r_err.c_str(); }

int ehm_reach_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_reach_opts), (int64_t)sizeof(ehm_reach_result),
                           (int64_t)sizeof(ehm_reach_leaves)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_compiled_reach(ehm_compiled* law, const ehm_reach_opts* o, ehm_reach_result* res,
                       const ehm_reach_leaves* lv) {
    if (!law || !o || !res || !lv) return r_err.fail(EHM_E_INVALID, "reach: bad argument");
    if (!o->root_vertices || !o->indptr || !o->level || !o->start || (o->n_edges > 0 && !o->indices))
        return r_err.fail(EHM_E_INVALID, "reach: a required array is NULL");
    if (!lv->arrival || !lv->depart || !lv->limit || !lv->tube_box || !lv->tube_count ||
        !lv->settle_box || !lv->settle_count || !lv->step_box || !lv->step_count ||
        (o->want_steps && !lv->steps))
        return r_err.fail(EHM_E_INVALID, "reach: a required output is NULL");
    const auto t_up = std::chrono::steady_clock::now();
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    int rc = check_law_shape(r_err, v, "reach");
    if (rc) return rc;
    rc = ehm_reach::check_options(r_err, o, v.n_leaf);
    if (rc) return rc;
    std::vector<int32_t> ptr32;
    rc = ehm_reach::check_relation(r_err, o, ptr32);
    if (rc) return rc;
    std::vector<uint8_t> mask;
    rc = ehm_reach::start_mask(r_err, o, mask);
    if (rc) return rc;
    std::memset(res, 0, sizeof *res);
    res->leak_step = -1;
    const long long n = o->n_leaf;
    const int p = v.p, p2 = 2 * p;
    const long long cap = std::min<long long>(o->max_sweeps, n);     // sweeps of a phase
    const bool wave = o->row_map == EHM_REACH_MAP_WAVE;

    EHM_HIP_TRY(r_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(r_err, stream.create());
    ParentTable T;
    EHM_HIP_TRY(r_err, make_parents(v, stream, T));
    DevBuf d_roots, d_lbox, d_arrival, d_part, d_size, d_gone, d_box;
    DevRelation rel;
    const size_t cell = (size_t)(p + 1) * p;
    EHM_HIP_TRY(r_err, d_roots.upload(o->root_vertices, (size_t)v.n_roots * cell * sizeof(double)));
    EHM_HIP_TRY(r_err, rel.upload(ptr32, o->indices, o->n_edges, o->level, n));
    res->seconds_upload = wall_since(t_up);
    EHM_HIP_TRY(r_err, d_lbox.alloc((size_t)p2 * n * sizeof(double)));
    const long long blocks = blocks_of(n, EHM_REACH_BLOCK);
    EHM_HIP_TRY(r_err, d_part.alloc((size_t)blocks * p2 * sizeof(double)));
    // the counters and boxes of one phase at a time, indexed by the step
    const long long steps_cap = std::max<long long>(cap, o->horizon) + 1;
    const size_t cnt_bytes = (size_t)steps_cap * sizeof(unsigned long long);
    EHM_HIP_TRY(r_err, d_size.alloc(cnt_bytes));
    EHM_HIP_TRY(r_err, d_gone.alloc(cnt_bytes));
    EHM_HIP_TRY(r_err, d_box.alloc((size_t)steps_cap * p2 * sizeof(double)));

    // the boxes of all leaves, once
    EventPair ev;
    {
        LeafBoxArgs A{n, v.node, v.root_entry, d_roots.as<const double>(), T.view(),
                      d_lbox.as<double>()};
        (void)hipEventRecord(ev.e0, stream);
        hipLaunchKernelGGL((v.single ? k_boxes32 : k_boxes64)[p - 1],
                           dim3(blocks_of(n, EHM_REACH_CELL_BLOCK)), dim3(EHM_REACH_CELL_BLOCK), 0,
                           stream, A);
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(r_err, hipGetLastError());
        if (lv->leaf_box)
            EHM_HIP_TRY(r_err, hipMemcpyAsync(lv->leaf_box, d_lbox.ptr,
                                              (size_t)p2 * n * sizeof(double),
                                              hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(r_err, hipStreamSynchronize(stream));
        ev.seconds(&res->seconds_boxes);
    }

    const dim3 block(EHM_REACH_BLOCK), lgrid((unsigned)blocks);
    const dim3 rgrid(wave ? blocks_of(n * EHM_REACH_WAVE, EHM_REACH_BLOCK) : (unsigned)blocks);
    const int32_t* ptr = rel.ptr.as<const int32_t>();
    const int32_t* idx = rel.idx.as<const int32_t>();
    const int32_t* level = rel.level.as<const int32_t>();
    BookArgs B{};
    B.n = n;
    B.p = p;
    B.leaf_box = d_lbox.as<const double>();
    B.size = d_size.as<unsigned long long>();
    B.gone = d_gone.as<unsigned long long>();
    B.partial = d_part.as<double>();
    // the bookkeeping of step k: the set's size, what left it, its box
    auto book = [&](long long k, const int32_t* arrival, const uint8_t* set, const uint8_t* prev,
                    int32_t* depart, int join) {
        B.k = (int)k;
        B.arrival = arrival;
        B.set = set;
        B.prev = prev;
        B.depart = depart;
        hipLaunchKernelGGL(k_reach_book, lgrid, block, 0, stream, B);
        hipLaunchKernelGGL(k_reach_final, dim3(1), block, 0, stream, blocks, p, (int)k, join,
                           d_part.as<const double>(), d_box.as<double>());
    };
    auto post = [&](const uint8_t* cur, uint8_t* next) -> hipError_t {
        const hipError_t e = hipMemsetAsync(next, 0, (size_t)n, stream);
        if (e != hipSuccess) return e;
        if (wave)
            hipLaunchKernelGGL(k_reach_post<true>, rgrid, block, 0, stream, n, ptr, idx, level, cur,
                               next);
        else
            hipLaunchKernelGGL(k_reach_post<false>, rgrid, block, 0, stream, n, ptr, idx, level, cur,
                               next);
        return hipGetLastError();
    };
    auto clear_counters = [&]() -> hipError_t {
        const hipError_t e = hipMemsetAsync(d_size.ptr, 0, cnt_bytes, stream);
        return e != hipSuccess ? e : hipMemsetAsync(d_gone.ptr, 0, cnt_bytes, stream);
    };
    std::vector<unsigned long long> h_size((size_t)steps_cap), h_gone((size_t)steps_cap);
    // rows 0 .. last of the phase's counters and boxes to the host
    auto fetch = [&](long long last, double* box_out) -> hipError_t {
        hipError_t e = hipMemcpyAsync(h_size.data(), d_size.ptr,
                                      (size_t)(last + 1) * sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(h_gone.data(), d_gone.ptr,
                               (size_t)(last + 1) * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(box_out, d_box.ptr, (size_t)(last + 1) * p2 * sizeof(double),
                               hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    };

    // ---- phase A ----
    for (long long l = 0; l < n; ++l) lv->arrival[l] = mask[(size_t)l] ? 0 : -1;
    EHM_HIP_TRY(r_err, d_arrival.upload(lv->arrival, (size_t)n * sizeof(int32_t)));
    EHM_HIP_TRY(r_err, clear_counters());
    (void)hipEventRecord(ev.e0, stream);
    book(0, d_arrival.as<const int32_t>(), nullptr, nullptr, nullptr, 0);
    EHM_HIP_TRY(r_err, hipGetLastError());
    long long made = 0;
    while (made < cap) {
        for (int j = 0; j < EHM_REACH_POLL && made < cap; ++j) {
            ++made;
            if (wave)
                hipLaunchKernelGGL(k_reach_push<true>, rgrid, block, 0, stream, n, (int)made, ptr,
                                   idx, level, d_arrival.as<int32_t>());
            else
                hipLaunchKernelGGL(k_reach_push<false>, rgrid, block, 0, stream, n, (int)made, ptr,
                                   idx, level, d_arrival.as<int32_t>());
            book(made, d_arrival.as<const int32_t>(), nullptr, nullptr, nullptr, 1);
        }
        EHM_HIP_TRY(r_err, hipGetLastError());
        unsigned long long fresh = 0;
        EHM_HIP_TRY(r_err, hipMemcpyAsync(&fresh, d_size.as<unsigned long long>() + made,
                                          sizeof fresh, hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(r_err, hipStreamSynchronize(stream));
        if (!fresh) break;
    }
    (void)hipEventRecord(ev.e1, stream);
    EHM_HIP_TRY(r_err, hipMemcpyAsync(lv->arrival, d_arrival.ptr, (size_t)n * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, stream));
    std::vector<double> h_box((size_t)steps_cap * p2);
    EHM_HIP_TRY(r_err, fetch(made, h_box.data()));
    ev.seconds(&res->seconds_arrival);
    bool a_done = false;
    ehm_reach::arrival_outcome(h_size.data(), made, a_done, res->n_arrival);
    res->arrival_done = a_done ? 1 : 0;
    res->sweeps_arrival = made;
    {
        long long total = 0;
        for (long long k = 0; k <= res->n_arrival; ++k) {
            total += (long long)h_size[(size_t)k];
            lv->tube_count[k] = total;
        }
        std::memcpy(lv->tube_box, h_box.data(), (size_t)(res->n_arrival + 1) * p2 * sizeof(double));
    }
    res->leak_step = ehm_reach::leak_step(lv->arrival, o->level, n);

    // ---- phase B ----
    DevBuf d_a, d_b, d_depart;
    std::memset(lv->limit, 0, (size_t)n);
    for (long long l = 0; l < n; ++l) lv->depart[l] = -1;
    if (a_done && res->leak_step < 0) {
        std::vector<uint8_t> closure((size_t)n);
        for (long long l = 0; l < n; ++l) closure[(size_t)l] = lv->arrival[l] >= 0;
        EHM_HIP_TRY(r_err, d_a.upload(closure.data(), (size_t)n));
        EHM_HIP_TRY(r_err, d_b.alloc((size_t)n));
        EHM_HIP_TRY(r_err, d_depart.alloc((size_t)n * sizeof(int32_t)));
        EHM_HIP_TRY(r_err, hipMemsetAsync(d_depart.ptr, 0xff, (size_t)n * sizeof(int32_t), stream));
        EHM_HIP_TRY(r_err, clear_counters());
        uint8_t* cur = d_a.as<uint8_t>();
        uint8_t* next = d_b.as<uint8_t>();
        (void)hipEventRecord(ev.e0, stream);
        book(0, nullptr, cur, nullptr, nullptr, 0);
        EHM_HIP_TRY(r_err, hipGetLastError());
        made = 0;
        while (made < cap) {
            for (int j = 0; j < EHM_REACH_POLL && made < cap; ++j) {
                ++made;
                EHM_HIP_TRY(r_err, post(cur, next));
                book(made, nullptr, next, cur, d_depart.as<int32_t>(), 0);
                std::swap(cur, next);
            }
            EHM_HIP_TRY(r_err, hipGetLastError());
            unsigned long long last[2] = {0, 0};
            EHM_HIP_TRY(r_err, hipMemcpyAsync(&last[0], d_size.as<unsigned long long>() + made,
                                              sizeof last[0], hipMemcpyDeviceToHost, stream));
            EHM_HIP_TRY(r_err, hipMemcpyAsync(&last[1], d_gone.as<unsigned long long>() + made,
                                              sizeof last[1], hipMemcpyDeviceToHost, stream));
            EHM_HIP_TRY(r_err, hipStreamSynchronize(stream));
            if (!last[0] || !last[1]) break;
        }
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(r_err, hipMemcpyAsync(lv->limit, cur, (size_t)n, hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(r_err, hipMemcpyAsync(lv->depart, d_depart.ptr, (size_t)n * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(r_err, fetch(made, h_box.data()));
        ev.seconds(&res->seconds_settle);
        bool b_done = false;
        ehm_reach::settle_outcome(h_size.data(), h_gone.data(), made, b_done, res->settle);
        res->settle_done = b_done ? 1 : 0;
        res->sweeps_settle = made;
        for (long long j = 0; j <= res->settle; ++j)
            lv->settle_count[j] = (int64_t)h_size[(size_t)j];
        std::memcpy(lv->settle_box, h_box.data(), (size_t)(res->settle + 1) * p2 * sizeof(double));
        d_a.reset();
        d_b.reset();
    }

    // ---- phase C ----
    {
        const long long last = ehm_reach::last_step(o->horizon, res->leak_step, a_done,
                                                    o->max_sweeps);
        res->n_steps = last + 1;
        const size_t rows = o->want_steps ? (size_t)(last + 1) : 2;
        EHM_HIP_TRY(r_err, d_a.alloc(rows * (size_t)n));
        uint8_t* base = d_a.as<uint8_t>();
        EHM_HIP_TRY(r_err, hipMemcpyAsync(base, mask.data(), (size_t)n, hipMemcpyHostToDevice,
                                          stream));
        EHM_HIP_TRY(r_err, clear_counters());
        (void)hipEventRecord(ev.e0, stream);
        uint8_t* cur = base;
        book(0, nullptr, cur, nullptr, nullptr, 0);
        for (long long k = 1; k <= last; ++k) {
            uint8_t* next = base + (o->want_steps ? (size_t)k : (size_t)(k & 1)) * (size_t)n;
            EHM_HIP_TRY(r_err, post(cur, next));
            book(k, nullptr, next, nullptr, nullptr, 0);
            cur = next;
        }
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(r_err, hipGetLastError());
        if (o->want_steps)
            EHM_HIP_TRY(r_err, hipMemcpyAsync(lv->steps, base, rows * (size_t)n,
                                              hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(r_err, fetch(last, lv->step_box));
        ev.seconds(&res->seconds_steps);
        for (long long k = 0; k <= last; ++k) lv->step_count[k] = (int64_t)h_size[(size_t)k];
    }
    return EHM_OK;
}

}  // extern "C"
