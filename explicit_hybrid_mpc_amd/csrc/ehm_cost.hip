// Certified fuel bounds of a compiled law's closed loop: on a domain D of
// leaves that holds no seed and is closed under the may-reach relation (host CSR, as ehm_reach.hip
// takes it), a max-plus and a min-plus dynamic program over the rows bound the summed input 2-norm
// of every trajectory over k steps from above and from below:
//   U_0 = L_0 = 0,  U_(k+1)(l) = w_hi[l] + max_{t in row(l)} U_k(t),  L_(k+1)(l) = w_lo[l] + min L_k(t)
//
//   k_cost_closed   one wavefront per row of D: a seed, or a target outside D, puts the row into one
//                   word by atomicMin; the host names the smallest such row and refuses the domain
//   k_cost_weights  one thread per leaf of D, templated on the law's scalar, P and NU: the cell
//                   (leaf_cell through the parent table) and the leaf's map at its vertices as
//                   k_certify_cells, the 2-norm of each vertex input by the expression of
//                   rollout_apply, the distance of 0 from the hull of the vertex inputs and the pad
//                   that covers the rounding of the law's evaluation inside the cell
//   k_cost_sweep    one wavefront per row of D, the lanes striding `indices` so that the loads
//                   coalesce; each target's U_k and L_k are gathered behind one load of its index, a
//                   lane-local (value, index) maximum and minimum, a butterfly over the wavefront
//                   under the lexicographic rule (the larger / smaller value, among equals the smaller
//                   leaf), lane 0 writes U_(k+1), L_(k+1) and the two args into the other buffer
//   k_cost_book     one thread per leaf of D per sweep: the maximum of U_k and the minimum of L_k over
//                   D and over the start set, by shuffles, LDS and one integer atomic per block on
//                   order-preserving keys (key_of, ehm_cost_host.h) into arrays indexed by k, read
//                   once at the end
// A value is one double addition of a maximum or minimum, which do not depend on the order, and the
// args are decided by the leaf's index, not by its place in the row: every array is the numpy
// mirror's bit for bit (tests/cost_cpu.py).  All stores are plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_cost_host.h"
#include "ehm_relation_dev.h"

#define EHM_COST_CELL_BLOCK 64
#define EHM_COST_BLOCK 256
#define EHM_COST_WAVE 64

static_assert(ehm_cost::MAX_NU == EHM_R_MAX_NU, "the inputs a rollout steps");

namespace {

struct WeightArgs {
    long long n_dom;
    const int32_t* dom;             // [n_dom] the rows of D, ascending
    const void* node;               // of the law's scalar
    const void* leaf_rec;
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    ehm_cert::Parents par;
    int leaf_stride;
    double *w_hi, *w_lo, *pad;      // [n_leaf], NaN outside D
    int32_t* no_cell;               // the smallest leaf of D without a cell
};

template <class T, int P, int NU>
__global__ __launch_bounds__(EHM_COST_CELL_BLOCK) void k_cost_weights(WeightArgs A) {
#pragma clang fp contract(off)
    constexpr bool SINGLE = std::is_same<T, float>::value;
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n_dom) return;
    const int32_t l = A.dom[q];
    double V[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, static_cast<const T*>(A.node), A.root_entry,
                                    A.root_vertices, l, V);
    if (!ok) {
        atomicMin(A.no_cell, l);
        return;
    }
    const T* lr = static_cast<const T*>(A.leaf_rec) + (size_t)l * A.leaf_stride;
    double u[(P + 1) * NU];
#pragma unroll
    for (int i = 0; i <= P; ++i)
#pragma unroll
        for (int c = 0; c < NU; ++c) u[i * NU + c] = leaf_map_at<P>(lr, NU, c, &V[i * P]);
    // the largest vertex norm, each as rollout_apply takes it
    double top = 0.0;
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        double su = 0.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) su = su + u[i * NU + c] * u[i * NU + c];
        const double nrm = sqrt(su);
        top = (i == 0 || nrm > top) ? nrm : top;
    }
    // what a coordinate of the state moves by in the cell (a single law narrows the state first)
    double span[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double v0 = (double)lr[j];
        double d = 0.0, x = 0.0;
#pragma unroll
        for (int i = 0; i <= P; ++i) {
            const double di = fabs(V[i * P + j] - v0), xi = fabs(V[i * P + j]);
            d = di > d ? di : d;
            x = xi > x ? xi : x;
        }
        span[j] = SINGLE ? d + x : d;
    }
    double sg = 0.0, sr = 0.0;
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        double mn = u[c], mx = u[c];
#pragma unroll
        for (int i = 1; i <= P; ++i) {
            mn = u[i * NU + c] < mn ? u[i * NU + c] : mn;
            mx = u[i * NU + c] > mx ? u[i * NU + c] : mx;
        }
        const double g = mn > 0.0 ? mn : (-mx > 0.0 ? -mx : 0.0);
        sg = sg + g * g;
        double r = fabs((double)lr[P + c]);
#pragma unroll
        for (int j = 0; j < P; ++j) r = r + fabs((double)lr[P + NU + c * P + j]) * span[j];
        sr = sr + r * r;
    }
    const double eps = SINGLE ? 0x1p-24 : 0x1p-53;
    const double pad = ((double)(2 * P + NU + 8) * eps) * sqrt(sr);
    const double low = sqrt(sg) - pad;
    A.pad[l] = pad;
    A.w_hi[l] = top + pad;
    A.w_lo[l] = low > 0.0 ? low : 0.0;
}

// the row of a wavefront and its lane
__device__ __forceinline__ bool wave_row(long long n_dom, const int32_t* __restrict__ dom,
                                         int32_t& row, int& lane) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    lane = (int)(threadIdx.x % EHM_COST_WAVE);
    if (g / EHM_COST_WAVE >= n_dom) return false;
    row = dom[g / EHM_COST_WAVE];
    return true;
}

__global__ __launch_bounds__(EHM_COST_BLOCK) void k_cost_closed(
    long long n_dom, const int32_t* __restrict__ dom, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const int32_t* __restrict__ level,
    const uint8_t* __restrict__ in_dom, int32_t* bad) {
    int32_t row;
    int lane;
    if (!wave_row(n_dom, dom, row, lane)) return;
    bool off = level[row] == 0;
    const int32_t end = indptr[row + 1];
    for (int32_t e = indptr[row] + lane; e < end; e += EHM_COST_WAVE) off = off || !in_dom[indices[e]];
    if (__ballot(off) != 0ull && lane == 0) atomicMin(bad, row);
}

template <bool ARGS>
__global__ __launch_bounds__(EHM_COST_BLOCK) void k_cost_sweep(
    long long n_dom, const int32_t* __restrict__ dom, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, const double* __restrict__ w_hi,
    const double* __restrict__ w_lo, const double* __restrict__ U, const double* __restrict__ L,
    double* __restrict__ U_next, double* __restrict__ L_next, int32_t* __restrict__ arg_hi,
    int32_t* __restrict__ arg_lo) {
    int32_t row;
    int lane;
    if (!wave_row(n_dom, dom, row, lane)) return;
    const int32_t begin = indptr[row], end = indptr[row + 1];
    double hi = -INFINITY, lo = INFINITY;
    int32_t at_hi = INT_MAX, at_lo = INT_MAX;
    for (int32_t e = begin + lane; e < end; e += EHM_COST_WAVE) {
        const int32_t t = indices[e];
        const double u = U[t], l = L[t];
        if (u > hi || (u == hi && t < at_hi)) {
            hi = u;
            at_hi = t;
        }
        if (l < lo || (l == lo && t < at_lo)) {
            lo = l;
            at_lo = t;
        }
    }
#pragma unroll
    for (int s = EHM_COST_WAVE / 2; s > 0; s >>= 1) {
        const double u = __shfl_xor(hi, s, EHM_COST_WAVE), l = __shfl_xor(lo, s, EHM_COST_WAVE);
        const int32_t tu = __shfl_xor(at_hi, s, EHM_COST_WAVE);
        const int32_t tl = __shfl_xor(at_lo, s, EHM_COST_WAVE);
        if (u > hi || (u == hi && tu < at_hi)) {
            hi = u;
            at_hi = tu;
        }
        if (l < lo || (l == lo && tl < at_lo)) {
            lo = l;
            at_lo = tl;
        }
    }
    if (lane != 0) return;
    const bool empty = end == begin;        // no trajectory continues: nothing is claimed
    U_next[row] = w_hi[row] + (empty ? 0.0 : hi);
    L_next[row] = w_lo[row] + (empty ? 0.0 : lo);
    if (ARGS) {
        arg_hi[row] = empty ? -1 : at_hi;
        arg_lo[row] = empty ? -1 : at_lo;
    }
}

// keys [4][steps]: the maxima of U_k over D and over S, then the minima of L_k over D and over S
__global__ __launch_bounds__(EHM_COST_BLOCK) void k_cost_book(
    long long n_dom, const int32_t* __restrict__ dom, const uint8_t* __restrict__ in_start,
    const double* __restrict__ U, const double* __restrict__ L, long long steps, long long k,
    unsigned long long* keys) {
    constexpr int WAVES = EHM_COST_BLOCK / EHM_COST_WAVE;
    __shared__ unsigned long long red[4][WAVES];
    const int t = threadIdx.x, lane = t % EHM_COST_WAVE, wave = t / EHM_COST_WAVE;
    const long long q = (long long)blockIdx.x * EHM_COST_BLOCK + t;
    unsigned long long v[4] = {0ull, 0ull, ~0ull, ~0ull};
    if (q < n_dom) {
        const int32_t l = dom[q];
        const unsigned long long ku = ehm_cost::key_of(U[l]), kl = ehm_cost::key_of(L[l]);
        const bool s = in_start[l] != 0;
        v[0] = ku;
        v[1] = s ? ku : 0ull;
        v[2] = kl;
        v[3] = s ? kl : ~0ull;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int s = EHM_COST_WAVE / 2; s > 0; s >>= 1) {
            const unsigned long long o = __shfl_xor(v[j], s, EHM_COST_WAVE);
            v[j] = j < 2 ? (o > v[j] ? o : v[j]) : (o < v[j] ? o : v[j]);
        }
        if (lane == 0) red[j][wave] = v[j];
    }
    __syncthreads();
    if (t < 4) {
        unsigned long long r = red[t][0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const unsigned long long o = red[t][w];
            r = t < 2 ? (o > r ? o : r) : (o < r ? o : r);
        }
        if (t < 2) atomicMax(keys + (size_t)t * steps + k, r);
        else atomicMin(keys + (size_t)t * steps + k, r);
    }
}

typedef void (*weights_fn)(WeightArgs);
#define EHM_COST_NU(T, P) {&k_cost_weights<T, P, 1>, &k_cost_weights<T, P, 2>,      \
                           &k_cost_weights<T, P, 3>, &k_cost_weights<T, P, 4>}
#define EHM_COST_ALL(T) {EHM_COST_NU(T, 1), EHM_COST_NU(T, 2), EHM_COST_NU(T, 3),   \
                         EHM_COST_NU(T, 4), EHM_COST_NU(T, 5), EHM_COST_NU(T, 6),   \
                         EHM_COST_NU(T, 7), EHM_COST_NU(T, 8)}
const weights_fn k_weights64[EHM_CP][EHM_R_MAX_NU] = EHM_COST_ALL(double);
const weights_fn k_weights32[EHM_CP][EHM_R_MAX_NU] = EHM_COST_ALL(float);
#undef EHM_COST_ALL
#undef EHM_COST_NU

thread_local ehm_err_channel c_err;

}  // namespace

extern "C" {

const char* ehm_cost_last_error(void) { return c_err.c_str(); }

int ehm_cost_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_cost_opts), (int64_t)sizeof(ehm_cost_result),
                           (int64_t)sizeof(ehm_cost_leaves)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_compiled_cost(ehm_compiled* law, const ehm_cost_opts* o, ehm_cost_result* res,
                      const ehm_cost_leaves* lv) {
    if (!law || !o || !res || !lv) return c_err.fail(EHM_E_INVALID, "cost: bad argument");
    if (!o->root_vertices || !o->indptr || !o->level || !o->domain || !o->start ||
        (o->n_edges > 0 && !o->indices))
        return c_err.fail(EHM_E_INVALID, "cost: a required array is NULL");
    if (!lv->w_hi || !lv->w_lo || !lv->pad || !lv->hi || !lv->lo || !lv->max_hi || !lv->min_lo ||
        !lv->start_hi || !lv->start_lo || (o->want_paths && (!lv->path_hi || !lv->path_lo)))
        return c_err.fail(EHM_E_INVALID, "cost: a required output is NULL");
    const auto t_up = std::chrono::steady_clock::now();
    ehm_compiled_view v;
    ehm_compiled_get_view(law, &v);
    int rc = check_law_shape(c_err, v, "cost");
    if (rc) return rc;
    rc = ehm_cost::check_options(c_err, o, v.n_leaf, v.n_u);
    if (rc) return rc;
    std::vector<int32_t> ptr32, dom, start;
    rc = ehm_reach::check_csr(c_err, "cost", o->n_leaf, o->n_edges, o->n_level, o->indptr,
                              o->indices, ptr32);
    if (rc) return rc;
    const long long n = o->n_leaf;
    std::vector<uint8_t> dmask, smask;
    rc = ehm_cost::rows_of(c_err, "domain", o->domain, o->n_domain, n, dmask, dom);
    if (rc) return rc;
    rc = ehm_cost::rows_of(c_err, "start", o->start, o->n_start, n, smask, start);
    if (rc) return rc;
    rc = ehm_cost::check_subset(c_err, start, dmask);
    if (rc) return rc;
    const bool given = o->w_hi != nullptr;
    if (given) {
        rc = ehm_cost::check_weights(c_err, o->w_hi, o->w_lo, dom);
        if (rc) return rc;
    }
    std::memset(res, 0, sizeof *res);
    res->n_domain = (int64_t)dom.size();
    res->n_start = (int64_t)start.size();
    const int p = v.p, H = o->horizon;
    const long long n_dom = (long long)dom.size(), steps = (long long)H + 1;
    const size_t leaf_bytes = (size_t)n * sizeof(double);

    EHM_HIP_TRY(c_err, hipSetDevice(v.device));
    Stream stream;
    EHM_HIP_TRY(c_err, stream.create());
    DevRelation rel;
    DevBuf d_dom, d_dmask, d_smask, d_word;
    EHM_HIP_TRY(c_err, rel.upload(ptr32, o->indices, o->n_edges, o->level, n));
    EHM_HIP_TRY(c_err, d_dom.upload(dom.data(), dom.size() * sizeof(int32_t)));
    EHM_HIP_TRY(c_err, d_dmask.upload(dmask.data(), (size_t)n));
    EHM_HIP_TRY(c_err, d_smask.upload(smask.data(), (size_t)n));
    res->seconds_upload = wall_since(t_up);
    const int32_t* ptr = rel.ptr.as<const int32_t>();
    const int32_t* idx = rel.idx.as<const int32_t>();
    const int32_t* rows = d_dom.as<const int32_t>();
    const dim3 block(EHM_COST_BLOCK);
    const dim3 rgrid(blocks_of(n_dom * EHM_COST_WAVE, EHM_COST_BLOCK));
    const dim3 lgrid(blocks_of(n_dom, EHM_COST_BLOCK));

    // the domain: no seed, closed
    const int32_t none = INT_MAX;
    int32_t word = none;
    EHM_HIP_TRY(c_err, d_word.upload(&none, sizeof none));
    hipLaunchKernelGGL(k_cost_closed, rgrid, block, 0, stream, n_dom, rows, ptr, idx,
                       rel.level.as<const int32_t>(), d_dmask.as<const uint8_t>(),
                       d_word.as<int32_t>());
    EHM_HIP_TRY(c_err, hipGetLastError());
    EHM_HIP_TRY(c_err, hipMemcpyAsync(&word, d_word.ptr, sizeof word, hipMemcpyDeviceToHost, stream));
    EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
    rc = ehm_cost::domain_verdict(c_err, word == none ? -1 : word, n, o->level, ptr32.data(),
                                  o->indices, dmask);
    if (rc) return rc;

    // the weights
    DevBuf d_whi, d_wlo, d_pad;
    EventPair ev;
    if (given) {
        for (long long l = 0; l < n; ++l) {
            lv->w_hi[l] = dmask[(size_t)l] ? o->w_hi[l] : NAN;
            lv->w_lo[l] = dmask[(size_t)l] ? o->w_lo[l] : NAN;
            lv->pad[l] = dmask[(size_t)l] ? 0.0 : NAN;
        }
        EHM_HIP_TRY(c_err, d_whi.upload(lv->w_hi, leaf_bytes));
        EHM_HIP_TRY(c_err, d_wlo.upload(lv->w_lo, leaf_bytes));
    } else {
        ParentTable T;
        DevBuf d_roots;
        EHM_HIP_TRY(c_err, make_parents(v, stream, T));
        EHM_HIP_TRY(c_err, d_roots.upload(o->root_vertices,
                                          (size_t)v.n_roots * (p + 1) * p * sizeof(double)));
        EHM_HIP_TRY(c_err, d_whi.alloc(leaf_bytes));
        EHM_HIP_TRY(c_err, d_wlo.alloc(leaf_bytes));
        EHM_HIP_TRY(c_err, d_pad.alloc(leaf_bytes));
        // all ones is a NaN
        EHM_HIP_TRY(c_err, hipMemsetAsync(d_whi.ptr, 0xff, leaf_bytes, stream));
        EHM_HIP_TRY(c_err, hipMemsetAsync(d_wlo.ptr, 0xff, leaf_bytes, stream));
        EHM_HIP_TRY(c_err, hipMemsetAsync(d_pad.ptr, 0xff, leaf_bytes, stream));
        EHM_HIP_TRY(c_err, hipMemcpyAsync(d_word.ptr, &none, sizeof none, hipMemcpyHostToDevice,
                                          stream));
        WeightArgs A{n_dom, rows, v.node, v.leaf_rec, v.root_entry, d_roots.as<const double>(),
                     T.view(), v.leaf_stride, d_whi.as<double>(), d_wlo.as<double>(),
                     d_pad.as<double>(), d_word.as<int32_t>()};
        (void)hipEventRecord(ev.e0, stream);
        hipLaunchKernelGGL((v.single ? k_weights32 : k_weights64)[p - 1][v.n_u - 1],
                           dim3(blocks_of(n_dom, EHM_COST_CELL_BLOCK)), dim3(EHM_COST_CELL_BLOCK),
                           0, stream, A);
        (void)hipEventRecord(ev.e1, stream);
        EHM_HIP_TRY(c_err, hipGetLastError());
        EHM_HIP_TRY(c_err, hipMemcpyAsync(&word, d_word.ptr, sizeof word, hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->w_hi, d_whi.ptr, leaf_bytes, hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->w_lo, d_wlo.ptr, leaf_bytes, hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->pad, d_pad.ptr, leaf_bytes, hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
        ev.seconds(&res->seconds_weights);
        if (word != none)
            return c_err.fail(EHM_E_INVALID, "cost: leaf %d of the domain has no cell (no_cell)",
                              (int)word);
        for (long long l = 0; l < n; ++l)       // one NaN outside D, whatever filled the buffers
            if (!dmask[(size_t)l]) lv->w_hi[l] = lv->w_lo[l] = lv->pad[l] = NAN;
        rc = ehm_cost::check_weights(c_err, lv->w_hi, lv->w_lo, dom);
        if (rc) return rc;
    }

    // U_0 = L_0 = 0 on D, NaN outside; two buffers of each
    DevBuf d_U[2], d_L[2], d_keys, d_arg_hi, d_arg_lo;
    for (long long l = 0; l < n; ++l) lv->hi[l] = dmask[(size_t)l] ? 0.0 : NAN;
    for (int b = 0; b < 2; ++b) {
        EHM_HIP_TRY(c_err, d_U[b].upload(lv->hi, leaf_bytes));
        EHM_HIP_TRY(c_err, d_L[b].upload(lv->hi, leaf_bytes));
    }
    const size_t half = 2 * (size_t)steps * sizeof(unsigned long long);
    EHM_HIP_TRY(c_err, d_keys.alloc(2 * half));
    EHM_HIP_TRY(c_err, hipMemsetAsync(d_keys.ptr, 0, half, stream));
    EHM_HIP_TRY(c_err, hipMemsetAsync(d_keys.as<char>() + half, 0xff, half, stream));
    const size_t arg_bytes = (size_t)H * (size_t)n * sizeof(int32_t);
    if (o->want_paths) {
        EHM_HIP_TRY(c_err, d_arg_hi.alloc(arg_bytes));
        EHM_HIP_TRY(c_err, d_arg_lo.alloc(arg_bytes));
    }
    auto book = [&](long long k, int b) {
        hipLaunchKernelGGL(k_cost_book, lgrid, block, 0, stream, n_dom, rows,
                           d_smask.as<const uint8_t>(), d_U[b].as<const double>(),
                           d_L[b].as<const double>(), steps, k, d_keys.as<unsigned long long>());
    };
    (void)hipEventRecord(ev.e0, stream);
    book(0, 0);
    int cur = 0;
    for (long long k = 1; k <= H; ++k) {
        const size_t at = (size_t)(k - 1) * (size_t)n;
        if (o->want_paths)
            hipLaunchKernelGGL(k_cost_sweep<true>, rgrid, block, 0, stream, n_dom, rows, ptr, idx,
                               d_whi.as<const double>(), d_wlo.as<const double>(),
                               d_U[cur].as<const double>(), d_L[cur].as<const double>(),
                               d_U[cur ^ 1].as<double>(), d_L[cur ^ 1].as<double>(),
                               d_arg_hi.as<int32_t>() + at, d_arg_lo.as<int32_t>() + at);
        else
            hipLaunchKernelGGL(k_cost_sweep<false>, rgrid, block, 0, stream, n_dom, rows, ptr, idx,
                               d_whi.as<const double>(), d_wlo.as<const double>(),
                               d_U[cur].as<const double>(), d_L[cur].as<const double>(),
                               d_U[cur ^ 1].as<double>(), d_L[cur ^ 1].as<double>(),
                               (int32_t*)nullptr, (int32_t*)nullptr);
        cur ^= 1;
        book(k, cur);
    }
    (void)hipEventRecord(ev.e1, stream);
    EHM_HIP_TRY(c_err, hipGetLastError());
    std::vector<unsigned long long> keys(4 * (size_t)steps);
    EHM_HIP_TRY(c_err, hipMemcpyAsync(keys.data(), d_keys.ptr, 2 * half, hipMemcpyDeviceToHost,
                                      stream));
    EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->hi, d_U[cur].ptr, leaf_bytes, hipMemcpyDeviceToHost,
                                      stream));
    EHM_HIP_TRY(c_err, hipMemcpyAsync(lv->lo, d_L[cur].ptr, leaf_bytes, hipMemcpyDeviceToHost,
                                      stream));
    EHM_HIP_TRY(c_err, hipStreamSynchronize(stream));
    ev.seconds(&res->seconds_sweeps);
    for (long long k = 0; k < steps; ++k) {
        lv->max_hi[k] = ehm_cost::value_of(keys[(size_t)k]);
        lv->start_hi[k] = ehm_cost::value_of(keys[(size_t)(steps + k)]);
        lv->min_lo[k] = ehm_cost::value_of(keys[(size_t)(2 * steps + k)]);
        lv->start_lo[k] = ehm_cost::value_of(keys[(size_t)(3 * steps + k)]);
    }
    if (o->want_paths) {
        std::vector<int32_t> arg((size_t)H * (size_t)n);
        EHM_HIP_TRY(c_err, hipMemcpy(arg.data(), d_arg_hi.ptr, arg_bytes, hipMemcpyDeviceToHost));
        ehm_cost::walk_path(arg.data(), n, H,
                            ehm_cost::first_attaining(lv->hi, start, lv->start_hi[H]), lv->path_hi);
        EHM_HIP_TRY(c_err, hipMemcpy(arg.data(), d_arg_lo.ptr, arg_bytes, hipMemcpyDeviceToHost));
        ehm_cost::walk_path(arg.data(), n, H,
                            ehm_cost::first_attaining(lv->lo, start, lv->start_lo[H]), lv->path_lo);
    }
    return EHM_OK;
}

}  // extern "C"
