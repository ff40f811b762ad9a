// Sampled audit of an explicit law's epsilon-suboptimality: what the
// reference's PostProcessor does with invariant_set.randomPoint after a partition, on the device.
//
//   k_audit_sample   one thread per sample id: Philox words -> a cell and a point uniform in it
//   k_audit_cost     the law as deployed at each sample: the walk of k_explicit_eval (the device
//                    functions of ehm_explicit_dev.h, root locator included), the weights in the
//                    located leaf, Vbar interpolated from the leaf's vertex costs
//   k_audit_reduce   statuses, counts and the histogram by integer atomics, the worst sample by a
//                    per-workgroup reduction the host merges (ties to the smaller id; a NaN ratio
//                    is binned and never the worst): the rules and the tree of ehm_verdict.h
//
// V* and delta_idx come from ehm_solve_pt_batch itself (its re-solve of stalled LPs included): the
// points of a chunk make one round trip through the host, which the LPs dwarf.  All arithmetic
// that a result depends on runs under fp contract(off) from 0.0 in a fixed order -- one rounding
// per operation, so a numpy mirror (tests/audit_cpu.py) is bit-equal -- except the weights, which
// are those of the evaluation kernel (products fused into their sums).  No floating-point sum is
// reduced across samples: nothing reported depends on the launch shape or the chunk size.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_audit_sample.h"
#include "ehm_explicit_dev.h"
#include "ehm_explicit_view.h"
#include "ehm_host.h"
#include "ehm_philox.h"
#include "ehm_verdict.h"

#define EHM_AUDIT_BLOCK 256
#define EHM_AUDIT_BINS EHM_VERDICT_BINS
// counters of a run: [0..4] statuses, [5] relocated, [6..38] histogram
#define EHM_AUDIT_COUNTERS (5 + 1 + EHM_AUDIT_BINS)
#define EHM_AUDIT_NO_ID 0xffffffffffffffffULL

namespace {

__global__ void k_audit_sample(long long n, uint64_t first, int mode, int kper, uint64_t seed,
                               int p, long long n_cells, const double* __restrict__ cdf,
                               const double* __restrict__ V, double* __restrict__ X,
                               int32_t* __restrict__ cell) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint64_t s = first + (uint64_t)q;
    // words 0..p: word k is word k % 4 of the block with counter (s, k / 4, 0, 0)
    uint64_t w[4 * ((EHM_XP + 4) / 4)];
    const int n_blk = (p + 4) / 4;
    for (int j = 0; j < n_blk; ++j) {
        uint64_t c[4] = {s, (uint64_t)j, 0, 0};
        ehm_philox4x64_10(c, seed, 1);
        for (int i = 0; i < 4; ++i) w[4 * j + i] = c[i];
    }
    long long ci;
    if (mode == EHM_AUDIT_PER_LEAF) {
        const uint64_t cq = s / (uint64_t)kper;
        ci = cq < (uint64_t)n_cells ? (long long)cq : n_cells - 1;
    } else {
        const double u = (double)(w[0] >> 11) * 0x1p-53;
        const double t = u * cdf[n_cells - 1];
        long long lo = 0, hi = n_cells - 1;         // first i with cdf[i] > t, at most the last
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (cdf[mid] > t) hi = mid;
            else lo = mid + 1;
        }
        ci = lo;
    }
    double g[EHM_XP];
    for (int i = 0; i < p; ++i) {                   // insertion sort, ascending
        const double v = (double)(w[1 + i] >> 11) * 0x1p-53;
        int j = i;
        while (j > 0 && g[j - 1] > v) {
            g[j] = g[j - 1];
            --j;
        }
        g[j] = v;
    }
    const double* R = V + (size_t)ci * (p + 1) * p;
    double x[EHM_XP];
    const double w0 = g[0];
    for (int c = 0; c < p; ++c) x[c] = w0 * R[c];
    for (int i = 1; i <= p; ++i) {
        const double wi = (i < p) ? (g[i] - g[i - 1]) : (1.0 - g[p - 1]);
        for (int c = 0; c < p; ++c) x[c] = x[c] + wi * R[i * p + c];
    }
    for (int c = 0; c < p; ++c) X[q * p + c] = x[c];
    cell[q] = (int32_t)ci;
}

__global__ void k_audit_cost(DevExplicit E, long long n, const double* __restrict__ X,
                             const int32_t* __restrict__ nbr, const double* __restrict__ vcost,
                             const uint8_t* __restrict__ nflags, int32_t* __restrict__ leaf,
                             double* __restrict__ vbar, double* __restrict__ wmin,
                             int32_t* __restrict__ closed) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int p = E.p;
    double x[EHM_XP], alpha[EHM_XP], a0;
    for (int c = 0; c < p; ++c) x[c] = X[q * p + c];
    int visited = 0;
    const int32_t root = nbr ? explicit_locate_root(E, x, q, nbr) : -1;
    const long long k = explicit_walk(E, x, root, visited);
    (void)weights(E, k, x, alpha, a0);
    const double* c = vcost + (size_t)k * (p + 1);
    double v = a0 * c[0], lo = a0;
    for (int i = 0; i < p; ++i) {
        v += c[i + 1] * alpha[i];
        lo = alpha[i] < lo ? alpha[i] : lo;
    }
    leaf[q] = (int32_t)k;
    vbar[q] = v;
    wmin[q] = lo;
    closed[q] = nflags[k] & 1;
}

__global__ __launch_bounds__(EHM_AUDIT_BLOCK) void k_audit_reduce(
    long long n, uint64_t first, const double* __restrict__ vbar, const double* __restrict__ vstar,
    const int32_t* __restrict__ didx, const int32_t* __restrict__ closed,
    const int32_t* __restrict__ leaf, const int32_t* __restrict__ cell,
    const int32_t* __restrict__ cell_node, double eps_a, double eps_r, double rtol,
    int32_t* __restrict__ status, unsigned long long* __restrict__ counters,
    double* __restrict__ blk_ratio, unsigned long long* __restrict__ blk_id) {
#pragma clang fp contract(off)
    __shared__ unsigned int cnt[EHM_AUDIT_COUNTERS];
    ehm_verdict::counters_zero<EHM_AUDIT_BLOCK, EHM_AUDIT_COUNTERS>(cnt);
    __syncthreads();
    const long long q = (long long)blockIdx.x * EHM_AUDIT_BLOCK + threadIdx.x;
    double ratio = -INFINITY;
    unsigned long long id = EHM_AUDIT_NO_ID;
    if (q < n) {
        const double vs = vstar[q];
        const double gap = vbar[q] - vs;
        const double bound = ehm_verdict::bound_of(eps_a, eps_r, vs);
        int st;
        if (didx[q] < 0) st = 4;
        else if (!closed[q]) st = 3;
        else st = ehm_verdict::gap_status(gap, bound, ehm_verdict::slack_of(rtol, vs));
        status[q] = st;
        atomicAdd(&cnt[st], 1u);
        if (leaf[q] != cell_node[cell[q]]) atomicAdd(&cnt[5], 1u);
        if (st <= 2) {
            const double r = ehm_verdict::ratio_of(gap, bound);
            atomicAdd(&cnt[6 + ehm_verdict::ratio_bin(r)], 1u);
            if (ehm_verdict::ratio_is_candidate(r)) {
                ratio = r;
                id = first + (unsigned long long)q;
            }
        }
    }
    ehm_verdict::block_worst<EHM_AUDIT_BLOCK>(
        ratio, id,
        [](double ra, unsigned long long ia, double rb, unsigned long long ib) {
            return ehm_verdict::ratio_beats(ra, ia, rb, ib);
        },
        [](unsigned long long i) { return i != EHM_AUDIT_NO_ID; });
    if (threadIdx.x == 0) {
        blk_ratio[blockIdx.x] = ratio;
        blk_id[blockIdx.x] = id;
    }
    ehm_verdict::counters_flush<EHM_AUDIT_BLOCK, EHM_AUDIT_COUNTERS>(cnt, counters);
}

// what both entry points ask of opts; `audit`: also the fields the sampler alone does not read
int check_opts(const ehm_explicit_view& v, const ehm_audit_opts* o, bool audit) {
    if (!o) return ehm_explicit_fail(EHM_E_INVALID, "audit: no options");
    if (o->mode != EHM_AUDIT_UNIFORM && o->mode != EHM_AUDIT_PER_LEAF)
        return ehm_explicit_fail(EHM_E_INVALID, "audit: unknown mode %d", (int)o->mode);
    if (o->n < 0 || o->chunk < 0) return ehm_explicit_fail(EHM_E_INVALID, "audit: n, chunk < 0");
    if (o->n == 0) return EHM_OK;
    if (o->n_cells < 1 || o->n_cells > 0x7fffffffLL || !o->cell_vertices)
        return ehm_explicit_fail(EHM_E_INVALID, "audit: no cells (or more than 2^31 - 1)");
    if (o->mode == EHM_AUDIT_PER_LEAF) {
        if (o->k < 1) return ehm_explicit_fail(EHM_E_INVALID, "audit: per-leaf mode needs k >= 1");
        const uint64_t total = (uint64_t)o->n_cells * (uint64_t)o->k;
        if (o->first > total || (uint64_t)o->n > total - o->first)
            return ehm_explicit_fail(EHM_E_INVALID,
                                     "audit: per-leaf ids end at n_cells * k = %llu",
                                     (unsigned long long)total);
    } else {
        if (!o->cdf) return ehm_explicit_fail(EHM_E_INVALID, "audit: uniform mode needs cdf");
        const double total = o->cdf[o->n_cells - 1];
        if (!(total > 0.0) || !std::isfinite(total))
            return ehm_explicit_fail(EHM_E_INVALID, "audit: the cells have no volume");
    }
    if (audit) {
        if (!o->cell_node) return ehm_explicit_fail(EHM_E_INVALID, "audit: no cell_node");
        for (int64_t i = 0; i < o->n_cells; ++i)
            if (o->cell_node[i] < 0 || o->cell_node[i] >= v.n_nodes)
                return ehm_explicit_fail(EHM_E_INVALID, "audit: cell %lld names node %d",
                                         (long long)i, (int)o->cell_node[i]);
        if (!v.vcost || !v.nflags)
            return ehm_explicit_fail(EHM_E_INVALID, "audit: ehm_explicit_set_costs first");
        if (!(o->rtol >= 0.0)) return ehm_explicit_fail(EHM_E_INVALID, "audit: rtol < 0");
    }
    return EHM_OK;
}

// the cells on the device
struct Cells {
    DevBuf vert, cdf, node;
    int upload(const ehm_explicit_view& v, const ehm_audit_opts* o, bool audit) {
        ehm_err_channel& x_err = ehm_explicit_channel();
        const size_t nc = (size_t)o->n_cells;
        EHM_HIP_TRY(x_err, vert.upload(o->cell_vertices,
                                       nc * (size_t)(v.p + 1) * v.p * sizeof(double)));
        if (o->mode == EHM_AUDIT_UNIFORM)
            EHM_HIP_TRY(x_err, cdf.upload(o->cdf, nc * sizeof(double)));
        if (audit) EHM_HIP_TRY(x_err, node.upload(o->cell_node, nc * sizeof(int32_t)));
        return EHM_OK;
    }
};

void launch_sample(const ehm_explicit_view& v, const ehm_audit_opts* o, const Cells& C,
                   long long nc, uint64_t first, double* x, int32_t* cell) {
    ehm_audit_launch_sample(v.stream, nc, first, (int)o->mode, (int)o->k, o->seed, v.p,
                            (long long)o->n_cells, C.cdf.as<const double>(),
                            C.vert.as<const double>(), x, cell);
}

}  // namespace

void ehm_audit_launch_sample(hipStream_t stream, long long n, uint64_t first, int mode, int kper,
                             uint64_t seed, int p, long long n_cells, const double* cdf,
                             const double* V, double* X, int32_t* cell) {
    hipLaunchKernelGGL(k_audit_sample, dim3(blocks_of(n, EHM_AUDIT_BLOCK)), dim3(EHM_AUDIT_BLOCK),
                       0, stream, n, first, mode, kper, seed, p, n_cells, cdf, V, X, cell);
}

extern "C" {

int ehm_audit_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_audit_opts), (int64_t)sizeof(ehm_audit_result),
                           (int64_t)sizeof(ehm_audit_samples)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_explicit_sample(ehm_explicit* E, const ehm_audit_opts* o, double* x, int32_t* cell) {
    if (!E) return ehm_explicit_fail(EHM_E_INVALID, "sample: no handle");
    ehm_err_channel& x_err = ehm_explicit_channel();
    ehm_explicit_view v;
    ehm_explicit_get_view(E, &v);
    int rc = check_opts(v, o, false);
    if (rc || o->n == 0) return rc;
    EHM_HIP_TRY(x_err, hipSetDevice(v.device));
    Cells C;
    rc = C.upload(v, o, false);
    if (rc) return rc;
    const long long chunk = o->chunk > 0 ? o->chunk : 65536;
    const long long cap = std::min<long long>(chunk, o->n);
    DevBuf dx, dcell;
    EHM_HIP_TRY(x_err, dx.alloc((size_t)cap * v.p * sizeof(double)));
    EHM_HIP_TRY(x_err, dcell.alloc((size_t)cap * sizeof(int32_t)));
    for (long long off = 0; off < o->n; off += chunk) {
        const long long nc = std::min<long long>(chunk, o->n - off);
        launch_sample(v, o, C, nc, o->first + (uint64_t)off, dx.as<double>(),
                      dcell.as<int32_t>());
        EHM_HIP_TRY(x_err, hipGetLastError());
        if (x)
            EHM_HIP_TRY(x_err, hipMemcpyAsync(x + (size_t)off * v.p, dx.ptr,
                                              (size_t)nc * v.p * sizeof(double),
                                              hipMemcpyDeviceToHost, v.stream));
        if (cell)
            EHM_HIP_TRY(x_err, hipMemcpyAsync(cell + off, dcell.ptr, (size_t)nc * sizeof(int32_t),
                                              hipMemcpyDeviceToHost, v.stream));
        EHM_HIP_TRY(x_err, hipStreamSynchronize(v.stream));
    }
    return EHM_OK;
}

int ehm_explicit_audit(ehm_explicit* E, ehm_problem* prob, const ehm_audit_opts* o,
                       ehm_audit_result* res, const ehm_audit_samples* smp) {
    if (!E || !prob || !res) return ehm_explicit_fail(EHM_E_INVALID, "audit: bad argument");
    ehm_err_channel& x_err = ehm_explicit_channel();
    ehm_explicit_view v;
    ehm_explicit_get_view(E, &v);
    int rc = check_opts(v, o, true);
    if (rc) return rc;
    std::memset(res, 0, sizeof *res);
    res->worst_id = -1;
    res->worst_leaf = res->worst_cell = -1;
    res->max_ratio = -INFINITY;
    res->worst_vbar = res->worst_vstar = res->worst_bound = NAN;
    for (double& c : res->worst_x) c = NAN;
    if (o->n == 0) return EHM_OK;
    EHM_HIP_TRY(x_err, hipSetDevice(v.device));
    const DevExplicit D{v.rec, v.child, v.vinput, v.rec_stride, v.p, v.n_u, v.n_roots, v.n_nodes};
    const int p = v.p;
    Cells C;
    rc = C.upload(v, o, true);
    if (rc) return rc;
    const long long chunk = o->chunk > 0 ? o->chunk : 65536;
    const size_t cap = (size_t)std::min<long long>(chunk, o->n);
    const unsigned max_blocks = blocks_of((long long)cap, EHM_AUDIT_BLOCK);
    DevBuf dx, dcell, dleaf, dvbar, dwmin, dclosed, dvstar, ddidx, dstatus, dcnt, dbr, dbi;
    EHM_HIP_TRY(x_err, dx.alloc(cap * p * sizeof(double)));
    EHM_HIP_TRY(x_err, dcell.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(x_err, dleaf.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(x_err, dvbar.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(x_err, dwmin.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(x_err, dclosed.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(x_err, dvstar.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(x_err, ddidx.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(x_err, dstatus.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(x_err, dcnt.alloc(EHM_AUDIT_COUNTERS * sizeof(unsigned long long)));
    EHM_HIP_TRY(x_err, dbr.alloc(max_blocks * sizeof(double)));
    EHM_HIP_TRY(x_err, dbi.alloc(max_blocks * sizeof(unsigned long long)));
    EHM_HIP_TRY(x_err, hipMemsetAsync(dcnt.ptr, 0, EHM_AUDIT_COUNTERS * sizeof(unsigned long long),
                                      v.stream));
    std::vector<double> hx(cap * p), hJ(cap), hbr(max_blocks);
    std::vector<int32_t> hdidx(cap);
    std::vector<unsigned long long> hbi(max_blocks);
    EventPair ev_s, ev_c, ev_r;
    unsigned long long best_id = EHM_AUDIT_NO_ID;
    double best_ratio = -INFINITY;
    for (long long off = 0; off < o->n; off += chunk) {
        const long long nc = std::min<long long>(chunk, o->n - off);
        const uint64_t first = o->first + (uint64_t)off;
        const unsigned nb = blocks_of(nc, EHM_AUDIT_BLOCK);
        (void)hipEventRecord(ev_s.e0, v.stream);
        launch_sample(v, o, C, nc, first, dx.as<double>(), dcell.as<int32_t>());
        (void)hipEventRecord(ev_s.e1, v.stream);
        (void)hipEventRecord(ev_c.e0, v.stream);
        hipLaunchKernelGGL(k_audit_cost, dim3(nb), dim3(EHM_AUDIT_BLOCK), 0, v.stream, D, nc,
                           dx.as<const double>(), v.nbr, v.vcost, v.nflags, dleaf.as<int32_t>(),
                           dvbar.as<double>(), dwmin.as<double>(), dclosed.as<int32_t>());
        (void)hipEventRecord(ev_c.e1, v.stream);
        EHM_HIP_TRY(x_err, hipGetLastError());
        EHM_HIP_TRY(x_err, hipMemcpyAsync(hx.data(), dx.ptr, (size_t)nc * p * sizeof(double),
                                          hipMemcpyDeviceToHost, v.stream));
        EHM_HIP_TRY(x_err, hipStreamSynchronize(v.stream));
        // V* and delta_idx: the entry point GpuProblem.solve_pt calls, on the problem's own stream
        // (and device)
        const auto t0 = std::chrono::steady_clock::now();
        rc = ehm_solve_pt_batch(prob, nc, hx.data(), hJ.data(), nullptr, hdidx.data());
        res->seconds[2] += wall_since(t0);
        if (rc) return ehm_explicit_fail(rc, "audit: ehm_solve_pt_batch: %s", ehm_last_error());
        EHM_HIP_TRY(x_err, hipSetDevice(v.device));
        EHM_HIP_TRY(x_err, hipMemcpyAsync(dvstar.ptr, hJ.data(), (size_t)nc * sizeof(double),
                                          hipMemcpyHostToDevice, v.stream));
        EHM_HIP_TRY(x_err, hipMemcpyAsync(ddidx.ptr, hdidx.data(), (size_t)nc * sizeof(int32_t),
                                          hipMemcpyHostToDevice, v.stream));
        (void)hipEventRecord(ev_r.e0, v.stream);
        hipLaunchKernelGGL(k_audit_reduce, dim3(nb), dim3(EHM_AUDIT_BLOCK), 0, v.stream, nc, first,
                           dvbar.as<const double>(), dvstar.as<const double>(),
                           ddidx.as<const int32_t>(), dclosed.as<const int32_t>(),
                           dleaf.as<const int32_t>(), dcell.as<const int32_t>(),
                           C.node.as<const int32_t>(), o->eps_a, o->eps_r, o->rtol,
                           dstatus.as<int32_t>(), dcnt.as<unsigned long long>(), dbr.as<double>(),
                           dbi.as<unsigned long long>());
        (void)hipEventRecord(ev_r.e1, v.stream);
        EHM_HIP_TRY(x_err, hipGetLastError());
        EHM_HIP_TRY(x_err, hipMemcpyAsync(hbr.data(), dbr.ptr, nb * sizeof(double),
                                          hipMemcpyDeviceToHost, v.stream));
        EHM_HIP_TRY(x_err, hipMemcpyAsync(hbi.data(), dbi.ptr, nb * sizeof(unsigned long long),
                                          hipMemcpyDeviceToHost, v.stream));
        if (smp) {
            const size_t o8 = (size_t)off * sizeof(double), o4 = (size_t)off * sizeof(int32_t);
            const size_t n8 = (size_t)nc * sizeof(double), n4 = (size_t)nc * sizeof(int32_t);
            if (smp->x) std::memcpy(smp->x + (size_t)off * p, hx.data(), n8 * p);
            if (smp->vstar) std::memcpy(smp->vstar + off, hJ.data(), n8);
            if (smp->delta_idx) std::memcpy(smp->delta_idx + off, hdidx.data(), n4);
            struct { void* dst; const DevBuf* src; size_t at, bytes; } back[] = {
                {smp->cell, &dcell, o4, n4},     {smp->leaf, &dleaf, o4, n4},
                {smp->vbar, &dvbar, o8, n8},     {smp->wmin, &dwmin, o8, n8},
                {smp->status, &dstatus, o4, n4}};
            for (const auto& b : back)
                if (b.dst)
                    EHM_HIP_TRY(x_err, hipMemcpyAsync((char*)b.dst + b.at, b.src->ptr, b.bytes,
                                                      hipMemcpyDeviceToHost, v.stream));
        }
        EHM_HIP_TRY(x_err, hipStreamSynchronize(v.stream));
        double s = 0.0;
        ev_s.seconds(&s);
        res->seconds[0] += s;
        ev_c.seconds(&s);
        res->seconds[1] += s;
        ev_r.seconds(&s);
        res->seconds[1] += s;
        // merge the workgroups' worst samples; fetch the record of a new overall worst
        if (ehm_verdict::merge_block_worst(hbr.data(), hbi.data(), nb, EHM_AUDIT_NO_ID,
                                           ehm_verdict::ratio_beats, best_ratio, best_id)) {
            const size_t q = (size_t)(best_id - first);
            int32_t lf = -1, cl = -1;
            double vb = NAN;
            EHM_HIP_TRY(x_err, hipMemcpy(&lf, dleaf.as<int32_t>() + q, sizeof lf,
                                         hipMemcpyDeviceToHost));
            EHM_HIP_TRY(x_err, hipMemcpy(&cl, dcell.as<int32_t>() + q, sizeof cl,
                                         hipMemcpyDeviceToHost));
            EHM_HIP_TRY(x_err, hipMemcpy(&vb, dvbar.as<double>() + q, sizeof vb,
                                         hipMemcpyDeviceToHost));
            res->worst_id = (int64_t)best_id;
            res->worst_leaf = lf;
            res->worst_cell = cl;
            res->max_ratio = best_ratio;
            res->worst_vbar = vb;
            res->worst_vstar = hJ[q];
            res->worst_bound = std::max(o->eps_a, o->eps_r * hJ[q]);
            for (int c = 0; c < p; ++c) res->worst_x[c] = hx[q * p + c];
        }
    }
    unsigned long long cnt[EHM_AUDIT_COUNTERS];
    EHM_HIP_TRY(x_err, hipMemcpy(cnt, dcnt.ptr, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) res->counts[i] = (int64_t)cnt[i];
    res->relocated = (int64_t)cnt[5];
    for (int i = 0; i < EHM_AUDIT_BINS; ++i) res->histogram[i] = (int64_t)cnt[6 + i];
    return EHM_OK;
}

}  // extern "C"
