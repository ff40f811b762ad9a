// Audit of a law by the cost of the input it applies: at every sample x
// the law's input ubar is priced by the fixed-first-input problem -- P_theta with u_0 = ubar, again
// a canonical form, with the columns of u_0 moved to the parameters -- against V* = P_theta(x).
//
//   k_audit_sample    (ehm_audit.hip, through ehm_audit_sample.h) the points, uniform in the roots
//   k_applied_pack    one thread per sample: theta' = (x, ubar), the cost constant, the flag of an
//                     input that is not finite (pack_applied_row of ehm_verdict.h)
//   k_applied_reduce  V_u = optimum + constant, statuses, counts and the histogram by integer
//                     atomics, the worst sample per workgroup (the host merges, ties to the smaller
//                     id): the rules and the tree of ehm_verdict.h
//
// The input is the law's own: ehm_compiled_eval_batch (double and single laws) or
// ehm_explicit_eval_batch, so (u, leaf) are `evaluate` bit for bit.  Both optima come from
// ehm_solve_pt_batch; V_u from the exact substitution, and only where no commutation of it is
// feasible from the problem widened by input_tol (opts->relaxed).  A chunk's points, inputs and
// optima make their round trips through the host, which the two LP batches dwarf.  Every operation
// a result depends on runs under fp contract(off) in a fixed order (tests/applied_cpu.py is the
// numpy mirror); no floating-point sum is reduced across samples.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_audit_sample.h"
#include "ehm_explicit_view.h"
#include "ehm_host.h"
#include "ehm_verdict.h"

#define EHM_APPLIED_BLOCK 256
#define EHM_APPLIED_BINS EHM_VERDICT_BINS
// counters of a run: [0..5] statuses, [6..38] histogram
#define EHM_APPLIED_COUNTERS (6 + EHM_APPLIED_BINS)
#define EHM_APPLIED_NO_ID 0xffffffffffffffffULL

namespace {

__global__ void k_applied_pack(long long n, int p, int n_u, const double* __restrict__ X,
                               const double* __restrict__ U, const double* __restrict__ cost_u,
                               double* __restrict__ theta, double* __restrict__ konst,
                               int32_t* __restrict__ no_law) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const bool bad = ehm_verdict::pack_applied_row(
        p, n_u, [&](int c) { return X[q * p + c]; }, [&](int j) { return U[q * n_u + j]; }, cost_u,
        theta + (size_t)q * (p + n_u), &konst[q]);
    no_law[q] = bad;
}

__global__ __launch_bounds__(EHM_APPLIED_BLOCK) void k_applied_reduce(
    long long n, uint64_t first, const double* __restrict__ ju, const double* __restrict__ konst,
    const double* __restrict__ vstar, const int32_t* __restrict__ didx,
    const int32_t* __restrict__ didx_u, const int32_t* __restrict__ no_law, double eps_a,
    double eps_r, double rtol, double* __restrict__ vu, int32_t* __restrict__ status,
    unsigned long long* __restrict__ counters, double* __restrict__ blk_ratio,
    unsigned long long* __restrict__ blk_id) {
#pragma clang fp contract(off)
    __shared__ unsigned int cnt[EHM_APPLIED_COUNTERS];
    ehm_verdict::counters_zero<EHM_APPLIED_BLOCK, EHM_APPLIED_COUNTERS>(cnt);
    __syncthreads();
    const long long q = (long long)blockIdx.x * EHM_APPLIED_BLOCK + threadIdx.x;
    double ratio = -INFINITY;
    unsigned long long id = EHM_APPLIED_NO_ID;
    if (q < n) {
        const double vs = vstar[q];
        const double v = ju[q] + konst[q];
        const double gap = v - vs;
        const double bound = ehm_verdict::bound_of(eps_a, eps_r, vs);
        int st;
        if (didx[q] < 0) st = 5;
        else if (no_law[q]) st = 4;
        else if (didx_u[q] < 0) st = 3;
        else st = ehm_verdict::gap_status(gap, bound, ehm_verdict::slack_of(rtol, vs));
        vu[q] = v;
        status[q] = st;
        atomicAdd(&cnt[st], 1u);
        if (st <= 2) {
            const double r = ehm_verdict::ratio_of(gap, bound);
            atomicAdd(&cnt[6 + ehm_verdict::ratio_bin(r)], 1u);
            if (ehm_verdict::ratio_is_candidate(r)) {
                ratio = r;
                id = first + (unsigned long long)q;
            }
        }
    }
    ehm_verdict::block_worst<EHM_APPLIED_BLOCK>(
        ratio, id,
        [](double ra, unsigned long long ia, double rb, unsigned long long ib) {
            return ehm_verdict::ratio_beats(ra, ia, rb, ib);
        },
        [](unsigned long long i) { return i != EHM_APPLIED_NO_ID; });
    if (threadIdx.x == 0) {
        blk_ratio[blockIdx.x] = ratio;
        blk_id[blockIdx.x] = id;
    }
    ehm_verdict::counters_flush<EHM_APPLIED_BLOCK, EHM_APPLIED_COUNTERS>(cnt, counters);
}

thread_local ehm_err_channel a_err;

int check_opts(const ehm_compiled* law, const ehm_applied_opts* o) {
    if (!o) return a_err.fail(EHM_E_INVALID, "applied audit: no options");
    if (o->n < 0 || o->chunk < 0) return a_err.fail(EHM_E_INVALID, "applied audit: n, chunk < 0");
    if (o->p < 1 || o->n_u < 1 || o->p + o->n_u > EHM_MAX_P)
        return a_err.fail(EHM_E_INVALID, "applied audit: p = %d, n_u = %d: p + n_u must be <= %d",
                          (int)o->p, (int)o->n_u, EHM_MAX_P);
    if (!o->cost_u) return a_err.fail(EHM_E_INVALID, "applied audit: no cost_u");
    if (!(o->rtol >= 0.0)) return a_err.fail(EHM_E_INVALID, "applied audit: rtol < 0");
    if (law) {
        int64_t info[14];
        if (ehm_compiled_info(law, info) != EHM_OK)
            return a_err.fail(EHM_E_INVALID, "applied audit: %s", ehm_compiled_last_error());
        if (info[1] != o->p || info[2] != o->n_u)
            return a_err.fail(EHM_E_INVALID, "applied audit: the law has p = %lld, n_u = %lld, the "
                              "options %d, %d", (long long)info[1], (long long)info[2], (int)o->p,
                              (int)o->n_u);
        if (info[6] > 0)
            return a_err.fail(EHM_E_INVALID, "applied audit: the law has %lld test nodes (children "
                              "that are no bisection); its roots do not tile the set -- compile it "
                              "with the spine as its root table", (long long)info[6]);
    } else if (o->source) {
        ehm_explicit_view v;
        ehm_explicit_get_view(o->source, &v);
        if (v.p != o->p || v.n_u != o->n_u)
            return a_err.fail(EHM_E_INVALID, "applied audit: the source law has p = %d, n_u = %d, "
                              "the options %d, %d", v.p, v.n_u, (int)o->p, (int)o->n_u);
    } else if (!o->u && o->n > 0) {
        return a_err.fail(EHM_E_INVALID, "applied audit: no law, no source and no inputs");
    }
    if (!o->x && o->n > 0) {
        if (o->n_cells < 1 || o->n_cells > 0x7fffffffLL || !o->cell_vertices || !o->cdf)
            return a_err.fail(EHM_E_INVALID, "applied audit: no points and no cells to draw them "
                              "in");
        const double total = o->cdf[o->n_cells - 1];
        if (!(total > 0.0) || !std::isfinite(total))
            return a_err.fail(EHM_E_INVALID, "applied audit: the cells have no volume");
    }
    return EHM_OK;
}

}  // namespace

extern "C" {

const char* ehm_applied_last_error(void) { return a_err.c_str(); }

int ehm_applied_abi_sizes(int64_t* sizes, int32_t n) {
    const int64_t all[] = {(int64_t)sizeof(ehm_applied_opts), (int64_t)sizeof(ehm_applied_result),
                           (int64_t)sizeof(ehm_applied_samples)};
    return ehm_copy_abi_sizes(all, (int32_t)(sizeof all / sizeof all[0]), sizes, n);
}

int ehm_compiled_audit(ehm_compiled* law, ehm_problem* oracle, ehm_problem* applied,
                       const ehm_applied_opts* o, ehm_applied_result* res,
                       const ehm_applied_samples* smp) {
    if (!oracle || !applied || !res) return a_err.fail(EHM_E_INVALID, "applied audit: bad "
                                                       "argument");
    int rc = check_opts(law, o);
    if (rc) return rc;
    std::memset(res, 0, sizeof *res);
    res->worst_id = -1;
    res->worst_leaf = -1;
    res->max_ratio = -INFINITY;
    res->worst_vu = res->worst_vstar = res->worst_bound = NAN;
    for (double& c : res->worst_x) c = NAN;
    for (double& c : res->worst_u) c = NAN;
    if (o->n == 0) return EHM_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || o->device < 0 || o->device >= ndev)
        return a_err.fail(EHM_E_NO_DEVICE, "no HIP device %d (libehmpc has no CPU fallback)",
                          (int)o->device);
    EHM_HIP_TRY(a_err, hipSetDevice(o->device));
    const int p = o->p, n_u = o->n_u, pp = p + n_u;
    const bool draw = o->x == nullptr;
    Stream stream;
    EHM_HIP_TRY(a_err, stream.create());
    DevBuf cvert, ccdf, dcost;
    if (draw) {
        EHM_HIP_TRY(a_err, cvert.upload(o->cell_vertices,
                                        (size_t)o->n_cells * (size_t)(p + 1) * p * sizeof(double)));
        EHM_HIP_TRY(a_err, ccdf.upload(o->cdf, (size_t)o->n_cells * sizeof(double)));
    }
    EHM_HIP_TRY(a_err, dcost.upload(o->cost_u, (size_t)n_u * sizeof(double)));
    const long long chunk = o->chunk > 0 ? o->chunk : 65536;
    const size_t cap = (size_t)std::min<long long>(chunk, o->n);
    const unsigned max_blocks = blocks_of((long long)cap, EHM_APPLIED_BLOCK);
    DevBuf dx, dcell, du, dtheta, dkonst, dflag, dju, dvstar, ddidx, ddidxu, dvu, dstatus, dcnt,
        dbr, dbi;
    EHM_HIP_TRY(a_err, dx.alloc(cap * p * sizeof(double)));
    EHM_HIP_TRY(a_err, dcell.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(a_err, du.alloc(cap * n_u * sizeof(double)));
    EHM_HIP_TRY(a_err, dtheta.alloc(cap * pp * sizeof(double)));
    EHM_HIP_TRY(a_err, dkonst.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(a_err, dflag.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(a_err, dju.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(a_err, dvstar.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(a_err, ddidx.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(a_err, ddidxu.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(a_err, dvu.alloc(cap * sizeof(double)));
    EHM_HIP_TRY(a_err, dstatus.alloc(cap * sizeof(int32_t)));
    EHM_HIP_TRY(a_err, dcnt.alloc(EHM_APPLIED_COUNTERS * sizeof(unsigned long long)));
    EHM_HIP_TRY(a_err, dbr.alloc(max_blocks * sizeof(double)));
    EHM_HIP_TRY(a_err, dbi.alloc(max_blocks * sizeof(unsigned long long)));
    EHM_HIP_TRY(a_err, hipMemsetAsync(dcnt.ptr, 0,
                                      EHM_APPLIED_COUNTERS * sizeof(unsigned long long), stream));
    std::vector<double> hx(draw ? cap * p : 0), hu(o->u && !law && !o->source ? 0 : cap * n_u),
        htheta(cap * pp), hJ(cap), hJu(cap), hvu(cap), hbr(max_blocks);
    std::vector<int32_t> hcell(cap, -1), hleaf(cap, -1), hdidx(cap), hdidxu(cap), hrelaxed(cap, 0);
    std::vector<long long> again;           // the samples solved again on opts->relaxed
    std::vector<double> tsub, jsub;
    std::vector<int32_t> dsub;
    std::vector<unsigned long long> hbi(max_blocks);
    EventPair ev_s, ev_p, ev_r;
    unsigned long long best_id = EHM_APPLIED_NO_ID;
    double best_ratio = -INFINITY;
    for (long long off = 0; off < o->n; off += chunk) {
        const long long nc = std::min<long long>(chunk, o->n - off);
        const uint64_t first = o->first + (uint64_t)off;
        const unsigned nb = blocks_of(nc, EHM_APPLIED_BLOCK);
        // the points
        const double* xs = draw ? hx.data() : o->x + (size_t)off * p;
        if (draw) {
            (void)hipEventRecord(ev_s.e0, stream);
            ehm_audit_launch_sample(stream, nc, first, EHM_AUDIT_UNIFORM, 0, o->seed, p,
                                    (long long)o->n_cells, ccdf.as<const double>(),
                                    cvert.as<const double>(), dx.as<double>(),
                                    dcell.as<int32_t>());
            (void)hipEventRecord(ev_s.e1, stream);
            EHM_HIP_TRY(a_err, hipGetLastError());
            EHM_HIP_TRY(a_err, hipMemcpyAsync(hx.data(), dx.ptr, (size_t)nc * p * sizeof(double),
                                              hipMemcpyDeviceToHost, stream));
            EHM_HIP_TRY(a_err, hipMemcpyAsync(hcell.data(), dcell.ptr, (size_t)nc * sizeof(int32_t),
                                              hipMemcpyDeviceToHost, stream));
            EHM_HIP_TRY(a_err, hipStreamSynchronize(stream));
            double s = 0.0;
            ev_s.seconds(&s);
            res->seconds[0] += s;
        } else {
            EHM_HIP_TRY(a_err, hipMemcpyAsync(dx.ptr, xs, (size_t)nc * p * sizeof(double),
                                              hipMemcpyHostToDevice, stream));
        }
        // the input the law applies there: the law's own entry point
        const double* us = hu.data();
        if (law) {
            double s = 0.0;
            rc = ehm_compiled_eval_batch(law, nc, xs, hu.data(), hleaf.data(), nullptr, &s);
            if (rc) return a_err.fail(rc, "applied audit: ehm_compiled_eval_batch: %s",
                                      ehm_compiled_last_error());
            res->seconds[1] += s;
        } else if (o->source) {
            double s = 0.0;
            rc = ehm_explicit_eval_batch(o->source, nc, xs, hu.data(), hleaf.data(), nullptr, &s);
            if (rc) return a_err.fail(rc, "applied audit: ehm_explicit_eval_batch: %s",
                                      ehm_explicit_last_error());
            res->seconds[1] += s;
        } else {
            us = o->u + (size_t)off * n_u;
        }
        EHM_HIP_TRY(a_err, hipSetDevice(o->device));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(du.ptr, us, (size_t)nc * n_u * sizeof(double),
                                          hipMemcpyHostToDevice, stream));
        (void)hipEventRecord(ev_p.e0, stream);
        hipLaunchKernelGGL(k_applied_pack, dim3(nb), dim3(EHM_APPLIED_BLOCK), 0, stream, nc, p, n_u,
                           dx.as<const double>(), du.as<const double>(),
                           dcost.as<const double>(), dtheta.as<double>(), dkonst.as<double>(),
                           dflag.as<int32_t>());
        (void)hipEventRecord(ev_p.e1, stream);
        EHM_HIP_TRY(a_err, hipGetLastError());
        EHM_HIP_TRY(a_err, hipMemcpyAsync(htheta.data(), dtheta.ptr,
                                          (size_t)nc * pp * sizeof(double), hipMemcpyDeviceToHost,
                                          stream));
        EHM_HIP_TRY(a_err, hipStreamSynchronize(stream));
        // V* and V_u: the entry point GpuProblem.solve_pt calls, each on its problem's own stream
        auto t0 = std::chrono::steady_clock::now();
        rc = ehm_solve_pt_batch(oracle, nc, xs, hJ.data(), nullptr, hdidx.data());
        res->seconds[3] += wall_since(t0);
        if (rc) return a_err.fail(rc, "applied audit: ehm_solve_pt_batch (oracle): %s",
                                  ehm_last_error());
        t0 = std::chrono::steady_clock::now();
        rc = ehm_solve_pt_batch(applied, nc, htheta.data(), hJu.data(), nullptr, hdidxu.data());
        if (rc) return a_err.fail(rc, "applied audit: ehm_solve_pt_batch (applied): %s",
                                  ehm_last_error());
        // an input that is not admissible as it stands: once more on the widened problem
        std::fill(hrelaxed.begin(), hrelaxed.begin() + nc, 0);
        if (o->relaxed) {
            again.clear();
            for (long long q = 0; q < nc; ++q)
                if (hdidx[q] >= 0 && hdidxu[q] < 0) again.push_back(q);
            if (!again.empty()) {
                const size_t na = again.size();
                tsub.resize(na * pp);
                jsub.resize(na);
                dsub.resize(na);
                for (size_t a = 0; a < na; ++a)
                    std::memcpy(&tsub[a * pp], &htheta[(size_t)again[a] * pp],
                                pp * sizeof(double));
                rc = ehm_solve_pt_batch(o->relaxed, (int64_t)na, tsub.data(), jsub.data(), nullptr,
                                        dsub.data());
                if (rc) return a_err.fail(rc, "applied audit: ehm_solve_pt_batch (relaxed): %s",
                                          ehm_last_error());
                for (size_t a = 0; a < na; ++a)
                    if (dsub[a] >= 0) {
                        hJu[again[a]] = jsub[a];
                        hdidxu[again[a]] = dsub[a];
                        hrelaxed[again[a]] = 1;
                        res->relaxed += 1;
                    }
            }
        }
        res->seconds[4] += wall_since(t0);
        EHM_HIP_TRY(a_err, hipSetDevice(o->device));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(dvstar.ptr, hJ.data(), (size_t)nc * sizeof(double),
                                          hipMemcpyHostToDevice, stream));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(ddidx.ptr, hdidx.data(), (size_t)nc * sizeof(int32_t),
                                          hipMemcpyHostToDevice, stream));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(dju.ptr, hJu.data(), (size_t)nc * sizeof(double),
                                          hipMemcpyHostToDevice, stream));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(ddidxu.ptr, hdidxu.data(), (size_t)nc * sizeof(int32_t),
                                          hipMemcpyHostToDevice, stream));
        (void)hipEventRecord(ev_r.e0, stream);
        hipLaunchKernelGGL(k_applied_reduce, dim3(nb), dim3(EHM_APPLIED_BLOCK), 0, stream, nc,
                           first,
                           dju.as<const double>(), dkonst.as<const double>(),
                           dvstar.as<const double>(), ddidx.as<const int32_t>(),
                           ddidxu.as<const int32_t>(), dflag.as<const int32_t>(), o->eps_a,
                           o->eps_r, o->rtol, dvu.as<double>(), dstatus.as<int32_t>(),
                           dcnt.as<unsigned long long>(), dbr.as<double>(),
                           dbi.as<unsigned long long>());
        (void)hipEventRecord(ev_r.e1, stream);
        EHM_HIP_TRY(a_err, hipGetLastError());
        EHM_HIP_TRY(a_err, hipMemcpyAsync(hbr.data(), dbr.ptr, nb * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(hbi.data(), dbi.ptr, nb * sizeof(unsigned long long),
                                          hipMemcpyDeviceToHost, stream));
        EHM_HIP_TRY(a_err, hipMemcpyAsync(hvu.data(), dvu.ptr, (size_t)nc * sizeof(double),
                                          hipMemcpyDeviceToHost, stream));
        if (smp && smp->status)
            EHM_HIP_TRY(a_err, hipMemcpyAsync(smp->status + off, dstatus.ptr,
                                              (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost,
                                              stream));
        EHM_HIP_TRY(a_err, hipStreamSynchronize(stream));
        if (smp) {
            const size_t n8 = (size_t)nc * sizeof(double), n4 = (size_t)nc * sizeof(int32_t);
            if (smp->x) std::memcpy(smp->x + (size_t)off * p, xs, n8 * p);
            if (smp->u) std::memcpy(smp->u + (size_t)off * n_u, us, n8 * n_u);
            if (smp->root) std::memcpy(smp->root + off, hcell.data(), n4);
            if (smp->leaf) std::memcpy(smp->leaf + off, hleaf.data(), n4);
            if (smp->vu) std::memcpy(smp->vu + off, hvu.data(), n8);
            if (smp->vstar) std::memcpy(smp->vstar + off, hJ.data(), n8);
            if (smp->delta_idx) std::memcpy(smp->delta_idx + off, hdidx.data(), n4);
            if (smp->delta_idx_applied)
                std::memcpy(smp->delta_idx_applied + off, hdidxu.data(), n4);
            if (smp->relaxed) std::memcpy(smp->relaxed + off, hrelaxed.data(), n4);
        }
        double s = 0.0;
        ev_p.seconds(&s);
        res->seconds[2] += s;
        ev_r.seconds(&s);
        res->seconds[2] += s;
        // merge the workgroups' worst samples
        if (ehm_verdict::merge_block_worst(hbr.data(), hbi.data(), nb, EHM_APPLIED_NO_ID,
                                           ehm_verdict::ratio_beats, best_ratio, best_id)) {
            const size_t q = (size_t)(best_id - first);
            res->worst_id = (int64_t)best_id;
            res->worst_leaf = hleaf[q];
            res->max_ratio = best_ratio;
            res->worst_vu = hvu[q];
            res->worst_vstar = hJ[q];
            res->worst_bound = std::max(o->eps_a, o->eps_r * hJ[q]);
            for (int c = 0; c < p; ++c) res->worst_x[c] = xs[q * p + c];
            for (int c = 0; c < n_u; ++c) res->worst_u[c] = us[q * n_u + c];
        }
    }
    unsigned long long cnt[EHM_APPLIED_COUNTERS];
    EHM_HIP_TRY(a_err, hipMemcpy(cnt, dcnt.ptr, sizeof cnt, hipMemcpyDeviceToHost));
    for (int i = 0; i < 6; ++i) res->counts[i] = (int64_t)cnt[i];
    for (int i = 0; i < EHM_APPLIED_BINS; ++i) res->histogram[i] = (int64_t)cnt[6 + i];
    return EHM_OK;
}

}  // extern "C"
