// What ehm_cost.hip checks and derives without a device: the options, the domain
// and the start set as masks and as ascending rows, caller-supplied weights, the byte cap of the
// paths, the target a domain row leaves the domain by, the order-preserving key the per-step maxima
// and minima are reduced in, and the walk of the args into a path.  The relation itself is checked
// by check_csr of ehm_reach_host.h.  Plain C++ on the error channel of ehm_err.h;
// tests/native/cost_host_main.cpp drives it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_err.h"
#include "ehm_reach_host.h"

#if defined(__HIPCC__)
#define EHM_COST_HD __host__ __device__ __forceinline__
#else
#define EHM_COST_HD inline
#endif

namespace ehm_cost {

constexpr int64_t MAX_PATH_BYTES = (int64_t)1 << 28;    // horizon n_leaf 4, per direction
constexpr int MAX_NU = 4;                               // EHM_R_MAX_NU

// An order-preserving map of the doubles that are no NaN into 64-bit unsigned keys: a < b as
// numbers gives key(a) < key(b), and -0 sorts below +0.  The maximum and minimum of a step are
// taken on the keys with integer atomics, so they do not depend on the order.
EHM_COST_HD uint64_t key_of(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
EHM_COST_HD double value_of(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

// The options that are no array: n_leaf against the law's, the inputs, the horizon, both weights
// or neither, the bytes of the args behind the paths.
inline int check_options(ehm_err_channel& err, const ehm_cost_opts* o, int64_t law_leaves,
                         int n_u) {
    if (o->n_leaf < 1 || o->n_leaf > law_leaves)
        return err.fail(EHM_E_INVALID, "cost: n_leaf = %lld of %lld leaves", (long long)o->n_leaf,
                        (long long)law_leaves);
    if (n_u < 1 || n_u > MAX_NU)
        return err.fail(EHM_E_INVALID, "cost: n_u = %d, at most %d inputs", n_u, MAX_NU);
    if (o->horizon < 1)
        return err.fail(EHM_E_INVALID, "cost: horizon = %d < 1", (int)o->horizon);
    if ((o->w_hi == nullptr) != (o->w_lo == nullptr))
        return err.fail(EHM_E_INVALID, "cost: w_hi and w_lo come together or not at all");
    if (o->want_paths && (int64_t)o->horizon > MAX_PATH_BYTES / 4 / o->n_leaf)
        return err.fail(EHM_E_INVALID,
                        "cost: the paths of horizon %d over %lld leaves need more than 2^28 bytes "
                        "per direction",
                        (int)o->horizon, (long long)o->n_leaf);
    return EHM_OK;
}

// `what` ("domain" or "start") as a mask [n] and as ascending distinct rows: nonempty, every row in
// range; a row named twice is one row.
inline int rows_of(ehm_err_channel& err, const char* what, const int32_t* rows, int64_t n_rows,
                   int64_t n, std::vector<uint8_t>& mask, std::vector<int32_t>& sorted) {
    if (n_rows < 1) return err.fail(EHM_E_INVALID, "cost: the %s set is empty", what);
    mask.assign((size_t)n, 0);
    for (int64_t k = 0; k < n_rows; ++k) {
        const int32_t l = rows[k];
        if (l < 0 || l >= n)
            return err.fail(EHM_E_INVALID, "cost: %s[%lld] = %d of %lld leaves", what, (long long)k,
                            (int)l, (long long)n);
        mask[(size_t)l] = 1;
    }
    sorted.clear();
    for (int64_t l = 0; l < n; ++l)
        if (mask[(size_t)l]) sorted.push_back((int32_t)l);
    return EHM_OK;
}

// The start set lies in the domain.
inline int check_subset(ehm_err_channel& err, const std::vector<int32_t>& start,
                        const std::vector<uint8_t>& domain) {
    for (const int32_t l : start)
        if (!domain[(size_t)l])
            return err.fail(EHM_E_INVALID, "cost: start row %d is not in the domain", (int)l);
    return EHM_OK;
}

// Caller-supplied weights on the domain: finite, w_lo <= w_hi.
inline int check_weights(ehm_err_channel& err, const double* w_hi, const double* w_lo,
                         const std::vector<int32_t>& domain) {
    for (const int32_t l : domain) {
        if (!std::isfinite(w_hi[l]) || !std::isfinite(w_lo[l]))
            return err.fail(EHM_E_INVALID, "cost: the weights of row %d are [%g, %g], not finite",
                            (int)l, w_lo[l], w_hi[l]);
        if (w_lo[l] > w_hi[l])
            return err.fail(EHM_E_INVALID, "cost: w_lo = %g > w_hi = %g on row %d", w_lo[l],
                            w_hi[l], (int)l);
    }
    return EHM_OK;
}

// The smallest target of `row` outside the domain, -1 when the row stays in it.
inline int32_t first_outside(const int32_t* ptr32, const int32_t* indices, int64_t row,
                             const std::vector<uint8_t>& domain) {
    int32_t t = -1;
    for (int32_t e = ptr32[row]; e < ptr32[row + 1]; ++e)
        if (!domain[(size_t)indices[e]] && (t < 0 || indices[e] < t)) t = indices[e];
    return t;
}

// What the device's check of the domain found: `row` is its smallest row that is a seed or leaves
// the domain (n_leaf or more: none).
inline int domain_verdict(ehm_err_channel& err, int64_t row, int64_t n, const int32_t* level,
                          const int32_t* ptr32, const int32_t* indices,
                          const std::vector<uint8_t>& domain) {
    if (row < 0 || row >= n) return EHM_OK;
    if (level[row] == 0)
        return err.fail(EHM_E_INVALID, "cost: row %lld is a seed", (long long)row);
    return err.fail(EHM_E_INVALID, "cost: row %lld of the domain reaches leaf %d outside it",
                    (long long)row, (int)first_outside(ptr32, indices, row, domain));
}

// The smallest row of `rows` (ascending) whose value is `target`, -1 without one.
inline int32_t first_attaining(const double* value, const std::vector<int32_t>& rows,
                               double target) {
    for (const int32_t l : rows)
        if (value[l] == target) return l;
    return -1;
}

// path [horizon + 1] from `first`: path[t + 1] = arg[horizon - 1 - t][path[t]], arg [horizon][n] the
// args of the sweeps in the order they were made; -1 from the first empty row on.
inline void walk_path(const int32_t* arg, int64_t n, int32_t horizon, int32_t first,
                      int32_t* path) {
    path[0] = first;
    for (int32_t t = 0; t < horizon; ++t)
        path[t + 1] = path[t] < 0 ? -1 : arg[(size_t)(horizon - 1 - t) * (size_t)n + path[t]];
}

}  // namespace ehm_cost
