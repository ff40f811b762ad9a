// What ehm_reach.hip checks and derives without a device: the relation it is handed
// (a CSR over the first n_leaf leaf records), the options, the narrowing of indptr to the 32 bits the
// kernels read, the start mask, and what the host reads off the per-step counters at the end.  Plain
// C++ on the error channel of ehm_err.h; tests/native/reach_host_main.cpp drives it under the address
// and undefined-behaviour sanitizers.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_err.h"

namespace ehm_reach {

constexpr int64_t MAX_STEP_BYTES = (int64_t)1 << 28;    // (horizon + 1) n_leaf with want_steps

// The options that are no array: n_leaf against the law's, horizon, max_sweeps, row_map, the bytes
// of the step sets.
inline int check_options(ehm_err_channel& err, const ehm_reach_opts* o, int64_t law_leaves) {
    if (o->n_leaf < 1 || o->n_leaf > law_leaves)
        return err.fail(EHM_E_INVALID, "reach: n_leaf = %lld of %lld leaves", (long long)o->n_leaf,
                        (long long)law_leaves);
    if (o->horizon < 0)
        return err.fail(EHM_E_INVALID, "reach: horizon = %d < 0", (int)o->horizon);
    if (o->max_sweeps < 1)
        return err.fail(EHM_E_INVALID, "reach: max_sweeps = %lld < 1", (long long)o->max_sweeps);
    if (o->row_map != EHM_REACH_MAP_THREAD && o->row_map != EHM_REACH_MAP_WAVE)
        return err.fail(EHM_E_INVALID, "reach: row_map = %d", (int)o->row_map);
    if (o->want_steps && ((int64_t)o->horizon + 1) > MAX_STEP_BYTES / o->n_leaf)
        return err.fail(EHM_E_INVALID,
                        "reach: the step sets of horizon %d over %lld leaves need more than 2^28 "
                        "bytes",
                        (int)o->horizon, (long long)o->n_leaf);
    return EHM_OK;
}

// A relation as CSR over n leaves: indptr[0] = 0, nondecreasing, indptr[n] = n_edges < 2^31, every
// index in 0 .. n - 1, a level per leaf.  On success ptr32 [n + 1] is indptr in the 32 bits the
// kernels read.  `who` names the entry point (ehm_cost.hip checks its relation here too).
inline int check_csr(ehm_err_channel& err, const char* who, int64_t n, int64_t n_edges,
                     int64_t n_level, const int64_t* indptr, const int32_t* indices,
                     std::vector<int32_t>& ptr32) {
    if (n_edges < 0 || n_edges > 0x7fffffffLL)
        return err.fail(EHM_E_INVALID, "%s: n_edges = %lld (0 .. 2^31 - 1)", who,
                        (long long)n_edges);
    if (n_level != n)
        return err.fail(EHM_E_INVALID, "%s: a level array of %lld for %lld leaves", who,
                        (long long)n_level, (long long)n);
    if (indptr[0] != 0)
        return err.fail(EHM_E_INVALID, "%s: indptr[0] = %lld, not 0", who, (long long)indptr[0]);
    for (int64_t l = 0; l < n; ++l)
        if (indptr[l + 1] < indptr[l])
            return err.fail(EHM_E_INVALID, "%s: indptr decreases at row %lld (%lld after %lld)", who,
                            (long long)l, (long long)indptr[l + 1], (long long)indptr[l]);
    if (indptr[n] != n_edges)
        return err.fail(EHM_E_INVALID, "%s: indptr ends at %lld, n_edges is %lld", who,
                        (long long)indptr[n], (long long)n_edges);
    for (int64_t e = 0; e < n_edges; ++e)
        if (indices[e] < 0 || indices[e] >= n)
            return err.fail(EHM_E_INVALID, "%s: indices[%lld] = %d of %lld leaves", who,
                            (long long)e, (int)indices[e], (long long)n);
    ptr32.resize((size_t)n + 1);
    for (int64_t l = 0; l <= n; ++l) ptr32[(size_t)l] = (int32_t)indptr[l];
    return EHM_OK;
}

// The relation of a reach call.
inline int check_relation(ehm_err_channel& err, const ehm_reach_opts* o,
                          std::vector<int32_t>& ptr32) {
    return check_csr(err, "reach", o->n_leaf, o->n_edges, o->n_level, o->indptr, o->indices, ptr32);
}

// The start rows as a mask [n_leaf]: nonempty, every row in range; a row named twice is one row.
inline int start_mask(ehm_err_channel& err, const ehm_reach_opts* o, std::vector<uint8_t>& mask) {
    if (o->n_start < 1) return err.fail(EHM_E_INVALID, "reach: the start set is empty");
    mask.assign((size_t)o->n_leaf, 0);
    for (int64_t k = 0; k < o->n_start; ++k) {
        const int32_t l = o->start[k];
        if (l < 0 || l >= o->n_leaf)
            return err.fail(EHM_E_INVALID, "reach: start[%lld] = %d of %lld leaves", (long long)k,
                            (int)l, (long long)o->n_leaf);
        mask[(size_t)l] = 1;
    }
    return EHM_OK;
}

// Phase A from the per-sweep counters: fresh[k] leaves got arrival k in sweep k (k = 1 .. made; [0]
// is the start set's size).  done: some sweep reached nothing new; n_arrival: the last that did.
inline void arrival_outcome(const unsigned long long* fresh, int64_t made, bool& done,
                            int64_t& n_arrival) {
    done = false;
    n_arrival = 0;
    for (int64_t k = 1; k <= made; ++k) {
        if (fresh[k] == 0) {
            done = true;
            return;
        }
        n_arrival = k;
    }
}

// The smallest arrival of a seed (level 0), -1 without one.
inline int64_t leak_step(const int32_t* arrival, const int32_t* level, int64_t n) {
    int64_t leak = -1;
    for (int64_t l = 0; l < n; ++l)
        if (level[l] == 0 && arrival[l] >= 0 && (leak < 0 || arrival[l] < leak)) leak = arrival[l];
    return leak;
}

// Phase B from the per-sweep counters: size[j] = |D_j| and gone[j] = |D_(j-1) \ D_j| for
// j = 1 .. made.  done: a sweep removed nothing (settle = the sweep before it) or left nothing
// (settle = that sweep); else settle = made.
inline void settle_outcome(const unsigned long long* size, const unsigned long long* gone,
                           int64_t made, bool& done, int64_t& settle) {
    done = false;
    settle = made;
    for (int64_t j = 1; j <= made; ++j) {
        if (gone[j] == 0) {
            done = true;
            settle = j - 1;
            return;
        }
        if (size[j] == 0) {
            done = true;
            settle = j;
            return;
        }
    }
}

// The last step set phase C makes: the horizon, cut at the leak and, where phase A did not finish,
// at the sweeps it made.
inline int64_t last_step(int64_t horizon, int64_t leak, bool arrival_done, int64_t max_sweeps) {
    int64_t last = horizon;
    if (leak >= 0 && leak < last) last = leak;
    if (!arrival_done && max_sweeps < last) last = max_sweeps;
    return last;
}

}  // namespace ehm_reach
