// What the compile step of ehm_compiled.hip and the audit of ehm_audit.hip read of an ehm_explicit
// handle (ehm_explicit.hip owns the struct): device pointers that stay the handle's, valid while it
// lives.  Not exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_err.h"

struct ehm_explicit_view {
    int device;
    const double* rec;          // [n_nodes][rec_stride]: v0 | inv(E)
    const int2* child;          // (left, right), -1 for a leaf
    const double* vinput;       // [n_nodes][(p+1) n_u]
    const int32_t* nbr;         // [n_roots][p+1] face adjacency of the roots, or nullptr
    int rec_stride, p, n_u, n_roots;
    long long n_nodes;
    // what the audit (ehm_audit.hip) reads besides: the costs and flags of ehm_explicit_set_costs
    // (nullptr until set) and the handle's stream
    const double* vcost;        // [n_nodes][p+1]
    const uint8_t* nflags;      // [n_nodes]
    hipStream_t stream;
};

void ehm_explicit_get_view(const ehm_explicit* E, ehm_explicit_view* out);
// sets the message of ehm_explicit_last_error and returns `code` (the error channel of every entry
// point that takes an ehm_explicit handle)
int ehm_explicit_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// the channel itself, for EHM_HIP_TRY
ehm_err_channel& ehm_explicit_channel();

// Face adjacency of n_roots simplices (host): nbr [n_roots][p+1], the root across the face opposite
// vertex i, -1 on the hull.  Root r has the vertices [p+1][p] of node ids[r] (ids nullptr: node r).
// Vertices are one vertex by value (-0.0 == 0.0), faces are matched by their sorted vertex ids.
void ehm_root_adjacency(int64_t n_roots, int p, const double* vertices, const int32_t* ids,
                        std::vector<int32_t>& nbr);
