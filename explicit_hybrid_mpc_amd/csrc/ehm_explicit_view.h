// What the compile step of ehm_compiled.hip reads of an ehm_explicit handle (ehm_explicit.hip owns
// the struct): device pointers that stay the handle's, valid while it lives.  Not exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ehmpc.h"

struct ehm_explicit_view {
    int device;
    const double* rec;          // [n_nodes][rec_stride]: v0 | inv(E)
    const int2* child;          // (left, right), -1 for a leaf
    const double* vinput;       // [n_nodes][(p+1) n_u]
    const int32_t* nbr;         // [n_roots][p+1] face adjacency of the roots, or nullptr
    int rec_stride, p, n_u, n_roots;
    long long n_nodes;
};

void ehm_explicit_get_view(const ehm_explicit* E, ehm_explicit_view* out);
