// What ehm_certify.hip, ehm_reduce.hip and ehm_invariance.hip read of an ehm_compiled handle
// (ehm_compiled.hip owns the struct): device pointers that stay the handle's, valid while it lives.
// Not exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ehmpc.h"
#include "ehm_host.h"

struct ehm_compiled_view {
    int device;
    bool single;                // node and leaf_rec hold floats
    const void* node;           // [n_int][node_stride] of the law's scalar
    const void* leaf_rec;       // [n_leaf][leaf_stride] of the law's scalar
    const int32_t* leaf_node;   // [n_leaf]
    const int32_t* root_entry;  // [n_roots]
    int p, n_u, node_stride, leaf_stride;
    long long n_roots, n_int, n_leaf, n_test;
    hipStream_t stream;
    const double* root_rec;     // [n_roots][side_stride] doubles in either precision
    const int32_t* nbr;         // [n_roots][p+1] the roots' face adjacency, or nullptr
    int side_stride;
};

void ehm_compiled_get_view(const ehm_compiled* C, ehm_compiled_view* out);

// A new law on the device of `like` with n_int internal and n_leaf leaf records of like's scalar
// and strides (ehm_reduce.hip, ehm_refine.hip): it takes over the four buffers, copies like's root records and
// adjacency table, and is checked as ehm_compiled_import checks a file's arrays (on a host copy)
// before it is returned; the header's source node count is raised to n_leaf where it was below
// (the leaves of a refined law share source nodes).  Errors through ehm_compiled_last_error.
int ehm_compiled_adopt(const ehm_compiled* like, int64_t n_int, int64_t n_leaf, DevBuf& node,
                       DevBuf& leaf_rec, DevBuf& leaf_node, DevBuf& root_entry,
                       ehm_compiled** out);
