// What ehm_certify.hip reads of an ehm_compiled handle (ehm_compiled.hip owns the struct): device
// pointers that stay the handle's, valid while it lives.  Not exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ehmpc.h"

struct ehm_compiled_view {
    int device;
    bool single;                // node and leaf_rec hold floats
    const void* node;           // [n_int][node_stride] of the law's scalar
    const void* leaf_rec;       // [n_leaf][leaf_stride] of the law's scalar
    const int32_t* root_entry;  // [n_roots]
    int p, n_u, node_stride, leaf_stride;
    long long n_roots, n_int, n_leaf, n_test;
    hipStream_t stream;
};

void ehm_compiled_get_view(const ehm_compiled* C, ehm_compiled_view* out);
