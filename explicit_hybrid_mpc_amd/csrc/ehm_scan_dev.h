// The order-preserving exclusive scan of int32 on the device that ehm_reduce.hip (the compaction of
// the survivors), ehm_core.hip (the row offsets of the may-reach relation, 3.8i) and
// ehm_refine.hip (the places of the appended records, 3.8n) share: tiles of 1024, the tiles' totals scanned the same way.  Every translation unit that includes
// this gets its own copy (unnamed namespace), as of ehm_cells_dev.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ehmpc.h"
#include "ehm_host.h"

#define EHM_RED_SCAN_BLOCK 256
#define EHM_RED_SCAN_ITEMS 4
#define EHM_RED_SCAN_TILE (EHM_RED_SCAN_BLOCK * EHM_RED_SCAN_ITEMS)

namespace {

// out [n]: the exclusive sums of in [n] within tiles of 1024; sums [tiles]: the tiles' totals
__global__ __launch_bounds__(EHM_RED_SCAN_BLOCK) void k_reduce_scan(
    long long n, const int32_t* __restrict__ in, int32_t* __restrict__ out,
    int32_t* __restrict__ sums) {
    __shared__ int32_t sh[EHM_RED_SCAN_BLOCK];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * EHM_RED_SCAN_TILE + (long long)t * EHM_RED_SCAN_ITEMS;
    int32_t v[EHM_RED_SCAN_ITEMS];
    int32_t local = 0;
#pragma unroll
    for (int j = 0; j < EHM_RED_SCAN_ITEMS; ++j) {
        v[j] = base + j < n ? in[base + j] : 0;
        local += v[j];
    }
    sh[t] = local;
    __syncthreads();
    for (int off = 1; off < EHM_RED_SCAN_BLOCK; off <<= 1) {
        const int32_t x = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    int32_t run = sh[t] - local;
#pragma unroll
    for (int j = 0; j < EHM_RED_SCAN_ITEMS; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (t == EHM_RED_SCAN_BLOCK - 1) sums[blockIdx.x] = sh[t];
}

__global__ void k_reduce_scan_add(long long n, int32_t* __restrict__ out,
                                  const int32_t* __restrict__ offs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += offs[i / EHM_RED_SCAN_TILE];
}

// out [n] = the exclusive sums of in [n] on the device; failures through `err`
inline int exclusive_scan(ehm_err_channel& err, hipStream_t stream, const int32_t* in,
                          int32_t* out, long long n) {
    const long long tiles = (n + EHM_RED_SCAN_TILE - 1) / EHM_RED_SCAN_TILE;
    DevBuf sums, offs;
    EHM_HIP_TRY(err, sums.alloc((size_t)tiles * sizeof(int32_t)));
    hipLaunchKernelGGL(k_reduce_scan, dim3((unsigned)tiles), dim3(EHM_RED_SCAN_BLOCK), 0, stream,
                       n, in, out, sums.as<int32_t>());
    EHM_HIP_TRY(err, hipGetLastError());
    if (tiles > 1) {
        EHM_HIP_TRY(err, offs.alloc((size_t)tiles * sizeof(int32_t)));
        const int rc = exclusive_scan(err, stream, sums.as<const int32_t>(), offs.as<int32_t>(),
                                      tiles);
        if (rc) return rc;
        hipLaunchKernelGGL(k_reduce_scan_add, dim3(blocks_of(n, 256)), dim3(256), 0, stream,
                           n, out, offs.as<const int32_t>());
        EHM_HIP_TRY(err, hipGetLastError());
    }
    // the buffers are freed on return: hipFree waits for the work that uses them
    EHM_HIP_TRY(err, hipStreamSynchronize(stream));
    return EHM_OK;
}

}  // namespace
