// Philox4x64-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011), the
// counter-based generator of the noisy rollout.  numpy's np.random.Philox is the same function:
// its random_raw(4) with counter c returns philox4x64_10(c + 1, key).  The host mirror is
// noise.py (philox4x64_10), which splits the 64 x 64 -> 128 products into 32-bit halves.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#define EHM_PHILOX_M0 0xD2E7470EE14C6C93ULL
#define EHM_PHILOX_M1 0xCA5A826395121157ULL
#define EHM_PHILOX_W0 0x9E3779B97F4A7C15ULL
#define EHM_PHILOX_W1 0xBB67AE8584CAA73BULL

// c [4] in: the counter, out: the block.  Key (k0, k1).
__device__ __forceinline__ void ehm_philox4x64_10(uint64_t* c, uint64_t k0, uint64_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t lo0 = EHM_PHILOX_M0 * c[0], hi0 = __umul64hi(EHM_PHILOX_M0, c[0]);
        const uint64_t lo1 = EHM_PHILOX_M1 * c[2], hi1 = __umul64hi(EHM_PHILOX_M1, c[2]);
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += EHM_PHILOX_W0;
        k1 += EHM_PHILOX_W1;
    }
}

// a raw word -> uniform in [-1, 1): (r >> 11) 2^-52 - 1, exact in FP64
__device__ __forceinline__ double ehm_uniform_pm1(uint64_t r) {
    return (double)(r >> 11) * 0x1p-52 - 1.0;
}
