// A may-reach relation on the device, as ehm_reach.hip and ehm_cost.hip read it: indptr narrowed to
// 32 bits (check_csr of ehm_reach_host.h), indices and the level per leaf.
#pragma once

#include <cstdint>
#include <vector>

#include "ehm_host.h"

struct DevRelation {
    DevBuf ptr, idx, level;
    hipError_t upload(const std::vector<int32_t>& ptr32, const int32_t* indices, int64_t n_edges,
                      const int32_t* level_in, int64_t n) {
        hipError_t e = ptr.upload(ptr32.data(), ptr32.size() * sizeof(int32_t));
        if (e == hipSuccess) e = idx.upload(indices, (size_t)n_edges * sizeof(int32_t));
        if (e == hipSuccess) e = level.upload(level_in, (size_t)n * sizeof(int32_t));
        return e;
    }
};
