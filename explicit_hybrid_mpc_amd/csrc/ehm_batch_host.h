// Host-side row bookkeeping of the batched oracles (ehm_capi.hip: run_batch and the multi-commutation
// orchestration on top of it).  Plain C++, no HIP: tests/host/batch_host_main.cpp runs it under the
// host sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// stable counting sort of a batch by commutation index: order[k] = original position of the
// k-th instance of the sorted batch, seg[d] = first sorted position of commutation d
static inline void sort_by_commutation(int nd, int64_t n, const int32_t* didx,
                                       std::vector<int64_t>& order, std::vector<int32_t>& seg) {
    seg.assign((size_t)nd + 1, 0);
    for (int64_t k = 0; k < n; ++k) seg[(size_t)didx[k] + 1]++;
    for (int d = 0; d < nd; ++d) seg[(size_t)d + 1] += seg[(size_t)d];
    std::vector<int32_t> pos(seg.begin(), seg.end() - 1);
    order.resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) order[(size_t)pos[(size_t)didx[k]]++] = k;
}

// the indices k in [0, n) with keep(k), ascending
template <class Keep>
static inline std::vector<int64_t> where(int64_t n, const Keep& keep) {
    std::vector<int64_t> idx;
    for (int64_t k = 0; k < n; ++k)
        if (keep(k)) idx.push_back(k);
    return idx;
}

// Rows of `width` elements.  gather: row k of dst = row idx[k] of src; scatter: row idx[k] of
// dst = row k of src (the inverse where idx is a permutation).
template <class T>
static inline void gather_rows(T* dst, const T* src, const std::vector<int64_t>& idx, size_t width) {
    for (size_t k = 0; k < idx.size() && width; ++k)
        std::memcpy(dst + k * width, src + (size_t)idx[k] * width, width * sizeof(T));
}

template <class T>
static inline void scatter_rows(T* dst, const T* src, const std::vector<int64_t>& idx, size_t width) {
    for (size_t k = 0; k < idx.size() && width; ++k)
        std::memcpy(dst + (size_t)idx[k] * width, src + k * width, width * sizeof(T));
}

template <class T>
static inline std::vector<T> gathered(const T* src, const std::vector<int64_t>& idx, size_t width) {
    std::vector<T> out(idx.size() * width);
    gather_rows(out.data(), src, idx, width);
    return out;
}

// Results of a retried subset into the full results: row idx[k] of dst = row k of src where the
// retry converged (status[k] == 0).  Returns how many rows it took.
template <class T>
static inline int64_t merge_retried(T* dst, const T* src, const std::vector<int64_t>& idx,
                                    const int32_t* status, size_t width) {
    int64_t taken = 0;
    for (size_t k = 0; k < idx.size(); ++k) {
        if (status[k] != 0) continue;
        std::memcpy(dst + (size_t)idx[k] * width, src + k * width, width * sizeof(T));
        ++taken;
    }
    return taken;
}
