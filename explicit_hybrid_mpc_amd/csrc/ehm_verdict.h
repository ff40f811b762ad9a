// What the law checks share when they judge and reduce: the contract
// V - V* <= max(eps_a, eps_r V*) with its slack, the ratio's histogram bin, who is the worst, and
// on the device the LDS counters, the workgroup's worst (key, id) and the row of the applied-input
// problem.  The rules are plain C++ that the kernels inline and a host program can drive
// (tests/native/verdict_host_main.cpp runs them under the address and undefined-behaviour
// sanitizers); tests/audit_cpu.py and tests/applied_cpu.py are their numpy mirrors.  Every function
// whose arithmetic a result depends on runs under fp contract(off): one rounding per operation.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define EHM_VERDICT_HD __host__ __device__ __forceinline__
#else
#define EHM_VERDICT_HD inline
#endif
#if defined(__clang__)
#define EHM_VERDICT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EHM_VERDICT_NO_CONTRACT         // other compilers: build with -ffp-contract=off
#endif

#define EHM_VERDICT_BINS 33         // 32 bins of [0, 1], the last for ratios above 1

namespace ehm_verdict {

// the suboptimality the contract allows at optimal cost vs
EHM_VERDICT_HD double bound_of(double eps_a, double eps_r, double vs) {
    EHM_VERDICT_NO_CONTRACT
    const double er = eps_r * vs;
    return eps_a > er ? eps_a : er;
}

// what two solves of one problem may differ by
EHM_VERDICT_HD double slack_of(double rtol, double vs) {
    EHM_VERDICT_NO_CONTRACT
    return rtol * (1.0 + fabs(vs));
}

// The ladder every audit ends with: 2 for a gap below -slack (a NaN gap too), 1 for one above
// bound + slack, else 0.
EHM_VERDICT_HD int gap_status(double gap, double bound, double slack) {
    EHM_VERDICT_NO_CONTRACT
    if (!(gap >= -slack)) return 2;
    if (gap > bound + slack) return 1;
    return 0;
}

EHM_VERDICT_HD double ratio_of(double gap, double bound) {
    EHM_VERDICT_NO_CONTRACT
    return gap / bound;
}

// the histogram bin of a ratio: negative and NaN ratios 0, ratios above 1 the last, else
// min(31, int(32 r))
EHM_VERDICT_HD int ratio_bin(double r) {
    EHM_VERDICT_NO_CONTRACT
    if (r > 1.0) return EHM_VERDICT_BINS - 1;
    if (!(r >= 0.0)) return 0;
    const int bin = (int)(r * 32.0);
    return bin > 31 ? 31 : bin;
}

// a NaN ratio is binned and never the worst sample
EHM_VERDICT_HD bool ratio_is_candidate(double r) { return r == r; }

// (ratio, id) a beats b: the larger ratio, the smaller id on ties (a NaN never wins)
EHM_VERDICT_HD bool ratio_beats(double ra, uint64_t ia, double rb, uint64_t ib) {
    return ra > rb || (ra == rb && ia < ib);
}

// Folds the (key, id) of a chunk's n workgroups into the running best (no_id: none yet) and says
// whether the best moved.  A workgroup without a candidate (id == no_id) never wins.  The first
// candidate is taken without asking `beats` (the certificate's sentinel id, -1, would win a tie), so
// a NaN key is refused here too: a second guard, the kernels' candidate rules give no NaN an id.
template <class Id, class Beats>
inline bool merge_block_worst(const double* key, const Id* id, size_t n, Id no_id, Beats beats,
                              double& best_key, Id& best_id) {
    bool moved = false;
    for (size_t b = 0; b < n; ++b)
        if (id[b] != no_id && key[b] == key[b] &&
            (best_id == no_id || beats(key[b], id[b], best_key, best_id))) {
            best_key = key[b];
            best_id = id[b];
            moved = true;
        }
    return moved;
}

#if defined(__HIPCC__)

// an N-entry block of LDS counters (static, or a kernel's place in its dynamic LDS): zeroed (a
// barrier follows in the kernel), and its counts added to the run's once the workgroup's atomics
// are behind a barrier
template <int BLOCK, int N>
__device__ __forceinline__ void counters_zero(unsigned int* cnt) {
    for (int i = threadIdx.x; i < N; i += BLOCK) cnt[i] = 0;
}

template <int BLOCK, int N>
__device__ __forceinline__ void counters_flush(const unsigned int* cnt,
                                               unsigned long long* __restrict__ counters) {
    for (int i = threadIdx.x; i < N; i += BLOCK)
        if (cnt[i]) atomicAdd(&counters[i], (unsigned long long)cnt[i]);
}

// The workgroup's worst (key, id) by an LDS tree: of the threads whose id `has` one, the one that
// `beats` every other.  All BLOCK threads call it; (key, id) is the result in every thread (no
// thread's id has one: some thread's own pair).
template <int BLOCK, class Id, class Beats, class Has>
__device__ __forceinline__ void block_worst(double& key, Id& id, Beats beats, Has has) {
    __shared__ double sk[BLOCK];
    __shared__ Id si[BLOCK];
    const int t = threadIdx.x;
    sk[t] = key;
    si[t] = id;
    __syncthreads();
    for (int h = BLOCK / 2; h > 0; h >>= 1) {
        if (t < h && has(si[t + h]) &&
            (!has(si[t]) || beats(sk[t + h], si[t + h], sk[t], si[t]))) {
            sk[t] = sk[t + h];
            si[t] = si[t + h];
        }
        __syncthreads();
    }
    key = sk[0];
    id = si[0];
}

// One row of the applied-input problem: theta' = (x, ubar) into t [p + n_u] and the cost constant
// ((0 + cost_u[0] u_0) + cost_u[1] u_1) + .. into konst.  x(c) and u(j) load the components; one of
// u that is not finite enters as 0 and the row is bad (returned).
template <class LoadX, class LoadU>
__device__ __forceinline__ bool pack_applied_row(int p, int n_u, LoadX x, LoadU u,
                                                 const double* __restrict__ cost_u,
                                                 double* __restrict__ t, double* konst) {
#pragma clang fp contract(off)
    for (int c = 0; c < p; ++c) t[c] = x(c);
    double k = 0.0;
    bool bad = false;
    for (int j = 0; j < n_u; ++j) {
        double uj = u(j);
        if (!isfinite(uj)) {
            bad = true;
            uj = 0.0;
        }
        t[p + j] = uj;
        k = k + cost_u[j] * uj;
    }
    *konst = k;
    return bad;
}

#endif  // __HIPCC__

}  // namespace ehm_verdict
