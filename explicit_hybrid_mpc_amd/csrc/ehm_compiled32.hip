// The kernels of the single-precision compiled law ("single precision"): the
// narrowing of a double law's records, the evaluation and the closed loop.  Device code only -- the
// host code of ehm_compiled.hip owns the handles and launches these through ehm_compiled32_api.
//
// Only the internal records and the leaf records are floats.  The root is chosen in double on the
// double state by the double law's code (k_compiled_locate of ehm_compiled.hip, c_contains), and the
// rollout's exit test is the double law's too; below the root xs = (float) x, and every product and
// every sum of the walk and of the leaf map is rounded once to float (fp contract off).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "ehm_compiled_dev.h"

namespace {

// ---- narrowing: one thread per record ----------------------------------------------------------------

// round to nearest float; a value that leaves the normal range (or was not finite) raises its flag.
// Under `flush` a nonzero value whose float is zero or subnormal (|v| < 2^-126) becomes +0.0f and is
// counted in `flushed` instead.
__device__ __forceinline__ float narrow_value(double v, int& flags, bool flush, int& flushed) {
    const float f = (float)v;
    if (!(fabsf(f) <= FLT_MAX)) flags |= NARROW_OVERFLOW;
    else if (v != 0.0 && fabsf(f) < FLT_MIN) {
        if (!flush) flags |= NARROW_UNDERFLOW;
        else {
            ++flushed;
            return 0.0f;
        }
    }
    return f;
}

__global__ __launch_bounds__(256) void k_compiled_narrow(NarrowArgs A) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_int + A.n_leaf) return;
    const bool flush = A.flushed != nullptr;
    int flags = 0, gone[3] = {0, 0, 0};     // flushed plane coefficients, offsets, leaf values
    if (k < A.n_int) {
        const double* r = A.node + (size_t)k * A.ns64;
        float* out = A.node32 + (size_t)k * A.ns32;
        bool zero = true;
        for (int c = 0; c <= A.p; ++c) {
            const float f = narrow_value(r[c], flags, flush, gone[c < A.p ? 0 : 1]);
            if (c < A.p) zero = zero && f == 0.0f;
            out[c] = f;
        }
        if (zero) flags |= NARROW_ZERO_NORMAL;
        const int2 ch = *reinterpret_cast<const int2*>(r + A.p + 1);
        int32_t* cp = reinterpret_cast<int32_t*>(out + A.p + 1);
        cp[0] = ch.x;
        cp[1] = ch.y;
        for (int c = A.p + 3; c < A.ns32; ++c) out[c] = 0.0f;
    } else {
        const long long l = k - A.n_int;
        const double* r = A.leaf_rec + (size_t)l * A.ls64;
        float* out = A.leaf32 + (size_t)l * A.ls32;
        for (int c = 0; c < A.leaf_used; ++c) out[c] = narrow_value(r[c], flags, flush, gone[2]);
        for (int c = A.leaf_used; c < A.ls32; ++c) out[c] = 0.0f;
    }
    if (flags) atomicOr(A.flags, flags);
    for (int i = 0; i < 3; ++i)
        if (gone[i]) atomicAdd(A.flushed + i, (unsigned long long)gone[i]);
}

// ---- evaluation ----------------------------------------------------------------------------------------

// k_compiled_eval for the single law: the root as there (the locator's result, else the serial rule,
// both on the double state), then the float walk and the float leaf map; u is widened on store.
template <int P>
__global__ __launch_bounds__(256) void k_compiled_eval32(DevLaw<float> C, long long n,
                                                         const double* __restrict__ X,
                                                         double* __restrict__ U,
                                                         int32_t* __restrict__ leaf,
                                                         int32_t* __restrict__ depth_out,
                                                         const int32_t* __restrict__ root) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double x[P];
#pragma unroll
    for (int c = 0; c < P; ++c) x[c] = X[q * P + c];
    // roots: first root that contains x, the last one without a test
    int kr = C.n_roots - 1, visited = 0;
    if (root && root[q] >= 0) {
        kr = root[q] & 0xfffff;
        visited = root[q] >> 20;
    } else {
        for (int r = 0; r + 1 < C.n_roots; ++r) {
            ++visited;
            if (c_contains<P>(C.root_rec + (size_t)r * C.side_stride, x)) {
                kr = r;
                break;
            }
        }
    }
    float xs[P], d[P];
#pragma unroll
    for (int c = 0; c < P; ++c) xs[c] = (float)x[c];
    const int l = walk32<P>(C.node, C.root_entry[kr], xs, visited);
    const float* lr = C.leaf_rec + (size_t)l * C.leaf_stride;
    leaf_offset32<P>(lr, xs, d);
    const int n_u = C.n_u;
    for (int c = 0; c < n_u; ++c) U[q * n_u + c] = leaf_input32<P>(lr, n_u, c, d);
    if (leaf) leaf[q] = C.leaf_node[l];
    if (depth_out) depth_out[q] = visited;
}

#define EHM_K(f) reinterpret_cast<const void*>(&f)
#define EHM_R_NU(P, K) EHM_K((k_compiled_rollout<float, P, 1, K>)), \
                       EHM_K((k_compiled_rollout<float, P, 2, K>)), \
                       EHM_K((k_compiled_rollout<float, P, 3, K>)), \
                       EHM_K((k_compiled_rollout<float, P, 4, K>))
#define EHM_R_ALL(K) {{EHM_R_NU(1, K)}, {EHM_R_NU(2, K)}, {EHM_R_NU(3, K)}, {EHM_R_NU(4, K)}, \
                      {EHM_R_NU(5, K)}, {EHM_R_NU(6, K)}, {EHM_R_NU(7, K)}, {EHM_R_NU(8, K)}}
const ehm::Compiled32Api g_api = {
    EHM_K(k_compiled_narrow),
    {EHM_K(k_compiled_eval32<1>), EHM_K(k_compiled_eval32<2>), EHM_K(k_compiled_eval32<3>),
     EHM_K(k_compiled_eval32<4>), EHM_K(k_compiled_eval32<5>), EHM_K(k_compiled_eval32<6>),
     EHM_K(k_compiled_eval32<7>), EHM_K(k_compiled_eval32<8>)},
    {EHM_R_ALL(PK_NOMINAL), EHM_R_ALL(PK_NOISY), EHM_R_ALL(PK_GUARDED)}};
#undef EHM_R_ALL
#undef EHM_R_NU
#undef EHM_K

}  // namespace

extern "C" const ehm::Compiled32Api* ehm_compiled32_api() { return &g_api; }
