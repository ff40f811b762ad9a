// What the two objects of the compiled law share: ehm_compiled.hip -- the double
// law's kernels and all host code -- and ehm_compiled32.hip -- the kernels of the single-precision
// law.  The device view of a law in either precision, the record strides, the containment sums the
// root is chosen with, the walk below the root with the leaf's affine map in both precisions, and
// the closed-loop kernel, whose step is the same code for both but for that walk.  Every translation
// unit that includes this gets its own copy (unnamed namespace), as of ehm_rollout_dev.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ehm_rollout_dev.h"

#define EHM_CP 8                 // max parameter dimension (EHM_MAX_P)
#define EHM_C_LOCATE_MIN 128     // as EHM_X_LOCATE_MIN: spines at least this long get the locator
#define EHM_C_STRICT 1e-9        // as EHM_X_STRICT
#define EHM_C_STEPS 96           // as EHM_X_STEPS
#define EHM_C_EPS 2.220446049250313e-16
#define EHM_C_EPS32 1.1920928955078125e-07f      // 2^-23: the single law goes left iff s >= -2^-23

namespace ehm {

// The kernels of ehm_compiled32.hip, as the host code of ehm_compiled.hip launches them
// (hipLaunchKernel): their arguments are the structs of this header and of ehm_rollout_dev.h.
struct Compiled32Api {
    const void* narrow;                                     // k_compiled_narrow
    const void* eval[EHM_CP];                               // k_compiled_eval32<P>, [p - 1]
    const void* rollout[PK_KINDS][EHM_CP][EHM_R_MAX_NU];    // k_compiled_rollout<float, P, NU, KIND>
};

}  // namespace ehm

namespace {

// T = double: node [n_int][8 or 16 doubles], leaf_rec [n_leaf][leaf_stride doubles].
// T = float: node [n_int][8 or 16 floats] = [a (p) | b | left, right int32 | 0..], 32 B (p <= 5) or
// 64 B, leaf_rec [n_leaf][leaf_stride floats] (a multiple of 4: 16 B).  The rest is the same arrays
// in both: the root is chosen in double on the double state.
template <class T>
struct DevLaw {
    const T* node;
    const T* leaf_rec;
    const int32_t* leaf_node;
    const double* test_rec;
    const double* root_rec;
    const int32_t* root_entry;
    int leaf_stride, side_stride, p, n_u, n_roots;
};
typedef DevLaw<double> DevCompiled;

// elements per internal record, per leaf record (of the law's scalar), per [v0 | inv(E)] record
__host__ __device__ inline int node_stride_of(int p) { return p <= 6 ? 8 : 16; }
inline int leaf_stride_of(int p, int n_u) { return ((p + n_u + n_u * p + 1) / 2) * 2; }
inline int side_stride_of(int p) { return ((p + p * p + 1) / 2) * 2; }
__host__ __device__ inline int node_stride32_of(int p) { return p <= 5 ? 8 : 16; }
inline int leaf_stride32_of(int p, int n_u) { return ((p + n_u + n_u * p + 3) / 4) * 4; }

// k_compiled_narrow (one thread per record): its arguments, and the flags it raises -- what makes
// ehm_compiled_narrow refuse the law
enum { NARROW_OVERFLOW = 1, NARROW_UNDERFLOW = 2, NARROW_ZERO_NORMAL = 4 };

struct NarrowArgs {
    long long n_int, n_leaf;
    int p, leaf_used;                   // leaf_used = p + n_u + n_u p doubles of a leaf record
    int ns64, ns32, ls64, ls32;
    const double *node, *leaf_rec;
    float *node32, *leaf32;
    int* flags;
    // EHM_NARROW_FLUSH (else nullptr): counters of the plane coefficients, plane offsets and leaf
    // values whose float is zero or subnormal and which are stored as +0.0f instead of refused
    unsigned long long* flushed;
};

// The sums of `contains` / `weights` of ehm_explicit.hip (their products fused into the sums, as the
// compiler fuses them there), written out: a = fma(Minv[q][c], x_c - v0_c, a) from 0.0.
template <int P>
__device__ __forceinline__ bool c_contains(const double* __restrict__ r, const double* x) {
    double d[P];
#pragma unroll
    for (int c = 0; c < P; ++c) d[c] = x[c] - r[c];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) a = fma(r[P + q * P + c], d[c], a);
        if (!((a >= -EHM_C_EPS) && (a <= 1.0 + EHM_C_EPS))) return false;
        s += a;
    }
    const double a0 = 1.0 - s;
    return (a0 >= -EHM_C_EPS) && (a0 <= 1.0 + EHM_C_EPS);
}

// (alpha, a0) of x in the [v0 | inv(E)] record r: the sums of c_contains / k_compiled_locate
template <int P>
__device__ __forceinline__ void c_weights(const double* __restrict__ r, const double* x,
                                          double* alpha, double& a0) {
    double d[P];
#pragma unroll
    for (int c = 0; c < P; ++c) d[c] = x[c] - r[c];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) a = fma(r[P + i * P + c], d[c], a);
        alpha[i] = a;
        s += a;
    }
    a0 = 1.0 - s;
}

// ---- below the root: the walk by planes and the leaf's affine map ---------------------------------

// The double law from entry k (plane nodes only): the walk and the leaf map of k_compiled_eval.
// Returns the leaf, u [NU] its input for z.
template <int P, int NU>
__device__ __forceinline__ int law_input(const DevLaw<double>& C, int k, const double* z,
                                         double* u) {
#pragma clang fp contract(off)
    constexpr int NS = P <= 6 ? 8 : 16;
    constexpr int NL = (P + 3) / 2;
    while (k >= 0) {
        const double2* nd = reinterpret_cast<const double2*>(C.node + (size_t)k * NS);
        double r[2 * NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const double2 w = nd[i];
            r[2 * i] = w.x;
            r[2 * i + 1] = w.y;
        }
        const long long ch = __double_as_longlong(r[P + 1]);
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) s = s + r[c] * z[c];
        s = s + r[P];
        k = (s >= -EHM_C_EPS) ? (int)(ch & 0xffffffffll) : (int)(ch >> 32);
    }
    const int l = ~k;
    const double* lr = C.leaf_rec + (size_t)l * C.leaf_stride;
    const double2* lv = reinterpret_cast<const double2*>(lr);
    double d[P];
#pragma unroll
    for (int c = 0; c + 1 < P; c += 2) {
        const double2 w = lv[c / 2];
        d[c] = z[c] - w.x;
        d[c + 1] = z[c + 1] - w.y;
    }
    if (P % 2) d[P - 1] = z[P - 1] - lr[P - 1];
    const double* Kc = lr + P + NU;
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        double w = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) w = w + Kc[c * P + i] * d[i];
        u[c] = lr[P + c] + w;
    }
    return l;
}

// The single law's walk from entry k for the narrowed state xs: one record of 16-byte loads per
// level, s = ((0 + a_0 xs_0) + .. + a_(P-1) xs_(P-1)) + b with every product and every sum rounded
// once to float, left iff s >= -2^-23.  Returns the leaf and adds the levels to `visited`.
template <int P>
__device__ __forceinline__ int walk32(const float* __restrict__ node, int k, const float* xs,
                                      int& visited) {
#pragma clang fp contract(off)
    constexpr int NS = P <= 5 ? 8 : 16;         // node_stride32_of(P)
    constexpr int NL = (P + 6) / 4;             // 16-byte loads that cover [a | b | children]
    while (k >= 0) {
        const float4* nd = reinterpret_cast<const float4*>(node + (size_t)k * NS);
        float r[4 * NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const float4 w = nd[i];
            r[4 * i] = w.x;
            r[4 * i + 1] = w.y;
            r[4 * i + 2] = w.z;
            r[4 * i + 3] = w.w;
        }
        ++visited;
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < P; ++c) s = s + r[c] * xs[c];
        s = s + r[P];
        k = (s >= -EHM_C_EPS32) ? __float_as_int(r[P + 1]) : __float_as_int(r[P + 2]);
    }
    return ~k;
}

// d = xs - v_0 in float; u_c = u_0c + ((0 + K_c0 d_0) + .. + K_c(P-1) d_(P-1)) in float, widened
template <int P>
__device__ __forceinline__ void leaf_offset32(const float* __restrict__ lr, const float* xs,
                                              float* d) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < P; ++c) d[c] = xs[c] - lr[c];
}

template <int P>
__device__ __forceinline__ double leaf_input32(const float* __restrict__ lr, int n_u, int c,
                                               const float* d) {
#pragma clang fp contract(off)
    const float* Kc = lr + P + n_u + c * P;
    float w = 0.0f;
#pragma unroll
    for (int i = 0; i < P; ++i) w = w + Kc[i] * d[i];
    return (double)(lr[P + c] + w);
}

// The single law from entry k: xs = (float) z, walk32, the leaf map.
template <int P, int NU>
__device__ __forceinline__ int law_input(const DevLaw<float>& C, int k, const double* z,
                                         double* u) {
    float xs[P], d[P];
#pragma unroll
    for (int c = 0; c < P; ++c) xs[c] = (float)z[c];
    int visited = 0;
    const int l = walk32<P>(C.node, k, xs, visited);
    const float* lr = C.leaf_rec + (size_t)l * C.leaf_stride;
    leaf_offset32<P>(lr, xs, d);
#pragma unroll
    for (int c = 0; c < NU; ++c) u[c] = leaf_input32<P>(lr, NU, c, d);
    return l;
}

// ---- fused closed-loop rollout ---------------------------------------------------------------------

// The step of k_explicit_rollout around the compiled law.  Laws without test nodes
// only (ehm_compiled_set_plant refuses the others): a state its root holds ends, by the signs of the
// planes, in a leaf that holds it to rounding, so the exit test is made once, on the root's weights.
// The root and the exit test are double arithmetic on the double state for a law of either scalar;
// only law_input differs.
template <class T, int P, int NU, PlantKind KIND>
__global__ __launch_bounds__(256) void k_compiled_rollout(DevLaw<T> C, DevPlant PL, RollArgs R,
                                                          DevNoise NZ, DevGuard GD) {
#pragma clang fp contract(off)
    extern __shared__ double sh[];
    rollout_load<KIND>(PL, NZ, sh);
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= R.n) return;
    RollState<P, NU> S;
    double z[P], alpha[P], u[NU], a0;
    const uint64_t id = NZ.traj0 + (uint64_t)q;
    rollout_begin<P, NU>(R, q, S);
    int status = 0, t = 0;
    int kr = (int)(q % C.n_roots);          // the visibility walk starts at the last step's root
    for (; t < R.T; ++t) {
        rollout_measure<P, NU, KIND>(PL, R, NZ, sh, q, t, id, S, z);
        // root: k_compiled_locate from kr, else the serial rule of k_compiled_eval
        bool found = false;
        if (R.nbr) {
            int kw = kr;
            for (int step = 0; step < EHM_C_STEPS; ++step) {
                c_weights<P>(C.root_rec + (size_t)kw * C.side_stride, z, alpha, a0);
                double lo = a0;
                int at = 0;
#pragma unroll
                for (int i = 0; i < P; ++i)
                    if (alpha[i] < lo) {
                        lo = alpha[i];
                        at = i + 1;
                    }
                if (lo > EHM_C_STRICT) {
                    found = true;
                    break;
                }
                if (lo >= -EHM_C_STRICT) break;
                const int k2 = R.nbr[(size_t)kw * (P + 1) + at];
                if (k2 < 0) break;
                kw = k2;
            }
            if (found) kr = kw;
        }
        if (!found) {
            kr = C.n_roots - 1;
            for (int r = 0; r + 1 < C.n_roots; ++r)
                if (c_contains<P>(C.root_rec + (size_t)r * C.side_stride, z)) {
                    kr = r;
                    break;
                }
            c_weights<P>(C.root_rec + (size_t)kr * C.side_stride, z, alpha, a0);
        }
        // exit test on the root's weights (a NaN state fails it)
        bool inside = a0 >= -R.tol_exit;
#pragma unroll
        for (int i = 0; i < P; ++i) inside = inside && (alpha[i] >= -R.tol_exit);
        if (!inside) {
            status = 1;
            break;
        }
        const int l = law_input<P, NU>(C, C.root_entry[kr], z, u);
        status = rollout_apply<P, NU, KIND>(PL, R, NZ, GD, sh, q, t, id, R.mode[l],
                                            C.leaf_node[l], u, S);
        if (status) break;
    }
    rollout_finish<P, NU, KIND>(PL, R, q, t, status, S);
}

}  // namespace
