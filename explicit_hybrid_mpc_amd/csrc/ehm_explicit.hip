// Batched evaluation of the explicit control law: the consumer of the
// partition, ExplicitMPC.__call__ of the reference (lib/mpc_library.py:685-792), for whole
// batches of states on the device.
//
// Reference semantics kept: the partition is one binary tree; at an internal node the query
// goes LEFT iff it lies in the left child's simplex (all barycentric weights in
// [-eps, 1+eps], eps = machine epsilon, lib/mpc_library.py:714-735), otherwise right without a
// test; at the leaf the input is the barycentric interpolation of the vertex inputs
// (lib/mpc_library.py:786-789).  The root simplices hang off a right spine (tools.delaunay,
// lib/tools.py:152-189): root i is the left child of spine node i, the last two roots share
// the last spine node -- so the walk over the spine is "first root 0..Nsx-2 that contains x,
// else the last root".
//
// Layout: one 64-byte-aligned record per node, [v0 (p) | Minv (p x p, row-major)] with
// Minv = inv([v1-v0 ... vp-v0]) (computed on the device once, Gauss-Jordan with partial
// pivoting), child pair (left, right) as int2, vertex inputs (p+1) x n_u.  One thread per
// query: a walk reads one record per level (top levels L2-resident), i.e. the kernel is
// latency/HBM-bound, not arithmetic-bound.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_explicit_dev.h"
#include "ehm_explicit_view.h"
#include "ehm_host.h"
#include "ehm_philox.h"
#include "ehm_rollout_dev.h"

#define EHM_X_LOCATE_MIN 128     // spines at least this long get the root locator

namespace {

// Minv per node from its vertices [(p+1) p]
__global__ void k_explicit_setup(long long n_nodes, int p, int rec_stride,
                                 const double* __restrict__ vertices, double* __restrict__ rec,
                                 int32_t* __restrict__ singular) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_nodes) return;
    const double* V = vertices + (size_t)k * (p + 1) * p;
    double A[EHM_XP * 2 * EHM_XP];       // [E | I], E[r][q] = V[q+1][r] - V[0][r]
    const int w = 2 * p;
    for (int r = 0; r < p; ++r)
        for (int c = 0; c < w; ++c)
            A[r * w + c] = (c < p) ? (V[(c + 1) * p + r] - V[r]) : ((c - p == r) ? 1.0 : 0.0);
    bool bad = false;
    for (int c = 0; c < p; ++c) {
        int piv = c;
        double best = fabs(A[c * w + c]);
        for (int r = c + 1; r < p; ++r)
            if (fabs(A[r * w + c]) > best) {
                best = fabs(A[r * w + c]);
                piv = r;
            }
        if (best == 0.0) {
            bad = true;
            break;
        }
        if (piv != c)
            for (int q = 0; q < w; ++q) {
                const double t = A[c * w + q];
                A[c * w + q] = A[piv * w + q];
                A[piv * w + q] = t;
            }
        const double rp = 1.0 / A[c * w + c];
        for (int q = 0; q < w; ++q) A[c * w + q] *= rp;
        for (int r = 0; r < p; ++r) {
            if (r == c) continue;
            const double f = A[r * w + c];
            for (int q = 0; q < w; ++q) A[r * w + q] = fma(-f, A[c * w + q], A[r * w + q]);
        }
    }
    double* out = rec + (size_t)k * rec_stride;
    for (int c = 0; c < p; ++c) out[c] = V[c];
    for (int r = 0; r < p; ++r)
        for (int c = 0; c < p; ++c) out[p + r * p + c] = bad ? 0.0 : A[r * w + p + c];
    if (bad) atomicAdd(singular, 1);
}

// the root locator of long spines (explicit_locate_root, ehm_explicit_dev.h), one thread per state
__global__ void k_explicit_locate(DevExplicit E, long long n, const double* __restrict__ X,
                                  const int32_t* __restrict__ nbr, int32_t* __restrict__ root) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int p = E.p;
    double x[EHM_XP];
    for (int c = 0; c < p; ++c) x[c] = X[q * p + c];
    root[q] = explicit_locate_root(E, x, q, nbr);
}

__global__ void k_explicit_eval(DevExplicit E, long long n, const double* __restrict__ X,
                                double* __restrict__ U, int32_t* __restrict__ leaf,
                                int32_t* __restrict__ depth_out,
                                const int32_t* __restrict__ root) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int p = E.p, n_u = E.n_u;
    double x[EHM_XP], alpha[EHM_XP], a0;
    for (int c = 0; c < p; ++c) x[c] = X[q * p + c];
    // spine (the root k_explicit_locate found where the spine is long), then the partition subtree
    int visited = 0;
    const long long k = explicit_walk(E, x, root ? root[q] : -1, visited);
    (void)weights(E, k, x, alpha, a0);
    const double* vi = E.vinput + (size_t)k * (p + 1) * n_u;
    for (int c = 0; c < n_u; ++c) {
        double u = a0 * vi[c];
        for (int i = 0; i < p; ++i) u += vi[(i + 1) * n_u + c] * alpha[i];
        U[q * n_u + c] = u;
    }
    if (leaf) leaf[q] = (int32_t)k;
    if (depth_out) depth_out[q] = visited;
}

// ---- fused closed-loop rollout (lib/simulator.py:124-188 for batches of trajectories) --------
//
// One thread per trajectory, the T steps inside the kernel: measure z = x + v (no error at t = 0,
// lib/simulator.py:168), locate z with the walk of k_explicit_eval, stop if z is outside the leaf
// (weight < -tol_exit), interpolate u as k_explicit_eval does, step the plant in the step-0 mode of
// the leaf's commutation, accumulate stage cost / input 2-norm / worst constraint value.  Templated
// on (p, n_u) so that state, weights and inputs live in VGPRs, and on the plant kind (PlantKind);
// the plant sits in LDS (its layout, the guards', the model's and the sampler: ehm_rollout_dev.h,
// which also states the step once the input is known -- rollout_apply -- and the records).

// the sums of `contains` / `weights` with p fixed at compile time.  Kept outside any fp-contract
// pragma, as those two are: the compiler fuses the same products into the same FMAs, so the
// containment verdicts and weights are bit-identical to k_explicit_eval's.
template <int P>
__device__ __forceinline__ bool contains_t(const DevExplicit& E, long long k, const double* x) {
    const double* r = E.rec + (size_t)k * E.rec_stride;
    const double eps = 2.220446049250313e-16;
    double d[P];
#pragma unroll
    for (int c = 0; c < P; ++c) d[c] = x[c] - r[c];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) a += r[P + q * P + c] * d[c];
        if (!((a >= -eps) && (a <= 1.0 + eps))) return false;
        s += a;
    }
    const double a0 = 1.0 - s;
    return (a0 >= -eps) && (a0 <= 1.0 + eps);
}

template <int P>
__device__ __forceinline__ void weights_t(const DevExplicit& E, long long k, const double* x,
                                          double* alpha, double& alpha0) {
    const double* r = E.rec + (size_t)k * E.rec_stride;
    double d[P];
#pragma unroll
    for (int c = 0; c < P; ++c) d[c] = x[c] - r[c];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) a += r[P + q * P + c] * d[c];
        alpha[q] = a;
        s += a;
    }
    alpha0 = 1.0 - s;
}

template <int P, int NU, PlantKind KIND>
__global__ __launch_bounds__(256) void k_explicit_rollout(DevExplicit E, DevPlant PL, RollArgs R,
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
    int kr = (int)(q % E.n_roots);          // warm start of the root locator: the last step's root
    for (; t < R.T; ++t) {
        rollout_measure<P, NU, KIND>(PL, R, NZ, sh, q, t, id, S, z);
        // locate: the spine (visibility walk from the last root where the spine is long, the
        // serial walk wherever that walk gives up), then left iff inside the left child
        long long k = E.n_roots - 1;
        bool found = false;
        if (R.nbr) {
            int kw = kr;
            for (int step = 0; step < EHM_X_STEPS; ++step) {
                weights_t<P>(E, kw, z, alpha, a0);
                double lo = a0;
                int at = 0;
#pragma unroll
                for (int i = 0; i < P; ++i)
                    if (alpha[i] < lo) {
                        lo = alpha[i];
                        at = i + 1;
                    }
                if (lo > EHM_X_STRICT) {
                    found = true;
                    break;
                }
                if (!(lo >= -EHM_X_STRICT)) {
                    const int k2 = R.nbr[(size_t)kw * (P + 1) + at];
                    if (k2 < 0) break;
                    kw = k2;
                } else {
                    break;
                }
            }
            if (found) k = kw;
        }
        if (!found)
            for (int r = 0; r + 1 < E.n_roots; ++r)
                if (contains_t<P>(E, r, z)) {
                    k = r;
                    break;
                }
        kr = (int)k;
        for (;;) {
            const int2 ch = E.child[k];
            if (ch.x < 0) break;
            k = contains_t<P>(E, ch.x, z) ? ch.x : ch.y;
        }
        // exit test: the walk ends in a leaf even for states outside the partitioned set
        weights_t<P>(E, k, z, alpha, a0);
        bool inside = a0 >= -R.tol_exit;
#pragma unroll
        for (int i = 0; i < P; ++i) inside = inside && (alpha[i] >= -R.tol_exit);
        if (!inside) {
            status = 1;
            break;
        }
        // interpolate (the sums of k_explicit_eval)
        const double* vi = E.vinput + (size_t)k * (P + 1) * NU;
#pragma unroll
        for (int c = 0; c < NU; ++c) {
            double a = a0 * vi[c];
#pragma unroll
            for (int i = 0; i < P; ++i) a += vi[(i + 1) * NU + c] * alpha[i];
            u[c] = a;
        }
        // the mode the leaf's commutation applies at step 0; the rest of the step
        status = rollout_apply<P, NU, KIND>(PL, R, NZ, GD, sh, q, t, id, R.mode[k], (int32_t)k, u,
                                            S);
        if (status) break;
    }
    rollout_finish<P, NU, KIND>(PL, R, q, t, status, S);
}

typedef void (*rollout_fn)(DevExplicit, DevPlant, RollArgs, DevNoise, DevGuard);
#define EHM_R_NU(P, K) &k_explicit_rollout<P, 1, K>, &k_explicit_rollout<P, 2, K>, \
                       &k_explicit_rollout<P, 3, K>, &k_explicit_rollout<P, 4, K>
#define EHM_R_ALL(K) {{EHM_R_NU(1, K)}, {EHM_R_NU(2, K)}, {EHM_R_NU(3, K)}, {EHM_R_NU(4, K)}, \
                      {EHM_R_NU(5, K)}, {EHM_R_NU(6, K)}, {EHM_R_NU(7, K)}, {EHM_R_NU(8, K)}}
// [kind][p - 1][n_u - 1]
const rollout_fn k_rollout_table[PK_KINDS][EHM_XP][EHM_R_MAX_NU] = {
    EHM_R_ALL(PK_NOMINAL), EHM_R_ALL(PK_NOISY), EHM_R_ALL(PK_GUARDED)};
#undef EHM_R_ALL
#undef EHM_R_NU

// raw Philox4x64-10 blocks (the oracle test of the generator)
__global__ void k_philox_batch(long long n, const uint64_t* __restrict__ ctr, uint64_t k0,
                               uint64_t k1, uint64_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t c[4] = {ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]};
    ehm_philox4x64_10(c, k0, k1);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * i + k] = c[k];
}

// EHM_EXPLICIT_LOCATE=0 in the environment: the reference's serial walk for every state
bool locate_off() {
    static const bool off = [] {
        const char* e = getenv("EHM_EXPLICIT_LOCATE");
        return e && atoi(e) == 0;
    }();
    return off;
}

thread_local ehm_err_channel x_err;


}  // namespace

struct ehm_explicit {
    int device = 0;
    DevExplicit d{};
    DevBuf rec, child, vinput;
    DevBuf x, u, leaf, depth, root;     // ehm_explicit_eval_batch, cap queries
    DevBuf nbr;         // [n_roots][p+1] root across the face opposite vertex i (-1: hull)
    DevBuf vcost, nflags;   // ehm_explicit_set_costs: [n_nodes][p+1] doubles, [n_nodes] bytes
    RolloutAttach ro;   // plant, node modes and model of the rollouts (ehm_explicit_set_*)
    size_t cap = 0;
    Stream stream;
};

// what ehm_compiled_create reads of a handle (ehm_explicit_view.h)
void ehm_explicit_get_view(const ehm_explicit* E, ehm_explicit_view* out) {
    *out = ehm_explicit_view{E->device, E->d.rec, E->d.child, E->d.vinput,
                             E->nbr.as<const int32_t>(), E->d.rec_stride, E->d.p, E->d.n_u,
                             E->d.n_roots, E->d.n_nodes,
                             E->vcost.as<const double>(), E->nflags.as<const uint8_t>(),
                             E->stream};
}

ehm_err_channel& ehm_explicit_channel() { return x_err; }

int ehm_explicit_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    x_err.vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

// face adjacency of the roots (ehm_explicit_view.h): vertices by value, faces by their sorted
// vertex ids (the key holds -0.0 as 0.0: one vertex however a root writes its zero coordinates)
void ehm_root_adjacency(int64_t n_roots, int p, const double* vertices, const int32_t* ids_of,
                        std::vector<int32_t>& nbr) {
    std::unordered_map<std::string, int32_t> vid;
    std::vector<int32_t> ids((size_t)n_roots * (p + 1));
    double vk[EHM_XP];
    for (int64_t r = 0; r < n_roots; ++r) {
        const size_t node = ids_of ? (size_t)ids_of[r] : (size_t)r;
        for (int i = 0; i <= p; ++i) {
            const double* v = vertices + (node * (p + 1) + i) * p;
            for (int c = 0; c < p; ++c) vk[c] = (v[c] == 0.0) ? 0.0 : v[c];
            std::string key((const char*)vk, sizeof(double) * p);
            auto it = vid.find(key);
            if (it == vid.end()) it = vid.emplace(std::move(key), (int32_t)vid.size()).first;
            ids[(size_t)r * (p + 1) + i] = it->second;
        }
    }
    nbr.assign((size_t)n_roots * (p + 1), -1);
    std::unordered_map<std::string, int64_t> face;      // key -> root * (p+1) + i of the first owner
    std::vector<int32_t> f((size_t)p);
    for (int64_t r = 0; r < n_roots; ++r)
        for (int i = 0; i <= p; ++i) {
            int w = 0;
            for (int j = 0; j <= p; ++j)
                if (j != i) f[(size_t)w++] = ids[(size_t)r * (p + 1) + j];
            std::sort(f.begin(), f.end());
            std::string key((const char*)f.data(), sizeof(int32_t) * p);
            auto it = face.find(key);
            if (it == face.end()) {
                face.emplace(std::move(key), r * (p + 1) + i);
            } else {
                const int64_t o = it->second;
                nbr[(size_t)r * (p + 1) + i] = (int32_t)(o / (p + 1));
                nbr[(size_t)o] = (int32_t)r;
            }
        }
}

extern "C" {

const char* ehm_explicit_last_error(void) { return x_err.c_str(); }

int ehm_explicit_destroy(ehm_explicit* E) {
    if (!E) return EHM_OK;
    (void)hipSetDevice(E->device);
    delete E;       // the stream and the buffers free themselves
    return EHM_OK;
}

int ehm_explicit_create(int device, int64_t n_nodes, int32_t n_roots, int32_t p, int32_t n_u,
                        const int32_t* left, const int32_t* right, const double* vertices,
                        const double* vinput, ehm_explicit** out) {
    if (!out || !left || !right || !vertices || !vinput || n_nodes < 1 || n_roots < 1 ||
        n_roots > n_nodes || p < 1 || p > EHM_XP || n_u < 1)
        return x_err.fail(EHM_E_INVALID, "bad argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return x_err.fail(EHM_E_NO_DEVICE, "no HIP device %d (libehmpc has no CPU fallback)",
                          device);
    // destroyed on every error return below
    std::unique_ptr<ehm_explicit, int (*)(ehm_explicit*)> E(new ehm_explicit(),
                                                            ehm_explicit_destroy);
    E->device = device;
    EHM_HIP_TRY(x_err, hipSetDevice(device));
    EHM_HIP_TRY(x_err, E->stream.create());
    const int stride = ((p + p * p + 7) / 8) * 8;
    const size_t nV = (size_t)n_nodes * (p + 1) * p, nU = (size_t)n_nodes * (p + 1) * n_u;
    std::vector<int2> ch((size_t)n_nodes);
    for (int64_t k = 0; k < n_nodes; ++k) ch[(size_t)k] = make_int2(left[k], right[k]);
    DevBuf d_vert, d_sing;
    EHM_HIP_TRY(x_err, E->rec.alloc((size_t)n_nodes * stride * sizeof(double)));
    EHM_HIP_TRY(x_err, E->child.upload(ch.data(), ch.size() * sizeof(int2)));
    EHM_HIP_TRY(x_err, E->vinput.upload(vinput, nU * sizeof(double)));
    EHM_HIP_TRY(x_err, d_vert.upload(vertices, nV * sizeof(double)));
    EHM_HIP_TRY(x_err, d_sing.alloc(sizeof(int32_t)));
    EHM_HIP_TRY(x_err, hipMemset(d_sing.ptr, 0, sizeof(int32_t)));
    hipLaunchKernelGGL(k_explicit_setup, dim3((unsigned)((n_nodes + 127) / 128)), dim3(128), 0,
                       E->stream, (long long)n_nodes, (int)p, stride, d_vert.as<const double>(),
                       E->rec.as<double>(), d_sing.as<int32_t>());
    int32_t sing = 0;
    EHM_HIP_TRY(x_err, hipMemcpyAsync(&sing, d_sing.ptr, sizeof sing, hipMemcpyDeviceToHost,
                                      E->stream));
    EHM_HIP_TRY(x_err, hipStreamSynchronize(E->stream));
    if (sing) return x_err.fail(EHM_E_NUMERIC, "%d degenerate simplices in the partition",
                                (int)sing);
    if (n_roots >= EHM_X_LOCATE_MIN && n_roots < (1 << 20)) {
        std::vector<int32_t> nbr;
        ehm_root_adjacency(n_roots, p, vertices, nullptr, nbr);
        EHM_HIP_TRY(x_err, E->nbr.upload(nbr.data(), nbr.size() * sizeof(int32_t)));
    }
    E->d.rec = E->rec.as<const double>();
    E->d.child = E->child.as<const int2>();
    E->d.vinput = E->vinput.as<const double>();
    E->d.rec_stride = stride;
    E->d.p = p;
    E->d.n_u = n_u;
    E->d.n_roots = n_roots;
    E->d.n_nodes = n_nodes;
    *out = E.release();
    return EHM_OK;
}

int ehm_explicit_eval_batch(ehm_explicit* E, int64_t n, const double* x, double* u,
                            int32_t* leaf, int32_t* visited, double* kernel_seconds) {
    if (!E || !x || !u || n < 0) return x_err.fail(EHM_E_INVALID, "bad argument");
    if (n == 0) return EHM_OK;
    hipError_t e = hipSetDevice(E->device);
    if (e != hipSuccess) return x_err.fail(EHM_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    const int p = E->d.p, n_u = E->d.n_u;
    if ((size_t)n > E->cap) {
        for (DevBuf* b : {&E->x, &E->u, &E->leaf, &E->depth, &E->root}) b->reset();
        E->cap = 0;
        if (E->x.alloc((size_t)n * p * sizeof(double)) != hipSuccess ||
            E->u.alloc((size_t)n * n_u * sizeof(double)) != hipSuccess ||
            E->leaf.alloc((size_t)n * sizeof(int32_t)) != hipSuccess ||
            E->depth.alloc((size_t)n * sizeof(int32_t)) != hipSuccess ||
            E->root.alloc((size_t)n * sizeof(int32_t)) != hipSuccess)
            return x_err.fail(EHM_E_HIP, "out of device memory for %lld queries", (long long)n);
        E->cap = (size_t)n;
    }
    EventPair ev;
    EHM_HIP_TRY(x_err, hipMemcpyAsync(E->x.ptr, x, (size_t)n * p * sizeof(double),
                                      hipMemcpyHostToDevice, E->stream));
    (void)hipEventRecord(ev.e0, E->stream);
    // long spines: the visibility walk over the roots finds the root first (locate_off: the
    // reference's serial walk for every state)
    const bool locate = E->nbr && !locate_off();
    if (locate)
        hipLaunchKernelGGL(k_explicit_locate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           E->stream, E->d, (long long)n, E->x.as<const double>(),
                           E->nbr.as<const int32_t>(), E->root.as<int32_t>());
    hipLaunchKernelGGL(k_explicit_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       E->stream, E->d, (long long)n, E->x.as<const double>(), E->u.as<double>(),
                       E->leaf.as<int32_t>(), E->depth.as<int32_t>(),
                       locate ? E->root.as<const int32_t>() : (const int32_t*)nullptr);
    (void)hipEventRecord(ev.e1, E->stream);
    EHM_HIP_TRY(x_err, hipGetLastError());
    EHM_HIP_TRY(x_err, hipMemcpyAsync(u, E->u.ptr, (size_t)n * n_u * sizeof(double),
                                      hipMemcpyDeviceToHost, E->stream));
    if (leaf)
        EHM_HIP_TRY(x_err, hipMemcpyAsync(leaf, E->leaf.ptr, (size_t)n * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, E->stream));
    if (visited)
        EHM_HIP_TRY(x_err, hipMemcpyAsync(visited, E->depth.ptr, (size_t)n * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, E->stream));
    EHM_HIP_TRY(x_err, hipStreamSynchronize(E->stream));
    ev.seconds(kernel_seconds);
    return EHM_OK;
}

int ehm_explicit_set_costs(ehm_explicit* E, const double* vcost, const uint8_t* flags) {
    if (!E || !vcost || !flags) return x_err.fail(EHM_E_INVALID, "set_costs: a required array is "
                                                  "NULL");
    EHM_HIP_TRY(x_err, hipSetDevice(E->device));
    const size_t n = (size_t)E->d.n_nodes;
    DevBuf c, f;        // the handle keeps its earlier pair if an upload fails
    EHM_HIP_TRY(x_err, c.upload(vcost, n * (size_t)(E->d.p + 1) * sizeof(double)));
    EHM_HIP_TRY(x_err, f.upload(flags, n * sizeof(uint8_t)));
    E->vcost = std::move(c);
    E->nflags = std::move(f);
    return EHM_OK;
}

int ehm_explicit_records(ehm_explicit* E, double* rec) {
    if (!E || !rec) return x_err.fail(EHM_E_INVALID, "records: bad argument");
    EHM_HIP_TRY(x_err, hipSetDevice(E->device));
    const size_t w = (size_t)(E->d.p + E->d.p * E->d.p) * sizeof(double);
    EHM_HIP_TRY(x_err, hipMemcpy2D(rec, w, E->rec.ptr, (size_t)E->d.rec_stride * sizeof(double), w,
                                   (size_t)E->d.n_nodes, hipMemcpyDeviceToHost));
    return EHM_OK;
}

int ehm_explicit_set_plant(ehm_explicit* E, int32_t n_modes, const double* A, const double* B,
                           const double* w, int32_t n_d, const double* Emat,
                           const int32_t* region_rows, const double* H, const double* h,
                           int32_t n_g, const double* Gx, const double* gx,
                           const int32_t* node_mode, int32_t cost_kind, const double* Q,
                           const double* R) {
    if (!E) return x_err.fail(EHM_E_INVALID, "set_plant: a required array is NULL");
    return install_plant(E->ro, x_err, E->device, E->d.p, E->d.n_u, E->d.n_nodes, "node",
                         "set_plant", n_modes, EHM_R_MAX_MODES, A, B, w, n_g, Gx, gx, node_mode,
                         cost_kind, Q, R, nullptr, [&](Pack& pk, DevPlant& pl, int p, int) {
                             return pack_nominal(x_err, pk, pl, p, n_modes, n_d, Emat, region_rows,
                                                 H, h);
                         });
}

int ehm_explicit_set_plant_guarded(ehm_explicit* E, int32_t n_modes, const double* A,
                                   const double* B, const double* w, int32_t substeps,
                                   int32_t n_guards, const int32_t* guard_mode,
                                   const int32_t* guard_row0, const double* ga, const double* gb,
                                   const double* gc, const double* gt, const int32_t* strict,
                                   int32_t default_mode, int32_t n_g, const double* Gx,
                                   const double* gx, const int32_t* node_mode, int32_t cost_kind,
                                   const double* Q, const double* R) {
    if (!E) return x_err.fail(EHM_E_INVALID, "set_plant_guarded: a required array is NULL");
    DevGuard gd{};
    return install_plant(E->ro, x_err, E->device, E->d.p, E->d.n_u, E->d.n_nodes, "node",
                         "set_plant_guarded", n_modes, EHM_G_MAX_MODES, A, B, w, n_g, Gx, gx,
                         node_mode, cost_kind, Q, R, &gd, [&](Pack& pk, DevPlant&, int p, int n_u) {
                             return pack_guarded(x_err, pk, gd, p, n_u, n_modes, substeps, n_guards,
                                                 guard_mode, guard_row0, ga, gb, gc, gt, strict,
                                                 default_mode);
                         });
}

int ehm_explicit_rollout(ehm_explicit* E, int64_t n, int32_t T, const double* x0,
                         const double* d, const double* v, double tol_exit, double* x_traj,
                         double* u_traj, int32_t* leaf_traj, double* x_final, int32_t* steps,
                         int32_t* status, double* cost, double* u_norm_sum,
                         double* max_violation, double* kernel_seconds) {
    if (!E) return x_err.fail(EHM_E_INVALID, "rollout: bad argument");
    return rollout_run(E->ro, x_err, E->device, E->stream, E->d, E->d.p, E->d.n_u,
                       (E->nbr && !locate_off()) ? E->nbr.as<const int32_t>() : nullptr,
                       k_rollout_table, n, T, x0, d, v, tol_exit, x_traj, u_traj, leaf_traj,
                       x_final, steps, status, cost, u_norm_sum, max_violation, kernel_seconds,
                       nullptr);
}

int ehm_explicit_set_noise(ehm_explicit* E, int32_t n_terms, const int32_t* desc,
                           const double* data, int32_t n_data, int32_t n_d) {
    if (!E) return x_err.fail(EHM_E_INVALID, "set_noise: no handle");
    return install_noise(E->ro, x_err, E->device, E->d.p, E->d.n_u, n_terms, desc, data, n_data,
                         n_d);
}

int ehm_explicit_rollout_noisy(ehm_explicit* E, int64_t n, int32_t T, const double* x0,
                               uint64_t seed, uint64_t traj0, double tol_exit, double* x_traj,
                               double* u_traj, int32_t* leaf_traj, double* v_traj,
                               double* e_traj, double* w_traj, double* x_final, int32_t* steps,
                               int32_t* status, double* cost, double* u_norm_sum,
                               double* max_violation, double* kernel_seconds) {
    if (!E) return x_err.fail(EHM_E_INVALID, "rollout_noisy: no handle");
    const int rc = noisy_ready(E->ro, x_err);
    if (rc != EHM_OK) return rc;
    const NoisyCall nz{seed, traj0, v_traj, e_traj, w_traj};
    return rollout_run(E->ro, x_err, E->device, E->stream, E->d, E->d.p, E->d.n_u,
                       (E->nbr && !locate_off()) ? E->nbr.as<const int32_t>() : nullptr,
                       k_rollout_table, n, T, x0, nullptr, nullptr, tol_exit, x_traj, u_traj,
                       leaf_traj, x_final, steps, status, cost, u_norm_sum, max_violation,
                       kernel_seconds, &nz);
}

int ehm_philox_batch(int64_t n, const uint64_t* counters, const uint64_t* key, uint64_t* out) {
    if (n < 0 || (n > 0 && (!counters || !key || !out)))
        return x_err.fail(EHM_E_INVALID, "philox_batch: bad argument");
    if (n == 0) return EHM_OK;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return x_err.fail(EHM_E_NO_DEVICE, "philox_batch: %s",
                                           hipGetErrorString(e));
    const size_t bytes = (size_t)n * 4 * sizeof(uint64_t);
    DevBuf dc, dout;
    EHM_HIP_TRY(x_err, dc.upload(counters, bytes));
    EHM_HIP_TRY(x_err, dout.alloc(bytes));
    hipLaunchKernelGGL(k_philox_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0,
                       (long long)n, dc.as<const uint64_t>(), key[0], key[1],
                       dout.as<uint64_t>());
    EHM_HIP_TRY(x_err, hipGetLastError());
    EHM_HIP_TRY(x_err, hipMemcpy(out, dout.ptr, bytes, hipMemcpyDeviceToHost));
    return EHM_OK;
}

}  // extern "C"
