// The explicit law compiled into a hyperplane tree with affine leaf gains.
//
// Every split of a partition tree is a bisection: the two children share a face, so for a state
// inside the parent "is it in the left child" is the sign of ONE affine function (p + 1 doubles
// instead of the child's p + p^2 record), and the interpolation of the vertex inputs over a leaf
// is an affine map u = u_0 + K (x - v_0).  ehm_compiled_create classifies the nodes of an
// ehm_explicit handle on the device and writes
//   node     [n_int][NS]   [a (p) | b | (left, right) int32 pair], 64 B (p <= 6) or 128 B; a child
//                          index >= 0 is an internal node, < 0 is ~leaf.  PLANE node: left iff
//                          ((0 + a_0 x_0) + .. + a_(p-1) x_(p-1)) + b >= -eps.  TEST node (children
//                          that are no bisection, the data-less spine of a nested tree): a = +0.0
//                          everywhere (no plane has a zero normal), b = its row of test_rec; left iff
//                          the left child's simplex holds x, the reference's rule verbatim.
//   leaf_rec [n_leaf][LS]  [v_0 (p) | u_0 (n_u) | K (n_u x p)], leaf_node [n_leaf] source node id
//   test_rec / root_rec    [v_0 | inv(E)] of a test node's left child / of every root
//   root_entry [n_roots]   a root's index (internal or ~leaf); nbr: the face adjacency of the roots
// Internal nodes and leaves keep the source order, children come after their parents: a walk's
// index grows strictly, so no array -- compiled here or imported from a file -- can hold a cycle.
// One level of the walk is one dependent load (the source evaluator: child pair, then the child's
// record).  The handle owns copies of all it needs: it outlives its source.
// ehm_compiled_create_opts with EHM_COMPILE_SPINE_ROOTS turns the chain of test nodes on top of a
// nested tree (node 0 and on along the right children) into the root table instead: those nodes get
// no record, and what hangs off them is the law's roots, with the locator's adjacency from 128 on.
//
// k_compiled_rollout closes the loop around the compiled law (one thread per trajectory, the T steps
// in the kernel): the root as k_compiled_locate / k_compiled_eval choose it, the exit test on the
// root's weights, the walk and the leaf map of k_compiled_eval, then the step of ehm_rollout_dev.h
// in the mode leaf_mode gives -- a rollout attachment of the handle like the plant, not part of the
// law (ehm_compiled_set_plant).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_compiled_dev.h"
#include "ehm_compiled_view.h"
#include "ehm_explicit_view.h"
#include "ehm_host.h"

#define EHM_C_VERSION 1          // format of the arrays (ehm_compiled_export / _import)
#define EHM_C_HEADER 12          // int64 entries of the header

// the kernels of the single-precision law (ehm_compiled32.hip)
extern "C" const ehm::Compiled32Api* ehm_compiled32_api();

namespace {

// ---- compile kernels: one thread per source node -------------------------------------------------

// cls[k]: -1 leaf; 0 test node; 1 + j plane node whose split face is the face of the left child
// opposite its vertex j.  Vertices are compared by value (-0.0 == 0.0).
__global__ void k_compiled_classify(long long n_nodes, int p, const int2* __restrict__ child,
                                    const double* __restrict__ vertices,
                                    int32_t* __restrict__ cls) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_nodes) return;
    const int2 ch = child[k];
    if (ch.x < 0) {
        cls[k] = -1;
        return;
    }
    const size_t vs = (size_t)(p + 1) * p;
    const double* V = vertices + (size_t)k * vs;
    const double* L = vertices + (size_t)ch.x * vs;
    const double* R = vertices + (size_t)ch.y * vs;
    int i = -1, j = -1, nl = 0, nr = 0;
    for (int v = 0; v <= p; ++v) {
        bool dl = false, dr = false;
        for (int c = 0; c < p; ++c) {
            dl = dl || !(L[v * p + c] == V[v * p + c]);
            dr = dr || !(R[v * p + c] == V[v * p + c]);
        }
        if (dl) {
            ++nl;
            i = v;
        }
        if (dr) {
            ++nr;
            j = v;
        }
    }
    bool plane = nl == 1 && nr == 1 && i != j;
    if (plane)
        for (int c = 0; c < p; ++c) plane = plane && (L[i * p + c] == R[j * p + c]);
    cls[k] = plane ? 1 + j : 0;
}

// what the host writes over the class of a spine node that became the root table
// (EHM_COMPILE_SPINE_ROOTS)
#define CLS_SPINE (-2)

struct CompileArgs {
    long long n_nodes;
    int p, n_u, rec_stride, node_stride, leaf_stride, side_stride;
    const int2* child;
    const double* rec;          // the source's [v0 | inv(E)] records
    const double* vinput;
    const int32_t* cls;
    const int32_t* newid;       // internal index, or ~leaf index
    const int32_t* test_idx;    // row of test_rec (test nodes)
    double *node, *leaf_rec, *test_rec;
    int32_t* leaf_node;
};

__global__ void k_compiled_write(CompileArgs A) {
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_nodes) return;
    const int p = A.p, n_u = A.n_u;
    if (A.cls[k] == CLS_SPINE) return;      // its children are roots of the law: no record
    const int id = A.newid[k];
    if (id < 0) {
        // leaf: u = u_0 + K (x - v_0), K = (U_1..p - u_0)^T inv(E)
        const int l = ~id;
        const double* r = A.rec + (size_t)k * A.rec_stride;
        const double* U = A.vinput + (size_t)k * (p + 1) * n_u;
        double* out = A.leaf_rec + (size_t)l * A.leaf_stride;
        for (int c = 0; c < p; ++c) out[c] = r[c];
        for (int c = 0; c < n_u; ++c) out[p + c] = U[c];
        for (int c = 0; c < n_u; ++c)
            for (int q = 0; q < p; ++q) {
                double s = 0.0;
                for (int i = 0; i < p; ++i) s += (U[(i + 1) * n_u + c] - U[c]) * r[p + i * p + q];
                out[p + n_u + c * p + q] = s;
            }
        for (int c = p + n_u + n_u * p; c < A.leaf_stride; ++c) out[c] = 0.0;
        A.leaf_node[l] = (int32_t)k;
        return;
    }
    const int2 ch = A.child[k];
    double* out = A.node + (size_t)id * A.node_stride;
    const double* r = A.rec + (size_t)ch.x * A.rec_stride;        // the left child's record
    const int cls = A.cls[k];
    for (int c = 0; c < A.node_stride; ++c) out[c] = 0.0;
    if (cls == 0) {
        const int t = A.test_idx[k];
        out[p] = (double)t;
        double* tr = A.test_rec + (size_t)t * A.side_stride;
        for (int c = 0; c < p + p * p; ++c) tr[c] = r[c];
        for (int c = p + p * p; c < A.side_stride; ++c) tr[c] = 0.0;
    } else {
        // the weight of x for vertex j of the left child, as a . x + b
        const int j = cls - 1;
        double b = (j == 0) ? 1.0 : 0.0;
        for (int c = 0; c < p; ++c) {
            double a = 0.0;
            if (j == 0)
                for (int q = 0; q < p; ++q) a -= r[p + q * p + c];
            else
                a = r[p + (j - 1) * p + c];
            out[c] = a;
            b -= a * r[c];
        }
        out[p] = b;
    }
    int2* cp = reinterpret_cast<int2*>(out + p + 1);
    *cp = make_int2(A.newid[ch.x], A.newid[ch.y]);
}

// the source's records of the nodes ids[0..n_roots-1] (ids nullptr: rows 0..n_roots-1), repacked
// at the side stride
__global__ void k_compiled_roots(int n_roots, int p, int rec_stride, int side_stride,
                                 const int32_t* __restrict__ ids, const double* __restrict__ rec,
                                 double* __restrict__ root_rec) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_roots) return;
    const size_t from = ids ? (size_t)ids[k] : (size_t)k;
    for (int c = 0; c < side_stride; ++c)
        root_rec[(size_t)k * side_stride + c] = c < p + p * p ? rec[from * rec_stride + c] : 0.0;
}

// ---- evaluation ----------------------------------------------------------------------------------

// k_explicit_locate on the compiled law's own root records: a visibility walk over the face
// adjacency, root[q] = found | steps << 20, or -1 (the serial walk decides).
template <int P>
__global__ __launch_bounds__(256) void k_compiled_locate(DevCompiled C, long long n,
                                                         const double* __restrict__ X,
                                                         const int32_t* __restrict__ nbr,
                                                         int32_t* __restrict__ root) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double x[P];
#pragma unroll
    for (int c = 0; c < P; ++c) x[c] = X[q * P + c];
    int k = (int)(q % C.n_roots);
    int found = -1, steps = 0;
    for (int step = 0; step < EHM_C_STEPS; ++step) {
        ++steps;
        const double* r = C.root_rec + (size_t)k * C.side_stride;
        double d[P];
#pragma unroll
        for (int c = 0; c < P; ++c) d[c] = x[c] - r[c];
        double alpha[P], s = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double a = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) a = fma(r[P + i * P + c], d[c], a);
            alpha[i] = a;
            s += a;
        }
        double lo = 1.0 - s;
        int at = 0;
#pragma unroll
        for (int i = 0; i < P; ++i)
            if (alpha[i] < lo) {
                lo = alpha[i];
                at = i + 1;
            }
        if (lo > EHM_C_STRICT) {
            found = k;
            break;
        }
        if (lo >= -EHM_C_STRICT) break;
        const int k2 = nbr[(size_t)k * (P + 1) + at];
        if (k2 < 0) break;
        k = k2;
    }
    root[q] = (found < 0) ? -1 : (found | (steps << 20));
}

template <int P>
__global__ __launch_bounds__(256) void k_compiled_eval(DevCompiled C, long long n,
                                                       const double* __restrict__ X,
                                                       double* __restrict__ U,
                                                       int32_t* __restrict__ leaf,
                                                       int32_t* __restrict__ depth_out,
                                                       const int32_t* __restrict__ root) {
#pragma clang fp contract(off)
    constexpr int NS = P <= 6 ? 8 : 16;         // node_stride_of(P)
    constexpr int NL = (P + 3) / 2;             // 16-byte loads that cover [a | b | children]
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
    int k = C.root_entry[kr];
    // the walk: one record per level, plane and children together
    while (k >= 0) {
        const double2* nd = reinterpret_cast<const double2*>(C.node + (size_t)k * NS);
        double r[2 * NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const double2 t = nd[i];
            r[2 * i] = t.x;
            r[2 * i + 1] = t.y;
        }
        ++visited;
        const long long ch = __double_as_longlong(r[P + 1]);
        long long bits = 0;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            bits |= __double_as_longlong(r[c]);
            s = s + r[c] * x[c];
        }
        s = s + r[P];
        bool go_left = s >= -EHM_C_EPS;
        if (bits == 0)      // test node: the reference's containment test of the left child
            go_left = c_contains<P>(C.test_rec + (size_t)(int)r[P] * C.side_stride, x);
        k = go_left ? (int)(ch & 0xffffffffll) : (int)(ch >> 32);
    }
    const int l = ~k;
    const double* lr = C.leaf_rec + (size_t)l * C.leaf_stride;
    const double2* lv = reinterpret_cast<const double2*>(lr);
    double d[P];
#pragma unroll
    for (int c = 0; c + 1 < P; c += 2) {
        const double2 t = lv[c / 2];
        d[c] = x[c] - t.x;
        d[c + 1] = x[c + 1] - t.y;
    }
    if (P % 2) d[P - 1] = x[P - 1] - lr[P - 1];
    const int n_u = C.n_u;
    const double* Kc = lr + P + n_u;
    for (int c = 0; c < n_u; ++c) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) t = t + Kc[c * P + i] * d[i];
        U[q * n_u + c] = lr[P + c] + t;
    }
    if (leaf) leaf[q] = C.leaf_node[l];
    if (depth_out) depth_out[q] = visited;
}

// ---- dispatch tables (k_compiled_rollout: ehm_compiled_dev.h) ------------------------------------------

typedef void (*rollout_fn)(DevCompiled, DevPlant, RollArgs, DevNoise, DevGuard);
#define EHM_R_NU(P, K) &k_compiled_rollout<double, P, 1, K>, &k_compiled_rollout<double, P, 2, K>, \
                       &k_compiled_rollout<double, P, 3, K>, &k_compiled_rollout<double, P, 4, K>
#define EHM_R_ALL(K) {{EHM_R_NU(1, K)}, {EHM_R_NU(2, K)}, {EHM_R_NU(3, K)}, {EHM_R_NU(4, K)}, \
                      {EHM_R_NU(5, K)}, {EHM_R_NU(6, K)}, {EHM_R_NU(7, K)}, {EHM_R_NU(8, K)}}
// [kind][p - 1][n_u - 1]
const rollout_fn k_rollout_table[PK_KINDS][EHM_CP][EHM_R_MAX_NU] = {
    EHM_R_ALL(PK_NOMINAL), EHM_R_ALL(PK_NOISY), EHM_R_ALL(PK_GUARDED)};
#undef EHM_R_ALL
#undef EHM_R_NU

// the same table of the single law's instances: the kernels of ehm_compiled32.hip under the types
// rollout_run launches them with
typedef void (*rollout32_fn)(DevLaw<float>, DevPlant, RollArgs, DevNoise, DevGuard);
struct Rollout32Table {
    rollout32_fn fn[PK_KINDS][EHM_CP][EHM_R_MAX_NU];
    Rollout32Table() {
        const ehm::Compiled32Api* api = ehm_compiled32_api();
        for (int k = 0; k < PK_KINDS; ++k)
            for (int p = 0; p < EHM_CP; ++p)
                for (int u = 0; u < EHM_R_MAX_NU; ++u)
                    fn[k][p][u] = reinterpret_cast<rollout32_fn>(
                        const_cast<void*>(api->rollout[k][p][u]));
    }
};

typedef void (*locate_fn)(DevCompiled, long long, const double*, const int32_t*, int32_t*);
typedef void (*eval_fn)(DevCompiled, long long, const double*, double*, int32_t*, int32_t*,
                        const int32_t*);
const locate_fn k_locate_table[EHM_CP] = {
    &k_compiled_locate<1>, &k_compiled_locate<2>, &k_compiled_locate<3>, &k_compiled_locate<4>,
    &k_compiled_locate<5>, &k_compiled_locate<6>, &k_compiled_locate<7>, &k_compiled_locate<8>};
const eval_fn k_eval_table[EHM_CP] = {
    &k_compiled_eval<1>, &k_compiled_eval<2>, &k_compiled_eval<3>, &k_compiled_eval<4>,
    &k_compiled_eval<5>, &k_compiled_eval<6>, &k_compiled_eval<7>, &k_compiled_eval<8>};

bool locate_off() {
    static const bool off = [] {
        const char* e = getenv("EHM_EXPLICIT_LOCATE");
        return e && atoi(e) == 0;
    }();
    return off;
}

thread_local ehm_err_channel c_err;

// header of the arrays: [version, p, n_u, n_roots, n_int, n_leaf, n_test, node_stride,
// leaf_stride, side_stride, has_nbr, n_source_nodes]
enum { H_VERSION, H_P, H_NU, H_ROOTS, H_INT, H_LEAF, H_TEST, H_NS, H_LS, H_SS, H_NBR, H_SRC };

template <class T>
bool all_finite(const T* a, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// a single law holds zeros and normal floats only: its arithmetic must not depend on how a device
// treats subnormal numbers
bool all_normal(const float* a, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (a[i] != 0.0f && !std::isnormal(a[i])) return false;
    return true;
}

bool entry_ok(int64_t c, int64_t n_int, int64_t n_leaf) {
    return c >= 0 ? c < n_int : ~c < n_leaf;
}

// A file is untrusted input: every index the kernels follow is checked here.  T = float: the arrays
// of a single law (node and leaf_rec in floats at their own strides, no test nodes, no zero normal,
// no subnormal value).
template <class T>
int validate(const int64_t* h, const T* node, const T* leaf_rec,
             const int32_t* leaf_node, const double* test_rec, const double* root_rec,
             const int32_t* root_entry, const int32_t* nbr) {
    constexpr bool SINGLE = sizeof(T) == sizeof(float);
    if (!h) return c_err.fail(EHM_E_INVALID, "compiled law: no header");
    if (h[H_VERSION] != EHM_C_VERSION)
        return c_err.fail(EHM_E_INVALID, "compiled law: format version %lld (this library reads "
                          "%d)", (long long)h[H_VERSION], EHM_C_VERSION);
    const int64_t p = h[H_P], n_u = h[H_NU], n_roots = h[H_ROOTS], n_int = h[H_INT],
                  n_leaf = h[H_LEAF], n_test = h[H_TEST];
    if (p < 1 || p > EHM_CP || n_u < 1 || n_u > (1 << 20))
        return c_err.fail(EHM_E_INVALID, "compiled law: p = %lld (1..%d), n_u = %lld", (long long)p,
                          EHM_CP, (long long)n_u);
    const int64_t lim = (int64_t)1 << 31;
    if (n_roots < 1 || n_int < 0 || n_leaf < 1 || n_test < 0 || n_test > n_int ||
        n_int >= lim || n_leaf >= lim || n_roots > n_int + n_leaf || h[H_SRC] < n_leaf ||
        h[H_SRC] >= lim)
        return c_err.fail(EHM_E_INVALID, "compiled law: bad counts");
    if (SINGLE && n_test > 0)
        return c_err.fail(EHM_E_INVALID, "compiled law: a single-precision law has no test nodes "
                          "(%lld)", (long long)n_test);
    const int ns = SINGLE ? node_stride32_of((int)p) : node_stride_of((int)p),
              ls = SINGLE ? leaf_stride32_of((int)p, (int)n_u) : leaf_stride_of((int)p, (int)n_u),
              ss = side_stride_of((int)p);
    if (h[H_NS] != ns || h[H_LS] != ls || h[H_SS] != ss)
        return c_err.fail(EHM_E_INVALID, "compiled law: record strides %lld / %lld / %lld, not %d "
                          "/ %d / %d", (long long)h[H_NS], (long long)h[H_LS], (long long)h[H_SS],
                          ns, ls, ss);
    if (h[H_NBR] != 0 && h[H_NBR] != 1)
        return c_err.fail(EHM_E_INVALID, "compiled law: bad adjacency flag");
    if (h[H_NBR] && (n_roots < EHM_C_LOCATE_MIN || n_roots >= (1 << 20)))
        return c_err.fail(EHM_E_INVALID, "compiled law: an adjacency table with %lld roots",
                          (long long)n_roots);
    if ((n_int && !node) || !leaf_rec || !leaf_node || (n_test && !test_rec) || !root_rec ||
        !root_entry || (h[H_NBR] && !nbr))
        return c_err.fail(EHM_E_INVALID, "compiled law: an array is missing");
    for (int64_t k = 0; k < n_int; ++k) {
        const T* r = node + (size_t)k * ns;
        if (!all_finite(r, (size_t)p + 1))
            return c_err.fail(EHM_E_INVALID, "compiled law: node %lld is not finite", (long long)k);
        int32_t ch[2];
        std::memcpy(ch, r + p + 1, sizeof ch);
        for (int s = 0; s < 2; ++s)
            if (!entry_ok(ch[s], n_int, n_leaf) || (ch[s] >= 0 && ch[s] <= k))
                return c_err.fail(EHM_E_INVALID, "compiled law: node %lld has child %d (children "
                                  "come after their parents)", (long long)k, (int)ch[s]);
        bool zero = true, bits = true;
        for (int c = 0; c < p; ++c) {
            zero = zero && r[c] == 0.0;
            bits = bits && !std::signbit(r[c]);
        }
        if (zero && !(bits && r[p] >= 0.0 && r[p] < (double)n_test && r[p] == std::floor(r[p])))
            return c_err.fail(EHM_E_INVALID, "compiled law: node %lld has a zero normal and names "
                              "no test record", (long long)k);
    }
    if constexpr (SINGLE) {
        bool normal = all_normal(leaf_rec, (size_t)n_leaf * ls);
        for (int64_t k = 0; k < n_int && normal; ++k)
            normal = all_normal(node + (size_t)k * ns, (size_t)p + 1);
        if (!normal)
            return c_err.fail(EHM_E_INVALID, "compiled law: a single-precision record holds a "
                              "subnormal or non-finite value");
    }
    if (!all_finite(leaf_rec, (size_t)n_leaf * ls) || (n_test && !all_finite(test_rec, (size_t)n_test * ss)) ||
        !all_finite(root_rec, (size_t)n_roots * ss))
        return c_err.fail(EHM_E_INVALID, "compiled law: a record is not finite");
    for (int64_t l = 0; l < n_leaf; ++l)
        if (leaf_node[l] < 0 || leaf_node[l] >= h[H_SRC])
            return c_err.fail(EHM_E_INVALID, "compiled law: leaf %lld names node %d of %lld",
                              (long long)l, (int)leaf_node[l], (long long)h[H_SRC]);
    for (int64_t r = 0; r < n_roots; ++r)
        if (!entry_ok(root_entry[r], n_int, n_leaf))
            return c_err.fail(EHM_E_INVALID, "compiled law: root %lld enters at %d", (long long)r,
                              (int)root_entry[r]);
    if (h[H_NBR])
        for (int64_t i = 0; i < n_roots * (p + 1); ++i)
            if (nbr[i] < -1 || nbr[i] >= n_roots)
                return c_err.fail(EHM_E_INVALID, "compiled law: adjacency entry %lld is %d",
                                  (long long)i, (int)nbr[i]);
    return EHM_OK;
}

}  // namespace

struct ehm_compiled {
    int device = 0;
    bool single = false;        // node and leaf_rec hold floats (ehm_compiled_narrow, _import_single)
    DevCompiled d{};            // a single law: its root arrays only (the locator)
    DevLaw<float> d32{};        // a single law
    int64_t h[EHM_C_HEADER] = {};
    int64_t source_bytes = 0;
    DevBuf node, leaf_rec, leaf_node, test_rec, root_rec, root_entry, nbr;
    DevBuf x, u, leaf, depth, root;         // ehm_compiled_eval_batch, cap queries
    size_t cap = 0;
    RolloutAttach ro;   // plant, leaf modes and model of the rollouts: not part of the law
    Stream stream;

    size_t scalar() const { return single ? sizeof(float) : sizeof(double); }
    size_t node_bytes() const { return (size_t)h[H_INT] * h[H_NS] * scalar(); }
    size_t leaf_bytes() const { return (size_t)h[H_LEAF] * h[H_LS] * scalar(); }
    size_t leaf_node_bytes() const { return (size_t)h[H_LEAF] * sizeof(int32_t); }
    size_t test_bytes() const { return (size_t)h[H_TEST] * h[H_SS] * sizeof(double); }
    size_t root_bytes() const { return (size_t)h[H_ROOTS] * h[H_SS] * sizeof(double); }
    size_t entry_bytes() const { return (size_t)h[H_ROOTS] * sizeof(int32_t); }
    size_t nbr_bytes() const {
        return h[H_NBR] ? (size_t)h[H_ROOTS] * (h[H_P] + 1) * sizeof(int32_t) : 0;
    }
    size_t bytes() const {
        return node_bytes() + leaf_bytes() + leaf_node_bytes() + test_bytes() + root_bytes() +
               entry_bytes() + nbr_bytes();
    }
    void bind() {
        d.node = single ? nullptr : node.as<const double>();
        d.leaf_rec = single ? nullptr : leaf_rec.as<const double>();
        d.leaf_node = leaf_node.as<const int32_t>();
        d.test_rec = test_rec.as<const double>();
        d.root_rec = root_rec.as<const double>();
        d.root_entry = root_entry.as<const int32_t>();
        d.leaf_stride = (int)h[H_LS];
        d.side_stride = (int)h[H_SS];
        d.p = (int)h[H_P];
        d.n_u = (int)h[H_NU];
        d.n_roots = (int)h[H_ROOTS];
        d32 = DevLaw<float>{single ? node.as<const float>() : nullptr,
                            single ? leaf_rec.as<const float>() : nullptr,
                            d.leaf_node, d.test_rec, d.root_rec, d.root_entry,
                            d.leaf_stride, d.side_stride, d.p, d.n_u, d.n_roots};
    }
};

void ehm_compiled_get_view(const ehm_compiled* C, ehm_compiled_view* out) {
    out->device = C->device;
    out->single = C->single;
    out->node = C->node.ptr;
    out->leaf_rec = C->leaf_rec.ptr;
    out->leaf_node = C->leaf_node.as<const int32_t>();
    out->root_entry = C->root_entry.as<const int32_t>();
    out->p = (int)C->h[H_P];
    out->n_u = (int)C->h[H_NU];
    out->node_stride = (int)C->h[H_NS];
    out->leaf_stride = (int)C->h[H_LS];
    out->n_roots = C->h[H_ROOTS];
    out->n_int = C->h[H_INT];
    out->n_leaf = C->h[H_LEAF];
    out->n_test = C->h[H_TEST];
    out->stream = C->stream;
    out->root_rec = C->root_rec.as<const double>();
    out->nbr = C->h[H_NBR] ? C->nbr.as<const int32_t>() : nullptr;
    out->side_stride = (int)C->h[H_SS];
}

namespace {

typedef std::unique_ptr<ehm_compiled, int (*)(ehm_compiled*)> LawPtr;

// ehm_compiled_import / _import_single
template <class T>
int import_law(int device, const int64_t* header, const T* node, const T* leaf_rec,
               const int32_t* leaf_node, const double* test_rec, const double* root_rec,
               const int32_t* root_entry, const int32_t* nbr, ehm_compiled** out) {
    if (!out) return c_err.fail(EHM_E_INVALID, "import: bad argument");
    *out = nullptr;
    const int rc = validate(header, node, leaf_rec, leaf_node, test_rec, root_rec, root_entry, nbr);
    if (rc != EHM_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return c_err.fail(EHM_E_NO_DEVICE, "no HIP device %d (libehmpc has no CPU fallback)",
                          device);
    LawPtr C(new ehm_compiled(), ehm_compiled_destroy);
    C->device = device;
    C->single = sizeof(T) == sizeof(float);
    std::memcpy(C->h, header, sizeof C->h);
    EHM_HIP_TRY(c_err, hipSetDevice(device));
    EHM_HIP_TRY(c_err, C->stream.create());
    EHM_HIP_TRY(c_err, C->node.upload(node, C->node_bytes()));
    EHM_HIP_TRY(c_err, C->leaf_rec.upload(leaf_rec, C->leaf_bytes()));
    EHM_HIP_TRY(c_err, C->leaf_node.upload(leaf_node, C->leaf_node_bytes()));
    EHM_HIP_TRY(c_err, C->test_rec.upload(test_rec, C->test_bytes()));
    EHM_HIP_TRY(c_err, C->root_rec.upload(root_rec, C->root_bytes()));
    EHM_HIP_TRY(c_err, C->root_entry.upload(root_entry, C->entry_bytes()));
    if (header[H_NBR]) EHM_HIP_TRY(c_err, C->nbr.upload(nbr, C->nbr_bytes()));
    C->bind();
    *out = C.release();
    return EHM_OK;
}

// ehm_compiled_export / _export_single
int export_law(ehm_compiled* C, bool single, void* node, void* leaf_rec, int32_t* leaf_node,
               double* test_rec, double* root_rec, int32_t* root_entry, int32_t* nbr) {
    if (!C) return c_err.fail(EHM_E_INVALID, "export: bad argument");
    if (C->single != single)
        return c_err.fail(EHM_E_INVALID, "export: the law is in %s precision "
                          "(ehm_compiled_export%s)", C->single ? "single" : "double",
                          C->single ? "_single" : "");
    EHM_HIP_TRY(c_err, hipSetDevice(C->device));
    struct {
        void* host;
        const DevBuf* buf;
        size_t bytes;
    } parts[] = {{node, &C->node, C->node_bytes()},
                 {leaf_rec, &C->leaf_rec, C->leaf_bytes()},
                 {leaf_node, &C->leaf_node, C->leaf_node_bytes()},
                 {test_rec, &C->test_rec, C->test_bytes()},
                 {root_rec, &C->root_rec, C->root_bytes()},
                 {root_entry, &C->root_entry, C->entry_bytes()},
                 {nbr, &C->nbr, C->nbr_bytes()}};
    for (const auto& part : parts)
        if (part.host && part.bytes)
            EHM_HIP_TRY(c_err, hipMemcpy(part.host, part.buf->ptr, part.bytes,
                                         hipMemcpyDeviceToHost));
    return EHM_OK;
}

}  // namespace

int ehm_compiled_adopt(const ehm_compiled* like, int64_t n_int, int64_t n_leaf, DevBuf& node,
                       DevBuf& leaf_rec, DevBuf& leaf_node, DevBuf& root_entry,
                       ehm_compiled** out) {
    if (!like || !out) return c_err.fail(EHM_E_INVALID, "adopt: bad argument");
    *out = nullptr;
    LawPtr C(new ehm_compiled(), ehm_compiled_destroy);
    C->device = like->device;
    C->single = like->single;
    std::memcpy(C->h, like->h, sizeof C->h);
    C->h[H_INT] = n_int;
    C->h[H_LEAF] = n_leaf;
    // a refined law (ehm_refine.hip) has leaves that share a source node: the header's node count
    // stays an upper bound of leaf_node and is never below the leaves (what an import asks)
    C->h[H_SRC] = std::max(C->h[H_SRC], n_leaf);
    C->source_bytes = like->source_bytes;
    EHM_HIP_TRY(c_err, hipSetDevice(C->device));
    EHM_HIP_TRY(c_err, C->stream.create());
    C->node = std::move(node);
    C->leaf_rec = std::move(leaf_rec);
    C->leaf_node = std::move(leaf_node);
    C->root_entry = std::move(root_entry);
    EHM_HIP_TRY(c_err, C->test_rec.alloc(0));
    EHM_HIP_TRY(c_err, C->root_rec.alloc(C->root_bytes()));
    EHM_HIP_TRY(c_err, hipMemcpy(C->root_rec.ptr, like->root_rec.ptr, C->root_bytes(),
                                 hipMemcpyDeviceToDevice));
    if (C->nbr_bytes()) {
        EHM_HIP_TRY(c_err, C->nbr.alloc(C->nbr_bytes()));
        EHM_HIP_TRY(c_err, hipMemcpy(C->nbr.ptr, like->nbr.ptr, C->nbr_bytes(),
                                     hipMemcpyDeviceToDevice));
    }
    // the check of an import, on a host copy of what the device now holds
    std::vector<char> h_node(C->node_bytes()), h_leaf(C->leaf_bytes());
    std::vector<int32_t> h_leaf_node((size_t)n_leaf), h_entry((size_t)C->h[H_ROOTS]),
        h_nbr(C->nbr_bytes() / sizeof(int32_t));
    std::vector<double> h_root(C->root_bytes() / sizeof(double));
    const int rc0 = export_law(C.get(), C->single, h_node.data(), h_leaf.data(),
                               h_leaf_node.data(), nullptr, h_root.data(), h_entry.data(),
                               h_nbr.data());
    if (rc0 != EHM_OK) return rc0;
    const int rc = C->single
        ? validate(C->h, reinterpret_cast<const float*>(h_node.data()),
                   reinterpret_cast<const float*>(h_leaf.data()), h_leaf_node.data(),
                   (const double*)nullptr, h_root.data(), h_entry.data(), h_nbr.data())
        : validate(C->h, reinterpret_cast<const double*>(h_node.data()),
                   reinterpret_cast<const double*>(h_leaf.data()), h_leaf_node.data(),
                   (const double*)nullptr, h_root.data(), h_entry.data(), h_nbr.data());
    if (rc != EHM_OK) return rc;
    C->bind();
    *out = C.release();
    return EHM_OK;
}

extern "C" {

const char* ehm_compiled_last_error(void) { return c_err.c_str(); }

int ehm_compiled_destroy(ehm_compiled* C) {
    if (!C) return EHM_OK;
    (void)hipSetDevice(C->device);
    delete C;
    return EHM_OK;
}

int ehm_compiled_create(ehm_explicit* src, const double* vertices, ehm_compiled** out,
                        double* compile_seconds) {
    return ehm_compiled_create_opts(src, vertices, 0, out, compile_seconds);
}

int ehm_compiled_create_opts(ehm_explicit* src, const double* vertices, int32_t flags,
                             ehm_compiled** out, double* compile_seconds) {
    if (!src || !vertices || !out) return c_err.fail(EHM_E_INVALID, "compile: bad argument");
    *out = nullptr;
    if (flags & ~EHM_COMPILE_SPINE_ROOTS)
        return c_err.fail(EHM_E_INVALID, "compile: unknown flags %d", (int)flags);
    ehm_explicit_view v{};
    ehm_explicit_get_view(src, &v);
    const int p = v.p, n_u = v.n_u;
    const int64_t n = v.n_nodes;
    if (n >= ((int64_t)1 << 31)) return c_err.fail(EHM_E_INVALID, "compile: %lld nodes",
                                                   (long long)n);
    LawPtr C(new ehm_compiled(), ehm_compiled_destroy);
    C->device = v.device;
    EHM_HIP_TRY(c_err, hipSetDevice(v.device));
    EHM_HIP_TRY(c_err, C->stream.create());
    const auto t0 = std::chrono::steady_clock::now();
    // the numbering (host: a prefix count over the child pairs): internal nodes and leaves in
    // source order
    std::vector<int2> ch((size_t)n);
    EHM_HIP_TRY(c_err, hipMemcpy(ch.data(), v.child, ch.size() * sizeof(int2),
                                 hipMemcpyDeviceToHost));
    std::vector<int32_t> newid((size_t)n);
    int64_t n_int = 0, n_leaf = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int2 c = ch[(size_t)k];
        if (c.x < 0) {
            newid[(size_t)k] = ~(int32_t)n_leaf++;
            continue;
        }
        if (c.x <= k || c.y <= k || c.x >= n || c.y >= n)
            return c_err.fail(EHM_E_INVALID, "compile: node %lld has children %d, %d (a compiled "
                              "law needs children after their parents)", (long long)k, c.x, c.y);
        newid[(size_t)k] = (int32_t)n_int++;
    }
    const int ns = node_stride_of(p), ls = leaf_stride_of(p, n_u), ss = side_stride_of(p);
    DevBuf d_vert, d_cls, d_newid, d_tidx;
    EHM_HIP_TRY(c_err, d_vert.upload(vertices, (size_t)n * (p + 1) * p * sizeof(double)));
    EHM_HIP_TRY(c_err, d_cls.alloc((size_t)n * sizeof(int32_t)));
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    hipLaunchKernelGGL(k_compiled_classify, grid, block, 0, C->stream, (long long)n, p, v.child,
                       d_vert.as<const double>(), d_cls.as<int32_t>());
    EHM_HIP_TRY(c_err, hipGetLastError());
    std::vector<int32_t> cls((size_t)n), tidx((size_t)n, -1);
    EHM_HIP_TRY(c_err, hipMemcpyAsync(cls.data(), d_cls.ptr, cls.size() * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, C->stream));
    EHM_HIP_TRY(c_err, hipStreamSynchronize(C->stream));
    d_vert.reset();             // the vertices were needed for the classification only
    // EHM_COMPILE_SPINE_ROOTS: the chain of test nodes from node 0 along the right children gets
    // no records, and what hangs off it becomes the roots (source ids in root_ids; empty: the
    // source's own roots).  The rest is numbered again without the chain, in source order.
    std::vector<int32_t> root_ids;
    if ((flags & EHM_COMPILE_SPINE_ROOTS) && v.n_roots == 1) {
        int64_t k = 0;
        while (ch[(size_t)k].x >= 0 && cls[(size_t)k] == 0) {
            cls[(size_t)k] = CLS_SPINE;
            root_ids.push_back(ch[(size_t)k].x);
            k = ch[(size_t)k].y;
        }
        if (!root_ids.empty()) {
            root_ids.push_back((int32_t)k);
            EHM_HIP_TRY(c_err, hipMemcpyAsync(d_cls.ptr, cls.data(), cls.size() * sizeof(int32_t),
                                              hipMemcpyHostToDevice, C->stream));
            n_int = 0;
            for (int64_t i = 0; i < n; ++i)
                if (ch[(size_t)i].x >= 0)
                    newid[(size_t)i] = cls[(size_t)i] == CLS_SPINE ? 0 : (int32_t)n_int++;
        }
    }
    const int64_t n_roots = root_ids.empty() ? (int64_t)v.n_roots : (int64_t)root_ids.size();
    EHM_HIP_TRY(c_err, d_newid.upload(newid.data(), newid.size() * sizeof(int32_t)));
    int64_t n_test = 0;
    for (int64_t k = 0; k < n; ++k)
        if (cls[(size_t)k] == 0) tidx[(size_t)k] = (int32_t)n_test++;
    EHM_HIP_TRY(c_err, d_tidx.upload(tidx.data(), tidx.size() * sizeof(int32_t)));
    int64_t* h = C->h;
    h[H_VERSION] = EHM_C_VERSION;
    h[H_P] = p;
    h[H_NU] = n_u;
    h[H_ROOTS] = n_roots;
    h[H_INT] = n_int;
    h[H_LEAF] = n_leaf;
    h[H_TEST] = n_test;
    h[H_NS] = ns;
    h[H_LS] = ls;
    h[H_SS] = ss;
    const bool own_nbr = !root_ids.empty() && n_roots >= EHM_C_LOCATE_MIN && n_roots < (1 << 20);
    h[H_NBR] = (root_ids.empty() ? v.nbr != nullptr : own_nbr) ? 1 : 0;
    h[H_SRC] = n;
    EHM_HIP_TRY(c_err, C->node.alloc(C->node_bytes()));
    EHM_HIP_TRY(c_err, C->leaf_rec.alloc(C->leaf_bytes()));
    EHM_HIP_TRY(c_err, C->leaf_node.alloc(C->leaf_node_bytes()));
    EHM_HIP_TRY(c_err, C->test_rec.alloc(C->test_bytes()));
    EHM_HIP_TRY(c_err, C->root_rec.alloc(C->root_bytes()));
    DevBuf d_root_ids;
    if (root_ids.empty()) {
        EHM_HIP_TRY(c_err, C->root_entry.upload(newid.data(), C->entry_bytes()));
        if (v.nbr) {
            EHM_HIP_TRY(c_err, C->nbr.alloc(C->nbr_bytes()));
            EHM_HIP_TRY(c_err, hipMemcpyAsync(C->nbr.ptr, v.nbr, C->nbr_bytes(),
                                              hipMemcpyDeviceToDevice, C->stream));
        }
    } else {
        std::vector<int32_t> entry(root_ids.size());
        for (size_t i = 0; i < root_ids.size(); ++i) entry[i] = newid[(size_t)root_ids[i]];
        EHM_HIP_TRY(c_err, C->root_entry.upload(entry.data(), C->entry_bytes()));
        EHM_HIP_TRY(c_err, d_root_ids.upload(root_ids.data(), root_ids.size() * sizeof(int32_t)));
        if (own_nbr) {
            std::vector<int32_t> nbr;
            ehm_root_adjacency(n_roots, p, vertices, root_ids.data(), nbr);
            EHM_HIP_TRY(c_err, C->nbr.upload(nbr.data(), C->nbr_bytes()));
        }
    }
    CompileArgs A{};
    A.n_nodes = n;
    A.p = p;
    A.n_u = n_u;
    A.rec_stride = v.rec_stride;
    A.node_stride = ns;
    A.leaf_stride = ls;
    A.side_stride = ss;
    A.child = v.child;
    A.rec = v.rec;
    A.vinput = v.vinput;
    A.cls = d_cls.as<const int32_t>();
    A.newid = d_newid.as<const int32_t>();
    A.test_idx = d_tidx.as<const int32_t>();
    A.node = C->node.as<double>();
    A.leaf_rec = C->leaf_rec.as<double>();
    A.test_rec = C->test_rec.as<double>();
    A.leaf_node = C->leaf_node.as<int32_t>();
    hipLaunchKernelGGL(k_compiled_write, grid, block, 0, C->stream, A);
    hipLaunchKernelGGL(k_compiled_roots, dim3((unsigned)((n_roots + 127) / 128)), block, 0,
                       C->stream, (int)n_roots, p, v.rec_stride, ss,
                       d_root_ids.as<const int32_t>(), v.rec, C->root_rec.as<double>());
    EHM_HIP_TRY(c_err, hipGetLastError());
    EHM_HIP_TRY(c_err, hipStreamSynchronize(C->stream));
    if (compile_seconds)
        *compile_seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    C->source_bytes = n * ((int64_t)v.rec_stride * 8 + 8 + (int64_t)(p + 1) * n_u * 8) +
                      (v.nbr ? (int64_t)v.n_roots * (p + 1) * (int64_t)sizeof(int32_t) : 0);
    C->bind();
    *out = C.release();
    return EHM_OK;
}

int ehm_compiled_validate(const int64_t* header, const double* node, const double* leaf_rec,
                          const int32_t* leaf_node, const double* test_rec,
                          const double* root_rec, const int32_t* root_entry,
                          const int32_t* nbr) {
    return validate(header, node, leaf_rec, leaf_node, test_rec, root_rec, root_entry, nbr);
}

int ehm_compiled_validate_single(const int64_t* header, const float* node, const float* leaf_rec,
                            const int32_t* leaf_node, const double* root_rec,
                            const int32_t* root_entry, const int32_t* nbr) {
    return validate(header, node, leaf_rec, leaf_node, (const double*)nullptr, root_rec, root_entry,
                    nbr);
}

int ehm_compiled_import(int device, const int64_t* header, const double* node,
                        const double* leaf_rec, const int32_t* leaf_node, const double* test_rec,
                        const double* root_rec, const int32_t* root_entry, const int32_t* nbr,
                        ehm_compiled** out) {
    return import_law(device, header, node, leaf_rec, leaf_node, test_rec, root_rec, root_entry,
                      nbr, out);
}

int ehm_compiled_import_single(int device, const int64_t* header, const float* node,
                          const float* leaf_rec, const int32_t* leaf_node, const double* root_rec,
                          const int32_t* root_entry, const int32_t* nbr, ehm_compiled** out) {
    return import_law(device, header, node, leaf_rec, leaf_node, (const double*)nullptr, root_rec,
                      root_entry, nbr, out);
}

// The single-precision law of a double law: a new handle with the records narrowed on the device.
int ehm_compiled_narrow(ehm_compiled* src, ehm_compiled** out) {
    return ehm_compiled_narrow_opts(src, 0, nullptr, out);
}

int ehm_compiled_narrow_opts(ehm_compiled* src, int32_t opts, int64_t* flushed,
                             ehm_compiled** out) {
    if (!src || !out) return c_err.fail(EHM_E_INVALID, "narrow: bad argument");
    *out = nullptr;
    if (flushed) flushed[0] = flushed[1] = flushed[2] = 0;
    if (opts & ~EHM_NARROW_FLUSH)
        return c_err.fail(EHM_E_INVALID, "narrow: unknown flags %d", (int)opts);
    if (src->single) return c_err.fail(EHM_E_INVALID, "narrow: the law is in single precision "
                                       "already");
    if (src->h[H_TEST] > 0)
        return c_err.fail(EHM_E_INVALID, "narrow: the law has %lld test nodes (children that are "
                          "no bisection); only a walk by planes alone has a single-precision form",
                          (long long)src->h[H_TEST]);
    const int p = src->d.p, n_u = src->d.n_u;
    LawPtr C(new ehm_compiled(), ehm_compiled_destroy);
    C->device = src->device;
    C->single = true;
    std::memcpy(C->h, src->h, sizeof C->h);
    C->h[H_NS] = node_stride32_of(p);
    C->h[H_LS] = leaf_stride32_of(p, n_u);
    C->source_bytes = src->source_bytes;
    EHM_HIP_TRY(c_err, hipSetDevice(C->device));
    EHM_HIP_TRY(c_err, C->stream.create());
    EHM_HIP_TRY(c_err, C->node.alloc(C->node_bytes()));
    EHM_HIP_TRY(c_err, C->leaf_rec.alloc(C->leaf_bytes()));
    EHM_HIP_TRY(c_err, C->test_rec.alloc(0));
    struct {
        DevBuf* dst;
        const DevBuf* from;
        size_t bytes;
    } same[] = {{&C->leaf_node, &src->leaf_node, C->leaf_node_bytes()},
                {&C->root_rec, &src->root_rec, C->root_bytes()},
                {&C->root_entry, &src->root_entry, C->entry_bytes()},
                {&C->nbr, &src->nbr, C->nbr_bytes()}};
    for (const auto& part : same) {
        if (!part.bytes) continue;
        EHM_HIP_TRY(c_err, part.dst->alloc(part.bytes));
        EHM_HIP_TRY(c_err, hipMemcpyAsync(part.dst->ptr, part.from->ptr, part.bytes,
                                          hipMemcpyDeviceToDevice, C->stream));
    }
    DevBuf d_flags, d_flushed;
    EHM_HIP_TRY(c_err, d_flags.alloc(sizeof(int)));
    EHM_HIP_TRY(c_err, hipMemsetAsync(d_flags.ptr, 0, sizeof(int), C->stream));
    unsigned long long gone[3] = {0, 0, 0};
    if (opts & EHM_NARROW_FLUSH) {
        EHM_HIP_TRY(c_err, d_flushed.alloc(sizeof gone));
        EHM_HIP_TRY(c_err, hipMemsetAsync(d_flushed.ptr, 0, sizeof gone, C->stream));
    }
    NarrowArgs A{};
    A.n_int = src->h[H_INT];
    A.n_leaf = src->h[H_LEAF];
    A.p = p;
    A.leaf_used = p + n_u + n_u * p;
    A.ns64 = (int)src->h[H_NS];
    A.ns32 = (int)C->h[H_NS];
    A.ls64 = (int)src->h[H_LS];
    A.ls32 = (int)C->h[H_LS];
    A.node = src->node.as<const double>();
    A.leaf_rec = src->leaf_rec.as<const double>();
    A.node32 = C->node.as<float>();
    A.leaf32 = C->leaf_rec.as<float>();
    A.flags = d_flags.as<int>();
    A.flushed = d_flushed.as<unsigned long long>();
    void* args[] = {&A};
    // the source's arrays were written on its own stream (create) or by blocking copies (import)
    EHM_HIP_TRY(c_err, hipStreamSynchronize(src->stream));
    EHM_HIP_TRY(c_err, hipLaunchKernel(ehm_compiled32_api()->narrow,
                                       dim3((unsigned)((A.n_int + A.n_leaf + 255) / 256)),
                                       dim3(256), args, 0, C->stream));
    int flags = 0;
    EHM_HIP_TRY(c_err, hipMemcpyAsync(&flags, d_flags.ptr, sizeof flags, hipMemcpyDeviceToHost,
                                      C->stream));
    if (d_flushed)
        EHM_HIP_TRY(c_err, hipMemcpyAsync(gone, d_flushed.ptr, sizeof gone, hipMemcpyDeviceToHost,
                                          C->stream));
    EHM_HIP_TRY(c_err, hipStreamSynchronize(C->stream));
    if (flags)
        return c_err.fail(
            EHM_E_INVALID, "narrow: the law has no single-precision form:%s%s%s",
            flags & NARROW_OVERFLOW ? " a value overflows or is not finite;" : "",
            flags & NARROW_UNDERFLOW ? " a nonzero value becomes zero or subnormal;" : "",
            flags & NARROW_ZERO_NORMAL ? " a plane's normal becomes zero;" : "");
    if (flushed)
        for (int i = 0; i < 3; ++i) flushed[i] = (int64_t)gone[i];
    C->bind();
    *out = C.release();
    return EHM_OK;
}

int ehm_compiled_info(const ehm_compiled* C, int64_t* info) {
    if (!C || !info) return c_err.fail(EHM_E_INVALID, "info: bad argument");
    for (int i = 0; i < EHM_C_HEADER; ++i) info[i] = C->h[i];
    info[EHM_C_HEADER] = (int64_t)C->bytes();
    info[EHM_C_HEADER + 1] = C->source_bytes;
    return EHM_OK;
}

int ehm_compiled_export(ehm_compiled* C, double* node, double* leaf_rec, int32_t* leaf_node,
                        double* test_rec, double* root_rec, int32_t* root_entry, int32_t* nbr) {
    return export_law(C, false, node, leaf_rec, leaf_node, test_rec, root_rec, root_entry, nbr);
}

int ehm_compiled_export_single(ehm_compiled* C, float* node, float* leaf_rec, int32_t* leaf_node,
                          double* root_rec, int32_t* root_entry, int32_t* nbr) {
    return export_law(C, true, node, leaf_rec, leaf_node, nullptr, root_rec, root_entry, nbr);
}

int ehm_compiled_eval_batch(ehm_compiled* C, int64_t n, const double* x, double* u,
                            int32_t* leaf, int32_t* depth, double* kernel_seconds) {
    if (!C || n < 0 || (n > 0 && (!x || !u))) return c_err.fail(EHM_E_INVALID, "eval: bad "
                                                                "argument");
    if (kernel_seconds) *kernel_seconds = 0.0;
    if (n == 0) return EHM_OK;
    EHM_HIP_TRY(c_err, hipSetDevice(C->device));
    const int p = C->d.p, n_u = C->d.n_u;
    if ((size_t)n > C->cap) {
        for (DevBuf* b : {&C->x, &C->u, &C->leaf, &C->depth, &C->root}) b->reset();
        C->cap = 0;
        if (C->x.alloc((size_t)n * p * sizeof(double)) != hipSuccess ||
            C->u.alloc((size_t)n * n_u * sizeof(double)) != hipSuccess ||
            C->leaf.alloc((size_t)n * sizeof(int32_t)) != hipSuccess ||
            C->depth.alloc((size_t)n * sizeof(int32_t)) != hipSuccess ||
            C->root.alloc((size_t)n * sizeof(int32_t)) != hipSuccess)
            return c_err.fail(EHM_E_HIP, "out of device memory for %lld queries", (long long)n);
        C->cap = (size_t)n;
    }
    EventPair ev;
    EHM_HIP_TRY(c_err, hipMemcpyAsync(C->x.ptr, x, (size_t)n * p * sizeof(double),
                                      hipMemcpyHostToDevice, C->stream));
    (void)hipEventRecord(ev.e0, C->stream);
    const bool locate = C->nbr && !locate_off();
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (locate)
        hipLaunchKernelGGL(k_locate_table[p - 1], grid, block, 0, C->stream, C->d, (long long)n,
                           C->x.as<const double>(), C->nbr.as<const int32_t>(),
                           C->root.as<int32_t>());
    const int32_t* root = locate ? C->root.as<const int32_t>() : nullptr;
    if (C->single) {
        long long nn = n;
        const double* xp = C->x.as<const double>();
        double* up = C->u.as<double>();
        int32_t *lp = C->leaf.as<int32_t>(), *dp = C->depth.as<int32_t>();
        void* args[] = {&C->d32, &nn, &xp, &up, &lp, &dp, &root};
        EHM_HIP_TRY(c_err, hipLaunchKernel(ehm_compiled32_api()->eval[p - 1], grid, block, args, 0,
                                           C->stream));
    } else {
        hipLaunchKernelGGL(k_eval_table[p - 1], grid, block, 0, C->stream, C->d, (long long)n,
                           C->x.as<const double>(), C->u.as<double>(), C->leaf.as<int32_t>(),
                           C->depth.as<int32_t>(), root);
    }
    (void)hipEventRecord(ev.e1, C->stream);
    EHM_HIP_TRY(c_err, hipGetLastError());
    EHM_HIP_TRY(c_err, hipMemcpyAsync(u, C->u.ptr, (size_t)n * n_u * sizeof(double),
                                      hipMemcpyDeviceToHost, C->stream));
    if (leaf)
        EHM_HIP_TRY(c_err, hipMemcpyAsync(leaf, C->leaf.ptr, (size_t)n * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, C->stream));
    if (depth)
        EHM_HIP_TRY(c_err, hipMemcpyAsync(depth, C->depth.ptr, (size_t)n * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, C->stream));
    EHM_HIP_TRY(c_err, hipStreamSynchronize(C->stream));
    ev.seconds(kernel_seconds);
    return EHM_OK;
}

// ---- closed loop (ehm_compiled_set_plant .. ehm_compiled_rollout_noisy) ---------------------------

}  // extern "C"

namespace {

// what the plant setters refuse about the law itself
int rollout_law_ok(const ehm_compiled* C, const char* who) {
    if (!C) return c_err.fail(EHM_E_INVALID, "%s: a required array is NULL", who);
    if (C->h[H_TEST] > 0)
        return c_err.fail(EHM_E_INVALID, "%s: the law has %lld test nodes (children that are no "
                          "bisection); the rollout's exit test is made on the root and needs a "
                          "walk by planes alone -- roll such a tree out on the source evaluator",
                          who, (long long)C->h[H_TEST]);
    return EHM_OK;
}

const Rollout32Table& rollout32_table() {
    static const Rollout32Table table;
    return table;
}

const int32_t* rollout_nbr(const ehm_compiled* C) {
    return (C->nbr && !locate_off()) ? C->nbr.as<const int32_t>() : nullptr;
}

}  // namespace

extern "C" {

int ehm_compiled_set_plant(ehm_compiled* C, int32_t n_modes, const double* A, const double* B,
                           const double* w, int32_t n_d, const double* Emat,
                           const int32_t* region_rows, const double* H, const double* h,
                           int32_t n_g, const double* Gx, const double* gx,
                           const int32_t* leaf_mode, int32_t cost_kind, const double* Q,
                           const double* R) {
    const int rc = rollout_law_ok(C, "set_plant");
    if (rc != EHM_OK) return rc;
    return install_plant(C->ro, c_err, C->device, C->d.p, C->d.n_u, C->h[H_LEAF], "leaf",
                         "set_plant", n_modes, EHM_R_MAX_MODES, A, B, w, n_g, Gx, gx, leaf_mode,
                         cost_kind, Q, R, nullptr, [&](Pack& pk, DevPlant& pl, int p, int) {
                             return pack_nominal(c_err, pk, pl, p, n_modes, n_d, Emat, region_rows,
                                                 H, h);
                         });
}

int ehm_compiled_set_plant_guarded(ehm_compiled* C, int32_t n_modes, const double* A,
                                   const double* B, const double* w, int32_t substeps,
                                   int32_t n_guards, const int32_t* guard_mode,
                                   const int32_t* guard_row0, const double* ga, const double* gb,
                                   const double* gc, const double* gt, const int32_t* strict,
                                   int32_t default_mode, int32_t n_g, const double* Gx,
                                   const double* gx, const int32_t* leaf_mode, int32_t cost_kind,
                                   const double* Q, const double* R) {
    const int rc = rollout_law_ok(C, "set_plant_guarded");
    if (rc != EHM_OK) return rc;
    DevGuard gd{};
    return install_plant(C->ro, c_err, C->device, C->d.p, C->d.n_u, C->h[H_LEAF], "leaf",
                         "set_plant_guarded", n_modes, EHM_G_MAX_MODES, A, B, w, n_g, Gx, gx,
                         leaf_mode, cost_kind, Q, R, &gd, [&](Pack& pk, DevPlant&, int p, int n_u) {
                             return pack_guarded(c_err, pk, gd, p, n_u, n_modes, substeps, n_guards,
                                                 guard_mode, guard_row0, ga, gb, gc, gt, strict,
                                                 default_mode);
                         });
}

int ehm_compiled_set_noise(ehm_compiled* C, int32_t n_terms, const int32_t* desc,
                           const double* data, int32_t n_data, int32_t n_d) {
    if (!C) return c_err.fail(EHM_E_INVALID, "set_noise: no handle");
    return install_noise(C->ro, c_err, C->device, C->d.p, C->d.n_u, n_terms, desc, data, n_data,
                         n_d);
}

int ehm_compiled_rollout(ehm_compiled* C, int64_t n, int32_t T, const double* x0,
                         const double* d, const double* v, double tol_exit, double* x_traj,
                         double* u_traj, int32_t* leaf_traj, double* x_final, int32_t* steps,
                         int32_t* status, double* cost, double* u_norm_sum,
                         double* max_violation, double* kernel_seconds) {
    if (!C) return c_err.fail(EHM_E_INVALID, "rollout: bad argument");
    if (C->single)
        return rollout_run(C->ro, c_err, C->device, C->stream, C->d32, C->d.p, C->d.n_u,
                           rollout_nbr(C), rollout32_table().fn, n, T, x0, d, v, tol_exit, x_traj,
                           u_traj, leaf_traj, x_final, steps, status, cost, u_norm_sum,
                           max_violation, kernel_seconds, nullptr);
    return rollout_run(C->ro, c_err, C->device, C->stream, C->d, C->d.p, C->d.n_u, rollout_nbr(C),
                       k_rollout_table, n, T, x0, d, v, tol_exit, x_traj, u_traj, leaf_traj,
                       x_final, steps, status, cost, u_norm_sum, max_violation, kernel_seconds,
                       nullptr);
}

int ehm_compiled_rollout_noisy(ehm_compiled* C, int64_t n, int32_t T, const double* x0,
                               uint64_t seed, uint64_t traj0, double tol_exit, double* x_traj,
                               double* u_traj, int32_t* leaf_traj, double* v_traj,
                               double* e_traj, double* w_traj, double* x_final, int32_t* steps,
                               int32_t* status, double* cost, double* u_norm_sum,
                               double* max_violation, double* kernel_seconds) {
    if (!C) return c_err.fail(EHM_E_INVALID, "rollout_noisy: no handle");
    const int rc = noisy_ready(C->ro, c_err);
    if (rc != EHM_OK) return rc;
    const NoisyCall nz{seed, traj0, v_traj, e_traj, w_traj};
    if (C->single)
        return rollout_run(C->ro, c_err, C->device, C->stream, C->d32, C->d.p, C->d.n_u,
                           rollout_nbr(C), rollout32_table().fn, n, T, x0, nullptr, nullptr,
                           tol_exit, x_traj, u_traj, leaf_traj, x_final, steps, status, cost,
                           u_norm_sum, max_violation, kernel_seconds, &nz);
    return rollout_run(C->ro, c_err, C->device, C->stream, C->d, C->d.p, C->d.n_u, rollout_nbr(C),
                       k_rollout_table, n, T, x0, nullptr, nullptr, tol_exit, x_traj, u_traj,
                       leaf_traj, x_final, steps, status, cost, u_norm_sum, max_violation,
                       kernel_seconds, &nz);
}

}  // extern "C"
