// Device side of the explicit law's point location, shared by the kernels of ehm_explicit.hip and
// ehm_audit.hip: the record layout, the barycentric weights, the containment test, the root
// locator's walk and the walk from the spine to the leaf.  One statement of each, so every kernel
// that locates a state ends in the same leaf with the same weights, bit for bit.
//
// None of this sits under an fp-contract pragma: the compiler fuses the products of `weights` and
// `contains` into their sums the same way wherever they are inlined (the walks below do no other
// floating-point arithmetic).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define EHM_XP 8   // max parameter dimension (EHM_MAX_P)

struct DevExplicit {
    const double* rec;       // [n_nodes][rec_stride]: v0 | Minv
    const int2* child;       // (left, right), -1 for a leaf
    const double* vinput;    // [n_nodes][(p+1) n_u]
    int rec_stride, p, n_u, n_roots;
    long long n_nodes;
};

// barycentric weights of x in node k; returns containment (lib/mpc_library.py:714-735)
__device__ __forceinline__ bool weights(const DevExplicit& E, long long k, const double* x,
                                        double* alpha, double& alpha0) {
    const double* r = E.rec + (size_t)k * E.rec_stride;
    const int p = E.p;
    const double eps = 2.220446049250313e-16;
    double d[EHM_XP];
    for (int c = 0; c < p; ++c) d[c] = x[c] - r[c];
    double s = 0.0;
    bool in = true;
    for (int q = 0; q < p; ++q) {
        double a = 0.0;
        for (int c = 0; c < p; ++c) a += r[p + q * p + c] * d[c];     // Minv.dot(x - c)
        alpha[q] = a;
        s += a;
        in = in && (a >= -eps) && (a <= 1.0 + eps);
    }
    alpha0 = 1.0 - s;
    return in && (alpha0 >= -eps) && (alpha0 <= 1.0 + eps);
}

// Containment only, the coordinates tested one after the other and the test left at the first
// weight outside [-eps, 1+eps]: the SAME sums in the same order as `weights`, so the verdict is
// bit-identical -- but a root that does not hold x is usually dismissed after one or two rows of
// Minv instead of p (the spine walk reads 3p instead of p + p^2 doubles per dismissed root).
__device__ __forceinline__ bool contains(const DevExplicit& E, long long k, const double* x) {
    const double* r = E.rec + (size_t)k * E.rec_stride;
    const int p = E.p;
    const double eps = 2.220446049250313e-16;
    double d[EHM_XP];
    for (int c = 0; c < p; ++c) d[c] = x[c] - r[c];
    double s = 0.0;
    for (int q = 0; q < p; ++q) {
        double a = 0.0;
        for (int c = 0; c < p; ++c) a += r[p + q * p + c] * d[c];
        if (!((a >= -eps) && (a <= 1.0 + eps))) return false;
        s += a;
    }
    const double a0 = 1.0 - s;
    return (a0 >= -eps) && (a0 <= 1.0 + eps);
}

// Root locator for long spines (tools.delaunay of a p = 8 box: 34 871 roots).  The reference walks
// the right spine and takes the FIRST root, in spine order, that contains x
// (lib/mpc_library.py:737-767): 17 000 containment tests per state on that spine, and one
// wavefront per query testing 64 roots at a time costs the same lane-steps (measured: 0.85 M
// against 0.95 M states/s).  The roots are a triangulation, so a state in the INTERIOR of a root
// (every barycentric weight > EHM_X_STRICT) is in no other root and the first one in spine order
// is that one -- found by a visibility walk over the face adjacency of the roots (built at
// set-up): from the current root cross the face opposite its most negative weight.  A state
// within EHM_X_STRICT of a face, a walk that leaves the hull or does not end in EHM_X_STEPS steps
// gets root = -1 and the reference's serial walk (explicit_walk): same leaf in every case.
#define EHM_X_STRICT 1e-9
#define EHM_X_STEPS 96
// state number q (any start root does: the walk is short from everywhere).  Returns -1 or the root
// with the containment tests made in the upper bits (`visited` reports the device's work).
__device__ __forceinline__ int32_t explicit_locate_root(const DevExplicit& E, const double* x,
                                                        long long q,
                                                        const int32_t* __restrict__ nbr) {
    const int p = E.p;
    double alpha[EHM_XP], a0;
    int k = (int)(q % E.n_roots);
    int found = -1, steps = 0;
    for (int step = 0; step < EHM_X_STEPS; ++step) {
        ++steps;
        (void)weights(E, k, x, alpha, a0);
        double lo = a0;
        int at = 0;
        for (int i = 0; i < p; ++i)
            if (alpha[i] < lo) {
                lo = alpha[i];
                at = i + 1;
            }
        if (lo > EHM_X_STRICT) {            // strictly inside: the only root that holds x
            found = k;
            break;
        }
        if (lo >= -EHM_X_STRICT) break;     // on a face: the serial walk decides
        const int k2 = nbr[(size_t)k * (p + 1) + at];
        if (k2 < 0) break;                  // left the hull (x outside the set, or rounding)
        k = k2;
    }
    return (found < 0) ? -1 : (found | (steps << 20));
}

// The leaf of x.  Spine: the root the locator found (root >= 0), else the first root that contains
// x, the last one without a test; partition subtree: left iff inside the left child.  `visited`
// counts the tests the reference's walk makes.
__device__ __forceinline__ long long explicit_walk(const DevExplicit& E, const double* x,
                                                   int32_t root, int& visited) {
    long long k = E.n_roots - 1;
    visited = 0;
    if (root >= 0) {
        k = root & 0xfffff;
        visited = root >> 20;
    } else {
        for (int r = 0; r + 1 < E.n_roots; ++r) {
            ++visited;
            if (contains(E, r, x)) {
                k = r;
                break;
            }
        }
    }
    for (;;) {
        const int2 ch = E.child[k];
        if (ch.x < 0) break;
        ++visited;
        k = contains(E, ch.x, x) ? ch.x : ch.y;
    }
    return k;
}
