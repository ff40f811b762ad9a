// The rules of ehm_refine.hip that need no device, on the parent table and the
// bisected-edge rule of ehm_certify_host.h: the stop codes, the worst-case leaf count of a call, the
// depth of a leaf, the first longest edge of a cell in the partition engine's arithmetic, the
// criteria, the plane of the bisection by a p x p solve in ONE fixed operation order, its rounding
// to the law's scalar, the acceptance test (the test ehm_compiled_cells applies afterwards) and the
// re-pointing of the one reference that named a split leaf.  Plain C++ that the kernels inline and
// a host program can drive (tests/native/refine_host_main.cpp runs it under the address and
// undefined-behaviour sanitizers); tests/refine_cpu.py restates it operation for operation.
#pragma once

#include <cmath>
#include <cstdint>

#include "ehm_certify_host.h"

#if defined(__clang__)
#define EHM_REF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EHM_REF_NO_CONTRACT
#endif

#define EHM_REF_MAX_LEVELS 16           // EHM_REFINE_MAX_LEVELS of include/ehmpc.h

namespace ehm_ref {

using ehm_cert::Parents;

// stop codes of ehm_compiled_refine (include/ehmpc.h); PENDING never leaves the library
enum { STOP_PENDING = -1, STOP_UNSELECTED = 0, STOP_SATISFIED = 1, STOP_LEVELS = 2,
       STOP_NO_CELL = 3, STOP_UNSEPARATED = 4, STOP_TOO_DEEP = 5, STOP_CODES = 6 };

// The most leaves a call can make: 2^levels per selected leaf, one per other leaf.  -1 - l for the
// first leaf l whose levels are outside 0 .. EHM_REF_MAX_LEVELS.
inline int64_t worst_case_leaves(int64_t n_leaf, const int32_t* levels, const uint8_t* selected) {
    int64_t total = 0;
    for (int64_t l = 0; l < n_leaf; ++l) {
        if (levels[l] < 0 || levels[l] > EHM_REF_MAX_LEVELS) return -1 - l;
        total += (!selected || selected[l]) ? (int64_t)1 << levels[l] : 1;
    }
    return total;
}

// levels between leaf l and its root (0: the root's entry); the walk ends as walk_up's does
EHM_CERT_HD int depth_of(const Parents& P, int32_t l) {
    int depth = 0;
    for (int32_t up = P.leaf[l]; up >= 0; up = P.node[up]) ++depth;
    return depth;
}

EHM_CERT_HD double fma_rn(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fma_rn(a, b, c);
#else
    return std::fma(a, b, c);
#endif
}

EHM_CERT_HD double sqrt_rn(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

// longest_edge of ehm_dev.h on a cell in registers: sqrt of the fma chain of the squared
// differences from 0, the first maximal edge (i, j), i < j, in itertools.combinations order.
// Returns its length.
template <int P>
EHM_CERT_HD double longest_edge_of(const double (&V)[(P + 1) * P], int& bi, int& bj) {
    EHM_REF_NO_CONTRACT
    double best = -1.0;
    bi = 0;
    bj = 1;
    EHM_CERT_UNROLL
    for (int i = 0; i <= P; ++i) {
        EHM_CERT_UNROLL
        for (int j = i + 1; j <= P; ++j) {
            double s = 0.0;
            EHM_CERT_UNROLL
            for (int k = 0; k < P; ++k) {
                const double df = V[i * P + k] - V[j * P + k];
                s = fma_rn(df, df, s);
            }
            const double len = sqrt_rn(s);
            if (len > best) {
                best = len;
                bi = i;
                bj = j;
            }
        }
    }
    return best;
}

// a criterion is exceeded; false for a NaN on either side
EHM_CERT_HD bool exceeds(double value, double bound) { return value > bound; }

// max_i w_i - min_i w_i, NaN if any w_i is
template <int N>
EHM_CERT_HD double spread_of(const double (&w)[N]) {
    EHM_REF_NO_CONTRACT
    double hi = w[0], lo = w[0];
    bool nan = w[0] != w[0];
    EHM_CERT_UNROLL
    for (int i = 1; i < N; ++i) {
        hi = w[i] > hi ? w[i] : hi;
        lo = w[i] < lo ? w[i] : lo;
        nan = nan || w[i] != w[i];
    }
    return nan ? NAN : hi - lo;
}

// The plane s = a . x + b with s(v_j) = +1, s(v_i) = -1 and s(v_k) = 0 at the other vertices of the
// cell V, i < j.  Row r of M is v_k - v_i for the r-th k != i (ascending), its right-hand side 2 for
// k = j and 1 otherwise; elimination by columns with partial pivoting, the FIRST largest modulus
// on ties; below the pivot f = M_rk / M_kk, M_rc = M_rc - f M_kc (c > k ascending), then the right-
// hand side; back substitution a_k = (t_k - M_k(k+1) a_(k+1) - .. ) / M_kk with the terms subtracted
// in ascending column order; b = -1 - ((0 + a_0 v_i0) + .. + a_(P-1) v_i(P-1)).  Every product and
// sum is rounded once.  A singular cell gives values that are not finite, which the acceptance test
// refuses.  Every array is indexed statically, so on the device all of it stays in registers.
template <int P>
EHM_CERT_HD void solve_plane(const double (&V)[(P + 1) * P], int i, int j, double (&a)[P],
                             double& b) {
    EHM_REF_NO_CONTRACT
    double vi[P];
    EHM_CERT_UNROLL
    for (int c = 0; c < P; ++c) {
        double t = 0.0;
        EHM_CERT_UNROLL
        for (int k = 0; k <= P; ++k) t = k == i ? V[k * P + c] : t;
        vi[c] = t;
    }
    double M[P * P], t[P];
    EHM_CERT_UNROLL
    for (int r = 0; r < P; ++r) {
        const bool after = r >= i;              // the r-th k != i is r, or r + 1 from i on
        EHM_CERT_UNROLL
        for (int c = 0; c < P; ++c)
            M[r * P + c] = (after ? V[(r + 1) * P + c] : V[r * P + c]) - vi[c];
        t[r] = (after ? r + 1 : r) == j ? 2.0 : 1.0;
    }
    EHM_CERT_UNROLL
    for (int k = 0; k < P; ++k) {
        int piv = k;
        double big = std::fabs(M[k * P + k]);
        EHM_CERT_UNROLL
        for (int r = k + 1; r < P; ++r) {
            const double m = std::fabs(M[r * P + k]);
            if (m > big) {
                big = m;
                piv = r;
            }
        }
        // rows k and piv change places (nothing moves when piv == k)
        EHM_CERT_UNROLL
        for (int c = k; c < P; ++c) {
            const double top = M[k * P + c];
            double got = top;
            EHM_CERT_UNROLL
            for (int r = k + 1; r < P; ++r) {
                got = r == piv ? M[r * P + c] : got;
                M[r * P + c] = r == piv ? top : M[r * P + c];
            }
            M[k * P + c] = got;
        }
        {
            const double top = t[k];
            double got = top;
            EHM_CERT_UNROLL
            for (int r = k + 1; r < P; ++r) {
                got = r == piv ? t[r] : got;
                t[r] = r == piv ? top : t[r];
            }
            t[k] = got;
        }
        EHM_CERT_UNROLL
        for (int r = k + 1; r < P; ++r) {
            const double f = M[r * P + k] / M[k * P + k];
            EHM_CERT_UNROLL
            for (int c = k + 1; c < P; ++c) M[r * P + c] = M[r * P + c] - f * M[k * P + c];
            t[r] = t[r] - f * t[k];
        }
    }
    EHM_CERT_UNROLL
    for (int k = P - 1; k >= 0; --k) {
        double s = t[k];
        EHM_CERT_UNROLL
        for (int c = k + 1; c < P; ++c) s = s - M[k * P + c] * a[c];
        a[k] = s / M[k * P + k];
    }
    double d = 0.0;
    EHM_CERT_UNROLL
    for (int c = 0; c < P; ++c) d = d + a[c] * vi[c];
    b = -1.0 - d;
}

// A coefficient a record of the law's scalar may hold: finite, and in a single law a normal float
// or exactly zero (the import check of a single law).
EHM_CERT_HD bool storable(double x) { return std::isfinite(x); }
EHM_CERT_HD bool storable(float x) { return std::isfinite(x) && (x == 0.0f || std::isnormal(x)); }

// [a | b] rounded to the law's scalar into rec [P + 1]; false if a coefficient is not storable
template <class T, int P>
EHM_CERT_HD bool store_plane(const double (&a)[P], double b, T (&rec)[P + 1]) {
    bool ok = true;
    EHM_CERT_UNROLL
    for (int c = 0; c < P; ++c) {
        rec[c] = (T)a[c];
        ok = ok && storable(rec[c]);
    }
    rec[P] = (T)b;
    return ok && storable(rec[P]);
}

// The acceptance test: the stored plane, widened as leaf_cell reads it, at the vertices of the cell
// -- s_k = ((0 + a_0 v_k0) + .. ) + b -- passes bisected_edge with pos == j and neg == i.
// residual: the largest |s_k - target_k| (meaningful when accepted).
template <class T, int P>
EHM_CERT_HD bool accept_plane(const double (&V)[(P + 1) * P], const T (&rec)[P + 1], int i, int j,
                              double& residual) {
    EHM_REF_NO_CONTRACT
    double s[P + 1];
    residual = 0.0;
    EHM_CERT_UNROLL
    for (int k = 0; k <= P; ++k) {
        double d = 0.0;
        EHM_CERT_UNROLL
        for (int c = 0; c < P; ++c) d = d + (double)rec[c] * V[k * P + c];
        s[k] = d + (double)rec[P];
        const double target = k == j ? 1.0 : k == i ? -1.0 : 0.0;
        const double off = std::fabs(s[k] - target);
        residual = off > residual ? off : residual;
    }
    int pos, neg;
    return ehm_cert::bisected_edge<P + 1>(s, pos, neg) && pos == j && neg == i;
}

// The child c on `side` of internal record k after a pass: the new internal record of a split leaf
// in place of ~l, through the parent table -- only the one reference the table holds is re-pointed.
EHM_CERT_HD int32_t repoint_child(const Parents& P, int32_t k, int side, int32_t c,
                                  const int32_t* split, const int32_t* offset, int64_t n_int) {
    if (c >= 0) return c;
    const int32_t l = ~c;
    if (!split[l] || P.leaf[l] != k || P.leaf_side[l] != side) return c;
    return (int32_t)(n_int + offset[l]);
}

// the same for the entry of root r
EHM_CERT_HD int32_t repoint_entry(const Parents& P, int32_t r, int32_t entry, const int32_t* split,
                                  const int32_t* offset, int64_t n_int) {
    if (entry >= 0) return entry;
    const int32_t l = ~entry;
    if (!split[l] || P.leaf[l] != ~r) return entry;
    return (int32_t)(n_int + offset[l]);
}

}  // namespace ehm_ref
