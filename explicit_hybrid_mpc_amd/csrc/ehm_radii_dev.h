// Per-leaf error boxes of the noisy closed loop, shared by ehm_robust.hip and
// ehm_core.hip: on leaf L every error is bounded at the states and inputs that L itself can see.
//
//   k_leaf_radii   one thread per leaf, templated on the law's scalar and on P: the cell (leaf_cell),
//                  c_L = max_i |V_i|, the vertex inputs (leaf_map_at) and ubar_L = max_i |u(V_i)|, the
//                  y_i in the order of k_successors; a_L by radius_iters steps of
//                  a <- min(a, c_L + vhalf(a, u_abs)) from x_abs; v_L = box_state(a_L, u_abs),
//                  e_L = box_input(a_L, ubar_L), d_L = box_process(a_L, ubar_L);
//                  xplus_L = max_i |y_i| + |E| dmax_L + |A_m| vmax_L + |B_m| emax_L in that order,
//                  a'_L = min(x_abs, xplus_L); v'_L = box_state(a'_L, ubar_L).  The box goes out
//                  leaf-fastest, [2][n_g][box_n] in the column order [d; v; e; v'] of G_m, so that the
//                  lanes of the kernels that read it do so coalesced.
//
// The plant, x_abs, u_abs and after them the model's doubles sit in LDS.  Every operation runs under
// fp contract(off) in a fixed order (tests/robust_radii_cpu.py is the numpy mirror).  Every
// translation unit that includes this gets its own copy (unnamed namespace).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_cells_dev.h"
#include "ehm_noise_box_dev.h"

#define EHM_RAD_BLOCK 64
#define EHM_RAD_MAX_ITERS 16
#define EHM_RAD_MAX_G 64            // generators, as EHM_ROB_MAX_G and EHM_CORE_MAX_D

namespace {

struct RadiiArgs {
    long long n, first;             // leaves first .. first + n - 1, or leaf_ids[0 .. n - 1]
    const int32_t* leaf_ids;
    const void* node;               // of the law's scalar, as leaf_rec
    const void* leaf_rec;
    const int32_t* root_entry;
    const double* root_vertices;    // [n_roots][P+1][P]
    ehm_cert::Parents par;
    const int32_t* leaf_mode;       // [n_leaf]
    int n_u, leaf_stride;
    int n_dd, n_v, n_e, n_g;        // columns of d, of v (twice) and of e; n_g = n_dd + 2 n_v + n_e
    int iters;
    int o_xabs, o_uabs;             // x_abs [P] and u_abs [n_u] in the plant's doubles
    long long box_n;                // leaves the box buffer holds
    double* box;                    // [2][n_g][box_n]
    double* x_abs_leaf;             // [n][P]
    double* x_next_abs;             // [n][P]
    double* u_abs_leaf;             // [n][n_u]
};

// the larger modulus of the two bounds
__device__ __forceinline__ double half_of(double lo, double hi) {
    return fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
}

template <class T, int P>
__global__ __launch_bounds__(EHM_RAD_BLOCK) void k_leaf_radii(RadiiArgs A, DevPlant PL,
                                                              DevNoise NZ) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double sh[];
    plant_load(PL, sh);
    for (int i = threadIdx.x; i < NZ.total; i += blockDim.x) sh[PL.total + i] = NZ.data[i];
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n) return;
    const double* sn = sh + PL.total;
    const int32_t l = A.leaf_ids ? A.leaf_ids[q] : (int32_t)(A.first + q);
    const int n_u = A.n_u, n_g = A.n_g;
    const T* node = static_cast<const T*>(A.node);
    double Y[(P + 1) * P];
    const bool ok = leaf_cell<T, P>(A.par, node, A.root_entry, A.root_vertices, l, Y);
    const int m = A.leaf_mode[l];
    double* box_lo = A.box + q;
    double* box_hi = A.box + (size_t)n_g * A.box_n + q;
    if (!ok || m < 0 || m >= PL.n_modes) {
        for (int k = 0; k < n_g; ++k) {
            box_lo[(size_t)k * A.box_n] = NAN;
            box_hi[(size_t)k * A.box_n] = NAN;
        }
#pragma unroll
        for (int c = 0; c < P; ++c) {
            A.x_abs_leaf[(size_t)q * P + c] = NAN;
            A.x_next_abs[(size_t)q * P + c] = NAN;
        }
        for (int c = 0; c < n_u; ++c) A.u_abs_leaf[(size_t)q * n_u + c] = NAN;
        return;
    }
    // step 1: the cell's and the inputs' largest moduli; the y_i in place of the cell
    double cL[P], ub[EHM_R_MAX_NU];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        double t = fabs(Y[c]);
#pragma unroll
        for (int i = 1; i <= P; ++i) t = fabs(Y[i * P + c]) > t ? fabs(Y[i * P + c]) : t;
        cL[c] = t;
    }
    const T* lr = static_cast<const T*>(A.leaf_rec) + (size_t)l * A.leaf_stride;
    const double* sA = sh + PL.oA + m * P * P;
    const double* sB = sh + PL.oB + m * P * n_u;
    const double* sw = sh + PL.ow + m * P;
    const double* sG = sh + PL.oE + m * (P * n_g);
#pragma unroll
    for (int c = 0; c < EHM_R_MAX_NU; ++c) ub[c] = 0.0;
    for (int i = 0; i <= P; ++i) {
        double v[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double t = 0.0;
#pragma unroll
            for (int ii = 0; ii <= P; ++ii) t = ii == i ? Y[ii * P + c] : t;
            v[c] = t;
        }
        double u[EHM_R_MAX_NU];
#pragma unroll
        for (int c = 0; c < EHM_R_MAX_NU; ++c) {
            u[c] = c < n_u ? leaf_map_at<P>(lr, n_u, c, v) : 0.0;
            ub[c] = (i == 0 || fabs(u[c]) > ub[c]) ? fabs(u[c]) : ub[c];
        }
        double y[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s = s + sA[k * P + c] * v[c];
#pragma unroll
            for (int c = 0; c < EHM_R_MAX_NU; ++c)
                if (c < n_u) s = s + sB[k * n_u + c] * u[c];
            y[k] = s + sw[k];
        }
#pragma unroll
        for (int c = 0; c < P; ++c)
#pragma unroll
            for (int ii = 0; ii <= P; ++ii) Y[ii * P + c] = ii == i ? y[c] : Y[ii * P + c];
    }
    // steps 2 to 4 around one call of the state box: radius_iters times a <- min(a, c_L + vhalf(a)),
    // then the boxes on L at a_L and what they add to the true state next, then v' at a'_L
    const double* x_abs = sh + A.o_xabs;
    const double* u_abs = sh + A.o_uabs;
    double ua[EHM_R_MAX_NU], a[P], lo[P], hi[P];
#pragma unroll
    for (int c = 0; c < EHM_R_MAX_NU; ++c) ua[c] = c < n_u ? u_abs[c] : 0.0;
#pragma unroll
    for (int c = 0; c < P; ++c) a[c] = x_abs[c];
    for (int st = 0; st <= A.iters + 1; ++st) {
        noise_box<P, EHM_R_MAX_NU, P>(NZ, sn, 1, P, P, n_u, a, ua, lo, hi);
        if (st < A.iters) {
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const double t = cL[c] + half_of(lo[c], hi[c]);
                a[c] = t < a[c] ? t : a[c];
            }
            continue;
        }
        if (st > A.iters) {
            // v'_L = box_state(a'_L, ubar_L)
#pragma unroll
            for (int k = 0; k < P; ++k) {
                box_lo[(size_t)(A.n_dd + A.n_v + A.n_e + k) * A.box_n] = lo[k];
                box_hi[(size_t)(A.n_dd + A.n_v + A.n_e + k) * A.box_n] = hi[k];
            }
            break;
        }
        // a = a_L; lo, hi = v_L
        double xp[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            double t = fabs(Y[c]);
#pragma unroll
            for (int i = 1; i <= P; ++i) t = fabs(Y[i * P + c]) > t ? fabs(Y[i * P + c]) : t;
            xp[c] = t;
            A.x_abs_leaf[(size_t)q * P + c] = a[c];
        }
#pragma unroll
        for (int c = 0; c < EHM_R_MAX_NU; ++c)
            if (c < n_u) A.u_abs_leaf[(size_t)q * n_u + c] = ub[c];
        {
            double dlo[EHM_R_MAX_D], dhi[EHM_R_MAX_D];
            noise_box<P, EHM_R_MAX_NU, EHM_R_MAX_D>(NZ, sn, 0, A.n_dd, P, n_u, a, ub, dlo, dhi);
#pragma unroll
            for (int k = 0; k < EHM_R_MAX_D; ++k) {
                if (k >= A.n_dd) break;
                box_lo[(size_t)k * A.box_n] = dlo[k];
                box_hi[(size_t)k * A.box_n] = dhi[k];
                const double h = half_of(dlo[k], dhi[k]);
#pragma unroll
                for (int c = 0; c < P; ++c) xp[c] = xp[c] + fabs(sG[c * n_g + k]) * h;
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (A.n_v) {
                box_lo[(size_t)(A.n_dd + k) * A.box_n] = lo[k];
                box_hi[(size_t)(A.n_dd + k) * A.box_n] = hi[k];
            }
            const double h = half_of(lo[k], hi[k]);
#pragma unroll
            for (int c = 0; c < P; ++c) xp[c] = xp[c] + fabs(sA[c * P + k]) * h;
        }
        {
            double elo[EHM_R_MAX_NU], ehi[EHM_R_MAX_NU];
            noise_box<P, EHM_R_MAX_NU, EHM_R_MAX_NU>(NZ, sn, 2, n_u, P, n_u, a, ub, elo, ehi);
#pragma unroll
            for (int k = 0; k < EHM_R_MAX_NU; ++k) {
                if (k >= n_u) break;
                if (A.n_e) {
                    box_lo[(size_t)(A.n_dd + A.n_v + k) * A.box_n] = elo[k];
                    box_hi[(size_t)(A.n_dd + A.n_v + k) * A.box_n] = ehi[k];
                }
                const double h = half_of(elo[k], ehi[k]);
#pragma unroll
                for (int c = 0; c < P; ++c) xp[c] = xp[c] + fabs(sB[c * n_u + k]) * h;
            }
        }
        // a'_L = min(x_abs, xplus_L): the next round's box is at it and at ubar_L
#pragma unroll
        for (int c = 0; c < P; ++c) {
            a[c] = xp[c] < x_abs[c] ? xp[c] : x_abs[c];
            A.x_next_abs[(size_t)q * P + c] = a[c];
        }
#pragma unroll
        for (int c = 0; c < EHM_R_MAX_NU; ++c) ua[c] = ub[c];
        if (!A.n_v) break;
    }
}

typedef void (*radii_fn)(RadiiArgs, DevPlant, DevNoise);
#define EHM_RAD_ALL(T) {&k_leaf_radii<T, 1>, &k_leaf_radii<T, 2>, &k_leaf_radii<T, 3>, \
                        &k_leaf_radii<T, 4>, &k_leaf_radii<T, 5>, &k_leaf_radii<T, 6>, \
                        &k_leaf_radii<T, 7>, &k_leaf_radii<T, 8>}
const radii_fn k_rad64[EHM_CP] = EHM_RAD_ALL(double);
const radii_fn k_rad32[EHM_CP] = EHM_RAD_ALL(float);
#undef EHM_RAD_ALL

// What both per-leaf entry points refuse of an ehm_robust_radii before the device is touched, and
// what they make of it: the descriptors in nz, the columns each kind has (a kind without terms has
// none), and the generators G_m of those columns with a box of zeros in `gen` (the box is the
// leaf's).  `og` is the caller's plant with n_d the process columns and the zeros as its box.
struct RadiiPlan {
    DevNoise nz{};
    int n_dd = 0, n_v = 0, n_e = 0;
    RobustGen gen;
    std::vector<double> zeros;
    ehm_invariance_opts og;
    ehm_robust_opts rg;
};

inline int radii_plan(ehm_err_channel& err, const ehm_invariance_opts* o, const ehm_robust_opts* ro,
                      const ehm_robust_radii* rr, int p, int n_u, int max_g, const char* who,
                      RadiiPlan& pl) {
    if (rr->n_terms < 0 || rr->n_terms > EHM_N_MAX_TERMS || rr->n_data < 0 ||
        (rr->n_terms > 0 && !rr->desc) || (rr->n_data > 0 && !rr->data))
        return err.fail(EHM_E_INVALID, "%s: a model of %d terms and %d doubles (0..%d terms)", who,
                        (int)rr->n_terms, (int)rr->n_data, EHM_N_MAX_TERMS);
    if (rr->n_x != p || rr->n_u != n_u || rr->n_d != o->n_d)
        return err.fail(EHM_E_INVALID,
                        "%s: the model (n_x %d, n_u %d, n_d %d) does not fit the plant (%d, %d, %d)",
                        who, (int)rr->n_x, (int)rr->n_u, (int)rr->n_d, p, n_u, (int)o->n_d);
    if (rr->radius_iters < 1 || rr->radius_iters > EHM_RAD_MAX_ITERS)
        return err.fail(EHM_E_INVALID, "%s: radius_iters = %d (1..%d)", who, (int)rr->radius_iters,
                        EHM_RAD_MAX_ITERS);
    if (!rr->x_abs || !rr->u_abs)
        return err.fail(EHM_E_INVALID, "%s: x_abs or u_abs is NULL", who);
    for (int c = 0; c < p; ++c)
        if (!std::isfinite(rr->x_abs[c]) || rr->x_abs[c] < 0.0)
            return err.fail(EHM_E_INVALID, "%s: x_abs[%d] = %g", who, c, rr->x_abs[c]);
    for (int c = 0; c < n_u; ++c)
        if (!std::isfinite(rr->u_abs[c]) || rr->u_abs[c] < 0.0)
            return err.fail(EHM_E_INVALID, "%s: u_abs[%d] = %g", who, c, rr->u_abs[c]);
    if (o->n_d < 0 || o->n_d > EHM_R_MAX_D)
        return err.fail(EHM_E_INVALID, "%s: n_d = %d (0..%d under a model)", who, (int)o->n_d,
                        EHM_R_MAX_D);
    const int bad = noise_fill(pl.nz, rr->n_terms, rr->desc, rr->n_data, p, n_u, o->n_d);
    if (bad >= 0) return err.fail(EHM_E_INVALID, "%s: the descriptor of term %d is bad", who, bad);
    bool has[3] = {false, false, false};
    for (int j = 0; j < rr->n_terms; ++j) has[pl.nz.desc[j][0]] = true;
    // the constant part of the v and e boxes must hold 0: a leaf's box is a subset of the global one
    {
        const double zero[EHM_CP] = {0, 0, 0, 0, 0, 0, 0, 0};
        double lo[EHM_CP], hi[EHM_CP];
        for (int kind = 1; kind <= 2; ++kind) {
            const int n_out = kind == 1 ? p : n_u;
            noise_box<EHM_CP, EHM_R_MAX_NU, EHM_CP>(pl.nz, rr->data, kind, n_out, p, n_u, zero, zero,
                                                    lo, hi);
            for (int c = 0; c < n_out; ++c)
                if (!(lo[c] <= 0.0 && hi[c] >= 0.0))
                    return err.fail(EHM_E_INVALID,
                                    "%s: the constant part [%g, %g] of the %s box on axis %d does "
                                    "not hold 0", who, lo[c], hi[c], kind == 1 ? "v" : "e", c);
        }
    }
    pl.n_dd = has[0] ? o->n_d : 0;
    pl.n_v = has[1] ? p : 0;
    pl.n_e = has[2] ? n_u : 0;
    pl.zeros.assign(EHM_RAD_MAX_G, 0.0);
    pl.og = *o;
    pl.og.n_d = pl.n_dd;
    pl.og.d_lo = pl.og.d_hi = pl.zeros.data();
    pl.rg = *ro;
    pl.rg.v_lo = pl.rg.v_hi = pl.n_v ? pl.zeros.data() : nullptr;
    pl.rg.e_lo = pl.rg.e_hi = pl.n_e ? pl.zeros.data() : nullptr;
    int rc = check_step_plant(err, &pl.og, n_u, max_g, who);
    if (rc) return rc;
    return robust_generators(err, &pl.og, &pl.rg, p, n_u, max_g, who, pl.gen);
}

}  // namespace
