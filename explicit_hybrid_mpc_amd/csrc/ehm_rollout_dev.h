// What the closed-loop kernels of the laws share (ehm_explicit.hip: the fused rollout of the
// explicit law; ehm_compiled.hip: the same around the compiled law; ehm_implicit.hip: the per-step
// kernels around the implicit law): the device layouts of the plant, the guards and the
// uncertainty model, the sampler of the model, the host-side packing of a plant's doubles, and --
// for the two fused rollouts -- the step itself once the input is known (rollout_apply), its
// records, and the host plumbing that installs a plant and launches a rollout.  Every translation
// unit that includes this gets its own copy (unnamed namespace), as it would of any inline device
// code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/ehmpc.h"
#include "ehm_host.h"
#include "ehm_philox.h"

namespace {

#define EHM_R_MAX_NU 4
#define EHM_R_MAX_MODES 4
#define EHM_R_MAX_D 8
#define EHM_R_MAX_ROWS 256       // constraint rows Gx, and mode-region rows of all modes together

struct DevPlant {
    const double* data;      // [total] doubles, the offsets below
    int total, n_modes, n_d, n_g, cost_kind;          // cost_kind 0: inf-norm, 1: quadratic
    int oA, oB, ow, oE, oH, oh, oG, og, oQ, oR;
    int row0[EHM_R_MAX_MODES + 1];                    // region rows of mode m: row0[m] .. row0[m+1]
};

// ---- guarded multi-rate plants (simulate.GuardedPlant, ehm_explicit_set_plant_guarded) -----------
//
// The plant picks its own mode before every plant step: the first guard whose rows all hold, else
// the default mode; row r holds iff ((sum_c a_c x_c) + sum_c b_c u_c) + c_r  <=  t_r  (< if strict).
// S plant steps per controller step, u held.  The modes sit in the DevPlant arrays (oA, oB, ow),
// the rows after them in the same LDS block: a [rows][p] at oGa, b [rows][n_u] at oGb, c at oGc,
// t at oGt.
#define EHM_G_MAX_MODES 8
#define EHM_G_MAX_ROWS 16
#define EHM_G_MAX_SUB 64

struct DevGuard {
    int substeps, n_guards, default_mode;
    int oGa, oGb, oGc, oGt;
    int mode[EHM_G_MAX_ROWS];                 // guard g selects mode[g]
    int row0[EHM_G_MAX_ROWS + 1];             // its rows row0[g] .. row0[g+1]
    int strict[EHM_G_MAX_ROWS];               // per row
};

// ---- the uncertainty model of the noisy rollout (noise.py, ehm_explicit_set_noise) -----------
//
// Terms in model order; desc per term: kind (0 process, 1 state, 2 input), shape (0 box, 1 ball),
// dim, ball norm code, radius dependency (0 const, 1 state, 2 input), its norm code, rows of F,
// offset of the term's doubles (box: c, h, M [out][dim]; ball: sigma, F [rows][p or n_u],
// L [out][dim]); norm codes 0 inf, 1, 2.  The doubles sit in LDS after the plant's.
#define EHM_N_MAX_TERMS 16
#define EHM_N_DESC 8
#define EHM_N_MAX_BOX 8
#define EHM_N_MAX_BALL 3
#define EHM_N_MAX_F_ROWS 8
#define EHM_N_ATTEMPTS 64
#define EHM_N_MAX_LDS 8192       // doubles of plant and model together in the noisy kernel's LDS

struct DevNoise {
    const double* data;
    int total, n_terms;
    unsigned long long seed, traj0;
    int desc[EHM_N_MAX_TERMS][EHM_N_DESC];
};

// The draw of one kind, summed over its terms in model order from 0.0 (OUT slots, n_out used),
// counter (id, t, j, attempt) under the key (seed, 0).  No FMA: bit-equal to noise.py.
template <int P, int NU, int OUT>
__device__ __forceinline__ void noise_kind(const DevNoise& N, const double* sn, int kind,
                                           int n_out, uint64_t id, uint64_t t, const double* x,
                                           const double* u, double* acc) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < OUT; ++i) acc[i] = 0.0;
    for (int j = 0; j < N.n_terms; ++j) {
        const int* ds = N.desc[j];
        if (ds[0] != kind) continue;
        const int dim = ds[2];
        const double* td = sn + ds[7];
        const double* map;
        double q[EHM_N_MAX_BOX];
        if (ds[1] == 0) {
            uint64_t w[EHM_N_MAX_BOX];
#pragma unroll
            for (int b = 0; b < EHM_N_MAX_BOX / 4; ++b) {
                uint64_t c[4] = {id, t, (uint64_t)j, (uint64_t)b};
                if (4 * b < dim) ehm_philox4x64_10(c, N.seed, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) w[4 * b + k] = c[k];
            }
#pragma unroll
            for (int k = 0; k < EHM_N_MAX_BOX; ++k)
                q[k] = (k < dim) ? td[k] + td[dim + k] * ehm_uniform_pm1(w[k]) : 0.0;
            map = td + 2 * dim;
        } else {
            double r = td[0];
            int off = 1;
            if (ds[4] != 0) {
                const int rows = ds[6], code = ds[5];
                double nrm = 0.0;
                for (int i = 0; i < rows; ++i) {
                    double y = 0.0;
                    if (ds[4] == 1) {
#pragma unroll
                        for (int c = 0; c < P; ++c) y += td[1 + i * P + c] * x[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < NU; ++c) y += td[1 + i * NU + c] * u[c];
                    }
                    if (code == 0) nrm = fmax(nrm, fabs(y));
                    else if (code == 1) nrm += fabs(y);
                    else nrm += y * y;
                }
                if (code == 2) nrm = sqrt(nrm);
                r = r * nrm;
                off += rows * (ds[4] == 1 ? P : NU);
            }
            double s[EHM_N_MAX_BALL];
            if (ds[3] != 2) {
                uint64_t c[4] = {id, t, (uint64_t)j, 0};
                ehm_philox4x64_10(c, N.seed, 0);
#pragma unroll
                for (int k = 0; k < EHM_N_MAX_BALL; ++k) s[k] = ehm_uniform_pm1(c[k]);
            } else {
                // uniform in the 2-ball: rejection from the cube, zero after the last attempt
                bool ok = false;
                for (int a = 0; a < EHM_N_ATTEMPTS && !ok; ++a) {
                    uint64_t c[4] = {id, t, (uint64_t)j, (uint64_t)a};
                    ehm_philox4x64_10(c, N.seed, 0);
                    double ss = 0.0;
#pragma unroll
                    for (int k = 0; k < EHM_N_MAX_BALL; ++k) {
                        s[k] = ehm_uniform_pm1(c[k]);
                        if (k < dim) ss += s[k] * s[k];
                    }
                    ok = ss <= 1.0;
                }
                if (!ok)
#pragma unroll
                    for (int k = 0; k < EHM_N_MAX_BALL; ++k) s[k] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < EHM_N_MAX_BOX; ++k)
                q[k] = (k < EHM_N_MAX_BALL && k < dim) ? r * s[k < EHM_N_MAX_BALL ? k : 0] : 0.0;
            map = td + off;
        }
#pragma unroll
        for (int i = 0; i < OUT; ++i) {
            if (i >= n_out) break;
            double y = 0.0;
#pragma unroll
            for (int k = 0; k < EHM_N_MAX_BOX; ++k)
                if (k < dim) y += map[i * dim + k] * q[k];
            acc[i] += y;
        }
    }
}

// The descriptors of a packed model (NoiseModel.pack) checked against the limits above and copied
// into nz (data and keys are the caller's): -1, or the first term whose descriptor is bad.
inline int noise_fill(DevNoise& nz, int n_terms, const int32_t* desc, int n_data, int p, int n_u,
                      int n_d) {
    nz.n_terms = n_terms;
    nz.total = n_data;
    for (int j = 0; j < n_terms; ++j) {
        const int32_t* ds = desc + (size_t)j * EHM_N_DESC;
        const int kind = ds[0], shape = ds[1], dim = ds[2], norm = ds[3], dep = ds[4],
                  pdep = ds[5], rows = ds[6], off = ds[7];
        const int out = kind == 0 ? n_d : kind == 1 ? p : n_u;
        long long need = -1;
        if (kind < 0 || kind > 2 || off < 0) {
        } else if (shape == 0 && dim >= 1 && dim <= EHM_N_MAX_BOX) {
            need = 2LL * dim + (long long)out * dim;
        } else if (shape == 1 && dim >= 1 && dim <= EHM_N_MAX_BALL && norm >= 0 && norm <= 2 &&
                   (norm != 1 || dim == 1) && dep >= 0 && dep <= 2 && pdep >= 0 && pdep <= 2 &&
                   rows >= 0 && rows <= EHM_N_MAX_F_ROWS && (dep != 0 || rows == 0)) {
            need = 1LL + (long long)rows * (dep == 1 ? p : n_u) + (long long)out * dim;
        }
        if (need < 0 || off + need > n_data) return j;
        for (int k = 0; k < EHM_N_DESC; ++k) nz.desc[j][k] = ds[k];
    }
    return -1;
}

// The doubles of a plant, one array after the other; put gives the array's offset (NULL: zeros).
struct Pack {
    std::vector<double> buf;
    int put(const double* src, size_t cnt) {
        const int off = (int)buf.size();
        if (src) buf.insert(buf.end(), src, src + cnt);
        else buf.insert(buf.end(), cnt, 0.0);
        return off;
    }
};

// ---- the fused rollout of a law given as a tree (k_explicit_rollout, k_compiled_rollout) --------
//
// One thread per trajectory, the T steps inside the kernel; the plant (and under noise the model)
// in LDS.  A kernel states how its law finds (leaf, u, mode) for a measured state; everything else
// of a step is stated here once, under fp contract(off), and is bit for bit the same in both.

// The plant a rollout kernel closes the loop around.
// PK_NOISY: the nominal plant, with v, e and w drawn from the model in NZ (noise_kind) instead of
// read from R.v / R.d: v at the true state and the last commanded input, e and w at the true state
// and the commanded input, e = 0 where u = 0; the plant steps with u + e, cost and ||u|| stay the
// commanded input's.
// PK_GUARDED: the plant of GD -- no mode-region check (status 2), and the commanded u is held over
// GD.substeps plant steps whose modes the guards choose.
enum PlantKind { PK_NOMINAL, PK_NOISY, PK_GUARDED, PK_KINDS };

struct RollArgs {
    long long n;
    int T;
    double tol_exit;
    const double *x0, *d, *v;
    const int32_t* mode;     // the step-0 mode per node (explicit law) / per leaf (compiled law)
    const int32_t* nbr;      // root face adjacency (long spines) or nullptr
    double *x_traj, *u_traj;
    int32_t* leaf_traj;
    double *x_final, *cost, *u_norm, *max_viol;
    int32_t *steps, *status;
    double *v_traj, *e_traj, *w_traj;       // records of the noisy rollout
};

// what a trajectory carries from step to step
template <int P, int NU>
struct RollState {
    double x[P];
    double up[NU];           // the last commanded input (noisy: v is drawn at it)
    double cost, unorm, maxv;
};

// the plant's doubles into LDS (all threads of the block; the caller synchronises)
__device__ __forceinline__ void plant_load(const DevPlant& PL, double* sh) {
    for (int i = threadIdx.x; i < PL.total; i += blockDim.x) sh[i] = PL.data[i];
}

// plant and model into LDS (likewise)
template <PlantKind KIND>
__device__ __forceinline__ void rollout_load(const DevPlant& PL, const DevNoise& NZ, double* sh) {
    plant_load(PL, sh);
    if constexpr (KIND == PK_NOISY)
        for (int i = threadIdx.x; i < NZ.total; i += blockDim.x) sh[PL.total + i] = NZ.data[i];
}

template <int P, int NU>
__device__ __forceinline__ void rollout_begin(const RollArgs& R, long long q,
                                              RollState<P, NU>& S) {
#pragma unroll
    for (int c = 0; c < NU; ++c) S.up[c] = 0.0;
#pragma unroll
    for (int c = 0; c < P; ++c) S.x[c] = R.x0[q * P + c];
    if (R.x_traj)
#pragma unroll
        for (int c = 0; c < P; ++c) R.x_traj[(size_t)q * P + c] = S.x[c];
    S.cost = 0.0;
    S.unorm = 0.0;
    S.maxv = -__builtin_inf();
}

// measure: z = x + v_t, no error at t = 0
template <int P, int NU, PlantKind KIND>
__device__ __forceinline__ void rollout_measure(const DevPlant& PL, const RollArgs& R,
                                                const DevNoise& NZ, const double* sh, long long q,
                                                int t, uint64_t id, const RollState<P, NU>& S,
                                                double* z) {
#pragma clang fp contract(off)
    const long long n = R.n;
    if constexpr (KIND == PK_NOISY) {
        double vn[P];
        noise_kind<P, NU, P>(NZ, sh + PL.total, 1, P, id, (uint64_t)t, S.x, S.up, vn);
        if (R.v_traj)
#pragma unroll
            for (int c = 0; c < P; ++c) R.v_traj[((size_t)t * n + q) * P + c] = vn[c];
#pragma unroll
        for (int c = 0; c < P; ++c) z[c] = t > 0 ? S.x[c] + vn[c] : S.x[c];
    } else if (R.v && t > 0) {
#pragma unroll
        for (int c = 0; c < P; ++c) z[c] = S.x[c] + R.v[((size_t)t * n + q) * P + c];
    } else {
#pragma unroll
        for (int c = 0; c < P; ++c) z[c] = S.x[c];
    }
}

// The step once the law has answered: u the commanded input, m the step-0 mode of the leaf's
// commutation, leaf the id the record takes.  Returns 0 (applied: S holds x+), 3 (no commutation)
// or 2 (the mode's region does not hold the true state); nothing is applied or recorded then.
template <int P, int NU, PlantKind KIND>
__device__ __forceinline__ int rollout_apply(const DevPlant& PL, const RollArgs& R,
                                             const DevNoise& NZ, const DevGuard& GD,
                                             const double* sh, long long q, int t, uint64_t id,
                                             int m, int32_t leaf, const double* u,
                                             RollState<P, NU>& S) {
#pragma clang fp contract(off)
    constexpr bool NOISY = KIND == PK_NOISY, GUARDED = KIND == PK_GUARDED;
    const long long n = R.n;
    const double* sQ = sh + PL.oQ;
    const double* sR = sh + PL.oR;
    const double* sG = sh + PL.oG;
    const double* sg = sh + PL.og;
    const double* sE = sh + PL.oE;
    double* x = S.x;
    double xn[P];
    if (m < 0 || (!GUARDED && m >= PL.n_modes)) return 3;
    if constexpr (!GUARDED) {
        bool in_region = true;
        for (int r = PL.row0[m]; r < PL.row0[m + 1]; ++r) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s += sh[PL.oH + r * P + c] * x[c];
            in_region = in_region && (s <= sh[PL.oh + r] + R.tol_exit);
        }
        if (!in_region) return 2;
    }
    if (R.u_traj)
#pragma unroll
        for (int c = 0; c < NU; ++c) R.u_traj[((size_t)t * n + q) * NU + c] = u[c];
    if (R.leaf_traj) R.leaf_traj[(size_t)t * n + q] = leaf;
    // stage cost and input 2-norm
    double su = 0.0;
#pragma unroll
    for (int c = 0; c < NU; ++c) su += u[c] * u[c];
    S.unorm += sqrt(su);
    if (PL.cost_kind == 0) {
        double qx = 0.0, ru = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s += sQ[i * P + c] * x[c];
            qx = fmax(qx, fabs(s));
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < NU; ++c) s += sR[i * NU + c] * u[c];
            ru = fmax(ru, fabs(s));
        }
        S.cost += qx + ru;
    } else {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double r = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) r += sQ[i * P + c] * x[c];
            s += x[i] * r;
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            double r = 0.0;
#pragma unroll
            for (int c = 0; c < NU; ++c) r += sR[i * NU + c] * u[c];
            s += u[i] * r;
        }
        S.cost += s;
    }
    // input error and process noise at (x, u)
    double ua[NU], wn[EHM_R_MAX_D];
#pragma unroll
    for (int c = 0; c < NU; ++c) ua[c] = u[c];
    if constexpr (NOISY) {
        const double* sn = sh + PL.total;
        double en[NU];
        noise_kind<P, NU, NU>(NZ, sn, 2, NU, id, (uint64_t)t, x, u, en);
        if (su == 0.0)
#pragma unroll
            for (int c = 0; c < NU; ++c) en[c] = 0.0;
        noise_kind<P, NU, EHM_R_MAX_D>(NZ, sn, 0, PL.n_d, id, (uint64_t)t, x, u, wn);
#pragma unroll
        for (int c = 0; c < NU; ++c) {
            ua[c] = u[c] + en[c];
            S.up[c] = u[c];
        }
        if (R.e_traj)
#pragma unroll
            for (int c = 0; c < NU; ++c) R.e_traj[((size_t)t * n + q) * NU + c] = en[c];
        if (R.w_traj)
#pragma unroll
            for (int j = 0; j < EHM_R_MAX_D; ++j)
                if (j < PL.n_d) R.w_traj[((size_t)t * n + q) * PL.n_d + j] = wn[j];
    }
    if constexpr (GUARDED) {
        // S plant steps with u held, each in the mode the guards choose at (x, u)
        for (int sub = 0; sub < GD.substeps; ++sub) {
            int gm = GD.default_mode;
            for (int g = 0; g < GD.n_guards; ++g) {
                bool ok = true;
                for (int r = GD.row0[g]; r < GD.row0[g + 1]; ++r) {
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < P; ++c) s += sh[GD.oGa + r * P + c] * x[c];
#pragma unroll
                    for (int c = 0; c < NU; ++c) s += sh[GD.oGb + r * NU + c] * u[c];
                    s += sh[GD.oGc + r];
                    const double th = sh[GD.oGt + r];
                    ok = ok && (GD.strict[r] ? (s < th) : (s <= th));
                }
                if (ok) {
                    gm = GD.mode[g];
                    break;
                }
            }
            const double* gA = sh + PL.oA + gm * P * P;
            const double* gB = sh + PL.oB + gm * P * NU;
            const double* gw = sh + PL.ow + gm * P;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) s += gA[i * P + c] * x[c];
#pragma unroll
                for (int c = 0; c < NU; ++c) s += gB[i * NU + c] * u[c];
                xn[i] = s + gw[i];
            }
#pragma unroll
            for (int c = 0; c < P; ++c) x[c] = xn[c];
        }
    } else {
        // plant step x+ = A_m x + B_m u + w_m + E d
        const double* sA = sh + PL.oA + m * P * P;
        const double* sB = sh + PL.oB + m * P * NU;
        const double* sw = sh + PL.ow + m * P;
        const double* dt = R.d ? R.d + ((size_t)t * n + q) * PL.n_d : nullptr;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) s += sA[i * P + c] * x[c];
#pragma unroll
            for (int c = 0; c < NU; ++c) s += sB[i * NU + c] * ua[c];
            s += sw[i];
            if constexpr (NOISY) {
#pragma unroll
                for (int j = 0; j < EHM_R_MAX_D; ++j)
                    if (j < PL.n_d) s += sE[i * PL.n_d + j] * wn[j];
            } else if (dt) {
                for (int j = 0; j < PL.n_d; ++j) s += sE[i * PL.n_d + j] * dt[j];
            }
            xn[i] = s;
        }
    }
    for (int j = 0; j < PL.n_g; ++j) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) s += sG[j * P + c] * xn[c];
        S.maxv = fmax(S.maxv, s - sg[j]);
    }
#pragma unroll
    for (int c = 0; c < P; ++c) x[c] = xn[c];
    if (R.x_traj)
#pragma unroll
        for (int c = 0; c < P; ++c) R.x_traj[((size_t)(t + 1) * n + q) * P + c] = x[c];
    return 0;
}

// The records after a stop at step t (NaN states / inputs, leaf -1) and the trajectory's outputs.
template <int P, int NU, PlantKind KIND>
__device__ __forceinline__ void rollout_finish(const DevPlant& PL, const RollArgs& R, long long q,
                                               int t, int status, const RollState<P, NU>& S) {
    const long long n = R.n;
    const double nan = __builtin_nan("");
    for (int s = t; s < R.T; ++s) {
        if (R.x_traj)
#pragma unroll
            for (int c = 0; c < P; ++c) R.x_traj[((size_t)(s + 1) * n + q) * P + c] = nan;
        if (R.u_traj)
#pragma unroll
            for (int c = 0; c < NU; ++c) R.u_traj[((size_t)s * n + q) * NU + c] = nan;
        if (R.leaf_traj) R.leaf_traj[(size_t)s * n + q] = -1;
        if constexpr (KIND == PK_NOISY) {
            // v of the step a trajectory stopped at was drawn and is kept
            if (R.v_traj && s > t)
#pragma unroll
                for (int c = 0; c < P; ++c) R.v_traj[((size_t)s * n + q) * P + c] = nan;
            if (R.e_traj)
#pragma unroll
                for (int c = 0; c < NU; ++c) R.e_traj[((size_t)s * n + q) * NU + c] = nan;
            if (R.w_traj)
                for (int j = 0; j < PL.n_d; ++j) R.w_traj[((size_t)s * n + q) * PL.n_d + j] = nan;
        }
    }
#pragma unroll
    for (int c = 0; c < P; ++c) R.x_final[q * P + c] = S.x[c];
    R.steps[q] = t;
    R.status[q] = status;
    R.cost[q] = S.cost;
    R.u_norm[q] = S.unorm;
    R.max_viol[q] = S.maxv;
}

// ---- host side: what a law's handle holds for its rollouts, and the plumbing around it ---------

struct RolloutAttach {
    DevBuf plant, mode;                              // set_plant(_guarded)
    DevPlant pl{};
    PlantKind kind = PK_NOMINAL;                     // PK_GUARDED: set_plant_guarded
    DevGuard gd{};
    DevBuf noise;                                    // set_noise
    DevNoise nz{};
    int noise_n_d = 0;
};

// What the two plant setters share: the checks of the common arguments; A, B, w, Gx, gx, Q and R
// packed, then the setter's own arrays (`own` checks and packs them); the mode table (n_mode
// entries, one per `what`) checked (< n_modes for the nominal plant; >= -1 for a guarded one, whose
// guards choose the modes); the new device buffers swapped in.  gd: the guards of a guarded plant
// (filled by `own`), nullptr for the nominal.
template <class Own>
int install_plant(RolloutAttach& ro, ehm_err_channel& err, int device, int p, int n_u,
                  int64_t n_mode, const char* what, const char* who, int32_t n_modes, int max_modes,
                  const double* A, const double* B, const double* w, int32_t n_g, const double* Gx,
                  const double* gx, const int32_t* mode, int32_t cost_kind, const double* Q,
                  const double* R, const DevGuard* gd, Own own) {
    if (!A || !B || !w || !mode || !Q || !R)
        return err.fail(EHM_E_INVALID, "%s: a required array is NULL", who);
    if (n_modes < 1 || n_modes > max_modes)
        return err.fail(EHM_E_INVALID, "%s: %d modes (1..%d)", who, (int)n_modes, max_modes);
    if (n_g < 0 || n_g > EHM_R_MAX_ROWS || (n_g > 0 && (!Gx || !gx)))
        return err.fail(EHM_E_INVALID, "%s: n_g = %d (0..%d)", who, (int)n_g, EHM_R_MAX_ROWS);
    if (cost_kind != 0 && cost_kind != 1)
        return err.fail(EHM_E_INVALID, "%s: cost_kind %d (0 inf-norm, 1 quadratic)", who,
                        (int)cost_kind);
    if (n_u > EHM_R_MAX_NU)
        return err.fail(EHM_E_INVALID, "%s: n_u = %d, the rollout takes at most %d inputs", who,
                        n_u, EHM_R_MAX_NU);
    DevPlant pl{};
    pl.n_modes = n_modes;
    pl.n_g = n_g;
    pl.cost_kind = cost_kind;
    Pack pk;
    pl.oA = pk.put(A, (size_t)n_modes * p * p);
    pl.oB = pk.put(B, (size_t)n_modes * p * n_u);
    pl.ow = pk.put(w, (size_t)n_modes * p);
    pl.oG = pk.put(Gx, (size_t)n_g * p);
    pl.og = pk.put(gx, (size_t)n_g);
    pl.oQ = pk.put(Q, (size_t)p * p);
    pl.oR = pk.put(R, (size_t)n_u * n_u);
    const int rc = own(pk, pl, p, n_u);
    if (rc != EHM_OK) return rc;
    pl.total = (int)pk.buf.size();
    for (int64_t k = 0; k < n_mode; ++k)
        if (gd ? mode[k] < -1 : mode[k] >= n_modes)
            return err.fail(EHM_E_INVALID, "%s: %s %lld has mode %d of %d", who, what, (long long)k,
                            (int)mode[k], (int)n_modes);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return err.fail(EHM_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    DevBuf d_plant, d_mode;
    if (d_plant.upload(pk.buf.data(), pk.buf.size() * sizeof(double)) != hipSuccess ||
        d_mode.upload(mode, (size_t)n_mode * sizeof(int32_t)) != hipSuccess)
        return err.fail(EHM_E_HIP, "%s: device allocation / copy failed", who);
    ro.plant = std::move(d_plant);
    ro.mode = std::move(d_mode);
    pl.data = ro.plant.as<const double>();
    ro.pl = pl;
    ro.kind = gd ? PK_GUARDED : PK_NOMINAL;
    if (gd) ro.gd = *gd;
    return EHM_OK;
}

// `own` of the nominal setter: E, and the mode regions stacked by mode
inline int pack_nominal(ehm_err_channel& err, Pack& pk, DevPlant& pl, int p, int32_t n_modes,
                        int32_t n_d, const double* Emat, const int32_t* region_rows,
                        const double* H, const double* h) {
    if (n_d < 0 || n_d > EHM_R_MAX_D || (n_d > 0 && !Emat))
        return err.fail(EHM_E_INVALID, "set_plant: n_d = %d (0..%d, E needed if > 0)", (int)n_d,
                        EHM_R_MAX_D);
    int rows = 0;
    for (int m = 0; m < n_modes; ++m) {
        const int r = region_rows ? region_rows[m] : 0;
        if (r < 0) return err.fail(EHM_E_INVALID, "set_plant: mode %d has %d region rows", m, r);
        pl.row0[m] = rows;
        rows += r;
    }
    if (rows > EHM_R_MAX_ROWS || (rows > 0 && (!H || !h)))
        return err.fail(EHM_E_INVALID, "set_plant: %d mode-region rows (0..%d)", rows,
                        EHM_R_MAX_ROWS);
    for (int m = n_modes; m <= EHM_R_MAX_MODES; ++m) pl.row0[m] = rows;
    pl.n_d = n_d;
    pl.oE = pk.put(Emat, (size_t)p * n_d);
    pl.oH = pk.put(H, (size_t)rows * p);
    pl.oh = pk.put(h, (size_t)rows);
    return (int)EHM_OK;
}

// `own` of the guarded setter: the guards into gd, their rows after the modes
inline int pack_guarded(ehm_err_channel& err, Pack& pk, DevGuard& gd, int p, int n_u,
                        int32_t n_modes, int32_t substeps, int32_t n_guards,
                        const int32_t* guard_mode, const int32_t* guard_row0, const double* ga,
                        const double* gb, const double* gc, const double* gt,
                        const int32_t* strict, int32_t default_mode) {
    if ((n_guards > 0 && !guard_mode) || !guard_row0)
        return err.fail(EHM_E_INVALID, "set_plant_guarded: a required array is NULL");
    if (substeps < 1 || substeps > EHM_G_MAX_SUB)
        return err.fail(EHM_E_INVALID, "set_plant_guarded: %d substeps (1..%d)", (int)substeps,
                        EHM_G_MAX_SUB);
    if (n_guards < 0 || n_guards > EHM_G_MAX_ROWS)
        return err.fail(EHM_E_INVALID, "set_plant_guarded: %d guards (0..%d)", (int)n_guards,
                        EHM_G_MAX_ROWS);
    if (default_mode < 0 || default_mode >= n_modes)
        return err.fail(EHM_E_INVALID, "set_plant_guarded: default mode %d of %d",
                        (int)default_mode, (int)n_modes);
    if (guard_row0[0] != 0)
        return err.fail(EHM_E_INVALID, "set_plant_guarded: the rows of guard 0 start at %d",
                        (int)guard_row0[0]);
    gd.substeps = substeps;
    gd.n_guards = n_guards;
    gd.default_mode = default_mode;
    for (int g = 0; g <= n_guards; ++g) {
        if (g < n_guards) {
            if (guard_mode[g] < 0 || guard_mode[g] >= n_modes)
                return err.fail(EHM_E_INVALID, "set_plant_guarded: guard %d selects mode %d of %d",
                                g, (int)guard_mode[g], (int)n_modes);
            if (guard_row0[g + 1] <= guard_row0[g])
                return err.fail(EHM_E_INVALID, "set_plant_guarded: guard %d has no rows", g);
            gd.mode[g] = guard_mode[g];
        }
        gd.row0[g] = guard_row0[g];
    }
    const int rows = guard_row0[n_guards];
    if (rows > EHM_G_MAX_ROWS || (rows > 0 && (!ga || !gb || !gc || !gt || !strict)))
        return err.fail(EHM_E_INVALID, "set_plant_guarded: %d guard rows (0..%d)", rows,
                        EHM_G_MAX_ROWS);
    for (int r = 0; r < rows; ++r) gd.strict[r] = strict[r] != 0;
    gd.oGa = pk.put(ga, (size_t)rows * p);
    gd.oGb = pk.put(gb, (size_t)rows * n_u);
    gd.oGc = pk.put(gc, (size_t)rows);
    gd.oGt = pk.put(gt, (size_t)rows);
    return (int)EHM_OK;
}

// set_noise of a fused rollout's handle
inline int install_noise(RolloutAttach& ro, ehm_err_channel& err, int device, int p, int n_u,
                         int32_t n_terms, const int32_t* desc, const double* data, int32_t n_data,
                         int32_t n_d) {
    if (n_terms < 0 || n_terms > EHM_N_MAX_TERMS || (n_terms > 0 && !desc) || n_data < 0 ||
        (n_data > 0 && !data) || n_d < 0 || n_d > EHM_R_MAX_D)
        return err.fail(EHM_E_INVALID, "set_noise: bad argument (at most %d terms, n_d <= %d)",
                        EHM_N_MAX_TERMS, EHM_R_MAX_D);
    DevNoise nz{};
    const int bad = noise_fill(nz, n_terms, desc, n_data, p, n_u, n_d);
    if (bad >= 0) return err.fail(EHM_E_INVALID, "set_noise: term %d has a bad descriptor", bad);
    if (ro.pl.total + n_data > EHM_N_MAX_LDS)
        return err.fail(EHM_E_INVALID, "set_noise: plant and model take %d doubles of LDS (%d)",
                        ro.pl.total + n_data, EHM_N_MAX_LDS);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return err.fail(EHM_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    DevBuf d_noise;
    if (d_noise.upload(data, (size_t)n_data * sizeof(double)) != hipSuccess)
        return err.fail(EHM_E_HIP, "set_noise: device allocation / copy failed");
    ro.noise = std::move(d_noise);
    nz.data = ro.noise.as<const double>();
    ro.nz = nz;
    ro.noise_n_d = n_d;
    return EHM_OK;
}

// the noisy rollout's extra arguments
struct NoisyCall {
    uint64_t seed, traj0;
    double *v_traj, *e_traj, *w_traj;
};

// What the noisy entry point checks before rollout_run
inline int noisy_ready(const RolloutAttach& ro, ehm_err_channel& err) {
    if (!ro.noise) return err.fail(EHM_E_INVALID, "rollout_noisy: no model (set_noise)");
    if (ro.plant && ro.noise_n_d != ro.pl.n_d)
        return err.fail(EHM_E_INVALID, "rollout_noisy: the model has n_d = %d, the plant %d",
                        ro.noise_n_d, ro.pl.n_d);
    return EHM_OK;
}

// A rollout (nz == nullptr) or a noisy rollout of the law `law` (its device view, the kernels'
// first argument) in one launch on `stream`; table [kind][p - 1][n_u - 1] are the law's kernels,
// nbr its root adjacency (or nullptr: the serial walk).
template <class Law>
int rollout_run(RolloutAttach& ro, ehm_err_channel& err, int device, hipStream_t stream,
                const Law& law, int p, int n_u, const int32_t* nbr,
                void (*const (&table)[PK_KINDS][8][EHM_R_MAX_NU])(Law, DevPlant, RollArgs, DevNoise,
                                                                  DevGuard),
                int64_t n, int32_t T, const double* x0, const double* d, const double* v,
                double tol_exit, double* x_traj, double* u_traj, int32_t* leaf_traj,
                double* x_final, int32_t* steps, int32_t* status, double* cost,
                double* u_norm_sum, double* max_violation, double* kernel_seconds,
                const NoisyCall* nz) {
    if (!x0 || !x_final || !steps || !status || !cost || !u_norm_sum || !max_violation || n < 0 ||
        T < 0 || !(tol_exit >= 0.0))
        return err.fail(EHM_E_INVALID, "rollout: bad argument");
    if (!ro.plant) return err.fail(EHM_E_INVALID, "rollout: no plant (set_plant)");
    if (d && ro.pl.n_d == 0)
        return err.fail(EHM_E_INVALID, "rollout: a disturbance was given but the plant has no E");
    // a plant set after the model may have grown past what set_noise checked
    if (nz && ro.kind == PK_GUARDED)
        return err.fail(EHM_E_INVALID, "rollout_noisy: the plant is guarded (noisy guarded plants "
                                       "are not supported)");
    if (nz && ro.pl.total + ro.nz.total > EHM_N_MAX_LDS)
        return err.fail(EHM_E_INVALID, "rollout_noisy: plant and model take %d doubles of LDS (%d)",
                        ro.pl.total + ro.nz.total, EHM_N_MAX_LDS);
    const int n_d = ro.pl.n_d;
    if (n == 0) return EHM_OK;
    if (n > (int64_t)1 << 31)
        return err.fail(EHM_E_INVALID, "rollout: %lld trajectories", (long long)n);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return err.fail(EHM_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    const size_t N = (size_t)n, nT = (size_t)T, D = sizeof(double), I = sizeof(int32_t);
    RollArgs R{};
    R.n = n;
    R.T = T;
    R.tol_exit = tol_exit;
    // the per-trajectory outputs: host array (nullptr: not asked for), the RollArgs pointer its
    // device buffer goes to, bytes
    struct Out {
        void* host;
        void* field;
        size_t bytes;
        DevBuf buf;
    } out[] = {
        {x_final, &R.x_final, N * p * D},
        {steps, &R.steps, N * I},
        {status, &R.status, N * I},
        {cost, &R.cost, N * D},
        {u_norm_sum, &R.u_norm, N * D},
        {max_violation, &R.max_viol, N * D},
        {x_traj, &R.x_traj, (nT + 1) * N * p * D},
        {u_traj, &R.u_traj, nT * N * n_u * D},
        {leaf_traj, &R.leaf_traj, nT * N * I},
        {nz ? nz->v_traj : nullptr, &R.v_traj, nT * N * p * D},
        {nz ? nz->e_traj : nullptr, &R.e_traj, nT * N * n_u * D},
        {nz ? nz->w_traj : nullptr, &R.w_traj, nT * N * n_d * D},
    };
    DevBuf dx0, dd, dv;
    bool ok = dx0.alloc(N * p * D) == hipSuccess &&
              (!d || dd.alloc(nT * N * n_d * D) == hipSuccess) &&
              (!v || dv.alloc(nT * N * p * D) == hipSuccess);
    for (Out& o : out)
        if (ok && o.host) {
            ok = o.buf.alloc(o.bytes) == hipSuccess;
            std::memcpy(o.field, &o.buf.ptr, sizeof o.buf.ptr);
        }
    if (!ok)
        return err.fail(EHM_E_HIP, "rollout: out of device memory for %lld x %d steps",
                        (long long)n, (int)T);
    R.x0 = dx0.as<const double>();
    R.d = dd.as<const double>();
    R.v = dv.as<const double>();
    R.mode = ro.mode.as<const int32_t>();
    R.nbr = nbr;
    EHM_HIP_TRY(err, hipMemcpyAsync(dx0.ptr, x0, N * p * D, hipMemcpyHostToDevice, stream));
    if (d) EHM_HIP_TRY(err, hipMemcpyAsync(dd.ptr, d, nT * N * n_d * D, hipMemcpyHostToDevice,
                                           stream));
    if (v) EHM_HIP_TRY(err, hipMemcpyAsync(dv.ptr, v, nT * N * p * D, hipMemcpyHostToDevice,
                                           stream));
    EventPair ev;
    (void)hipEventRecord(ev.e0, stream);
    DevNoise NZ{};
    size_t lds = (size_t)ro.pl.total * sizeof(double);
    if (nz) {
        NZ = ro.nz;
        NZ.seed = nz->seed;
        NZ.traj0 = nz->traj0;
        lds += (size_t)NZ.total * sizeof(double);
    }
    hipLaunchKernelGGL(table[nz ? PK_NOISY : ro.kind][p - 1][n_u - 1],
                       dim3((unsigned)((n + 255) / 256)), dim3(256), lds, stream, law, ro.pl, R,
                       NZ, ro.gd);
    (void)hipEventRecord(ev.e1, stream);
    EHM_HIP_TRY(err, hipGetLastError());
    for (const Out& o : out)
        if (o.host)
            EHM_HIP_TRY(err, hipMemcpyAsync(o.host, o.buf.ptr, o.bytes, hipMemcpyDeviceToHost,
                                            stream));
    EHM_HIP_TRY(err, hipStreamSynchronize(stream));
    ev.seconds(kernel_seconds);
    return EHM_OK;
}

}  // namespace
