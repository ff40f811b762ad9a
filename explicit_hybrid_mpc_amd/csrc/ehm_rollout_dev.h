// What the closed-loop kernels of both laws share (ehm_explicit.hip: the fused rollout of the
// explicit law; ehm_implicit.hip: the per-step kernels around the implicit law): the device
// layouts of the plant, the guards and the uncertainty model, the sampler of the model, and the
// host-side packing of a plant's doubles.  Every translation unit that includes this gets its own
// copy (unnamed namespace), as it would of any inline device code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

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

}  // namespace
