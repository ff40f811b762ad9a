// The interval hull of one kind of a packed uncertainty model (NoiseModel.pack, noise_fill, DevNoise:
// ehm_rollout_dev.h) over every draw at |x| <= a, |u| <= b: what noise.bounding_boxes states, from the
// doubles the rollout's sampler noise_kind reads.  A header of its own, so that the
// code of the rollout kernels cannot move.
#pragma once

#include <cmath>

#include "ehm_rollout_dev.h"

namespace {

// (lo, hi) [OUT slots, n_out used] of `kind` at the moduli a [p] and b [n_u]; P >= p and NU >= n_u are
// the slots of a and b.  Terms in model order, the sums from 0.0, no FMA.  A box term M (c + h s) adds
// mid -+ rad, mid = sum_k M_ik c_k, rad = sum_k |M_ik| h_k.  A ball term L q, ||q|| <= r, adds
// -+ r dual_i: r as noise_kind computes it with |F| and a or b in the place of F and x or u (the same
// fmax / += / sqrt sequence), dual_i the norm of row i of L that is dual to the ball's (2: 2, inf: 1,
// 1: inf).
template <int P, int NU, int OUT>
__host__ __device__ __forceinline__ void noise_box(const DevNoise& N, const double* sn, int kind,
                                                   int n_out, int p, int n_u, const double* a,
                                                   const double* b, double* lo, double* hi) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < OUT; ++i) {
        lo[i] = 0.0;
        hi[i] = 0.0;
    }
    for (int j = 0; j < N.n_terms; ++j) {
        const int* ds = N.desc[j];
        if (ds[0] != kind) continue;
        const int dim = ds[2];
        const double* td = sn + ds[7];
        if (ds[1] == 0) {
            const double* map = td + 2 * dim;
#pragma unroll
            for (int i = 0; i < OUT; ++i) {
                if (i >= n_out) break;
                double mid = 0.0, rad = 0.0;
                for (int k = 0; k < dim; ++k) {
                    mid = mid + map[i * dim + k] * td[k];
                    rad = rad + fabs(map[i * dim + k]) * td[dim + k];
                }
                lo[i] = lo[i] + (mid - rad);
                hi[i] = hi[i] + (mid + rad);
            }
            continue;
        }
        double r = td[0];
        int off = 1;
        if (ds[4] != 0) {
            const int rows = ds[6], code = ds[5];
            double nrm = 0.0;
            for (int i = 0; i < rows; ++i) {
                double y = 0.0;
                if (ds[4] == 1) {
#pragma unroll
                    for (int c = 0; c < P; ++c)
                        if (c < p) y = y + fabs(td[1 + i * p + c]) * a[c];
                } else {
#pragma unroll
                    for (int c = 0; c < NU; ++c)
                        if (c < n_u) y = y + fabs(td[1 + i * n_u + c]) * b[c];
                }
                if (code == 0) nrm = fmax(nrm, fabs(y));
                else if (code == 1) nrm = nrm + fabs(y);
                else nrm = nrm + y * y;
            }
            if (code == 2) nrm = sqrt(nrm);
            r = r * nrm;
            off += rows * (ds[4] == 1 ? p : n_u);
        }
        const double* map = td + off;
        const int norm = ds[3];
#pragma unroll
        for (int i = 0; i < OUT; ++i) {
            if (i >= n_out) break;
            double dual = 0.0;
            for (int k = 0; k < dim; ++k) {
                const double L = fabs(map[i * dim + k]);
                if (norm == 2) dual = dual + L * L;
                else if (norm == 0) dual = dual + L;
                else dual = fmax(dual, L);
            }
            if (norm == 2) dual = sqrt(dual);
            const double w = r * dual;
            lo[i] = lo[i] - w;
            hi[i] = hi[i] + w;
        }
    }
}

}  // namespace
