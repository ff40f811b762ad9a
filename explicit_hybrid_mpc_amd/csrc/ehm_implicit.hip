// The closed loop around the IMPLICIT law on the device (simulate.rollout_implicit with
// on_device=True): n trajectories, T steps, state, last input, status and accumulators resident in
// device memory, no copy and no synchronisation between steps.  Per step a fixed sequence of
// launches on the solver handle's stream:
//
//   1 k_imp_measure   z = x + v (no error at t = 0); v drawn at (x, u_{t-1}) under a noise model
//   2 phase one       the n * n_delta (trajectory, commutation) pairs, commutation-major: pair
//                     i = d n + q reads z of trajectory q through K2Gather::src -- no parameter is
//                     replicated; segments [0, n, 2n, ...]; verdict tau <= EHM_FEAS_TOL
//   3 k_imp_count,    order-preserving compaction of the feasible pairs of live trajectories, per
//     k_imp_compact   commutation segment: src / dst lists, new segments, a device-side count
//   4 point solve     on the compacted list (results land at the pair's own index), then
//     k_imp_select    min J over the pairs with status 0, FIRST commutation within EHM_TIE_TOL of
//                     it (the rule of ehm_solve_pt_batch); none: status 3
//   5 k_imp_step      region check of the commutation's step-0 mode at the TRUE state (status 2),
//                     stage cost, ||u||_2, e and d drawn at (x, u), the plant step with u + e,
//                     worst Gx x+ - gx, records
//
// The two solves are the launches ehm_solve_pt_batch makes (ehm_imp_point, ehm_implicit.h): the
// same kernel instance on the same (z, commutation) inputs.  What the host path adds and this loop
// cannot without leaving the device is the generation-1 re-solve of a stalled LP, in EITHER solve:
// a phase-one solve that ends with a non-zero status keeps the tau it reached (its verdict may
// differ from the host's), a feasible pair whose point solve ends with one is left out of the
// minimum; both are counted and the trajectory flagged.
//
// Known costs, not attacked here: phase one keeps solving the n_delta pairs of a stopped
// trajectory for the rest of the horizon (the compaction drops them before the point solve), and
// every workgroup of k_imp_compact sums the tile counts before its own (tiles * n_delta loads per
// workgroup: 3 240 tiles at 10 000 x 81, about 40 000 at a full 768 MB chunk of that law -- a
// per-segment prefix from k_imp_count would remove it).
//
// Arithmetic of the kernels in this file: every sum in a fixed order from 0.0, one rounding per
// product and per sum (fp-contract off), so a numpy mirror reproduces every state bit for bit:
// the plant step is ((A x) + (B u)) + w, then + (E d), each product summed over its columns; a
// guarded plant steps as simulate.GuardedPlant does (one running sum over A's, then B's columns,
// then + w).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/ehmpc.h"
#include "ehm_host.h"
#include "ehm_implicit.h"
#include "ehm_rollout_dev.h"

#define EHM_I_MAX_P 8        // EHM_MAX_P
#define EHM_I_TILE 256       // pairs per workgroup of the compaction kernels

namespace {

enum ImpKind { IK_NOMINAL, IK_NOISY, IK_GUARDED, IK_KINDS };

struct ImpArgs {
    long long n;             // trajectories
    int T, t, n_delta, n_u;
    double tol_exit;
    const double *d, *v;     // the caller's [T][n][n_d], [T][n][p], or nullptr
    const int32_t* mode_of;  // [n_delta] step-0 mode of each commutation
    // per trajectory
    double *x, *z, *u_prev, *u0, *cost, *u_norm, *max_viol;
    int32_t *didx, *steps, *status, *stalled;
    // per pair i = d n + q
    double *tau, *J, *pu0;
    int32_t *st1, *st2;      // status words of phase one and of the point solve
    // time-major records (nullptr: not asked for), pre-filled with NaN / -1
    double *x_traj, *u_traj, *v_traj, *e_traj, *w_traj;
    int32_t *comm_traj, *mode_traj;
    unsigned long long* counts;      // [0] stalled pairs (both solves), [1] point LPs solved,
                                     // [2] stalled phase-one pairs
};

// the pairs of the second solve: feasible by phase one, trajectory still running
__device__ __forceinline__ bool imp_listed(const ImpArgs& A, long long i, long long q) {
    return A.status[q] == 0 && A.tau[i] <= EHM_FEAS_TOL;
}

// state of every trajectory, the dense instance list of phase one and its segments
__global__ void k_imp_init(ImpArgs A, int p, const double* __restrict__ x0,
                           long long* __restrict__ src1, int32_t* __restrict__ seg1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < A.n * A.n_delta) src1[i] = (i % A.n) * p;
    if (i <= A.n_delta) seg1[i] = (int32_t)(i * A.n);
    if (i >= A.n) return;
    for (int c = 0; c < p; ++c) {
        const double v = x0[i * p + c];
        A.x[i * p + c] = v;
        A.z[i * p + c] = v;
        if (A.x_traj) A.x_traj[i * p + c] = v;
    }
    for (int c = 0; c < A.n_u; ++c) A.u_prev[i * A.n_u + c] = 0.0;
    A.cost[i] = 0.0;
    A.u_norm[i] = 0.0;
    A.max_viol[i] = -__builtin_inf();
    A.steps[i] = A.T;
    A.status[i] = 0;
    A.stalled[i] = 0;
}

// Stage 1.  A stopped trajectory keeps its last z (the solver still sees a finite parameter; its
// pairs are dropped by the compaction).
template <int P, int NU, bool NOISY>
__global__ __launch_bounds__(256) void k_imp_measure(ImpArgs A, DevNoise NZ) {
#pragma clang fp contract(off)
    extern __shared__ double sh[];
    if constexpr (NOISY) {
        for (int i = threadIdx.x; i < NZ.total; i += blockDim.x) sh[i] = NZ.data[i];
        __syncthreads();
    }
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n || A.status[q] != 0) return;
    const long long n = A.n;
    const int t = A.t;
    double x[P], z[P];
#pragma unroll
    for (int c = 0; c < P; ++c) x[c] = A.x[q * P + c];
    if constexpr (NOISY) {
        double up[NU], vn[P];
#pragma unroll
        for (int c = 0; c < NU; ++c) up[c] = A.u_prev[q * NU + c];
        noise_kind<P, NU, P>(NZ, sh, 1, P, NZ.traj0 + (uint64_t)q, (uint64_t)t, x, up, vn);
        if (A.v_traj)
#pragma unroll
            for (int c = 0; c < P; ++c) A.v_traj[((size_t)t * n + q) * P + c] = vn[c];
#pragma unroll
        for (int c = 0; c < P; ++c) z[c] = t > 0 ? x[c] + vn[c] : x[c];
    } else if (A.v && t > 0) {
#pragma unroll
        for (int c = 0; c < P; ++c) z[c] = x[c] + A.v[((size_t)t * n + q) * P + c];
    } else {
#pragma unroll
        for (int c = 0; c < P; ++c) z[c] = x[c];
    }
#pragma unroll
    for (int c = 0; c < P; ++c) A.z[q * P + c] = z[c];
}

// Stage 3.  Grid (tiles, n_delta): workgroup (tile, d) owns the pairs d n + [256 tile, 256 tile +
// 256).  k_imp_count leaves the listed pairs of every tile; k_imp_compact sums the tiles before its
// own (segments in order, tiles in order), ranks its pairs by ballot and prefix, and writes them:
// the list holds the listed pairs in ascending pair index, whatever the scheduling.
__global__ __launch_bounds__(EHM_I_TILE) void k_imp_count(ImpArgs A, int32_t* __restrict__ tilecnt) {
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const long long q = (long long)blockIdx.x * EHM_I_TILE + threadIdx.x;
    const int d = blockIdx.y;
    const bool in = q < A.n && imp_listed(A, d * A.n + q, q);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(in);
    if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, __popcll(mask));
    __syncthreads();
    if (threadIdx.x == 0) tilecnt[(size_t)d * gridDim.x + blockIdx.x] = cnt;
}

__global__ __launch_bounds__(EHM_I_TILE) void k_imp_compact(
    ImpArgs A, int p, const int32_t* __restrict__ tilecnt, long long* __restrict__ src2,
    int32_t* __restrict__ dst2, int32_t* __restrict__ seg2, int32_t* __restrict__ n_dev) {
    __shared__ int base, wave_cnt[EHM_I_TILE / 64];
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int d = blockIdx.y;
    const long long mine = (long long)d * gridDim.x + blockIdx.x;
    int part = 0;
    for (long long k = threadIdx.x; k < mine; k += EHM_I_TILE) part += tilecnt[k];
    if (part) atomicAdd(&base, part);       // integer sum: the same whatever the order
    const long long q = (long long)blockIdx.x * EHM_I_TILE + threadIdx.x;
    const long long i = d * A.n + q;
    const bool in = q < A.n && imp_listed(A, i, q);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(in);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    if (in) {
        src2[pos] = q * p;
        dst2[pos] = (int32_t)i;
    }
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) seg2[d] = base;
        if (blockIdx.x == gridDim.x - 1 && d == (int)gridDim.y - 1) {
            int total = base;
            for (int w = 0; w < EHM_I_TILE / 64; ++w) total += wave_cnt[w];
            seg2[A.n_delta] = total;
            *n_dev = total;
            A.counts[1] += (unsigned long long)total;      // the only writer, launches in order
        }
    }
}

// Stage 4, after the point solve: the rule of ehm_solve_pt_batch.
__global__ void k_imp_select(ImpArgs A) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n || A.status[q] != 0) return;
    const int n_u = A.n_u;
    double jm = __builtin_inf();
    int n_stalled = 0, n_stalled1 = 0;
    for (int d = 0; d < A.n_delta; ++d) {
        const long long i = d * A.n + q;
        // a phase-one solve that did not converge: its tau stands (the host path would repeat the
        // solve on the generation-1 kernels before it takes the verdict), the pair is counted
        if (A.st1[i] != 0) ++n_stalled1;
        if (!(A.tau[i] <= EHM_FEAS_TOL)) continue;
        if (A.st2[i] != 0) {
            ++n_stalled;
            continue;
        }
        const double J = A.J[i];
        jm = (J < jm) ? J : jm;
    }
    int sel = -1;
    const double bound = jm + EHM_TIE_TOL * (1.0 + fabs(jm));
    for (int d = 0; d < A.n_delta && sel < 0; ++d) {
        const long long i = d * A.n + q;
        if (A.tau[i] <= EHM_FEAS_TOL && A.st2[i] == 0 && A.J[i] <= bound) sel = d;
    }
    bool bad = sel < 0;
    for (int c = 0; c < n_u; ++c) {
        const double u = bad ? __builtin_nan("") : A.pu0[(sel * A.n + q) * n_u + c];
        A.u0[q * n_u + c] = u;
        bad = bad || !(fabs(u) < __builtin_inf());
    }
    A.didx[q] = sel;
    if (n_stalled + n_stalled1) {
        A.stalled[q] = 1;
        atomicAdd(&A.counts[0], (unsigned long long)(n_stalled + n_stalled1));
        if (n_stalled1) atomicAdd(&A.counts[2], (unsigned long long)n_stalled1);
    }
    if (bad) {
        A.status[q] = 3;
        A.steps[q] = A.t;
    }
}

// Stage 5.
template <int P, int NU, ImpKind KIND>
__global__ __launch_bounds__(256) void k_imp_step(ImpArgs A, DevPlant PL, DevNoise NZ,
                                                  DevGuard GD) {
#pragma clang fp contract(off)
    constexpr bool NOISY = KIND == IK_NOISY, GUARDED = KIND == IK_GUARDED;
    extern __shared__ double sh[];
    for (int i = threadIdx.x; i < PL.total; i += blockDim.x) sh[i] = PL.data[i];
    if constexpr (NOISY)
        for (int i = threadIdx.x; i < NZ.total; i += blockDim.x) sh[PL.total + i] = NZ.data[i];
    __syncthreads();
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.n || A.status[q] != 0) return;
    const long long n = A.n;
    const int t = A.t;
    const double* sQ = sh + PL.oQ;
    const double* sR = sh + PL.oR;
    const double* sG = sh + PL.oG;
    const double* sg = sh + PL.og;
    const double* sE = sh + PL.oE;
    const double* sn = sh + PL.total;
    double x[P], u[NU], ua[NU], xn[P];
#pragma unroll
    for (int c = 0; c < P; ++c) x[c] = A.x[q * P + c];
#pragma unroll
    for (int c = 0; c < NU; ++c) u[c] = A.u0[q * NU + c];
    const int didx = A.didx[q];
    const int m = A.mode_of[didx];
    if constexpr (!GUARDED) {
        bool in_region = m >= 0 && m < PL.n_modes;
        if (in_region)
            for (int r = PL.row0[m]; r < PL.row0[m + 1]; ++r) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < P; ++c) s += sh[PL.oH + r * P + c] * x[c];
                in_region = in_region && (s <= sh[PL.oh + r] + A.tol_exit);
            }
        if (!in_region) {
            A.status[q] = 2;
            A.steps[q] = t;
            return;
        }
    }
    if (A.u_traj)
#pragma unroll
        for (int c = 0; c < NU; ++c) A.u_traj[((size_t)t * n + q) * NU + c] = u[c];
    if (A.comm_traj) A.comm_traj[(size_t)t * n + q] = didx;
    if (A.mode_traj) A.mode_traj[(size_t)t * n + q] = m;
    // stage cost and input 2-norm
    double su = 0.0;
#pragma unroll
    for (int c = 0; c < NU; ++c) su += u[c] * u[c];
    A.u_norm[q] += sqrt(su);
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
        A.cost[q] += qx + ru;
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
        A.cost[q] += s;
    }
    // input error and process noise at (x, u)
#pragma unroll
    for (int c = 0; c < NU; ++c) ua[c] = u[c];
    double wn[EHM_R_MAX_D];
    if constexpr (NOISY) {
        double en[NU];
        const uint64_t id = NZ.traj0 + (uint64_t)q;
        noise_kind<P, NU, NU>(NZ, sn, 2, NU, id, (uint64_t)t, x, u, en);
        if (su == 0.0)
#pragma unroll
            for (int c = 0; c < NU; ++c) en[c] = 0.0;
        noise_kind<P, NU, EHM_R_MAX_D>(NZ, sn, 0, PL.n_d, id, (uint64_t)t, x, u, wn);
#pragma unroll
        for (int c = 0; c < NU; ++c) ua[c] = u[c] + en[c];
        if (A.e_traj)
#pragma unroll
            for (int c = 0; c < NU; ++c) A.e_traj[((size_t)t * n + q) * NU + c] = en[c];
        if (A.w_traj)
#pragma unroll
            for (int j = 0; j < EHM_R_MAX_D; ++j)
                if (j < PL.n_d) A.w_traj[((size_t)t * n + q) * PL.n_d + j] = wn[j];
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
        // x+ = ((A_m x) + (B_m (u + e))) + w_m, then + (E d)
        const double* sA = sh + PL.oA + m * P * P;
        const double* sB = sh + PL.oB + m * P * NU;
        const double* sw = sh + PL.ow + m * P;
        const double* dt = (!NOISY && A.d) ? A.d + ((size_t)t * n + q) * PL.n_d : nullptr;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            double ax = 0.0, bu = 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) ax += sA[i * P + c] * x[c];
#pragma unroll
            for (int c = 0; c < NU; ++c) bu += sB[i * NU + c] * ua[c];
            double s = (ax + bu) + sw[i];
            if constexpr (NOISY) {
                if (PL.n_d > 0) {
                    double ed = 0.0;
#pragma unroll
                    for (int j = 0; j < EHM_R_MAX_D; ++j)
                        if (j < PL.n_d) ed += sE[i * PL.n_d + j] * wn[j];
                    s = s + ed;
                }
            } else if (dt) {
                double ed = 0.0;
                for (int j = 0; j < PL.n_d; ++j) ed += sE[i * PL.n_d + j] * dt[j];
                s = s + ed;
            }
            xn[i] = s;
        }
    }
    double maxv = A.max_viol[q];
    for (int j = 0; j < PL.n_g; ++j) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) s += sG[j * P + c] * xn[c];
        maxv = fmax(maxv, s - sg[j]);
    }
    A.max_viol[q] = maxv;
#pragma unroll
    for (int c = 0; c < P; ++c) A.x[q * P + c] = xn[c];
#pragma unroll
    for (int c = 0; c < NU; ++c) A.u_prev[q * NU + c] = u[c];
    if (A.x_traj)
#pragma unroll
        for (int c = 0; c < P; ++c) A.x_traj[((size_t)(t + 1) * n + q) * P + c] = xn[c];
}

typedef void (*measure_fn)(ImpArgs, DevNoise);
typedef void (*step_fn)(ImpArgs, DevPlant, DevNoise, DevGuard);
#define EHM_I_M_NU(P, Z) &k_imp_measure<P, 1, Z>, &k_imp_measure<P, 2, Z>, \
                         &k_imp_measure<P, 3, Z>, &k_imp_measure<P, 4, Z>
#define EHM_I_S_NU(P, K) &k_imp_step<P, 1, K>, &k_imp_step<P, 2, K>, &k_imp_step<P, 3, K>, \
                         &k_imp_step<P, 4, K>
#define EHM_I_ALL(F, K) {{F(1, K)}, {F(2, K)}, {F(3, K)}, {F(4, K)}, {F(5, K)}, {F(6, K)}, \
                         {F(7, K)}, {F(8, K)}}
// [noisy][p - 1][n_u - 1] and [kind][p - 1][n_u - 1]
const measure_fn k_measure_table[2][EHM_I_MAX_P][EHM_R_MAX_NU] = {EHM_I_ALL(EHM_I_M_NU, false),
                                                                  EHM_I_ALL(EHM_I_M_NU, true)};
const step_fn k_step_table[IK_KINDS][EHM_I_MAX_P][EHM_R_MAX_NU] = {
    EHM_I_ALL(EHM_I_S_NU, IK_NOMINAL), EHM_I_ALL(EHM_I_S_NU, IK_NOISY),
    EHM_I_ALL(EHM_I_S_NU, IK_GUARDED)};
#undef EHM_I_ALL
#undef EHM_I_S_NU
#undef EHM_I_M_NU

thread_local ehm_err_channel i_err;
// a call into the solver handle: its message travels with the code
#define I_SOLVER(expr)                                                                     \
    do {                                                                                   \
        const int rc_ = (expr);                                                            \
        if (rc_ != EHM_OK) return i_err.fail(rc_, "%s", ehm_last_error());                      \
    } while (0)

}  // namespace

struct ehm_implicit {
    ehm_problem* prob = nullptr;
    ImpProblem ip{};
    DevBuf plant, mode_of, noise;
    DevPlant pl{};
    bool guarded = false;
    DevGuard gd{};
    DevNoise nz{};
    int noise_n_d = 0;
};

namespace {

// What the two plant setters share (the counterpart of install_plant in ehm_explicit.hip, with
// one mode per commutation instead of one per node).
template <class Own>
int imp_install_plant(ehm_implicit* I, const char* who, int32_t n_modes, int max_modes,
                      const double* A, const double* B, const double* w, int32_t n_g,
                      const double* Gx, const double* gx, const int32_t* mode_of,
                      int32_t cost_kind, const double* Q, const double* R, const DevGuard* gd,
                      Own own) {
    if (!I || !A || !B || !w || !mode_of || !Q || !R)
        return i_err.fail(EHM_E_INVALID, "%s: a required array is NULL", who);
    if (n_modes < 1 || n_modes > max_modes)
        return i_err.fail(EHM_E_INVALID, "%s: %d modes (1..%d)", who, (int)n_modes, max_modes);
    if (n_g < 0 || n_g > EHM_R_MAX_ROWS || (n_g > 0 && (!Gx || !gx)))
        return i_err.fail(EHM_E_INVALID, "%s: n_g = %d (0..%d)", who, (int)n_g, EHM_R_MAX_ROWS);
    if (cost_kind != 0 && cost_kind != 1)
        return i_err.fail(EHM_E_INVALID, "%s: cost_kind %d (0 inf-norm, 1 quadratic)", who,
                          (int)cost_kind);
    const int p = I->ip.p, n_u = I->ip.n_u, nd = I->ip.n_delta;
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
    if (pl.total > EHM_N_MAX_LDS)
        return i_err.fail(EHM_E_INVALID, "%s: the plant takes %d doubles of LDS (%d)", who,
                          pl.total, EHM_N_MAX_LDS);
    for (int d = 0; d < nd; ++d)
        if (mode_of[d] < 0 || (!gd && mode_of[d] >= n_modes))
            return i_err.fail(EHM_E_INVALID, "%s: commutation %d has mode %d of %d", who, d,
                              (int)mode_of[d], (int)n_modes);
    EHM_HIP_TRY(i_err, hipSetDevice(I->ip.device));
    DevBuf d_plant, d_mode;
    if (d_plant.upload(pk.buf.data(), pk.buf.size() * sizeof(double)) != hipSuccess ||
        d_mode.upload(mode_of, (size_t)nd * sizeof(int32_t)) != hipSuccess)
        return i_err.fail(EHM_E_HIP, "%s: device allocation / copy failed", who);
    I->plant = std::move(d_plant);
    I->mode_of = std::move(d_mode);
    pl.data = I->plant.as<const double>();
    I->pl = pl;
    I->guarded = gd != nullptr;
    if (gd) I->gd = *gd;
    return EHM_OK;
}

}  // namespace

extern "C" {

const char* ehm_implicit_last_error(void) { return i_err.c_str(); }

int ehm_implicit_destroy(ehm_implicit* I) {
    if (!I) return EHM_OK;
    (void)hipSetDevice(I->ip.device);
    delete I;
    return EHM_OK;
}

int ehm_implicit_create(ehm_problem* prob, ehm_implicit** out) {
    if (!prob || !out) return i_err.fail(EHM_E_INVALID, "bad argument");
    *out = nullptr;
    ImpProblem ip{};
    I_SOLVER(ehm_imp_describe(prob, &ip));
    if (ip.p < 1 || ip.p > EHM_I_MAX_P || ip.n_u < 1 || ip.n_u > EHM_R_MAX_NU)
        return i_err.fail(EHM_E_INVALID, "the device loop takes p <= %d and n_u <= %d (p %d, n_u "
                          "%d)", EHM_I_MAX_P, EHM_R_MAX_NU, ip.p, ip.n_u);
    ehm_implicit* I = new ehm_implicit();
    I->prob = prob;
    I->ip = ip;
    *out = I;
    return EHM_OK;
}

int ehm_implicit_set_plant(ehm_implicit* I, int32_t n_modes, const double* A, const double* B,
                           const double* w, int32_t n_d, const double* Emat,
                           const int32_t* region_rows, const double* H, const double* h,
                           int32_t n_g, const double* Gx, const double* gx,
                           const int32_t* mode_of, int32_t cost_kind, const double* Q,
                           const double* R) {
    return imp_install_plant(
        I, "implicit_set_plant", n_modes, EHM_R_MAX_MODES, A, B, w, n_g, Gx, gx, mode_of,
        cost_kind, Q, R, nullptr, [&](Pack& pk, DevPlant& pl, int p, int) {
            if (n_d < 0 || n_d > EHM_R_MAX_D || (n_d > 0 && !Emat))
                return i_err.fail(EHM_E_INVALID, "implicit_set_plant: n_d = %d (0..%d, E needed if "
                                  "> 0)", (int)n_d, EHM_R_MAX_D);
            int rows = 0;
            for (int m = 0; m < n_modes; ++m) {
                const int r = region_rows ? region_rows[m] : 0;
                if (r < 0)
                    return i_err.fail(EHM_E_INVALID, "implicit_set_plant: mode %d has %d region "
                                      "rows", m, r);
                pl.row0[m] = rows;
                rows += r;
            }
            if (rows > EHM_R_MAX_ROWS || (rows > 0 && (!H || !h)))
                return i_err.fail(EHM_E_INVALID, "implicit_set_plant: %d mode-region rows (0..%d)",
                                  rows, EHM_R_MAX_ROWS);
            for (int m = n_modes; m <= EHM_R_MAX_MODES; ++m) pl.row0[m] = rows;
            pl.n_d = n_d;
            pl.oE = pk.put(Emat, (size_t)p * n_d);
            pl.oH = pk.put(H, (size_t)rows * p);
            pl.oh = pk.put(h, (size_t)rows);
            return (int)EHM_OK;
        });
}

int ehm_implicit_set_plant_guarded(ehm_implicit* I, int32_t n_modes, const double* A,
                                   const double* B, const double* w, int32_t substeps,
                                   int32_t n_guards, const int32_t* guard_mode,
                                   const int32_t* guard_row0, const double* ga, const double* gb,
                                   const double* gc, const double* gt, const int32_t* strict,
                                   int32_t default_mode, int32_t n_g, const double* Gx,
                                   const double* gx, const int32_t* mode_of, int32_t cost_kind,
                                   const double* Q, const double* R) {
    DevGuard gd{};
    return imp_install_plant(
        I, "implicit_set_plant_guarded", n_modes, EHM_G_MAX_MODES, A, B, w, n_g, Gx, gx, mode_of,
        cost_kind, Q, R, &gd, [&](Pack& pk, DevPlant&, int p, int n_u) {
            const char* who = "implicit_set_plant_guarded";
            if ((n_guards > 0 && !guard_mode) || !guard_row0)
                return i_err.fail(EHM_E_INVALID, "%s: a required array is NULL", who);
            if (substeps < 1 || substeps > EHM_G_MAX_SUB)
                return i_err.fail(EHM_E_INVALID, "%s: %d substeps (1..%d)", who, (int)substeps,
                                  EHM_G_MAX_SUB);
            if (n_guards < 0 || n_guards > EHM_G_MAX_ROWS)
                return i_err.fail(EHM_E_INVALID, "%s: %d guards (0..%d)", who, (int)n_guards,
                                  EHM_G_MAX_ROWS);
            if (default_mode < 0 || default_mode >= n_modes)
                return i_err.fail(EHM_E_INVALID, "%s: default mode %d of %d", who,
                                  (int)default_mode, (int)n_modes);
            if (guard_row0[0] != 0)
                return i_err.fail(EHM_E_INVALID, "%s: the rows of guard 0 start at %d", who,
                                  (int)guard_row0[0]);
            gd.substeps = substeps;
            gd.n_guards = n_guards;
            gd.default_mode = default_mode;
            for (int g = 0; g <= n_guards; ++g) {
                if (g < n_guards) {
                    if (guard_mode[g] < 0 || guard_mode[g] >= n_modes)
                        return i_err.fail(EHM_E_INVALID, "%s: guard %d selects mode %d of %d", who,
                                          g, (int)guard_mode[g], (int)n_modes);
                    if (guard_row0[g + 1] <= guard_row0[g])
                        return i_err.fail(EHM_E_INVALID, "%s: guard %d has no rows", who, g);
                    gd.mode[g] = guard_mode[g];
                }
                gd.row0[g] = guard_row0[g];
            }
            const int rows = guard_row0[n_guards];
            if (rows > EHM_G_MAX_ROWS || (rows > 0 && (!ga || !gb || !gc || !gt || !strict)))
                return i_err.fail(EHM_E_INVALID, "%s: %d guard rows (0..%d)", who, rows,
                                  EHM_G_MAX_ROWS);
            for (int r = 0; r < rows; ++r) gd.strict[r] = strict[r] != 0;
            gd.oGa = pk.put(ga, (size_t)rows * p);
            gd.oGb = pk.put(gb, (size_t)rows * n_u);
            gd.oGc = pk.put(gc, (size_t)rows);
            gd.oGt = pk.put(gt, (size_t)rows);
            return (int)EHM_OK;
        });
}

int ehm_implicit_set_noise(ehm_implicit* I, int32_t n_terms, const int32_t* desc,
                           const double* data, int32_t n_data, int32_t n_d) {
    if (!I || n_terms < 0 || n_terms > EHM_N_MAX_TERMS || (n_terms > 0 && !desc) || n_data < 0 ||
        (n_data > 0 && !data) || n_d < 0 || n_d > EHM_R_MAX_D)
        return i_err.fail(EHM_E_INVALID, "implicit_set_noise: bad argument (at most %d terms, n_d "
                          "<= %d)", EHM_N_MAX_TERMS, EHM_R_MAX_D);
    DevNoise nz{};
    const int bad = noise_fill(nz, n_terms, desc, n_data, I->ip.p, I->ip.n_u, n_d);
    if (bad >= 0)
        return i_err.fail(EHM_E_INVALID, "implicit_set_noise: term %d has a bad descriptor", bad);
    if (I->pl.total + n_data > EHM_N_MAX_LDS)
        return i_err.fail(EHM_E_INVALID, "implicit_set_noise: plant and model take %d doubles of "
                          "LDS (%d)", I->pl.total + n_data, EHM_N_MAX_LDS);
    EHM_HIP_TRY(i_err, hipSetDevice(I->ip.device));
    DevBuf d_noise;
    if (d_noise.upload(data, (size_t)n_data * sizeof(double)) != hipSuccess)
        return i_err.fail(EHM_E_HIP, "implicit_set_noise: device allocation / copy failed");
    I->noise = std::move(d_noise);
    nz.data = I->noise.as<const double>();
    I->nz = nz;
    I->noise_n_d = n_d;
    return EHM_OK;
}

int ehm_implicit_rollout(ehm_implicit* I, int64_t n, int32_t T, const double* x0, const double* d,
                         const double* v, int32_t noisy, uint64_t seed, uint64_t traj0,
                         double tol_exit, double* x_traj, double* u_traj,
                         int32_t* commutation_traj, int32_t* mode_traj, double* v_traj,
                         double* e_traj, double* w_traj, double* x_final, int32_t* steps,
                         int32_t* status, double* cost, double* u_norm_sum,
                         double* max_violation, int32_t* stalled, int64_t* counts,
                         double* device_seconds) {
    if (!I || !x0 || !x_final || !steps || !status || !cost || !u_norm_sum || !max_violation ||
        !stalled || !counts || n < 0 || T < 0 || !(tol_exit >= 0.0))
        return i_err.fail(EHM_E_INVALID, "implicit_rollout: bad argument");
    if (!I->plant) return i_err.fail(EHM_E_INVALID, "implicit_rollout: no plant "
                                     "(ehm_implicit_set_plant)");
    const int p = I->ip.p, n_u = I->ip.n_u, nd = I->ip.n_delta, n_d = I->pl.n_d;
    if (noisy) {
        if (d || v)
            return i_err.fail(EHM_E_INVALID, "implicit_rollout: the model draws d and v itself");
        if (!I->noise)
            return i_err.fail(EHM_E_INVALID, "implicit_rollout: no model (ehm_implicit_set_noise)");
        if (I->guarded)
            return i_err.fail(EHM_E_INVALID, "implicit_rollout: the plant is guarded (noisy "
                              "guarded plants are not supported)");
        if (I->noise_n_d != n_d)
            return i_err.fail(EHM_E_INVALID, "implicit_rollout: the model has n_d = %d, the plant "
                              "%d", I->noise_n_d, n_d);
        if (I->pl.total + I->nz.total > EHM_N_MAX_LDS)
            return i_err.fail(EHM_E_INVALID, "implicit_rollout: plant and model take %d doubles of "
                              "LDS (%d)", I->pl.total + I->nz.total, EHM_N_MAX_LDS);
    }
    if (d && (n_d == 0 || I->guarded))
        return i_err.fail(EHM_E_INVALID, "implicit_rollout: a disturbance was given but the plant "
                                         "takes none");
    for (int k = 0; k < 5; ++k) counts[k] = 0;
    if (n == 0) return EHM_OK;
    if (nd > 65535)
        return i_err.fail(EHM_E_INVALID, "implicit_rollout: %d commutations (the compaction grid "
                          "takes 65535)", nd);
    if (n * nd >= (int64_t)1 << 31)
        return i_err.fail(EHM_E_INVALID, "implicit_rollout: %lld trajectories x %d commutations "
                          "(split the batch)", (long long)n, nd);
    EHM_HIP_TRY(i_err, hipSetDevice(I->ip.device));
    hipStream_t st = I->ip.stream;
    const size_t N = (size_t)n, nT = (size_t)T, K = N * nd, D = sizeof(double),
                 I4 = sizeof(int32_t);
    const int tiles = (int)((n + EHM_I_TILE - 1) / EHM_I_TILE);
    ImpArgs A{};
    A.n = n;
    A.T = T;
    A.n_delta = nd;
    A.n_u = n_u;
    A.tol_exit = tol_exit;
    A.mode_of = I->mode_of.as<const int32_t>();
    // device arrays: the host array they are copied to at the end (nullptr: stays on the device;
    // records not asked for are not allocated), the ImpArgs pointer, bytes, whether a record
    struct Buf {
        void* host;
        void* field;
        size_t bytes;
        bool record;
        DevBuf buf;
    } bufs[] = {
        {x_final, &A.x, N * p * D, false},
        {steps, &A.steps, N * I4, false},
        {status, &A.status, N * I4, false},
        {cost, &A.cost, N * D, false},
        {u_norm_sum, &A.u_norm, N * D, false},
        {max_violation, &A.max_viol, N * D, false},
        {stalled, &A.stalled, N * I4, false},
        {nullptr, &A.z, N * p * D, false},
        {nullptr, &A.u_prev, N * n_u * D, false},
        {nullptr, &A.u0, N * n_u * D, false},
        {nullptr, &A.didx, N * I4, false},
        {nullptr, &A.tau, K * D, false},
        {nullptr, &A.J, K * D, false},
        {nullptr, &A.pu0, K * n_u * D, false},
        {nullptr, &A.st1, K * I4, false},
        {nullptr, &A.st2, K * I4, false},
        {x_traj, &A.x_traj, (nT + 1) * N * p * D, true},
        {u_traj, &A.u_traj, nT * N * n_u * D, true},
        {commutation_traj, &A.comm_traj, nT * N * I4, true},
        {mode_traj, &A.mode_traj, nT * N * I4, true},
        {noisy ? v_traj : nullptr, &A.v_traj, nT * N * p * D, true},
        {noisy ? e_traj : nullptr, &A.e_traj, nT * N * n_u * D, true},
        {noisy ? w_traj : nullptr, &A.w_traj, nT * N * n_d * D, true},
    };
    DevBuf dx0, dd, dv, src1, src2, dst2, seg1, seg2, ndev, tilecnt, dcounts;
    bool ok = dx0.alloc(N * p * D) == hipSuccess &&
              (!d || dd.alloc(nT * N * n_d * D) == hipSuccess) &&
              (!v || dv.alloc(nT * N * p * D) == hipSuccess) &&
              src1.alloc(K * sizeof(long long)) == hipSuccess &&
              src2.alloc(K * sizeof(long long)) == hipSuccess && dst2.alloc(K * I4) == hipSuccess &&
              seg1.alloc((nd + 1) * I4) == hipSuccess && seg2.alloc((nd + 1) * I4) == hipSuccess &&
              ndev.alloc(I4) == hipSuccess && tilecnt.alloc((size_t)tiles * nd * I4) == hipSuccess &&
              dcounts.alloc(3 * sizeof(unsigned long long)) == hipSuccess;
    for (Buf& b : bufs)
        if (ok && (b.host || !b.record)) {
            ok = b.buf.alloc(b.bytes) == hipSuccess;
            std::memcpy(b.field, &b.buf.ptr, sizeof b.buf.ptr);
        }
    if (!ok)
        return i_err.fail(EHM_E_HIP, "implicit_rollout: out of device memory for %lld x %d steps x "
                          "%d commutations", (long long)n, (int)T, nd);
    A.d = dd.as<const double>();
    A.v = dv.as<const double>();
    A.counts = dcounts.as<unsigned long long>();
    EHM_HIP_TRY(i_err, hipMemcpyAsync(dx0.ptr, x0, N * p * D, hipMemcpyHostToDevice, st));
    if (d) EHM_HIP_TRY(i_err, hipMemcpyAsync(dd.ptr, d, nT * N * n_d * D, hipMemcpyHostToDevice,
                                             st));
    if (v) EHM_HIP_TRY(i_err, hipMemcpyAsync(dv.ptr, v, nT * N * p * D, hipMemcpyHostToDevice, st));
    EHM_HIP_TRY(i_err, hipMemsetAsync(dcounts.ptr, 0, 3 * sizeof(unsigned long long), st));
    // records of steps a trajectory does not reach: all-ones bytes, i.e. NaN and -1
    for (Buf& b : bufs)
        if (b.record && b.buf) EHM_HIP_TRY(i_err, hipMemsetAsync(b.buf.ptr, 0xff, b.bytes, st));
    DevNoise NZ{};
    size_t lds_step = (size_t)I->pl.total * D, lds_meas = 0;
    if (noisy) {
        NZ = I->nz;
        NZ.seed = seed;
        NZ.traj0 = traj0;
        lds_step += (size_t)NZ.total * D;
        lds_meas = (size_t)NZ.total * D;
    }
    const measure_fn f_meas = k_measure_table[noisy ? 1 : 0][p - 1][n_u - 1];
    const step_fn f_step =
        k_step_table[noisy ? IK_NOISY : I->guarded ? IK_GUARDED : IK_NOMINAL][p - 1][n_u - 1];
    const dim3 g_traj((unsigned)((n + 255) / 256)), g_pair((unsigned)((K + nd + 255) / 256)),
        g_tile((unsigned)tiles, (unsigned)nd);
    EventPair ev;
    (void)hipEventRecord(ev.e0, st);
    hipLaunchKernelGGL(k_imp_init, g_pair, dim3(256), 0, st, A, p, dx0.as<const double>(),
                       src1.as<long long>(), seg1.as<int32_t>());
    for (int t = 0; t < T; ++t) {
        A.t = t;
        hipLaunchKernelGGL(f_meas, g_traj, dim3(256), lds_meas, st, A, NZ);
        I_SOLVER(ehm_imp_point(I->prob, 1, (long long)K, A.z, seg1.as<const int32_t>(), A.tau,
                               nullptr, A.st1, src1.as<const long long>(), nullptr, nullptr));
        hipLaunchKernelGGL(k_imp_count, g_tile, dim3(EHM_I_TILE), 0, st, A,
                           tilecnt.as<int32_t>());
        hipLaunchKernelGGL(k_imp_compact, g_tile, dim3(EHM_I_TILE), 0, st, A, p,
                           tilecnt.as<const int32_t>(), src2.as<long long>(), dst2.as<int32_t>(),
                           seg2.as<int32_t>(), ndev.as<int32_t>());
        I_SOLVER(ehm_imp_point(I->prob, 0, (long long)K, A.z, seg2.as<const int32_t>(), A.J, A.pu0,
                               A.st2, src2.as<const long long>(), dst2.as<const int32_t>(),
                               ndev.as<const int32_t>()));
        hipLaunchKernelGGL(k_imp_select, g_traj, dim3(256), 0, st, A);
        hipLaunchKernelGGL(f_step, g_traj, dim3(256), lds_step, st, A, I->pl, NZ, I->gd);
    }
    (void)hipEventRecord(ev.e1, st);
    EHM_HIP_TRY(i_err, hipGetLastError());
    for (const Buf& b : bufs)
        if (b.host) EHM_HIP_TRY(i_err, hipMemcpyAsync(b.host, b.buf.ptr, b.bytes,
                                                      hipMemcpyDeviceToHost, st));
    unsigned long long c2[3] = {0, 0, 0};
    EHM_HIP_TRY(i_err, hipMemcpyAsync(c2, dcounts.ptr, sizeof c2, hipMemcpyDeviceToHost, st));
    EHM_HIP_TRY(i_err, hipStreamSynchronize(st));
    ev.seconds(device_seconds);
    counts[0] = (int64_t)c2[0];              // stalled pairs, both solves
    counts[1] = (int64_t)K * T;              // phase-one LPs
    counts[2] = (int64_t)c2[1];              // point LPs
    counts[3] = 1 + 7LL * T;                 // launches of the fixed sequence (set-up + 7 per step)
    counts[4] = (int64_t)c2[2];              // stalled pairs of phase one
    return EHM_OK;
}

}  // extern "C"
