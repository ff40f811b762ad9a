// Second-generation kernels of libehmpc (gfx950): one copy of the commutation's constant LP
// block in LDS per workgroup, several wavefronts per workgroup, each solving its own LP.
// Compiled once per (EHM_NP, EHM_SLOTS) pair; ehm_capi.hip picks the instance that fits
// the LP of each launch.  See ehm_ipm2.h for the solver, ehm_k2_asm.h for the assembly of the
// oracle problems and DESIGN.md section 3.
#include <hip/hip_runtime.h>

#include "ehm_k2_asm.h"

using namespace ehm;

namespace EHM2_NS {

#if EHM2_PROF
#define K2_PROF_HOOK(S) S.gprof = cnt ? cnt->phase : nullptr;
#else
#define K2_PROF_HOOK(S)
#endif
#define K2_PROLOGUE()                                                            \
    double* sm = reinterpret_cast<double*>(k2_smem);                             \
    __shared__ int s_ctr;                                                        \
    const int tid = threadIdx.x;                                                 \
    const int lane0 = tid & 63;                                                  \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   /* uniform: SGPR pointers */ \
    Shared S;                                                                    \
    carve_shared(S, sm, P);                                                      \
    K2_PROF_HOOK(S)                                                              \
    NodeBuf nb;                                                                  \
    carve_node(nb, sm + shared_doubles(P) + (size_t)wave * wave_doubles, P.p, P.n_u)

// ---- a2: P_theta_delta batch / its feasibility form; instances sorted by commutation -----
// (compiled once per kind: with the kind a compile-time constant the assembly of the other kinds
// is not in the kernel, which is what keeps it near the register budget)
template <int feas>
__global__ __launch_bounds__(EHM_K2_THREADS) void k2_point_batch(
    DevProblem P, long long n_inst, const double* __restrict__ theta,
    const int32_t* __restrict__ seg, double* __restrict__ J, double* __restrict__ u0,
    int32_t* __restrict__ status, int32_t* __restrict__ iters, DevCounters* cnt,
    int wave_doubles, K2Gather G) {
    K2_PROLOGUE();
    if (G.n_dev) n_inst = *G.n_dev;
    const long long t_start = wall_clock64();
    const long long per = (n_inst + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per;
    const long long hi = (lo + per < n_inst) ? lo + per : n_inst;
    long long pos = lo;
    while (pos < hi) {      // workgroup-uniform
        int d = 0;
        while (d + 1 < P.n_delta && seg[d + 1] <= pos) ++d;
        const long long run_end = (seg[d + 1] < hi) ? seg[d + 1] : hi;
        __syncthreads();
        load_shared(P, d, sm, tid, blockDim.x);
        use_commutation(S, P, d);
        if (tid == 0) s_ctr = (int)(pos - lo);
        __syncthreads();
        for (;;) {
            const long long inst = lo + pull(&s_ctr, lane0);
            if (inst >= run_end) break;
            const int lane = pin(lane0);
            const double* tsrc = G.src ? theta + G.src[inst] : theta + inst * P.p;
            const long long o = G.dst ? (long long)G.dst[inst] : inst;
            if (lane < P.p) nb.th[lane] = tsrc[lane];
            wsync();
            // shared results (K2Gather::pt): the first wavefront to ask for (parameter,
            // commutation, kind) solves and publishes, the others take the entry -- an LP's
            // optimum does not depend on who solves it
            int pt_res = MT_NONE, pt_slot = 0;
            unsigned long long pt_tg = 0ull;
            const unsigned int pt_kind = (unsigned int)((d * 2 + (feas ? 1 : 0)) * 4 + G.sign_mode);
            if (G.pt.state && !G.grad) {
                unsigned int pt_i = 0u;
                pt_tg = pt_tag(nb.th, P.p, pt_kind, G.pt.mask, &pt_i);
                if (lane == 0)
                    pt_res = mt_claim(G.pt, pt_tg, pt_i, t_start, 60LL * 100000000LL, &pt_slot);
                pt_res = __builtin_amdgcn_readfirstlane(pt_res);
                pt_slot = __builtin_amdgcn_readfirstlane(pt_slot);
                if (pt_res == MT_HIT) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    const double* e = G.pt.data + (size_t)pt_slot * MT_DOUBLES;
                    const double ev = lane < MT_DOUBLES ? e[lane] : 0.0;
                    const bool differs =
                        (lane < P.p && __double_as_longlong(ev) != __double_as_longlong(nb.th[lane])) ||
                        (lane == 26 && ev != (double)pt_kind);
                    if (__builtin_amdgcn_ballot_w64(differs) == 0ull) {
                        const double Jv = __shfl(ev, 8);
                        const int word = (int)__shfl(ev, 9);
                        if (lane == 0) {
                            J[o] = Jv;
                            if (status) status[o] = word;
                            if (iters) iters[o] = 0;
                            atomicAdd(&cnt->mid_shared, 1ULL);
                        }
                        if (u0 && lane >= 10 && lane < 10 + P.n_u) u0[o * P.n_u + lane - 10] = ev;
                        wsync();
                        continue;
                    }
                    pt_res = MT_NONE;           // another problem with this tag
                }
            }
            Wave W;
            IpmResult r;
            int its = 0;
            for (int attempt = 0; attempt < EHM2_ATTEMPTS; ++attempt) {     // see EHM2_STEP_FRAC
                double b[SLOTS];
                const int ln = pin(lane);     // nothing of the assembly outlives the attempt
                assemble_point(S, W, nb.lp, nb.th, feas != 0, b, ln, P, d);
                r = ipm_solve(S, W, b, ln, feas ? G.sign_mode : 0,
                              step_fraction(attempt), (G.grad && !feas) ? nb.F : nullptr);
                its += r.iters;
                if (r.status == 0) break;
            }
            r.iters = its;
            count_solve(cnt, r, lane);
            if (G.grad && !feas) {
#if EHM2_QUAD
                quad_grad_add(W, P, d, nb.th, nb.F, lane);
#endif
                if (lane < P.p) G.grad[o * P.p + lane] = nb.F[lane];
            }
            const double Jout = (feas && G.sign_mode) ? copysign(r.margin, r.obj) : r.obj;
            if (lane == 0) {
                J[o] = Jout;
                if (status) status[o] = ehm_status_word(r.status, r.merit);
                if (iters) iters[o] = r.iters;
            }
            if (u0 && lane < P.n_u) u0[o * P.n_u + lane] = W.xb[lane];
            if (pt_res == MT_OWN) {
                double* e = G.pt.data + (size_t)pt_slot * MT_DOUBLES;
                if (lane < MT_DOUBLES) {
                    double v = 0.0;
                    if (lane < 8) v = lane < P.p ? nb.th[lane] : 0.0;
                    else if (lane == 8) v = Jout;
                    else if (lane == 9) v = (double)r.status;
                    else if (lane < 18) v = lane - 10 < P.n_u ? W.xb[lane - 10] : 0.0;
                    else if (lane == 26) v = (double)pt_kind;
                    __hip_atomic_store(e + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_s_waitcnt(0);
                if (lane == 0)
                    __hip_atomic_store(&G.pt.state[pt_slot], pt_tg | 3ull, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            wsync();
        }
        pos = run_end;
    }
}

// ---- a5 / a7': problems over a simplex, one commutation per instance (sorted) -------------
template <int mode>
__global__ __launch_bounds__(EHM_K2_THREADS) void k2_simplex_batch(
    DevProblem P, long long n_inst, const double* __restrict__ R,
    const double* __restrict__ Vbar, const int32_t* __restrict__ seg,
    double* __restrict__ obj, double* __restrict__ alpha, int32_t* __restrict__ status,
    int32_t* __restrict__ iters, DevCounters* cnt, int wave_doubles, K2Gather G) {
    K2_PROLOGUE();
    const int p = P.p;
    const int nR = (p + 1) * p;
    if (G.n_dev) n_inst = *G.n_dev;
    const long long per = (n_inst + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per;
    const long long hi = (lo + per < n_inst) ? lo + per : n_inst;
    long long pos = lo;
    while (pos < hi) {
        int d = 0;
        while (d + 1 < P.n_delta && seg[d + 1] <= pos) ++d;
        const long long run_end = (seg[d + 1] < hi) ? seg[d + 1] : hi;
        __syncthreads();
        load_shared(P, d, sm, tid, blockDim.x);
        use_commutation(S, P, d);
        if (tid == 0) s_ctr = (int)(pos - lo);
        __syncthreads();
        for (;;) {
            const long long inst = lo + pull(&s_ctr, lane0);
            if (inst >= run_end) break;
            const int lane = pin(lane0);
            double* Rl = nb.rec;
            double* Vl = nb.rec + nR;
            const double* Rsrc = G.src ? R + G.src[inst] : R + inst * nR;
            const double* Vsrc = G.src ? Rsrc + G.v_off : Vbar + inst * (p + 1);
            const long long o = G.dst ? (long long)G.dst[inst] : inst;
            for (int k = lane; k < nR; k += 64) Rl[k] = Rsrc[k];
            if (mode == SX_SLACK && lane <= p) Vl[lane] = Vsrc[lane];
            wsync();
            Wave W;
            IpmResult r;
            int its = 0;
            for (int attempt = 0; attempt < EHM2_ATTEMPTS; ++attempt) {
                double b[SLOTS];
                const int ln = pin(lane);
                assemble_simplex(S, W, nb, Rl, Vl, mode, P.eps_a, P.eps_r, b, ln, P, d);
                r = ipm_solve(S, W, b, ln, (mode == SX_MIN) ? 0 : G.sign_mode,
                              step_fraction(attempt));
                its += r.iters;
                if (r.status == 0) break;
            }
            r.iters = its;
            count_solve(cnt, r, lane);
            if (lane == 0) {
                const double val = (G.sign_mode && mode != SX_MIN) ? copysign(r.margin, r.obj) : r.obj;
                obj[o] = (mode == SX_SLACK) ? -val : val;         // t* = -(min -t)
                if (status) status[o] = ehm_status_word(r.status, r.merit);
                if (iters) iters[o] = r.iters;
            }
            if (alpha) {
                const double beta = (lane < p) ? W.xb[W.psi0 + lane] : 0.0;
                const double sb = wave_sum(beta);
                if (lane < p) alpha[o * (p + 1) + lane + 1] = beta;
                if (lane == 0) alpha[o * (p + 1)] = 1.0 - sb;
            }
            wsync();
        }
        pos = run_end;
    }
}

// ---- frontier sweep (single commutation): epsilon-suboptimality decision per node --------
// (lib/worker.py:368-375)
__global__ __launch_bounds__(EHM_K2_THREADS) void k2_lcss_decide(
    DevProblem P, DevTree T, const int32_t* __restrict__ frontier, int nf,
    int32_t* __restrict__ open_flag, DevCounters* cnt, int wave_doubles, int sign_only) {
    K2_PROLOGUE();
    const int nrec = rec_doubles(P.p, P.n_u);
    const int per = (nf + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per;
    const int hi = (lo + per < nf) ? lo + per : nf;
    if (lo >= hi) return;
    load_shared(P, 0, sm, tid, blockDim.x);
    if (tid == 0) s_ctr = lo;
    __syncthreads();
    for (;;) {
        const int f = pull(&s_ctr, lane0);
        if (f >= hi) break;
        const int lane = pin(lane0);
        const int id = frontier[f];
        const double* rec = T.rec + (size_t)id * T.rec_stride;
        for (int k = lane; k < nrec; k += 64) nb.rec[k] = rec[k];
        wsync();
        if (T.grad && sign_only) {
            // tangent-plane bound of t* (ehm_dev.h, cut_bound): negative => the leaf is closed,
            // exactly as a negative t* would close it, without solving the LP
            const double thr = -EHM_ROUTE_TOL * (1.0 + fabs(nb.rec[rec_off_vcost(P.p)]));
            const double bnd = cut_bound(nb.rec, T.grad + (size_t)id * (P.p + 1) * P.p, P.p,
                                         P.eps_a, P.eps_r, lane, nb.lp, thr);
            if (bnd < thr) {
                if (lane == 0) {
                    atomicAdd(&cnt->cert_closed, 1ULL);
                    T.tstar[id] = bnd;
                    open_flag[f] = 0;
                    T.flags[id] |= 1;
                    atomicMin(&cnt->min_margin_bits,
                              (unsigned long long)__double_as_longlong(-bnd));
                }
                wsync();
                continue;
            }
        }
        Wave W;
        IpmResult r;
        int its = 0;
        for (int attempt = 0; attempt < EHM2_ATTEMPTS; ++attempt) {
            double b[SLOTS];
            const int ln = pin(lane);
            assemble_simplex(S, W, nb, nb.rec, nb.rec + rec_off_vcost(P.p), SX_SLACK, P.eps_a,
                             P.eps_r, b, ln, P, 0);
            r = ipm_solve(S, W, b, ln, sign_only != 0,
                          step_fraction(attempt));
            its += r.iters;
            if (r.status == 0) break;
        }
        r.iters = its;
        count_solve(cnt, r, lane);
        if (lane == 0) {
            if (r.status != 0) {
                atomicAdd(&cnt->errors, 1ULL);
                T.flags[id] |= 8;
            }
            atomicAdd(&cnt->slack_solves, 1ULL);
            atomicAdd(&cnt->slack_iters, (unsigned long long)r.iters);
            const double t = -r.obj;
            const bool open = (t >= 0.0);
            T.tstar[id] = t;
            open_flag[f] = open ? 1 : 0;
            if (!open) T.flags[id] |= 1;
            atomicMin(&cnt->min_margin_bits, (unsigned long long)__double_as_longlong(r.margin));
            if (r.margin < EHM_ROUTE_TOL * (1.0 + fabs(nb.rec[rec_off_vcost(P.p)])))
                atomicAdd(&cnt->routed, 1ULL);
        }
        wsync();
    }
}

// ---- split every open node, solve P_theta_delta at the midpoint, write the children -------
// (lib/worker.py:403-414, 354-365)
__global__ __launch_bounds__(EHM_K2_THREADS) void k2_lcss_expand(
    DevProblem P, DevTree T, const int32_t* __restrict__ open_list, int n_open, int child_base,
    int32_t* __restrict__ next_frontier, DevCounters* cnt, int wave_doubles) {
    K2_PROLOGUE();
    const int p = P.p, n_u = P.n_u;
    const int nrec = rec_doubles(p, n_u);
    const int per = (n_open + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per;
    const int hi = (lo + per < n_open) ? lo + per : n_open;
    if (lo >= hi) return;
    load_shared(P, 0, sm, tid, blockDim.x);
    if (tid == 0) s_ctr = lo;
    __syncthreads();
    for (;;) {
        const int f = pull(&s_ctr, lane0);
        if (f >= hi) break;
        const int lane = pin(lane0);
        const int id = open_list[f];
        const double* rec = T.rec + (size_t)id * T.rec_stride;
        double* node = nb.rec;
        double* mid = nb.th;
        for (int k = lane; k < nrec; k += 64) node[k] = rec[k];
        wsync();
        int bi, bj;
        longest_edge_wave(node, p, lane, bi, bj);
        if (lane < p) {
#pragma clang fp contract(off)
            mid[lane] = (node[bi * p + lane] + node[bj * p + lane]) / 2.0;
        }
        wsync();
        const int d = T.didx[id];
        Wave W;
        IpmResult r;
        int its = 0;
        for (int attempt = 0; attempt < EHM2_ATTEMPTS; ++attempt) {
            double b[SLOTS];
            const int ln = pin(lane);
            assemble_point(S, W, nb.lp, mid, false, b, ln, P, 0);
            r = ipm_solve(S, W, b, ln, false, step_fraction(attempt), T.grad ? nb.F : nullptr);
            its += r.iters;
            if (r.status == 0) break;
        }
        r.iters = its;
#if EHM2_QUAD
        if (T.grad) quad_grad_add(W, P, 0, mid, nb.F, lane);
#endif
        count_solve(cnt, r, lane);
        if (r.status != 0 && lane == 0) {
            atomicAdd(&cnt->errors, 1ULL);
            T.flags[id] |= 16;
        }
        const int c0 = child_base + 2 * f;
        if (T.grad) {       // the children inherit the vertex gradients, the midpoint's is new
            const int ng = (p + 1) * p;
            const double* gp_ = T.grad + (size_t)id * ng;
            double* g0 = T.grad + (size_t)c0 * ng;
            for (int k = lane; k < ng; k += 64) {
                const double gv = gp_[k];
                g0[k] = (k >= bi * p && k < bi * p + p) ? nb.F[k - bi * p] : gv;
                g0[ng + k] = (k >= bj * p && k < bj * p + p) ? nb.F[k - bj * p] : gv;
            }
        }
        if (T.wit && lane < 2 * (p + 2))    // the sweeps do not hand witnesses on (DevTree::wit)
            T.wit[(size_t)c0 * (p + 2) + lane] = 0.0;
        double* rec0 = T.rec + (size_t)c0 * T.rec_stride;
        double* rec1 = rec0 + T.rec_stride;
        const int ov = rec_off_vcost(p), ou = rec_off_vinput(p);
        for (int k = lane; k < nrec; k += 64) {
            double v0 = node[k], v1 = node[k];
            // row bi / bj of each block is replaced (range tests instead of k / p)
            if (k < ov) {                       // vertices
                if (k >= bi * p && k < bi * p + p) v0 = mid[k - bi * p];
                if (k >= bj * p && k < bj * p + p) v1 = mid[k - bj * p];
            } else if (k < ou) {                // vertex costs
                if (k - ov == bi) v0 = r.obj;
                if (k - ov == bj) v1 = r.obj;
            } else {                            // vertex inputs
                const int q = k - ou;
                if (q >= bi * n_u && q < bi * n_u + n_u) v0 = W.xb[q - bi * n_u];
                if (q >= bj * n_u && q < bj * n_u + n_u) v1 = W.xb[q - bj * n_u];
            }
            rec0[k] = v0;
            rec1[k] = v1;
        }
        if (lane == 0) {
            T.left[id] = c0;
            const int dep = T.depth[id] + 1;
            T.left[c0] = -1;
            T.left[c0 + 1] = -1;
            T.didx[c0] = d;
            T.didx[c0 + 1] = d;
            T.depth[c0] = dep;
            T.depth[c0 + 1] = dep;
            T.flags[c0] = 2;
            T.flags[c0 + 1] = 2;
            T.tstar[c0] = 0.0;
            T.tstar[c0 + 1] = 0.0;
            next_frontier[2 * f] = c0;
            next_frontier[2 * f + 1] = c0 + 1;
        }
        wsync();
    }
}


// ---- persistent frontier kernel (ehm_persist.h), both solves at this instance's width -------
namespace kd = EHM2_NS;
namespace ke = EHM2_NS;
#define kx_persist k2_persist
#include "ehm_persist.h"

// ---- vertex solves that seed a node's costs / inputs (lib/oracle.py:416-443) ---------------
__global__ __launch_bounds__(EHM_K2_THREADS) void k2_vertex_solve(
    DevProblem P, DevTree T, const int32_t* __restrict__ nodes, int n_nodes, DevCounters* cnt,
    int wave_doubles) {
    K2_PROLOGUE();
    const int p = P.p, n_u = P.n_u;
    const int total = n_nodes * (p + 1);
    const int per = (total + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per;
    const int hi = (lo + per < total) ? lo + per : total;
    if (lo >= hi) return;
    load_shared(P, 0, sm, tid, blockDim.x);
    if (tid == 0) s_ctr = lo;
    __syncthreads();
    for (;;) {
        const int t = pull(&s_ctr, lane0);
        if (t >= hi) break;
        const int lane = pin(lane0);
        const int id = nodes[t / (p + 1)];
        const int v = t % (p + 1);
        double* rec = T.rec + (size_t)id * T.rec_stride;
        if (lane < p) nb.th[lane] = rec[v * p + lane];
        wsync();
        Wave W;
        IpmResult r;
        int its = 0;
        for (int attempt = 0; attempt < EHM2_ATTEMPTS; ++attempt) {
            double b[SLOTS];
            const int ln = pin(lane);
            assemble_point(S, W, nb.lp, nb.th, false, b, ln, P, 0);
            r = ipm_solve(S, W, b, ln, false, step_fraction(attempt), T.grad ? nb.F : nullptr);
            its += r.iters;
            if (r.status == 0) break;
        }
        r.iters = its;
        count_solve(cnt, r, lane);
        if (r.status != 0 && lane == 0) atomicAdd(&cnt->errors, 1ULL);
#if EHM2_QUAD
        if (T.grad) quad_grad_add(W, P, 0, nb.th, nb.F, lane);
#endif
        if (T.grad && lane < p) T.grad[((size_t)id * (p + 1) + v) * p + lane] = nb.F[lane];
        if (lane == 0) rec[rec_off_vcost(p) + v] = r.obj;
        if (lane < n_u) rec[rec_off_vinput(p) + v * n_u + lane] = W.xb[lane];
        wsync();
    }
}

// ---- self test of the wave primitives (ehm_selftest) --------------------------------------
__global__ __launch_bounds__(64) void k2_selftest(double* out) {
    const int lane = threadIdx.x;
    const double v = 1.0 + 0.5 * lane;                       // sum = 64 + 0.5*2016 = 1072
    out[0] = wave_sum(v);
    out[1] = wave_max((lane == 37) ? 99.0 : -(double)lane);
    out[2] = wave_sum((lane < 25) ? 1.0 : 0.0);
    out[3] = frcp(3.0);
    out[4] = wave_max(-1.0 - lane);
}

}  // namespace EHM2_NS

// ---------------------------------------------------------------------------------------
// host-side launchers (one set per compiled instance)
// ---------------------------------------------------------------------------------------
namespace {

using namespace EHM2_NS;

hipError_t set_lds(int bytes) {
    const void* ks[] = {(const void*)k2_point_batch<0>, (const void*)k2_point_batch<1>,
                        (const void*)k2_simplex_batch<SX_MIN>,
                        (const void*)k2_simplex_batch<SX_SLACK>,
                        (const void*)k2_simplex_batch<SX_FEAS>,
                        (const void*)k2_lcss_decide, (const void*)k2_lcss_expand,
                        (const void*)k2_vertex_solve, (const void*)k2_persist};
    for (const void* k : ks) {
        hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

size_t wave_doubles_for(const DevProblem& P, int n_lp, int ne, int persist) {
    // (+ k2_stash_doubles: what the midpoint-first flow of k2_persist parks per node behind the
    // wavefront's workspace; the batch and sweep kernels park nothing)
    return k2_node_doubles(P.p, P.n_u) + wave_lp_doubles(n_lp, ne, P.n - P.nd0, P.p) +
           ((EHM_PERSIST_MIDFIRST && persist) ? k2_stash_doubles(P.p, P.n_u) : 0);
}
size_t shared_doubles_for(const DevProblem& P) { return shared_doubles(P); }

void l_point(const K2Launch& L, DevProblem P, long long n_inst, const double* theta,
             const int32_t* seg, int feas, double* J, double* u0, int32_t* status,
             int32_t* iters, DevCounters* cnt, K2Gather G) {
    P.wc_lds = L.wc_lds;
    if (feas)
        hipLaunchKernelGGL(k2_point_batch<1>, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream,
                           P, n_inst, theta, seg, J, u0, status, iters, cnt, L.wave_doubles, G);
    else
        hipLaunchKernelGGL(k2_point_batch<0>, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream,
                           P, n_inst, theta, seg, J, u0, status, iters, cnt, L.wave_doubles, G);
}
void l_simplex(const K2Launch& L, DevProblem P, long long n_inst, const double* R,
               const double* Vbar, const int32_t* seg, int mode, double* obj, double* alpha,
               int32_t* status, int32_t* iters, DevCounters* cnt, K2Gather G) {
    P.wc_lds = L.wc_lds;
#define K2_SX_LAUNCH(M)                                                                      \
    hipLaunchKernelGGL(k2_simplex_batch<M>, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream, \
                       P, n_inst, R, Vbar, seg, obj, alpha, status, iters, cnt, L.wave_doubles, G)
    if (mode == SX_SLACK) K2_SX_LAUNCH(SX_SLACK);
    else if (mode == SX_FEAS) K2_SX_LAUNCH(SX_FEAS);
    else K2_SX_LAUNCH(SX_MIN);
#undef K2_SX_LAUNCH
}
void l_decide(const K2Launch& L, DevProblem P, DevTree T, const int32_t* frontier, int nf,
              int32_t* open_flag, DevCounters* cnt, int sign_only) {
    P.wc_lds = L.wc_lds;
    hipLaunchKernelGGL(k2_lcss_decide, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream, P,
                       T, frontier, nf, open_flag, cnt, L.wave_doubles, sign_only);
}
void l_expand(const K2Launch& L, DevProblem P, DevTree T, const int32_t* open_list, int n_open,
              int child_base, int32_t* next_frontier, DevCounters* cnt) {
    P.wc_lds = L.wc_lds;
    hipLaunchKernelGGL(k2_lcss_expand, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream, P,
                       T, open_list, n_open, child_base, next_frontier, cnt, L.wave_doubles);
}
void l_vertex(const K2Launch& L, DevProblem P, DevTree T, const int32_t* nodes, int n_nodes,
              DevCounters* cnt) {
    P.wc_lds = L.wc_lds;
    hipLaunchKernelGGL(k2_vertex_solve, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream, P,
                       T, nodes, n_nodes, cnt, L.wave_doubles);
}
void l_persist(const K2Launch& L, DevProblem P, DevTree T, int32_t* slots, int n_slots,
               PersistCtl* ctl, int node_cap, DevCounters* cnt, int sign_only, int max_depth,
               PersistDeal deal) {
    P.wc_lds = L.wc_lds;
    hipLaunchKernelGGL(k2_persist, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream, P, T,
                       slots, n_slots, ctl, node_cap, cnt, L.wave_doubles, sign_only, max_depth,
                       deal);
}
void l_selftest(hipStream_t stream, double* out) {
    hipLaunchKernelGGL(k2_selftest, dim3(1), dim3(64), 0, stream, out);
}

const K2Api g_api = {EHM_NP,   EHM_SLOTS,        EHM_K2_THREADS,     64,      set_lds,
                     wave_doubles_for, shared_doubles_for, l_point, l_simplex, l_decide,
                     l_expand, l_vertex,         l_selftest,     l_persist};

}  // namespace

#define K2_CAT2(a, b, c) a##b##_##c
#define K2_CAT(a, b, c) K2_CAT2(a, b, c)
#if EHM2_QUAD
extern "C" const ehm::K2Api* K2_CAT(ehm_k2q_api_, EHM_NP, EHM_SLOTS)() { return &g_api; }
#else
extern "C" const ehm::K2Api* K2_CAT(ehm_k2_api_, EHM_NP, EHM_SLOTS)() { return &g_api; }
#endif
