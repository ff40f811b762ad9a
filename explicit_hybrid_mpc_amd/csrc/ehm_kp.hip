// Persistent frontier kernel at two solver widths (gfx950).  The kernel's body is ehm_persist.h,
// the one ehm_k2.hip compiles as k2_persist (see there and DESIGN.md section 4 for the queue
// protocol); here the suboptimality-test LPs (n + p + 1 columns) and the midpoint LPs (n columns)
// each run in the instance of ehm_ipm2.h that fits them: a row of the normal matrix lives in
// registers, so the column capacity is a compile-time size and every elimination step costs
// that many FMAs per lane.
// Compiled per (EHM_NPD, EHM_NPE, EHM_SLOTS); ehm_capi.hip uses it when a matching pair exists.
#include <hip/hip_runtime.h>

#ifndef EHM_NPD
#error "EHM_NPD / EHM_NPE (column capacities of the two LP kinds) must be defined"
#endif

#define EHM_NP EHM_NPD
#include "ehm_k2_asm.h"
namespace kd = EHM2_NS;     // "decide": the suboptimality-test LP
#undef EHM_NP
#define EHM_NP EHM_NPE
#include "ehm_k2_asm.h"
namespace ke = EHM2_NS;     // "expand": the midpoint LP
#undef EHM_NP

using namespace ehm;

// one named namespace per instance (kernels of different objects must not share a symbol)
#define KP_CAT2(a, b, c, d) a##b##_##c##_##d
#define KP_CAT(a, b, c, d) KP_CAT2(a, b, c, d)
#ifndef EHM_PERSIST_MIDFIRST
#define EHM_PERSIST_MIDFIRST 0
#endif
#if EHM2_QUAD
#define KP_NS KP_CAT(ehm_kpq_, EHM_NPD, EHM_NPE, EHM_SLOTS)
#elif EHM_PERSIST_MIDFIRST
#define KP_NS KP_CAT(ehm_kpm_, EHM_NPD, EHM_NPE, EHM_SLOTS)
#else
#define KP_NS KP_CAT(ehm_kp_, EHM_NPD, EHM_NPE, EHM_SLOTS)
#endif

namespace KP_NS {

#define kx_persist kp_persist
#include "ehm_persist.h"

hipError_t set_lds(int bytes) {
    return hipFuncSetAttribute((const void*)kp_persist,
                               hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
size_t wave_doubles_for(const DevProblem& P, int n_lp_d, int ne_d, int n_lp_e) {
    const int nE = P.n - P.nd0;
    const size_t a = kd::wave_lp_doubles(n_lp_d, ne_d, nE, P.p), b = ke::wave_lp_doubles(n_lp_e, 0, nE, P.p);
    // (+ k2_stash_doubles: the midpoint-first flow parks the midpoint solve's input and gradient and the
    // node's witness there)
    return k2_node_doubles(P.p, P.n_u) + (a > b ? a : b) + (EHM_PERSIST_MIDFIRST ? k2_stash_doubles(P.p, P.n_u) : 0);
}
size_t shared_doubles_for(const DevProblem& P) { return kd::shared_doubles(P); }
void l_persist(const K2Launch& L, DevProblem P, DevTree T, int32_t* slots, int n_slots,
               PersistCtl* ctl, int node_cap, DevCounters* cnt, int sign_only, int max_depth,
               PersistDeal deal) {
    P.wc_lds = L.wc_lds;
    hipLaunchKernelGGL(kp_persist, dim3(L.grid), dim3(L.threads), L.lds_bytes, L.stream, P, T,
                       slots, n_slots, ctl, node_cap, cnt, L.wave_doubles, sign_only, max_depth,
                       deal);
}

const KpApi g_api = {EHM_NPD, EHM_NPE, EHM_SLOTS, EHM_K2_THREADS, set_lds, wave_doubles_for,
                     shared_doubles_for, l_persist};

}  // namespace KP_NS

#if EHM2_QUAD
extern "C" const ehm::KpApi* KP_CAT(ehm_kpq_api_, EHM_NPD, EHM_NPE, EHM_SLOTS)() {
    return &KP_NS::g_api;
}
#elif EHM_PERSIST_MIDFIRST
extern "C" const ehm::KpApi* KP_CAT(ehm_kpm_api_, EHM_NPD, EHM_NPE, EHM_SLOTS)() {
    return &KP_NS::g_api;
}
#else
extern "C" const ehm::KpApi* KP_CAT(ehm_kp_api_, EHM_NPD, EHM_NPE, EHM_SLOTS)() {
    return &KP_NS::g_api;
}
#endif
