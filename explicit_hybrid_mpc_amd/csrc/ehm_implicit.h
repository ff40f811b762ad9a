// Interface between ehm_capi.hip (the solver handle) and ehm_implicit.hip (the closed loop around
// the implicit law): what the loop needs of an ehm_problem without seeing the struct.  Neither
// function is part of the library's surface (hidden visibility, not in include/ehmpc.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ehmpc.h"

// feasibility margin: the phase-one optimum is compared against a tolerance that is far
// above the solver accuracy (1e-10 relative) and far below any constraint scale
#define EHM_FEAS_TOL 1e-8
// optimal values of different commutations closer than this (relative to 1+|value|) are
// ties, broken by enumeration order (DESIGN.md "canonical commutation rule")
#define EHM_TIE_TOL 1e-6

extern "C" {

struct ImpProblem {
    int device, p, n_u, n_delta;
    hipStream_t stream;
};

// The dimensions, device and stream of a solver handle.  Fails (EHM_E_INVALID, message in
// ehm_last_error) unless the handle runs the generation-2 kernels.
int ehm_imp_describe(ehm_problem* P, ImpProblem* out);

// One launch of the batched point oracle (feas = 1: its phase-one form, tau out in J) on the
// handle's stream, through the instance k2_config picks for the LP kind: the launch
// ehm_solve_pt_batch makes, with every array on the device.  Instance i reads its parameter at
// base + src[i] and writes its results at index dst[i] (NULL: i); seg [n_delta + 1] are the
// commutation segments of the instance list; n_dev (NULL: max_items) the device-side instance
// count.  Full accuracy (no sign-only stop).  u0, status may be NULL.  Nothing is copied and
// nothing synchronised.
int ehm_imp_point(ehm_problem* P, int feas, long long max_items, const double* base,
                  const int32_t* seg, double* J, double* u0, int32_t* status,
                  const long long* src, const int32_t* dst, const int32_t* n_dev);

}  // extern "C"
