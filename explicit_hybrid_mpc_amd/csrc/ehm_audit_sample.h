// The launch of k_audit_sample (ehm_audit.hip owns the kernel) for the other source that draws
// points with it, ehm_applied.hip: one statement of the sampler, so the two audits draw the same
// point for the same (seed, id, cells).  Not exported.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// n samples with the global ids first .. first + n - 1 on `stream`: X [n][p], cell [n] (device).
// mode EHM_AUDIT_UNIFORM reads cdf [n_cells], EHM_AUDIT_PER_LEAF reads kper; V [n_cells][p+1][p].
void ehm_audit_launch_sample(hipStream_t stream, long long n, uint64_t first, int mode, int kper,
                             uint64_t seed, int p, long long n_cells, const double* cdf,
                             const double* V, double* X, int32_t* cell);
