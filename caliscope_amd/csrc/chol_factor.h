// The launches of the blocked Cholesky on raw device pointers, for callers inside the library that factor a matrix of their own
// (cba_parameter_covariance, covariance_lib.hip).  Defined in cba_lib.hip, where the arguments are described; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace cba {

__attribute__((visibility("hidden"))) void enqueue_chol_factor(double* W, int n, int ldw, int* flags, long long* trace, double* Xinv, double* Tinv,
                                                               bool early, hipStream_t stream, bool without_last, bool pair);
// CBA_CHOL_EARLY=0 for callers without a handle, read per call
__attribute__((visibility("hidden"))) bool chol_early_from_env();

}  // namespace cba
