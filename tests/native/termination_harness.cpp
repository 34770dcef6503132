// trf::termination and trf::reduction_ratio of csrc/trf_math.h behind a C ABI (tests/test_termination_rule.py): the copy the host driver
// (csrc/cba_solve.cpp) and the packet workgroup of the fused iteration (csrc/cba_kernels.h) both run.
#include "../../caliscope_amd/csrc/trf_math.h"

extern "C" {
int th_termination(double dF, double F, double dx_norm, double x_norm, double ratio, double ftol, double xtol) {
  return trf::termination(dF, F, dx_norm, x_norm, ratio, ftol, xtol);
}
double th_reduction_ratio(double actual, double predicted) { return trf::reduction_ratio(actual, predicted); }
int th_none(void) { return trf::TERMINATION_NONE; }
}
