// stg_switch_verify_rk4.hip -- instantiations of the write-verify-write kernels for STG_SOLVER_RK4 (see stg_switch_verify.hpp)
#include "stg_switch_verify.hpp"

void stg_dispatch_switch_verify_rk4(const SwitchVerifyArgs& x, bool thermal, bool multi, hipStream_t st) {
    dispatch_switch_verify<STG_SOLVER_RK4>(x, thermal, multi, st);
}

void stg_dispatch_switch_verify_population_rk4(const SwitchVerifyPopArgs& x, bool thermal, hipStream_t st) {
    dispatch_switch_verify_population<STG_SOLVER_RK4>(x, thermal, st);
}
