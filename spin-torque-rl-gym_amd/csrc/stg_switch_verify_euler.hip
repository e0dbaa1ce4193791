// stg_switch_verify_euler.hip -- instantiations of the write-verify-write kernels for STG_SOLVER_EULER (see stg_switch_verify.hpp)
#include "stg_switch_verify.hpp"

void stg_dispatch_switch_verify_euler(const SwitchVerifyArgs& x, bool thermal, bool multi, hipStream_t st) {
    dispatch_switch_verify<STG_SOLVER_EULER>(x, thermal, multi, st);
}

void stg_dispatch_switch_verify_population_euler(const SwitchVerifyPopArgs& x, bool thermal, hipStream_t st) {
    dispatch_switch_verify_population<STG_SOLVER_EULER>(x, thermal, st);
}
