// stg_step_rk45.hip -- instantiations of the env-step kernel for STG_SOLVER_RK45 (see stg_kernels.hpp)
#include "stg_kernels.hpp"

void stg_dispatch_step_rk45(const StepArgs& a, bool thermal, int multi, bool axis_z, int act_f64, bool pc, hipStream_t st) {
    if (a.ids) dispatch_step<STG_SOLVER_RK45, true>(a, thermal, multi, axis_z, false, act_f64, pc, st);      // stg_step_ids
    else dispatch_step<STG_SOLVER_RK45, false>(a, thermal, multi, axis_z, false, act_f64, pc, st);
}

void stg_dispatch_step_rk45_refill(const StepArgs& a, bool thermal, bool multi, bool axis_z, int act_f64, hipStream_t st) {
    if (a.ids) dispatch_refill<true>(a, thermal, multi, axis_z, act_f64, st);
    else dispatch_refill<false>(a, thermal, multi, axis_z, act_f64, st);
}
