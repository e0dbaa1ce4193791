// stg_switch_rk4.hip -- instantiations of the switching trial kernel for STG_SOLVER_RK4 (see stg_switch.hpp)
#include "stg_switch.hpp"

void stg_dispatch_switch_rk4(const SwitchTimesArgs& x, bool times, bool thermal, bool multi, hipStream_t st) {
    dispatch_switch<STG_SOLVER_RK4>(x, times, thermal, multi, st);
}

void stg_dispatch_switch_vary_rk4(const SwitchPopArgs& x, bool times, bool thermal, hipStream_t st) {
    dispatch_switch_vary<STG_SOLVER_RK4>(x, times, thermal, st);
}
