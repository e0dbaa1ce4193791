// stg_switch_euler.hip -- instantiations of the switching trial kernel for STG_SOLVER_EULER (see stg_switch.hpp)
#include "stg_switch.hpp"

void stg_dispatch_switch_euler(const SwitchTimesArgs& x, bool times, bool thermal, bool multi, hipStream_t st) {
    dispatch_switch<STG_SOLVER_EULER>(x, times, thermal, multi, st);
}

void stg_dispatch_switch_vary_euler(const SwitchPopArgs& x, bool times, bool thermal, hipStream_t st) {
    dispatch_switch_vary<STG_SOLVER_EULER>(x, times, thermal, st);
}
