// stg_switch_stats.hpp -- argument block and launch entry of stg_switch_stats (kernels: stg_switch_stats.hip; C-ABI: spintorque_hip.hip).
#pragma once
#include "stg_kernels.hpp"

struct SwitchStatsArgs {
    CfgView c;
    int64_t env_id0;
    int64_t R, trial0, trial_stride;   // trials trial0 ... trial0 + R - 1 of every condition; trial r of condition g is problem g * trial_stride + r
    int64_t L;                         // trials per lane
    int32_t waves_per_cond;            // wavefronts (= workgroups) per condition: ceil(R / (64 L)); the grid is G * waves_per_cond
    int32_t G, P, n_bins, ncls;
    const double* ctab;
    const uint8_t* cond_cls;           // [G] or nullptr: class 0
    const double *m0, *J, *T, *target; // [3][G], [P][G], [P][G], [3][G]
    double threshold;
    uint32_t env_step;
    unsigned long long *n_switched, *n_failed, *hist;   // [G], [G], [G][n_bins] (nullptr iff n_bins == 0): added to
};

// (the launch rule, switch_stats_plan, is host-only C++: stg_launch_plan.hpp, pinned by tests/test_switch_stats_plan_host.py)

void stg_switch_stats_launch(const SwitchStatsArgs& a, int solver, bool thermal, bool multi, hipStream_t st);
