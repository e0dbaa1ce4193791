// stg_switch_stats_wave.hpp -- argument block and launch entry of stg_switch_stats_wave (kernels: stg_switch_stats_wave.hip; C-ABI:
// spintorque_hip.hip).
#pragma once
#include "stg_switch_stats.hpp"

struct SwitchStatsWaveArgs {
    SwitchStatsArgs s;            // as stg_switch_stats; J[wave_phase][g] is read only without a current table
    int32_t wave_phase;           // the phase the tables drive (0 ... P - 1); the others are rectangular
    int32_t kj, kh;               // knot counts; 0: rectangular J while t <= T / zero field (not both 0)
    const double *tj, *jk;        // [kj][G], [kj][G]
    const double *th, *hk;        // [kh][G], [kh][3][G]
};

void stg_switch_stats_wave_launch(const SwitchStatsWaveArgs& a, int solver, bool thermal, bool multi, hipStream_t st);
