// stg_switch_times.hpp -- argument block, first-passage observer and launch entry of stg_switch_times (kernels: stg_switch_times.hip;
// C-ABI: spintorque_hip.hip).
#pragma once
#include "stg_switch_stats_wave.hpp"

struct SwitchTimesArgs {
    SwitchStatsWaveArgs w;        // as stg_switch_stats_wave; w.wave_phase is the WATCHED phase, and kj = kh = 0 (rectangular) is valid
    int32_t n_tbins;              // 0 ... STG_MAX_TBINS
    unsigned long long *n_crossed, *n_returned, *t_hist;   // [G], [G], [G][n_tbins] (nullptr iff n_tbins == 0): added to
};

// The per-point observer of the watched phase (the REC parameter of the solvers, stg_physics.hpp: Recorder): the first passage of
// m . target over `threshold`, kept in three values per lane (crossed, t_x, t_prev: two fp64 register pairs and one bit of a wave mask).
// It stores nothing and wants no energy and no torque norm.
//   proj_k = ((m_k.x * tx) + (m_k.y * ty)) + (m_k.z * tz) without contraction, as the classification of stg_switch_stats forms it;
//   the trial crosses at the first row k with proj_k > threshold (a NaN never does);
//   t_x = 0.5 * (t_{k-1} + t_k), each operation rounded; row 0 has t_0 = 0 and t_prev starts at 0, so its t_x is 0.0.
struct FirstPassage {
    static constexpr bool kByProducts = false;
    static constexpr double* e = nullptr;
    static constexpr double* tq = nullptr;
    V3 tg;
    double threshold;
    mutable double t_prev, t_x;
    mutable bool crossed;
    __device__ __forceinline__ void put(int32_t, double tt, const V3& mm, double, double = 0.0) const {
        const double proj = add_x(add_x(mul_x(mm.x, tg.x), mul_x(mm.y, tg.y)), mul_x(mm.z, tg.z));
        const bool hit = !crossed && proj > threshold;
        t_x = hit ? mul_x(0.5, add_x(t_prev, tt)) : t_x;
        crossed = crossed || hit;
        t_prev = tt;
    }
};

void stg_switch_times_launch(const SwitchTimesArgs& a, int solver, bool thermal, bool multi, hipStream_t st);
