// stg_launch_plan.hpp -- which form a step launch takes (stg_step_many, stg_step_ids), decided on the host from the context's
// configuration and the launch's size alone.  Plain C++ with no HIP dependency: tests/test_launch_plan.py compiles it with the host
// compiler and pins every threshold below.  Results never depend on the plan -- only speed does -- so nothing else would notice a
// threshold that moved.
#pragma once
#include "../../include/spintorque_hip.h"

#include <cstdint>

constexpr int PLAN_DUR = 256;         // 20 ps of pulse duration per bucket at the default 5 ns maximum
constexpr int PLAN_BUCKETS = 3 * PLAN_DUR;   // x device kind (device-physics torque model: type-uniform wavefronts)
constexpr int PLAN_THREADS = 1024;
constexpr int PLAN_ITEMS = 4;
constexpr int TILE_ENVS = PLAN_THREADS * PLAN_ITEMS;   // 4096 envs sorted together (one plan workgroup)
constexpr int TILE_WAVES = TILE_ENVS / 64;             // = 64 wavefronts of the step launch

// largest launch the automatic wave specialisation applies to: one integrating wavefront per SIMD (256 CUs x 4 SIMDs x
// 64 lanes); beyond that the launch is throughput-bound and the rendezvous costs more than it gives
constexpr int64_t STG_WAVE_SPEC_MAX_ENVS = 65536;

// hybrid launch: fewest producer / consumer pairs it is taken with -- measured (profiles/r04_hybrid_range_ab.txt) ahead of the
// alternatives down to 512 pairs (RK45, 98 304 envs) / 640 pairs (RK4, 90 112 envs)
constexpr int64_t STG_HYBRID_MIN_PAIRS_RK45 = 512, STG_HYBRID_MIN_PAIRS_RK4 = 640;

// automatic lane refill of the RK45 step (stg_step_refill_kernel: persistent wavefronts sharing one global queue; measured on 81 921 ...
// 1 048 576 envs, profiles/r04_refill_global_ab.txt): 1024 wavefronts -- one per SIMD -- while that leaves at most 8 envs per lane (up
// to 524 288 envs), 2048 beyond.  From 131 073 envs at T = 0 K (up to there the one-env-per-lane launch with its two wavefronts per SIMD
// is as fast: 131 072 envs 1.96 against 1.94 ms, 98 304 envs 1.81 against 1.87) and from 98 305 envs with the thermal field (just
// above the hybrid wave-specialised launch: 98 304 envs hybrid 2.81 against 2.90 ms, 106 496 envs 3.08 against 2.93; up to 131 072 envs
// 3.1-3.2 -> 2.9-3.0 ms against one env per lane: there the launch is bound by its longest env at the inline-normal loop's
// lone-wavefront speed either way).  Attempts between refill points: 32 (16 with 2048 wavefronts).
constexpr int64_t STG_REFILL_AUTO_ENVS = 131073, STG_REFILL_AUTO_ENVS_THERMAL = 98305;
constexpr int32_t STG_REFILL_CHECK_DEFAULT = 32;
// (two wavefronts per SIMD: a refill point every 16 attempts -- 1 048 576 envs 13.3 against 13.6 ms; with one per SIMD 16 ... 64
// are alike, 8 and 128 worse)
constexpr int32_t STG_REFILL_CHECK_2048 = 16;
constexpr int64_t STG_REFILL_WAVES = 1024, STG_REFILL_WAVES_MANY = 2048, STG_REFILL_MAX_ENVS_PER_LANE = 8;

inline int64_t plan_blocks(int64_t n) { return ((n + TILE_ENVS - 1) / TILE_ENVS) * TILE_WAVES; }   // blocks of whole tiles (a ragged tile's empty blocks included)

inline void refill_auto(int64_t n, bool thermal, int& r, int64_t& nw) {
    r = 0; nw = 0;
    if (n < (thermal ? STG_REFILL_AUTO_ENVS_THERMAL : STG_REFILL_AUTO_ENVS)) return;
    const int64_t nblk = plan_blocks(n);
    nw = STG_REFILL_WAVES;
    int64_t rr = (nblk + nw - 1) / nw;
    if (rr > STG_REFILL_MAX_ENVS_PER_LANE) { nw = STG_REFILL_WAVES_MANY; rr = (nblk + nw - 1) / nw; }
    r = (int)(rr < 2 ? 2 : (rr > 0x7FFFFFFF ? 0x7FFFFFFF : rr));              // (envs per lane on average; only != 0 matters to the launch)
}

// stg_switch_stats (kernel: stg_switch.hpp; pinned by tests/test_switch_stats_plan_host.py).
// Launch rule: every lane runs one trial (L = 1) while that needs at most STG_SWITCH_STATS_WAVES wavefronts in all; beyond that the
// wavefronts per condition are capped at max(1, STG_SWITCH_STATS_WAVES / G) and each lane loops over L trials.
static inline void switch_stats_plan(int32_t G, int64_t R, int64_t* L, int32_t* waves_per_cond) {
    const int64_t w1 = (R + 63) / 64;                              // wavefronts per condition at one trial per lane
    int64_t cap = STG_SWITCH_STATS_WAVES / (int64_t)G;
    if (cap < 1) cap = 1;
    *L = w1 <= cap ? 1 : (w1 + cap - 1) / cap;
    *waves_per_cond = (int32_t)((w1 + *L - 1) / *L);
}

// stg_switch_verify (kernel: stg_switch_verify.hpp).  Launch rule: W = min(ceil(R / 64), max(1, cap / G)) wavefronts per condition, cap =
// max_waves if the caller gave one (> 0), else STG_SWITCH_STATS_WAVES; lane l of wavefront w runs trials w * 64 + l + k * 64 * W.
static inline int32_t switch_verify_plan(int32_t G, int64_t R, int32_t max_waves) {
    const int64_t w1 = (R + 63) / 64;
    int64_t cap = (max_waves > 0 ? (int64_t)max_waves : (int64_t)STG_SWITCH_STATS_WAVES) / (int64_t)G;
    if (cap < 1) cap = 1;
    return (int32_t)(w1 < cap ? w1 : cap);
}

struct StepPlan {
    bool sort;                // the plan kernel runs and the step launch follows its permutation (else: identity schedule)
    bool by_kind, regroup, skip_done;   // ... the plan kernel's arguments (read only with `sort`)
    bool thermal;             // THERMAL of the step kernel
    int multi;                // 0 one class, 1 class table, 2 per-env parameter records: every lane derives its constants from its env's record, in registers
    bool devphys, pc;         // device-physics torque model; wave-specialised (producer / consumer) kernel
    int32_t hybrid;           // StepArgs::hybrid: number of producer / consumer pairs + 1, 0 = not a hybrid launch
    int32_t refill, refill_check, refill_nw;   // StepArgs: refill != 0 selects the lane-refill launch
};

// n: the launch's slots -- the context's env count for the full step, the list length for an id launch (`ids`).  has_cls: the caller
// gave a class index per env.  Returns STG_OK, or an error code with *err set to its message.
inline int plan_step(const stg_config& cfg, int64_t n, int32_t K, bool autoreset, bool ids, bool per_env, int32_t ncls, bool has_cls,
                     StepPlan* out, const char** err) {
    StepPlan p{};
    // lane_sort: 0 = automatic (on: the single LDS-only plan kernel costs ~5 us and the sorted schedule is never slower
    // once there is more than one wavefront), 1 = always, -1 = never (identity schedule)
    p.sort = cfg.lane_sort >= 0 && n > 64;
    if (p.sort && n > 0xFFFFFFFFll) { *err = "lane sort supports up to 2^32 envs per context"; return STG_E_INVALID; }
    p.skip_done = cfg.skip_done && !autoreset;
    p.by_kind = cfg.torque_model == 1 && ((ncls > 1 && has_cls) || per_env);
    // device-physics model with a class table: kind-pure groups of four blocks (= whole workgroups of the step launch), dealt by the
    // estimated cost of their longest block (round 4, profiles/r04_devphys_order_ab.txt: 1.08-1.37x at 98 304 ... 1 048 576 envs;
    // 65 537 ... 98 303 envs not measured; there the rounds 2-3 grouping, keyed by a group's first env, lost to kind-major at 70 000
    // envs: 0.39 -> 0.60 ms).  Per-env parameter records keep the kind-major order, measured ahead when their launches were
    // one-wavefront workgroups (see stg_plan_tile_kernel) and not re-measured since they use 4-wavefront ones from 65 536 envs on.
    p.regroup = p.by_kind && !per_env;
    // the Simple solver only draws a thermal field when temperature > 0 (simple_solver.py:321,378); RK45 (LLGS) whenever cfg.thermal
    const bool rk45 = cfg.solver == STG_SOLVER_RK45;
    p.thermal = rk45 ? cfg.thermal != 0 : (cfg.thermal && cfg.temperature > 0);
    p.multi = per_env ? 2 : (ncls > 1 ? 1 : 0);
    p.devphys = cfg.torque_model == 1;
    // wave_spec: 0 = automatic (thermal launches of at most STG_WAVE_SPEC_MAX_ENVS envs, i.e. latency-bound ones),
    // 1 = always, -1 = never.  Results do not depend on it.  (The kernel exists for the thermal field without the device-physics model.)
    p.pc = p.thermal && !p.devphys && (cfg.wave_spec > 0 || (cfg.wave_spec == 0 && n <= STG_WAVE_SPEC_MAX_ENVS));
    // hybrid (RK45 / RK4 + thermal, sorted schedule, 65 536 < N <= 131 072, automatic mode): 1024 two-wavefront workgroups -- producer /
    // consumer pairs for the 2048 - nblk longest blocks, two blocks with inline normals in each of the others (stg_kernels.hpp:
    // stg_hybrid_block)
    if (!ids &&                                                        // (not measured for id launches)
        (rk45 || (cfg.solver == STG_SOLVER_RK4 && !p.devphys)) && p.thermal && cfg.wave_spec == 0 && p.sort && !per_env &&
        n > STG_WAVE_SPEC_MAX_ENVS) {
        // (a) up to 131 072 envs: pairs for the 2048 - nblk longest blocks, two fixed blocks in each other workgroup
        const int64_t n_pair = 2048 - plan_blocks(n);
        if (n <= 2 * STG_WAVE_SPEC_MAX_ENVS && n_pair >= (rk45 ? STG_HYBRID_MIN_PAIRS_RK45 : STG_HYBRID_MIN_PAIRS_RK4)) {
            p.pc = true; p.hybrid = (int32_t)n_pair + 1;
        }
    }
    // lane refill (RK45 throughput launches of one env-step, see stg_step_refill_kernel).  cfg.lane_refill: 0 = automatic, -1 never,
    // >= 2 forced.  Unlike the hybrid launch it does not need the sorted schedule.
    p.refill_check = STG_REFILL_CHECK_DEFAULT;
    if (rk45 && K == 1 && !per_env) {
        int r = 0, chk = STG_REFILL_CHECK_DEFAULT;
        int64_t nw = 0;
        if (cfg.lane_refill == 0) {
            refill_auto(n, p.thermal, r, nw);
            if (nw >= STG_REFILL_WAVES_MANY) chk = STG_REFILL_CHECK_2048;
        }
        else if (cfg.lane_refill > 0) { r = cfg.lane_refill; nw = (plan_blocks(n) + r - 1) / r; }
        // (not combined with the wave-specialised launch: a forced wave_spec = 1 keeps the one-env-per-lane kernel)
        if (r >= 2 && nw >= 1 && !(p.thermal && cfg.wave_spec > 0)) {
            if (nw > 0x7FFFFFFFll) { *err = "lane refill: too many wavefronts"; return STG_E_INVALID; }
            p.refill = r; p.refill_check = chk; p.refill_nw = (int32_t)nw;
        }
    }
    *out = p;
    return STG_OK;
}
