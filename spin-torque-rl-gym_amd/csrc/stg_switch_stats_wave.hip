// stg_switch_stats_wave.hip -- the kernels of stg_switch_stats_wave: stg_switch_stats (stg_switch_stats.hip) with ONE phase of the trial
// driven by the condition's piecewise-linear current and field tables, (rk4 | euler | rk45) x thermal x class table, fp64.  A
// translation unit of its own: no other kernel is compiled with it.
//
// The shape is stg_switch_stats_kernel's: one 64-lane wavefront per workgroup on ONE condition g, L trials per lane, counts in
// registers (ballot + popcount), the histogram in LDS, one 64-bit atomic per count and per bin at the end.  Phase `wave_phase` of a
// trial is exactly the solve of stg_solve_wave_kernel (simple_solve_wave / llgs_solve_wave of stg_wave.hpp with InlineNormals on the
// stream of problem g * trial_stride + trial at env_step + wave_phase); every other phase is run_solver, as in stg_switch_stats_kernel.
// The condition's tables are wave-uniform: the wavefront stages its column of them into LDS once and every trial opens its cursors
// there (SharedKnots, unscaled: the same doubles GlobalKnots hands Pwl for a replicated table, so Pwl's arithmetic gives the same bits).
#include "stg_switch_stats_wave.hpp"
#include "stg_wave.hpp"

// the condition's tables in LDS: tj, jk, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
constexpr int KN_TJ = 0, KN_JK = STG_MAX_KNOTS, KN_TH = 2 * STG_MAX_KNOTS, KN_HK = 3 * STG_MAX_KNOTS;
static_assert(KN_HK + 3 * STG_MAX_KNOTS == STG_SHAPE_DOUBLES, "layout of the staged tables");
static_assert(STG_MAX_KNOTS <= 64, "lane j stages knot j");

using StatsJ = Pwl<1, SharedKnots<1, false>>;
using StatsH = Pwl<3, SharedKnots<3, false>>;
using StatsSource = WaveSourceT<StatsJ, StatsH>;

template <int SOLVER, bool THERMAL, bool MULTI>
__global__ void __launch_bounds__(64) stg_switch_stats_wave_kernel(const SwitchStatsWaveArgs w) {
    static_assert(STG_MAX_BINS == 64, "lane b owns bin b");
    __shared__ unsigned long long s_hist[STG_MAX_BINS];
    __shared__ double s_knots[STG_SHAPE_DOUBLES];
    const SwitchStatsArgs& a = w.s;
    const int lane = (int)threadIdx.x;
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)a.waves_per_cond);
    const int64_t wv = (int64_t)(blockIdx.x % (uint32_t)a.waves_per_cond);
    const int32_t G = a.G;
    s_hist[lane] = 0ull;
    // 0. condition g's column of the tables -> LDS (lane j: knot j; the knots behind a table's last one are never read)
    if (lane < STG_MAX_KNOTS) {
        const bool in_j = lane < w.kj, in_h = lane < w.kh;
        s_knots[KN_TJ + lane] = in_j ? w.tj[(int64_t)lane * G + g] : 0.0;
        s_knots[KN_JK + lane] = in_j ? w.jk[(int64_t)lane * G + g] : 0.0;
        s_knots[KN_TH + lane] = in_h ? w.th[(int64_t)lane * G + g] : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_knots[KN_HK + lane * 3 + c] = in_h ? w.hk[((int64_t)lane * 3 + c) * G + g] : 0.0;
    }
    __syncthreads();
    const double* row = a.ctab;
    if (MULTI) {
        const int c = a.cond_cls ? (int)a.cond_cls[g] : 0;
        row = a.ctab + (c < a.ncls ? c : 0) * C_COUNT;
    }
    const V3 m0{a.m0[g], a.m0[G + g], a.m0[2 * G + g]};
    const V3 tg{a.target[g], a.target[G + g], a.target[2 * G + g]};
    const Recorder norec{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    const int64_t id0 = a.env_id0 + (int64_t)g * a.trial_stride + a.trial0;       // env id of the condition's trial trial0
    const double bin_scale = mul_x(0.5, (double)a.n_bins);
    const bool has_j = w.kj > 0, has_h = w.kh > 0;                                 // (kernel-uniform; at least one of them: the entry checks)
    StatsSource src;
    src.has_j = has_j; src.has_h = has_h;
    src.cj.tk = s_knots + KN_TJ; src.cj.vk = s_knots + KN_JK; src.cj.st = 1.0; src.cj.sv = 1.0; src.cj.K = w.kj; src.cj.k = 0;
    src.ch.tk = s_knots + KN_TH; src.ch.vk = s_knots + KN_HK; src.ch.st = 1.0; src.ch.sv = 1.0; src.ch.K = w.kh; src.ch.k = 0;
    // a table that is not finite or not strictly increasing fails the wave phase of every trial of this condition (wave-uniform)
    const bool tables_ok = (!has_j || src.cj.valid()) && (!has_h || src.ch.valid());
    unsigned long long n_sw = 0ull, n_fail = 0ull;                                 // wave-uniform
    for (int64_t l = 0; l < a.L; ++l) {
        const int64_t r = (wv * a.L + l) * 64 + lane;                              // this lane's trial, counted from trial0
        const bool active = r < a.R;
        V3 m = m0;
        bool failed = false;
        if (active) {
            InlineNormals ns;
#pragma clang loop unroll(disable)
            for (int32_t p = 0; p < a.P && !failed; ++p) {
                const double Tp = a.T[(int64_t)p * G + g];
                if (Tp == 0.0) continue;
                const bool is_wave = p == w.wave_phase;
                const double Jp = (is_wave && has_j) ? 0.0 : a.J[(int64_t)p * G + g];
                const RngKey rk{a.c.seed, (uint64_t)(id0 + r), a.env_step + (uint32_t)p};
                SolveOut so{m, 0, 0, 0, false};
                if (!is_wave) {
                    so = run_solver<SOLVER, THERMAL, false, false, false>(m, Jp, Tp, row, a.c, rk, norec, ns, true);
                } else if (tables_ok) {
                    // the drive of this trial: the cursors opened anew at the wave phase's t = 0
                    src.J = Jp;
                    src.T = Tp;
                    if (has_j) src.cj.open();
                    if (has_h) src.ch.open();
                    src.arm();
                    if (SOLVER == STG_SOLVER_RK45) {
                        const LlgsK k = load_llgs(row);
                        const double beta = row[C_BETA], betap = row[C_BETAP];
                        const bool useJ = !(fabs(src.J) < 1e-12);                           // llgs_solver.py:222
                        const LlgsWaveK wk{beta, betap, -row[C_GAMMA], useJ ? beta * src.J : 0.0, useJ ? betap * src.J : 0.0,
                                           (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
                        so = llgs_solve_wave<THERMAL, false>(m, Tp, k, a.c.rtol, a.c.atol, a.c.max_step, a.c.max_attempts, rk, norec, LlgsEnergyK{},
                                                             ns, src, wk);
                    } else {
                        const SimpleK k = load_simple(row);
                        so = simple_solve_wave<SOLVER == STG_SOLVER_EULER ? 1 : 0, THERMAL, false>(
                            m, Tp, k, -row[C_GEFF], row[C_POL], row[C_MSV], row[C_VALID] != 0.0, a.c.temperature, a.c.max_step, rk, norec, ns,
                            a.c.inv_tau, src);
                    }
                }
                m = so.m;
                failed = !so.ok;
            }
        }
        const double proj = add_x(add_x(mul_x(m.x, tg.x), mul_x(m.y, tg.y)), mul_x(m.z, tg.z));
        n_sw += (unsigned long long)__popcll(__ballot(active && proj > a.threshold));
        n_fail += (unsigned long long)__popcll(__ballot(active && failed));
        if (active && a.n_bins > 0) {
            // min(n_bins - 1, max(0, (int)floor(x))), clamped before the conversion: NaN -> bin 0, +-inf and huge values -> the outer bins
            const double b = floor(mul_x(add_x(proj, 1.0), bin_scale));
            const int bin = b >= 1.0 ? (b < (double)(a.n_bins - 1) ? (int)b : a.n_bins - 1) : 0;
            atomicAdd(&s_hist[bin], 1ull);
        }
    }
    __syncthreads();
    if (lane == 0) {
        if (n_sw) atomicAdd(a.n_switched + g, n_sw);
        if (n_fail) atomicAdd(a.n_failed + g, n_fail);
    }
    if (lane < a.n_bins) {
        const unsigned long long v = s_hist[lane];
        if (v) atomicAdd(a.hist + (int64_t)g * a.n_bins + lane, v);
    }
}

template <int SOLVER>
static void dispatch_switch_stats_wave(const SwitchStatsWaveArgs& a, bool thermal, bool multi, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)a.s.G * a.s.waves_per_cond));
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) {
        hipLaunchKernelGGL((stg_switch_stats_wave_kernel<SOLVER, THERMAL.value, MULTI.value>), grid, dim3(64), 0, st, a);
    }); });
}

void stg_switch_stats_wave_launch(const SwitchStatsWaveArgs& a, int solver, bool thermal, bool multi, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_switch_stats_wave<STG_SOLVER_RK4>(a, thermal, multi, st); break;
        case STG_SOLVER_EULER: dispatch_switch_stats_wave<STG_SOLVER_EULER>(a, thermal, multi, st); break;
        default: dispatch_switch_stats_wave<STG_SOLVER_RK45>(a, thermal, multi, st); break;
    }
}
