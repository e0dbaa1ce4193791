// stg_switch_times.hip -- the kernels of stg_switch_times: stg_switch_stats / stg_switch_stats_wave with the first passage of
// m . target over the threshold reduced for ONE phase of the trial, the watched phase, (rk4 | euler | rk45) x thermal x class table x
// (rectangular | tabled) watched phase, fp64.  A translation unit of its own: no other kernel is compiled with it.
//
// The shape is stg_switch_stats_kernel's: one 64-lane wavefront per workgroup on ONE condition g, L trials per lane, scalar counts in
// registers (ballot + popcount), both histograms in LDS with integer atomics, one 64-bit atomic per count and per bin at the end
// (lane b flushes bin b of hist and bins b, b + 64, ... of t_hist).  The time histogram's LDS is sized by the launch: 8 n_tbins bytes.
// The watched phase is the solve every other entry runs -- run_solver, or with tables (WAVE) simple_solve_wave / llgs_solve_wave on the
// condition's tables staged in LDS as in stg_switch_stats_wave_kernel -- with RECORD set and FirstPassage as its observer: the rows it
// sees are the rows stg_solve_traj / stg_solve_wave record.  Every other phase runs as in stg_switch_stats_kernel.
#include "stg_switch_times.hpp"
#include "stg_wave.hpp"

constexpr int KN_TJ = 0, KN_JK = STG_MAX_KNOTS, KN_TH = 2 * STG_MAX_KNOTS, KN_HK = 3 * STG_MAX_KNOTS;
static_assert(KN_HK + 3 * STG_MAX_KNOTS == STG_SHAPE_DOUBLES, "layout of the staged tables");
static_assert(STG_MAX_KNOTS <= 64, "lane j stages knot j");

using TimesJ = Pwl<1, SharedKnots<1, false>>;
using TimesH = Pwl<3, SharedKnots<3, false>>;
using TimesSource = WaveSourceT<TimesJ, TimesH>;

template <int SOLVER, bool THERMAL, bool MULTI, bool WAVE>
__global__ void __launch_bounds__(64) stg_switch_times_kernel(const SwitchTimesArgs x) {
    static_assert(STG_MAX_BINS == 64, "lane b owns bin b");
    __shared__ unsigned long long s_hist[STG_MAX_BINS];
    __shared__ double s_knots[WAVE ? STG_SHAPE_DOUBLES : 1];
    extern __shared__ unsigned long long s_thist[];                                // [n_tbins]
    const SwitchStatsWaveArgs& w = x.w;
    const SwitchStatsArgs& a = w.s;
    const int lane = (int)threadIdx.x;
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)a.waves_per_cond);
    const int64_t wv = (int64_t)(blockIdx.x % (uint32_t)a.waves_per_cond);
    const int32_t G = a.G;
    const int32_t n_tbins = x.n_tbins;
    s_hist[lane] = 0ull;
    for (int32_t b = lane; b < n_tbins; b += 64) s_thist[b] = 0ull;
    if (WAVE) {
        // condition g's column of the tables -> LDS (lane j: knot j; the knots behind a table's last one are never read)
        if (lane < STG_MAX_KNOTS) {
            const bool in_j = lane < w.kj, in_h = lane < w.kh;
            s_knots[KN_TJ + lane] = in_j ? w.tj[(int64_t)lane * G + g] : 0.0;
            s_knots[KN_JK + lane] = in_j ? w.jk[(int64_t)lane * G + g] : 0.0;
            s_knots[KN_TH + lane] = in_h ? w.th[(int64_t)lane * G + g] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) s_knots[KN_HK + lane * 3 + c] = in_h ? w.hk[((int64_t)lane * 3 + c) * G + g] : 0.0;
        }
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
    // n_tbins equal bins over the watched phase's [0, T] (a skipped watched phase, T == 0, bins nothing)
    const double tbin_scale = (double)n_tbins / a.T[(int64_t)w.wave_phase * G + g];
    const bool has_j = WAVE && w.kj > 0, has_h = WAVE && w.kh > 0;                 // (kernel-uniform; WAVE: at least one of them)
    TimesSource src;
    bool tables_ok = true;
    if (WAVE) {
        src.has_j = has_j; src.has_h = has_h;
        src.cj.tk = s_knots + KN_TJ; src.cj.vk = s_knots + KN_JK; src.cj.st = 1.0; src.cj.sv = 1.0; src.cj.K = w.kj; src.cj.k = 0;
        src.ch.tk = s_knots + KN_TH; src.ch.vk = s_knots + KN_HK; src.ch.st = 1.0; src.ch.sv = 1.0; src.ch.K = w.kh; src.ch.k = 0;
        // a table that is not finite or not strictly increasing fails the watched phase of every trial of this condition (wave-uniform)
        tables_ok = (!has_j || src.cj.valid()) && (!has_h || src.ch.valid());
    }
    unsigned long long n_sw = 0ull, n_fail = 0ull, n_cr = 0ull, n_ret = 0ull;      // wave-uniform
    for (int64_t l = 0; l < a.L; ++l) {
        const int64_t r = (wv * a.L + l) * 64 + lane;                              // this lane's trial, counted from trial0
        const bool active = r < a.R;
        V3 m = m0;
        bool failed = false;
        FirstPassage fp{tg, a.threshold, 0.0, 0.0, false};
        if (active) {
            InlineNormals ns;
#pragma clang loop unroll(disable)
            for (int32_t p = 0; p < a.P && !failed; ++p) {
                const double Tp = a.T[(int64_t)p * G + g];
                if (Tp == 0.0) continue;
                const bool watched = p == w.wave_phase;
                const double Jp = (watched && has_j) ? 0.0 : a.J[(int64_t)p * G + g];
                const RngKey rk{a.c.seed, (uint64_t)(id0 + r), a.env_step + (uint32_t)p};
                SolveOut so{m, 0, 0, 0, false};
                if (!watched) {
                    so = run_solver<SOLVER, THERMAL, false, false, false>(m, Jp, Tp, row, a.c, rk, norec, ns, true);
                } else {
                    if (!WAVE) {
                        so = run_solver<SOLVER, THERMAL, true, false, false>(m, Jp, Tp, row, a.c, rk, fp, ns, true);
                    } else if (tables_ok) {
                        // the drive of this trial: the cursors opened anew at the watched phase's t = 0
                        src.J = Jp;
                        src.T = Tp;
                        if (has_j) src.cj.open();
                        if (has_h) src.ch.open();
                        src.arm();
                        if (SOLVER == STG_SOLVER_RK45) {
                            const LlgsK k = load_llgs(row);
                            const double beta = row[C_BETA], betap = row[C_BETAP];
                            const bool useJ = !(fabs(src.J) < 1e-12);                       // llgs_solver.py:222
                            const LlgsWaveK wk{beta, betap, -row[C_GAMMA], useJ ? beta * src.J : 0.0, useJ ? betap * src.J : 0.0,
                                               (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
                            so = llgs_solve_wave<THERMAL, true>(m, Tp, k, a.c.rtol, a.c.atol, a.c.max_step, a.c.max_attempts, rk, fp, LlgsEnergyK{},
                                                                ns, src, wk);
                        } else {
                            const SimpleK k = load_simple(row);
                            so = simple_solve_wave<SOLVER == STG_SOLVER_EULER ? 1 : 0, THERMAL, true>(
                                m, Tp, k, -row[C_GEFF], row[C_POL], row[C_MSV], row[C_VALID] != 0.0, a.c.temperature, a.c.max_step, rk, fp, ns,
                                a.c.inv_tau, src);
                        }
                    }
                    // a watched phase that failed, by any cause, has not crossed: the rows it passed are discarded
                    fp.crossed = fp.crossed && so.ok;
                }
                m = so.m;
                failed = !so.ok;
            }
        }
        const double proj = add_x(add_x(mul_x(m.x, tg.x), mul_x(m.y, tg.y)), mul_x(m.z, tg.z));
        const bool switched = active && proj > a.threshold;
        const bool crossed = active && fp.crossed;
        n_sw += (unsigned long long)__popcll(__ballot(switched));
        n_fail += (unsigned long long)__popcll(__ballot(active && failed));
        n_cr += (unsigned long long)__popcll(__ballot(crossed));
        n_ret += (unsigned long long)__popcll(__ballot(crossed && !switched));
        if (active && a.n_bins > 0) {
            // min(n_bins - 1, max(0, (int)floor(x))), clamped before the conversion: NaN -> bin 0, +-inf and huge values -> the outer bins
            const double b = floor(mul_x(add_x(proj, 1.0), bin_scale));
            const int bin = b >= 1.0 ? (b < (double)(a.n_bins - 1) ? (int)b : a.n_bins - 1) : 0;
            atomicAdd(&s_hist[bin], 1ull);
        }
        if (crossed && n_tbins > 0) {
            const double b = floor(mul_x(fp.t_x, tbin_scale));                     // (clamped before the conversion, as above)
            const int bin = b >= 1.0 ? (b < (double)(n_tbins - 1) ? (int)b : n_tbins - 1) : 0;
            atomicAdd(&s_thist[bin], 1ull);
        }
    }
    __syncthreads();
    if (lane == 0) {
        if (n_sw) atomicAdd(a.n_switched + g, n_sw);
        if (n_fail) atomicAdd(a.n_failed + g, n_fail);
        if (n_cr) atomicAdd(x.n_crossed + g, n_cr);
        if (n_ret) atomicAdd(x.n_returned + g, n_ret);
    }
    if (lane < a.n_bins) {
        const unsigned long long v = s_hist[lane];
        if (v) atomicAdd(a.hist + (int64_t)g * a.n_bins + lane, v);
    }
    for (int32_t b = lane; b < n_tbins; b += 64) {
        const unsigned long long v = s_thist[b];
        if (v) atomicAdd(x.t_hist + (int64_t)g * n_tbins + b, v);
    }
}

template <int SOLVER>
static void dispatch_switch_times(const SwitchTimesArgs& a, bool thermal, bool multi, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)a.w.s.G * a.w.s.waves_per_cond));
    const size_t lds = sizeof(unsigned long long) * (size_t)a.n_tbins;
    const bool wave = a.w.kj > 0 || a.w.kh > 0;
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(wave, [&](auto WAVE) {
        hipLaunchKernelGGL((stg_switch_times_kernel<SOLVER, THERMAL.value, MULTI.value, WAVE.value>), grid, dim3(64), lds, st, a);
    }); }); });
}

void stg_switch_times_launch(const SwitchTimesArgs& a, int solver, bool thermal, bool multi, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_switch_times<STG_SOLVER_RK4>(a, thermal, multi, st); break;
        case STG_SOLVER_EULER: dispatch_switch_times<STG_SOLVER_EULER>(a, thermal, multi, st); break;
        default: dispatch_switch_times<STG_SOLVER_RK45>(a, thermal, multi, st); break;
    }
}
