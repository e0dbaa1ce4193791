// stg_step_wave.hip -- the kernel of stg_step_wave: SpinTorqueEnv.step with piecewise-linear current_func(t) and field_func(t) in place of
// the rectangular pulse in zero field that _simulate_dynamics hard-codes (spin_torque_env.py:442-447).  It joins what exists: the action
// parse and the state record of the step kernels, the waveform solvers of stg_wave.hpp (simple_solve_wave / llgs_solve_wave, the device
// functions of stg_solve_wave), and env_step_tail for everything after the solve.  (rk4 | euler | rk45) x thermal x class table x action
// dtype, fp64, one env per lane in identity order: no lane sort, no producer wavefronts, no refill -- deliberately the simple schedule.
// A translation unit of its own: the step kernels, stg_solve_kernel and the array kernels are compiled without it.
#include "stg_wave.hpp"

template <int SOLVER, bool THERMAL, bool MULTI, typename AT>
__global__ void __launch_bounds__(64) stg_step_wave_kernel(const WaveStepArgs w) {
    // the env-step arithmetic around the solver has no contraction, as in stg_step_kernel
#pragma clang fp contract(off)
    __shared__ double s_tab[MULTI ? STG_MAX_CLASSES * C_COUNT : 1];
    __shared__ unsigned long long s_cnt[3];
    const StepArgs& a = w.s;
    const int64_t N = a.N;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < N;
    // 1. class row, state record, action
    const double* row = class_row<MULTI>(a.ctab, a.cls, a.ncls, i, live, s_tab, EnvParams{});
    if (!live) return;
    const uint64_t env_id = (uint64_t)(a.env_id0 + i);
    V3 m, tgt;
    double etot;
    int32_t step;
    uint32_t rng;
    bool done;
    load_state(a.s, i, m, tgt, etot, step, rng, done);
    const AT* act = (const AT*)a.actions;
    double J, T;
    parse_action<AT>(act[i], act[N + i], a.c.max_current, a.c.max_duration, J, T);
    const bool lane_solves = !(a.c.skip_done && done);
    unsigned long long c_steps = 0, c_sub = 0, c_noop = 0;
    SolveOut so{m, 0, 0, 0, false};
    int e_mode = STG_PULSE_RECT;
    double e_int = 0.0;
    if (lane_solves) {
        const RngKey rk{a.c.seed, env_id, rng};                     // the step kernels' key: a zero-table call draws stg_step's stream
        const Recorder norec{};
        InlineNormals ns;
        const bool has_j = w.kj > 0, has_h = w.kh > 0;              // (kernel-uniform)
        if (!has_j && !has_h) {
            // no table at all is stg_step's pulse: its own integrator, in the form stg_step takes for this context (the easy-axis
            // specialisation rounds differently from the general form), so that the two entries agree bit for bit
            if (w.axis_z) so = run_solver<SOLVER, THERMAL, false, true, false>(m, J, T, row, a.c, rk, norec, ns, true);
            else so = run_solver<SOLVER, THERMAL, false, false, false>(m, J, T, row, a.c, rk, norec, ns, true);
        } else {
            // 2. the drive of this env: its columns of the tables
            WaveSource src;
            src.has_j = has_j; src.has_h = has_h;
            src.J = has_j ? 0.0 : J;
            src.T = T;
            src.cj.tk = w.tj; src.cj.vk = w.jk; src.cj.N = N; src.cj.i = i; src.cj.K = w.kj; src.cj.k = 0;
            src.ch.tk = w.th; src.ch.vk = w.hk; src.ch.N = N; src.ch.i = i; src.ch.K = w.kh; src.ch.k = 0;
            // 3. a table that is not finite or not strictly increasing fails its lane like a failed solve: no-op, no energy
            const bool tables_ok = (!has_j || src.cj.valid()) && (!has_h || src.ch.valid());
            if (!tables_ok) {
                e_mode = STG_PULSE_NONE;
            } else {
                if (has_j) { e_mode = STG_PULSE_TABLE; e_int = pulse_sq_integral(src.cj, T); }
                if (has_j) src.cj.open();
                if (has_h) src.ch.open();
                src.arm();
                // 4. the solve
                if (SOLVER == STG_SOLVER_RK45) {
                    const LlgsK k = load_llgs(row);
                    const double beta = row[C_BETA], betap = row[C_BETAP];
                    const bool useJ = !(fabs(src.J) < 1e-12);                           // llgs_solver.py:222
                    const LlgsWaveK wk{beta, betap, -row[C_GAMMA], useJ ? beta * src.J : 0.0, useJ ? betap * src.J : 0.0,
                                       (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
                    so = llgs_solve_wave<THERMAL, false>(m, T, k, a.c.rtol, a.c.atol, a.c.max_step, a.c.max_attempts, rk, norec, LlgsEnergyK{},
                                                         ns, src, wk);
                } else {
                    const SimpleK k = load_simple(row);
                    so = simple_solve_wave<SOLVER == STG_SOLVER_EULER ? 1 : 0, THERMAL, false>(
                        m, T, k, -row[C_GEFF], row[C_POL], row[C_MSV], row[C_VALID] != 0.0, a.c.temperature, a.c.max_step, rk, norec, ns,
                        a.c.inv_tau, src);
                }
            }
        }
    }
    // 5. energy, state update, reward, flags, same-step auto-reset, outputs: the step kernels' tail with this pulse's energy
    env_step_tail<true>(a, i, 0, true, true, lane_solves, row, env_id, m, tgt, etot, step, rng, done, J, T, so, c_steps, c_sub, c_noop,
                        e_mode, e_int);
    store_state(a.s, i, m, tgt, etot, step, rng, done);
    wave_add3(a.counters + (size_t)(blockIdx.x % COUNTER_STRIPES) * COUNTER_STRIDE, s_cnt, c_steps, c_sub, c_noop);
}

template <int SOLVER>
static void dispatch_step_wave(const WaveStepArgs& a, bool thermal, bool multi, int act_f64, hipStream_t st) {
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(act_f64 != 0, [&](auto F64) {
        using AT = typename std::conditional<F64.value, double, float>::type;
        hipLaunchKernelGGL((stg_step_wave_kernel<SOLVER, THERMAL.value, MULTI.value, AT>), dim3((unsigned)((a.s.N + 63) / 64)), dim3(64), 0, st,
                           a);
    }); }); });
}

void stg_step_wave_launch(const WaveStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_step_wave<STG_SOLVER_RK4>(a, thermal, multi, act_f64, st); break;
        case STG_SOLVER_EULER: dispatch_step_wave<STG_SOLVER_EULER>(a, thermal, multi, act_f64, st); break;
        default: dispatch_step_wave<STG_SOLVER_RK45>(a, thermal, multi, act_f64, st); break;
    }
}
