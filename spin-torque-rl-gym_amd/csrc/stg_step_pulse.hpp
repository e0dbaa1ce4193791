// stg_step_pulse.hpp -- the ONE kernel of the pulse-step family, stg_step_shaped / stg_step_shaped_ids and stg_step_knots /
// stg_step_knots_ids (C-ABI: spintorque_hip.hip): K env steps in one launch whose current pulse is a table (tau_j T, J s_j) under each
// step's parsed action (J, T), with one field table for every env.  The knot times tau and the field table are the context's, the same
// for every env and every step, staged in LDS: a lane's table is built from its action in the kernel, so nothing has to be made on the
// host or read back at stride N, and that is what lets K steps be fused -- the state stays in registers between the steps as in
// stg_step_kernel.  It is stg_step_wave_kernel (stg_step_wave.hip) in every other respect, and an env gets the bits stg_step_wave gives
// it for the tables (tau_j T, J s_j).
// (rk4 | euler | rk45) x thermal x class table x action dtype x IDS x PULSE, fp64, one env per lane in identity order, 64-thread blocks:
// no lane sort, no producer wavefronts, no refill.  The kernel is instantiated per policy in stg_step_shaped.hip (ShapedPulse) and
// stg_step_knots.hip (KnotsPulse) and nowhere else: two translation units, compiled side by side.
//
// PULSE says where the amplitudes s_j come from, and only that:
//   Args                   the launch's argument block: StepArgs s, kj, kh, tab (the context's device table), and s_limit with LANE_AMPS
//   DOUBLES, TAU, TH, HK   the size of the table and the offsets of tau, th [STG_MAX_KNOTS] each and hk [STG_MAX_KNOTS][3] in it
//   J, values(tab, amp)    the cursor type of the current table, and where it finds the amplitudes
//   LANE_AMPS              false (ShapedPulse): the amplitudes are a row of the table, an action is (J, T), and kj = 0 -- no current
//                          table, rectangular J while t <= T -- is a launch like any other: has_j is a run-time flag.
//                          true (KnotsPulse): an action is (J, T, s_0 ... s_{kj-1}); the lane parses the amplitudes into its column of
//                          a [kj][64] block in dynamic LDS at the top of each step.  There is always a current table, and the kernel
//                          knows it at compile time: the rectangular form and its selects fold away, which is worth 14-16 %
//                          (profiles/NOTEBOOK.md, round 15).
// An instantiation holds nothing of the other policy.  The statements stand in the order, and the drive constants in the form, in which
// both kernels compile to the machine code they had before they were merged (profiles/NOTEBOOK.md, round 27): a local more or less, or a
// policy member function where a flagged statement stands, moves it.
#pragma once
#include "stg_wave.hpp"

// IDS (the _ids entries): a.N is the list length M -- the launch's slots, and the stride and index of its outputs and actions --, the env
// of list position o is ids[o] (state record, Philox counter, class row); an id >= n_state is never dereferenced.
template <int SOLVER, bool THERMAL, bool MULTI, typename AT, bool IDS, class PULSE>
__global__ void __launch_bounds__(64) stg_step_pulse_kernel(const typename PULSE::Args w) {
    // the env-step arithmetic around the solver has no contraction, as in stg_step_kernel
#pragma clang fp contract(off)
    __shared__ double s_tab[MULTI ? STG_MAX_CLASSES * C_COUNT : 1];
    __shared__ double s_pulse[PULSE::DOUBLES];
    __shared__ unsigned long long s_cnt[3];
    extern __shared__ double s_amp[];                 // LANE_AMPS: [kj][64], lane l's amplitudes of the current step at s_amp[j * 64 + l]
    const StepArgs& a = w.s;
    const int64_t N = a.N;
    // 0. tau, the field table (and the shared amplitudes) -> LDS: a lane reaches a knot by its own index when its cursor crosses one
    for (int j = threadIdx.x; j < PULSE::DOUBLES; j += 64) s_pulse[j] = w.tab[j];
    __syncthreads();
    const int64_t o = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool in_list = o < N;
    const uint32_t id = (IDS && in_list) ? a.ids[o] : 0u;
    const bool bad = IDS && in_list && (int64_t)id >= a.n_state;
    const bool live = in_list && !bad;
    const int64_t i = IDS ? (live ? (int64_t)id : 0) : o;
    // 1. class row, state record
    const double* row = class_row<MULTI>(a.ctab, a.cls, a.ncls, i, live, s_tab, EnvParams{});
    if (bad) write_bad_id(a, o);
    if (!live) return;
    const uint64_t env_id = (uint64_t)(a.env_id0 + i);
    V3 m, tgt;
    double etot;
    int32_t step;
    uint32_t rng;
    bool done;
    load_state(a.s, i, m, tgt, etot, step, rng, done);
    const AT* act = (const AT*)a.actions;
    const Recorder norec{};
    const int32_t P = PULSE::LANE_AMPS ? w.kj : 0;                      // amplitude rows of one step's action block
    const int64_t rows = 2 + (int64_t)P;
    const bool has_j = PULSE::LANE_AMPS || w.kj > 0, has_h = w.kh > 0;  // (kernel-uniform; at least one of them: the entry checks)
    double* amp = s_amp + threadIdx.x;
    unsigned long long c_steps = 0, c_sub = 0, c_noop = 0;
    for (int k = 0; k < a.K; ++k) {
        // The step index and the lane's list position as this iteration sees them: opaque copies (an empty asm, no instruction).  With
        // the plain values the compiler turns every output and action address into an induction pointer of its own, kept in registers
        // across the solve: +86 VGPRs over stg_step_wave_kernel and a stack frame in the fixed-step kernels (profiles/NOTEBOOK.md).
        int64_t ol = o;
        int kl = k;
        asm volatile("" : "+v"(ol), "+s"(kl));
        // 2. the action: (J, T) as stg_step parses them
        double J, T;
        parse_action<AT>(act[((int64_t)kl * rows + 0) * N + ol], act[((int64_t)kl * rows + 1) * N + ol], a.c.max_current, a.c.max_duration, J, T);
        if constexpr (PULSE::LANE_AMPS) {
            // then the amplitudes: fp64, clamped to +-s_limit by compares that keep a NaN; one NaN among them voids the whole action to what
            // stg_step makes of a NaN action
            const double lim = w.s_limit;
            bool amp_nan = false;
            for (int32_t j = 0; j < P; ++j) {
                double s = (double)act[((int64_t)kl * rows + 2 + j) * N + ol];
                s = s < -lim ? -lim : (s > lim ? lim : s);
                amp_nan = amp_nan || isnan(s);
                amp[j * 64] = s;
            }
            if (amp_nan) {
                J = 0.0; T = 1e-12;
                for (int32_t j = 0; j < P; ++j) amp[j * 64] = 0.0;
            }
        }
        const bool last = (k == a.K - 1);
        const int64_t ko = a.out_every ? kl : 0;
        const bool wr = a.out_every || last;
        const bool lane_solves = !(a.c.skip_done && done);
        SolveOut so{m, 0, 0, 0, false};
        int e_mode = STG_PULSE_RECT;
        double e_int = 0.0;
        if (lane_solves) {
            const RngKey rk{a.c.seed, env_id, rng};
            InlineNormals ns;
            // 3. the drive of this env at this step: the amplitudes under its (J, T), cursors opened anew
            WaveSourceT<typename PULSE::J, Pwl<3, SharedKnots<3, false>>> src;     // (the field table as it is)
            src.has_j = has_j; src.has_h = has_h;
            src.J = has_j ? 0.0 : J;
            src.T = T;
            src.cj.tk = s_pulse + PULSE::TAU; src.cj.vk = PULSE::values(s_pulse, amp); src.cj.st = T; src.cj.sv = J; src.cj.K = w.kj; src.cj.k = 0;
            src.ch.tk = s_pulse + PULSE::TH; src.ch.vk = s_pulse + PULSE::HK; src.ch.st = 1.0; src.ch.sv = 1.0; src.ch.K = w.kh; src.ch.k = 0;
            // 4. products of adjacent tau can tie after rounding (and J s_j can overflow): such a lane takes stg_step_wave's bad-table
            // path for this step.  (The field table was checked on the host when it was set.)
            if (has_j && !src.cj.valid()) {
                e_mode = STG_PULSE_NONE;
            } else {
                if (has_j) { e_mode = STG_PULSE_TABLE; e_int = pulse_sq_integral(src.cj, T); }
                if (has_j) src.cj.open();
                if (has_h) src.ch.open();
                src.arm();
                // 5. the solve
                if (SOLVER == STG_SOLVER_RK45) {
                    const LlgsK kk = load_llgs(row);
                    const bool useJ = !PULSE::LANE_AMPS && !(fabs(src.J) < 1e-12);      // llgs_solver.py:222
                    const LlgsWaveK wk{row[C_BETA], row[C_BETAP], -row[C_GAMMA], useJ ? row[C_BETA] * src.J : 0.0,
                                       useJ ? row[C_BETAP] * src.J : 0.0, (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
                    so = llgs_solve_wave<THERMAL, false>(m, T, kk, a.c.rtol, a.c.atol, a.c.max_step, a.c.max_attempts, rk, norec, LlgsEnergyK{},
                                                         ns, src, wk);
                } else {
                    const SimpleK kk = load_simple(row);
                    so = simple_solve_wave<SOLVER == STG_SOLVER_EULER ? 1 : 0, THERMAL, false>(
                        m, T, kk, -row[C_GEFF], row[C_POL], row[C_MSV], row[C_VALID] != 0.0, a.c.temperature, a.c.max_step, rk, norec, ns,
                        a.c.inv_tau, src);
                }
            }
        }
        // 6. energy, state update, reward, flags, same-step auto-reset, outputs: the step kernels' tail with this pulse's energy
        env_step_tail<true>(a, ol, ko, wr, true, lane_solves, row, env_id, m, tgt, etot, step, rng, done, J, T, so, c_steps, c_sub, c_noop,
                            e_mode, e_int);
    }
    store_state(a.s, i, m, tgt, etot, step, rng, done);
    wave_add3(a.counters + (size_t)(blockIdx.x % COUNTER_STRIPES) * COUNTER_STRIDE, s_cnt, c_steps, c_sub, c_noop);
}

template <int SOLVER, class PULSE>
static void dispatch_step_pulse(const typename PULSE::Args& a, bool thermal, bool multi, int act_f64, hipStream_t st) {
    const size_t lds = PULSE::LANE_AMPS ? sizeof(double) * 64 * (size_t)a.kj : 0;      // s_amp: 16 KB at kj = STG_MAX_KNOTS
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(act_f64 != 0, [&](auto F64) {
        with_flag(a.s.ids != nullptr, [&](auto IDS) {
            using AT = typename std::conditional<F64.value, double, float>::type;
            hipLaunchKernelGGL((stg_step_pulse_kernel<SOLVER, THERMAL.value, MULTI.value, AT, IDS.value, PULSE>),
                               dim3((unsigned)((a.s.N + 63) / 64)), dim3(64), lds, st, a);
        });
    }); }); });
}

// s.ids != nullptr: the id form
template <class PULSE>
void stg_step_pulse_launch(const typename PULSE::Args& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_step_pulse<STG_SOLVER_RK4, PULSE>(a, thermal, multi, act_f64, st); break;
        case STG_SOLVER_EULER: dispatch_step_pulse<STG_SOLVER_EULER, PULSE>(a, thermal, multi, act_f64, st); break;
        default: dispatch_step_pulse<STG_SOLVER_RK45, PULSE>(a, thermal, multi, act_f64, st); break;
    }
}
