// stg_step_knots.hip -- the kernel of stg_step_knots and stg_step_knots_ids: K env steps in one launch whose actions carry the pulse's knot
// amplitudes, [J, T, s_0 ... s_{P-1}] per env and step.  The knot times tau and the field table are the context's (stg_set_pulse_knots),
// the same for every env and every step, staged in LDS; the amplitudes are parsed from the action itself.  It is stg_step_shaped_kernel
// (stg_step_shaped.hip) with one change: the current table's values come from the lane's own column of a [P][64] block in dynamic LDS,
// which the lane fills from its action at the top of each step (LaneKnots, stg_wave.hpp), instead of from the shared `scale` table.
// Staged rather than re-read from the action: valid(), pulse_sq_integral and the cursor each walk the amplitudes, the cursor at knot
// crossings that differ from lane to lane inside the sub-step loop -- an LDS read there costs what the shaped kernel's does, a global
// load would stall the whole wavefront per crossing and keep a 64-bit action address alive across the solve.
// (rk4 | euler | rk45) x thermal x class table x action dtype x IDS, fp64, one env per lane in identity order, 64-thread blocks: no lane
// sort, no producer wavefronts, no refill.  An env gets the bits stg_step_wave gives it for the tables (tau_j T, J s_j).
// A translation unit of its own: no other kernel is compiled with it.
#include "stg_wave.hpp"

// the knots as the context keeps them on the device and the kernel stages them into LDS: tau, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
constexpr int KNOTS_TAU = 0, KNOTS_TH = STG_MAX_KNOTS, KNOTS_HK = 2 * STG_MAX_KNOTS;
static_assert(KNOTS_HK + 3 * STG_MAX_KNOTS == STG_KNOTS_DOUBLES, "layout of the device copy of the pulse knots");

using KnotsJ = Pwl<1, LaneKnots>;                     // (tau_j * T, J * s_j), s_j from this step's action
using KnotsH = Pwl<3, SharedKnots<3, false>>;         // the field table as it is
using KnotsSource = WaveSourceT<KnotsJ, KnotsH>;

// IDS (stg_step_knots_ids): a.N is the list length M -- the launch's slots, and the stride and index of its outputs and actions --, the
// env of list position o is ids[o] (state record, Philox counter, class row); an id >= n_state is never dereferenced.
template <int SOLVER, bool THERMAL, bool MULTI, typename AT, bool IDS>
__global__ void __launch_bounds__(64) stg_step_knots_kernel(const KnotsStepArgs w) {
    // the env-step arithmetic around the solver has no contraction, as in stg_step_kernel
#pragma clang fp contract(off)
    __shared__ double s_tab[MULTI ? STG_MAX_CLASSES * C_COUNT : 1];
    __shared__ double s_knots[STG_KNOTS_DOUBLES];
    __shared__ unsigned long long s_cnt[3];
    extern __shared__ double s_amp[];                 // [P][64]: lane l's parsed amplitudes of the current step at s_amp[j * 64 + l]
    const StepArgs& a = w.s;
    const int64_t N = a.N;
    // 0. tau and the field table -> LDS: a lane reaches a knot by its own index when its cursor crosses one
    for (int j = threadIdx.x; j < STG_KNOTS_DOUBLES; j += 64) s_knots[j] = w.knots[j];
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
    const int32_t P = w.P;
    const int64_t rows = 2 + (int64_t)P;                                // rows of one step's action block
    const bool has_h = w.kh > 0;                                        // (kernel-uniform)
    const double lim = w.s_limit;
    double* amp = s_amp + threadIdx.x;
    unsigned long long c_steps = 0, c_sub = 0, c_noop = 0;
    for (int k = 0; k < a.K; ++k) {
        // the step index and the lane's list position as this iteration sees them: opaque copies, as in stg_step_shaped_kernel
        int64_t ol = o;
        int kl = k;
        asm volatile("" : "+v"(ol), "+s"(kl));
        // 2. the action: (J, T) as stg_step parses them, then the amplitudes -- fp64, clamped to +-s_limit by compares that keep a NaN;
        // one NaN among them voids the whole action to what stg_step makes of a NaN action
        double J, T;
        parse_action<AT>(act[((int64_t)kl * rows + 0) * N + ol], act[((int64_t)kl * rows + 1) * N + ol], a.c.max_current, a.c.max_duration, J, T);
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
            // 3. the drive of this env at this step: its amplitudes under its (J, T), cursors opened anew
            KnotsSource src;
            src.has_j = true; src.has_h = has_h;
            src.J = 0.0;
            src.T = T;
            src.cj.tk = s_knots + KNOTS_TAU; src.cj.vk = amp; src.cj.st = T; src.cj.sv = J; src.cj.K = P; src.cj.k = 0;
            src.ch.tk = s_knots + KNOTS_TH; src.ch.vk = s_knots + KNOTS_HK; src.ch.st = 1.0; src.ch.sv = 1.0; src.ch.K = w.kh; src.ch.k = 0;
            // 4. products of adjacent tau can tie after rounding (and J s_j can overflow): such a lane takes stg_step_wave's bad-table
            // path for this step.  (The field table was checked on the host when it was set.)
            if (!src.cj.valid()) {
                e_mode = STG_PULSE_NONE;
            } else {
                e_mode = STG_PULSE_TABLE;
                e_int = pulse_sq_integral(src.cj, T);
                src.cj.open();
                if (has_h) src.ch.open();
                src.arm();
                // 5. the solve
                if (SOLVER == STG_SOLVER_RK45) {
                    const LlgsK kk = load_llgs(row);
                    const LlgsWaveK wk{row[C_BETA], row[C_BETAP], -row[C_GAMMA], 0.0, 0.0, (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
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

template <int SOLVER>
static void dispatch_step_knots(const KnotsStepArgs& a, bool thermal, bool multi, int act_f64, hipStream_t st) {
    const size_t lds = sizeof(double) * 64 * (size_t)a.P;              // the amplitude block: 16 KB at P = STG_MAX_KNOTS
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(act_f64 != 0, [&](auto F64) {
        with_flag(a.s.ids != nullptr, [&](auto IDS) {
            using AT = typename std::conditional<F64.value, double, float>::type;
            hipLaunchKernelGGL((stg_step_knots_kernel<SOLVER, THERMAL.value, MULTI.value, AT, IDS.value>),
                               dim3((unsigned)((a.s.N + 63) / 64)), dim3(64), lds, st, a);
        });
    }); }); });
}

void stg_step_knots_launch(const KnotsStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_step_knots<STG_SOLVER_RK4>(a, thermal, multi, act_f64, st); break;
        case STG_SOLVER_EULER: dispatch_step_knots<STG_SOLVER_EULER>(a, thermal, multi, act_f64, st); break;
        default: dispatch_step_knots<STG_SOLVER_RK45>(a, thermal, multi, act_f64, st); break;
    }
}
