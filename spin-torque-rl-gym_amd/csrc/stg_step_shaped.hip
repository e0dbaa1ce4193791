// stg_step_shaped.hip -- the kernel of stg_step_shaped and stg_step_shaped_ids: K env steps in one launch under the context's pulse shape
// (stg_set_pulse_shape) -- a current shape (tau_j, s_j) applied to each step's parsed action (J, T), and one field table for every env.
// It is stg_step_wave_kernel (stg_step_wave.hip) with two changes: the knots come from LDS instead of per-env tables in HBM -- the shape
// is the same for every env and every step, a lane's current table is just (tau_j T, J s_j), so nothing has to be built on the host or
// read back at stride N --, and that is what lets K steps be fused: the state stays in registers between the steps as in stg_step_kernel.
// (rk4 | euler | rk45) x thermal x class table x action dtype x IDS, fp64, one env per lane in identity order, 64-thread blocks: no lane
// sort, no producer wavefronts, no refill.  An env gets the bits stg_step_wave gives it for the tables envs.pulse_tables builds.
// A translation unit of its own: no other kernel is compiled with it.
#include "stg_wave.hpp"

// the shape as the context keeps it on the device and the kernel stages it into LDS: tau, scale, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
constexpr int SHAPE_TAU = 0, SHAPE_SCALE = STG_MAX_KNOTS, SHAPE_TH = 2 * STG_MAX_KNOTS, SHAPE_HK = 3 * STG_MAX_KNOTS;
static_assert(SHAPE_HK + 3 * STG_MAX_KNOTS == STG_SHAPE_DOUBLES, "layout of the device copy of the pulse shape");

using ShapedJ = Pwl<1, SharedKnots<1, true>>;         // (tau_j * T, J * s_j)
using ShapedH = Pwl<3, SharedKnots<3, false>>;        // the field table as it is
using ShapedSource = WaveSourceT<ShapedJ, ShapedH>;

// IDS (stg_step_shaped_ids): a.N is the list length M -- the launch's slots, and the stride and index of its outputs and actions --, the
// env of list position o is ids[o] (state record, Philox counter, class row); an id >= n_state is never dereferenced.
template <int SOLVER, bool THERMAL, bool MULTI, typename AT, bool IDS>
__global__ void __launch_bounds__(64) stg_step_shaped_kernel(const ShapedStepArgs w) {
    // the env-step arithmetic around the solver has no contraction, as in stg_step_kernel
#pragma clang fp contract(off)
    __shared__ double s_tab[MULTI ? STG_MAX_CLASSES * C_COUNT : 1];
    __shared__ double s_shape[STG_SHAPE_DOUBLES];
    __shared__ unsigned long long s_cnt[3];
    const StepArgs& a = w.s;
    const int64_t N = a.N;
    // 0. the shape -> LDS: a lane reaches a knot by its own index when its cursor crosses one
    for (int j = threadIdx.x; j < STG_SHAPE_DOUBLES; j += 64) s_shape[j] = w.shape[j];
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
    const bool has_j = w.kj > 0, has_h = w.kh > 0;                      // (kernel-uniform; at least one of them: the entry checks)
    unsigned long long c_steps = 0, c_sub = 0, c_noop = 0;
    for (int k = 0; k < a.K; ++k) {
        // The step index and the lane's list position as this iteration sees them: opaque copies (an empty asm, no instruction).  With
        // the plain values the compiler turns every output and action address into an induction pointer of its own, kept in registers
        // across the solve: +86 VGPRs over stg_step_wave_kernel and a stack frame in the fixed-step kernels (profiles/NOTEBOOK.md).
        int64_t ol = o;
        int kl = k;
        asm volatile("" : "+v"(ol), "+s"(kl));
        double J, T;
        parse_action<AT>(act[((int64_t)kl * 2 + 0) * N + ol], act[((int64_t)kl * 2 + 1) * N + ol], a.c.max_current, a.c.max_duration, J, T);
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
            // 2. the drive of this env at this step: the shape under its action, cursors opened anew
            ShapedSource src;
            src.has_j = has_j; src.has_h = has_h;
            src.J = has_j ? 0.0 : J;
            src.T = T;
            src.cj.tk = s_shape + SHAPE_TAU; src.cj.vk = s_shape + SHAPE_SCALE; src.cj.st = T; src.cj.sv = J; src.cj.K = w.kj; src.cj.k = 0;
            src.ch.tk = s_shape + SHAPE_TH; src.ch.vk = s_shape + SHAPE_HK; src.ch.st = 1.0; src.ch.sv = 1.0; src.ch.K = w.kh; src.ch.k = 0;
            // 3. products of adjacent tau can tie after rounding (and J s_j can overflow): such a lane takes stg_step_wave's bad-table
            // path for this step.  (The field table was checked on the host when it was set.)
            if (has_j && !src.cj.valid()) {
                e_mode = STG_PULSE_NONE;
            } else {
                if (has_j) { e_mode = STG_PULSE_TABLE; e_int = pulse_sq_integral(src.cj, T); }
                if (has_j) src.cj.open();
                if (has_h) src.ch.open();
                src.arm();
                // 4. the solve
                if (SOLVER == STG_SOLVER_RK45) {
                    const LlgsK kk = load_llgs(row);
                    const double beta = row[C_BETA], betap = row[C_BETAP];
                    const bool useJ = !(fabs(src.J) < 1e-12);                           // llgs_solver.py:222
                    const LlgsWaveK wk{beta, betap, -row[C_GAMMA], useJ ? beta * src.J : 0.0, useJ ? betap * src.J : 0.0,
                                       (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
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
        // 5. energy, state update, reward, flags, same-step auto-reset, outputs: the step kernels' tail with this pulse's energy
        env_step_tail<true>(a, ol, ko, wr, true, lane_solves, row, env_id, m, tgt, etot, step, rng, done, J, T, so, c_steps, c_sub, c_noop,
                            e_mode, e_int);
    }
    store_state(a.s, i, m, tgt, etot, step, rng, done);
    wave_add3(a.counters + (size_t)(blockIdx.x % COUNTER_STRIPES) * COUNTER_STRIDE, s_cnt, c_steps, c_sub, c_noop);
}

template <int SOLVER>
static void dispatch_step_shaped(const ShapedStepArgs& a, bool thermal, bool multi, int act_f64, hipStream_t st) {
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(act_f64 != 0, [&](auto F64) {
        with_flag(a.s.ids != nullptr, [&](auto IDS) {
            using AT = typename std::conditional<F64.value, double, float>::type;
            hipLaunchKernelGGL((stg_step_shaped_kernel<SOLVER, THERMAL.value, MULTI.value, AT, IDS.value>),
                               dim3((unsigned)((a.s.N + 63) / 64)), dim3(64), 0, st, a);
        });
    }); }); });
}

void stg_step_shaped_launch(const ShapedStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_step_shaped<STG_SOLVER_RK4>(a, thermal, multi, act_f64, st); break;
        case STG_SOLVER_EULER: dispatch_step_shaped<STG_SOLVER_EULER>(a, thermal, multi, act_f64, st); break;
        default: dispatch_step_shaped<STG_SOLVER_RK45>(a, thermal, multi, act_f64, st); break;
    }
}
