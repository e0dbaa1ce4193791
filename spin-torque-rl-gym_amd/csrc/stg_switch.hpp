// stg_switch.hpp -- the Monte-Carlo switching family: the argument blocks, the first-passage observer and the ONE trial kernel of
// stg_switch_stats, stg_switch_stats_wave, stg_switch_times and stg_switch_population (C-ABI: spintorque_hip.hip), (rk4 | euler | rk45)
// x thermal x class table x WAVE x TIMES, and VARY x thermal x WAVE x TIMES, fp64.  The kernel is instantiated per solver in
// stg_switch_rk4.hip / _euler.hip / _rk45.hip and nowhere else.
//
// One 64-lane wavefront per workgroup works on ONE condition g: its m0, phase table, target, class row and waveform tables are
// wave-uniform (scalar loads, the tables staged in LDS), and the sub-step count of a fixed-step phase is the same in every lane.  A lane
// runs L trials one after the other; a trial is the chain of the condition's phases, each of them exactly the solve of stg_solve_kernel
// (run_solver with InlineNormals on the stream of problem g * trial_stride + trial at env_step + p).  The counts stay in registers
// (ballot + popcount) and in LDS (the histograms, integer atomics) until the wavefront is through with its trials; then one lane adds
// each scalar count, and lane b adds bin b (and bins b, b + 64, ... of t_hist), to the caller's arrays with 64-bit atomics.  Integer
// sums: the result does not depend on L, the grid or the arrival order.
//   WAVE   phase `wave_phase` is the solve of stg_solve_wave_kernel (simple_solve_wave / llgs_solve_wave of stg_wave.hpp) on the
//          condition's piecewise-linear tables: the wavefront stages its column of them into LDS once and every trial opens its cursors
//          there (SharedKnots, unscaled: the same doubles GlobalKnots hands Pwl for a replicated table, so Pwl gives the same bits).
//   TIMES  phase `wave_phase` -- rectangular or tabled -- runs with RECORD set and FirstPassage as its observer: the rows it sees are
//          the rows stg_solve_traj / stg_solve_wave record.  The time histogram's LDS is sized by the launch: 8 n_tbins bytes.
//   VARY   (stg_switch_population) every lane draws the device its trial belongs to (stg_vary.hpp: device r / Q, five clipped normals
//          of the device's own stream scale the nominal record's damping, Ms, K_u, volume and polarization), derives that device's row
//          with derive_row -- the arithmetic of a class table row -- into a private array, and runs every phase, plain, tabled and
//          watched alike, on it instead of the wave-uniform row.  The draw is kept while a lane's next trial is the same device's.
// An instantiation without a flag holds nothing of what the flag brings: no staged tables, no observer, no extra counts, no row of its own.
// (Constants fold the flagged statements away; their order is kept as it is on purpose: the TIMES instantiations compile to the same
// machine code as before the three entries were merged -- profiles/NOTEBOOK.md, round 23.)
#pragma once
#include "stg_wave.hpp"
#include "stg_vary.hpp"

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

struct SwitchStatsWaveArgs {
    SwitchStatsArgs s;            // as stg_switch_stats; J[wave_phase][g] is read only without a current table
    int32_t wave_phase;           // the phase the tables drive (0 ... P - 1); the others are rectangular
    int32_t kj, kh;               // knot counts; 0: rectangular J while t <= T / zero field (stg_switch_stats_wave: not both 0)
    const double *tj, *jk;        // [kj][G], [kj][G]
    const double *th, *hk;        // [kh][G], [kh][3][G]
};

struct SwitchTimesArgs {
    SwitchStatsWaveArgs w;        // as stg_switch_stats_wave; w.wave_phase is the WATCHED phase, and kj = kh = 0 (rectangular) is valid
    int32_t n_tbins;              // 0 ... STG_MAX_TBINS
    unsigned long long *n_crossed, *n_returned, *t_hist;   // [G], [G], [G][n_tbins] (nullptr iff n_tbins == 0): added to
};

// stg_switch_population: every lane draws the device of its trial and integrates with that device's own row (stg_vary.hpp: the rule)
struct SwitchVaryArgs {
    const double* sigma;              // [STG_NVARY][G]
    const stg_device_params* ptab;    // the context's class table as the caller gave it (the nominal records), [ncls]
    double z_clip, gamma;
    int64_t Q;                        // trials per device
    uint32_t var_step;
    unsigned long long* dev_switched; // [G][dev_stride], indexed by the absolute device id: added to; or nullptr
    int64_t dev_stride;
};
struct SwitchPopArgs {
    SwitchTimesArgs t;                // as stg_switch_times
    SwitchVaryArgs v;
};

// One device of the population: its six normals -- calls 0 and 1 of the thermal stream of `dev_env` at counter word var_step, the
// values stg_thermal_normals dumps -- and its record (vary_params on the first five).  The trial kernel and the diagnostic dump both
// call this and nothing else.
__device__ __forceinline__ void vary_draw(uint64_t seed, uint64_t dev_env, uint32_t var_step, const stg_device_params& nominal,
                                          const double* sigma, int64_t G, int64_t g, double z_clip, double (&z)[6], stg_device_params& out) {
    NormalStream s;
    s.init(seed, dev_env, var_step, 0u);
    const V3 a = s.draw3_even(), b = s.draw3_odd();
    z[0] = a.x; z[1] = a.y; z[2] = a.z; z[3] = b.x; z[4] = b.y; z[5] = b.z;
    vary_params(nominal, sigma, G, g, z, z_clip, out);
}

// The per-point observer of the watched phase (the REC parameter of the solvers, stg_physics.hpp: Recorder): the first passage of
// m . target over `threshold`, kept in three values per lane (crossed, t_x, t_prev: two fp64 register pairs and one bit of a wave mask).
// It stores nothing and wants no energy and no torque norm.
//   proj_k = ((m_k.x * tx) + (m_k.y * ty)) + (m_k.z * tz) without contraction, as the classification of the trial's end forms it;
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

// the condition's tables in LDS: tj, jk, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
constexpr int KN_TJ = 0, KN_JK = STG_MAX_KNOTS, KN_TH = 2 * STG_MAX_KNOTS, KN_HK = 3 * STG_MAX_KNOTS;
static_assert(KN_HK + 3 * STG_MAX_KNOTS == STG_SHAPE_DOUBLES, "layout of the staged tables");
static_assert(STG_MAX_KNOTS <= 64, "lane j stages knot j");

using SwitchSource = WaveSourceT<Pwl<1, SharedKnots<1, false>>, Pwl<3, SharedKnots<3, false>>>;

// The kernel's argument block: SwitchTimesArgs, or -- VARY -- SwitchPopArgs.  (The body reaches the block through `x`, set by a plain
// member access: handing the kernel argument to a function by reference, a forced-inline one included, changes the register allocation
// of every instantiation -- profiles/NOTEBOOK.md, round 24.)  Under VARY the class table only selects the nominal record, so MULTI is a
// run-time matter there -- cond_cls may be NULL -- and VARY is instantiated with MULTI = true alone.
template <int SOLVER, bool THERMAL, bool MULTI, bool WAVE, bool TIMES, bool VARY>
__global__ void __launch_bounds__(64) stg_switch_kernel(const std::conditional_t<VARY, SwitchPopArgs, SwitchTimesArgs> xa) {
    static_assert(STG_MAX_BINS == 64, "lane b owns bin b");
    const SwitchTimesArgs* xp;
    if constexpr (VARY) xp = &xa.t; else xp = &xa;
    const SwitchTimesArgs& x = *xp;
    __shared__ unsigned long long s_hist[STG_MAX_BINS];
    __shared__ double s_knots[WAVE ? STG_SHAPE_DOUBLES : 1];
    extern __shared__ unsigned long long s_thist[];                                // [n_tbins]
    const SwitchStatsWaveArgs& w = x.w;
    const SwitchStatsArgs& a = w.s;
    const int lane = (int)threadIdx.x;
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)a.waves_per_cond);
    const int64_t wv = (int64_t)(blockIdx.x % (uint32_t)a.waves_per_cond);
    const int32_t G = a.G;
    const int32_t n_tbins = TIMES ? x.n_tbins : 0;
    s_hist[lane] = 0ull;
    if (TIMES) {
        for (int32_t b = lane; b < n_tbins; b += 64) s_thist[b] = 0ull;
    }
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
    int nominal_cls = 0;                                                           // (VARY: the condition's nominal record)
    if (MULTI) {
        const int c = a.cond_cls ? (int)a.cond_cls[g] : 0;
        row = a.ctab + (c < a.ncls ? c : 0) * C_COUNT;
        nominal_cls = c < a.ncls ? c : 0;
    }
    // VARY: the lane's own row of derived constants (constant indices only: the array dissolves into registers), the device it was
    // derived for, and whether the condition's sigma column is valid (wave-uniform)
    double own_row[VARY ? C_COUNT : 1];
    int64_t own_dev = -1;
    bool sigma_ok = true;
    if constexpr (VARY) {
        sigma_ok = vary_column_ok(xa.v.sigma, G, g, xa.v.z_clip);
        row = own_row;
    }
    const V3 m0{a.m0[g], a.m0[G + g], a.m0[2 * G + g]};
    const V3 tg{a.target[g], a.target[G + g], a.target[2 * G + g]};
    const Recorder norec{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    const int64_t id0 = a.env_id0 + (int64_t)g * a.trial_stride + a.trial0;       // env id of the condition's trial trial0
    const double bin_scale = mul_x(0.5, (double)a.n_bins);
    // n_tbins equal bins over the watched phase's [0, T] (a skipped watched phase, T == 0, bins nothing)
    const double tbin_scale = TIMES ? (double)n_tbins / a.T[(int64_t)w.wave_phase * G + g] : 0.0;
    const bool has_j = WAVE && w.kj > 0, has_h = WAVE && w.kh > 0;                 // (kernel-uniform; WAVE: at least one of them)
    SwitchSource src;
    bool tables_ok = true;
    if (WAVE) {
        src.has_j = has_j; src.has_h = has_h;
        src.cj.tk = s_knots + KN_TJ; src.cj.vk = s_knots + KN_JK; src.cj.st = 1.0; src.cj.sv = 1.0; src.cj.K = w.kj; src.cj.k = 0;
        src.ch.tk = s_knots + KN_TH; src.ch.vk = s_knots + KN_HK; src.ch.st = 1.0; src.ch.sv = 1.0; src.ch.K = w.kh; src.ch.k = 0;
        // a table that is not finite or not strictly increasing fails the watched phase of every trial of this condition (wave-uniform)
        tables_ok = (!has_j || src.cj.valid()) && (!has_h || src.ch.valid());
    }
    unsigned long long n_sw = 0ull, n_fail = 0ull, n_cr = 0ull, n_ret = 0ull;      // wave-uniform (n_cr, n_ret: TIMES)
    for (int64_t l = 0; l < a.L; ++l) {
        const int64_t r = (wv * a.L + l) * 64 + lane;                              // this lane's trial, counted from trial0
        const bool active = r < a.R;
        V3 m = m0;
        bool failed = false;
        FirstPassage fp{tg, a.threshold, 0.0, 0.0, false};                         // (TIMES: with RECORD off no solver touches it)
        int64_t dev = 0;                                                           // (VARY: this trial's device)
        if constexpr (VARY) {
            dev = vary_device_of(a.trial0 + r, xa.v.Q);
            if (active && sigma_ok && dev != own_dev) {
                // a new device: its record from its own stream, its row by the arithmetic that builds a class table row
                const int64_t dev_env = vary_device_env(a.env_id0, g, a.trial_stride, dev, xa.v.Q);
                double z[6];
                stg_device_params dp;
                vary_draw(a.c.seed, (uint64_t)dev_env, xa.v.var_step, xa.v.ptab[nominal_cls], xa.v.sigma, G, g, xa.v.z_clip, z, dp);
                derive_row(dp, xa.v.gamma, a.c.temperature, own_row);
                own_dev = dev;
            }
        }
        if (active) {
            InlineNormals ns;
#pragma clang loop unroll(disable)
            for (int32_t p = 0; p < a.P && !failed; ++p) {
                const double Tp = a.T[(int64_t)p * G + g];
                if (Tp == 0.0) continue;
                if (VARY && !sigma_ok) {                                           // a bad sigma column: the first phase that would run fails
                    failed = true;
                    break;
                }
                // the tabled and / or watched phase (a compile-time `false` without a flag: the plain kernel keeps ONE call site of run_solver)
                const bool watched = (WAVE || TIMES) && p == w.wave_phase;
                const double Jp = (watched && has_j) ? 0.0 : a.J[(int64_t)p * G + g];
                const RngKey rk{a.c.seed, (uint64_t)(id0 + r), a.env_step + (uint32_t)p};
                SolveOut so{m, 0, 0, 0, false};
                if (!watched) {
                    so = run_solver<SOLVER, THERMAL, false, false, false>(m, Jp, Tp, row, a.c, rk, norec, ns, true);
                } else {
                    if (!WAVE) {
                        so = run_solver<SOLVER, THERMAL, TIMES, false, false>(m, Jp, Tp, row, a.c, rk, fp, ns, true);
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
                            so = llgs_solve_wave<THERMAL, TIMES>(m, Tp, k, a.c.rtol, a.c.atol, a.c.max_step, a.c.max_attempts, rk, fp, LlgsEnergyK{},
                                                                ns, src, wk);
                        } else {
                            const SimpleK k = load_simple(row);
                            so = simple_solve_wave<SOLVER == STG_SOLVER_EULER ? 1 : 0, THERMAL, TIMES>(
                                m, Tp, k, -row[C_GEFF], row[C_POL], row[C_MSV], row[C_VALID] != 0.0, a.c.temperature, a.c.max_step, rk, fp, ns,
                                a.c.inv_tau, src);
                        }
                    }
                    // a watched phase that failed, by any cause, has not crossed: the rows it passed are discarded
                    if (TIMES) fp.crossed = fp.crossed && so.ok;
                }
                m = so.m;
                failed = !so.ok;
            }
        }
        const double proj = add_x(add_x(mul_x(m.x, tg.x), mul_x(m.y, tg.y)), mul_x(m.z, tg.z));
        const bool switched = active && proj > a.threshold;
        const bool crossed = TIMES && active && fp.crossed;
        n_sw += (unsigned long long)__popcll(__ballot(switched));
        n_fail += (unsigned long long)__popcll(__ballot(active && failed));
        n_cr += (unsigned long long)__popcll(__ballot(crossed));
        n_ret += (unsigned long long)__popcll(__ballot(crossed && !switched));
        if constexpr (VARY) {
            // per-device counts: one atomic for the wavefront where the round's live lanes share a device (wave-uniform test on the
            // round's first and last live trial), one per switched lane where they straddle devices
            const int64_t r_first = (wv * a.L + l) * 64;
            if (xa.v.dev_switched && r_first < a.R) {
                const int64_t r_last = r_first + 63 < a.R ? r_first + 63 : a.R - 1;
                const int64_t d_first = vary_device_of(a.trial0 + r_first, xa.v.Q), d_last = vary_device_of(a.trial0 + r_last, xa.v.Q);
                unsigned long long* cnt = xa.v.dev_switched + (int64_t)g * xa.v.dev_stride;
                const unsigned long long sw = __ballot(switched);
                if (d_first == d_last) {
                    if (lane == 0 && sw) atomicAdd(cnt + d_first, (unsigned long long)__popcll(sw));
                } else if (switched) {
                    atomicAdd(cnt + dev, 1ull);
                }
            }
        }
        if (active && a.n_bins > 0) {
            // min(n_bins - 1, max(0, (int)floor(x))), clamped before the conversion: NaN -> bin 0, +-inf and huge values -> the outer bins
            const double b = floor(mul_x(add_x(proj, 1.0), bin_scale));
            const int bin = b >= 1.0 ? (b < (double)(a.n_bins - 1) ? (int)b : a.n_bins - 1) : 0;
            atomicAdd(&s_hist[bin], 1ull);
        }
        if (TIMES && crossed && n_tbins > 0) {
            const double b = floor(mul_x(fp.t_x, tbin_scale));                     // (clamped before the conversion, as above)
            const int bin = b >= 1.0 ? (b < (double)(n_tbins - 1) ? (int)b : n_tbins - 1) : 0;
            atomicAdd(&s_thist[bin], 1ull);
        }
    }
    __syncthreads();
    if (lane == 0) {
        if (n_sw) atomicAdd(a.n_switched + g, n_sw);
        if (n_fail) atomicAdd(a.n_failed + g, n_fail);
        if (TIMES && n_cr) atomicAdd(x.n_crossed + g, n_cr);
        if (TIMES && n_ret) atomicAdd(x.n_returned + g, n_ret);
    }
    if (lane < a.n_bins) {
        const unsigned long long v = s_hist[lane];
        if (v) atomicAdd(a.hist + (int64_t)g * a.n_bins + lane, v);
    }
    for (int32_t b = lane; TIMES && b < n_tbins; b += 64) {
        const unsigned long long v = s_thist[b];
        if (v) atomicAdd(x.t_hist + (int64_t)g * n_tbins + b, v);
    }
}

// one solver's 8 population kernels (VARY, with MULTI = true); `times`: the caller wants the first-passage counts
template <int SOLVER>
static void dispatch_switch_vary(const SwitchPopArgs& x, bool times, bool thermal, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)x.t.w.s.G * x.t.w.s.waves_per_cond));
    const size_t lds = times ? sizeof(unsigned long long) * (size_t)x.t.n_tbins : 0;
    with_flag(thermal, [&](auto THERMAL) { with_flag(x.t.w.kj > 0 || x.t.w.kh > 0, [&](auto WAVE) { with_flag(times, [&](auto TIMES) {
        hipLaunchKernelGGL((stg_switch_kernel<SOLVER, THERMAL.value, true, WAVE.value, TIMES.value, true>), grid, dim3(64), lds, st, x);
    }); }); });
}

// one solver's 16 kernels; WAVE: a table is there.  `times` is the entry, not the arguments: stg_switch_times with n_tbins = 0 still counts
template <int SOLVER>
static void dispatch_switch(const SwitchTimesArgs& x, bool times, bool thermal, bool multi, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)x.w.s.G * x.w.s.waves_per_cond));
    const size_t lds = times ? sizeof(unsigned long long) * (size_t)x.n_tbins : 0;
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(x.w.kj > 0 || x.w.kh > 0, [&](auto WAVE) {
        with_flag(times, [&](auto TIMES) {
            hipLaunchKernelGGL((stg_switch_kernel<SOLVER, THERMAL.value, MULTI.value, WAVE.value, TIMES.value, false>), grid, dim3(64), lds, st, x);
        });
    }); }); });
}

// defined in stg_switch_rk4.hip / _euler.hip / _rk45.hip: `make -j` compiles the three solvers' kernels in parallel
void stg_dispatch_switch_rk4(const SwitchTimesArgs& x, bool times, bool thermal, bool multi, hipStream_t st);
void stg_dispatch_switch_euler(const SwitchTimesArgs& x, bool times, bool thermal, bool multi, hipStream_t st);
void stg_dispatch_switch_rk45(const SwitchTimesArgs& x, bool times, bool thermal, bool multi, hipStream_t st);

// enqueues the one kernel of a switching entry: x.w.s alone filled in is stg_switch_stats, x.w stg_switch_stats_wave
inline void stg_switch_launch(const SwitchTimesArgs& x, bool times, int solver, bool thermal, bool multi, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: stg_dispatch_switch_rk4(x, times, thermal, multi, st); break;
        case STG_SOLVER_EULER: stg_dispatch_switch_euler(x, times, thermal, multi, st); break;
        default: stg_dispatch_switch_rk45(x, times, thermal, multi, st); break;
    }
}

// the same for stg_switch_population
void stg_dispatch_switch_vary_rk4(const SwitchPopArgs& x, bool times, bool thermal, hipStream_t st);
void stg_dispatch_switch_vary_euler(const SwitchPopArgs& x, bool times, bool thermal, hipStream_t st);
void stg_dispatch_switch_vary_rk45(const SwitchPopArgs& x, bool times, bool thermal, hipStream_t st);
inline void stg_switch_vary_launch(const SwitchPopArgs& x, bool times, int solver, bool thermal, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: stg_dispatch_switch_vary_rk4(x, times, thermal, st); break;
        case STG_SOLVER_EULER: stg_dispatch_switch_vary_euler(x, times, thermal, st); break;
        default: stg_dispatch_switch_vary_rk45(x, times, thermal, st); break;
    }
}
