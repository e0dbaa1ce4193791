// stg_switch_verify.hpp -- write - verify - write switching statistics: the argument block and the kernel of stg_switch_verify
// (C-ABI: spintorque_hip.hip), (rk4 | euler | rk45) x thermal x class table, fp64, and below it its sibling for a population of varied
// devices, stg_switch_verify_population, (rk4 | euler | rk45) x thermal.  Both kernels are instantiated per solver in
// stg_switch_verify_rk4.hip / _euler.hip / _rk45.hip and nowhere else.
//
// A trial is up to A attempts of P rectangular phases each; after every attempt it is classified, and only a trial that has not
// switched runs the next attempt, from the m the attempt before left behind.  The trial kernel of stg_switch.hpp marches its lanes in
// lockstep rounds, one trial per lane per round: with a verify in that loop a wavefront whose first attempt succeeds in 99 % of its
// lanes would run the second attempt with one lane in a hundred alive.  Here every lane walks ONE flattened loop over its own
// (trial, attempt, phase) sequence instead.  An iteration is one solve -- one call of run_solver, the only call site -- of whatever
// phase the lane is at; a lane whose trial ends starts its next trial in the next iteration, so the lanes of a wavefront are at
// different trials and attempts but execute the same solver code, and the wavefront stays full until its lanes run out of trials.
//   Trials   lane l of wavefront w of a condition takes trials w * 64 + l + k * 64 * W, k = 0, 1, ... (W = waves_per_cond): a static
//            stride, no queue, no memory.  The wavefront leaves the loop when every lane's list is exhausted.
//   State    trial, attempt, phase and m are carried in registers; the condition's J and T tables (A * P <= 32 doubles each) are staged
//            in LDS once per wavefront, because the lanes index them differently.
//   Counts   lanes are not aligned on trial boundaries, so nothing is reduced by ballots per round: a lane that ends a trial adds to
//            LDS counters [A] (integer atomics) and to the LDS histogram.  When the wavefront is through, lane a adds the counts of
//            attempt a, lane 0 the failures and lane b bin b to the caller's arrays, one 64-bit atomic per non-zero counter.  Integer
//            sums: the result does not depend on W or the arrival order.
//   A skipped phase (T == 0.0 exactly) costs its lane one idle iteration; the other lanes solve meanwhile.
#pragma once
#include "stg_switch.hpp"

static_assert(STG_MAX_VERIFY_ATTEMPTS * STG_MAX_PHASES <= 64, "lane j stages table entry j");

struct SwitchVerifyArgs {
    SwitchStatsArgs s;                 // as stg_switch_stats, with J, T [A][P][G], n_switched = n_switched_at [A][G], waves_per_cond = W; L is not read
    int32_t A;                         // attempts, 1 ... STG_MAX_VERIFY_ATTEMPTS
    unsigned long long* n_ended_at;    // [A][G]: added to
};

template <int SOLVER, bool THERMAL, bool MULTI>
__global__ void __launch_bounds__(64) stg_switch_verify_kernel(const SwitchVerifyArgs x) {
    static_assert(STG_MAX_BINS == 64, "lane b owns bin b");
    constexpr int NPH = STG_MAX_VERIFY_ATTEMPTS * STG_MAX_PHASES;
    __shared__ unsigned long long s_hist[STG_MAX_BINS];
    __shared__ unsigned long long s_ended[STG_MAX_VERIFY_ATTEMPTS], s_sw[STG_MAX_VERIFY_ATTEMPTS], s_fail;
    __shared__ double s_J[NPH], s_T[NPH];
    const SwitchStatsArgs& a = x.s;
    const int lane = (int)threadIdx.x;
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)a.waves_per_cond);
    const int64_t wv = (int64_t)(blockIdx.x % (uint32_t)a.waves_per_cond);
    const int32_t G = a.G, A = x.A, P = a.P;
    s_hist[lane] = 0ull;
    if (lane < STG_MAX_VERIFY_ATTEMPTS) {
        s_ended[lane] = 0ull;
        s_sw[lane] = 0ull;
    }
    if (lane == 0) s_fail = 0ull;
    if (lane < NPH) {
        // condition g's column of the tables -> LDS (lane j: entry j = a * P + p)
        const bool in = lane < A * P;
        s_J[lane] = in ? a.J[(int64_t)lane * G + g] : 0.0;
        s_T[lane] = in ? a.T[(int64_t)lane * G + g] : 0.0;
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
    const int64_t stride = 64 * (int64_t)a.waves_per_cond;
    // the lane's place in its list: trial r (counted from trial0), attempt at, phase ph of it, and the m that phase starts from
    int64_t r = wv * 64 + lane;
    int32_t at = 0, ph = 0;
    V3 m = m0;
    bool live = r < a.R;
    while (__ballot(live) != 0ull) {
        const int32_t k = at * P + ph;                                             // (< A * P also in a lane that is through)
        const double Tp = s_T[k], Jp = s_J[k];
        const bool runs = live && Tp != 0.0;                                       // T == 0.0 exactly: skipped, m passes through
        bool failed = false;
        if (runs) {
            InlineNormals ns;
            const RngKey rk{a.c.seed, (uint64_t)(id0 + r), a.env_step + (uint32_t)k};
            const SolveOut so = run_solver<SOLVER, THERMAL, false, false, false>(m, Jp, Tp, row, a.c, rk, norec, ns, true);
            m = so.m;
            failed = !so.ok;
        }
        if (live) {
            if (ph + 1 < P && !failed) {
                ++ph;
            } else {
                // the attempt is over (a failed phase ends it): verify
                const double proj = add_x(add_x(mul_x(m.x, tg.x), mul_x(m.y, tg.y)), mul_x(m.z, tg.z));
                const bool switched = proj > a.threshold;
                if (failed) atomicAdd(&s_fail, 1ull);
                if (switched || failed || at + 1 >= A) {
                    // the trial ends at this attempt; the lane's next trial starts in the next iteration
                    atomicAdd(&s_ended[at], 1ull);
                    if (switched) atomicAdd(&s_sw[at], 1ull);
                    if (a.n_bins > 0) {
                        // min(n_bins - 1, max(0, (int)floor(x))), clamped before the conversion: NaN -> bin 0, +-inf and huge values -> the outer bins
                        const double b = floor(mul_x(add_x(proj, 1.0), bin_scale));
                        const int bin = b >= 1.0 ? (b < (double)(a.n_bins - 1) ? (int)b : a.n_bins - 1) : 0;
                        atomicAdd(&s_hist[bin], 1ull);
                    }
                    r += stride;
                    live = r < a.R;
                    at = 0;
                    m = m0;
                } else {
                    ++at;
                }
                ph = 0;
            }
        }
    }
    __syncthreads();
    if (lane < A) {
        const unsigned long long e = s_ended[lane], s = s_sw[lane];
        if (e) atomicAdd(x.n_ended_at + (int64_t)lane * G + g, e);
        if (s) atomicAdd(a.n_switched + (int64_t)lane * G + g, s);
    }
    if (lane == 0) {
        const unsigned long long f = s_fail;
        if (f) atomicAdd(a.n_failed + g, f);
    }
    if (lane < a.n_bins) {
        const unsigned long long v = s_hist[lane];
        if (v) atomicAdd(a.hist + (int64_t)g * a.n_bins + lane, v);
    }
}

// stg_switch_verify_population: the flattened loop above with every trial on the row of its own device (stg_vary.hpp: the rule;
// stg_switch.hpp, VARY: the lockstep sibling).  A sibling of the kernel above, not a flag of it: that one stays as it is.
struct SwitchVerifyPopArgs {
    SwitchVerifyArgs y;                // as stg_switch_verify
    SwitchVaryArgs v;                  // as stg_switch_population, with dev_switched = dev_switched_at [A][G][dev_stride]
};

// What is new against stg_switch_verify_kernel: a lane that STARTS a trial (attempt 0, phase 0 of it) forms the trial's device, and
// where that is not the device its row was derived for, draws it (vary_draw) and derives its row (derive_row) into own_row, which
// run_solver -- still one call site -- reads in the place of the wave-uniform class row.  The draw is kept while the lane's next trial
// is the same device's (always, once Q >= 2 * 64 * W).  A lane that ends a trial switched adds one to its device's counter of that
// attempt: one 64-bit integer atomic per switched trial, so the counts depend neither on W nor on the arrival order.  A bad sigma
// column (wave-uniform) fails the first phase of a trial that is not skipped, before any draw.  As under VARY the class table only
// selects the nominal record, so there is no MULTI: cond_cls may be NULL.
template <int SOLVER, bool THERMAL>
__global__ void __launch_bounds__(64) stg_switch_verify_population_kernel(const SwitchVerifyPopArgs xa) {
    static_assert(STG_MAX_BINS == 64, "lane b owns bin b");
    constexpr int NPH = STG_MAX_VERIFY_ATTEMPTS * STG_MAX_PHASES;
    __shared__ unsigned long long s_hist[STG_MAX_BINS];
    __shared__ unsigned long long s_ended[STG_MAX_VERIFY_ATTEMPTS], s_sw[STG_MAX_VERIFY_ATTEMPTS], s_fail;
    __shared__ double s_J[NPH], s_T[NPH];
    const SwitchVerifyArgs& x = xa.y;
    const SwitchStatsArgs& a = x.s;
    const int lane = (int)threadIdx.x;
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)a.waves_per_cond);
    const int64_t wv = (int64_t)(blockIdx.x % (uint32_t)a.waves_per_cond);
    const int32_t G = a.G, A = x.A, P = a.P;
    s_hist[lane] = 0ull;
    if (lane < STG_MAX_VERIFY_ATTEMPTS) {
        s_ended[lane] = 0ull;
        s_sw[lane] = 0ull;
    }
    if (lane == 0) s_fail = 0ull;
    if (lane < NPH) {
        // condition g's column of the tables -> LDS (lane j: entry j = a * P + p)
        const bool in = lane < A * P;
        s_J[lane] = in ? a.J[(int64_t)lane * G + g] : 0.0;
        s_T[lane] = in ? a.T[(int64_t)lane * G + g] : 0.0;
    }
    __syncthreads();
    const int c = a.cond_cls ? (int)a.cond_cls[g] : 0;
    const int nominal_cls = c < a.ncls ? c : 0;                                    // the condition's nominal record
    // the lane's own row of derived constants (constant indices only: the array dissolves into registers), the device it holds, and
    // whether the condition's sigma column is valid (wave-uniform)
    double own_row[C_COUNT];
    int64_t own_dev = -1;
    const bool sigma_ok = vary_column_ok(xa.v.sigma, G, g, xa.v.z_clip);
    const V3 m0{a.m0[g], a.m0[G + g], a.m0[2 * G + g]};
    const V3 tg{a.target[g], a.target[G + g], a.target[2 * G + g]};
    const Recorder norec{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    const int64_t id0 = a.env_id0 + (int64_t)g * a.trial_stride + a.trial0;       // env id of the condition's trial trial0
    const double bin_scale = mul_x(0.5, (double)a.n_bins);
    const int64_t stride = 64 * (int64_t)a.waves_per_cond;
    int64_t r = wv * 64 + lane;
    int32_t at = 0, ph = 0;
    V3 m = m0;
    bool live = r < a.R;
    while (__ballot(live) != 0ull) {
        const int32_t k = at * P + ph;                                             // (< A * P also in a lane that is through)
        const double Tp = s_T[k], Jp = s_J[k];
        if (live && k == 0) {
            // the trial starts: its device; a new one gets its record from its own stream and its row by the arithmetic of a class table row
            const int64_t dev = vary_device_of(a.trial0 + r, xa.v.Q);
            if (dev != own_dev) {
                if (sigma_ok) {
                    const int64_t dev_env = vary_device_env(a.env_id0, g, a.trial_stride, dev, xa.v.Q);
                    double z[6];
                    stg_device_params dp;
                    vary_draw(a.c.seed, (uint64_t)dev_env, xa.v.var_step, xa.v.ptab[nominal_cls], xa.v.sigma, G, g, xa.v.z_clip, z, dp);
                    derive_row(dp, xa.v.gamma, a.c.temperature, own_row);
                }
                own_dev = dev;
            }
        }
        const bool runs = live && Tp != 0.0;                                       // T == 0.0 exactly: skipped, m passes through
        bool failed = runs && !sigma_ok;                                           // a bad sigma column: the first phase that would run fails
        if (runs && sigma_ok) {
            InlineNormals ns;
            const RngKey rk{a.c.seed, (uint64_t)(id0 + r), a.env_step + (uint32_t)k};
            const SolveOut so = run_solver<SOLVER, THERMAL, false, false, false>(m, Jp, Tp, own_row, a.c, rk, norec, ns, true);
            m = so.m;
            failed = !so.ok;
        }
        if (live) {
            if (ph + 1 < P && !failed) {
                ++ph;
            } else {
                // the attempt is over (a failed phase ends it): verify
                const double proj = add_x(add_x(mul_x(m.x, tg.x), mul_x(m.y, tg.y)), mul_x(m.z, tg.z));
                const bool switched = proj > a.threshold;
                if (failed) atomicAdd(&s_fail, 1ull);
                if (switched || failed || at + 1 >= A) {
                    // the trial ends at this attempt; the lane's next trial starts in the next iteration
                    atomicAdd(&s_ended[at], 1ull);
                    if (switched) {
                        atomicAdd(&s_sw[at], 1ull);
                        if (xa.v.dev_switched) atomicAdd(xa.v.dev_switched + ((int64_t)at * G + g) * xa.v.dev_stride + own_dev, 1ull);
                    }
                    if (a.n_bins > 0) {
                        // min(n_bins - 1, max(0, (int)floor(x))), clamped before the conversion: NaN -> bin 0, +-inf and huge values -> the outer bins
                        const double b = floor(mul_x(add_x(proj, 1.0), bin_scale));
                        const int bin = b >= 1.0 ? (b < (double)(a.n_bins - 1) ? (int)b : a.n_bins - 1) : 0;
                        atomicAdd(&s_hist[bin], 1ull);
                    }
                    r += stride;
                    live = r < a.R;
                    at = 0;
                    m = m0;
                } else {
                    ++at;
                }
                ph = 0;
            }
        }
    }
    __syncthreads();
    if (lane < A) {
        const unsigned long long e = s_ended[lane], s = s_sw[lane];
        if (e) atomicAdd(x.n_ended_at + (int64_t)lane * G + g, e);
        if (s) atomicAdd(a.n_switched + (int64_t)lane * G + g, s);
    }
    if (lane == 0) {
        const unsigned long long f = s_fail;
        if (f) atomicAdd(a.n_failed + g, f);
    }
    if (lane < a.n_bins) {
        const unsigned long long v = s_hist[lane];
        if (v) atomicAdd(a.hist + (int64_t)g * a.n_bins + lane, v);
    }
}

// one solver's 2 population kernels
template <int SOLVER>
static void dispatch_switch_verify_population(const SwitchVerifyPopArgs& x, bool thermal, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)x.y.s.G * x.y.s.waves_per_cond));
    with_flag(thermal, [&](auto THERMAL) {
        hipLaunchKernelGGL((stg_switch_verify_population_kernel<SOLVER, THERMAL.value>), grid, dim3(64), 0, st, x);
    });
}

// one solver's 4 kernels
template <int SOLVER>
static void dispatch_switch_verify(const SwitchVerifyArgs& x, bool thermal, bool multi, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)x.s.G * x.s.waves_per_cond));
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) {
        hipLaunchKernelGGL((stg_switch_verify_kernel<SOLVER, THERMAL.value, MULTI.value>), grid, dim3(64), 0, st, x);
    }); });
}

// defined in stg_switch_verify_rk4.hip / _euler.hip / _rk45.hip
void stg_dispatch_switch_verify_rk4(const SwitchVerifyArgs& x, bool thermal, bool multi, hipStream_t st);
void stg_dispatch_switch_verify_euler(const SwitchVerifyArgs& x, bool thermal, bool multi, hipStream_t st);
void stg_dispatch_switch_verify_rk45(const SwitchVerifyArgs& x, bool thermal, bool multi, hipStream_t st);

// enqueues the one kernel of stg_switch_verify; false: no kernel for this solver (the entry reports it)
inline bool stg_switch_verify_launch(const SwitchVerifyArgs& x, int solver, bool thermal, bool multi, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: stg_dispatch_switch_verify_rk4(x, thermal, multi, st); return true;
        case STG_SOLVER_EULER: stg_dispatch_switch_verify_euler(x, thermal, multi, st); return true;
        case STG_SOLVER_RK45: stg_dispatch_switch_verify_rk45(x, thermal, multi, st); return true;
        default: return false;
    }
}

// the same for stg_switch_verify_population
void stg_dispatch_switch_verify_population_rk4(const SwitchVerifyPopArgs& x, bool thermal, hipStream_t st);
void stg_dispatch_switch_verify_population_euler(const SwitchVerifyPopArgs& x, bool thermal, hipStream_t st);
void stg_dispatch_switch_verify_population_rk45(const SwitchVerifyPopArgs& x, bool thermal, hipStream_t st);
inline bool stg_switch_verify_population_launch(const SwitchVerifyPopArgs& x, int solver, bool thermal, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: stg_dispatch_switch_verify_population_rk4(x, thermal, st); return true;
        case STG_SOLVER_EULER: stg_dispatch_switch_verify_population_euler(x, thermal, st); return true;
        case STG_SOLVER_RK45: stg_dispatch_switch_verify_population_rk45(x, thermal, st); return true;
        default: return false;
    }
}
