// stg_switch_stats.hip -- the kernels of stg_switch_stats: Monte-Carlo switching statistics with the trial loop and the reduction on
// chip, (rk4 | euler | rk45) x thermal x class table, fp64.  A translation unit of its own: the step kernels, stg_solve_kernel, the
// waveform and the array kernels are compiled without it.
//
// One 64-lane wavefront per workgroup works on ONE condition g: its m0, phase table, target and class row are wave-uniform (scalar
// loads), and the sub-step count of a fixed-step phase is the same in every lane.  A lane runs L trials one after the other; a trial
// is the chain of the condition's phases, each of them exactly the solve of stg_solve_kernel (run_solver with InlineNormals on the
// stream of problem g * trial_stride + trial at env_step + p).  The counts stay in registers (ballot + popcount) and in LDS (the
// histogram, integer atomics) until the wavefront is through with its trials; then one lane adds each scalar count, and lane b adds
// bin b, to the caller's arrays with 64-bit atomics.  Integer sums: the result does not depend on L, the grid or the arrival order.
#include "stg_switch_stats.hpp"

template <int SOLVER, bool THERMAL, bool MULTI>
__global__ void __launch_bounds__(64) stg_switch_stats_kernel(const SwitchStatsArgs a) {
    static_assert(STG_MAX_BINS == 64, "lane b owns bin b");
    __shared__ unsigned long long s_hist[STG_MAX_BINS];
    const int lane = (int)threadIdx.x;
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)a.waves_per_cond);
    const int64_t w = (int64_t)(blockIdx.x % (uint32_t)a.waves_per_cond);
    const int32_t G = a.G;
    s_hist[lane] = 0ull;
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
    unsigned long long n_sw = 0ull, n_fail = 0ull;                                 // wave-uniform
    for (int64_t l = 0; l < a.L; ++l) {
        const int64_t r = (w * a.L + l) * 64 + lane;                               // this lane's trial, counted from trial0
        const bool active = r < a.R;
        V3 m = m0;
        bool failed = false;
        if (active) {
            InlineNormals ns;
#pragma clang loop unroll(disable)
            for (int32_t p = 0; p < a.P && !failed; ++p) {
                const double Jp = a.J[(int64_t)p * G + g], Tp = a.T[(int64_t)p * G + g];
                if (Tp == 0.0) continue;
                const RngKey rk{a.c.seed, (uint64_t)(id0 + r), a.env_step + (uint32_t)p};
                const SolveOut so = run_solver<SOLVER, THERMAL, false, false, false>(m, Jp, Tp, row, a.c, rk, norec, ns, true);
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
static void dispatch_switch_stats(const SwitchStatsArgs& a, bool thermal, bool multi, hipStream_t st) {
    const dim3 grid((unsigned)((int64_t)a.G * a.waves_per_cond));
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) {
        hipLaunchKernelGGL((stg_switch_stats_kernel<SOLVER, THERMAL.value, MULTI.value>), grid, dim3(64), 0, st, a);
    }); });
}

void stg_switch_stats_launch(const SwitchStatsArgs& a, int solver, bool thermal, bool multi, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_switch_stats<STG_SOLVER_RK4>(a, thermal, multi, st); break;
        case STG_SOLVER_EULER: dispatch_switch_stats<STG_SOLVER_EULER>(a, thermal, multi, st); break;
        default: dispatch_switch_stats<STG_SOLVER_RK45>(a, thermal, multi, st); break;
    }
}
