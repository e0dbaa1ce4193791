// stg_solve_wave.hip -- the kernels of stg_solve_wave: RobustLLGSSolver.solve / LLGSSolver.solve with piecewise-linear
// current_func(t) and field_func(t) (stg_wave.hpp), (rk4 | euler | rk45) x thermal x record, fp64, one problem per lane.
// A translation unit of its own: the step kernels, stg_solve_kernel and the array kernels are compiled without it.
#include "stg_wave.hpp"

template <int SOLVER, bool THERMAL, bool MULTI, bool RECORD>
__global__ void __launch_bounds__(64) stg_solve_wave_kernel(const WaveSolveArgs w) {
    __shared__ double s_tab[MULTI ? STG_MAX_CLASSES * C_COUNT : 1];
    const SolveArgs& a = w.s;
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool in_range = i < a.N;
    const double* row = class_row<MULTI>(a.ctab, a.cls, a.ncls, i, in_range, s_tab, EnvParams{});
    if (!in_range) return;
    const int64_t N = a.N;
    const V3 m0{a.m0[i], a.m0[N + i], a.m0[2 * N + i]};
    const double T = a.T[i];
    WaveSource src;
    src.has_j = w.kj > 0; src.has_h = w.kh > 0;
    src.J = src.has_j ? 0.0 : a.J[i];
    src.T = T;
    src.cj.tk = w.tj; src.cj.vk = w.jk; src.cj.N = N; src.cj.i = i; src.cj.K = w.kj; src.cj.k = 0;
    src.ch.tk = w.th; src.ch.vk = w.hk; src.ch.N = N; src.ch.i = i; src.ch.K = w.kh; src.ch.k = 0;
    // a table that is not finite or not strictly increasing fails its lane like a rejected input: m_final = m0, no rows
    const bool tables_ok = (!src.has_j || src.cj.valid()) && (!src.has_h || src.ch.valid());
    if (!tables_ok) {
        a.m_final[i] = m0.x; a.m_final[N + i] = m0.y; a.m_final[2 * N + i] = m0.z;
        if (a.n_points) a.n_points[i] = 0;
        if (a.success) a.success[i] = 0;
        return;
    }
    if (src.has_j) src.cj.open();
    if (src.has_h) src.ch.open();
    src.arm();
    const RngKey rk{a.c.seed, (uint64_t)(a.env_id0 + i), a.env_step};
    const Recorder rec{a.traj_t, a.traj_m, a.traj_e, a.traj_tq, N, i, a.traj_cap};
    InlineNormals ns;
    SolveOut so;
    if (SOLVER == STG_SOLVER_RK45) {
        const LlgsK k = load_llgs(row);
        LlgsEnergyK ek{};
        if (RECORD) ek = load_energy(row);
        const double beta = row[C_BETA], betap = row[C_BETAP];
        const bool useJ = !(fabs(src.J) < 1e-12);                           // llgs_solver.py:222
        const LlgsWaveK wk{beta, betap, -row[C_GAMMA], useJ ? beta * src.J : 0.0, useJ ? betap * src.J : 0.0,
                           (4 * 3.14159265358979323846 * 1e-7) * row[C_MSV]};
        so = llgs_solve_wave<THERMAL, RECORD>(m0, T, k, a.c.rtol, a.c.atol, a.c.max_step, a.c.max_attempts, rk, rec, ek, ns, src, wk);
    } else {
        const SimpleK k = load_simple(row);
        so = simple_solve_wave<SOLVER == STG_SOLVER_EULER ? 1 : 0, THERMAL, RECORD>(
            m0, T, k, -row[C_GEFF], row[C_POL], row[C_MSV], row[C_VALID] != 0.0, a.c.temperature, a.c.max_step, rk, rec, ns, a.c.inv_tau, src);
    }
    a.m_final[i] = so.m.x; a.m_final[N + i] = so.m.y; a.m_final[2 * N + i] = so.m.z;
    if (a.n_points) a.n_points[i] = so.n;
    if (a.success) a.success[i] = so.ok ? 1 : 0;
}

template <int SOLVER>
static void dispatch_wave(const WaveSolveArgs& a, bool thermal, bool multi, bool record, hipStream_t st) {
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(record, [&](auto RECORD) {
        hipLaunchKernelGGL((stg_solve_wave_kernel<SOLVER, THERMAL.value, MULTI.value, RECORD.value>), dim3((unsigned)((a.s.N + 63) / 64)),
                           dim3(64), 0, st, a);
    }); }); });
}

void stg_wave_launch(const WaveSolveArgs& a, int solver, bool thermal, bool multi, bool record, hipStream_t st) {
    switch (solver) {
        case STG_SOLVER_RK4: dispatch_wave<STG_SOLVER_RK4>(a, thermal, multi, record, st); break;
        case STG_SOLVER_EULER: dispatch_wave<STG_SOLVER_EULER>(a, thermal, multi, record, st); break;
        default: dispatch_wave<STG_SOLVER_RK45>(a, thermal, multi, record, st); break;
    }
}
