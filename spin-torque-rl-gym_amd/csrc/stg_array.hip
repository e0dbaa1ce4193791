// stg_array.hip -- SpinTorqueArray-v0 step path: N independent R x C device arrays per launch.
//
// Reference: spin_torque_gym/envs/array_env.py -- step :362-409, _apply_action :411-476, _compute_effective_field :478-494,
// _simulate_device_dynamics :496-521, _compute_pattern_similarity :523-531, _get_observation :533-569,
// default reward :183-224, coupling matrix :301-334.
//
// Unlike SpinTorque-v0 this env is memory-shaped: a step touches every device's magnetisation (coupling sum, similarity,
// observation) but integrates only the addressed devices with ten Euler sub-steps of ONE derivative -- ~1 KB of HBM
// traffic per array-step against a few hundred flops in 'individual' mode.  Layout: one array per lane; the array's
// pattern lives in LDS for the duration of the step (lane-fastest: [device*3+component][64 lanes], conflict-free
// ds_read_b64), because the addressed devices update sequentially and each sees its predecessors' new states (the
// reference updates current_pattern in place).  Global state is SoA [device][component][N] so every wavefront access is
// a coalesced 512-B row.
#include "../../include/spintorque_hip.h"
#include "stg_physics.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

using namespace stg;

namespace {

constexpr int ARR_MAX_DEV = 64;

struct ArrDev {            // per-class constants of the (single) device class of the array
    double hk, ms;
    double ex, ey, ez;     // raw easy axis
    double nx, ny, nz;     // shape demag factors (SOT/VCMA)
    double area, r_p, r_ap, tmr, refx, refy, refz, r_series;
    int32_t dev_type;
};

struct ArrArgs {
    int64_t N;
    int32_t rows, cols, mode, include_coupling, max_steps, obs_mode;
    double max_current, max_duration, thr, w_energy, temperature;
    ArrDev dev;
    const double* coupling;        // [n][n] device memory
    double *pattern, *target;      // [n][3][N]
    double* etot;                  // [N]
    int32_t* step;                 // [N]
    const float* actions;          // [A][N]
    float* obs;                    // [obs_dim][N]
    float* reward;
    double *reward64, *energy;
    uint8_t *term, *trunc;
};

// device.compute_effective_field(m, 0): stt_mram.py:55-76 (re-normalised m, anisotropy only); sot_mram.py:79-112 and
// vcma_mram.py:85-120 (raw m, anisotropy + shape demagnetisation; thermal/DMI/exchange terms are zero there)
__device__ __forceinline__ V3 device_field(const V3& m_in, const ArrDev& d) {
    if (d.dev_type == STG_DEV_STT) {
        const double inv = rsqrt_fast(dot(m_in, m_in));
        const V3 m{m_in.x * inv, m_in.y * inv, m_in.z * inv};
        const double c = d.hk * (m.x * d.ex + m.y * d.ey + m.z * d.ez);
        return V3{c * d.ex, c * d.ey, c * d.ez};
    }
    const double c = d.hk * (m_in.x * d.ex + m_in.y * d.ey + m_in.z * d.ez);
    return V3{c * d.ex - d.ms * d.nx * m_in.x, c * d.ey - d.ms * d.ny * m_in.y, c * d.ez - d.ms * d.nz * m_in.z};
}

// device.compute_resistance(m) as the array env's energy term sees it (stt_mram.py:78-94, sot_mram.py:196-228, vcma_mram.py:236-257):
// stg::resistance with Python's max(r, floor) in place of fmax -- r unless floor > r, so the NaN of a cell that a NaN duration (or a NaN
// neighbour, through the coupling sum) has spoilt reaches the energy as it does in the reference instead of turning into the floor value.
// Same operations in the same order otherwise: identical for every other input.
__device__ __forceinline__ double cell_resistance(const V3& m_in, const ArrDev& d) {
#pragma clang fp contract(off)
    const V3 ref{d.refx, d.refy, d.refz};
    if (d.dev_type == STG_DEV_STT) {
        const double inv = rsqrt_fast(dot(m_in, m_in));
        const V3 m{m_in.x * inv, m_in.y * inv, m_in.z * inv};
        const double r = d.r_p * (1.0 + d.tmr * (1.0 - dot(m, ref)) * 0.5);
        return d.r_p * 0.5 > r ? d.r_p * 0.5 : r;
    }
    double r = d.r_p + (d.r_ap - d.r_p) * (1.0 - dot(m_in, ref)) * 0.5;
    if (d.dev_type == STG_DEV_SOT) r = r + d.r_series;
    return 1.0 > r ? 1.0 : r;
}

// Observation rows: 'array' mode [R,C,6] = (pattern, target) per cell; 'vector' mode = flattened pattern, flattened
// target, then 4 global values (array_env.py:533-557).
__device__ __forceinline__ int64_t obs_row_pattern(int obs_mode, int n, int d, int k) { return obs_mode == 0 ? d * 6 + k : d * 3 + k; }
__device__ __forceinline__ int64_t obs_row_target(int obs_mode, int n, int d, int k) { return obs_mode == 0 ? d * 6 + 3 + k : 3 * n + d * 3 + k; }

// ---- pieces of one step that every kernel shares, each stated once ------------------------------------------------------------------
// Pure on values except the two that store; none holds a barrier or forms an address from a cell index.  Only uses that leave a kernel's
// machine code as it was are taken (profiles/array_pieces_isa.txt): the action decode, the LDS coupling sum, the reset's draw and the
// general kernel's dynamics block stay written out where they are, because sharing them changed the compiled kernels.

// the four global values behind the pattern and target rows of a 'vector' observation (array_env.py:547-557): value K goes to row 6 n + K
template <int K>
__device__ __forceinline__ float vector_value(int32_t max_steps, double temperature, double sim, int32_t step, double etot) {
    if (K == 0) return (float)sim;
    if (K == 1) return (float)((double)(max_steps - step) / (double)max_steps);
    if (K == 2) return (float)(etot / 1e-12);
    return (float)(temperature / 300.0);
}
__device__ __forceinline__ void vector_rows(const ArrArgs& a, float* dst, int n, int64_t i, double sim, int32_t step, double etot) {
    const int64_t N = a.N;
    dst[(int64_t)(6 * n + 0) * N + i] = vector_value<0>(a.max_steps, a.temperature, sim, step, etot);
    dst[(int64_t)(6 * n + 1) * N + i] = vector_value<1>(a.max_steps, a.temperature, sim, step, etot);
    dst[(int64_t)(6 * n + 2) * N + i] = vector_value<2>(a.max_steps, a.temperature, sim, step, etot);
    dst[(int64_t)(6 * n + 3) * N + i] = vector_value<3>(a.max_steps, a.temperature, sim, step, etot);
}

// _simulate_device_dynamics (array_env.py:496-521): alpha = 0.01, gamma = 2.21e5, p_hat = z; ONE derivative at m0 in the field h, then ten
// normalised Euler sub-steps of it
__device__ __forceinline__ V3 euler_cell(const V3& m0, const V3& h, double J, double T) {
    const V3 mxp{m0.y, -m0.x, 0.0};
    const V3 t2 = cross(m0, mxp);
    const double tj = 0.1 * J;
    const V3 mxh = cross(m0, h);
    V3 dm{-2.21e5 * mxh.x, -2.21e5 * mxh.y, -2.21e5 * mxh.z};
    const V3 mxdm = cross(m0, dm);
    dm = V3{dm.x + 0.01 * mxdm.x + tj * t2.x, dm.y + 0.01 * mxdm.y + tj * t2.y, dm.z + 0.01 * mxdm.z + tj * t2.z};
    const double dt = T / 10;
    V3 m = m0;
#pragma unroll
    for (int it = 0; it < 10; ++it) {
        m = V3{m.x + dm.x * dt, m.y + dm.y * dt, m.z + dm.z * dt};
        const double inv = rsqrt_fast(dot(m, m));               // m / |m| (array_env.py:518), <= 2 ulp per component
        m = V3{m.x * inv, m.y * inv, m.z * inv};
    }
    return m;
}

// a driven cell's energy, with the resistance of the UPDATED state m (current_m is a view of the pattern, array_env.py:455-463)
__device__ __forceinline__ double cell_energy(const V3& m, double J, double T, const ArrDev& dev) {
    const double r = cell_resistance(m, dev);
    const double v = J * r * dev.area;
    return (v * v) / r * T;
}

// default reward (array_env.py:183-224): pattern match, energy (sign as written), progress, uniformity
__device__ __forceinline__ double default_reward(double sim, double prev_sim, bool is_success, double e_total, double uniformity, double w_energy) {
    double reward = 10.0 * (is_success ? 10.0 : sim * 5.0);
    reward += (-w_energy) * (-e_total / 1e-12);
    reward += (sim - prev_sim);
    reward += 2.0 * uniformity;
    return reward;
}

// the per-array outputs of one step, at element o of each
__device__ __forceinline__ void write_step_outputs(const ArrArgs& a, int64_t o, double reward, double e_total, bool is_success, bool truncated) {
    a.reward[o] = (float)reward;
    if (a.reward64) a.reward64[o] = reward;
    if (a.energy) a.energy[o] = e_total;
    a.term[o] = is_success ? 1 : 0;
    a.trunc[o] = truncated ? 1 : 0;
}

// NDEV > 0: the number of cells is a compile-time constant and the coupling sum unrolls (4 x 4, the registered
// SpinTorqueArray-v0: 'global' mode 0.178 -> 0.167 ms per launch at 262 144 arrays, 'row' / 'column' unchanged).
// (Round 3, measured and rejected: a software-pipelined sweep that forms the coupling sum of the NEXT addressed cell -- all
// terms but the current cell's -- before the current cell's ten dependent Euler sub-steps and adds that one term afterwards:
// 0.169-0.172 ms against 0.167-0.168 ms for the plain unrolled form; the launch is not bound by that dependency chain.)
template <int NDEV>
__global__ void __launch_bounds__(64) stg_array_step_kernel(const ArrArgs a) {
    extern __shared__ double lds[];           // pattern [n*3][64] then coupling [n*n]
    const int n = NDEV > 0 ? NDEV : a.rows * a.cols;
    double* lp = lds;
    double* lc = lds + (size_t)n * 3 * 64;
    const int lane = threadIdx.x;
    if (a.include_coupling) {
        for (int q = lane; q < n * n; q += 64) lc[q] = a.coupling[q];
    }
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool in_range = i < a.N;
    const int64_t N = a.N;
    // The similarity is a running sum, formed here and corrected by each updated cell's change; the fused kernel forms it from scratch
    // every step instead.  The two differ at rounding level and each is pinned by its tests: behaviour, not duplication.
    // ONE pass over the state: pattern -> LDS, target -> its observation rows, and the similarity sum on the fly
    // (np.mean of the per-cell dot products, array_env.py:523-531); the target is not touched again except for the
    // addressed cells.
    double sim_sum = 0.0;
    if (in_range) {
        for (int d = 0; d < n; ++d) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double pv = a.pattern[(int64_t)(d * 3 + k) * N + i];
                const double tv = a.target[(int64_t)(d * 3 + k) * N + i];
                lp[(d * 3 + k) * 64 + lane] = pv;
                a.obs[obs_row_target(a.obs_mode, n, d, k) * N + i] = (float)tv;
                sim_sum += pv * tv;
            }
        }
    }
    __syncthreads();
    if (!in_range) return;
    const double prev_sim = sim_sum / n;                                               // array_env.py:372-373
    // _apply_action (array_env.py:411-445).  In 'global' mode the action is [current, duration]: action[1] (the
    // duration) is what the reference reads as the current density, and the duration defaults to 1 ns -- kept as is.
    const int n_act = a.mode == 3 ? 2 : 3;
    double J = (double)a.actions[N + i];
    double T = n_act > 2 ? (double)a.actions[2 * N + i] : 1e-9;
    J = isnan(J) ? J : fmin(fmax(J, -a.max_current), a.max_current);
    T = isnan(T) ? T : fmin(fmax(T, 1e-12), a.max_duration);
    int first = 0, count = n, stride = 1;
    if (a.mode != 3) {
        const double lim = a.mode == 0 ? n - 1 : (a.mode == 1 ? a.rows - 1 : a.cols - 1);
        const double a0 = (double)a.actions[i];
        // int(np.clip(action[0], 0, lim)); a NaN index raises in the reference -- here it addresses nothing
        const int idx = isnan(a0) ? -1 : (int)fmin(fmax(a0, 0.0), lim);
        if (a.mode == 0) { first = idx; count = 1; stride = 1; }
        else if (a.mode == 1) { first = idx * a.cols; count = a.cols; stride = 1; }
        else { first = idx; count = a.rows; stride = a.cols; }
        if (idx < 0) count = 0;
    }
    const bool drive = fabs(J) > 1e-12;                                                // array_env.py:506
    double e_total = 0.0;
    if (drive) {
        // The addressed cells update sequentially and each sees its predecessors' new states through the coupling sum
        // (the reference updates current_pattern in place, array_env.py:447-476).
#pragma unroll 1
        for (int q = 0; q < count; ++q) {
            const int d = first + q * stride;
            const V3 m0{lp[(d * 3) * 64 + lane], lp[(d * 3 + 1) * 64 + lane], lp[(d * 3 + 2) * 64 + lane]};
            V3 h = device_field(m0, a.dev);
            if (a.include_coupling) {                                                  // array_env.py:485-492
                V3 hc{0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < (NDEV > 0 ? NDEV : n); ++j) {
                    const double c = (j == d) ? 0.0 : lc[d * n + j];
                    hc = V3{hc.x + c * lp[(j * 3) * 64 + lane], hc.y + c * lp[(j * 3 + 1) * 64 + lane],
                            hc.z + c * lp[(j * 3 + 2) * 64 + lane]};
                }
                h = V3{h.x + hc.x, h.y + hc.y, h.z + hc.z};
            }
            // euler_cell, written out: as a call it compiled with one multiply's operands swapped in the similarity update below
            const V3 mxp{m0.y, -m0.x, 0.0};
            const V3 t2 = cross(m0, mxp);
            const double tj = 0.1 * J;
            const V3 mxh = cross(m0, h);
            V3 dm{-2.21e5 * mxh.x, -2.21e5 * mxh.y, -2.21e5 * mxh.z};
            const V3 mxdm = cross(m0, dm);
            dm = V3{dm.x + 0.01 * mxdm.x + tj * t2.x, dm.y + 0.01 * mxdm.y + tj * t2.y, dm.z + 0.01 * mxdm.z + tj * t2.z};
            const double dt = T / 10;
            V3 m = m0;
#pragma unroll
            for (int it = 0; it < 10; ++it) {
                m = V3{m.x + dm.x * dt, m.y + dm.y * dt, m.z + dm.z * dt};
                const double inv = rsqrt_fast(dot(m, m));       // m / |m| (array_env.py:518), <= 2 ulp per component
                m = V3{m.x * inv, m.y * inv, m.z * inv};
            }
            lp[(d * 3) * 64 + lane] = m.x; lp[(d * 3 + 1) * 64 + lane] = m.y; lp[(d * 3 + 2) * 64 + lane] = m.z;
            a.pattern[(int64_t)(d * 3) * N + i] = m.x;
            a.pattern[(int64_t)(d * 3 + 1) * N + i] = m.y;
            a.pattern[(int64_t)(d * 3 + 2) * N + i] = m.z;
            // similarity: only this cell's dot product changed
            const V3 tg{a.target[(int64_t)(d * 3) * N + i], a.target[(int64_t)(d * 3 + 1) * N + i], a.target[(int64_t)(d * 3 + 2) * N + i]};
            sim_sum += dot(m, tg) - dot(m0, tg);
            // energy with the resistance of the UPDATED state (current_m is a view of the pattern, array_env.py:455-463)
            e_total += cell_energy(m, J, T, a.dev);
        }
    }
    const double etot = a.etot[i] + e_total;
    const int32_t step = a.step[i] + 1;
    a.etot[i] = etot;
    a.step[i] = step;
    const double sim = sim_sum / n;
    const bool is_success = sim >= a.thr;
    // pattern rows of the observation + uniformity (1 - population std of the cell magnitudes, array_env.py:216-224)
    double mean = 0.0;
    for (int d = 0; d < n; ++d) {
        const V3 m{lp[(d * 3) * 64 + lane], lp[(d * 3 + 1) * 64 + lane], lp[(d * 3 + 2) * 64 + lane]};
        a.obs[obs_row_pattern(a.obs_mode, n, d, 0) * N + i] = (float)m.x;
        a.obs[obs_row_pattern(a.obs_mode, n, d, 1) * N + i] = (float)m.y;
        a.obs[obs_row_pattern(a.obs_mode, n, d, 2) * N + i] = (float)m.z;
        mean += sqrt(dot(m, m));
    }
    mean /= n;
    double var = 0.0;
    for (int d = 0; d < n; ++d) {
        const V3 m{lp[(d * 3) * 64 + lane], lp[(d * 3 + 1) * 64 + lane], lp[(d * 3 + 2) * 64 + lane]};
        const double dv = sqrt(dot(m, m)) - mean;
        var += dv * dv;
    }
    if (a.obs_mode == 1) {
        a.obs[(int64_t)(6 * n + 0) * N + i] = vector_value<0>(a.max_steps, a.temperature, sim, step, etot);
        a.obs[(int64_t)(6 * n + 1) * N + i] = vector_value<1>(a.max_steps, a.temperature, sim, step, etot);
        a.obs[(int64_t)(6 * n + 2) * N + i] = vector_value<2>(a.max_steps, a.temperature, sim, step, etot);
        a.obs[(int64_t)(6 * n + 3) * N + i] = vector_value<3>(a.max_steps, a.temperature, sim, step, etot);
    }
    const double uniformity = fmax(0.0, 1.0 - sqrt(var / n));
    // default reward (array_env.py:183-224): pattern match, energy (sign as written), progress, uniformity
    const double reward = default_reward(sim, prev_sim, is_success, e_total, uniformity, a.w_energy);
    write_step_outputs(a, i, reward, e_total, is_success, step >= a.max_steps);
}

// 'global' action mode on NDEV cells (4 x 4, the registered SpinTorqueArray-v0): every cell is addressed, in order.  The whole pattern
// lives in REGISTERS (48 doubles) instead of a 24.6 KB per-wavefront copy in LDS: that copy bounded the general kernel at six
// single-wavefront workgroups per CU (1.5 wavefronts per SIMD) for a launch that is a chain of 160 dependent normalise-and-step
// iterations per lane -- latency-bound.  Registers cannot be indexed by the running cell, so the register file is ROTATED instead: at
// the top of iteration d, pm[0] is cell d and pm[k] cell (d + k) mod n; after the update everything moves down one place (48 64-bit
// moves per cell) and after n iterations it is back in place.  The coupling matrix is staged in LDS in that rotated order
// (lc[d][k] = C[d][(d + k) mod n]), so a row is sixteen consecutive doubles.  All row accesses to the pattern / target / observation
// arrays are BUFFER instructions: descriptor and row offset in scalar registers, one 32-bit lane offset in a VGPR -- no per-row 64-bit
// VGPR addresses.  (A fully unrolled sweep, the other way to keep the pattern in registers, needed more than 340 of them: one
// wavefront per SIMD.)  The coupling sum runs over the cells in rotated order (d+1, ..., n-1, 0, ..., d-1) instead of 0 ... n-1: the
// only arithmetic difference to the general kernel, at the rounding level of a term that is ~1e-3 of the field.
template <int NDEV>
__global__ void __launch_bounds__(256, 3) stg_array_step_global_kernel(const ArrArgs a) {
    extern __shared__ double lds[];           // rotated coupling [n][n]
    constexpr int n = NDEV;
    double* lc = lds;
    if (a.include_coupling) {
        for (int q = threadIdx.x; q < n * n; q += blockDim.x) {
            const int d = q / n, k = q % n;
            lc[q] = a.coupling[d * n + (d + k) % n];
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const uint32_t off8 = (uint32_t)i * 8u, off4 = (uint32_t)i * 4u;
    const uint32_t row8 = (uint32_t)N * 8u, row4 = (uint32_t)N * 4u;
    const int obs_rows = 6 * n + (a.obs_mode == 1 ? 4 : 0);
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)a.pattern, 0, (int)(3u * n * row8), 0x00020000);
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc((void*)a.target, 0, (int)(3u * n * row8), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)a.obs, 0, (int)((uint32_t)obs_rows * row4), 0x00020000);
    auto ldp = [&](int row) -> double { return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rp, off8, (uint32_t)row * row8, 0)); };
    auto ldt = [&](int row) -> double { return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rt, off8, (uint32_t)row * row8, 0)); };
    auto stp = [&](int row, double v) { __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rp, off8, (uint32_t)row * row8, 0); };
    auto sto = [&](int64_t row, float v) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), ro, off4, (uint32_t)row * row4, 0); };
    V3 pm[NDEV];
    double sim_sum = 0.0;
#pragma unroll
    for (int d = 0; d < n; ++d) {
        double pv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pv[k] = ldp(d * 3 + k);
            const double tv = ldt(d * 3 + k);
            sto(obs_row_target(a.obs_mode, n, d, k), (float)tv);
            sim_sum += pv[k] * tv;
        }
        pm[d] = V3{pv[0], pv[1], pv[2]};
    }
    const double prev_sim = sim_sum / n;                                               // array_env.py:372-373
    // _apply_action in 'global' mode (array_env.py:411-445): the action is [current, duration]; action[1] is what the reference reads
    // as the current density and the duration defaults to 1 ns -- kept as is
    double J = (double)a.actions[N + i];
    double T = 1e-9;
    J = isnan(J) ? J : fmin(fmax(J, -a.max_current), a.max_current);
    T = isnan(T) ? T : fmin(fmax(T, 1e-12), a.max_duration);
    const bool drive = fabs(J) > 1e-12;                                                // array_env.py:506
    double e_total = 0.0;
    if (drive) {
#pragma unroll 1
        for (int d = 0; d < n; ++d) {
            const V3 m0 = pm[0];
            V3 h = device_field(m0, a.dev);
            if (a.include_coupling) {                                                  // array_env.py:485-492
                const double* crow = lc + d * n;                                       // crow[k] = C[d][(d + k) mod n]
                V3 hc{0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 1; k < n; ++k) {
                    const double c = crow[k];
                    hc = V3{hc.x + c * pm[k].x, hc.y + c * pm[k].y, hc.z + c * pm[k].z};
                }
                h = V3{h.x + hc.x, h.y + hc.y, h.z + hc.z};
            }
            const V3 m = euler_cell(m0, h, J, T);
            stp(d * 3, m.x);
            stp(d * 3 + 1, m.y);
            stp(d * 3 + 2, m.z);
            // similarity: only this cell's dot product changed
            const V3 tg{ldt(d * 3), ldt(d * 3 + 1), ldt(d * 3 + 2)};
            sim_sum += dot(m, tg) - dot(m0, tg);
            // energy with the resistance of the UPDATED state (current_m is a view of the pattern, array_env.py:455-463)
            e_total += cell_energy(m, J, T, a.dev);
            // rotate: cell d (updated) goes to the end, cell d+1 to the front
#pragma unroll
            for (int k = 0; k + 1 < n; ++k) pm[k] = pm[k + 1];
            pm[n - 1] = m;
        }
    }
    const double etot = a.etot[i] + e_total;
    const int32_t step = a.step[i] + 1;
    a.etot[i] = etot;
    a.step[i] = step;
    const double sim = sim_sum / n;
    const bool is_success = sim >= a.thr;
    // pattern rows of the observation + uniformity (1 - population std of the cell magnitudes, array_env.py:216-224)
    double mean = 0.0;
#pragma unroll
    for (int d = 0; d < n; ++d) {
        const V3 m = pm[d];
        sto(obs_row_pattern(a.obs_mode, n, d, 0), (float)m.x);
        sto(obs_row_pattern(a.obs_mode, n, d, 1), (float)m.y);
        sto(obs_row_pattern(a.obs_mode, n, d, 2), (float)m.z);
        mean += sqrt(dot(m, m));
    }
    mean /= n;
    double var = 0.0;
#pragma unroll
    for (int d = 0; d < n; ++d) {
        const double dv = sqrt(dot(pm[d], pm[d])) - mean;
        var += dv * dv;
    }
    if (a.obs_mode == 1) {
        sto(6 * n + 0, vector_value<0>(a.max_steps, a.temperature, sim, step, etot));
        sto(6 * n + 1, vector_value<1>(a.max_steps, a.temperature, sim, step, etot));
        sto(6 * n + 2, vector_value<2>(a.max_steps, a.temperature, sim, step, etot));
        sto(6 * n + 3, vector_value<3>(a.max_steps, a.temperature, sim, step, etot));
    }
    const double uniformity = fmax(0.0, 1.0 - sqrt(var / n));
    // default reward (array_env.py:183-224): pattern match, energy (sign as written), progress, uniformity
    const double reward = default_reward(sim, prev_sim, is_success, e_total, uniformity, a.w_energy);
    write_step_outputs(a, i, reward, e_total, is_success, step >= a.max_steps);
}

// 'individual' action mode (one addressed cell per step): nothing but that one cell changes, so the step is ONE streaming
// pass over the array -- pattern and target in, both halves of the observation out, similarity, norm statistics and the
// addressed cell's coupling sum accumulated on the way -- with no per-lane copy of the pattern in LDS.  Only the coupling
// matrix sits in LDS (shared by the workgroup), so occupancy is set by registers, not by 24 KB of LDS per wavefront, and
// the kernel keeps far more loads in flight.  Same arithmetic as the general kernel except the population standard
// deviation of the cell norms (uniformity term), which is formed in one pass from e_j = |m_j| - 1 (the norms are 1 to
// rounding, so sum(e^2)/n - mean(e)^2 has no cancellation problem at the 1e-16 level the quantity lives at).
__global__ void __launch_bounds__(256) stg_array_step_individual_kernel(const ArrArgs a) {
    extern __shared__ double lds[];           // coupling [n*n]
    const int n = a.rows * a.cols;
    double* lc = lds;
    if (a.include_coupling) {
        for (int q = threadIdx.x; q < n * n; q += blockDim.x) lc[q] = a.coupling[q];
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N) return;
    const int64_t N = a.N;
    // _apply_action (array_env.py:411-445)
    double J = (double)a.actions[N + i];
    double T = (double)a.actions[2 * N + i];
    J = isnan(J) ? J : fmin(fmax(J, -a.max_current), a.max_current);
    T = isnan(T) ? T : fmin(fmax(T, 1e-12), a.max_duration);
    const double a0 = (double)a.actions[i];
    // int(np.clip(action[0], 0, n-1)); a NaN index raises in the reference -- here it addresses nothing
    const int d = isnan(a0) ? -1 : (int)fmin(fmax(a0, 0.0), (double)(n - 1));
    const bool drive = fabs(J) > 1e-12 && d >= 0;                                      // array_env.py:506
    const double* crow = lc + (d >= 0 ? d : 0) * n;
    double sim_sum = 0.0, se = 0.0, se2 = 0.0;
    V3 m0{0.0, 0.0, 1.0}, tg{0.0, 0.0, 1.0}, hc{0.0, 0.0, 0.0};
    double e_d = 0.0;
    for (int j = 0; j < n; ++j) {
        const V3 pv{a.pattern[(int64_t)(j * 3) * N + i], a.pattern[(int64_t)(j * 3 + 1) * N + i], a.pattern[(int64_t)(j * 3 + 2) * N + i]};
        const V3 tv{a.target[(int64_t)(j * 3) * N + i], a.target[(int64_t)(j * 3 + 1) * N + i], a.target[(int64_t)(j * 3 + 2) * N + i]};
        a.obs[obs_row_target(a.obs_mode, n, j, 0) * N + i] = (float)tv.x;
        a.obs[obs_row_target(a.obs_mode, n, j, 1) * N + i] = (float)tv.y;
        a.obs[obs_row_target(a.obs_mode, n, j, 2) * N + i] = (float)tv.z;
        a.obs[obs_row_pattern(a.obs_mode, n, j, 0) * N + i] = (float)pv.x;          // (the addressed cell is rewritten below)
        a.obs[obs_row_pattern(a.obs_mode, n, j, 1) * N + i] = (float)pv.y;
        a.obs[obs_row_pattern(a.obs_mode, n, j, 2) * N + i] = (float)pv.z;
        sim_sum += pv.x * tv.x; sim_sum += pv.y * tv.y; sim_sum += pv.z * tv.z;       // same order as the general kernel
        const double e = sqrt(dot(pv, pv)) - 1.0;
        se += e; se2 += e * e;
        if (j == d) { m0 = pv; tg = tv; e_d = e; }
        if (a.include_coupling && drive) {                                             // array_env.py:485-492
            const double c = (j == d) ? 0.0 : crow[j];
            hc = V3{hc.x + c * pv.x, hc.y + c * pv.y, hc.z + c * pv.z};
        }
    }
    const double prev_sim = sim_sum / n;                                               // array_env.py:372-373
    double e_total = 0.0;
    if (drive) {
        V3 h = device_field(m0, a.dev);
        if (a.include_coupling) h = V3{h.x + hc.x, h.y + hc.y, h.z + hc.z};
        const V3 m = euler_cell(m0, h, J, T);
        a.pattern[(int64_t)(d * 3) * N + i] = m.x;
        a.pattern[(int64_t)(d * 3 + 1) * N + i] = m.y;
        a.pattern[(int64_t)(d * 3 + 2) * N + i] = m.z;
        a.obs[obs_row_pattern(a.obs_mode, n, d, 0) * N + i] = (float)m.x;
        a.obs[obs_row_pattern(a.obs_mode, n, d, 1) * N + i] = (float)m.y;
        a.obs[obs_row_pattern(a.obs_mode, n, d, 2) * N + i] = (float)m.z;
        sim_sum += dot(m, tg) - dot(m0, tg);
        const double e_new = sqrt(dot(m, m)) - 1.0;
        se += e_new - e_d; se2 += e_new * e_new - e_d * e_d;
        // energy with the resistance of the UPDATED state (current_m is a view of the pattern, array_env.py:455-463)
        e_total = cell_energy(m, J, T, a.dev);
    }
    const double etot = a.etot[i] + e_total;
    const int32_t step = a.step[i] + 1;
    a.etot[i] = etot;
    a.step[i] = step;
    const double sim = sim_sum / n;
    const bool is_success = sim >= a.thr;
    if (a.obs_mode == 1) vector_rows(a, a.obs, n, i, sim, step, etot);
    // uniformity = 1 - population std of the cell norms (array_env.py:216-224)
    const double me = se / n;
    const double var = fmax(se2 / n - me * me, 0.0);
    const double uniformity = fmax(0.0, 1.0 - sqrt(var));
    const double reward = default_reward(sim, prev_sim, is_success, e_total, uniformity, a.w_energy);
    write_step_outputs(a, i, reward, e_total, is_success, step >= a.max_steps);
}

struct ArrResetArgs {
    int64_t N, env_id0;
    int32_t rows, cols, max_steps, obs_mode;
    double temperature;
    const uint8_t* mask;
    const double *init_pattern, *target_in;
    double *pattern, *target, *etot;
    int32_t* step;
    uint32_t* resets;
    uint64_t seed;
    int32_t default_target;
    float* obs;
};

__global__ void __launch_bounds__(64) stg_array_reset_kernel(const ArrResetArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.N) return;
    const int n = a.rows * a.cols;
    const int64_t N = a.N;
    const bool sel = !a.mask || a.mask[i];
    if (sel) {
        if (a.init_pattern) {
            for (int q = 0; q < 3 * n; ++q) a.pattern[(int64_t)q * N + i] = a.init_pattern[(int64_t)q * N + i];
        } else {   // normal(0,1,3) normalised per device (array_env.py:350-356), from the device generator
            NormalStream ns;
            ns.init(a.seed ^ 0x9E3779B97F4A7C15ull, (uint64_t)(a.env_id0 + i), a.resets[i], 0xFFFFFFFDu);
            for (int d = 0; d < n; ++d) {
                const V3 z = (d & 1) ? ns.draw3_odd() : ns.draw3_even();
                const double inv = 1.0 / sqrt(dot(z, z));
                a.pattern[(int64_t)(d * 3) * N + i] = z.x * inv;
                a.pattern[(int64_t)(d * 3 + 1) * N + i] = z.y * inv;
                a.pattern[(int64_t)(d * 3 + 2) * N + i] = z.z * inv;
            }
            a.resets[i] += 1;
        }
        if (a.target_in) {
            for (int q = 0; q < 3 * n; ++q) a.target[(int64_t)q * N + i] = a.target_in[(int64_t)q * N + i];
        } else if (a.default_target) {   // checkerboard of +-z (array_env.py:161-170)
            for (int d = 0; d < n; ++d) {
                const int r = d / a.cols, c = d % a.cols;
                a.target[(int64_t)(d * 3) * N + i] = 0.0;
                a.target[(int64_t)(d * 3 + 1) * N + i] = 0.0;
                a.target[(int64_t)(d * 3 + 2) * N + i] = ((r + c) % 2 == 0) ? 1.0 : -1.0;
            }
        }
        a.etot[i] = 0.0;
        a.step[i] = 0;
    }
    if (a.obs) {
        double s = 0.0;
        for (int d = 0; d < n; ++d)
            for (int k = 0; k < 3; ++k) s += a.pattern[(int64_t)(d * 3 + k) * N + i] * a.target[(int64_t)(d * 3 + k) * N + i];
        const double sim = s / n;
        if (a.obs_mode == 0) {
            for (int d = 0; d < n; ++d)
                for (int k = 0; k < 3; ++k) {
                    a.obs[(int64_t)(d * 6 + k) * N + i] = (float)a.pattern[(int64_t)(d * 3 + k) * N + i];
                    a.obs[(int64_t)(d * 6 + 3 + k) * N + i] = (float)a.target[(int64_t)(d * 3 + k) * N + i];
                }
        } else {
            for (int q = 0; q < 3 * n; ++q) {
                a.obs[(int64_t)q * N + i] = (float)a.pattern[(int64_t)q * N + i];
                a.obs[(int64_t)(3 * n + q) * N + i] = (float)a.target[(int64_t)q * N + i];
            }
            a.obs[(int64_t)(6 * n + 0) * N + i] = vector_value<0>(a.max_steps, a.temperature, sim, a.step[i], a.etot[i]);
            a.obs[(int64_t)(6 * n + 1) * N + i] = vector_value<1>(a.max_steps, a.temperature, sim, a.step[i], a.etot[i]);
            a.obs[(int64_t)(6 * n + 2) * N + i] = vector_value<2>(a.max_steps, a.temperature, sim, a.step[i], a.etot[i]);
            a.obs[(int64_t)(6 * n + 3) * N + i] = vector_value<3>(a.max_steps, a.temperature, sim, a.step[i], a.etot[i]);
        }
    }
}

// ---- K fused steps with same-step auto-reset (stg_array_step_many) ------------------------------------------------------------------
// The general kernel's layout (one array per lane, 64-lane workgroups, pattern in LDS as [cell*3+component][64], coupling matrix behind
// it), but the pattern is loaded ONCE, stays in LDS for all K steps and is written back once; total energy and step count live in
// registers.  After the one barrier that publishes the coupling matrix a lane touches only its own LDS column, so lanes beyond N leave
// and the in-kernel reset needs no further barrier.  The target is NOT LDS-resident (a second 24.6 KB copy per wavefront would halve the
// resident wavefronts of a latency-bound kernel): it is re-read once per step, in the pass that forms the similarity from scratch.
// Forming the similarity from scratch every step (instead of carrying an incrementally updated sum) makes a step a function of the
// state alone, so K steps in one launch equal the same steps split over several launches bit for bit.
struct ArrManyArgs {
    ArrArgs s;                 // actions / outputs point at step 0 / output slot 0
    int64_t env_id0;
    int32_t K, out_every, autoreset;
    uint64_t seed;
    uint32_t* resets;          // [N]
    float* final_obs;          // [K or 1][obs_dim][N] or NULL
};

// One pass over the array: similarity sum of the LDS-resident pattern with the target (np.mean of the per-cell dot products,
// array_env.py:523-531, same order as the general kernel's first pass), the sum of the cell norms and, when dst is not NULL, the pattern
// and target rows of one observation.
__device__ __forceinline__ double many_pass(const ArrArgs& a, const double* lp, int lane, int n, int64_t i, float* dst, double& norm_sum) {
    const int64_t N = a.N;
    double sim_sum = 0.0, ns = 0.0;
    for (int d = 0; d < n; ++d) {
        const double pv[3] = {lp[(d * 3) * 64 + lane], lp[(d * 3 + 1) * 64 + lane], lp[(d * 3 + 2) * 64 + lane]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double tv = a.target[(int64_t)(d * 3 + k) * N + i];
            sim_sum += pv[k] * tv;
            if (dst) {
                dst[obs_row_pattern(a.obs_mode, n, d, k) * N + i] = (float)pv[k];
                dst[obs_row_target(a.obs_mode, n, d, k) * N + i] = (float)tv;
            }
        }
        ns += sqrt(dot(V3{pv[0], pv[1], pv[2]}, V3{pv[0], pv[1], pv[2]}));
    }
    norm_sum = ns;
    return sim_sum;
}

// the pattern and target rows of one observation, nothing else (the terminal observation of an array that is about to restart)
__device__ __forceinline__ void many_copy_rows(const ArrArgs& a, const double* lp, int lane, int n, int64_t i, float* dst) {
    const int64_t N = a.N;
    for (int d = 0; d < n; ++d) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dst[obs_row_pattern(a.obs_mode, n, d, k) * N + i] = (float)lp[(d * 3 + k) * 64 + lane];
            dst[obs_row_target(a.obs_mode, n, d, k) * N + i] = (float)a.target[(int64_t)(d * 3 + k) * N + i];
        }
    }
}

// One addressed cell, in place in LDS: effective field with the coupling sum over the current pattern, ten normalised Euler sub-steps of
// one derivative (array_env.py:478-521).  Returns the cell's energy, with the resistance of the UPDATED state (array_env.py:455-463).
template <int NDEV>
__device__ __forceinline__ double many_update_cell(const ArrArgs& a, double* lp, const double* lc, int lane, int n, int d, double J, double T) {
    const V3 m0{lp[(d * 3) * 64 + lane], lp[(d * 3 + 1) * 64 + lane], lp[(d * 3 + 2) * 64 + lane]};
    V3 h = device_field(m0, a.dev);
    if (a.include_coupling) {                                                      // array_env.py:485-492
        V3 hc{0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < (NDEV > 0 ? NDEV : n); ++j) {
            const double c = (j == d) ? 0.0 : lc[d * n + j];
            hc = V3{hc.x + c * lp[(j * 3) * 64 + lane], hc.y + c * lp[(j * 3 + 1) * 64 + lane], hc.z + c * lp[(j * 3 + 2) * 64 + lane]};
        }
        h = V3{h.x + hc.x, h.y + hc.y, h.z + hc.z};
    }
    const V3 m = euler_cell(m0, h, J, T);
    lp[(d * 3) * 64 + lane] = m.x; lp[(d * 3 + 1) * 64 + lane] = m.y; lp[(d * 3 + 2) * 64 + lane] = m.z;
    return cell_energy(m, J, T, a.dev);
}

// stg_array_reset_kernel's random draw for one array (same stream key, same normalisation), into the array's LDS column
__device__ __forceinline__ void many_draw_pattern(double* lp, int lane, int n, uint64_t seed, uint64_t env_id, uint32_t resets) {
    NormalStream ns;
    ns.init(seed ^ 0x9E3779B97F4A7C15ull, env_id, resets, 0xFFFFFFFDu);
    for (int d = 0; d < n; ++d) {
        const V3 z = (d & 1) ? ns.draw3_odd() : ns.draw3_even();
        const double inv = 1.0 / sqrt(dot(z, z));
        lp[(d * 3) * 64 + lane] = z.x * inv;
        lp[(d * 3 + 1) * 64 + lane] = z.y * inv;
        lp[(d * 3 + 2) * 64 + lane] = z.z * inv;
    }
}

template <int NDEV>
__global__ void __launch_bounds__(64) stg_array_step_many_kernel(const ArrManyArgs b) {
    extern __shared__ double lds[];           // pattern [n*3][64] then coupling [n*n]
    const ArrArgs& a = b.s;
    const int n = NDEV > 0 ? NDEV : a.rows * a.cols;
    double* lp = lds;
    double* lc = lds + (size_t)n * 3 * 64;
    const int lane = threadIdx.x;
    if (a.include_coupling) {
        for (int q = lane; q < n * n; q += 64) lc[q] = a.coupling[q];
    }
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool in_range = i < a.N;
    const int64_t N = a.N;
    if (in_range) {
        for (int q = 0; q < 3 * n; ++q) lp[q * 64 + lane] = a.pattern[(int64_t)q * N + i];
    }
    __syncthreads();           // the only barrier: from here on a lane reads the coupling matrix and its own LDS column, nothing else
    if (!in_range) return;
    double etot = a.etot[i];
    int32_t step = a.step[i];
    const int n_act = a.mode == 3 ? 2 : 3;
    const int64_t obs_rows = 6 * n + (a.obs_mode == 1 ? 4 : 0);
    double norm_sum;
    double sim_sum = many_pass(a, lp, lane, n, i, nullptr, norm_sum);
#pragma unroll 1
    for (int k = 0; k < b.K; ++k) {
        const float* act = a.actions + (int64_t)k * n_act * N;
        const bool emit = b.out_every || k == b.K - 1;
        const int64_t slot = b.out_every ? k : 0;
        float* obs = emit ? a.obs + slot * obs_rows * N : nullptr;
        const double prev_sim = sim_sum / n;                                           // array_env.py:372-373
        // _apply_action (array_env.py:411-445).  In 'global' mode the action is [current, duration]: action[1] (the duration) is what
        // the reference reads as the current density, and the duration defaults to 1 ns -- kept as is.
        double J = (double)act[N + i];
        double T = n_act > 2 ? (double)act[2 * N + i] : 1e-9;
        J = isnan(J) ? J : fmin(fmax(J, -a.max_current), a.max_current);
        T = isnan(T) ? T : fmin(fmax(T, 1e-12), a.max_duration);
        int first = 0, count = n, stride = 1;
        if (a.mode != 3) {
            const double lim = a.mode == 0 ? n - 1 : (a.mode == 1 ? a.rows - 1 : a.cols - 1);
            const double a0 = (double)act[i];
            // int(np.clip(action[0], 0, lim)); a NaN index raises in the reference -- here it addresses nothing
            const int idx = isnan(a0) ? -1 : (int)fmin(fmax(a0, 0.0), lim);
            if (a.mode == 0) { first = idx; count = 1; stride = 1; }
            else if (a.mode == 1) { first = idx * a.cols; count = a.cols; stride = 1; }
            else { first = idx; count = a.rows; stride = a.cols; }
            if (idx < 0) count = 0;
        }
        double e_total = 0.0;
        if (fabs(J) > 1e-12) {                                                         // array_env.py:506
            // The addressed cells update sequentially and each sees its predecessors' new states through the coupling sum
            // (the reference updates current_pattern in place, array_env.py:447-476).
#pragma unroll 1
            for (int q = 0; q < count; ++q) e_total += many_update_cell<NDEV>(a, lp, lc, lane, n, first + q * stride, J, T);
        }
        etot += e_total;
        step += 1;
        sim_sum = many_pass(a, lp, lane, n, i, obs, norm_sum);
        const double sim = sim_sum / n;
        const bool is_success = sim >= a.thr;
        // uniformity: 1 - population std of the cell magnitudes (array_env.py:216-224)
        const double mean = norm_sum / n;
        double var = 0.0;
        for (int d = 0; d < n; ++d) {
            const V3 m{lp[(d * 3) * 64 + lane], lp[(d * 3 + 1) * 64 + lane], lp[(d * 3 + 2) * 64 + lane]};
            const double dv = sqrt(dot(m, m)) - mean;
            var += dv * dv;
        }
        const double uniformity = fmax(0.0, 1.0 - sqrt(var / n));
        // default reward (array_env.py:183-224): pattern match, energy (sign as written), progress, uniformity
        const double reward = default_reward(sim, prev_sim, is_success, e_total, uniformity, a.w_energy);
        const bool truncated = step >= a.max_steps;
        if (emit) {
            if (a.obs_mode == 1) vector_rows(a, obs, n, i, sim, step, etot);
            write_step_outputs(a, slot * N + i, reward, e_total, is_success, truncated);
        }
        if (b.autoreset && (is_success || truncated)) {
            // the step above reported the finished episode; its terminal observation goes to final_obs and the array restarts as
            // stg_array_reset(mask = this array, init_pattern = NULL, target = NULL, seed) restarts it
            if (emit && b.final_obs) {
                float* fo = b.final_obs + slot * obs_rows * N;
                many_copy_rows(a, lp, lane, n, i, fo);
                if (a.obs_mode == 1) vector_rows(a, fo, n, i, sim, step, etot);
            }
            const uint32_t rs = b.resets[i];
            many_draw_pattern(lp, lane, n, b.seed, (uint64_t)(b.env_id0 + i), rs);
            b.resets[i] = rs + 1;
            etot = 0.0;
            step = 0;
            sim_sum = many_pass(a, lp, lane, n, i, obs, norm_sum);
            if (emit && a.obs_mode == 1) vector_rows(a, obs, n, i, sim_sum / n, step, etot);
        }
    }
    for (int q = 0; q < 3 * n; ++q) a.pattern[(int64_t)q * N + i] = lp[q * 64 + lane];
    a.etot[i] = etot;
    a.step[i] = step;
}

}  // namespace

extern "C" int stg_internal_fail(int code, const char* msg);     // spintorque_hip.hip: sets stg_last_error()
static int afail(int code, const std::string& msg) { return stg_internal_fail(code, msg.c_str()); }

#define AHIP_TRY(expr)                                                                                  \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return afail(STG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct stg_array_ctx {
    int device;
    int64_t N, env_id0;
    stg_array_config cfg;
    ArrDev dev;
    void* slab = nullptr;
    double *pattern, *target, *etot, *coupling;
    int32_t* step;
    uint32_t* resets;
    bool have_state = false, have_target = false;
    int lds_max = 0;          // the device's LDS per workgroup, in bytes (stg_array_step_many checks its request against it)
    int variant = 1;          // experiment knob STG_ARRAY_VARIANT: 0 generic kernel for every size, 1 (default) the 4 x 4 specialisations,
                              // 2 the 4 x 4 kernel with the pattern in LDS in 'global' mode too
};

// LDS per workgroup: the coupling matrix alone (streaming and register kernels), and behind one wavefront's pattern [n*3][64] (the general
// and the fused kernel: 26 KB at 4 x 4, 128 KB at 8 x 8)
static size_t coupling_bytes(const stg_array_config& c) {
    const size_t n = (size_t)c.rows * c.cols;
    return c.include_coupling ? sizeof(double) * n * n : 0;
}
static size_t lds_bytes(const stg_array_config& c) { return sizeof(double) * ((size_t)c.rows * c.cols * 3 * 64) + coupling_bytes(c); }

// one step's kernel arguments: the context's configuration and state, the caller's actions and outputs
static ArrArgs fill_args(const stg_array_ctx* ctx, const float* actions, float* obs, float* reward, double* reward_f64, double* energy,
                         uint8_t* terminated, uint8_t* truncated) {
    const stg_array_config& c = ctx->cfg;
    ArrArgs a{};
    a.N = ctx->N; a.rows = c.rows; a.cols = c.cols; a.mode = c.action_mode; a.include_coupling = c.include_coupling;
    a.max_steps = c.max_steps; a.obs_mode = c.obs_mode; a.max_current = c.max_current; a.max_duration = c.max_duration;
    a.thr = c.success_threshold; a.w_energy = c.energy_penalty_weight; a.temperature = c.temperature; a.dev = ctx->dev;
    a.coupling = ctx->coupling; a.pattern = ctx->pattern; a.target = ctx->target; a.etot = ctx->etot; a.step = ctx->step;
    a.actions = actions; a.obs = obs; a.reward = reward; a.reward64 = reward_f64; a.energy = energy; a.term = terminated;
    a.trunc = truncated;
    return a;
}

extern "C" {

int stg_array_create(stg_array_ctx** out, int device_id, int64_t n_arrays, int64_t env_id0, const stg_array_config* cfg,
                     const stg_device_params* p, const double* coupling) {
    if (!out || !cfg || !p) return afail(STG_E_INVALID, "out/cfg/dev is NULL");
    *out = nullptr;
    if (n_arrays < 1) return afail(STG_E_INVALID, "n_arrays must be >= 1");
    const int n = cfg->rows * cfg->cols;
    if (cfg->rows < 1 || cfg->cols < 1 || n > ARR_MAX_DEV) return afail(STG_E_INVALID, "array size must be between 1 and 64 devices");
    if (cfg->action_mode < 0 || cfg->action_mode > 3) return afail(STG_E_INVALID, "action_mode must be 0..3");
    if (cfg->obs_mode < 0 || cfg->obs_mode > 1) return afail(STG_E_INVALID, "obs_mode must be 0 ('array') or 1 ('vector')");
    if (cfg->include_coupling && !coupling) return afail(STG_E_INVALID, "coupling matrix required when include_coupling is set");
    if (cfg->max_steps < 1) return afail(STG_E_INVALID, "max_steps must be >= 1");
    if (p->dev_type < 0 || p->dev_type > 2) return afail(STG_E_INVALID, "dev_type must be STG_DEV_STT/SOT/VCMA");
    int ndev = 0;
    AHIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return afail(STG_E_INVALID, "device_id out of range");
    AHIP_TRY(hipSetDevice(device_id));
    stg_array_ctx* c = new (std::nothrow) stg_array_ctx();
    if (!c) return afail(STG_E_NOMEM, "out of host memory");
    c->device = device_id; c->N = n_arrays; c->env_id0 = env_id0; c->cfg = *cfg;
    if (const char* e = std::getenv("STG_ARRAY_VARIANT")) c->variant = std::atoi(e);
    {
        hipError_t eq = hipDeviceGetAttribute(&c->lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id);
        if (eq != hipSuccess) { delete c; return afail(STG_E_HIP, std::string("hipDeviceGetAttribute: ") + hipGetErrorString(eq)); }
    }
    // A launch of the generic LDS kernels above 48 KB of LDS needs the opt-in once; here, so that a step call only enqueues.  The limit is
    // per kernel, not per context, so it is raised to the device's: a later context with smaller arrays must not lower it again.
    if (const size_t need = lds_bytes(*cfg); need > 48 * 1024 && need <= (size_t)c->lds_max) {
        for (const void* k : {(const void*)stg_array_step_kernel<0>, (const void*)stg_array_step_many_kernel<0>}) {
            hipError_t ea = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, c->lds_max);
            if (ea != hipSuccess) { delete c; return afail(STG_E_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(ea)); }
        }
    }
    const double mu0 = 4 * M_PI * 1e-7;
    ArrDev& d = c->dev;
    d.hk = 2 * p->ku / (mu0 * p->ms); d.ms = p->ms;                       // stt_mram.py:71, sot_mram.py:93
    d.ex = p->easy_axis[0]; d.ey = p->easy_axis[1]; d.ez = p->easy_axis[2];
    d.nx = p->shape_demag[0]; d.ny = p->shape_demag[1]; d.nz = p->shape_demag[2];
    d.area = p->area; d.r_p = p->r_p; d.r_ap = p->r_ap; d.tmr = (p->r_ap - p->r_p) / p->r_p;
    const double rn = std::sqrt((p->ref_m[0] * p->ref_m[0] + p->ref_m[1] * p->ref_m[1]) + p->ref_m[2] * p->ref_m[2]);
    d.refx = p->ref_m[0] / rn; d.refy = p->ref_m[1] / rn; d.refz = p->ref_m[2] / rn;
    d.r_series = p->r_series; d.dev_type = p->dev_type;
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t N = (size_t)n_arrays;
    const size_t rp = al(N * 8 * 3 * n), r8 = al(N * 8), r4 = al(N * 4), rc = al(sizeof(double) * n * n);
    const size_t total = 2 * rp + r8 + 2 * r4 + rc;
    hipError_t e = hipMalloc(&c->slab, total);
    if (e != hipSuccess) { delete c; return afail(STG_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    (void)hipMemset(c->slab, 0, total);
    char* q = (char*)c->slab;
    c->pattern = (double*)q; q += rp;
    c->target = (double*)q; q += rp;
    c->etot = (double*)q; q += r8;
    c->step = (int32_t*)q; q += r4;
    c->resets = (uint32_t*)q; q += r4;
    c->coupling = (double*)q;
    if (cfg->include_coupling) {
        e = hipMemcpy(c->coupling, coupling, sizeof(double) * n * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(c->slab); delete c; return afail(STG_E_HIP, "hipMemcpy(coupling) failed"); }
    }
    *out = c;
    return STG_OK;
}

void stg_array_destroy(stg_array_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->slab) (void)hipFree(ctx->slab);
    delete ctx;
}

int stg_array_reset(stg_array_ctx* ctx, const uint8_t* mask, const double* init_pattern, const double* target,
                    uint64_t seed, float* obs_out, void* stream) {
    if (!ctx) return afail(STG_E_INVALID, "ctx is NULL");
    AHIP_TRY(hipSetDevice(ctx->device));
    ArrResetArgs a{};
    a.N = ctx->N; a.env_id0 = ctx->env_id0; a.rows = ctx->cfg.rows; a.cols = ctx->cfg.cols; a.max_steps = ctx->cfg.max_steps;
    a.obs_mode = ctx->cfg.obs_mode; a.temperature = ctx->cfg.temperature; a.mask = mask; a.init_pattern = init_pattern;
    a.target_in = target; a.pattern = ctx->pattern; a.target = ctx->target; a.etot = ctx->etot; a.step = ctx->step;
    a.resets = ctx->resets; a.seed = seed; a.default_target = ctx->have_target ? 0 : 1; a.obs = obs_out;
    hipLaunchKernelGGL(stg_array_reset_kernel, dim3((unsigned)((ctx->N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    AHIP_TRY(hipGetLastError());
    ctx->have_state = true;
    ctx->have_target = true;
    return STG_OK;
}

int stg_array_step(stg_array_ctx* ctx, const float* actions, float* obs, float* reward, double* reward_f64, double* energy,
                   uint8_t* terminated, uint8_t* truncated, void* stream) {
    if (!ctx) return afail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_state) return afail(STG_E_STATE, "stg_array_reset must precede stg_array_step");
    if (!actions || !obs || !reward || !terminated || !truncated) return afail(STG_E_INVALID, "actions/obs/reward/terminated/truncated must not be NULL");
    AHIP_TRY(hipSetDevice(ctx->device));
    const stg_array_config& c = ctx->cfg;
    const ArrArgs a = fill_args(ctx, actions, obs, reward, reward_f64, energy, terminated, truncated);
    const int n = c.rows * c.cols;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid256((unsigned)((ctx->N + 255) / 256)), grid64((unsigned)((ctx->N + 63) / 64));
    if (c.action_mode == 0) {
        // one addressed cell per step: streaming kernel, only the coupling matrix in LDS (<= 32 KB at 8 x 8)
        hipLaunchKernelGGL(stg_array_step_individual_kernel, grid256, dim3(256), coupling_bytes(c), st, a);
    } else if (c.action_mode == 3 && n == 16 && ctx->variant >= 1 && ctx->variant != 2 && ctx->N <= (4ll << 20)) {
        // 'global' mode on 4 x 4 arrays: pattern in registers (STG_ARRAY_VARIANT=2: the LDS form of this size).  The kernel's buffer
        // descriptors hold 32-bit sizes: up to 4 M arrays.
        hipLaunchKernelGGL((stg_array_step_global_kernel<16>), grid256, dim3(256), coupling_bytes(c), st, a);
    } else if (n == 16 && ctx->variant != 0) {
        // 4 x 4 arrays (the registered SpinTorqueArray-v0): the coupling sum unrolled
        hipLaunchKernelGGL((stg_array_step_kernel<16>), grid64, dim3(64), lds_bytes(c), st, a);
    } else {
        hipLaunchKernelGGL((stg_array_step_kernel<0>), grid64, dim3(64), lds_bytes(c), st, a);
    }
    AHIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_array_get_state(stg_array_ctx* ctx, double* pattern, double* target, double* total_energy, int32_t* step_count,
                        void* stream) {
    if (!ctx) return afail(STG_E_INVALID, "ctx is NULL");
    AHIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)ctx->N, n = (size_t)ctx->cfg.rows * ctx->cfg.cols;
    if (pattern) AHIP_TRY(hipMemcpyAsync(pattern, ctx->pattern, N * 8 * 3 * n, hipMemcpyDeviceToDevice, st));
    if (target) AHIP_TRY(hipMemcpyAsync(target, ctx->target, N * 8 * 3 * n, hipMemcpyDeviceToDevice, st));
    if (total_energy) AHIP_TRY(hipMemcpyAsync(total_energy, ctx->etot, N * 8, hipMemcpyDeviceToDevice, st));
    if (step_count) AHIP_TRY(hipMemcpyAsync(step_count, ctx->step, N * 4, hipMemcpyDeviceToDevice, st));
    return STG_OK;
}

int stg_array_step_many(stg_array_ctx* ctx, int32_t K, const float* actions, int32_t out_every, int32_t autoreset, uint64_t seed,
                        float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                        uint8_t* truncated, void* stream) {
    if (!ctx) return afail(STG_E_INVALID, "ctx is NULL");
    if (K < 1) return afail(STG_E_INVALID, "K must be >= 1");
    if (!actions || !obs || !reward || !terminated || !truncated) return afail(STG_E_INVALID, "actions/obs/reward/terminated/truncated must not be NULL");
    if (!ctx->have_state) return afail(STG_E_STATE, "stg_array_reset (or stg_array_set_state) must precede stg_array_step_many");
    AHIP_TRY(hipSetDevice(ctx->device));
    const stg_array_config& c = ctx->cfg;
    const int n = c.rows * c.cols;
    const size_t lds = lds_bytes(c);           // checked against the device before anything is launched
    if (lds > (size_t)ctx->lds_max)
        return afail(STG_E_INVALID, "stg_array_step_many: the array's pattern and coupling matrix (" + std::to_string(lds) +
                                        " bytes per workgroup) do not fit the device's LDS (" + std::to_string(ctx->lds_max) + ")");
    ArrManyArgs b{};
    b.s = fill_args(ctx, actions, obs, reward, reward_f64, energy, terminated, truncated);
    b.env_id0 = ctx->env_id0; b.K = K; b.out_every = out_every ? 1 : 0; b.autoreset = autoreset ? 1 : 0; b.seed = seed;
    b.resets = ctx->resets; b.final_obs = final_obs;
    const dim3 grid((unsigned)((ctx->N + 63) / 64));
    if (n == 16) {
        hipLaunchKernelGGL((stg_array_step_many_kernel<16>), grid, dim3(64), lds, (hipStream_t)stream, b);
    } else {
        hipLaunchKernelGGL((stg_array_step_many_kernel<0>), grid, dim3(64), lds, (hipStream_t)stream, b);
    }
    AHIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_array_set_state(stg_array_ctx* ctx, const double* pattern, const double* target, const double* total_energy,
                        const int32_t* step_count, const uint32_t* resets, void* stream) {
    if (!ctx) return afail(STG_E_INVALID, "ctx is NULL");
    AHIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)ctx->N, n = (size_t)ctx->cfg.rows * ctx->cfg.cols;
    if (pattern) AHIP_TRY(hipMemcpyAsync(ctx->pattern, pattern, N * 8 * 3 * n, hipMemcpyDeviceToDevice, st));
    if (target) AHIP_TRY(hipMemcpyAsync(ctx->target, target, N * 8 * 3 * n, hipMemcpyDeviceToDevice, st));
    if (total_energy) AHIP_TRY(hipMemcpyAsync(ctx->etot, total_energy, N * 8, hipMemcpyDeviceToDevice, st));
    if (step_count) AHIP_TRY(hipMemcpyAsync(ctx->step, step_count, N * 4, hipMemcpyDeviceToDevice, st));
    if (resets) AHIP_TRY(hipMemcpyAsync(ctx->resets, resets, N * 4, hipMemcpyDeviceToDevice, st));
    if (pattern) ctx->have_state = true;       // a context that never had a pattern still needs its first reset
    if (target) ctx->have_target = true;
    return STG_OK;
}

int stg_array_get_resets(stg_array_ctx* ctx, uint32_t* resets, void* stream) {
    if (!ctx) return afail(STG_E_INVALID, "ctx is NULL");
    if (!resets) return afail(STG_E_INVALID, "resets is NULL");
    AHIP_TRY(hipSetDevice(ctx->device));
    AHIP_TRY(hipMemcpyAsync(resets, ctx->resets, (size_t)ctx->N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return STG_OK;
}

}  // extern "C"
