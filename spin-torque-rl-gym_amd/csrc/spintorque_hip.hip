// spintorque_hip.hip -- kernels and C-ABI of libspintorque_hip.so (see include/spintorque_hip.h).
//
// Layout in HBM (all owned by the context, structure-of-arrays, env index fastest):
//   state : EnvRec[N] = { f64 m[3], target[3], e_tot; u32 step | done << 31; u32 rng }        = 64 B/env, one record per env
//   class table                : f64[n_classes][C_COUNT]  (derived constants, <= 64 classes)
//   cls                        : u8[N] (caller-owned) when n_classes > 1
//   per-env parameters         : records f64[N][16 | 20 | 24] (library-owned, packed from the caller's rows: the fields the context's
//                                solver / torque model read, stg_kernels.hpp: EnvParams), alternative to the class table
// One lane per env; the step kernel's workgroups hold one integrating wavefront (launches below 65 536 envs: small
// batches spread over as many CUs as they have wavefronts) or four (one per SIMD of a CU), plus, in the wave-specialised
// thermal form, one producer wavefront each; the hot loops live entirely in registers.  With one device class the
// constants are read through scalar loads (SGPRs); with several each lane reads its row of derived constants from LDS;
// with per-env parameters each lane derives its constants from its env's record into registers (step kernel, MULTI == 2).
#include "stg_kernels.hpp"
#include "stg_wave.hpp"
#include "stg_switch.hpp"
#include "stg_switch_verify.hpp"

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

// ------------------------------------------------------------------------------------------------
// solver-level seam
// ------------------------------------------------------------------------------------------------
template <int SOLVER, bool THERMAL, bool MULTI, bool RECORD>
__global__ void __launch_bounds__(64) stg_solve_kernel(const SolveArgs a) {
    __shared__ double s_tab[MULTI ? STG_MAX_CLASSES * C_COUNT : 1];
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool in_range = i < a.N;
    const double* row = class_row<MULTI>(a.ctab, a.cls, a.ncls, i, in_range, s_tab, EnvParams{});
    if (!in_range) return;
    const int64_t N = a.N;
    const V3 m0{a.m0[i], a.m0[N + i], a.m0[2 * N + i]};
    const RngKey rk{a.c.seed, (uint64_t)(a.env_id0 + i), a.env_step};
    const Recorder rec{a.traj_t, a.traj_m, a.traj_e, a.traj_tq, N, i, a.traj_cap};
    InlineNormals ns;
    const SolveOut so = run_solver<SOLVER, THERMAL, RECORD, false, false>(m0, a.J[i], a.T[i], row, a.c, rk, rec, ns, true);
    a.m_final[i] = so.m.x; a.m_final[N + i] = so.m.y; a.m_final[2 * N + i] = so.m.z;
    if (a.n_points) a.n_points[i] = so.n;
    if (a.success) a.success[i] = so.ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// reset / state / diagnostics kernels
// ------------------------------------------------------------------------------------------------
struct ResetArgs {
    StateView s;
    CfgView c;
    int64_t N, env_id0;
    const double* ctab;
    const uint8_t* cls;
    int32_t ncls;
    const uint8_t* mask;
    const double *init_m, *target;
    uint64_t seed;
    float* obs;
    int32_t records;          // STG_OUT_RECORDS: obs is the record array
    EnvParams ep;
};

__global__ void __launch_bounds__(64) stg_reset_kernel(const ResetArgs a) {
    __shared__ double s_tab[STG_MAX_CLASSES * C_COUNT];
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool in_range = i < a.N;
    const double* row = (a.ncls > 1 || a.ep.rec) ? class_row<true>(a.ctab, a.cls, a.ncls, i, in_range, s_tab, a.ep, a.ep.layout) : a.ctab;
    if (!in_range) return;
    const int64_t N = a.N;
    V3 m0, t0;
    double etot0;
    int32_t step0;
    uint32_t rng0;
    bool done0;
    load_state(a.s, i, m0, t0, etot0, step0, rng0, done0);
    if (a.mask && !a.mask[i]) {
        if (a.obs) {   // unchanged env: report its current observation (last action unknown -> 0, as after reset)
            // (records: only the observation fields -- reward and flags of an env that is not reset are its last step's,
            // which the caller may still be reading: `reward`/`terminated` of SpinTorqueVecEnv.step are views of this array)
            if (a.records) write_record_obs(a.obs, i, m0, t0, row, a.c, step0, etot0, 0.0, 0.0);
            else write_obs(a.obs, N, i, m0, t0, row, a.c, step0, etot0, 0.0, 0.0);
        }
        return;
    }
    V3 m{0, 0, 1}, t{0, 0, 1};
    device_reset_draw(a.seed, (uint64_t)(a.env_id0 + i), rng0, a.c, a.init_m == nullptr, a.target == nullptr, m, t);
    if (a.init_m) {   // device.validate_magnetization (base_device.py:94-116): v / |v|
        const V3 v{a.init_m[i], a.init_m[N + i], a.init_m[2 * N + i]};
        const double n = sqrt(dot(v, v));
        m = V3{v.x / n, v.y / n, v.z / n};
    }
    if (a.target) {
        const V3 v{a.target[i], a.target[N + i], a.target[2 * N + i]};
        const double n = sqrt(dot(v, v));
        t = V3{v.x / n, v.y / n, v.z / n};
    }
    store_state(a.s, i, m, t, 0.0, 0, rng0, false);
    if (a.obs) {
        if (a.records) write_record(a.obs, i, m, t, row, a.c, 0, 0.0, 0.0, 0.0, 0.0f, 0u);
        else write_obs(a.obs, N, i, m, t, row, a.c, 0, 0.0, 0.0, 0.0);
    }
}

__global__ void stg_normals_kernel(uint64_t seed, int64_t env_id0, int64_t N, uint32_t env_step, uint32_t call0,
                                   int32_t n_calls, double* z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    NormalStream ns;
    ns.init(seed, (uint64_t)(env_id0 + i), env_step, 0u);
    for (uint32_t c = 0; c < call0 + (uint32_t)n_calls; ++c) {       // the stream is sequential: replay from call 0
        const V3 v = (c & 1u) ? ns.draw3_odd() : ns.draw3_even();
        if (c >= call0) {
            double* b = z + (int64_t)(c - call0) * 3 * N + i;
            b[0] = v.x; b[N] = v.y; b[2 * N] = v.z;
        }
    }
}

// stg_switch_population_devices: thread (g, j) dumps device dev0 + j of condition g through vary_draw, the trial kernel's own function
__global__ void stg_population_devices_kernel(uint64_t seed, int64_t env_id0, int32_t G, int64_t D, int64_t dev0, int64_t Q, int64_t trial_stride,
                                              uint32_t var_step, double z_clip, const double* sigma, const stg_device_params* ptab,
                                              const uint8_t* cond_cls, int32_t ncls, double* params, double* z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)G * D) return;
    const int64_t g = i / D, j = i % D;
    const int c = (cond_cls && ncls > 1) ? (int)cond_cls[g] : 0;
    double zz[6];
    stg_device_params p;
    vary_draw(seed, (uint64_t)vary_device_env(env_id0, g, trial_stride, dev0 + j, Q), var_step, ptab[c < ncls ? c : 0], sigma, G, g, z_clip, zz, p);
    const bool ok = vary_column_ok(sigma, G, g, z_clip);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double v[STG_NVARY] = {p.damping, p.ms, p.ku, p.volume, p.polarization};
    const int64_t n = (int64_t)G * D;
    for (int k = 0; k < STG_NVARY; ++k) params[k * n + i] = ok ? v[k] : nan;
    if (z)
        for (int k = 0; k < 6; ++k) z[k * n + i] = zz[k];
}

// stg_get_state / stg_set_state: between the library's state records and the caller's component-major arrays
// (m, target: double[3][N]; the others [N]; any may be NULL = field not copied)
template <bool SET>
__global__ void stg_state_copy_kernel(StateView s, int64_t N, double* m, double* target, double* etot, int32_t* step,
                                      uint32_t* rng, uint8_t* done) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    V3 mm, tt;
    double e;
    int32_t st;
    uint32_t r;
    bool d;
    load_state(s, i, mm, tt, e, st, r, d);
    if (SET) {
        if (m) mm = V3{m[i], m[N + i], m[2 * N + i]};
        if (target) tt = V3{target[i], target[N + i], target[2 * N + i]};
        if (etot) e = etot[i];
        if (step) st = step[i];
        if (rng) r = rng[i];
        if (done) d = done[i] != 0;
        store_state(s, i, mm, tt, e, st, r, d);
    } else {
        if (m) { m[i] = mm.x; m[N + i] = mm.y; m[2 * N + i] = mm.z; }
        if (target) { target[i] = tt.x; target[N + i] = tt.y; target[2 * N + i] = tt.z; }
        if (etot) etot[i] = e;
        if (step) step[i] = st;
        if (rng) rng[i] = r;
        if (done) done[i] = d ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// lane schedule: tile-local counting sort of the envs by this step's integration work (descending)
// ------------------------------------------------------------------------------------------------
// The trip count of a lane is set by its pulse duration (RK4: n = T/dt sub-steps; RK45: attempts ~ T / 0.65 ps), which
// the agent chooses per env: U[0.1, 1] ns gives a mean/max ratio of 0.55 inside a wavefront.  One kernel sorts each
// TILE of 4096 consecutive envs (= 64 wavefronts) by work in LDS (histogram -> scan -> scatter, no global atomics)
// and writes a tile-local permutation; slot j of the step launch then integrates env perm[j], so the lanes of a
// wavefront have (nearly) equal trip counts while every access of a wavefront stays inside its tile's 32 KB window of
// each SoA row.  The step kernel places a tile's 64 wavefronts on ONE XCD (stg_slot_block), whose L2 then merges the
// tile's scattered 4-8 B accesses into full lines before they reach HBM.

struct PlanArgs {
    const void* actions;      // [2][N] of the first fused step
    int32_t act_f64;
    int64_t N;
    double max_current, max_duration;
    const EnvRec* state;      // with skip_done: finished envs go last (no work)
    int32_t skip_done;
    const uint8_t* cls;       // device-physics torque model with several classes: group lanes by device kind
    const double* ctab;
    const uint8_t* env_type;  // (per-env parameters: the kind of each env)
    int32_t by_kind;
    int32_t regroup;          // (with by_kind) kind-pure groups of four blocks, renumbered by estimated cost; 0: kind-major order
    uint32_t* perm;
    void* act_sorted;         // [N][2] in the actions' dtype, slot order: the step kernel reads its action with one coalesced load
                              // instead of two scattered 4-byte reads through the permutation
    const uint32_t* ids;      // stg_step_ids (IDS kernel): N is the list length, i a list position, ids[i] its env (state, kind)
    int64_t n_state;          // ... the context's env count: an id beyond it is not dereferenced and sorts last (no work)
};

template <bool IDS>
__device__ __forceinline__ int plan_key(const PlanArgs& a, int64_t i) {
    double J, T;
    if (a.act_f64) parse_action<double>(((const double*)a.actions)[i], ((const double*)a.actions)[a.N + i], a.max_current, a.max_duration, J, T);
    else parse_action<float>(((const float*)a.actions)[i], ((const float*)a.actions)[a.N + i], a.max_current, a.max_duration, J, T);
    int64_t e = i;                                             // the env of list position i
    if constexpr (IDS) {
        const uint32_t id = a.ids[i];
        if ((int64_t)id >= a.n_state) return (a.by_kind ? PLAN_BUCKETS : PLAN_DUR) - 1;
        e = (int64_t)id;
    }
    if (a.skip_done && (a.state[e].stepw & STG_DONE_BIT)) return (a.by_kind ? PLAN_BUCKETS : PLAN_DUR) - 1;
    const double w = fmax(T, 1e-10) / a.max_duration;          // below 0.1 ns the RK4 sub-step count stays at ~100
    int b = (int)(w * (PLAN_DUR - 1));
    b = b < 0 ? 0 : (b > PLAN_DUR - 2 ? PLAN_DUR - 2 : b);
    const int kind = a.by_kind ? (a.env_type ? (int)a.env_type[e] : (int)a.ctab[(int)a.cls[e] * C_COUNT + C_DEVTYPE]) : 0;
    return kind * PLAN_DUR + (PLAN_DUR - 2) - b;               // descending work inside each kind: long pulses first
}

// IDS (stg_step_ids): the same sort over list positions 0..M); perm then maps a slot to a list position and act_sorted holds the actions of
// the list (read in list order), while the state and the device kind are read through ids.
template <bool IDS>
__global__ void __launch_bounds__(PLAN_THREADS) stg_plan_tile_kernel(const PlanArgs a) {
    __shared__ uint32_t cnt[PLAN_BUCKETS], start[PLAN_BUCKETS];
    const int nb = a.by_kind ? PLAN_BUCKETS : PLAN_DUR;       // buckets in use
    const int tid = threadIdx.x;
    if (tid < nb) cnt[tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * TILE_ENVS;
    uint32_t rank[PLAN_ITEMS];
    int key[PLAN_ITEMS];
#pragma unroll
    for (int r = 0; r < PLAN_ITEMS; ++r) {
        const int64_t i = base + r * PLAN_THREADS + tid;
        key[r] = -1;
        if (i < a.N) {
            key[r] = plan_key<IDS>(a, i);
            rank[r] = atomicAdd(&cnt[key[r]], 1u);             // rank inside the bucket (LDS atomic)
        }
    }
    __syncthreads();
    if (tid < nb) start[tid] = cnt[tid];
    __syncthreads();
    for (int off = 1; off < nb; off <<= 1) {                   // Hillis-Steele inclusive scan over the buckets
        uint32_t add = 0;
        if (tid < nb && tid >= off) add = start[tid - off];
        __syncthreads();
        if (tid < nb) start[tid] += add;
        __syncthreads();
    }
    // Grouped by device kind, the tile's slot sequence is one long-to-short ramp PER KIND, so its 64-slot blocks -- the step launch's
    // wavefronts, dealt longest rank first -- are not in order of work (the longest block of the last kind has rank ~43).  With
    // `regroup`, GROUPS OF FOUR consecutive blocks (= one 4-wavefront workgroup of the step launch) are renumbered longest-first again,
    // which is what the step kernel's schedule (stg_slot_block) assumes, while a workgroup's four wavefronts stay of one kind and of
    // nearly one duration -- they have to finish together for their four SIMD slots to come free together, and a sub-step of one
    // kind costs up to 1.5x that of another (renumbering single blocks mixed the kinds inside workgroups: 262 144 envs 0.72 -> 0.96 ms).
    // Without it the order stays kind-major: per-env records (then 64-thread workgroups) measured 131 072 envs 0.557 ms kind-major
    // against 0.745 ms with the rounds 2-3 grouping (groups keyed by their first env).
    __shared__ int grp_d[TILE_WAVES / 4];
    __shared__ uint8_t grp_rank[TILE_WAVES / 4];
    // Kind-pure groups.  A kind's ramp rarely ends on a group boundary (256 slots), so one group per boundary held the SHORT end of one
    // kind's ramp and the LONG start of the next: a 4-wavefront workgroup whose wavefronts run 150 ... 1000 sub-steps keeps its CU
    // slot until the longest is through.  Each kind therefore keeps a whole number of groups of its longest envs in place and hands
    // its remainder (< 256 slots, its SHORTEST envs) to a common tail behind all kinds: every group but the (at most three) tail
    // groups is of one kind and one duration, and the tail groups are short throughout.
    __shared__ uint32_t k_start[3], k_main[3], k_main_off[3], k_tail_off[3];
    const bool regroup = a.by_kind && a.regroup;
    if (regroup) {
        if (tid == 0) {
            uint32_t main_off = 0, tail_tot = 0, cnt_k[3];
            for (int k = 0; k < 3; ++k) {
                const uint32_t s0 = start[k * PLAN_DUR] - cnt[k * PLAN_DUR], e0 = start[(k + 1) * PLAN_DUR - 1];
                k_start[k] = s0; cnt_k[k] = e0 - s0;
                k_main[k] = cnt_k[k] & ~255u;
                k_main_off[k] = main_off; main_off += k_main[k];
            }
            for (int k = 0; k < 3; ++k) { k_tail_off[k] = main_off + tail_tot; tail_tot += cnt_k[k] - k_main[k]; }
        }
        __syncthreads();
    }
    auto slot_of = [&](int r) -> uint32_t {
        uint32_t sl = (start[key[r]] - cnt[key[r]]) + rank[r];                                     // exclusive start of the bucket + rank in it
        if (regroup) {
            const int k = key[r] / PLAN_DUR;
            const uint32_t pos = sl - k_start[k];
            sl = pos < k_main[k] ? k_main_off[k] + pos : k_tail_off[k] + (pos - k_main[k]);
        }
        return sl;
    };
    if (regroup) {
        constexpr int NG = TILE_WAVES / 4;
        if (tid < NG) grp_d[tid] = 0x7fffffff;                 // (groups beyond N: last)
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PLAN_ITEMS; ++r)
            if (key[r] >= 0) {
                const uint32_t sl = slot_of(r);
                // a group is keyed by its LONGEST block (keyed by its first env, a group that straddled the boundary between two kinds
                // sorted last and its long block then ran at the very end), at its estimated cost = duration x the kind's cost of a
                // sub-step (measured on homogeneous batches, profiles/r03_devphys_regroup.txt: STT 0.466, SOT 0.646, VCMA 0.419 ms per
                // step -> 32 : 44 : 29)
                const int dq = key[r] % PLAN_DUR, kind = key[r] / PLAN_DUR;
                const int f = kind == 1 ? 44 : (kind == 2 ? 29 : 32);
                if ((sl & 63u) == 0u) atomicMin(&grp_d[sl >> 8], (1 << 20) - (PLAN_DUR - dq) * f);
            }
        __syncthreads();
        // (a ragged tile's last, partly filled group keeps its place behind the full ones: the step kernel's "slot < N" test relies on
        // the tile's envs filling its first slots)
        const int64_t n_t = a.N - base < TILE_ENVS ? a.N - base : TILE_ENVS;
        if (tid == (int)(n_t >> 8) && (n_t & 255)) grp_d[tid] = 0x7ffffffe;
        __syncthreads();
        if (tid < NG) {
            const int d = grp_d[tid];
            int before = 0;
            for (int j = 0; j < NG; ++j) before += (grp_d[j] < d || (grp_d[j] == d && j < tid)) ? 1 : 0;
            grp_rank[tid] = (uint8_t)before;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < PLAN_ITEMS; ++r) {
        const int64_t i = base + r * PLAN_THREADS + tid;
        if (key[r] >= 0) {
            uint32_t sl = slot_of(r);
            if (regroup) sl = ((uint32_t)grp_rank[sl >> 8] << 8) | (sl & 255u);
            const int64_t slot = base + sl;
            a.perm[slot] = (uint32_t)i;
            if (a.act_f64) ((double2*)a.act_sorted)[slot] = make_double2(((const double*)a.actions)[i], ((const double*)a.actions)[a.N + i]);
            else ((float2*)a.act_sorted)[slot] = make_float2(((const float*)a.actions)[i], ((const float*)a.actions)[a.N + i]);
        }
    }
}

// device-class formulas evaluated per env (stg_device_terms)
__global__ void stg_device_terms_kernel(int64_t N, const double* ctab, const uint8_t* cls, int32_t ncls, const double* m,
                                        const double* J, const double* volt, double* tau_dl, double* tau_fl, double* k_eff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = (ncls > 1 && cls) ? (int)cls[i] : 0;
    const double* row = ctab + (c < ncls ? c : 0) * C_COUNT;
    const int kind = (int)row[C_DEVTYPE];
    if (tau_dl || tau_fl) {
        V3 dl{0.0, 0.0, 0.0}, fl{0.0, 0.0, 0.0};
        if (kind == STG_DEV_SOT) {      // sot_mram.py:186-192: tau_dl_factor*J*cross(sigma, m), tau_fl_factor*J*sigma
            const V3 mm{m[i], m[N + i], m[2 * N + i]}, sg{row[C_SIGX], row[C_SIGY], row[C_SIGZ]};
            const V3 sxm = cross(sg, mm);
            const double a = row[C_SOT_DL] * J[i], b = row[C_SOT_FL] * J[i];
            dl = V3{a * sxm.x, a * sxm.y, a * sxm.z};
            fl = V3{b * sg.x, b * sg.y, b * sg.z};
        }
        if (tau_dl) { tau_dl[i] = dl.x; tau_dl[N + i] = dl.y; tau_dl[2 * N + i] = dl.z; }
        if (tau_fl) { tau_fl[i] = fl.x; tau_fl[N + i] = fl.y; tau_fl[2 * N + i] = fl.z; }
    }
    if (k_eff)
        k_eff[i] = (kind == STG_DEV_VCMA) ? vcma_keff(volt[i], row[C_KU], row[C_VCMA_XI], row[C_VCMA_TD2], row[C_VCMA_VBD]) : row[C_KU];
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(STG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)

struct stg_ctx {
    int device;
    int64_t N, env_id0;
    stg_config cfg;
    StateView s{};
    void* slab = nullptr;
    double* ctab = nullptr;           // device, [ncls][C_COUNT]
    double h_ctab[STG_MAX_CLASSES][C_COUNT];
    stg_device_params* ptab = nullptr;   // device, [ncls]: the table as stg_set_params was given it (the nominal records of stg_switch_population)
    int32_t ncls = 0;
    const uint8_t* cls = nullptr;     // caller-owned device pointer
    unsigned long long* counters = nullptr;
    unsigned long long* refill_cursor = nullptr;   // the full step's refill launches: stripe cursors, then retire counters (each in a 128-byte line of its own);
                                                   // all 0 between launches (stg_kernels.hpp: refill_retire)
    uint32_t* placement = nullptr;    // [PLACEMENT_RING][PLACEMENT_WORDS]: where the wavefronts of the last launches ran (stg_get_placement)
    uint64_t launch_seq = 0;          // step launches so far
    uint32_t* perm = nullptr;
    void* act_sorted = nullptr;       // [N][2] actions of the step in slot order (written by the plan kernel)
    bool have_params = false, have_state = false;
    bool axis_z = false;              // every class has easy axis = +z exactly: the specialised Simple RHS applies
    bool axis_z_llgs = false;         // every class has raw easy axis (0,0,rz) and demag (0,0,Nz): specialised LLGS RHS
    // per-env parameters (stg_set_params_per_env): library-owned copies
    double* env_soa = nullptr;        // records [N][env_layout_doubles(env_layout)] (stg_kernels.hpp: EnvParams)
    int32_t env_layout = ENV_LAYOUT_CORE;
    uint8_t* env_type = nullptr;      // [N]: the device kind by itself, for the plan kernel (read in env order)
    bool per_env = false;
    // the pulse shape of stg_step_shaped (stg_set_pulse_shape): device copy in the slab, knot counts (both 0: none set)
    double* shape = nullptr;          // [STG_SHAPE_DOUBLES]: tau, scale, th, hk
    int32_t shape_kj = 0, shape_kh = 0;
    // the knot times of stg_step_knots (stg_set_pulse_knots): device copy in the slab, knot counts (knots_P 0: none set), amplitude clamp
    double* knots = nullptr;          // [STG_KNOTS_DOUBLES]: tau, th, hk
    int32_t knots_P = 0, knots_kh = 0;
    double knots_limit = 0.0;
};

static EnvParams env_params_of(const stg_ctx* ctx) {
    EnvParams e{};
    if (ctx->per_env) e.rec = ctx->env_soa;
    e.layout = ctx->env_layout;
    e.gamma = ctx->cfg.gamma; e.temperature = ctx->cfg.temperature;
    return e;
}

static CfgView cfg_view(const stg_config& c) {
    CfgView v{};
    v.temperature = c.temperature; v.max_step = c.max_step; v.rtol = c.rtol; v.atol = c.atol;
    v.max_current = c.max_current; v.max_duration = c.max_duration; v.thr = c.success_threshold;
    v.w_energy = c.energy_penalty_weight;
    v.inv_tau = c.solver == STG_SOLVER_RK45 ? 0.0 : (c.noise_model == 1 ? 1.0 / c.noise_corr_time : (c.noise_model == 2 ? -1.0 : 0.0));
    v.temp_norm = c.temperature / 300.0; v.inv_max_current = 1.0 / c.max_current; v.inv_max_duration = 1.0 / c.max_duration;
    std::memcpy(v.targets, c.targets, sizeof(v.targets));
    v.seed = c.seed; v.max_attempts = c.max_attempts; v.max_steps = c.max_steps; v.n_targets = c.n_targets;
    v.skip_done = c.skip_done;
    return v;
}

// the kernels' THERMAL flag: the fixed-step solvers draw a field only at a positive temperature, RK45 whenever thermal is on
static bool thermal_flag(const stg_config& c) {
    return c.solver == STG_SOLVER_RK45 ? c.thermal != 0 : (c.thermal && c.temperature > 0);
}

static int check_cfg(const stg_config* c) {
    if (!c) return fail(STG_E_INVALID, "cfg is NULL");
    if (c->solver < 0 || c->solver > 2) return fail(STG_E_INVALID, "cfg.solver must be STG_SOLVER_RK4/EULER/RK45");
    if (c->n_targets < 1 || c->n_targets > STG_MAX_TARGETS) return fail(STG_E_INVALID, "cfg.n_targets out of range");
    if (!(c->max_step > 0)) return fail(STG_E_INVALID, "cfg.max_step must be positive");
    if (c->max_steps < 1) return fail(STG_E_INVALID, "cfg.max_steps must be >= 1");
    if (!(c->max_current > 0) || !(c->max_duration > 0)) return fail(STG_E_INVALID, "cfg.max_current/max_duration must be positive");
    if (c->solver == STG_SOLVER_RK45 && (!(c->rtol > 0) || !(c->atol >= 0))) return fail(STG_E_INVALID, "cfg.rtol/atol invalid");
    if (c->noise_model < 0 || c->noise_model > 2) return fail(STG_E_INVALID, "cfg.noise_model must be 0 (white), 1 (Ornstein-Uhlenbeck) or 2 (Brown, 1/sqrt(dt))");
    if (c->noise_model == 1 && c->solver == STG_SOLVER_RK45) return fail(STG_E_INVALID, "cfg.noise_model = 1 needs a fixed-step solver (RK4 or Euler)");
    if (c->noise_model == 2 && c->solver == STG_SOLVER_RK45) return fail(STG_E_INVALID, "cfg.noise_model = 2 needs a fixed-step solver (RK4 or Euler)");
    if (c->noise_model == 1 && !(c->noise_corr_time > 0)) return fail(STG_E_INVALID, "cfg.noise_corr_time must be positive");
    // (the kernels count attempts in 32 bits)
    if (c->solver == STG_SOLVER_RK45 && (c->max_attempts < 1 || c->max_attempts > INT32_MAX)) return fail(STG_E_INVALID, "cfg.max_attempts must be in 1 ... 2^31 - 1");
    if (c->torque_model < 0 || c->torque_model > 1) return fail(STG_E_INVALID, "cfg.torque_model must be 0 or 1");
    if (c->out_layout != STG_OUT_SOA && c->out_layout != STG_OUT_RECORDS) return fail(STG_E_INVALID, "cfg.out_layout must be STG_OUT_SOA or STG_OUT_RECORDS");
    if (c->lane_refill < -1 || c->lane_refill == 1 || c->lane_refill > 1024) return fail(STG_E_INVALID, "cfg.lane_refill must be -1 (never), 0 (automatic) or the number of envs per lane (2..1024)");
    if (c->reserved0 != 0) return fail(STG_E_INVALID, "cfg.reserved0 must be 0");
    if (c->torque_model == 1 && c->solver == STG_SOLVER_RK45)
        return fail(STG_E_INVALID, "the device-physics torque model is implemented for the fixed-step solvers (rk4, euler)");
    return STG_OK;
}

extern "C" {

int stg_internal_fail(int code, const char* msg) { return fail(code, msg ? msg : ""); }   // used by stg_array.hip
const char* stg_last_error(void) { return g_err.c_str(); }
int stg_abi_version(void) { return STG_ABI_VERSION; }

int stg_create(stg_ctx** out, int device_id, int64_t n_envs, int64_t env_id0, const stg_config* cfg) {
    if (!out) return fail(STG_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_envs < 1) return fail(STG_E_INVALID, "n_envs must be >= 1");
    if (env_id0 < 0) return fail(STG_E_INVALID, "env_id0 must be >= 0");
    if (int rc = check_cfg(cfg)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(STG_E_INVALID, "device_id out of range");
    HIP_TRY(hipSetDevice(device_id));
    stg_ctx* c = new (std::nothrow) stg_ctx();
    if (!c) return fail(STG_E_NOMEM, "out of host memory");
    c->device = device_id; c->N = n_envs; c->env_id0 = env_id0; c->cfg = *cfg;
    // per-env parameter records hold what this context's kernels read: their solver and torque model are fixed here
    c->env_layout = cfg->solver == STG_SOLVER_RK45 ? ENV_LAYOUT_LLGS : (cfg->torque_model == 1 ? ENV_LAYOUT_DEV : ENV_LAYOUT_CORE);
    // one slab: the state records, the class table, the counter stripes, the lane permutation (each 256-B aligned)
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t N = (size_t)n_envs;
    const size_t rs = al(N * sizeof(EnvRec)), r4 = al(N * 4), ra = al(N * 16);
    const size_t rp = al(sizeof(uint32_t) * PLACEMENT_RING * PLACEMENT_WORDS);
    const size_t rc = al(2 * REFILL_STRIPES * REFILL_CURSOR_STRIDE * sizeof(unsigned long long));
    const size_t total = rs + r4 + ra + rp + rc + al(sizeof(double) * STG_MAX_CLASSES * C_COUNT) +
                         COUNTER_STRIPES * COUNTER_STRIDE * sizeof(unsigned long long) + al(sizeof(double) * STG_SHAPE_DOUBLES) +
                         al(sizeof(double) * STG_KNOTS_DOUBLES) + al(sizeof(stg_device_params) * STG_MAX_CLASSES);
    hipError_t e = hipMalloc(&c->slab, total);
    if (e != hipSuccess) { delete c; return fail(STG_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    e = hipMemset(c->slab, 0, total);
    if (e != hipSuccess) { (void)hipFree(c->slab); delete c; return fail(STG_E_HIP, std::string("hipMemset: ") + hipGetErrorString(e)); }
    char* p = (char*)c->slab;
    c->s.rec = (EnvRec*)p; p += rs;
    c->ctab = (double*)p; p += al(sizeof(double) * STG_MAX_CLASSES * C_COUNT);
    c->counters = (unsigned long long*)p; p += COUNTER_STRIPES * COUNTER_STRIDE * sizeof(unsigned long long);
    c->perm = (uint32_t*)p; p += r4;
    c->act_sorted = (void*)p; p += ra;
    c->placement = (uint32_t*)p; p += rp;
    c->refill_cursor = (unsigned long long*)p; p += rc;
    c->shape = (double*)p; p += al(sizeof(double) * STG_SHAPE_DOUBLES);
    c->knots = (double*)p; p += al(sizeof(double) * STG_KNOTS_DOUBLES);
    c->ptab = (stg_device_params*)p; p += al(sizeof(stg_device_params) * STG_MAX_CLASSES);
    *out = c;
    return STG_OK;
}

void stg_destroy(stg_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->slab) (void)hipFree(ctx->slab);
    if (ctx->env_soa) (void)hipFree(ctx->env_soa);
    if (ctx->env_type) (void)hipFree(ctx->env_type);
    delete ctx;
}

static void derive_class(const stg_device_params& p, const stg_config& cfg, double* r) {
    derive_row(p, cfg.gamma, cfg.temperature, r);      // stg_physics.hpp (shared with the per-env device path)
}

int stg_set_params(stg_ctx* ctx, const stg_device_params* table, int32_t n_classes, const uint8_t* cls) {
    if (!ctx || !table) return fail(STG_E_INVALID, "ctx/table is NULL");
    if (n_classes < 1 || n_classes > STG_MAX_CLASSES) return fail(STG_E_INVALID, "n_classes must be in [1, STG_MAX_CLASSES]");
    if (n_classes > 1 && !cls) return fail(STG_E_INVALID, "cls is required when n_classes > 1");
    for (int k = 0; k < n_classes; ++k) {
        const stg_device_params& p = table[k];
        if (p.dev_type < 0 || p.dev_type > 2) return fail(STG_E_INVALID, "dev_type must be STG_DEV_STT/SOT/VCMA");
        // BaseSpintronicDevice/STTMRAMDevice._validate_parameters raise on these at construction
        // (devices/stt_mram.py:46-53); the host mirror raises before getting here.
        if (!(p.volume > 0) || !(p.ms > 0)) return fail(STG_E_INVALID, "volume and saturation_magnetization must be positive");
        derive_class(p, ctx->cfg, ctx->h_ctab[k]);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(ctx->ctab, ctx->h_ctab, sizeof(double) * n_classes * C_COUNT, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->ptab, table, sizeof(stg_device_params) * n_classes, hipMemcpyHostToDevice));
    ctx->ncls = n_classes;
    ctx->axis_z = true;
    for (int k = 0; k < n_classes; ++k)
        ctx->axis_z = ctx->axis_z && ctx->h_ctab[k][C_EX] == 0.0 && ctx->h_ctab[k][C_EY] == 0.0 && ctx->h_ctab[k][C_EZ] == 1.0;
    ctx->axis_z_llgs = true;
    for (int k = 0; k < n_classes; ++k) {
        const double* r = ctx->h_ctab[k];
        ctx->axis_z_llgs = ctx->axis_z_llgs && r[C_RX] == 0.0 && r[C_RY] == 0.0 && r[C_DX] == 0.0 && r[C_DY] == 0.0;
    }
    ctx->cls = n_classes > 1 ? cls : nullptr;
    ctx->per_env = false;
    ctx->have_params = true;
    return STG_OK;
}

// rows of the caller's structure of arrays -> the library's per-env records (once per stg_set_params_per_env)
__global__ void stg_env_pack_kernel(const double* soa, const uint8_t* type, const uint8_t* valid, int64_t N, double* rec, int layout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    // rows of the caller's block = the double fields of stg_device_params in declaration order (include/spintorque_hip.h):
    // 0 damping, 1 ms, 2 ku, 3 volume, 4 polarization, 5-7 easy_axis, 8-10 demag, 11 a_ex, 12 area, 13 r_p, 14 r_ap, 15-17 ref_m,
    // 18 r_series, 19 sot_tau_dl, 20 sot_tau_fl, 21-23 sot_sigma, 24 vcma_xi, 25 vcma_td, 26 vcma_vbd, 27-29 shape_demag
    constexpr int core[15] = {0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18};
    constexpr int llgs[4] = {8, 9, 10, 11};
    constexpr int dev[8] = {19, 20, 21, 22, 23, 24, 25, 26};
    double* r = rec + i * env_layout_doubles(layout);
    for (int k = 0; k < 15; ++k) r[k] = soa[(int64_t)core[k] * N + i];
    r[15] = (double)((int)(type[i] & 3) + 4 * (valid[i] ? 1 : 0));
    if (layout == ENV_LAYOUT_LLGS) for (int k = 0; k < 4; ++k) r[16 + k] = soa[(int64_t)llgs[k] * N + i];
    if (layout == ENV_LAYOUT_DEV) for (int k = 0; k < 8; ++k) r[16 + k] = soa[(int64_t)dev[k] * N + i];
}

// axis flags of a per-env parameter block: flag[0] = some env's easy axis is not exactly +z after normalisation,
// flag[1] = some env's raw axis or demag factors have x/y components (LLGS specialisation)
__global__ void stg_env_axis_kernel(const double* soa, int64_t N, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double ex = soa[5 * N + i], ey = soa[6 * N + i], ez = soa[7 * N + i];
    const double dx = soa[8 * N + i], dy = soa[9 * N + i];
    const double en = sqrt((ex * ex + ey * ey) + ez * ez);
    if (!(ex / en == 0.0 && ey / en == 0.0 && ez / en == 1.0)) flag[0] = 1;
    if (!(ex == 0.0 && ey == 0.0 && -dx == 0.0 && -dy == 0.0)) flag[1] = 1;
}

int stg_set_params_per_env(stg_ctx* ctx, const double* soa_params, const uint8_t* dev_type, const uint8_t* params_valid) {
    if (!ctx || !soa_params || !dev_type || !params_valid) return fail(STG_E_INVALID, "ctx/soa_params/dev_type/params_valid is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t N = (size_t)ctx->N;
    if (!ctx->env_soa) {
        // both buffers or neither: a context is never left with one of them set
        double* soa = nullptr;
        uint8_t* bytes = nullptr;
        HIP_TRY(hipMalloc(&soa, sizeof(double) * env_layout_doubles(ctx->env_layout) * N));
        const hipError_t e2 = hipMalloc(&bytes, N);
        if (e2 != hipSuccess) {
            (void)hipFree(soa);
            return fail(STG_E_NOMEM, std::string("hipMalloc(env_type): ") + hipGetErrorString(e2));
        }
        ctx->env_soa = soa;
        ctx->env_type = bytes;
    }
    hipLaunchKernelGGL(stg_env_pack_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, soa_params, dev_type, params_valid,
                       (int64_t)N, ctx->env_soa, (int)ctx->env_layout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(ctx->env_type, dev_type, N, hipMemcpyDeviceToDevice));
    // the specialised right-hand sides apply only if EVERY env has the default axis geometry
    int32_t h_flag[2] = {0, 0};
    int32_t* d_flag = nullptr;
    HIP_TRY(hipMalloc(&d_flag, 8));
    hipError_t ef = hipMemset(d_flag, 0, 8);
    if (ef == hipSuccess) {
        hipLaunchKernelGGL(stg_env_axis_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, soa_params, (int64_t)N, d_flag);
        ef = hipMemcpy(h_flag, d_flag, 8, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_flag);                                  // on every path
    if (ef != hipSuccess) return fail(STG_E_HIP, std::string("axis flags: ") + hipGetErrorString(ef));
    ctx->axis_z = h_flag[0] == 0;
    ctx->axis_z_llgs = h_flag[1] == 0;
    ctx->ncls = 0; ctx->cls = nullptr;
    ctx->per_env = true;
    ctx->have_params = true;
    return STG_OK;
}

int stg_thermal_strength(stg_ctx* ctx, int32_t cls, double* out) {
    if (!ctx || !out) return fail(STG_E_INVALID, "ctx/out is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, "stg_set_params has not been called");
    if (ctx->per_env) return fail(STG_E_STATE, "per-env parameters have no class table");
    if (cls < 0 || cls >= ctx->ncls) return fail(STG_E_INVALID, "cls out of range");
    *out = ctx->h_ctab[cls][ctx->cfg.solver == STG_SOLVER_RK45 ? C_HS_LLGS : C_HS_SIMPLE];
    return STG_OK;
}

static inline dim3 grid_for(int64_t N) { return dim3((unsigned)((N + 63) / 64)); }

int stg_reset(stg_ctx* ctx, const uint8_t* mask, const double* init_m, const double* target, uint64_t seed,
              float* obs_out, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, "stg_set_params must be called before stg_reset");
    if (ctx->cfg.out_layout == STG_OUT_RECORDS && ((uintptr_t)obs_out & 7u))
        return fail(STG_E_INVALID, "the record array must be 8-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    ResetArgs a{};
    a.s = ctx->s; a.c = cfg_view(ctx->cfg); a.N = ctx->N; a.env_id0 = ctx->env_id0;
    a.ctab = ctx->ctab; a.cls = ctx->cls; a.ncls = ctx->ncls; a.ep = env_params_of(ctx);
    a.mask = mask; a.init_m = init_m; a.target = target; a.seed = seed; a.obs = obs_out;
    a.records = ctx->cfg.out_layout == STG_OUT_RECORDS ? 1 : 0;
    hipLaunchKernelGGL(stg_reset_kernel, grid_for(ctx->N), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    ctx->have_state = true;
    return STG_OK;
}

// stg_step_ids's workspace (caller-owned, one per launch in flight): slot -> list position, the slot-order actions, the refill launch's
// cursor set and, in a second block of the same size, its retire counters (both zeroed on the launch's stream).  The offsets grow with
// M, so a workspace sized for M serves every smaller list.
struct IdsWorkspace {
    uint32_t* perm;
    void* act_sorted;
    unsigned long long *cursor, *done;
    size_t cursor_bytes, bytes;
};
static IdsWorkspace ids_workspace(void* base, int64_t M) {
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    IdsWorkspace w{};
    const size_t rp = al((size_t)M * 4), ra = al((size_t)M * 16);
    w.cursor_bytes = al(REFILL_STRIPES * REFILL_CURSOR_STRIDE * sizeof(unsigned long long));
    char* p = (char*)base;
    w.perm = (uint32_t*)p;
    w.act_sorted = (void*)(p + rp);
    w.cursor = (unsigned long long*)(p + rp + ra);
    w.done = (unsigned long long*)(p + rp + ra + w.cursor_bytes);
    w.bytes = rp + ra + 2 * w.cursor_bytes;
    return w;
}

// the output pointers of a step launch: the NULL / alignment rules of the context's output layout, then into the kernel's arguments
static int step_outputs(const stg_ctx* ctx, StepArgs& a, float* obs, float* final_obs, float* reward, double* reward_f64, double* energy,
                        uint8_t* terminated, uint8_t* truncated, uint8_t* status) {
    const bool records = ctx->cfg.out_layout == STG_OUT_RECORDS;
    if (!records && (!reward || !terminated || !truncated)) return fail(STG_E_INVALID, "reward/terminated/truncated must not be NULL (cfg.out_layout = STG_OUT_SOA)");
    if (records && ((uintptr_t)obs & 7u)) return fail(STG_E_INVALID, "the record array must be 8-byte aligned");
    if (records && ((uintptr_t)final_obs & 7u)) return fail(STG_E_INVALID, "final_obs must be 8-byte aligned (cfg.out_layout = STG_OUT_RECORDS)");
    a.records = records ? 1 : 0;
    a.obs = obs; a.final_obs = final_obs; a.reward = reward; a.reward64 = reward_f64; a.energy = energy; a.term = terminated; a.trunc = truncated; a.status = status;
    return STG_OK;
}

// the context-owned fields of a step launch's arguments: state, config, env ids, class table, counters
static void step_context(const stg_ctx* ctx, StepArgs& a) {
    a.s = ctx->s; a.c = cfg_view(ctx->cfg); a.env_id0 = ctx->env_id0;
    a.ctab = ctx->ctab; a.cls = ctx->cls; a.ncls = ctx->ncls;
    a.counters = ctx->counters;
}

// Enqueues one step launch.  `a` arrives with what the entry point decides (N = the launch's slots, K, out_every, autoreset, actions,
// outputs, ids / n_state); the rest comes from the context and from the launch plan (stg_launch_plan.hpp).  ws: the workspace of an
// id launch, nullptr for the full step, which uses the context's own buffers.
static int enqueue_step(stg_ctx* ctx, StepArgs& a, int32_t act_f64, const IdsWorkspace* ws, hipStream_t st) {
    step_context(ctx, a);
    a.ep = env_params_of(ctx);
    a.placement = ctx->placement + (size_t)(ctx->launch_seq % PLACEMENT_RING) * PLACEMENT_WORDS;
    ctx->launch_seq += 1;
    StepPlan p;
    const char* err = "";
    if (int rc = plan_step(ctx->cfg, a.N, a.K, a.autoreset != 0, ws != nullptr, ctx->per_env, ctx->ncls, ctx->cls != nullptr, &p, &err)) return fail(rc, err);
    if (p.sort) {
        PlanArgs pa{};
        pa.actions = a.actions; pa.act_f64 = act_f64; pa.N = a.N; pa.ids = a.ids; pa.n_state = a.n_state;
        pa.max_current = ctx->cfg.max_current; pa.max_duration = ctx->cfg.max_duration;
        pa.state = ctx->s.rec; pa.skip_done = p.skip_done;
        pa.perm = ws ? ws->perm : ctx->perm; pa.act_sorted = ws ? ws->act_sorted : ctx->act_sorted;
        pa.cls = ctx->cls; pa.ctab = ctx->ctab;
        pa.env_type = ctx->per_env ? ctx->env_type : nullptr;
        pa.by_kind = p.by_kind; pa.regroup = p.regroup;
        const dim3 g((unsigned)((a.N + TILE_ENVS - 1) / TILE_ENVS));
        with_flag(ws != nullptr, [&](auto IDS) { hipLaunchKernelGGL(stg_plan_tile_kernel<IDS.value>, g, dim3(PLAN_THREADS), 0, st, pa); });
        a.perm = pa.perm;
        a.act_sorted = pa.act_sorted;
    }
    a.hybrid = p.hybrid;
    a.refill = p.refill; a.refill_check = p.refill_check; a.refill_nw = p.refill_nw;
    if (p.refill) {
        // Every refill launch leaves its cursors and retire counters at 0 (refill_retire), so the full step, whose launches are ordered,
        // finds the context's own set at 0 -- zeroed by stg_create, then by each launch -- and bakes nothing but two pointers into a captured
        // launch.  An id launch has its set in the caller's workspace, whose content is the caller's: zeroed on the launch's stream.
        if (ws) {
            HIP_TRY(hipMemsetAsync(ws->cursor, 0, 2 * ws->cursor_bytes, st));
            a.refill_cursor = ws->cursor;
            a.refill_done = ws->done;
        } else {
            a.refill_cursor = ctx->refill_cursor;
            a.refill_done = ctx->refill_cursor + REFILL_STRIPES * REFILL_CURSOR_STRIDE;
        }
        stg_dispatch_step_rk45_refill(a, p.thermal, p.multi != 0, ctx->axis_z_llgs, act_f64, st);
    } else {
        switch (ctx->cfg.solver) {
            case STG_SOLVER_RK4: stg_dispatch_step_rk4(a, p.thermal, p.multi, ctx->axis_z, p.devphys, act_f64, p.pc, st); break;
            case STG_SOLVER_EULER: stg_dispatch_step_euler(a, p.thermal, p.multi, ctx->axis_z, p.devphys, act_f64, p.pc, st); break;
            default: stg_dispatch_step_rk45(a, p.thermal, p.multi, ctx->axis_z_llgs, act_f64, p.pc, st); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_step_many(stg_ctx* ctx, int32_t K, const void* actions, int32_t act_f64, int32_t out_every, int32_t autoreset,
                  float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                  uint8_t* truncated, uint8_t* status, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params || !ctx->have_state) return fail(STG_E_STATE, "stg_set_params and stg_reset must precede stg_step");
    if (K < 1) return fail(STG_E_INVALID, "K must be >= 1");
    if (!actions || !obs) return fail(STG_E_INVALID, "actions/obs must not be NULL");
    StepArgs a{};
    if (int rc = step_outputs(ctx, a, obs, final_obs, reward, reward_f64, energy, terminated, truncated, status)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    a.N = ctx->N; a.actions = actions; a.K = K; a.out_every = out_every ? 1 : 0; a.autoreset = autoreset ? 1 : 0;
    return enqueue_step(ctx, a, act_f64, nullptr, (hipStream_t)stream);
}

int stg_step(stg_ctx* ctx, const void* actions, int32_t act_f64, float* obs, float* reward, double* reward_f64,
             double* energy, uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream) {
    return stg_step_many(ctx, 1, actions, act_f64, 1, 0, obs, nullptr, reward, reward_f64, energy, terminated, truncated,
                         status, stream);
}

size_t stg_step_ids_workspace_bytes(const stg_ctx* ctx, int64_t M) {
    if (!ctx || M < 1) return 0;
    return ids_workspace(nullptr, M).bytes;
}

// One env-step of the M envs env_ids: the schedule is decided by M as stg_step_many decides it by N (results do not depend on it)
int stg_step_ids(stg_ctx* ctx, int64_t M, const uint32_t* env_ids, const void* actions, int32_t act_f64, int32_t autoreset,
                 void* workspace, float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                 uint8_t* truncated, uint8_t* status, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params || !ctx->have_state) return fail(STG_E_STATE, "stg_set_params and stg_reset must precede stg_step_ids");
    if (M < 1 || M > 0xFFFFFFFFll) return fail(STG_E_INVALID, "M must be in [1, 2^32)");
    if (!env_ids || !actions || !obs || !workspace) return fail(STG_E_INVALID, "env_ids/actions/obs/workspace must not be NULL");
    if ((uintptr_t)workspace & 15u) return fail(STG_E_INVALID, "the workspace must be 16-byte aligned");
    StepArgs a{};
    if (int rc = step_outputs(ctx, a, obs, final_obs, reward, reward_f64, energy, terminated, truncated, status)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const IdsWorkspace ws = ids_workspace(workspace, M);
    a.N = M; a.ids = env_ids; a.n_state = ctx->N;
    a.actions = actions; a.K = 1; a.out_every = 1; a.autoreset = autoreset ? 1 : 0;
    return enqueue_step(ctx, a, act_f64, &ws, (hipStream_t)stream);
}

// One env step of all N envs with the drive of stg_solve_wave; its kernel lives in stg_step_wave.hip (stg_step_wave_launch).  Everything
// arrives as arguments: one kernel, identity order, no plan kernel and none of the context's launch scratch.
int stg_step_wave(stg_ctx* ctx, const void* actions, int32_t act_f64, int32_t autoreset, int32_t kj, const double* tj, const double* jk,
                  int32_t kh, const double* th, const double* hk, float* obs, float* final_obs, float* reward, double* reward_f64,
                  double* energy, uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params || !ctx->have_state) return fail(STG_E_STATE, "stg_set_params and stg_reset must precede stg_step_wave");
    if (ctx->per_env) return fail(STG_E_STATE, "stg_step_wave works on the class table (stg_set_params), not on per-env parameters");
    if (ctx->cfg.torque_model == 1) return fail(STG_E_INVALID, "stg_step_wave implements the reference torque model (cfg.torque_model = 0)");
    if (!actions || !obs) return fail(STG_E_INVALID, "actions/obs must not be NULL");
    if (kj != 0 && (kj < 2 || kj > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kj must be 0 or 2 ... STG_MAX_KNOTS");
    if (kh != 0 && (kh < 2 || kh > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kh must be 0 or 2 ... STG_MAX_KNOTS");
    if (kj != 0 && (!tj || !jk)) return fail(STG_E_INVALID, "tj/jk must not be NULL with kj > 0");
    if (kh != 0 && (!th || !hk)) return fail(STG_E_INVALID, "th/hk must not be NULL with kh > 0");
    WaveStepArgs w{};
    StepArgs& a = w.s;
    if (int rc = step_outputs(ctx, a, obs, final_obs, reward, reward_f64, energy, terminated, truncated, status)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    step_context(ctx, a);
    a.N = ctx->N; a.actions = actions; a.K = 1; a.out_every = 1; a.autoreset = autoreset ? 1 : 0;
    w.kj = kj; w.tj = tj; w.jk = jk; w.kh = kh; w.th = th; w.hk = hk;
    const bool rk45 = ctx->cfg.solver == STG_SOLVER_RK45;
    w.axis_z = (rk45 ? ctx->axis_z_llgs : ctx->axis_z) ? 1 : 0;
    stg_step_wave_launch(w, ctx->cfg.solver, thermal_flag(ctx->cfg), ctx->ncls > 1, act_f64, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

// What stg_set_pulse_shape and stg_set_pulse_knots check alike.  Everything is checked on the host, before the context is looked at: a
// refused call leaves what was set in force.  scale: the shape's amplitudes, nullptr for the knots, which have none of their own.
static int check_tau(int32_t n, const double* tau, const double* scale) {
    for (int32_t j = 0; j < n; ++j) {
        if (!std::isfinite(tau[j]) || (scale && !std::isfinite(scale[j]))) return fail(STG_E_INVALID, scale ? "tau/scale must be finite" : "tau must be finite");
        if (tau[j] < 0.0 || tau[j] > 1.0) return fail(STG_E_INVALID, "tau is normalised time: every knot must lie in [0, 1]");
        if (j > 0 && !(tau[j] > tau[j - 1])) return fail(STG_E_INVALID, "tau must be strictly increasing");
    }
    return STG_OK;
}
static int check_field_table(int32_t kh, const double* th, const double* hk) {
    for (int32_t j = 0; j < kh; ++j) {
        if (!std::isfinite(th[j]) || !std::isfinite(hk[3 * j]) || !std::isfinite(hk[3 * j + 1]) || !std::isfinite(hk[3 * j + 2]))
            return fail(STG_E_INVALID, "th/hk must be finite");
        if (j > 0 && !(th[j] > th[j - 1])) return fail(STG_E_INVALID, "th must be strictly increasing");
    }
    return STG_OK;
}

// The env-level drive of stg_step_shaped.
int stg_set_pulse_shape(stg_ctx* ctx, int32_t kj, const double* tau, const double* scale, int32_t kh, const double* th, const double* hk) {
    if (kj != 0 && (kj < 2 || kj > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kj must be 0 or 2 ... STG_MAX_KNOTS");
    if (kh != 0 && (kh < 2 || kh > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kh must be 0 or 2 ... STG_MAX_KNOTS");
    if (kj != 0 && (!tau || !scale)) return fail(STG_E_INVALID, "tau/scale must not be NULL with kj > 0");
    if (kh != 0 && (!th || !hk)) return fail(STG_E_INVALID, "th/hk must not be NULL with kh > 0");
    if (int rc = check_tau(kj, tau, scale)) return rc;
    if (int rc = check_field_table(kh, th, hk)) return rc;
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (kj != 0 || kh != 0) {
        double h[STG_SHAPE_DOUBLES] = {};
        for (int32_t j = 0; j < kj; ++j) { h[j] = tau[j]; h[STG_MAX_KNOTS + j] = scale[j]; }
        for (int32_t j = 0; j < kh; ++j) {
            h[2 * STG_MAX_KNOTS + j] = th[j];
            for (int c = 0; c < 3; ++c) h[3 * STG_MAX_KNOTS + 3 * j + c] = hk[3 * j + c];
        }
        // (a launch that still reads the old shape finishes first: streams created non-blocking do not wait for the copy by themselves)
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(ctx->shape, h, sizeof(h), hipMemcpyHostToDevice));
    }
    ctx->shape_kj = kj; ctx->shape_kh = kh;
    return STG_OK;
}

// The knot times and the field table of stg_step_knots.
int stg_set_pulse_knots(stg_ctx* ctx, int32_t P, const double* tau, double s_limit, int32_t kh, const double* th, const double* hk) {
    if (P != 0 && (P < 2 || P > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "P must be 0 or 2 ... STG_MAX_KNOTS");
    if (kh != 0 && (kh < 2 || kh > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kh must be 0 or 2 ... STG_MAX_KNOTS");
    if (P != 0 && !tau) return fail(STG_E_INVALID, "tau must not be NULL with P > 0");
    if (P != 0 && kh != 0 && (!th || !hk)) return fail(STG_E_INVALID, "th/hk must not be NULL with kh > 0");
    if (P != 0 && !(std::isfinite(s_limit) && s_limit > 0.0)) return fail(STG_E_INVALID, "s_limit must be finite and positive");
    if (int rc = check_tau(P, tau, nullptr)) return rc;
    if (int rc = check_field_table(P != 0 ? kh : 0, th, hk)) return rc;
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (P == 0) {                                          // cleared: the step entries return STG_E_STATE until knots are set again
        ctx->knots_P = 0; ctx->knots_kh = 0; ctx->knots_limit = 0.0;
        return STG_OK;
    }
    double h[STG_KNOTS_DOUBLES] = {};
    for (int32_t j = 0; j < P; ++j) h[j] = tau[j];
    for (int32_t j = 0; j < kh; ++j) {
        h[STG_MAX_KNOTS + j] = th[j];
        for (int c = 0; c < 3; ++c) h[2 * STG_MAX_KNOTS + 3 * j + c] = hk[3 * j + c];
    }
    // (a launch that still reads the old knots finishes first: streams created non-blocking do not wait for the copy by themselves)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ctx->knots, h, sizeof(h), hipMemcpyHostToDevice));
    ctx->knots_P = P; ctx->knots_kh = kh; ctx->knots_limit = s_limit;
    return STG_OK;
}

// The pulse-step entries -- stg_step_shaped / _ids and stg_step_knots / _ids -- are one host path over the argument block of their
// policy (stg_wave.hpp; the one kernel: stg_step_pulse.hpp).  Identity order, so none of the context's launch scratch is used and the
// placement ring is left alone.
// what the context has staged for each of them, into a launch's arguments (false: nothing is set)
static bool pulse_table(const stg_ctx* ctx, ShapedStepArgs& w) {
    w.kj = ctx->shape_kj; w.kh = ctx->shape_kh; w.tab = ctx->shape;
    return w.kj != 0 || w.kh != 0;
}
static bool pulse_table(const stg_ctx* ctx, KnotsStepArgs& w) {
    w.kj = ctx->knots_P; w.kh = ctx->knots_kh; w.s_limit = ctx->knots_limit; w.tab = ctx->knots;
    return w.kj != 0;
}
// the checks that need no list
static int pulse_checks(const stg_ctx* ctx, const char* who, const char* setter, bool is_set) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params || !ctx->have_state) return fail(STG_E_STATE, std::string("stg_set_params and stg_reset must precede ") + who);
    if (ctx->per_env) return fail(STG_E_STATE, std::string(who) + " works on the class table (stg_set_params), not on per-env parameters");
    if (ctx->cfg.torque_model == 1) return fail(STG_E_INVALID, std::string(who) + " implements the reference torque model (cfg.torque_model = 0)");
    if (!is_set) return fail(STG_E_STATE, std::string(setter) + " must precede " + who);
    return STG_OK;
}
extern "C++" {
// `w` arrives with the staged table and, in w.s, N (slots), K, out_every, autoreset, actions, ids / n_state and the outputs
template <class ARGS>
static int enqueue_pulse(stg_ctx* ctx, ARGS& w, int32_t act_f64, hipStream_t st) {
    HIP_TRY(hipSetDevice(ctx->device));
    step_context(ctx, w.s);
    stg_step_pulse_launch(w, ctx->cfg.solver, thermal_flag(ctx->cfg), ctx->ncls > 1, act_f64, st);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}
// the K form: all N envs, K steps
template <class ARGS>
static int pulse_step_many(stg_ctx* ctx, const char* who, const char* setter, int32_t K, const void* actions, int32_t act_f64, int32_t out_every,
                           int32_t autoreset, float* obs, float* final_obs, float* reward, double* reward_f64, double* energy,
                           uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream) {
    ARGS w{};
    StepArgs& a = w.s;
    if (int rc = pulse_checks(ctx, who, setter, ctx && pulse_table(ctx, w))) return rc;
    if (K < 1) return fail(STG_E_INVALID, "K must be >= 1");
    if (!actions || !obs) return fail(STG_E_INVALID, "actions/obs must not be NULL");
    if (int rc = step_outputs(ctx, a, obs, final_obs, reward, reward_f64, energy, terminated, truncated, status)) return rc;
    a.N = ctx->N; a.actions = actions; a.K = K; a.out_every = out_every ? 1 : 0; a.autoreset = autoreset ? 1 : 0;
    return enqueue_pulse(ctx, w, act_f64, (hipStream_t)stream);
}
// the id form: one step of the M envs env_ids
template <class ARGS>
static int pulse_step_ids(stg_ctx* ctx, const char* who, const char* setter, int64_t M, const uint32_t* env_ids, const void* actions,
                          int32_t act_f64, int32_t autoreset, float* obs, float* final_obs, float* reward, double* reward_f64, double* energy,
                          uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream) {
    ARGS w{};
    StepArgs& a = w.s;
    if (int rc = pulse_checks(ctx, who, setter, ctx && pulse_table(ctx, w))) return rc;
    if (M < 0 || M > 0xFFFFFFFFll) return fail(STG_E_INVALID, "M must be in [0, 2^32)");
    if (!env_ids || !actions || !obs) return fail(STG_E_INVALID, "env_ids/actions/obs must not be NULL");
    if (int rc = step_outputs(ctx, a, obs, final_obs, reward, reward_f64, energy, terminated, truncated, status)) return rc;
    if (M == 0) return STG_OK;                         // an empty list: nothing to launch
    a.N = M; a.ids = env_ids; a.n_state = ctx->N;
    a.actions = actions; a.K = 1; a.out_every = 1; a.autoreset = autoreset ? 1 : 0;
    return enqueue_pulse(ctx, w, act_f64, (hipStream_t)stream);
}
}

int stg_step_shaped(stg_ctx* ctx, int32_t K, const void* actions, int32_t act_f64, int32_t out_every, int32_t autoreset, float* obs,
                    float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated, uint8_t* truncated,
                    uint8_t* status, void* stream) {
    return pulse_step_many<ShapedStepArgs>(ctx, "stg_step_shaped", "stg_set_pulse_shape", K, actions, act_f64, out_every, autoreset, obs,
                                           final_obs, reward, reward_f64, energy, terminated, truncated, status, stream);
}

int stg_step_shaped_ids(stg_ctx* ctx, int64_t M, const uint32_t* env_ids, const void* actions, int32_t act_f64, int32_t autoreset, float* obs,
                        float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated, uint8_t* truncated,
                        uint8_t* status, void* stream) {
    return pulse_step_ids<ShapedStepArgs>(ctx, "stg_step_shaped_ids", "stg_set_pulse_shape", M, env_ids, actions, act_f64, autoreset, obs,
                                          final_obs, reward, reward_f64, energy, terminated, truncated, status, stream);
}

int stg_step_knots(stg_ctx* ctx, int32_t K, const void* actions, int32_t act_f64, int32_t out_every, int32_t autoreset, float* obs,
                   float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated, uint8_t* truncated,
                   uint8_t* status, void* stream) {
    return pulse_step_many<KnotsStepArgs>(ctx, "stg_step_knots", "stg_set_pulse_knots", K, actions, act_f64, out_every, autoreset, obs,
                                          final_obs, reward, reward_f64, energy, terminated, truncated, status, stream);
}

int stg_step_knots_ids(stg_ctx* ctx, int64_t M, const uint32_t* env_ids, const void* actions, int32_t act_f64, int32_t autoreset, float* obs,
                       float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated, uint8_t* truncated,
                       uint8_t* status, void* stream) {
    return pulse_step_ids<KnotsStepArgs>(ctx, "stg_step_knots_ids", "stg_set_pulse_knots", M, env_ids, actions, act_f64, autoreset, obs,
                                         final_obs, reward, reward_f64, energy, terminated, truncated, status, stream);
}

extern "C++" {
template <int SOLVER>
static void dispatch_solve(const SolveArgs& a, bool thermal, bool multi, bool record, hipStream_t st) {
    with_flag(thermal, [&](auto THERMAL) { with_flag(multi, [&](auto MULTI) { with_flag(record, [&](auto RECORD) {
        hipLaunchKernelGGL((stg_solve_kernel<SOLVER, THERMAL.value, MULTI.value, RECORD.value>), grid_for(a.N), dim3(64), 0, st, a);
    }); }); });
}
}  // extern "C++"

static int solve_common(stg_ctx* ctx, const double* m0, const double* J, const double* T, uint32_t env_step,
                        int32_t traj_cap, double* tt, double* tm, double* te, double* ttq, double* m_final, int32_t* n_points,
                        uint8_t* success, void* stream, bool record) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, "stg_set_params must precede stg_solve");
    if (ctx->per_env) return fail(STG_E_STATE, "stg_solve* works on the class table (stg_set_params), not on per-env parameters");
    if (!m0 || !J || !T || !m_final) return fail(STG_E_INVALID, "m0/J/T/m_final must not be NULL");
    if (record && traj_cap < 1) return fail(STG_E_INVALID, "traj_cap must be >= 1");
    HIP_TRY(hipSetDevice(ctx->device));
    SolveArgs a{};
    a.c = cfg_view(ctx->cfg); a.N = ctx->N; a.env_id0 = ctx->env_id0;
    a.ctab = ctx->ctab; a.cls = ctx->cls; a.ncls = ctx->ncls;
    a.m0 = m0; a.J = J; a.T = T; a.env_step = env_step; a.m_final = m_final; a.n_points = n_points; a.success = success;
    a.traj_cap = traj_cap; a.traj_t = tt; a.traj_m = tm; a.traj_e = te; a.traj_tq = ttq;
    const bool multi = ctx->ncls > 1;
    hipStream_t st = (hipStream_t)stream;
    const bool thermal = thermal_flag(ctx->cfg);
    switch (ctx->cfg.solver) {
        case STG_SOLVER_RK4: dispatch_solve<STG_SOLVER_RK4>(a, thermal, multi, record, st); break;
        case STG_SOLVER_EULER: dispatch_solve<STG_SOLVER_EULER>(a, thermal, multi, record, st); break;
        default: dispatch_solve<STG_SOLVER_RK45>(a, thermal, multi, record, st); break;
    }
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_solve(stg_ctx* ctx, const double* m0, const double* J, const double* T, uint32_t env_step, double* m_final,
              int32_t* n_points, uint8_t* success, void* stream) {
    return solve_common(ctx, m0, J, T, env_step, 0, nullptr, nullptr, nullptr, nullptr, m_final, n_points, success, stream, false);
}

int stg_solve_traj(stg_ctx* ctx, const double* m0, const double* J, const double* T, uint32_t env_step, int32_t traj_cap,
                   double* t, double* m, double* energy, double* torques, double* m_final, int32_t* n_points, uint8_t* success,
                   void* stream) {
    return solve_common(ctx, m0, J, T, env_step, traj_cap, t, m, energy, torques, m_final, n_points, success, stream, true);
}

// the waveform solve: its kernels live in stg_solve_wave.hip (stg_wave_launch); stg_solve_kernel is not involved
int stg_solve_wave(stg_ctx* ctx, const double* m0, const double* J, const double* T, int32_t kj, const double* tj, const double* jk,
                   int32_t kh, const double* th, const double* hk, uint32_t env_step, int32_t traj_cap, double* t, double* m,
                   double* energy, double* torques, double* m_final, int32_t* n_points, uint8_t* success, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, "stg_set_params must precede stg_solve_wave");
    if (ctx->per_env) return fail(STG_E_STATE, "stg_solve* works on the class table (stg_set_params), not on per-env parameters");
    if (!m0 || !T || !m_final) return fail(STG_E_INVALID, "m0/T/m_final must not be NULL");
    if (kj != 0 && (kj < 2 || kj > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kj must be 0 or 2 ... STG_MAX_KNOTS");
    if (kh != 0 && (kh < 2 || kh > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kh must be 0 or 2 ... STG_MAX_KNOTS");
    if (kj == 0 && !J) return fail(STG_E_INVALID, "J must not be NULL without a current table (kj = 0)");
    if (kj != 0 && (!tj || !jk)) return fail(STG_E_INVALID, "tj/jk must not be NULL with kj > 0");
    if (kh != 0 && (!th || !hk)) return fail(STG_E_INVALID, "th/hk must not be NULL with kh > 0");
    if (traj_cap < 0) return fail(STG_E_INVALID, "traj_cap must be >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    WaveSolveArgs w{};
    SolveArgs& a = w.s;
    a.c = cfg_view(ctx->cfg); a.N = ctx->N; a.env_id0 = ctx->env_id0;
    a.ctab = ctx->ctab; a.cls = ctx->cls; a.ncls = ctx->ncls;
    a.m0 = m0; a.J = J; a.T = T; a.env_step = env_step; a.m_final = m_final; a.n_points = n_points; a.success = success;
    const bool record = traj_cap > 0;
    a.traj_cap = traj_cap;
    if (record) { a.traj_t = t; a.traj_m = m; a.traj_e = energy; a.traj_tq = torques; }
    w.kj = kj; w.tj = tj; w.jk = jk; w.kh = kh; w.th = th; w.hk = hk;
    stg_wave_launch(w, ctx->cfg.solver, thermal_flag(ctx->cfg), ctx->ncls > 1, record, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

// Monte-Carlo switching statistics: the three entries launch the one trial kernel of stg_switch.hpp (stg_switch_launch) on the largest
// argument block, SwitchTimesArgs, of which stg_switch_stats fills in the innermost part and stg_switch_stats_wave the middle one.
// The argument checks and the argument block the three entries share; `need_J`: whether a NULL J is refused here.
static int switch_stats_args(stg_ctx* ctx, const char* what, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P,
                             const double* m0, const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step,
                             const double* target, double threshold, int32_t n_bins, unsigned long long* n_switched,
                             unsigned long long* n_failed, unsigned long long* hist, bool need_J, SwitchStatsArgs& a) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, std::string("stg_set_params must precede ") + what);
    if (ctx->per_env) return fail(STG_E_STATE, std::string(what) + " works on the class table (stg_set_params), not on per-env parameters");
    if (!m0 || (need_J && !J) || !T || !target || !n_switched || !n_failed) return fail(STG_E_INVALID, "m0/J/T/target/n_switched/n_failed must not be NULL");
    if (G < 1) return fail(STG_E_INVALID, "G must be >= 1");
    if (R < 0) return fail(STG_E_INVALID, "R must be >= 0");
    if (P < 1 || P > STG_MAX_PHASES) return fail(STG_E_INVALID, "P must be in 1 ... STG_MAX_PHASES");
    if (n_bins < 0 || n_bins > STG_MAX_BINS) return fail(STG_E_INVALID, "n_bins must be in 0 ... STG_MAX_BINS");
    if ((hist == nullptr) != (n_bins == 0)) return fail(STG_E_INVALID, "hist must be NULL if and only if n_bins == 0");
    if (trial0 < 0) return fail(STG_E_INVALID, "trial0 must be >= 0");
    if (R > INT64_MAX - trial0 || trial_stride < trial0 + R)
        return fail(STG_E_INVALID, "trial_stride must be >= trial0 + R (the streams of two conditions would overlap)");
    if (trial_stride > (INT64_MAX - ctx->env_id0) / (int64_t)G) return fail(STG_E_INVALID, "env_id0 + G * trial_stride exceeds int64");
    a.c = cfg_view(ctx->cfg); a.env_id0 = ctx->env_id0;
    a.R = R; a.trial0 = trial0; a.trial_stride = trial_stride;
    if (R > 0) switch_stats_plan(G, R, &a.L, &a.waves_per_cond);
    a.G = G; a.P = P; a.n_bins = n_bins; a.ncls = ctx->ncls;
    a.ctab = ctx->ctab; a.cond_cls = cond_cls;
    a.m0 = m0; a.J = J; a.T = T; a.target = target; a.threshold = threshold; a.env_step = env_step;
    a.n_switched = n_switched; a.n_failed = n_failed; a.hist = hist;
    return STG_OK;
}

// the tabled (stg_switch_stats_wave) or watched (stg_switch_times) phase and the tables: checks, then the wiring.  `need_table`: whether
// a call without any table is refused
static int switch_wave_args(const char* phase_name, bool need_table, int32_t phase, int32_t P, int32_t kj, const double* tj, const double* jk,
                            int32_t kh, const double* th, const double* hk, SwitchStatsWaveArgs& w) {
    if (phase < 0 || phase >= P) return fail(STG_E_INVALID, std::string(phase_name) + " must be in 0 ... P - 1");
    if (kj != 0 && (kj < 2 || kj > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kj must be 0 or 2 ... STG_MAX_KNOTS");
    if (kh != 0 && (kh < 2 || kh > STG_MAX_KNOTS)) return fail(STG_E_INVALID, "kh must be 0 or 2 ... STG_MAX_KNOTS");
    if (need_table && kj == 0 && kh == 0) return fail(STG_E_INVALID, "kj = kh = 0: no waveform, use stg_switch_stats");
    if (kj != 0 && (!tj || !jk)) return fail(STG_E_INVALID, "tj/jk must not be NULL with kj > 0");
    if (kh != 0 && (!th || !hk)) return fail(STG_E_INVALID, "th/hk must not be NULL with kh > 0");
    w.wave_phase = phase;
    w.kj = kj; w.tj = tj; w.jk = jk; w.kh = kh; w.th = th; w.hk = hk;
    return STG_OK;
}

// the first-passage outputs (stg_switch_times, stg_switch_population): checks, then the wiring.  `counts_optional`: n_crossed and
// n_returned may both be NULL with n_tbins == 0
static int switch_passage_args(int32_t n_tbins, unsigned long long* n_crossed, unsigned long long* n_returned, unsigned long long* t_hist,
                               bool counts_optional, SwitchTimesArgs& x) {
    if (n_tbins < 0 || n_tbins > STG_MAX_TBINS) return fail(STG_E_INVALID, "n_tbins must be in 0 ... STG_MAX_TBINS");
    const bool none = counts_optional && n_tbins == 0 && !n_crossed && !n_returned;
    if (!none && (!n_crossed || !n_returned)) return fail(STG_E_INVALID, "n_crossed/n_returned must not be NULL");
    if ((t_hist == nullptr) != (n_tbins == 0)) return fail(STG_E_INVALID, "t_hist must be NULL if and only if n_tbins == 0");
    x.n_tbins = n_tbins; x.n_crossed = n_crossed; x.n_returned = n_returned; x.t_hist = t_hist;
    return STG_OK;
}

// the launch tail of the three entries (`times`: stg_switch_times); no trials, no launch
static int switch_launch(stg_ctx* ctx, const SwitchTimesArgs& x, bool times, void* stream) {
    if (x.w.s.R == 0) return STG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    stg_switch_launch(x, times, ctx->cfg.solver, thermal_flag(ctx->cfg), ctx->ncls > 1 && x.w.s.cond_cls != nullptr, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_switch_stats(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P, const double* m0, const double* J,
                     const double* T, const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                     unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist, void* stream) {
    SwitchTimesArgs x{};
    if (int rc = switch_stats_args(ctx, "stg_switch_stats", G, R, trial0, trial_stride, P, m0, J, T, cond_cls, env_step, target, threshold, n_bins,
                                   n_switched, n_failed, hist, true, x.w.s)) return rc;
    return switch_launch(ctx, x, false, stream);
}

int stg_switch_stats_wave(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P, const double* m0, const double* J,
                          const double* T, int32_t wave_phase, int32_t kj, const double* tj, const double* jk, int32_t kh, const double* th,
                          const double* hk, const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                          unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist, void* stream) {
    SwitchTimesArgs x{};
    // (J is read for the rectangular phases, and for the wave phase without a current table: a single tabled phase needs none)
    if (int rc = switch_stats_args(ctx, "stg_switch_stats_wave", G, R, trial0, trial_stride, P, m0, J, T, cond_cls, env_step, target, threshold,
                                   n_bins, n_switched, n_failed, hist, !(P == 1 && kj > 0), x.w.s)) return rc;
    if (int rc = switch_wave_args("wave_phase", true, wave_phase, P, kj, tj, jk, kh, th, hk, x.w)) return rc;
    return switch_launch(ctx, x, false, stream);
}

int stg_switch_times(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P, const double* m0, const double* J,
                     const double* T, int32_t watch_phase, int32_t kj, const double* tj, const double* jk, int32_t kh, const double* th,
                     const double* hk, const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                     unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist, int32_t n_tbins,
                     unsigned long long* n_crossed, unsigned long long* n_returned, unsigned long long* t_hist, void* stream) {
    SwitchTimesArgs x{};
    // (J as in stg_switch_stats_wave: not read for a single phase with a current table)
    if (int rc = switch_stats_args(ctx, "stg_switch_times", G, R, trial0, trial_stride, P, m0, J, T, cond_cls, env_step, target, threshold,
                                   n_bins, n_switched, n_failed, hist, !(P == 1 && kj > 0), x.w.s)) return rc;
    if (int rc = switch_wave_args("watch_phase", false, watch_phase, P, kj, tj, jk, kh, th, hk, x.w)) return rc;
    if (int rc = switch_passage_args(n_tbins, n_crossed, n_returned, t_hist, false, x)) return rc;
    return switch_launch(ctx, x, true, stream);
}

// write - verify - write: the kernels of stg_switch_verify.hpp on stg_switch_stats' argument block, with the attempts in front of the phases.
// What stg_switch_verify and stg_switch_verify_population share: the checks, the argument block and the launch rule
static int switch_verify_args(stg_ctx* ctx, const char* what, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t A, int32_t P,
                              const double* m0, const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step,
                              const double* target, double threshold, int32_t n_bins, int32_t max_waves, unsigned long long* n_switched_at,
                              unsigned long long* n_ended_at, unsigned long long* n_failed, unsigned long long* hist, SwitchVerifyArgs& x) {
    if (int rc = switch_stats_args(ctx, what, G, R, trial0, trial_stride, P, m0, J, T, cond_cls, env_step, target, threshold, n_bins,
                                   n_switched_at, n_failed, hist, true, x.s)) return rc;
    if (!n_ended_at) return fail(STG_E_INVALID, "n_ended_at must not be NULL");
    if (A < 1 || A > STG_MAX_VERIFY_ATTEMPTS) return fail(STG_E_INVALID, "A must be in 1 ... STG_MAX_VERIFY_ATTEMPTS");
    if (max_waves < 0 || (max_waves > 0 && max_waves < G)) return fail(STG_E_INVALID, "max_waves must be 0 (the library's rule) or >= G");
    x.A = A; x.n_ended_at = n_ended_at;
    x.s.L = 0;                                                                     // (the lockstep kernel's; every lane walks its own list here)
    if (R > 0) x.s.waves_per_cond = switch_verify_plan(G, R, max_waves);
    return STG_OK;
}

int stg_switch_verify(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t A, int32_t P, const double* m0,
                      const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold,
                      int32_t n_bins, int32_t max_waves, unsigned long long* n_switched_at, unsigned long long* n_ended_at,
                      unsigned long long* n_failed, unsigned long long* hist, void* stream) {
    SwitchVerifyArgs x{};
    if (int rc = switch_verify_args(ctx, "stg_switch_verify", G, R, trial0, trial_stride, A, P, m0, J, T, cond_cls, env_step, target, threshold,
                                    n_bins, max_waves, n_switched_at, n_ended_at, n_failed, hist, x)) return rc;
    if (R == 0) return STG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!stg_switch_verify_launch(x, ctx->cfg.solver, thermal_flag(ctx->cfg), ctx->ncls > 1 && cond_cls != nullptr, (hipStream_t)stream))
        return fail(STG_E_INVALID, "stg_switch_verify has no kernel for this solver");
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

// what stg_switch_population and its diagnostic twin share: the checks of the draw's scalars
static int switch_vary_scalars(const double* sigma, double z_clip, int64_t trials_per_device) {
    if (!sigma) return fail(STG_E_INVALID, "sigma must not be NULL");
    if (!(z_clip > 0) || !std::isfinite(z_clip)) return fail(STG_E_INVALID, "z_clip must be finite and > 0");
    if (trials_per_device < 1) return fail(STG_E_INVALID, "trials_per_device must be >= 1");
    return STG_OK;
}

int stg_switch_population(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P, const double* m0, const double* J,
                          const double* T, int32_t watch_phase, int32_t kj, const double* tj, const double* jk, int32_t kh, const double* th,
                          const double* hk, const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                          unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist, int32_t n_tbins,
                          unsigned long long* n_crossed, unsigned long long* n_returned, unsigned long long* t_hist, const double* sigma,
                          double z_clip, uint32_t var_step, int64_t trials_per_device, unsigned long long* dev_switched, int64_t dev_stride,
                          void* stream) {
    SwitchPopArgs x{};
    if (int rc = switch_stats_args(ctx, "stg_switch_population", G, R, trial0, trial_stride, P, m0, J, T, cond_cls, env_step, target, threshold,
                                   n_bins, n_switched, n_failed, hist, !(P == 1 && kj > 0), x.t.w.s)) return rc;
    if (int rc = switch_wave_args("watch_phase", false, watch_phase, P, kj, tj, jk, kh, th, hk, x.t.w)) return rc;
    if (int rc = switch_passage_args(n_tbins, n_crossed, n_returned, t_hist, true, x.t)) return rc;
    if (int rc = switch_vary_scalars(sigma, z_clip, trials_per_device)) return rc;
    for (int32_t p = 0; p < P; ++p)
        if (var_step == env_step + (uint32_t)p)
            return fail(STG_E_INVALID, "var_step must differ from env_step + p for every phase p (the device's draw would reuse a thermal stream)");
    const int64_t Q = trials_per_device;
    if (dev_switched) {
        // devices 0 ... (trial0 + R - 1) / Q of a condition must fit its row: ceil((trial0 + R) / Q), formed without overflow
        const int64_t end = trial0 + R, need = end / Q + (end % Q != 0 ? 1 : 0);
        if (dev_stride < need) return fail(STG_E_INVALID, "dev_stride must be >= (trial0 + R + Q - 1) / Q");
        if (dev_stride > INT64_MAX / (int64_t)G) return fail(STG_E_INVALID, "G * dev_stride exceeds int64");
    }
    x.v.sigma = sigma; x.v.ptab = ctx->ptab; x.v.z_clip = z_clip; x.v.gamma = ctx->cfg.gamma; x.v.Q = Q; x.v.var_step = var_step;
    x.v.dev_switched = dev_switched; x.v.dev_stride = dev_stride;
    if (R == 0) return STG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    stg_switch_vary_launch(x, n_crossed != nullptr, ctx->cfg.solver, thermal_flag(ctx->cfg), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

// stg_switch_verify over a population: the checks of both parents, then the sibling kernel of stg_switch_verify.hpp
int stg_switch_verify_population(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t A, int32_t P, const double* m0,
                                 const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step, const double* target,
                                 double threshold, int32_t n_bins, int32_t max_waves, unsigned long long* n_switched_at,
                                 unsigned long long* n_ended_at, unsigned long long* n_failed, unsigned long long* hist, const double* sigma,
                                 double z_clip, uint32_t var_step, int64_t trials_per_device, unsigned long long* dev_switched_at,
                                 int64_t dev_stride, void* stream) {
    SwitchVerifyPopArgs x{};
    if (int rc = switch_verify_args(ctx, "stg_switch_verify_population", G, R, trial0, trial_stride, A, P, m0, J, T, cond_cls, env_step, target,
                                    threshold, n_bins, max_waves, n_switched_at, n_ended_at, n_failed, hist, x.y)) return rc;
    if (int rc = switch_vary_scalars(sigma, z_clip, trials_per_device)) return rc;
    if (var_step - env_step < (uint32_t)(A * P))                                   // (modulo 2^32, as the counter words are formed)
        return fail(STG_E_INVALID, "var_step must differ from env_step + a * P + p for every phase of every attempt (the device's draw would reuse a thermal stream)");
    const int64_t Q = trials_per_device;
    if (dev_switched_at) {
        // devices 0 ... (trial0 + R - 1) / Q of a condition must fit a row: ceil((trial0 + R) / Q), formed without overflow
        const int64_t end = trial0 + R, need = end / Q + (end % Q != 0 ? 1 : 0);
        if (dev_stride < need) return fail(STG_E_INVALID, "dev_stride must be >= (trial0 + R + Q - 1) / Q");
        if (dev_stride > INT64_MAX / ((int64_t)A * G)) return fail(STG_E_INVALID, "A * G * dev_stride exceeds int64");
    }
    x.v.sigma = sigma; x.v.ptab = ctx->ptab; x.v.z_clip = z_clip; x.v.gamma = ctx->cfg.gamma; x.v.Q = Q; x.v.var_step = var_step;
    x.v.dev_switched = dev_switched_at; x.v.dev_stride = dev_stride;
    if (R == 0) return STG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!stg_switch_verify_population_launch(x, ctx->cfg.solver, thermal_flag(ctx->cfg), (hipStream_t)stream))
        return fail(STG_E_INVALID, "stg_switch_verify_population has no kernel for this solver");
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_switch_population_devices(stg_ctx* ctx, int32_t G, int64_t D, int64_t dev0, int64_t trials_per_device, int64_t trial_stride,
                                  uint32_t var_step, double z_clip, const double* sigma, const uint8_t* cond_cls, double* params, double* z,
                                  void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, "stg_set_params must precede stg_switch_population_devices");
    if (ctx->per_env) return fail(STG_E_STATE, "stg_switch_population_devices works on the class table (stg_set_params), not on per-env parameters");
    if (!params) return fail(STG_E_INVALID, "params must not be NULL");
    if (G < 1) return fail(STG_E_INVALID, "G must be >= 1");
    if (D < 0 || dev0 < 0) return fail(STG_E_INVALID, "D and dev0 must be >= 0");
    if (int rc = switch_vary_scalars(sigma, z_clip, trials_per_device)) return rc;
    if (trial_stride < 1 || trial_stride > (INT64_MAX - ctx->env_id0) / (int64_t)G) return fail(STG_E_INVALID, "env_id0 + G * trial_stride exceeds int64");
    if (D > 0 && (D - 1 > INT64_MAX - dev0 || dev0 + D - 1 > (trial_stride - 1) / trials_per_device))
        return fail(STG_E_INVALID, "(dev0 + D - 1) * trials_per_device must be < trial_stride");
    if (D > INT64_MAX / (int64_t)G / 6 || (int64_t)G * D > (int64_t)UINT32_MAX * 256) return fail(STG_E_INVALID, "G * D too large");
    if (D == 0) return STG_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t n = (int64_t)G * D;
    hipLaunchKernelGGL(stg_population_devices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctx->cfg.seed,
                       ctx->env_id0, G, D, dev0, trials_per_device, trial_stride, var_step, z_clip, sigma, ctx->ptab, cond_cls, ctx->ncls, params, z);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_get_state(stg_ctx* ctx, double* m, double* target, double* total_energy, int32_t* step_count, uint32_t* rng_step,
                  uint8_t* done, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stg_state_copy_kernel<false>, dim3((unsigned)((ctx->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       ctx->s, ctx->N, m, target, total_energy, step_count, rng_step, done);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_set_state(stg_ctx* ctx, const double* m, const double* target, const double* total_energy,
                  const int32_t* step_count, const uint32_t* rng_step, const uint8_t* done, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stg_state_copy_kernel<true>, dim3((unsigned)((ctx->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       ctx->s, ctx->N, const_cast<double*>(m), const_cast<double*>(target), const_cast<double*>(total_energy),
                       const_cast<int32_t*>(step_count), const_cast<uint32_t*>(rng_step), const_cast<uint8_t*>(done));
    HIP_TRY(hipGetLastError());
    if (m && target) ctx->have_state = true;
    return STG_OK;
}

int stg_device_terms(stg_ctx* ctx, const double* m, const double* J, const double* volt, double* tau_dl, double* tau_fl,
                     double* k_eff, void* stream) {
    if (!ctx) return fail(STG_E_INVALID, "ctx is NULL");
    if (!ctx->have_params) return fail(STG_E_STATE, "stg_set_params must precede stg_device_terms");
    if (ctx->per_env) return fail(STG_E_STATE, "stg_device_terms works on the class table (stg_set_params), not on per-env parameters");
    if ((tau_dl || tau_fl) && (!m || !J)) return fail(STG_E_INVALID, "m and J are required for the SOT torques");
    if (k_eff && !volt) return fail(STG_E_INVALID, "volt is required for K_eff");
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stg_device_terms_kernel, dim3((unsigned)((ctx->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       ctx->N, ctx->ctab, ctx->cls, ctx->ncls, m, J, volt, tau_dl, tau_fl, k_eff);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

int stg_get_counters(stg_ctx* ctx, uint64_t* out, int32_t reset) {
    if (!ctx || !out) return fail(STG_E_INVALID, "ctx/out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    // the kernels add into COUNTER_STRIPES copies (a workgroup picks one by its index: thousands of wavefronts on one
    // address would serialise in the memory-side atomic unit); the stripes are summed here
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "counter width");
    uint64_t h[COUNTER_STRIPES * COUNTER_STRIDE];
    HIP_TRY(hipMemcpy(h, ctx->counters, sizeof(h), hipMemcpyDeviceToHost));
    for (int j = 0; j < 4; ++j) {
        out[j] = 0;
        for (int st = 0; st < COUNTER_STRIPES; ++st) out[j] += h[st * COUNTER_STRIDE + j];
    }
    if (reset) HIP_TRY(hipMemset(ctx->counters, 0, sizeof(h)));
    return STG_OK;
}

int stg_get_placement(stg_ctx* ctx, int32_t launches_back, uint32_t* out, int32_t cap, int32_t* n_workgroups, int32_t* waves_per_workgroup) {
    if (!ctx || !out || cap < 1) return fail(STG_E_INVALID, "ctx/out is NULL or cap < 1");
    if (launches_back < 0 || launches_back >= PLACEMENT_RING || (uint64_t)launches_back >= ctx->launch_seq)
        return fail(STG_E_INVALID, "launches_back must address one of the last launches (at most 32 are kept)");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    static thread_local uint32_t h[PLACEMENT_WORDS];
    const uint64_t seq = ctx->launch_seq - 1 - (uint64_t)launches_back;
    HIP_TRY(hipMemcpy(h, ctx->placement + (size_t)(seq % PLACEMENT_RING) * PLACEMENT_WORDS, sizeof(h), hipMemcpyDeviceToHost));
    const int64_t waves = (int64_t)h[0] * (int64_t)h[1];
    int32_t n = (int32_t)(waves < PLACEMENT_CAP ? waves : PLACEMENT_CAP);
    if (n > cap / STG_PLACEMENT_WORDS_PER_WAVE) n = cap / STG_PLACEMENT_WORDS_PER_WAVE;
    if (n_workgroups) *n_workgroups = (int32_t)h[0];
    if (waves_per_workgroup) *waves_per_workgroup = (int32_t)h[1];
    static_assert(STG_PLACEMENT_WORDS_PER_WAVE == PLACEMENT_ENTRY, "entry size of the placement table");
    std::memcpy(out, h + 2, sizeof(uint32_t) * (size_t)n * PLACEMENT_ENTRY);
    return n;
}

int stg_thermal_normals(stg_ctx* ctx, uint32_t env_step, uint32_t call0, int32_t n_calls, double* z, void* stream) {
    if (!ctx || !z) return fail(STG_E_INVALID, "ctx/z is NULL");
    if (n_calls < 1) return fail(STG_E_INVALID, "n_calls must be >= 1");
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(stg_normals_kernel, dim3((unsigned)((ctx->N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       ctx->cfg.seed, ctx->env_id0, ctx->N, env_step, call0, n_calls, z);
    HIP_TRY(hipGetLastError());
    return STG_OK;
}

}  // extern "C"
