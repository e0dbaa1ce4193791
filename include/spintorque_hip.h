/*
 * spintorque_hip.h -- C-ABI of libspintorque_hip.so: the MI355X (gfx950) implementation of the
 * SpinTorque-v0 env.step() hot path, vectorised over N independent macrospin environments.
 *
 * The reference (danieleschmidt/spin-torque-rl-gym) is pure Python and has no FFI of its own; the
 * seam this library replaces is Python duck-typing at two levels:
 *   env level    : SpinTorqueEnv.reset/step            (spin_torque_gym/envs/spin_torque_env.py:250-407)
 *   solver level : RobustLLGSSolver.solve / LLGSSolver.solve
 *                                                       (utils/robust_solver.py:75-150, physics/llgs_solver.py:51-180)
 * Each entry point below cites the reference code it stands in for.  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add to bind it.
 *
 * Conventions
 *   - plain C types only; every pointer marked [dev] is a device (HBM) pointer owned by the caller
 *     (any allocator: hipMalloc, a PyTorch-ROCm tensor's data_ptr(), ...); [host] pointers are host memory.
 *   - per-env arrays are structure-of-arrays: component-major, env index fastest (m is [3][N], obs is [12][N]),
 *     so that lane i of a wavefront touches element i of each row (coalesced).
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     nothing synchronises with the host except stg_create, stg_destroy, stg_set_params, stg_set_pulse_shape and stg_set_pulse_knots (stg_get_state / stg_set_state enqueue copies on `stream`).
 *   - return value 0 = success, negative = error (STG_E_*); stg_last_error() returns a thread-local message.
 *   - one context per GPU; a context is not thread-safe.  Contexts are independent (no global state).
 *   - IEEE fp64 state and arithmetic (the reference's NumPy float64); observations are rounded to fp32 last,
 *     as the reference does (spin_torque_env.py:520).
 */
#ifndef SPINTORQUE_HIP_H
#define SPINTORQUE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STG_ABI_VERSION 5

typedef struct stg_ctx stg_ctx;

enum {
    STG_OK = 0,
    STG_E_INVALID = -1,   /* bad argument */
    STG_E_HIP = -2,       /* a HIP runtime call failed */
    STG_E_NOMEM = -3,
    STG_E_STATE = -4      /* call order (e.g. step before set_params/reset) */
};

/* integrator: which reference solver's semantics a step/solve follows */
enum {
    STG_SOLVER_RK4 = 0,   /* SimpleLLGSSolver(method='rk4') behind RobustLLGSSolver -- what SpinTorqueEnv builds
                             (spin_torque_env.py:93-102; simple_solver.py:278-295) */
    STG_SOLVER_EULER = 1, /* SimpleLLGSSolver(method='euler') (simple_solver.py:263-276) */
    STG_SOLVER_RK45 = 2   /* LLGSSolver: SciPy solve_ivp(method='RK45') (llgs_solver.py:130-139) */
};

enum { STG_DEV_STT = 0, STG_DEV_SOT = 1, STG_DEV_VCMA = 2 };

/* per-lane status written by stg_step / stg_solve */
enum {
    STG_STATUS_OK = 0,
    STG_STATUS_NOOP = 1,       /* solver reported success=False -> magnetisation left unchanged
                                  (spin_torque_env.py:461-467; robust_solver.py:140-150) */
    STG_STATUS_RESET = 2,      /* success, but >= 1 sub-step took the non-finite -> [0,0,1] branch
                                  (simple_solver.py:213-216) */
    STG_STATUS_INACTIVE = 3,   /* env was already terminated/truncated and autoreset is off: not stepped */
    STG_STATUS_BAD_ID = 4      /* stg_step_ids: the list entry's env id is >= n_envs (nothing was read or written for it) */
};

enum { STG_OUT_SOA = 0, STG_OUT_RECORDS = 1 };
#define STG_RECORD_BYTES 56        /* 12 x f32 obs | f32 reward | u8 terminated | u8 truncated | u8 status | u8 0 */

#define STG_MAX_TARGETS 8
#define STG_MAX_CLASSES 64
#define STG_MAX_KNOTS 32          /* knots of one piecewise-linear waveform (stg_solve_wave, stg_step_wave, stg_set_pulse_shape, stg_set_pulse_knots) */

/* SpinTorqueEnv.__init__ keyword arguments + solver constructor arguments
 * (spin_torque_env.py:36-53,93-102; llgs_solver.py:24-31; simple_solver.py:24-31) */
typedef struct {
    int32_t solver;                 /* STG_SOLVER_* */
    int32_t thermal;                /* include_thermal_fluctuations */
    double temperature;             /* K */
    double gamma;                   /* 2.21e5 m/(A s) */
    double max_step;                /* 1e-12 s */
    double rtol, atol;              /* RK45: 1e-6, 1e-9 */
    int32_t max_steps;              /* 100 */
    int32_t n_targets;              /* len(target_states), <= STG_MAX_TARGETS */
    double max_current;             /* 2e6 A/m^2 */
    double max_duration;            /* 5e-9 s */
    double success_threshold;       /* 0.9 */
    double energy_penalty_weight;   /* 0.1 */
    double targets[STG_MAX_TARGETS][3]; /* target_states, unit vectors (default +z, -z) */
    uint64_t seed;                  /* key of the in-kernel Philox4x32-10 (thermal field, device-side resets) */
    int64_t max_attempts;           /* RK45 attempt budget per solve, 1 ... 2^31 - 1; exceeded -> STG_STATUS_NOOP.  The reference has
                                       no such guard (its stiff cases simply never return, SURVEY.md headline 3). */
    int32_t skip_done;              /* 1: lanes whose episode already ended are not integrated (wavefront-level
                                       early-out) and report STG_STATUS_INACTIVE; 0: reference behaviour (step anyway) */
    int32_t torque_model;           /* 0 (default): the reference env's type-agnostic RHS for every device type.
                                       1: opt-in device-physics torque model for the fixed-step solvers (SURVEY 8f #1,
                                       BASELINE config 4): SOT classes use SOTMRAMDevice.compute_spin_torque
                                       (sot_mram.py:163-194) instead of the Slonczewski term, VCMA classes use
                                       H_k from VCMAMRAMDevice._compute_effective_anisotropy (vcma_mram.py:122-147)
                                       at V = J R(m) A while the pulse is on.  The reference env never calls these
                                       formulas; the model is pinned against the device classes, not against env runs. */
    int32_t wave_spec;              /* thermal kernels: every integrating wavefront gets a second wavefront that runs the
                                       envs' normal streams ahead into LDS (same values, same order: results are
                                       bit-identical).  0 = automatic (launches of <= 65536 envs), 1 always, -1 never */
    int32_t lane_sort;              /* schedule of envs onto lanes: 0 = automatic (sort), 1 = always sort the envs by pulse duration
                                       on the device before each step so that the lanes of a wavefront have equal trip
                                       counts, -1 = identity.  Results are unaffected: an env's arithmetic does not depend
                                       on the lane that runs it. */
    int32_t noise_model;            /* thermal field of the fixed-step solvers: 0 (default) = white, three fresh normals
                                       per RHS call (what the reference solvers do, simple_solver.py:378-388);
                                       1 = Ornstein-Uhlenbeck, the reference's ThermalFluctuations model
                                       (physics/thermal_model.py:113-137): once per sub-step
                                       x <- d x + sqrt(1 - d^2) xi, d = exp(-dt / noise_corr_time), field = strength * x
                                       for all stages of the sub-step, x = 0 at the start of every pulse;
                                       2 = Brown's field with the 1/sqrt(dt) factor that the reference's lacks:
                                       per solve c = 1.0 / sqrt(dt) (IEEE square root, then IEEE division; dt as the solver
                                       forms it, = max_step in the usual case), per sub-step i one draw xi_i of three
                                       standard normals, taken from the env's stream exactly as model 1 takes its draw (same
                                       key, call index i, phase alternation and stream position), x_i = c * xi_i (one rounded
                                       product per component, nothing carried between sub-steps), field = strength * x_i
                                       for all stages of the sub-step -- the recurrence of model 1 with d = 0, w = c.
                                       `strength` is what stg_thermal_strength returns (dt-free, as for models 0 and 1), so
                                       the field's standard deviation per component is strength / sqrt(dt).  With RK4 the
                                       equilibrium is Boltzmann's to about 2e-3 in <m_z^2> at dt = 1 ps; Euler converges
                                       at first order only (<m_z^2> = 0.48 against 0.705 at Delta = 4, dt = 1 ps): use RK4.
                                       noise_corr_time is ignored.
                                       Models 1 and 2 are not available with STG_SOLVER_RK45 (no fixed dt). */
    int32_t out_layout;             /* layout of a step's RL-facing outputs (obs, reward, terminated, truncated):
                                       STG_OUT_SOA (0, default): four caller arrays, obs component-major float[12][N];
                                       STG_OUT_RECORDS (1): ONE array of STG_RECORD_BYTES-byte records, env index major --
                                       record i = { float obs[12]; float reward; uint8 terminated, truncated, status, 0 } --
                                       passed as `obs` (reward/terminated/truncated arguments are ignored, may be NULL);
                                       final_obs is then env-major too, float[N][12].
                                       A shard's records are one contiguous block, so the multi-GPU exchange is a single
                                       all-gather straight into the learner's [N_global] record array: obs is then the
                                       [N_global, 12] strided view of it (Gym's own orientation), no transposition or
                                       concatenation copy anywhere. */
    double noise_corr_time;         /* correlation_time of ThermalFluctuations (default 1e-12 s); used when noise_model = 1 */
    int32_t lane_refill;            /* STG_SOLVER_RK45, single-step launches: persistent wavefronts share one global queue of the launch's
                                       envs in the sorted schedule's longest-first order, and a lane that has finished its env takes the next
                                       entry while its neighbours keep integrating (ABI v3; since round 4 the queue is global, striped over 64 cursors so that the atomics do not serialise).  0 = automatic
                                       (launches of more than 131072 envs, more than 98304 with the thermal field: 1024 wavefronts -- one per
                                       SIMD -- up to 8 envs per lane on average, 2048 beyond), -1 = never, >= 2 = that many envs per lane on
                                       average (ceil(blocks / lane_refill) wavefronts).  Per-env arithmetic is untouched: results are
                                       bit-identical to the one-env-per-lane launch.  Not used with per-env parameter records, fused steps
                                       (K > 1) or a forced wave_spec = 1. */
    int32_t reserved0;              /* must be 0 */
} stg_config;

/* one reference-style device_params dict, flattened with the defaults the reference's .get() calls use
 * (simple_solver.py:126-131; llgs_solver.py:79-82,192-205; spin_torque_env.py:476,502; devices/ (all three device modules)) */
typedef struct {
    double damping;                 /* 'damping' */
    double ms;                      /* 'saturation_magnetization' */
    double ku;                      /* 'uniaxial_anisotropy' */
    double volume;                  /* 'volume' */
    double polarization;            /* 'polarization' */
    double easy_axis[3];            /* 'easy_axis', raw */
    double demag[3];                /* 'demag_factors' (LLGSSolver), default 0,0,1 */
    double a_ex;                    /* 'exchange_constant' (LLGSSolver), default 20e-12 */
    double area;                    /* 'area', default 1e-14 */
    double r_p, r_ap;               /* 'resistance_parallel', 'resistance_antiparallel' */
    double ref_m[3];                /* 'reference_magnetization', raw */
    double r_series;                /* SOT: 0.1*(rho_hm/t_hm)/(area*1e-12) (sot_mram.py:218-223); else 0 */
    double sot_tau_dl, sot_tau_fl;  /* SOT: tau_dl_factor, tau_fl_factor (sot_mram.py:61-72); else 0 */
    double sot_sigma[3];            /* SOT: z x current_direction (sot_mram.py:180-186), default (0,1,0) */
    double vcma_xi;                 /* VCMA: 'vcma_coefficient' */
    double vcma_td;                 /* VCMA: 'dielectric_thickness' */
    double vcma_vbd;                /* VCMA: 'breakdown_voltage' */
    double shape_demag[3];          /* SOT/VCMA: demag factors of compute_effective_field from 'aspect_ratio'
                                       (sot_mram.py:114-132, vcma_mram.py:149-166); zeros for STT.  Array env only. */
    int32_t dev_type;               /* STG_DEV_* : selects the compute_resistance form */
    int32_t params_valid;           /* outcome of validate_parameters(params,'stt_mram') (utils/validation.py:176-234),
                                       evaluated by the host mirror; 0 -> every solve falls back (no-op) */
} stg_device_params;

/* ---- lifecycle -------------------------------------------------------------------------------------- */

/* Allocates the SoA state for n_envs environments on GPU `device_id`.
 * env_id0 = global index of this context's first env (multi-GPU shards: rank r owns [env_id0, env_id0+n_envs)),
 * used only as the Philox counter so that results do not depend on the partition. */
int stg_create(stg_ctx** out, int device_id, int64_t n_envs, int64_t env_id0, const stg_config* cfg);
void stg_destroy(stg_ctx* ctx);
const char* stg_last_error(void);
int stg_abi_version(void);

/* ---- device parameter surface (spin_torque_gym.devices; DeviceFactory.create_device, device_factory.py:49-77) --- */

/* n_classes parameter sets (<= STG_MAX_CLASSES) [host]; cls [dev] uint8[N] selects the set of each env
 * (NULL: every env uses table[0]).  The derived per-class constants are staged in LDS by the kernels. */
int stg_set_params(stg_ctx* ctx, const stg_device_params* table, int32_t n_classes, const uint8_t* cls);

/* ---- env level ---------------------------------------------------------------------------------------- */

/* Per-env parameters (SURVEY 8b `stg_set_params_per_env`; domain randomisation / device-to-device variation): instead of
 * a class table, every env carries its own parameter record.  soa_params is a DEVICE array [STG_NPARAM][N] of doubles
 * whose rows are the double-valued fields of stg_device_params in declaration order (damping, ms, ku, volume,
 * polarization, easy_axis[3], demag[3], a_ex, area, r_p, r_ap, ref_m[3], r_series, sot_tau_dl, sot_tau_fl,
 * sot_sigma[3], vcma_xi, vcma_td, vcma_vbd, shape_demag[3]); dev_type and params_valid are DEVICE arrays uint8[N]
 * (STG_DEV_*; the host-evaluated outcome of utils/validation.py:176-234 per env).  The library copies all three.
 * Each lane derives its constants in the kernel prologue with the same arithmetic the host uses for a class table, so
 * an env gives bit-identical results either way.  Replaces a previous stg_set_params (and vice versa); stg_solve*,
 * stg_device_terms and stg_thermal_strength work on class tables only. */
#define STG_NPARAM 30
int stg_set_params_per_env(stg_ctx* ctx, const double* soa_params, const uint8_t* dev_type, const uint8_t* params_valid);

/* SpinTorqueEnv.reset (spin_torque_env.py:250-308) for the envs with mask[i] != 0 (mask NULL: all).
 * init_m / target [dev] double[3][N]: options['initial_state'] / options['target_state'] (normalised by the kernel as
 * device.validate_magnetization does); NULL: drawn on the device (normal(0,1,3) normalised; uniform choice among
 * cfg.targets) from Philox(seed, env_id, episode).  obs_out [dev] float[12][N] (cfg.out_layout = STG_OUT_RECORDS: the
 * record array, 8-byte aligned: the obs fields of every env are written -- a masked call reports the current observation of
 * the envs it leaves alone --, the reward/flag fields are zeroed for the reset envs and left untouched for the others: bytes
 * 0-47 of every record are written, bytes 48-55 of the reset envs' records only) may be NULL. */
int stg_reset(stg_ctx* ctx, const uint8_t* mask, const double* init_m, const double* target,
              uint64_t seed, float* obs_out, void* stream);

/* SpinTorqueEnv.step (spin_torque_env.py:310-407) for all N envs.
 * actions [dev]: [2][N] (row 0 current density A/m^2, row 1 pulse duration s), float32 (act_f64 = 0) or float64.
 * obs float[12][N]; reward float[N]; terminated/truncated uint8[N] (cfg.out_layout = STG_OUT_RECORDS: obs is the record
 * array uint8[N][STG_RECORD_BYTES] and the other three are ignored); optional (may be NULL): reward_f64 double[N]
 * (the reward before rounding to fp32), energy double[N] (info['energy_consumed'], spin_torque_env.py:474-480),
 * status uint8[N] (STG_STATUS_*). */
int stg_step(stg_ctx* ctx, const void* actions, int32_t act_f64, float* obs, float* reward, double* reward_f64,
             double* energy, uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream);

/* K consecutive env steps in one launch (state stays in registers between steps).
 * actions [K][2][N]; outputs as stg_step with a leading [K] dimension (records: [K][N][STG_RECORD_BYTES]); out_every = 1
 * writes every step's outputs, 0 only the last step's (leading dimension 1).
 * autoreset != 0 (same-step auto-reset, the usual GPU vector-env convention): an env whose episode ends at step k
 * reports that step's reward / terminated / truncated, is then reset on the device (as stg_reset with NULL
 * init_m/target, Philox key cfg.seed) and its obs row holds the NEW episode's first observation; final_obs
 * (float[K or 1][12][N] -- float[K or 1][N][12] with STG_OUT_RECORDS --, may be NULL) receives the terminal observation of
 * such envs (entries of other envs untouched).  With STG_OUT_RECORDS the record array and final_obs must be 8-byte
 * aligned (the kernel stores float pairs); a misaligned pointer is rejected with STG_E_INVALID.
 * Graph capture.  stg_step, stg_step_many and stg_step_wave enqueue only kernels and memsets on `stream` (as it stands only kernels;
 * no host synchronisation, no allocation, and nothing that the host counts from launch to launch: the RK45 lane-refill kernel puts
 * the cursors of its queue back to zero itself when its last wavefront retires), so a call may be captured in a graph and replayed
 * any number of times, also interleaved with eager calls on the same context: a replay gives the bits of the eager call.  Launches
 * of one context must be ordered (one stream, or streams ordered by events): they share the context's lane schedule and refill
 * cursors.  A captured launch bakes in
 *   - the static buffers: the action, table and output pointers of the call, and the context's state and scratch;
 *   - the slot of the placement ring it was given at capture: a replay overwrites that slot, and stg_get_placement's launches_back
 *     counts host calls, not replays. */
int stg_step_many(stg_ctx* ctx, int32_t K, const void* actions, int32_t act_f64, int32_t out_every, int32_t autoreset,
                  float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                  uint8_t* truncated, uint8_t* status, void* stream);

/* SpinTorqueEnv.step for the M envs env_ids[0..M) only (ABI v5; EnvPool-style asynchronous stepping, event-driven control,
 * curricula in which some envs wait).  Semantics: stg_step_many with K = 1 applied to the listed envs -- autoreset and cfg.skip_done
 * as there, for every solver, thermal field, class table, per-env parameter records, torque model, out_layout and action dtype --
 * while every other env's state stays bit for bit as it is.  An env's results do not depend on which other envs share the launch.
 *   env_ids [dev] uint32[M]; actions [dev] [2][M] in LIST order (float32, act_f64 = 0, or float64).
 *   Outputs are compact and in list order: output j belongs to env_ids[j].  STG_OUT_SOA: obs float[12][M], reward float[M],
 *   terminated / truncated / status uint8[M]; STG_OUT_RECORDS: obs is the record array uint8[M][STG_RECORD_BYTES].  final_obs,
 *   reward_f64, energy, status: as stg_step_many with N = M.
 *   Ids: an id >= n_envs is never dereferenced; its slot reports STG_STATUS_BAD_ID with a zero observation, reward and flags.
 *   Duplicate ids give unspecified results for those envs, but no access leaves the arrays.
 *   workspace [dev]: stg_step_ids_workspace_bytes(ctx, M) bytes (one sized for M serves every smaller list), 16-byte aligned, owned by
 *   the caller.  It holds the launch's lane schedule, its slot-order actions and -- RK45 lane-refill launches -- its own queue cursors,
 *   zeroed by hipMemsetAsync on `stream`: the call enqueues kernels and memsets only, touches no context-owned scratch other than the
 *   on-device counters (atomics) and the placement ring, and can be captured in a graph and replayed.
 * Concurrency contract.  Launches of one context on different streams may overlap if
 *   (1) each has its own workspace (and its own output arrays), and
 *   (2) their id sets are disjoint at 128-byte-line granularity: env records are 64 B, so envs 2k and 2k+1 share a line -- both ids of a
 *       pair are in one in-flight set, or the partner is in none.
 * (2) is needed because the L2 caches of the XCDs are not coherent with one another: a kernel that writes env 2k while another one on
 * another XCD holds a stale clean copy of the same line (env 2k+1 written) could write that stale half back.  Pair-closed sets never
 * share a line, so no kernel-boundary cache action is relied on.  The schedule heuristics (lane sort above 64 ids, wave specialisation
 * up to 65 536, RK45 lane refill, all decided by M) never change results.  The C-ABI caller owns the bookkeeping; SpinTorqueVecEnv's
 * send/recv pool enforces both conditions. */
size_t stg_step_ids_workspace_bytes(const stg_ctx* ctx, int64_t M);
int stg_step_ids(stg_ctx* ctx, int64_t M, const uint32_t* env_ids, const void* actions, int32_t act_f64, int32_t autoreset,
                 void* workspace, float* obs, float* final_obs, float* reward, double* reward_f64, double* energy,
                 uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream);

/* state access for parity checks and checkpoint/resume; all pointers [dev], any may be NULL.
 * m, target: double[3][N]; total_energy: double[N]; step_count: int32[N]; rng_step: uint32[N]; done: uint8[N] */
int stg_get_state(stg_ctx* ctx, double* m, double* target, double* total_energy, int32_t* step_count,
                  uint32_t* rng_step, uint8_t* done, void* stream);
int stg_set_state(stg_ctx* ctx, const double* m, const double* target, const double* total_energy,
                  const int32_t* step_count, const uint32_t* rng_step, const uint8_t* done, void* stream);

/* On-device metrics since creation / the last reset of the counters ([host] out[4]): env steps taken, integrator
 * work units (RK4/Euler sub-steps, RK45 attempted steps), reserved, steps that ended as STG_STATUS_NOOP.
 * Stands in for the host-side bookkeeping of EnvironmentMonitor / RobustLLGSSolver.get_statistics
 * (utils/monitoring.py:30-268, utils/robust_solver.py:311-328).  Synchronises the device. */
int stg_get_counters(stg_ctx* ctx, uint64_t* out, int32_t reset);

/* Where the dispatcher placed the wavefronts of a recent step launch, and when each ran (ABI v4).  The launch schedules of this
 * library (which 64-env block a wavefront takes) are speed heuristics built on observed dispatcher behaviour; every step launch
 * records, once per wavefront, the SIMD it ran on and the real-time counter when it started and when it retired, so that a caller
 * (bench.py: `roofline.placement`) can tell "this run got an unlucky placement" from "this build is slower" and see the per-SIMD
 * timeline of a launch.  launches_back = 0 addresses the most recent step launch of the context, 1 the one before, ... (the last 32
 * are kept).  out [host] receives STG_PLACEMENT_WORDS_PER_WAVE words per wavefront, wavefront index = workgroup *
 * waves_per_workgroup + wavefront (the first 4096 wavefronts of the launch; cap = size of out in words):
 *   word 0: bits 0-15 = HW_ID[15:0] (bits 5:4 SIMD, 11:8 CU, 12 SH, 15:13 SE), bits 16-19 = XCC_ID, bit 20 = producer wavefront of a
 *           wave-specialised pair, bit 31 = valid (a workgroup beyond the batch leaves 0)
 *   word 1, word 2: low 32 bits of the 100 MHz real-time counter (s_memrealtime) at the wavefront's start / when it retired (0: the
 *           wavefront had no env)
 *   word 3: the wavefront's work -- the largest number of integrator work units (sub-steps / RK45 attempts) any of its lanes did in
 *           this launch; 0 for a producer
 * Returns the number of WAVEFRONTS written or a negative error.  Synchronises the device.  Cost per launch: two s_getreg, two
 * s_memrealtime, a six-step lane reduction and four 4-byte stores per wavefront, nothing inside any loop.  The reference has no counterpart (its bookkeeping is
 * host-side: utils/monitoring.py:30-268). */
#define STG_PLACEMENT_WORDS_PER_WAVE 4
int stg_get_placement(stg_ctx* ctx, int32_t launches_back, uint32_t* out, int32_t cap, int32_t* n_workgroups,
                      int32_t* waves_per_workgroup);

/* ---- solver level ------------------------------------------------------------------------------------- */

/* RobustLLGSSolver.solve / LLGSSolver.solve over (0, T[i]) for N independent problems.  stg_solve and stg_solve_traj integrate
 * the rectangular form -- current_func(t) = J[i] if t <= T[i] else 0 and zero applied field, as SpinTorqueEnv._simulate_dynamics
 * calls the solvers (spin_torque_env.py:442-459); stg_solve_wave below takes current_func(t) and field_func(t) as
 * piecewise-linear tables.  m0 double[3][N]; J, T double[N]; m_final double[3][N] (last trajectory row; m0 when success = 0);
 * n_points int32[N] (RK4/Euler: sub-steps n; RK45: accepted points excluding t0); success uint8[N].
 * env_step: Philox counter word (thermal on only).  Uses the context's config and parameter table/classes. */
int stg_solve(stg_ctx* ctx, const double* m0, const double* J, const double* T, uint32_t env_step,
              double* m_final, int32_t* n_points, uint8_t* success, void* stream);

/* as stg_solve, additionally recording the trajectory: the first traj_cap rows of t [traj_cap][N],
 * m [traj_cap][3][N] (normalised rows, llgs_solver.py:152-153), energy [traj_cap][N] (llgs_solver.py:239-262) and
 * torques [traj_cap][N] = |tau_stt| + |tau_fl| at each accepted point (llgs_solver.py:159-172); energy and torques are
 * the LLGSSolver result dict's by-products: RK45 only, either may be NULL; t and m may be NULL too.  Row 0 is t0.
 * Footprint: lane i writes rows 0 ... min(n_points[i], traj_cap - 1) of each array and nothing else -- the rows behind a lane's last
 * point, and everything from row traj_cap on, are left untouched (not zeroed); m_final, n_points and success do not depend on
 * traj_cap.  A failed solve (success = 0; m_final = m0): a fixed-step solve whose inputs are rejected (T <= 0, a non-finite m0,
 * an invalid parameter set) records NO row, not even row 0, and reports n_points = 0.  An RK45 solve that exhausts
 * cfg.max_attempts keeps the rows of the points it accepted until then, and n_points counts them. */
int stg_solve_traj(stg_ctx* ctx, const double* m0, const double* J, const double* T, uint32_t env_step,
                   int32_t traj_cap, double* t, double* m, double* energy, double* torques,
                   double* m_final, int32_t* n_points, uint8_t* success, void* stream);

/* The same solvers with piecewise-linear waveforms for current_func(t) [A/m^2] and field_func(t) [A/m, three components].
 *
 * A waveform is K knots, 2 <= K <= STG_MAX_KNOTS: times tk[0] < tk[1] < ... < tk[K-1], strictly increasing and finite, and values
 * vk (finite).  Its value at time t:
 *   t <= tk[0]   -> vk[0]
 *   t >= tk[K-1] -> vk[K-1]
 *   otherwise    -> k = the largest index with tk[k] <= t (k <= K-2),
 *                   v = vk[k] + (t - tk[k]) * ((vk[k+1] - vk[k]) / (tk[k+1] - tk[k]))
 *                   in IEEE fp64 with the quotient rounded first, then the product, then the sum (no FMA contraction); each field
 *                   component is evaluated separately.
 * The integration span is still (0, T[i]); the knots need not cover it and may extend past it.  A current table has no built-in
 * t <= T gate: what the table says is what the solver sees, also at a stage time an ulp beyond T (the gate belongs to the
 * rectangular form only).  The solvers use the value as the reference does, per RHS call at that call's own time:
 *   RK4 / Euler (simple_solver.py:297-388): the Slonczewski term is on iff |current| > 1e-12 at that stage, h_applied is added to
 *     the effective field; stage times are t_i, t_i + dt/2, t_i + dt with t_i = i * dt (np.linspace).  RobustLLGSSolver's gates
 *     (robust_solver.py:152-205) apply as in stg_solve.
 *   RK45 (llgs_solver.py:92-126,182-237): torques are off iff |current| < 1e-12, h_applied starts h_eff; stage times are
 *     t + c h (SciPy rk_step).  The by-products of each accepted point use the waveforms at that point's time: energy includes the
 *     Zeeman term -mu_0 Ms V m.h_applied (llgs_solver.py:250), torques use current(t).
 *
 * Tables are per problem, problem index fastest [dev]: tj, jk double[kj][N]; th double[kh][N]; hk double[kh][3][N].
 *   kj = 0: no current table -- the rectangular J[i] while t <= T[i] of stg_solve (J must be non-NULL; tj, jk unused).  With kj > 0, J
 *           is not read and may be NULL.
 *   kh = 0: zero field (th, hk unused).
 * A knot count of 1 or above STG_MAX_KNOTS (or negative), a missing pointer, or traj_cap < 0 returns STG_E_INVALID with nothing
 * launched.  Table CONTENTS are checked on the device: a problem whose table is not strictly increasing or not finite fails like a
 * rejected input -- success = 0, m_final = m0, n_points = 0, no trajectory row -- and leaves the other problems as they are.
 *
 * traj_cap = 0 (t, m, energy, torques then unused, NULL) is the plain solve; traj_cap >= 1 records as stg_solve_traj does, with the
 * same footprint: lane i writes rows 0 ... min(n_points[i], traj_cap - 1) of each array and nothing else -- the rows behind a lane's
 * last point, and everything from row traj_cap on, are left untouched (not zeroed); m_final, n_points and success do not depend on
 * traj_cap.  energy and torques are RK45 only; any of t, m, energy, torques, n_points, success may be NULL.  A failed solve
 * (success = 0; m_final = m0): a solve whose inputs are rejected (fixed-step: T <= 0, a non-finite m0, an invalid parameter set; any
 * solver: a bad table) records NO row, not even row 0, and reports n_points = 0.  An RK45 solve that exhausts cfg.max_attempts keeps
 * the rows of the points it accepted until then, and n_points counts them.
 * Enqueues kernels only (no synchronisation, no allocation); works on the class table (stg_set_params), as stg_solve does.  The
 * thermal field draws from the same per-problem stream as stg_solve: with all-zero tables the two agree up to rounding. */
int stg_solve_wave(stg_ctx* ctx, const double* m0, const double* J, const double* T, int32_t kj, const double* tj,
                   const double* jk, int32_t kh, const double* th, const double* hk, uint32_t env_step, int32_t traj_cap,
                   double* t, double* m, double* energy, double* torques, double* m_final, int32_t* n_points, uint8_t* success,
                   void* stream);

/* Monte-Carlo switching statistics, reduced on the device: R thermal trials of each of G conditions, of which only integer counts
 * reach memory.  A trial is a chain of up to P rectangular-pulse solves ("phases", e.g. equilibrate, pulse, relax) that starts from
 * the condition's m0 and hands each phase's final m to the next.
 *
 * Stream rule: trial r (trial0 <= r < trial0 + R) of condition g IS problem i = g * trial_stride + r of stg_solve -- phase p is the
 * solve of stg_solve with (m, J[p][g], T[p][g]) at Philox counter word env_step + p modulo 2^32 on the stream of env id env_id0 + i (env_id0 of
 * stg_create), with the context's solver, thermal field and class row.  With P = 1 and trial_stride = R the G * R trials are the
 * problems of ONE stg_solve over the arrays replicated R times per condition, and the counts below equal the host's reduction of
 * that call's m_final and success exactly.
 *   A phase with T[p][g] == 0.0 exactly is skipped (m passes through; it is not a failed solve).
 *   A phase whose solve fails (success = 0 in stg_solve's terms) ends the trial with the m that solve hands back; the trial adds
 *   one to n_failed[g] and is classified like any other.
 * Classification of a trial's last m against the condition's target row, in IEEE fp64 without FMA contraction:
 *   proj = ((m.x * target[0][g]) + (m.y * target[1][g])) + (m.z * target[2][g])
 *   switched iff proj > threshold                                   (a NaN proj is not switched)
 *   bin = min(n_bins - 1, max(0, (int)floor((proj + 1.0) * (0.5 * n_bins))))      (a NaN proj goes to bin 0)
 * i.e. n_bins equal bins over [-1, 1], the outer two open-ended.
 *
 * m0, target double[3][G]; J, T double[P][G] (condition index fastest); cond_cls uint8[G] selects each condition's row of the
 * context's class table (stg_set_params; a value >= n_classes reads class 0, as stg_solve's cls does) or NULL: class 0 for all --
 * the context's own cls array and n_envs play no part.  1 <= P <= STG_MAX_PHASES, 0 <= n_bins <= STG_MAX_BINS.
 * The call ADDS to n_switched[G], n_failed[G] and hist[G][n_bins] (NULL iff n_bins == 0); the caller zeroes them.  So chunks of a
 * trial range (trial0), or ranks of a sharded job, sum to the counts of one call; the counts do not depend on how the library
 * spreads the trials over wavefronts.  It touches no other memory and nothing beyond those G, G and G * n_bins elements.
 * Launch: one 64-lane wavefront per workgroup works on one condition; below STG_SWITCH_STATS_WAVES wavefronts in all each lane runs
 * one trial, above it each lane loops over as many trials as keep the launch at about that many wavefronts.  A single call runs
 * all R trials in one launch: callers sharing a device should bound R per call (the Python method does).
 * Enqueues kernels only (no allocation, no synchronisation).  Per-env parameters (stg_set_params_per_env) return STG_E_STATE, as
 * for stg_solve*.  STG_E_INVALID with nothing launched: a NULL ctx / m0 / J / T / target / n_switched / n_failed, hist NULL with
 * n_bins > 0 or non-NULL with n_bins == 0, G < 1, R < 0, P or n_bins out of range, trial0 < 0, trial_stride < trial0 + R (the
 * streams of two conditions would overlap), G * trial_stride (+ env_id0) beyond int64.  R == 0 is valid and does nothing. */
#define STG_MAX_PHASES 4
#define STG_MAX_BINS 64
#define STG_SWITCH_STATS_WAVES 12288       /* 12 per SIMD of a 256-CU device: whole rounds at 2, 3, 4 or 6 resident wavefronts per SIMD */
int stg_switch_stats(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P,
                     const double* m0, const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step,
                     const double* target, double threshold, int32_t n_bins, unsigned long long* n_switched,
                     unsigned long long* n_failed, unsigned long long* hist, void* stream);

/* Write - verify - write switching statistics, reduced on the device: the write-error rate after at most A attempts and the number
 * of pulses that costs, which is how an MRAM macro writes -- after the pulse the bit is read, and only a bit that failed gets another,
 * usually stronger or longer, pulse.  Like stg_switch_stats it holds no per-trial memory (A chained stg_solve launches with a host-side
 * mask cost 69 bytes per trial), so the regime where the error after a retry is a product of two small numbers is bounded by time.
 *
 * Trial: trial r (trial0 <= r < trial0 + R) of condition g is up to A attempts.  Attempt a is the chain of P rectangular phases of
 * stg_switch_stats with (J[a][p][g], T[a][p][g]); J, T double[A][P][G], condition index fastest.  The first attempt starts from the
 * condition's m0, every later attempt from the m the attempt before left behind.  1 <= A <= STG_MAX_VERIFY_ATTEMPTS.
 * Stream rule: phase p of attempt a IS the solve of stg_solve with (m, J[a][p][g], T[a][p][g]) at Philox counter word
 * env_step + a * P + p modulo 2^32 on the stream of env id env_id0 + g * trial_stride + r, with the context's solver, thermal field and
 * class row (cond_cls as in stg_switch_stats).  A phase with T == 0.0 exactly is skipped (m passes through; it is not a failed solve).
 * Verify: after every attempt the trial is classified by stg_switch_stats' arithmetic, IEEE fp64 without FMA contraction:
 *   proj = ((m.x * target[0][g]) + (m.y * target[1][g])) + (m.z * target[2][g])
 *   switched iff proj > threshold                                   (a NaN proj is not switched)
 * End of a trial: it ends at attempt a when it is classified switched after attempt a, or when a phase of attempt a fails, or when
 * a == A - 1.  A failed phase (success = 0 in stg_solve's terms) ends its attempt with the m that solve hands back, adds one to
 * n_failed[g], and the trial is classified like any other.
 * Outputs, all ADDED to (the caller zeroes them):
 *   n_ended_at[A][G]      trials whose last attempt was a
 *   n_switched_at[A][G]   those of them classified switched
 *   n_failed[G]
 *   hist[G][n_bins]       of the final proj, with stg_switch_stats' bin rule; NULL iff n_bins == 0
 * Hence sum_a n_ended_at[a][g] = R; the trials that ran attempt a number R - sum_{b<a} n_ended_at[b][g]; the write-error rate after
 * a + 1 attempts is 1 - sum_{b<=a} n_switched_at[b][g] / R.  No other memory is touched, and nothing beyond those A * G, A * G, G and
 * G * n_bins elements.  Chunks of a trial range (trial0) and ranks of a sharded job add up to one call's integers.
 * A == 1: n_switched_at[0], n_failed and hist are those of stg_switch_stats on the same arguments, integer for integer.
 * Launch rule: one 64-lane wavefront per workgroup works on one condition; W wavefronts per condition,
 * W = min(ceil(R / 64), max(1, cap / G)), cap = max_waves if max_waves > 0, else STG_SWITCH_STATS_WAVES.  Lane l of wavefront w runs its
 * own list of trials, w * 64 + l + k * 64 * W (k = 0, 1, ...), moving on to the next one as soon as a trial ends, so a wavefront stays
 * full until its lanes run out of trials; the counts never depend on W.  max_waves lets a caller sharing a device bound the launch's width.
 * Enqueues kernels only (no allocation, no synchronisation).  Rectangular phases only: piecewise-linear tables and first-passage
 * times under verify are follow-ups; a population of devices is stg_switch_verify_population.  Per-env parameters (stg_set_params_per_env) return STG_E_STATE.
 * STG_E_INVALID with nothing launched and nothing written: everything stg_switch_stats lists (n_switched_at, n_ended_at in the place
 * of n_switched), A outside 1 ... STG_MAX_VERIFY_ATTEMPTS, max_waves < 0 or 0 < max_waves < G.  env_step + A * P is formed modulo
 * 2^32, as in the siblings: a counter word that wraps is not an error.  R == 0 is valid and does nothing. */
#define STG_MAX_VERIFY_ATTEMPTS 8
int stg_switch_verify(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t A, int32_t P,
                      const double* m0, const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step,
                      const double* target, double threshold, int32_t n_bins, int32_t max_waves,
                      unsigned long long* n_switched_at, unsigned long long* n_ended_at, unsigned long long* n_failed,
                      unsigned long long* hist, void* stream);

/* stg_switch_stats with ONE phase of the trial, `wave_phase`, driven by piecewise-linear tables: a shaped current pulse (rise time,
 * pre-emphasis, bipolar tails) and / or an applied field, per condition.  Like stg_switch_stats it holds no per-trial memory: a
 * condition's tables are read once per wavefront, whatever R is.
 *
 * Tables: layout, value rule, knot limits and validity are those of stg_solve_wave above with N = G (condition index fastest):
 * tj, jk double[kj][G]; th double[kh][G]; hk double[kh][3][G].  Times are in seconds, t = 0 at the START OF THE WAVE PHASE; there is no
 * built-in t <= T gate.  (A bias field across equilibrate, pulse and relax is one phase whose tables cover the whole trial.)
 *   kj = 0: the wave phase's current is the rectangular J[wave_phase][g] while t <= T[wave_phase][g].  With kj > 0 that J entry is not
 *           read; with kj > 0 and P == 1 no J entry is, and J may be NULL.
 *   kh = 0: zero field.
 *   kj = kh = 0 is STG_E_INVALID: the call for it is stg_switch_stats.
 *
 * Stream rule: trial r (trial0 <= r < trial0 + R) of condition g IS problem i = g * trial_stride + r.  Phase wave_phase is its solve of
 * stg_solve_wave with (m, T[wave_phase][g], condition g's tables) at Philox counter word env_step + wave_phase; every other phase p is
 * its solve of stg_solve with (m, J[p][g], T[p][g]) at env_step + p -- all modulo 2^32, on the stream of env id env_id0 + i, with the
 * context's solver, thermal field and class row.  With P = 1 and trial_stride = R the G * R trials are the problems of ONE
 * stg_solve_wave over the arrays and the tables replicated R times per condition, and the counts equal the host's reduction of that
 * call's m_final and success exactly.
 * Table CONTENTS are checked on the device, once per wavefront: a condition whose table is not strictly increasing or not finite has
 * the wave phase of every trial fail as in stg_solve_wave -- m stays the phase's input m, the trial ends there, adds one to
 * n_failed[g] and is classified like any other; the other conditions are not affected.
 *
 * Everything else is stg_switch_stats word for word: a phase with T[p][g] == 0.0 exactly is skipped (the wave phase too, bad table
 * or not), a failed phase ends the trial, the classification and the bin arithmetic, cond_cls, the launch rule; the call ADDS to
 * n_switched[G], n_failed[G] and hist[G][n_bins] and touches no other memory; it enqueues kernels only (no allocation, no
 * synchronisation); per-env parameters return STG_E_STATE.  STG_E_INVALID with nothing launched: the causes stg_switch_stats lists
 * (J == NULL only where J is read, above), wave_phase outside [0, P), a knot count of 1, negative or above STG_MAX_KNOTS, a missing
 * table pointer for a positive knot count, kj = kh = 0.  R == 0 is valid and does nothing. */
int stg_switch_stats_wave(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P,
                          const double* m0, const double* J, const double* T, int32_t wave_phase, int32_t kj, const double* tj,
                          const double* jk, int32_t kh, const double* th, const double* hk, const uint8_t* cond_cls,
                          uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                          unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist, void* stream);

/* stg_switch_stats / stg_switch_stats_wave with the question WHEN a trial switched answered for ONE phase of the trial, the watched
 * phase `watch_phase`: the first passage of m . target over `threshold` during that phase, reduced to integer counts.  Like its
 * siblings it holds no per-trial memory (the route through stg_solve_traj costs (n + 1) * 32 bytes per trial).
 *
 * Trials, streams, phases, cond_cls, the class table, the launch rule, n_switched / n_failed / hist with their classification and bin
 * arithmetic are those of stg_switch_stats_wave word for word, with watch_phase in the place of wave_phase: the tables (layout, knot
 * limits, validity, t = 0 at the start of the watched phase, a bad table fails that phase of every trial of its condition, J == NULL
 * only where J is not read) drive the watched phase.  kj = kh = 0 is VALID here: the watched phase is then the rectangular solve of
 * stg_solve, and the three old outputs are those of stg_switch_stats on the same arguments, bit for bit.
 *
 * The watched phase's points are the rows stg_solve_traj records for that solve with an unlimited traj_cap (with tables: the rows of
 * stg_solve_wave with traj_cap > 0): row k = 0 ... n_points has time t_k and magnetisation m_k, row 0 is t = 0; RK45: the
 * renormalised output row of every accepted point.  In IEEE fp64 without FMA contraction:
 *   proj_k = ((m_k.x * target[0][g]) + (m_k.y * target[1][g])) + (m_k.z * target[2][g])
 *   the trial crosses at the FIRST k with proj_k > threshold                  (a NaN never crosses)
 *   t_x = 0.0 for k = 0, else 0.5 * (t_{k-1} + t_k)                           (each operation rounded)
 *   bin = min(n_tbins - 1, max(0, (int)floor(t_x * ((double)n_tbins / T[watch_phase][g]))))     (clamped before the conversion)
 * i.e. n_tbins equal bins over the watched phase's [0, T].  t_x is the midpoint of the interval in which the crossing happened: a
 * better estimator than t_k, and one that keeps the point times of a fixed-step solve -- multiples of T / n -- off the bin edges in
 * the usual case of n_tbins dividing n.
 * A trial has NOT crossed when no row satisfies the test, when the watched phase is skipped (T == 0.0 exactly), when an earlier phase
 * failed, or when the watched phase's own solve failed by any cause (rejected input, a mid-run reset, a bad table, RK45 out of
 * attempts): whatever rows such a solve passed are discarded.
 *   n_crossed[G]         trials that crossed
 *   n_returned[G]        trials that crossed AND whose final classification is not "switched": back-hops, and pulses cut short by a
 *                        later phase
 *   t_hist[G][n_tbins]   the time histogram of the crossed trials; 0 <= n_tbins <= STG_MAX_TBINS, NULL iff n_tbins == 0
 * The call ADDS to all six arrays and touches no other memory; it enqueues kernels only; per-env parameters return STG_E_STATE.
 * STG_E_INVALID with nothing launched and nothing written: the causes stg_switch_stats_wave lists except kj = kh = 0, watch_phase
 * outside [0, P), n_tbins out of range, n_crossed or n_returned NULL, t_hist NULL with n_tbins > 0 or non-NULL with n_tbins == 0.
 * R == 0 is valid and does nothing. */
#define STG_MAX_TBINS 1024
int stg_switch_times(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P,
                     const double* m0, const double* J, const double* T, int32_t watch_phase,
                     int32_t kj, const double* tj, const double* jk, int32_t kh, const double* th, const double* hk,
                     const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                     unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist,
                     int32_t n_tbins, unsigned long long* n_crossed, unsigned long long* n_returned,
                     unsigned long long* t_hist, void* stream);

/* stg_switch_times over a POPULATION of devices: the switching statistics of a chip whose bits scatter in damping, Ms, K_u, volume and
 * polarization, not of one device.  A condition's class row (cond_cls) is the NOMINAL device; every trial belongs to a device drawn
 * around it, and integrates with that device's own derived constants -- its thermal strength follows its own volume, Ms and damping.
 * No per-device memory is held: the number of devices is bounded by time, not by STG_MAX_CLASSES.
 *
 * The draw.  Five fields vary, the first STG_NVARY doubles of stg_device_params in declaration order: damping, ms, ku, volume,
 * polarization (k = 0 ... 4).  Every other field, dev_type and params_valid are the nominal record's (the record stg_set_params was
 * given for the condition's class).
 *   Device identity: trial r of condition g (the ABSOLUTE trial index, trial0 <= r < trial0 + R) belongs to device d = r / Q (integer
 *   division), Q = trials_per_device >= 1.  The device's draws come from the stream of env id env_id0 + g * trial_stride + d * Q -- the
 *   id of the device's first trial -- at Philox counter word var_step, tag 0, calls 0 and 1: exactly the six normals z_0 ... z_5 that
 *   stg_thermal_normals(env_step = var_step, call0 = 0, n_calls = 2) dumps for that env id.  z_0 ... z_4 are used, z_5 is discarded.
 *   A device therefore depends on (cfg.seed, that env id, var_step) and on nothing else: not on chunks (trial0), ranks, the number of
 *   trials per lane or the grid.
 *   Arithmetic, IEEE fp64, each operation rounded, no FMA contraction:
 *       zc_k    = min(max(z_k, -z_clip), z_clip)
 *       f_k     = 1.0 + sigma[k][g] * zc_k
 *       value_k = nominal_k * f_k
 *   sigma[k][g] == 0 gives the nominal value bit for bit.  The device's row of derived constants is formed from the varied record by
 *   the arithmetic that forms a class table row (gamma and temperature of the configuration), so a trial of device d equals, bit for
 *   bit, the same trial run on a class table that holds device d's record.
 *   Validity: a condition's sigma column is checked on the device, once per wavefront, like a bad knot table.  It is bad if an entry
 *   is negative or not finite, or if sigma[k][g] * z_clip >= 1.0 (a parameter could come out non-positive).  A bad column makes every
 *   trial of that condition fail at its first phase that is not skipped: m stays m0, n_failed[g] gains one, the trial is classified
 *   like any other and has not crossed.  The other conditions are not affected.
 *
 * Arguments: those of stg_switch_times, with this difference: n_crossed and n_returned may BOTH be NULL when n_tbins == 0 (t_hist is
 * NULL then anyway); the first passage is then not observed at all and the watched phase runs as in stg_switch_stats(_wave).
 * watch_phase still names the phase the tables drive.  Then:
 *   sigma [dev] double[STG_NVARY][G], condition index fastest; z_clip finite and > 0; var_step; trials_per_device = Q;
 *   dev_switched [dev] or NULL, with dev_stride: dev_switched[g * dev_stride + d] gains one per switched trial of device d.  It is
 *   indexed by the ABSOLUTE device id, so every chunk and every rank adds into the same array; only the elements
 *   trial0 / Q ... (trial0 + R - 1) / Q of each condition are touched.
 * Everything else is stg_switch_times word for word: the stream rule of the trials, the phases, skipped and failed phases, the
 * classification and both bin rules, the first passage, cond_cls, the launch rule; the call ADDS to its output arrays and touches no
 * other memory; it enqueues kernels only (no allocation, no synchronisation); per-env parameters return STG_E_STATE.  With every sigma
 * 0 the six outputs of stg_switch_times are reproduced integer for integer.
 * STG_E_INVALID with nothing launched and nothing written: every cause stg_switch_times lists (n_crossed / n_returned: one of them
 * NULL, or both NULL with n_tbins > 0); sigma NULL; z_clip not finite or <= 0; trials_per_device < 1; var_step equal to env_step + p
 * modulo 2^32 for some p < P (the device's draw would reuse a thermal stream of its own first trial); dev_switched non-NULL with
 * dev_stride < (trial0 + R + Q - 1) / Q; G * dev_stride beyond int64.  R == 0 is valid and does nothing. */
#define STG_NVARY 5
int stg_switch_population(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t P,
                          const double* m0, const double* J, const double* T, int32_t watch_phase,
                          int32_t kj, const double* tj, const double* jk, int32_t kh, const double* th, const double* hk,
                          const uint8_t* cond_cls, uint32_t env_step, const double* target, double threshold, int32_t n_bins,
                          unsigned long long* n_switched, unsigned long long* n_failed, unsigned long long* hist,
                          int32_t n_tbins, unsigned long long* n_crossed, unsigned long long* n_returned,
                          unsigned long long* t_hist, const double* sigma, double z_clip, uint32_t var_step,
                          int64_t trials_per_device, unsigned long long* dev_switched, int64_t dev_stride, void* stream);

/* The devices of stg_switch_population made observable (the diagnostic twin of stg_thermal_normals): the parameters, and optionally
 * the raw normals, of devices dev0 ... dev0 + D - 1 of each of the G conditions, formed by the device function the trial kernel calls.
 *   params [dev] double[STG_NVARY][G][D]   (device index fastest): damping, ms, ku, volume, polarization of device dev0 + j
 *   z      [dev] double[6][G][D] or NULL:  the device's six normals, z_5 included
 * A condition with a bad sigma column (above) gets NaN parameters; its normals are still written.  G, trials_per_device,
 * trial_stride, var_step, z_clip, sigma and cond_cls mean what they mean in stg_switch_population; the env id of device d of condition
 * g is env_id0 + g * trial_stride + d * trials_per_device.  Enqueues one kernel; writes those arrays and nothing else.
 * Per-env parameters return STG_E_STATE.  STG_E_INVALID with nothing launched: a NULL ctx / sigma / params, G < 1, D < 0, dev0 < 0,
 * trials_per_device < 1, a bad z_clip, (dev0 + D - 1) * trials_per_device >= trial_stride (the device's first trial would lie in the
 * next condition's streams), G * trial_stride (+ env_id0) beyond int64, G * D above 2^40.  D == 0 is valid and does nothing. */
int stg_switch_population_devices(stg_ctx* ctx, int32_t G, int64_t D, int64_t dev0, int64_t trials_per_device, int64_t trial_stride,
                                  uint32_t var_step, double z_clip, const double* sigma, const uint8_t* cond_cls, double* params,
                                  double* z, void* stream);

/* stg_switch_verify over a POPULATION of devices: write - verify - write on a chip whose bits scatter.  On one device the attempts
 * of a trial are nearly independent and the error after A attempts falls about geometrically; on a chip a weak bit stays weak, the
 * retries are correlated, and the residual error is set by the tail of the device distribution.  No per-trial and no per-device
 * memory is held beyond the optional counts below.
 *
 * It is stg_switch_verify word for word -- trials, attempts, phases, the stream rule env_step + a * P + p, skipped and failed
 * phases, the verify arithmetic, the bin rule, the launch rule, max_waves, outputs that are ADDED to -- with ONE difference: every
 * trial integrates with the row of its own device.  The draw is stg_switch_population's word for word: absolute trial r of condition
 * g belongs to device d = r / Q, Q = trials_per_device; the device's normals are calls 0 and 1 of the stream of env id
 * env_id0 + g * trial_stride + d * Q at counter word var_step, tag 0; the five varied fields, the arithmetic, the clip and the derived
 * row are those stated there, so stg_switch_population_devices dumps exactly these devices.  With every sigma 0 the four outputs of
 * stg_switch_verify are reproduced integer for integer; with A == 1, n_switched_at[0], n_failed, hist and dev_switched_at[0] are
 * those of stg_switch_population without tables and without the first passage.
 *   sigma [dev] double[STG_NVARY][G]; z_clip finite and > 0; var_step; trials_per_device = Q >= 1;
 *   dev_switched_at [dev] or NULL, unsigned long long[A][G][dev_stride]: element (a * G + g) * dev_stride + d gains one per trial of
 *   device d (the ABSOLUTE device id) that ended switched at attempt a.  For each (a, g) only the elements
 *   trial0 / Q ... (trial0 + R - 1) / Q are touched, so chunks and ranks add into one array.
 * A bad sigma column (stg_switch_population: the rule) is found on the device, once per wavefront: every trial of that condition
 * fails at its first phase that is not skipped -- with a phase to run in attempt 0 the trial ends at attempt 0 with m = m0, adds one
 * to n_failed[g] and to n_ended_at[0][g], and is classified and binned like any other.  The other conditions are not affected.
 * Enqueues kernels only.  Per-env parameters return STG_E_STATE.  STG_E_INVALID with nothing launched and nothing written: everything
 * stg_switch_verify lists; sigma NULL; z_clip not finite or <= 0; trials_per_device < 1; var_step equal to env_step + k modulo 2^32
 * for some k < A * P (the device's draw would reuse a thermal stream of its own first trial); dev_switched_at non-NULL with
 * dev_stride < (trial0 + R + Q - 1) / Q; A * G * dev_stride beyond int64.  R == 0 is valid and does nothing. */
int stg_switch_verify_population(stg_ctx* ctx, int32_t G, int64_t R, int64_t trial0, int64_t trial_stride, int32_t A, int32_t P,
                                 const double* m0, const double* J, const double* T, const uint8_t* cond_cls, uint32_t env_step,
                                 const double* target, double threshold, int32_t n_bins, int32_t max_waves,
                                 unsigned long long* n_switched_at, unsigned long long* n_ended_at, unsigned long long* n_failed,
                                 unsigned long long* hist, const double* sigma, double z_clip, uint32_t var_step,
                                 int64_t trials_per_device, unsigned long long* dev_switched_at, int64_t dev_stride, void* stream);

/* SpinTorqueEnv.step for all N envs with the drive of stg_solve_wave: current_func(t) and field_func(t) as piecewise-linear tables
 * in place of the rectangular pulse in zero field of stg_step (spin_torque_env.py:442-447).
 *
 * Actions are parsed exactly as in stg_step (safety clamp, NaN/Inf -> (0, 1e-12), clips to cfg.max_current / cfg.max_duration).  The
 * parsed T[i] is the integration span (0, T[i]); the parsed J[i] and T[i] fill obs[10], obs[11] and the last-action fields as in
 * stg_step.  With kj > 0 the parsed J is not the drive.
 * Tables: layout, value rule, knot limits and validity are those of stg_solve_wave above (env index fastest: tj, jk double[kj][N];
 * th double[kh][N]; hk double[kh][3][N]; times absolute, in seconds, t = 0 at the start of this pulse; no built-in t <= T gate).
 *   kj = 0: the rectangular J[i] while t <= T[i] (tj, jk unused);  kh = 0: zero field (th, hk unused).
 *   kj = kh = 0 is stg_step: the kernel then runs stg_step's own integrator and every output, the state and the counters equal
 *   stg_step's bit for bit (thermal field included: the Philox key is (cfg.seed, env_id0 + i, stream position), as there).
 * A knot count of 1 or above STG_MAX_KNOTS (or negative) or a missing pointer returns STG_E_INVALID with nothing launched.  Table
 * CONTENTS are checked on the device: an env whose table is not strictly increasing or not finite takes the failed-solve path --
 * STG_STATUS_NOOP, m unchanged, energy 0 -- and the step still counts (step count, stream position, counters); other envs are not
 * affected.
 * Energy of the pulse (info['energy_consumed']; with R = the resistance of m before the step, A = the area):
 *   kj = 0: stg_step's (J R A)^2 / R * T  (0 when |J| <= 1e-12);
 *   kj > 0: E = ((R A) * (R A)) / R * I,  I = the integral of j(t)^2 over [0, T], in closed form per env, in knot order, IEEE fp64
 *           without FMA contraction, starting from I = 0:
 *             if tk[0] > 0:      I = min(tk[0], T) * (vk[0] * vk[0])
 *             for k = 0 ... K-2, with a = max(tk[k], 0), b = min(tk[k+1], T), if b > a:
 *                 s  = (vk[k+1] - vk[k]) / (tk[k+1] - tk[k])
 *                 ja = vk[k]   if a == tk[k]   else vk[k] + (a - tk[k]) * s          (the table's values at a and at b)
 *                 jb = vk[k+1] if b == tk[k+1] else vk[k] + (b - tk[k]) * s
 *                 I  = I + ((b - a) * ((ja * ja + ja * jb) + jb * jb)) / 3
 *             if T > tk[K-1]:    I = I + (T - max(tk[K-1], 0)) * (vk[K-1] * vk[K-1])
 * Outputs, cfg.out_layout (SoA and records), autoreset with final_obs, cfg.skip_done, the status values and the counters: as
 * stg_step_many with K = 1.  All three solvers, with and without the thermal field (cfg.noise_model = 1 for the fixed-step solvers
 * included), class tables (stg_set_params with cls).
 * Limits, each a checked error with nothing launched: per-env parameter records (stg_set_params_per_env) -> STG_E_STATE;
 * cfg.torque_model = 1 -> STG_E_INVALID.
 * One kernel, one env per lane in env order (no lane sort, no wave specialisation, no refill).  Enqueues that kernel only: no
 * synchronisation, no allocation, none of the context's launch scratch (the on-device counters take atomics) -- the call can be
 * captured in a graph.  stg_get_placement does not see these launches. */
int stg_step_wave(stg_ctx* ctx, const void* actions, int32_t act_f64, int32_t autoreset, int32_t kj, const double* tj,
                  const double* jk, int32_t kh, const double* th, const double* hk, float* obs, float* final_obs, float* reward,
                  double* reward_f64, double* energy, uint8_t* terminated, uint8_t* truncated, uint8_t* status, void* stream);

/* The env-level drive of stg_step_shaped / stg_step_shaped_ids: ONE pulse shape and ONE field table for every env and every step of the
 * context, in place of stg_step_wave's per-env tables.  All pointers [host]:
 *   tau, scale double[kj]: normalised knot times in [0, 1], strictly increasing, and factors on the action's current density -- with a
 *                          step's parsed action (J, T) the env's current table is the knots (tau_j * T, J * s_j);
 *   th double[kh]:         knot times of the field in seconds, strictly increasing, t = 0 at the start of every pulse;
 *   hk double[kh][3]:      field values in A/m.
 * Each of kj and kh is 0 (absent) or 2 ... STG_MAX_KNOTS.  kj = 0: the rectangular J while t <= T; kh = 0: zero field; kj = kh = 0
 * clears the shape (the shaped step entries then return STG_E_STATE).
 * Checked on the host, before anything else: knot counts, missing pointers, finite values, tau strictly increasing within [0, 1], th
 * strictly increasing.  A violation returns STG_E_INVALID and the previously set shape stays in force.
 * The context keeps a device copy of 6 * STG_MAX_KNOTS doubles.  Synchronises as stg_set_params does (a blocking copy, after the
 * device's work in flight): not for use during graph capture; launches captured earlier read the new shape when replayed. */
int stg_set_pulse_shape(stg_ctx* ctx, int32_t kj, const double* tau, const double* scale, int32_t kh, const double* th,
                        const double* hk);

/* K consecutive env steps in ONE launch under the shape set by stg_set_pulse_shape, state in registers between the steps: the fused
 * rollout of stg_step_many with the drive of stg_step_wave.
 * Signature, shapes (actions [K][2][N], outputs with a leading [K] or [1]), out_every, autoreset / final_obs, cfg.out_layout,
 * cfg.skip_done, alignment rules and status values are those of stg_step_many.
 * The drive of env i at step k is the shape applied to that step's parsed action (J, T):
 *   current table (kj > 0): knots (tau_j * T, J * s_j), each ONE rounded fp64 product (no contraction) -- what
 *                           spin_torque_gym_amd.envs.pulse_tables builds for stg_step_wave;  kj = 0: the rectangular J while t <= T;
 *   field table (kh > 0):   (th, hk) as set, the same for every env and step;  kh = 0: zero field.
 * Everything else is stg_step_wave as stated above: the value rule, no built-in t <= T gate, the energy ((R A) * (R A)) / R * I with
 * the closed-form I.  An env gets, bit for bit, what K calls of stg_step_wave with those tables give it (state, every output,
 * counters, thermal stream).  Products of adjacent tau can tie after rounding (or J * s_j overflow): a lane whose scaled current table
 * is not strictly increasing and finite takes stg_step_wave's bad-table path for that step only -- STG_STATUS_NOOP, m unchanged,
 * energy 0, the step still counts.
 * Limits, each a checked error with nothing launched: no shape set -> STG_E_STATE; per-env parameter records -> STG_E_STATE;
 * cfg.torque_model = 1 -> STG_E_INVALID; K < 1 or a missing mandatory pointer -> STG_E_INVALID.
 * One kernel, one env per lane in env order (no lane sort, no wave specialisation, no refill); the shape is staged in LDS, so no table
 * is read from HBM and nothing is built on the host per step.  Enqueues that kernel only -- no synchronisation, no allocation, none of
 * the context's launch scratch (the counters take atomics): the call can be captured in a graph.  stg_get_placement does not see these
 * launches. */
int stg_step_shaped(stg_ctx* ctx, int32_t K, const void* actions, int32_t act_f64, int32_t out_every, int32_t autoreset,
                    float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                    uint8_t* truncated, uint8_t* status, void* stream);

/* stg_step_shaped with K = 1 for the M envs env_ids[0..M) only, under every rule of stg_step_ids: env_ids [dev] uint32[M], actions
 * [2][M] in list order, compact outputs in list order; an id >= n_envs is never dereferenced and reports STG_STATUS_BAD_ID with zero
 * outputs; every other env's state stays bit for bit as it was; duplicate ids give unspecified results for those envs.  The same
 * concurrency contract: launches on different streams may overlap if each has its own outputs and their id sets are disjoint and
 * pair-closed at 128-byte lines (envs 2k and 2k+1).  No workspace: the schedule is identity order, there is nothing to stage.
 * M < 0 -> STG_E_INVALID; M = 0 launches nothing.  Limits and graph capture as stg_step_shaped. */
int stg_step_shaped_ids(stg_ctx* ctx, int64_t M, const uint32_t* env_ids, const void* actions, int32_t act_f64, int32_t autoreset,
                        float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                        uint8_t* truncated, uint8_t* status, void* stream);

/* The knot times of stg_step_knots / stg_step_knots_ids: the action of those entries is [J, T, s_0 ... s_{P-1}] -- the agent chooses the
 * pulse's knot amplitudes per env and per step; the knot times, the clamp of an amplitude and the field table are fixed here, once, for
 * every env and every step of the context.  All pointers [host]:
 *   tau double[P]:     normalised knot times in [0, 1], strictly increasing and finite, 2 <= P <= STG_MAX_KNOTS;
 *   s_limit:           finite and > 0: an amplitude is clamped to [-s_limit, +s_limit];
 *   th double[kh], hk double[kh][3]: the field table with the rules of stg_set_pulse_shape; kh is 0 (zero field) or 2 ... STG_MAX_KNOTS.
 * P = 0 clears the knots (the knot step entries then return STG_E_STATE).
 * Everything is checked on the host, before anything else; a violation returns STG_E_INVALID and what was set before stays in force.
 * The context keeps a device copy of 5 * STG_MAX_KNOTS doubles and synchronises as stg_set_pulse_shape does (a blocking copy, after the
 * device's work in flight): not for use during graph capture; launches captured earlier read the new knots when replayed.
 * Independent of stg_set_pulse_shape: a context may hold both, and each step entry reads its own. */
int stg_set_pulse_knots(stg_ctx* ctx, int32_t P, const double* tau, double s_limit, int32_t kh, const double* th, const double* hk);

/* K consecutive env steps in ONE launch whose actions carry the pulse's knot amplitudes, state in registers between the steps.
 * Signature, outputs (a leading [K] or [1]), out_every, autoreset / final_obs, cfg.out_layout, cfg.skip_done, alignment rules and status
 * values are those of stg_step_shaped; actions are [dev] [K][2 + P][N], float or double (act_f64), env index fastest.
 * Action parse, per env and per step, in this order:
 *   1. rows 0 and 1 go through parse_action exactly as in stg_step (safety clamp, NaN/Inf -> (0, 1e-12), clips to cfg.max_current /
 *      cfg.max_duration), giving (J, T);
 *   2. amplitude row j is converted to fp64, then clamped  s < -s_limit ? -s_limit : (s > s_limit ? s_limit : s),  which keeps NaN
 *      (and takes +-Inf to +-s_limit);
 *   3. if any amplitude of the lane is NaN the whole action is void: J = 0, T = 1e-12 and every s_j = 0 -- the values stg_step gives a
 *      NaN action;
 *   4. the lane's current table is the knots (tau_j * T, J * s_j), each ONE rounded fp64 product without contraction.
 * obs[10], obs[11] and the last-action fields hold the parsed (J, T) as today; the observation stays 12 floats.
 * Everything else is stg_step_wave as stated above: the value rule, no built-in t <= T gate, the energy ((R A) * (R A)) / R * I with the
 * closed-form I, the bad-table path for a lane whose scaled table ties or overflows (STG_STATUS_NOOP, m unchanged, energy 0, the step
 * still counts), autoreset with final_obs, cfg.skip_done, both output layouts, the counters, the thermal stream position.
 * Contract: an env gets, bit for bit, what K calls of stg_step_wave give it with the tables tj = tau_j * T, jk = J * s_j built from the
 * parsed action and the field table replicated.
 * Limits, each a checked error with nothing launched: knots not set -> STG_E_STATE; per-env parameter records -> STG_E_STATE;
 * cfg.torque_model = 1 -> STG_E_INVALID; K < 1 or a missing mandatory pointer -> STG_E_INVALID.
 * One kernel, one env per lane in env order; tau and the field table are staged in LDS, and so are the lane's parsed amplitudes at the top
 * of each step (8 * 64 * P bytes of dynamic LDS per 64-env block).  Enqueues that kernel only -- no synchronisation, no allocation, none of
 * the context's launch scratch (the counters take atomics): the call can be captured in a graph.  stg_get_placement does not see these
 * launches. */
int stg_step_knots(stg_ctx* ctx, int32_t K, const void* actions, int32_t act_f64, int32_t out_every, int32_t autoreset,
                   float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                   uint8_t* truncated, uint8_t* status, void* stream);

/* stg_step_knots with K = 1 for the M envs env_ids[0..M) only, under every rule of stg_step_shaped_ids: env_ids [dev] uint32[M], actions
 * [2 + P][M] in list order, compact outputs in list order; an id >= n_envs is never dereferenced and reports STG_STATUS_BAD_ID with zero
 * outputs; every other env's state stays bit for bit as it was; the concurrency contract of stg_step_shaped_ids applies.
 * M < 0 -> STG_E_INVALID; M = 0 launches nothing and returns 0.  Limits and graph capture as stg_step_knots. */
int stg_step_knots_ids(stg_ctx* ctx, int64_t M, const uint32_t* env_ids, const void* actions, int32_t act_f64, int32_t autoreset,
                       float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                       uint8_t* truncated, uint8_t* status, void* stream);

/* ---- device-class formulas (opt-in torque model) ------------------------------------------- */

/* Evaluates, per env, the device-class formulas the torque model uses: for SOT classes tau_dl, tau_fl of
 * SOTMRAMDevice.compute_spin_torque(J, m) (double[3][N] each, zeros for other classes), and for VCMA classes
 * K_eff(volt) of VCMAMRAMDevice._compute_effective_anisotropy (double[N]; the class' K for other classes).
 * m double[3][N], J, volt double[N]; any output may be NULL. */
int stg_device_terms(stg_ctx* ctx, const double* m, const double* J, const double* volt, double* tau_dl, double* tau_fl,
                     double* k_eff, void* stream);

/* ---- thermal field (physics/thermal_model.py:12-137; simple_solver.py:378-386; llgs_solver.py:85-90,111-113) ---- */

/* Brown field strength of class `cls` for the context's solver kind and temperature ([host] out). */
int stg_thermal_strength(stg_ctx* ctx, int32_t cls, double* out);
/* Dumps the standard normals the kernels would draw for RHS calls call0..call0+n_calls-1 of env step `env_step`:
 * z [dev] double[n_calls][3][N].  Diagnostic entry used by the distribution tests. */
int stg_thermal_normals(stg_ctx* ctx, uint32_t env_step, uint32_t call0, int32_t n_calls, double* z, void* stream);

/* ---- SpinTorqueArray-v0 (spin_torque_gym/envs/array_env.py) --------------------------------- */

typedef struct stg_array_ctx stg_array_ctx;

/* SpinTorqueArrayEnv.__init__ keyword arguments that reach the step path (array_env.py:30-52) */
typedef struct {
    int32_t rows, cols;             /* array_size; rows*cols <= 64 */
    int32_t action_mode;            /* 0 'individual' [device, J, T], 1 'row', 2 'column', 3 'global' [J, T] (:427-445) */
    int32_t include_coupling;
    int32_t max_steps;              /* 200 */
    int32_t obs_mode;               /* 0 'array' (rows*cols*6 floats), 1 'vector' (rows*cols*6 + 4) (:533-557) */
    double max_current, max_duration, success_threshold, energy_penalty_weight, temperature;
} stg_array_config;

/* n_arrays independent arrays on GPU device_id; dev = the device class of every cell (DeviceFactory.create_device per
 * cell, array_env.py:113-120); coupling [host] double[n][n] = _compute_coupling_matrix (:301-334), may be NULL when
 * include_coupling = 0.  env_id0: global index of the first array (device-side reset draws). */
int stg_array_create(stg_array_ctx** out, int device_id, int64_t n_arrays, int64_t env_id0, const stg_array_config* cfg,
                     const stg_device_params* dev, const double* coupling);
void stg_array_destroy(stg_array_ctx* ctx);

/* SpinTorqueArrayEnv.reset (array_env.py:336-360) for arrays with mask[i] != 0 (NULL: all).  init_pattern / target [dev]
 * double[rows*cols][3][N] (options['initial_pattern'] / options['target_pattern']); NULL init_pattern: normalised normal
 * draws on the device; NULL target: keep the current target (the +-z checkerboard of :161-170 at first).
 * obs_out float[obs_dim][N] or NULL. */
int stg_array_reset(stg_array_ctx* ctx, const uint8_t* mask, const double* init_pattern, const double* target,
                    uint64_t seed, float* obs_out, void* stream);

/* SpinTorqueArrayEnv.step (array_env.py:362-409) for all N arrays.  actions [dev] float[A][N], A = 3 ([index, J, T]) or
 * 2 in 'global' mode -- where, as in the reference, action[1] is read as the current density and the duration defaults
 * to 1 ns.  obs float[obs_dim][N]; reward float[N]; reward_f64 / energy double[N] or NULL; terminated / truncated uint8[N]. */
int stg_array_step(stg_array_ctx* ctx, const float* actions, float* obs, float* reward, double* reward_f64, double* energy,
                   uint8_t* terminated, uint8_t* truncated, void* stream);

/* pattern, target: double[rows*cols][3][N]; total_energy double[N]; step_count int32[N]; any may be NULL */
int stg_array_get_state(stg_array_ctx* ctx, double* pattern, double* target, double* total_energy, int32_t* step_count,
                        void* stream);

/* K steps of every array in ONE launch: the pattern stays on chip for all K steps, with optional same-step auto-reset (the array
 * env's counterpart of stg_step_many).  actions [dev] float[K][A][N].  out_every = 1: obs float[K][obs_dim][N], reward float[K][N],
 * reward_f64 / energy double[K][N] or NULL, terminated / truncated uint8[K][N]; out_every = 0: only the last step's outputs are
 * written, with a leading dimension of 1 (reward / energy are the last step's values, not sums).
 * autoreset = 0: exactly K calls of stg_array_step, finished arrays keep stepping as in the reference.  autoreset != 0: an array
 * with terminated | truncated at step k reports that step's reward and flags and is then reset in the kernel as
 * stg_array_reset(mask = that array, init_pattern = NULL, target = NULL, seed) would reset it (random pattern of the same stream,
 * its reset counter advanced, target kept, energy and step count zero); its obs column holds the new episode's first observation
 * and final_obs float[K or 1][obs_dim][N] (may be NULL) receives the terminal observation of such arrays ONLY -- other entries are
 * left untouched; the next step of the launch continues the new episode.
 * Enqueues kernels only (no host synchronisation, no scratch): may be captured in a graph.  STG_E_INVALID for K < 1, a missing
 * mandatory pointer or an array too large for the device's LDS, STG_E_STATE before the first reset; nothing is launched then. */
int stg_array_step_many(stg_array_ctx* ctx, int32_t K, const float* actions, int32_t out_every, int32_t autoreset, uint64_t seed,
                        float* obs, float* final_obs, float* reward, double* reward_f64, double* energy, uint8_t* terminated,
                        uint8_t* truncated, void* stream);

/* The inverse of stg_array_get_state plus the per-array reset counters (which key the device-side random reset draws): asynchronous
 * copies on `stream` from [dev] buffers of stg_array_get_state's shapes, resets uint32[N]; any may be NULL.  A pattern marks the
 * context as having state and a target as having a target, so a context restored with both can step without a reset. */
int stg_array_set_state(stg_array_ctx* ctx, const double* pattern, const double* target, const double* total_energy,
                        const int32_t* step_count, const uint32_t* resets, void* stream);

/* resets [dev] uint32[N]: how many device-side random resets each array has had (asynchronous copy on `stream`) */
int stg_array_get_resets(stg_array_ctx* ctx, uint32_t* resets, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPINTORQUE_HIP_H */
