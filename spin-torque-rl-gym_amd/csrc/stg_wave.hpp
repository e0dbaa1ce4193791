// stg_wave.hpp -- piecewise-linear current and field waveforms on the solve path and the env step path (stg_solve_wave, stg_step_wave,
// include/spintorque_hip.h).
//
// The solvers of the reference take current_func(t) and field_func(t); a Python callable cannot run in a kernel, a table of knots can.
// This header holds the waveform variants of the functions of stg_physics.hpp that take J as a per-solve constant (simple_solve, the
// llgs_lane_* family); the functions in which the drive enters as an argument -- llgs_rhs, validation, the RK45 controller pieces, the
// recorder, the normal stream -- are reused as they are.  Only stg_solve_wave.hip, stg_step_wave.hip, the pulse-step kernel
// (stg_step_pulse.hpp: stg_step_shaped.hip / stg_step_knots.hip) and the switching trial kernel (stg_switch.hpp: stg_switch_rk4.hip /
// _euler.hip / _rk45.hip) instantiate anything in here: the step kernels, stg_solve_kernel and the array kernels do not see this file's
// device code
// (profiles/waveform_existing_kernels_unchanged.txt, profiles/step_wave_existing_kernels_unchanged.txt,
// profiles/step_shaped_existing_kernels_unchanged.txt, profiles/step_knots_existing_kernels_unchanged.txt,
// profiles/step_pulse_existing_kernels_unchanged.txt,
// profiles/switch_stats_wave_existing_kernels_unchanged.txt, profiles/switch_family_existing_kernels_unchanged.txt).
//
// Waveform semantics (the C header states them for callers; physics.PiecewiseLinear and tests/waveform_ref.py use the same arithmetic):
//   K knots, 2 <= K <= STG_MAX_KNOTS, times tk[0] < ... < tk[K-1] finite, values vk (a scalar, or three field components).
//   t <= tk[0] -> vk[0];  t >= tk[K-1] -> vk[K-1];  otherwise k = the largest index with tk[k] <= t (k <= K-2) and
//   v = vk[k] + (t - tk[k]) * ((vk[k+1] - vk[k]) / (tk[k+1] - tk[k])):  the quotient is rounded first, then the product, then the
//   sum; no FMA contraction.  Each field component is evaluated separately.
// Tables are per problem and lane-coalesced: times double[K][N], values double[K][C][N] (GlobalKnots) -- or, for the env-level pulse
// shape of stg_step_shaped, one table for all lanes in LDS, scaled per lane (SharedKnots) -- or, for the agent-shaped pulse of
// stg_step_knots, shared times and the lane's own amplitudes, both in LDS (LaneKnots).  The solvers are templates over the source.
#pragma once

#include "stg_kernels.hpp"

struct WaveSolveArgs {
    SolveArgs s;
    int32_t kj, kh;               // knot counts; 0: rectangular J[i] while t <= T[i] / zero field
    const double *tj, *jk;        // [kj][N], [kj][N]
    const double *th, *hk;        // [kh][N], [kh][3][N]
};

// defined in stg_solve_wave.hip: enqueues the one kernel of a waveform solve
void stg_wave_launch(const WaveSolveArgs& a, int solver, bool thermal, bool multi, bool record, hipStream_t st);

// one env step with the same drive (stg_step_wave): the step launch's arguments plus the tables, [k][N] over the context's envs
struct WaveStepArgs {
    StepArgs s;
    int32_t kj, kh;
    const double *tj, *jk;
    const double *th, *hk;
    int32_t axis_z;               // which form of the rectangular solvers stg_step takes for this context (zero-table launches run it)
};

// defined in stg_step_wave.hip: enqueues the one kernel of a waveform step
void stg_step_wave_launch(const WaveStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st);

// K env steps under the context's pulse shape (stg_step_shaped, stg_step_shaped_ids): the step launch's arguments (K, out_every, and for
// the id form ids / n_state) plus the shape, which is the same for every env and every step
constexpr int STG_SHAPE_DOUBLES = 6 * STG_MAX_KNOTS;      // tau, scale, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
struct ShapedStepArgs {
    StepArgs s;
    int32_t kj, kh;               // knot counts; 0: rectangular J while t <= T / zero field (not both 0)
    const double* tab;            // [STG_SHAPE_DOUBLES] on the device (stg_set_pulse_shape)
};


// K env steps whose actions carry the pulse's knot amplitudes (stg_step_knots, stg_step_knots_ids): the step launch's arguments plus the
// knot times and the field table, which are the same for every env and every step (stg_set_pulse_knots)
constexpr int STG_KNOTS_DOUBLES = 5 * STG_MAX_KNOTS;      // tau, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
struct KnotsStepArgs {
    StepArgs s;
    int32_t kj, kh;               // amplitude knots (2 ... STG_MAX_KNOTS); field knots, 0: zero field
    double s_limit;               // the clamp of an amplitude
    const double* tab;            // [STG_KNOTS_DOUBLES] on the device (stg_set_pulse_knots)
};

// defined in stg_step_shaped.hip and stg_step_knots.hip: enqueues the pulse-step kernel (stg_step_pulse.hpp) of a shaped or an
// agent-shaped step launch (s.ids != nullptr: the id form)
void stg_step_pulse_launch(const ShapedStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st);
void stg_step_pulse_launch(const KnotsStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st);

namespace stg {

// Where a table's knots come from.  GlobalKnots: this lane's column of a per-problem table in HBM (stg_solve_wave, stg_step_wave).
// SharedKnots: ONE table for every lane, staged in LDS by the kernel (stg_step_shaped) -- with SCALED, knot time j is tk[j] * st and
// knot value j is sv * vk[j], each one rounded product: an env-level pulse shape (tau_j, s_j) under this lane's parsed action
// (st = T, sv = J) gives the knots (tau_j T, J s_j) that envs.pulse_tables writes into a global table, bit for bit.
template <int C>
struct GlobalKnots {
    const double* tk;
    const double* vk;
    int64_t N, i;
    __device__ __forceinline__ double time_at(int32_t j) const { return tk[(int64_t)j * N + i]; }
    __device__ __forceinline__ double value_at(int32_t j, int c) const { return vk[((int64_t)j * C + c) * N + i]; }
};
template <int C, bool SCALED>
struct SharedKnots {
    const double* tk;             // [K] (LDS)
    const double* vk;             // [K][C] (LDS)
    double st, sv;
    // (The index goes through an empty asm, so a knot is read where the source says so -- when a cursor opens or crosses one -- and the
    // load is not moved or merged across the sub-step loop: an LDS load cannot fault, so the compiler is otherwise free to.  Worth 4
    // VGPRs in the fixed-step kernels of stg_step_shaped.hip, profiles/NOTEBOOK.md, round 14.  A volatile load pins it too but loses
    // the LDS address space: flat loads.)
    __device__ __forceinline__ double knot(const double* p, int32_t j) const {
        asm volatile("" : "+v"(j));
        return p[j];
    }
    __device__ __forceinline__ double time_at(int32_t j) const { return SCALED ? mul_x(knot(tk, j), st) : knot(tk, j); }
    __device__ __forceinline__ double value_at(int32_t j, int c) const { return SCALED ? mul_x(sv, knot(vk, j * C + c)) : knot(vk, j * C + c); }
};

// LaneKnots: the times as SharedKnots<1, true> has them -- tk[j] * st from one table in LDS --, the values sv * vk[j * 64] from THIS
// lane's column of a [K][64] block in LDS, which the kernel fills from the lane's action at the top of each step (stg_step_knots: st = T,
// sv = J, vk = the parsed amplitudes).  A lane reads only what it wrote itself, so no barrier stands between the fill and the reads.
struct LaneKnots {
    const double* tk;             // [K] (LDS)
    const double* vk;             // this lane's column: knot j at vk[j * 64] (LDS)
    double st, sv;
    __device__ __forceinline__ double knot(const double* p, int32_t j) const {      // (as SharedKnots::knot)
        asm volatile("" : "+v"(j));
        return p[j];
    }
    __device__ __forceinline__ double time_at(int32_t j) const { return mul_x(knot(tk, j), st); }
    __device__ __forceinline__ double value_at(int32_t j, int) const { return mul_x(sv, knot(vk, j * 64)); }
};

// One lane's view of one table, with the segment cursor: k is the segment [tk[k], tk[k+1]] the last query fell into (or the first / last
// one for a query outside the table), its two knots and its slope are held in registers.  Time only moves forward between queries of one
// cursor (seek), so a query costs a compare unless it crosses a knot; the slope is recomputed then.
template <int C, class KNOTS = GlobalKnots<C>>
struct Pwl : KNOTS {
    using KNOTS::time_at;
    using KNOTS::value_at;
    int32_t K, k;
    double t0, tn;                // tk[k], tk[k+1]
    double v0[C], vn[C], sl[C];   // vk[k], vk[k+1], (vk[k+1] - vk[k]) / (tk[k+1] - tk[k])

    // the table as the C-ABI wants it: finite, times strictly increasing
    __device__ __forceinline__ bool valid() const {
        bool ok = true;
        double prev = 0.0;
        for (int32_t j = 0; j < K; ++j) {
            const double t = time_at(j);
            ok = ok && isfinite(t) && (j == 0 || t > prev);
            prev = t;
#pragma unroll
            for (int c = 0; c < C; ++c) ok = ok && isfinite(value_at(j, c));
        }
        return ok;
    }
    __device__ __forceinline__ void slopes() {
#pragma clang fp contract(off)
        const double dt = tn - t0;
#pragma unroll
        for (int c = 0; c < C; ++c) sl[c] = (vn[c] - v0[c]) / dt;
    }
    __device__ __forceinline__ void open() {
        k = 0;
        t0 = time_at(0); tn = time_at(1);
#pragma unroll
        for (int c = 0; c < C; ++c) { v0[c] = value_at(0, c); vn[c] = value_at(1, c); }
        slopes();
    }
    // moves the cursor to the segment of t (t not below the cursor's last query)
    __device__ __forceinline__ void seek(double t) {
        while (k < K - 2 && t >= tn) {
            ++k;
            t0 = tn;
            tn = time_at(k + 1);
#pragma unroll
            for (int c = 0; c < C; ++c) { v0[c] = vn[c]; vn[c] = value_at(k + 1, c); }
            slopes();
        }
    }
    // the value at t, for a cursor that seek(t) has placed
    __device__ __forceinline__ double eval(double t, int c) const {
        if (k == 0 && t <= t0) return v0[c];
        if (t >= tn) return vn[c];                      // (beyond the last knot: seek stops at k = K - 2)
        return add_x(v0[c], mul_x(sub_x(t, t0), sl[c]));
    }
};

// what the two tables (or the rectangular form) give one RHS call
struct WaveDrive {
    double cur;     // current_func(t)
    V3 h;           // field_func(t), A/m
};

// The drive of one solve: the two cursors, or -- no current table -- the rectangular pulse J while t <= T of stg_solve.  `has_j` and
// `has_h` are kernel-uniform.
template <class PJ, class PH>
struct WaveSourceT {
    PJ cj;
    PH ch;
    bool has_j, has_h;
    double J, T;
    double t_evt;       // the earliest time at which one of the cursors has to move on (+inf: never again)
    __device__ __forceinline__ void arm() {
        const double inf = __builtin_inf();
        t_evt = fmin(has_j && cj.k < cj.K - 2 ? cj.tn : inf, has_h && ch.k < ch.K - 2 ? ch.tn : inf);
    }
    // ONE compare per query while no knot is crossed
    __device__ __forceinline__ void seek(double t) {
        if (t >= t_evt) {
            if (has_j) cj.seek(t);
            if (has_h) ch.seek(t);
            arm();
        }
    }
    // (seeks first: a stage time is never below the one before it)
    __device__ __forceinline__ WaveDrive at(double t) {
        seek(t);
        WaveDrive d;
        d.cur = has_j ? cj.eval(t, 0) : (t <= T ? J : 0.0);          // spin_torque_env.py:442-443 for the rectangular form
        d.h = has_h ? V3{ch.eval(t, 0), ch.eval(t, 1), ch.eval(t, 2)} : V3{0.0, 0.0, 0.0};
        return d;
    }
};
using WaveSource = WaveSourceT<Pwl<1>, Pwl<3>>;      // per-problem tables in HBM

// I = the integral of j(t)^2 over [0, T] of one lane's current table, in closed form and in knot order (include/spintorque_hip.h,
// stg_step_wave: the same formula, which tests/wave_step_ref.py restates): a head piece where the first value holds, one piece per
// segment that overlaps [0, T], a tail piece where the last value holds.  No contraction, so NumPy gives the same bits.
template <class PJ>
__device__ __forceinline__ double pulse_sq_integral(const PJ& c, double T) {
#pragma clang fp contract(off)
    double t0 = c.time_at(0), v0 = c.value_at(0, 0);
    double I = 0.0;
    if (t0 > 0.0) I = fmin(t0, T) * (v0 * v0);
    for (int32_t k = 0; k + 1 < c.K; ++k) {
        const double t1 = c.time_at(k + 1), v1 = c.value_at(k + 1, 0);
        const double lo = fmax(t0, 0.0), hi = fmin(t1, T);
        if (hi > lo) {
            const double sl = (v1 - v0) / (t1 - t0);
            const double ja = lo == t0 ? v0 : v0 + (lo - t0) * sl;
            const double jb = hi == t1 ? v1 : v0 + (hi - t0) * sl;
            I = I + ((hi - lo) * ((ja * ja + ja * jb) + jb * jb)) / 3.0;
        }
        t0 = t1; v0 = v1;
    }
    if (T > t0) I = I + (T - fmax(t0, 0.0)) * (v0 * v0);
    return I;
}

// simple_rhs (general easy axis) with h_applied: G gains -g' h_applied (simple_solver.py:364-367,388), i.e. p = m x G gains
// q = m x (-g' h_applied).  A stage whose field is exactly zero keeps p as it is (a select per lane, not a branch): q is then a signed
// zero, and p + q would turn a -0 of p into +0 -- with the select a zero field reproduces simple_rhs bit for bit.
template <bool THERMAL>
__device__ __forceinline__ V3 simple_rhs_wave(const V3& m, const SimpleK& k, double aJ, const V3& z, bool has_field, const V3& gh, bool field_zero) {
#pragma clang fp contract(off)
    const V3 t = cross(m, k.e);
    const double c = k.ghk * dot(m, k.e);
    const double d = k.gdm * m.z;
    V3 p;
    if (THERMAL) {
        const V3 g{__builtin_fma(k.ghs, z.x, c * k.e.x), __builtin_fma(k.ghs, z.y, c * k.e.y),
                   __builtin_fma(k.ghs, z.z, __builtin_fma(c, k.e.z, d))};                // simple_solver.py:384,388
        p = cross(m, g);
    } else {
        p = V3{__builtin_fma(c, t.x, d * m.y), __builtin_fma(c, t.y, -(d * m.x)), c * t.z};
    }
    if (has_field) {          // (kernel-uniform)
        const V3 q = cross(m, gh);
        p = V3{field_zero ? p.x : p.x + q.x, field_zero ? p.y : p.y + q.y, field_zero ? p.z : p.z + q.z};
    }
    const V3 w{__builtin_fma(k.alpha, p.x, aJ * t.x), __builtin_fma(k.alpha, p.y, aJ * t.y),
               __builtin_fma(k.alpha, p.z, aJ * t.z)};
    return V3{__builtin_fma(m.y, w.z, __builtin_fma(-m.z, w.y, p.x)), __builtin_fma(m.z, w.x, __builtin_fma(-m.x, w.z, p.y)),
              __builtin_fma(m.x, w.y, __builtin_fma(-m.y, w.x, p.z))};
}

// simple_solve with the drive evaluated per RHS call at that call's own time (simple_solver.py:290-293,324-326,364-367): stage times
// t_i = i dt (np.linspace), t_i + dt/2, t_i + dt, in exactly those roundings.  One env per lane, normals inline, reference torque model.
// ngeff = -gamma/(1+alpha^2).
template <int METHOD, bool THERMAL, bool RECORD, class WS, class REC = Recorder>
__device__ __forceinline__ SolveOut simple_solve_wave(const V3& m0, double T, const SimpleK& k, double ngeff, double pol, double msv,
                                                      bool class_valid, double temperature, double max_step, const RngKey& rk,
                                                      const REC& rec, InlineNormals& ns, double inv_tau, WS& src) {
#pragma clang fp contract(off)
    SolveOut o{m0, 0, 0, 0, false};
    // robust_solver.py:152-190 (_validate_inputs); any failure ends in the fallback result (:140-150)
    if (validation_rejects(m0) || !(T > 0.0) || !class_valid || !(temperature > 0.0)) return o;
    V3 m = m0;
    bool zr;
    int resets = simple_validate(m, zr);                                   // simple_solver.py:119
    // simple_solver.py:137-139, in exactly these roundings
    double dt = fmin(max_step, (T / 100.0));
    int n = (int)(T / dt);
    n = n < 10 ? 10 : n;
    dt = T / (double)n;
    o.n = n;
    o.work = n;
    const double half_dt = 0.5 * dt, sixth_dt = dt / 6.0;
    // the rectangular form's a_J, formed once as simple_solve forms it
    const double aJ_rect = fabs(src.J) > 1e-12 ? (pol * src.J) / msv : 0.0;
    bool fail = false;
    const V3 zero{0.0, 0.0, 0.0};
    if (THERMAL) ns.begin(rk);
    const bool ou_sel = THERMAL && inv_tau != 0.0;         // Ornstein-Uhlenbeck field, or (inv_tau < 0) the Brown field: see simple_solve
    double ou_d = 0.0, ou_c = 1.0;
    V3 ou_x = zero;
    if (ou_sel) {
        if (inv_tau > 0.0) {
            ou_d = exp(-dt * inv_tau);
            ou_c = sqrt(1.0 - ou_d * ou_d);
        } else {
            ou_c = 1.0 / sqrt(dt);
        }
    }
    // The drive of one stage time: the Slonczewski term is on iff |current| > 1e-12 there (simple_solver.py:326,330).  The quotient
    // (P current) / (Ms V) is a product with 1 / (Ms V), formed once: an IEEE division per stage costs about as much as half an RHS, and
    // the product is within 1.5 ulp of the quotient.  (The rectangular form keeps simple_solve's own a_J, so that it stays bit for bit.)
    const double inv_msv = 1.0 / msv;
    struct StageDrive {
        double aJ;
        V3 gh;          // -g' h_applied
        bool fz;        // h_applied == 0 exactly
    };
    auto drive = [&](double ts) -> StageDrive {
        const WaveDrive dr = src.at(ts);
        StageDrive sd;
        if (src.has_j) sd.aJ = fabs(dr.cur) > 1e-12 ? (pol * dr.cur) * inv_msv : 0.0;
        else sd.aJ = ts <= T ? aJ_rect : 0.0;
        sd.fz = dr.h.x == 0.0 && dr.h.y == 0.0 && dr.h.z == 0.0;
        sd.gh = V3{ngeff * dr.h.x, ngeff * dr.h.y, ngeff * dr.h.z};
        return sd;
    };
    auto stage = [&](const V3& y, const StageDrive& sd, const V3& z) -> V3 {
        return simple_rhs_wave<THERMAL>(y, k, sd.aJ, z, src.has_h, sd.gh, sd.fz);
    };
    if (RECORD) rec.put(0, 0.0, m, 0.0);
    auto run = [&](auto ou_tag) {
        constexpr bool ou = decltype(ou_tag)::value;
        for (int i = 0; i < n; ++i) {
            const double ti = mul_x((double)i, dt);
            V3 mn;
            if (METHOD == 1) {
                V3 z0 = zero;
                if (THERMAL) z0 = ns.draw((i & 1) == 0);
                if (ou) {
                    ou_x = V3{__builtin_fma(ou_d, ou_x.x, ou_c * z0.x), __builtin_fma(ou_d, ou_x.y, ou_c * z0.y),
                              __builtin_fma(ou_d, ou_x.z, ou_c * z0.z)};
                    z0 = ou_x;
                }
                const V3 f = stage(m, drive(ti), z0);
                mn = V3{__builtin_fma(dt, f.x, m.x), __builtin_fma(dt, f.y, m.y), __builtin_fma(dt, f.z, m.z)};   // simple_solver.py:275-276
            } else {
                V3 z0 = zero, z1 = zero, z2 = zero, z3 = zero;
                if (ou) {
                    const V3 xi = ns.draw((i & 1) == 0);
                    ou_x = V3{__builtin_fma(ou_d, ou_x.x, ou_c * xi.x), __builtin_fma(ou_d, ou_x.y, ou_c * xi.y),
                              __builtin_fma(ou_d, ou_x.z, ou_c * xi.z)};
                    z0 = ou_x; z1 = ou_x; z2 = ou_x; z3 = ou_x;
                } else if (THERMAL) {
                    z0 = ns.draw(true); z1 = ns.draw(false); z2 = ns.draw(true); z3 = ns.draw(false);
                }
                const double t2 = add_x(ti, mul_x(dt, 0.5)), t4 = add_x(ti, dt);          // simple_solver.py:291-293
                const V3 f1 = stage(m, drive(ti), z0);
                const StageDrive d2 = drive(t2);                     // k2 and k3 share their stage time
                const V3 y2{__builtin_fma(half_dt, f1.x, m.x), __builtin_fma(half_dt, f1.y, m.y), __builtin_fma(half_dt, f1.z, m.z)};
                const V3 f2 = stage(y2, d2, z1);
                const V3 y3{__builtin_fma(half_dt, f2.x, m.x), __builtin_fma(half_dt, f2.y, m.y), __builtin_fma(half_dt, f2.z, m.z)};
                const V3 f3 = stage(y3, d2, z2);
                const V3 y4{__builtin_fma(dt, f3.x, m.x), __builtin_fma(dt, f3.y, m.y), __builtin_fma(dt, f3.z, m.z)};
                const V3 f4 = stage(y4, drive(t4), z3);
                // m + (k1 + 2 k2 + 2 k3 + k4)/6 with k = dt*f                  simple_solver.py:290-295
                mn = V3{__builtin_fma(sixth_dt, __builtin_fma(2.0, f2.x, f1.x) + __builtin_fma(2.0, f3.x, f4.x), m.x),
                        __builtin_fma(sixth_dt, __builtin_fma(2.0, f2.y, f1.y) + __builtin_fma(2.0, f3.y, f4.y), m.y),
                        __builtin_fma(sixth_dt, __builtin_fma(2.0, f2.z, f1.z) + __builtin_fma(2.0, f3.z, f4.z), m.z)};
            }
            resets += simple_validate(mn, zr);                                 // simple_solver.py:168
            fail |= zr;                                                        // robust_solver.py:192-205
            m = mn;
            if (RECORD) rec.put(i + 1, i == n - 1 ? T : mul_x((double)(i + 1), dt), m, 0.0);
        }
    };
    if (THERMAL && ou_sel) run(std::true_type{}); else run(std::false_type{});
    o.resets = resets;
    if (fail) return o;
    o.m = m;
    o.ok = true;
    return o;
}

// ---- RK45 -----------------------------------------------------------------------------------------------------------------------
// The drive of one RHS call of LLGSSolver.solve::llgs_rhs, ready for llgs_rhs: torques are off iff |current| < 1e-12
// (llgs_solver.py:222), h_applied starts h_eff (llgs_solver.py:189).  The applied field rides with the thermal field: llgs_rhs adds
// its `ht` argument (a field already times -gamma) to G, so the waveform kernels call its THERMAL form with ht = thermal + (-gamma h).
struct LlgsDrive {
    double bJ, bpJ;
    V3 h, gh;       // h_applied and -gamma h_applied
};
struct LlgsWaveK {
    double beta, betap, ngamma;
    double bJ_rect, bpJ_rect;     // the rectangular form's products, formed once as llgs_lane_begin forms them
    double mu0msv;                // mu_0 Ms V of the Zeeman energy (llgs_solver.py:250)
};
template <class WS>
__device__ __forceinline__ LlgsDrive llgs_drive(WS& src, const LlgsWaveK& wk, double t) {
#pragma clang fp contract(off)
    const WaveDrive d = src.at(t);
    LlgsDrive r;
    if (src.has_j) {
        const bool useJ = !(fabs(d.cur) < 1e-12);
        r.bJ = useJ ? wk.beta * d.cur : 0.0;
        r.bpJ = useJ ? wk.betap * d.cur : 0.0;
    } else {
        const bool on = t <= src.T;
        r.bJ = on ? wk.bJ_rect : 0.0;
        r.bpJ = on ? wk.bpJ_rect : 0.0;
    }
    r.h = d.h;
    r.gh = V3{wk.ngamma * d.h.x, wk.ngamma * d.h.y, wk.ngamma * d.h.z};
    return r;
}
template <bool THERMAL, bool CHECKED>
__device__ __forceinline__ V3 llgs_fun_wave(bool has_h, const LlgsDrive& d, const LlgsK& k, const V3& y, const V3& ht) {
    if (!THERMAL && !has_h) return llgs_rhs<false, false, CHECKED>(y, k, d.bJ, d.bpJ, ht);
    return llgs_rhs<true, false, CHECKED>(y, k, d.bJ, d.bpJ, V3{ht.x + d.gh.x, ht.y + d.gh.y, ht.z + d.gh.z});
}

// llgs_lane_emit with the by-products taken at the point's own time: energy includes the Zeeman term -mu0 Ms V m.h_applied
// (llgs_solver.py:250), torques use current(t) (llgs_solver.py:161,169-172).  `src` is the solve's own cursor pair, which stands at or
// before L.t.
template <bool RECORD, class WS, class REC = Recorder>
__device__ __forceinline__ void llgs_lane_emit_wave(LlgsLane& L, V3& out_m, const REC& rec, const LlgsEnergyK& ek, WS& src,
                                                    const LlgsWaveK& wk) {
    const double inv = rsqrt_fast(dot(L.y, L.y));
    out_m = V3{L.y.x * inv, L.y.y * inv, L.y.z * inv};
    if (RECORD) {
        if constexpr (REC::kByProducts) {
            const LlgsDrive d = llgs_drive(src, wk, L.t);
            const double e = rec.e ? -wk.mu0msv * dot(out_m, d.h) + llgs_energy(out_m, ek) : 0.0;
            rec.put(L.npts, L.t, out_m, e, rec.tq ? llgs_torque_norms(out_m, d.bJ, d.bpJ) : 0.0);
        } else {
            // (an observer that wants neither by-product: no drive lookup; the next attempt seeks the cursors to its start time itself)
            rec.put(L.npts, L.t, out_m, 0.0, 0.0);
        }
    }
    ++L.npts;
}

// llgs_lane_begin: f(t0, y0) sees the drive at t0 = 0, select_initial_step's second call the drive at t0 + h0 (common.py:117-118)
template <bool THERMAL, bool RECORD, class WS, class REC = Recorder>
__device__ __forceinline__ void llgs_lane_begin_wave(LlgsLane& L, V3& out_m, const V3& m0, double T, const LlgsK& k, double rtol, double atol,
                                                     double max_step, const RngKey& rk, const REC& rec, const LlgsEnergyK& ek,
                                                     InlineNormals& ns, WS& src, const LlgsWaveK& wk) {
    L.bJ = 0.0; L.bpJ = 0.0;               // (unused here: the drive is per call)
    L.m0 = m0;
    L.T = T;
    if (THERMAL) ns.begin(rk);
    const double n0 = rsqrt_fast(dot(m0, m0));                              // llgs_solver.py:76
    L.y = V3{m0.x * n0, m0.y * n0, m0.z * n0};
    L.t = 0.0;
    L.npts = 0;
    if (RECORD) llgs_lane_emit_wave<RECORD>(L, out_m, rec, ek, src, wk); else ++L.npts;
    L.f = llgs_fun_wave<THERMAL, true>(src.has_h, llgs_drive(src, wk, 0.0), k, L.y, llgs_draw<THERMAL>(ns, k, true));
    double h_abs;
    {   // select_initial_step (common.py:68-134), as llgs_lane_begin
        const V3& y = L.y;
        const V3& f = L.f;
        const V3 sc{atol + fabs(y.x) * rtol, atol + fabs(y.y) * rtol, atol + fabs(y.z) * rtol};
        const V3 isc{rcp_fast(sc.x), rcp_fast(sc.y), rcp_fast(sc.z)};
        const double d0 = rms3(V3{y.x * isc.x, y.y * isc.y, y.z * isc.z});
        const double d1 = rms3(V3{f.x * isc.x, f.y * isc.y, f.z * isc.z});
        double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : (0.01 * d0) * rcp_fast(d1);
        h0 = fmin(h0, T);
        const V3 y1{y.x + h0 * f.x, y.y + h0 * f.y, y.z + h0 * f.z};
        // (a scratch copy of the cursors: the solve's own stay at t0 for the first attempt)
        WS probe = src;
        const V3 f1 = llgs_fun_wave<THERMAL, true>(src.has_h, llgs_drive(probe, wk, h0), k, y1, llgs_draw<THERMAL>(ns, k, false));
        const double d2 = rms3(V3{(f1.x - f.x) * isc.x, (f1.y - f.y) * isc.y, (f1.z - f.z) * isc.z}) * rcp_fast(h0);
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : fifth_root(0.01 * rcp_fast(fmax(d1, d2)));
        h_abs = fmin(fmin(100.0 * h0, h1), fmin(T, max_step));
    }
    L.rejected = false;
    L.attempts = 0;
    const double min_step = min_step_at(L.t);
    L.h_abs = h_abs > max_step ? max_step : (h_abs < min_step ? min_step : h_abs);          // rk.py:121-126
    L.h_floor = isfinite(T) ? min_step_at(T) : __builtin_inf();
    L.active = L.t != T;
    L.idle = !L.active;
}

// llgs_lane_attempt (one env per lane, normals inline) with the drive of every RHS call taken at its stage time t + c h, c = 1/5, 3/10,
// 4/5, 8/9, 1 and -- f_new -- t + h (rk.py:64-68).  A rejected attempt retries from the same t with a smaller h, so the solve's cursors
// (`src`) only ever move to the attempt's START time; the stage times are looked up with a copy that scans forward from there and is
// dropped afterwards.
template <bool THERMAL, bool RECORD, class WS, class REC = Recorder>
__device__ __forceinline__ void llgs_lane_attempt_wave(LlgsLane& L, LlgsMasks& M, V3& out_m, const LlgsK& k, const Dp5Tab& tb, double rtol,
                                                       double atol, double max_step, const REC& rec, const LlgsEnergyK& ek,
                                                       InlineNormals& ns, WS& src, const LlgsWaveK& wk) {
    constexpr double A21 = 1.0 / 5;
    constexpr double A31 = 3.0 / 40, A32 = 9.0 / 40;
    constexpr double A41 = 44.0 / 45, A42 = -56.0 / 15, A43 = 32.0 / 9;
    constexpr double B1 = 35.0 / 384, B3 = 500.0 / 1113, B5 = -2187.0 / 6784, B6 = 11.0 / 84;
    constexpr double C2 = 1.0 / 5, C3 = 3.0 / 10, C4 = 4.0 / 5, C5 = 8.0 / 9;
    const double B4 = tb.B4;
    const double A51 = tb.A51, A52 = tb.A52, A53 = tb.A53, A54 = tb.A54, A61 = tb.A61, A62 = tb.A62, A63 = tb.A63, A64 = tb.A64, A65 = tb.A65;
    const double E1 = tb.E1, E3 = tb.E3, E4 = tb.E4, E5 = tb.E5, E6 = tb.E6, E7 = tb.E7;
    const double T = L.T;
    const bool active = lane_in(M.active);
    const V3 y = L.y;
    const double t = L.t;
    src.seek(t);
    WS stg_at = src;                    // this attempt's forward scan
    L.attempts += active ? 1 : 0;
    const double t_new = fmin(add_x(t, L.h_abs), T);                       // rk.py:135-138
    const double h = sub_x(t_new, t);
    const double h_try = fabs(h);
    // stage time fl(t + fl(c h)) (rk.py:64-68; c = 1: t + h), field drawn in call order (phases alternate per call)
    auto drive = [&](double c) -> LlgsDrive { return llgs_drive(stg_at, wk, add_x(t, mul_x(c, h))); };
    auto fun = [&](const LlgsDrive& d, const V3& yy, bool even) -> V3 {
        return llgs_fun_wave<THERMAL, false>(src.has_h, d, k, yy, llgs_draw<THERMAL>(ns, k, even));
    };
    const V3 k1 = L.f;
    const V3 k2 = fun(drive(C2), V3{y.x + (k1.x * A21) * h, y.y + (k1.y * A21) * h, y.z + (k1.z * A21) * h}, true);
    const V3 k3 = fun(drive(C3), V3{y.x + (k1.x * A31 + k2.x * A32) * h, y.y + (k1.y * A31 + k2.y * A32) * h,
                             y.z + (k1.z * A31 + k2.z * A32) * h}, false);
    const V3 k4 = fun(drive(C4), V3{y.x + (k1.x * A41 + k2.x * A42 + k3.x * A43) * h, y.y + (k1.y * A41 + k2.y * A42 + k3.y * A43) * h,
                             y.z + (k1.z * A41 + k2.z * A42 + k3.z * A43) * h}, true);
    const V3 k5 = fun(drive(C5), V3{y.x + (k1.x * A51 + k2.x * A52 + k3.x * A53 + k4.x * A54) * h,
                             y.y + (k1.y * A51 + k2.y * A52 + k3.y * A53 + k4.y * A54) * h,
                             y.z + (k1.z * A51 + k2.z * A52 + k3.z * A53 + k4.z * A54) * h}, false);
    const LlgsDrive d_end = drive(1.0);              // k6 and f_new share the stage time t + h
    const V3 k6 = fun(d_end, V3{y.x + (k1.x * A61 + k2.x * A62 + k3.x * A63 + k4.x * A64 + k5.x * A65) * h,
                              y.y + (k1.y * A61 + k2.y * A62 + k3.y * A63 + k4.y * A64 + k5.y * A65) * h,
                              y.z + (k1.z * A61 + k2.z * A62 + k3.z * A63 + k4.z * A64 + k5.z * A65) * h}, true);
    const V3 y_new{y.x + h * (k1.x * B1 + k3.x * B3 + k4.x * B4 + k5.x * B5 + k6.x * B6),
                   y.y + h * (k1.y * B1 + k3.y * B3 + k4.y * B4 + k5.y * B5 + k6.y * B6),
                   y.z + h * (k1.z * B1 + k3.z * B3 + k4.z * B4 + k5.z * B5 + k6.z * B6)};
    const V3 f_new = fun(d_end, y_new, false);
    const V3 ev{(k1.x * E1 + k3.x * E3 + k4.x * E4 + k5.x * E5 + k6.x * E6 + f_new.x * E7) * h,
                (k1.y * E1 + k3.y * E3 + k4.y * E4 + k5.y * E5 + k6.y * E6 + f_new.y * E7) * h,
                (k1.z * E1 + k3.z * E3 + k4.z * E4 + k5.z * E5 + k6.z * E6 + f_new.z * E7) * h};
    const V3 sc{atol + fmax_abs(y.x, y_new.x) * rtol, atol + fmax_abs(y.y, y_new.y) * rtol, atol + fmax_abs(y.z, y_new.z) * rtol};
    const V3 q{ev.x * rcp_fast(sc.x), ev.y * rcp_fast(sc.y), ev.z * rcp_fast(sc.z)};
    const double err = dot(q, q) * tb.third;          // the squared error norm, as in llgs_lane_attempt
    const lanemask accm = M.active & __ballot(err < 1.0);
    const bool acc = lane_in(accm);
    const double r9 = tb.c09 * inv_tenth_root(err, tb.tenth);
    const double fa = fmin(lane_in(M.pacc) ? 10.0 : 1.0, r9);
    const double fr = fmax(0.2, r9);
    const double h_next = fmin(h_try * (acc ? fa : fr), max_step);
    M.low = __ballot(h_next < L.h_floor);
    L.h_abs = h_next;
    commit_step(accm, L.t, t_new, L.y.x, y_new.x, L.y.y, y_new.y, L.y.z, y_new.z, L.f.x, f_new.x, L.f.y, f_new.y, L.f.z, f_new.z);
    if (RECORD) { if (acc) llgs_lane_emit_wave<RECORD>(L, out_m, rec, ek, src, wk); } else L.npts += acc ? 1 : 0;
    M.pacc = accm;
}

// llgs_solve with waveforms: begin / gate / attempt / finish as there, one env per lane from start to end
template <bool THERMAL, bool RECORD, class WS, class REC = Recorder>
__device__ __forceinline__ SolveOut llgs_solve_wave(const V3& m0, double T, const LlgsK& k, double rtol, double atol, double max_step,
                                                    int64_t max_attempts, const RngKey& rk, const REC& rec, const LlgsEnergyK& ek,
                                                    InlineNormals& ns, WS& src, const LlgsWaveK& wk) {
    const Dp5Tab tb = make_dp5_tab();
    LlgsLane L;
    V3 out_m = m0;
    llgs_lane_begin_wave<THERMAL, RECORD>(L, out_m, m0, T, k, rtol, atol, max_step, rk, rec, ek, ns, src, wk);
    LlgsMasks M = llgs_masks_open(L);
    int32_t budget = (int32_t)max_attempts;
    int32_t it = 0;
    if (M.active != 0ull)
    for (;;) {
        llgs_lane_gate<true>(L, M, budget);
        llgs_lane_attempt_wave<THERMAL, RECORD>(L, M, out_m, k, tb, rtol, atol, max_step, rec, ek, ns, src, wk);
        if (!attempt_loop_next(M.active, __ballot(L.t != L.T), it, budget)) break;
    }
    llgs_masks_close(L, M);
    return llgs_lane_finish<RECORD>(L, out_m, rec, ek, ns);
}

}  // namespace stg
