// stg_step_knots.hip -- the pulse-step kernel (stg_step_pulse.hpp) for stg_step_knots and stg_step_knots_ids: the action carries the
// amplitudes, [J, T, s_0 ... s_{kj-1}] per env and step, over the context's knot times (stg_set_pulse_knots).  The lane parses them into
// its own column of a [kj][64] block in dynamic LDS at the top of each step (LaneKnots, stg_wave.hpp).  Staged rather than re-read from
// the action: valid(), pulse_sq_integral and the cursor each walk the amplitudes, the cursor at knot crossings that differ from lane to
// lane inside the sub-step loop -- an LDS read there costs what the shaped policy's does, a global load would stall the whole wavefront
// per crossing and keep a 64-bit action address alive across the solve.  There is always a current table, and the
// kernel knows it at compile time: worth 14-16 % over the run-time flag (profiles/NOTEBOOK.md, round 15).
// A translation unit of its own: no other kernel is compiled with it.
#include "stg_step_pulse.hpp"

struct KnotsPulse {
    using Args = KnotsStepArgs;
    // the knots as the context keeps them on the device and the kernel stages them into LDS: tau, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
    static constexpr int DOUBLES = STG_KNOTS_DOUBLES, TAU = 0, TH = STG_MAX_KNOTS, HK = 2 * STG_MAX_KNOTS;
    static_assert(HK + 3 * STG_MAX_KNOTS == DOUBLES, "layout of the device copy of the pulse knots");
    static constexpr bool LANE_AMPS = true;
    using J = Pwl<1, LaneKnots>;                      // (tau_j * T, J * s_j), s_j from this step's action
    __device__ __forceinline__ static const double* values(const double*, const double* amp) { return amp; }
};

void stg_step_pulse_launch(const KnotsStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st) {
    stg_step_pulse_launch<KnotsPulse>(a, solver, thermal, multi, act_f64, st);
}
