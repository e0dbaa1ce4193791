// stg_step_shaped.hip -- the pulse-step kernel (stg_step_pulse.hpp) for stg_step_shaped and stg_step_shaped_ids: the amplitudes are the
// context's pulse shape (stg_set_pulse_shape), the `scale` row of the staged table, the same for every env and every step.  The shape
// may hold no current table at all (kj = 0: the field table alone over the rectangular pulse), so has_j is a run-time flag here.
// A translation unit of its own: no other kernel is compiled with it.
#include "stg_step_pulse.hpp"

struct ShapedPulse {
    using Args = ShapedStepArgs;
    // the shape as the context keeps it on the device and the kernel stages it into LDS: tau, scale, th [STG_MAX_KNOTS] each, hk [STG_MAX_KNOTS][3]
    static constexpr int DOUBLES = STG_SHAPE_DOUBLES, TAU = 0, SCALE = STG_MAX_KNOTS, TH = 2 * STG_MAX_KNOTS, HK = 3 * STG_MAX_KNOTS;
    static_assert(HK + 3 * STG_MAX_KNOTS == DOUBLES, "layout of the device copy of the pulse shape");
    static constexpr bool LANE_AMPS = false;
    using J = Pwl<1, SharedKnots<1, true>>;           // (tau_j * T, J * s_j)
    __device__ __forceinline__ static const double* values(const double* tab, const double*) { return tab + SCALE; }
};

void stg_step_pulse_launch(const ShapedStepArgs& a, int solver, bool thermal, bool multi, int act_f64, hipStream_t st) {
    stg_step_pulse_launch<ShapedPulse>(a, solver, thermal, multi, act_f64, st);
}
