// stg_vary.hpp -- device-to-device variation of stg_switch_population: which device a trial belongs to, which stream draws it, and
// how five normals turn a condition's nominal parameters into that device's.  The rule is stated once, here, for the trial kernel
// (stg_switch.hpp), the diagnostic dump (stg_switch_population_devices) and a CPU driver alike: the header has no HIP dependency and
// compiles with the host compiler (tests/test_switch_population_host.py), as stg_launch_plan.hpp and stg_minstep.hpp do.
//
// The rule (include/spintorque_hip.h states it for callers):
//   trial r (absolute index) of condition g belongs to device d = r / Q, Q = trials_per_device >= 1;
//   the device's normals z_0 ... z_5 are calls 0 and 1 of the thermal stream of env id env_id0 + g * trial_stride + d * Q -- the id of
//   the device's first trial -- at Philox counter word var_step, tag 0 (what stg_thermal_normals dumps for that id); z_5 is not used;
//   field k of (damping, ms, ku, volume, polarization), the first STG_NVARY doubles of stg_device_params, becomes
//       nominal_k * (1.0 + sigma[k][g] * min(max(z_k, -z_clip), z_clip))
//   in IEEE fp64, each operation rounded; every other field, dev_type and params_valid are the nominal record's.
//   A condition's sigma column is valid when every entry is >= 0 (a NaN is not) and sigma[k][g] * z_clip < 1.0 (an infinite sigma
//   fails here): a clipped normal then cannot drive a parameter to zero or below.
#pragma once

#include <stdint.h>

#include "../../include/spintorque_hip.h"
#include "stg_minstep.hpp"          // STG_HD

namespace stg {

// the device of absolute trial r, and the env id whose stream draws device d of condition g
STG_HD inline int64_t vary_device_of(int64_t r, int64_t Q) { return r / Q; }
STG_HD inline int64_t vary_device_env(int64_t env_id0, int64_t g, int64_t trial_stride, int64_t d, int64_t Q) {
    return env_id0 + g * trial_stride + d * Q;
}
// the devices a call on trials trial0 ... trial0 + R - 1 (R >= 1) touches: first and last, both inclusive
STG_HD inline int64_t vary_first_device(int64_t trial0, int64_t Q) { return trial0 / Q; }
STG_HD inline int64_t vary_last_device(int64_t trial0, int64_t R, int64_t Q) { return (trial0 + R - 1) / Q; }

// one entry of a sigma column
STG_HD inline bool vary_sigma_ok(double sigma, double z_clip) {
    return sigma >= 0.0 && sigma * z_clip < 1.0;
}
// condition g's column of sigma double[STG_NVARY][G]
STG_HD inline bool vary_column_ok(const double* sigma, int64_t G, int64_t g, double z_clip) {
    bool ok = true;
    for (int k = 0; k < STG_NVARY; ++k) ok = ok && vary_sigma_ok(sigma[(int64_t)k * G + g], z_clip);
    return ok;
}

// one field: three rounded operations, never contracted (sigma == 0 hands back the nominal bits: 1.0 + 0.0 * zc == 1.0 for finite zc)
STG_HD inline double vary_value(double nominal, double sigma, double z, double z_clip) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double lo = z < -z_clip ? -z_clip : z;            // max(z, -z_clip); a -0.0 passes through as it is
    const double zc = lo > z_clip ? z_clip : lo;            // min(., z_clip)
    const double prod = sigma * zc;
    const double f = 1.0 + prod;
    return nominal * f;
}

// the device's record from the nominal one, condition g's sigma column and the device's normals z[0 ... STG_NVARY - 1]
template <class P>
STG_HD inline void vary_params(const P& nominal, const double* sigma, int64_t G, int64_t g, const double* z, double z_clip, P& out) {
    out = nominal;
    out.damping = vary_value(nominal.damping, sigma[0 * G + g], z[0], z_clip);
    out.ms = vary_value(nominal.ms, sigma[1 * G + g], z[1], z_clip);
    out.ku = vary_value(nominal.ku, sigma[2 * G + g], z[2], z_clip);
    out.volume = vary_value(nominal.volume, sigma[3 * G + g], z[3], z_clip);
    out.polarization = vary_value(nominal.polarization, sigma[4 * G + g], z[4], z_clip);
}

}  // namespace stg
