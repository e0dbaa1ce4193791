// stg_minstep.hpp -- the RK45 controller's minimum step, 10 * ulp(t) (scipy/integrate/_ivp/rk.py:119), in two forms that are proven
// equal on the host (tests/test_min_step_host.py compiles this header with the host compiler; it has no HIP dependency).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STG_HD __host__ __device__
#else
#define STG_HD
#endif

namespace stg {

// the definition: 10 * (nextafter(t, inf) - t) for finite t >= 0, through the bit pattern (a 64-bit integer add, a subtraction, a product)
STG_HD inline double min_step_ref(double tt) {
    int64_t b;
    __builtin_memcpy(&b, &tt, 8);
    b += 1;
    double up;
    __builtin_memcpy(&up, &b, 8);
    return 10.0 * (up - tt);
}

// The same value from the exponent alone.  For t = f 2^e with f in [0.5, 1) (frexp), ulp(t) = 2^(e - 53), and every t below the
// smallest normal number (e <= -1022, zero included) has the subnormal spacing 2^-1074 = 2^(-1021 - 53).  10 * 2^(e - 53) has three
// significant bits, so it is exact wherever it is representable, which it is from 10 * 2^-1074 upwards: both forms round nothing.
constexpr int MIN_STEP_EXP_FLOOR = -1021;
constexpr double MIN_STEP_UNIT = 0x1.4p-50;          // 10 * 2^-53
// finite t > 0 (the device form is v_frexp_exp_i32_f64, v_max_i32, v_ldexp_f64; frexp's exponent of 0 is 0, hence the precondition)
STG_HD inline double min_step_pos(double tt) {
    int e;
    (void)__builtin_frexp(tt, &e);
    e = e < MIN_STEP_EXP_FLOOR ? MIN_STEP_EXP_FLOOR : e;
    return __builtin_ldexp(MIN_STEP_UNIT, e);
}
// finite t >= 0
STG_HD inline double min_step_at(double tt) {
    return tt == 0.0 ? __builtin_ldexp(MIN_STEP_UNIT, MIN_STEP_EXP_FLOOR) : min_step_pos(tt);
}

}  // namespace stg
