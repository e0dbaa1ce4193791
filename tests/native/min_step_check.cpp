// Host proof that the exponent form of the RK45 minimum step equals its definition bit for bit (csrc/stg_minstep.hpp).
// Prints the number of values compared; exits non-zero at the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "stg_minstep.hpp"

static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static double from_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

static long n_checked = 0;
static bool check(double t, bool positive_form) {
    const double ref = stg::min_step_ref(t);
    const double at = stg::min_step_at(t);
    const double pos = positive_form ? stg::min_step_pos(t) : ref;
    ++n_checked;
    if (bits(ref) == bits(at) && bits(ref) == bits(pos)) return true;
    std::printf("MISMATCH t=%a ref=%a at=%a pos=%a\n", t, ref, at, pos);
    return false;
}

int main() {
    bool ok = check(0.0, false);
    // every power of two from the smallest subnormal to 2^1022, with its neighbours on both sides
    for (int e = -1074; e <= 1022; ++e) {
        const double p = std::ldexp(1.0, e);
        ok = ok && check(p, true) && check(from_bits(bits(p) + 1), true);
        if (bits(p) > 1) ok = ok && check(from_bits(bits(p) - 1), true);
    }
    // subnormals: the first 4096, and the last ones below the smallest normal number
    for (uint64_t b = 1; b <= 4096; ++b) ok = ok && check(from_bits(b), true);
    for (uint64_t b = 0; b < 4096; ++b) ok = ok && check(from_bits(0x0010000000000000ull - 1 - b), true);
    // random bit patterns over all finite non-negative doubles up to 2^1022 (xorshift64*), and pulse-scale times
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 2000000 && ok; ++i) {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        const uint64_t r = s * 0x2545F4914F6CDD1Dull;
        const double t = from_bits(r % 0x7FD0000000000000ull);
        if (t > 0.0) ok = check(t, true);
        const double u = 1e-12 + (double)(r >> 11) * (1.0 / 9007199254740992.0) * 5e-9;      // [1e-12, 5e-9): where a solve's t lives
        ok = ok && check(u, true);
    }
    std::printf("checked %ld\n", n_checked);
    return ok ? 0 : 1;
}
