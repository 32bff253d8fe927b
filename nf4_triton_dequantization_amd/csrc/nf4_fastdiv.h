// nf4_fastdiv.h -- division by a run-time constant, host side: the divisor's magic
// numbers (plain C++; the device side, fdiv / fmodu, is in nf4_common.h).
#pragma once

#include <stdint.h>

namespace nf4dq {

// Division by a run-time constant for n < 2^31: q = (umulhi(n, mul) + n) >> shift.
struct FastDiv {
    uint32_t d, mul, shift;
};

inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{d, 0u, 0u};
    uint32_t s = 0;
    while (s < 32 && (uint64_t(1) << s) < d) ++s;
    f.shift = s;
    f.mul = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << s) - d)) / d + 1);
    return f;
}

}  // namespace nf4dq
