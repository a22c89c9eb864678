// tv16_const.h -- thresholdv16 constants that both the workspace layout (ws.h)
// and the finishes' shared rules (tv16_finish.h) need.  Plain C++.
#pragma once

#include <stdint.h>

namespace stg {

constexpr uint32_t CAND_CAP = 8192;          // regime-B window entries per bucket (+1 for the ragged tail)
constexpr uint32_t TV16_WIN = 1u << 18;      // regime-B window below t, in ulps of t (~3.1 %)
constexpr uint32_t TV16_DEC_B = 1, TV16_DEC_WIN = 2, TV16_DEC_TAIL = 4;  // Decision flags
constexpr uint32_t TV16_TAG_DEC = 3;

}  // namespace stg
