// scan_grid.h -- workgroups of one batched thresholdv16 scan launch (plain
// host C++: capi.cpp's launch_tv16_group, and the host test through
// stg_debug_tv16_scan_grid).
#pragma once

#include <stdint.h>

#include <algorithm>

namespace stg {

constexpr uint32_t TV16_MAXG = 512;  // scan workgroups per launch at most (two per CU of 256)

// Oversubscription of a launch's share of the chip, in halves (F = 2.5).  With
// S streams launching scans, each launch gets 2 * num_cu * F / S workgroups:
// F = 1 is the even split, which leaves a stream's slots idle while that
// stream is in its fill; F = S is the whole chip per launch, whose surplus
// workgroups start only after the launch's chunk counter has run out, take
// nothing and leave (they held a slot another launch's streaming workgroup
// was waiting for).  Measured at S = 4 (profiles/scan_grid_sweep.txt): F = 1.5
// and 2.5 are the headline's best, F = 2 (one workgroup per CU and launch) is
// worse than the whole chip, and the C4 stream wants the larger grids.
constexpr uint32_t TV16_GRID_F2 = 5;

// Workgroups of a scan launch of K chunks on a device of num_cu CUs, when
// `streams` distinct streams launched the device's recent batched scans and
// the process has `hw_queues` hardware queues (launches on more streams than
// queues do not overlap more than the queues do).  A multiple of 8 (the
// workgroups are dealt round-robin over 8 XCDs), at least 8, no more than two
// per CU, and no more than the chunks rounded up to 8.  One stream: two per CU.
inline uint32_t tv16_scan_grid(uint32_t num_cu, uint32_t streams, uint32_t hw_queues, uint32_t K,
                               uint32_t f2 = TV16_GRID_F2) {
    const uint32_t S = std::max(1u, std::min(streams, std::max(1u, hw_queues)));
    const uint64_t chip = 2ull * std::max(1u, num_cu);
    const uint64_t cap = std::max<uint64_t>(8, std::min<uint64_t>(chip, TV16_MAXG) / 8 * 8);
    const uint64_t share = (chip * f2 + 2ull * S - 1) / (2ull * S);  // ceil(2 num_cu F / S)
    const uint64_t want = (share + 7) / 8 * 8;
    const uint64_t byk = ((uint64_t)std::max(1u, K) + 7) / 8 * 8;
    return (uint32_t)std::max<uint64_t>(8, std::min({want, cap, byk}));
}

}  // namespace stg
