// adder_sort_util.hpp -- the pure rules the event tools' *_api.cpp share: the radix bits of a unit key, the scratch a
// call's records take, the Crf table.  No HIP: plain g++ compiles it (tests/cpu_sim/sort_util.cpp).
#pragma once
#include <stdint.h>

namespace adder {

// radix bits for keys 0..units (key `units` marks a record that takes part in nothing): the smallest b >= 1 with
// 2^b >= units + 1.  (Starting the search at b = 0, as the framer's feature pass once did, gives the same value: a
// plane has units >= 1, so units + 1 >= 2 never fits in 0 bits.)
inline uint32_t key_bits_for(uint64_t units) {
    uint32_t b = 1;
    while ((1ull << b) < units + 1u) ++b;
    return b;
}

// a call of n records reserves scratch for an eighth more, so that slowly growing calls do not reallocate each time;
// hipcub counts in int
inline uint64_t scratch_capacity(uint64_t n) {
    const uint64_t c = n + n / 8u;
    return c > (uint64_t)INT32_MAX ? (uint64_t)INT32_MAX : c;
}

// Crf rows 0..9 (rate_controller.rs)
enum { kCrfBaseline = 0, kCrfMax = 1, kCrfVelocity = 2 };
constexpr uint8_t kCrf[10][3] = {{0, 0, 10}, {0, 1, 9}, {1, 3, 8}, {2, 7, 7},  {5, 9, 6},
                                 {6, 10, 5}, {7, 13, 4}, {8, 16, 3}, {10, 20, 2}, {15, 25, 1}};

}  // namespace adder
