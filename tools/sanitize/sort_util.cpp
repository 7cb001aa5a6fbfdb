// Stand-alone walk of the event tools' pure rules (csrc/adder_sort_util.hpp) for a build with
// -fsanitize=address,undefined (see the end for the command).  It has its own main and loads nothing else.
//
// key_bits_for shifts by its own result and scratch_capacity adds to its argument, so the walk goes to the ends of
// their ranges: every power of two and its neighbours up to 2^32, and n up to 2^64 - 1 less an eighth.  Each value is
// checked against the rule written the long way; the Crf table is read through to its last row.  Exit status 1 on a
// mismatch; anything else that is wrong is the sanitizer's.
#include <stdint.h>
#include <stdio.h>

#include "adder_sort_util.hpp"

using namespace adder;

int main() {
    int bad = 0;
    for (uint32_t k = 0; k <= 32; ++k)
        for (int d = -1; d <= 1; ++d) {
            const uint64_t units = (1ull << k) + (uint64_t)d;
            if (units == 0 || units > 0xfffffffeull) continue;  // a plane has a pixel; a key is 32 bits
            uint32_t want = 1;
            while (want < 64 && (units >> want) != 0) ++want;  // max(1, bit length)
            if (key_bits_for(units) != want) {
                printf("key_bits_for(%llu) = %u, not %u\n", (unsigned long long)units, key_bits_for(units), want);
                bad = 1;
            }
        }
    for (uint32_t k = 0; k < 64; ++k)
        for (int d = -1; d <= 1; ++d) {
            const uint64_t n = (1ull << k) + (uint64_t)d;
            if (n > 0xffffffffffffffffull / 9u * 8u) continue;  // n + n / 8 would wrap; a call takes 2^31 - 1 at most
            const uint64_t c = scratch_capacity(n);
            if (c != (n + n / 8u < 0x7fffffffull ? n + n / 8u : 0x7fffffffull)) {
                printf("scratch_capacity(%llu) = %llu\n", (unsigned long long)n, (unsigned long long)c);
                bad = 1;
            }
        }
    unsigned sum = 0;
    for (int q = 0; q < 10; ++q) sum += kCrf[q][kCrfBaseline] + kCrf[q][kCrfMax] + kCrf[q][kCrfVelocity];
    if (sum != 54u + 104u + 55u) {
        printf("Crf table sums to %u\n", sum);
        bad = 1;
    }
    printf(bad ? "FAILED\n" : "clean\n");
    return bad;
}

// from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I adder-codec-rs_amd/csrc tools/sanitize/sort_util.cpp -o /tmp/sort_util && /tmp/sort_util
