// dvs_video_main.cpp -- adder_dvs_video_logic.hpp under plain g++, with its own main: the program for host sanitizer
// builds (g++ -fsanitize=address,undefined tests/cpu_sim/dvs_video_main.cpp) and the check that the header needs no HIP.
//
// stdin: one call per line, "n L B draw F cur E pt[0..n) fire_t[0..n)".  stdout, per line: "F cur E k emitted[0..k)",
// the state after the call and the frames it emitted.  Every line is also run cut in two at every position (the
// pieces must give the same frames and state), finished, and pushed through the scalar helpers; a disagreement
// returns 1.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../adder-codec-rs_amd/csrc/adder_dvs_video_logic.hpp"

using namespace adder;

int main() {
    std::string line;
    int bad = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        uint64_t n = 0, L = 0, B = 0, draw = 0;
        DvsVideoState st0{};
        if (!(in >> n >> L >> B >> draw >> st0.F >> st0.cur >> st0.E) || L == 0) return 2;
        std::vector<uint64_t> pt(n), fire(n);
        for (auto &v : pt) in >> v;
        for (auto &v : fire) in >> v;
        if (!in) return 2;

        DvsVideoState st = st0;
        std::vector<uint64_t> em(n);
        std::vector<uint8_t> pop(n), acc(n);
        const uint64_t k = dvs_video_schedule(pt.data(), fire.data(), n, L, B, draw != 0, &st, pop.data(), acc.data(),
                                              em.data(), n);
        std::printf("%llu %llu %llu %llu", (unsigned long long)st.F, (unsigned long long)st.cur,
                    (unsigned long long)st.E, (unsigned long long)k);
        for (uint64_t i = 0; i < k; ++i) std::printf(" %llu", (unsigned long long)em[i]);
        std::printf("\n");

        for (uint64_t cut = 0; cut <= n; ++cut) {  // two calls give what one gives
            DvsVideoState s2 = st0;
            std::vector<uint64_t> e2(n);
            const uint64_t a = dvs_video_schedule(pt.data(), fire.data(), cut, L, B, draw != 0, &s2, nullptr, nullptr,
                                                  e2.data(), n);
            const uint64_t b = dvs_video_schedule(pt.data() + cut, fire.data() + cut, n - cut, L, B, draw != 0, &s2,
                                                  nullptr, nullptr, e2.data() + a, n - a);
            bool same = a + b == k && s2.F == st.F && s2.cur == st.cur && s2.E == st.E;
            for (uint64_t i = 0; same && i < k; ++i) same = e2[i] == em[i];
            if (!same) {
                std::fprintf(stderr, "cut %llu of \"%s\" differs\n", (unsigned long long)cut, line.c_str());
                bad = 1;
            }
        }

        DvsVideoState fin = st;
        uint64_t first = 0;
        const uint64_t tail = dvs_video_finish(L, B, &fin, &first);
        if (tail == 0 || first + tail < fin.F || (k && first <= em[k - 1])) {
            std::fprintf(stderr, "finish of \"%s\": %llu frames from %llu\n", line.c_str(), (unsigned long long)tail,
                         (unsigned long long)first);
            bad = 1;
        }
        // the scalar helpers on the line's own numbers
        if (n <= 65535u && dvs_video_count_byte((uint32_t)n, dvs_video_count_peak((uint32_t)n)) != (n ? 255 : 0)) bad = 1;
        if (L < (1ull << 32) && dvs_video_frame_length((uint32_t)L, 1.0f) == 0) bad = 1;
        if (dvs_video_buffer_ticks((uint32_t)B, -1.0f) != 0) bad = 1;
    }
    return bad;
}
