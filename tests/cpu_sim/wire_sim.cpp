// wire_sim.cpp -- csrc/adder_wire.hpp compiled by g++ for tests/test_wire_decode_cpu.py: the decoder the event tools'
// kernels run, called record by record over a host buffer.
#include "adder_wire.hpp"

using namespace adder;

namespace {

// out: n rows of x, y, c, d, t, end
template <int SRC>
void load_all(const void *in, uint64_t n, uint32_t *out) {
    for (uint64_t i = 0; i < n; ++i) {
        const WireEv e = wire_load<SRC>(in, i);
        uint32_t *r = out + i * 6u;
        r[0] = e.x;
        r[1] = e.y;
        r[2] = e.c;
        r[3] = e.d;
        r[4] = e.t;
        r[5] = e.end ? 1u : 0u;
    }
}

}  // namespace

extern "C" {

// 0: the source is none of the three
int ws_load(int source, const void *in, uint64_t n, uint32_t *out) {
    if (source == kSrcEvents)
        load_all<kSrcEvents>(in, n, out);
    else if (source == kSrcWire9)
        load_all<kSrcWire9>(in, n, out);
    else if (source == kSrcWire11)
        load_all<kSrcWire11>(in, n, out);
    else
        return 0;
    return 1;
}

uint64_t ws_record_bytes(int source) { return wire_record_bytes(source); }
int ws_source(uint32_t channels) { return wire_source(channels); }
uint32_t ws_t_offset(uint32_t tag) { return wire11_t_offset(tag); }
uint64_t ws_round_up(uint64_t t, uint64_t ref) { return wire_round_up(t, ref); }
uint64_t ws_limit(uint64_t bad, uint64_t eof) { return wire_limit(bad, eof); }

}  // extern "C"
