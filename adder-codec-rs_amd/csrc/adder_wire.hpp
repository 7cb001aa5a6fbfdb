// adder_wire.hpp -- the one decoder of what the event tools read: AdderEvents and the 9 / 11-byte big-endian wire
// records of a .adder body (adder-codec-core raw/stream.rs:101-120, 177-201), and the three small functions every
// per-unit tool needs next to it.  adder_dvs.hip, adder_player.hip and adder_viz_player.hip decode through wire_load;
// adder_stream.hip too, except that its stream_load spells the 11-byte arm with wire11_t_offset (measured: see there).
// Their *_api.cpp pick the source with wire_source.  Compiled for the device and, by tests/cpu_sim/wire_sim.cpp, for
// the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/adder_hip.h"  // AdderEvent

#ifndef ADDER_HD  // as adder_pixel.hpp
#if defined(__HIPCC__)
#define ADDER_HD __host__ __device__ __forceinline__
#else
#define ADDER_HD inline
#endif
#endif

namespace adder {

enum EventSource : int { kSrcEvents = 0, kSrcWire9 = 1, kSrcWire11 = 2 };

struct WireEv {
    uint32_t x, y, c, d, t;
    bool end;  // EOF record or undecodable (raw/stream.rs:177-201: either ends the reading loop)
};

ADDER_HD uint32_t wire_be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
ADDER_HD uint32_t wire_be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// where the big-endian t sits in an 11-byte record: behind Some(c) (tag 1) or behind None (tag 0)
ADDER_HD uint32_t wire11_t_offset(uint32_t tag) { return tag == 1u ? 7u : 6u; }

// The wire records are read byte by byte: nothing is asked of the buffer's alignment.
template <int SRC>
ADDER_HD WireEv wire_load(const void *in, uint64_t i) {
    WireEv e;
    e.end = false;
    if (SRC == kSrcEvents) {
        const AdderEvent ev = ((const AdderEvent *)in)[i];
        e.x = ev.x;
        e.y = ev.y;
        e.c = ev.c == 0xffu ? 0u : ev.c;  // `c = None` counts as channel 0
        e.d = ev.d;
        e.t = ev.t;
    } else if (SRC == kSrcWire9) {
        const uint8_t *p = (const uint8_t *)in + i * 9u;
        e.x = wire_be16(p);
        e.y = wire_be16(p + 2);
        e.c = 0u;
        e.d = p[4];
        e.t = wire_be32(p + 5);
        e.end = e.x == 0xffffu && e.y == 0xffffu;
    } else {  // 11 bytes: x, y, Option<u8> c (bincode: tag byte, then the value when Some), d, t
        const uint8_t *p = (const uint8_t *)in + i * 11u;
        e.x = wire_be16(p);
        e.y = wire_be16(p + 2);
        const uint32_t tag = p[4];
        if (tag == 1u) {
            e.c = p[5];
            e.d = p[6];
            e.t = wire_be32(p + 7);
        } else {
            e.c = 0u;
            e.d = p[5];
            e.t = wire_be32(p + 6);
        }
        e.end = tag > 1u || (e.x == 0xffffu && e.y == 0xffffu);
    }
    return e;
}

ADDER_HD size_t wire_record_bytes(int src) { return src == kSrcEvents ? sizeof(AdderEvent) : src == kSrcWire9 ? 9u : 11u; }

// the wire form of a stream with this many channels (raw/stream.rs:101-120)
ADDER_HD int wire_source(uint32_t channels) { return channels == 1u ? kSrcWire9 : kSrcWire11; }

// t rounded up to a multiple of ref (ref >= 1)
ADDER_HD uint64_t wire_round_up(uint64_t t, uint64_t ref) { return t % ref == 0u ? t : (t / ref + 1u) * ref; }

// the first index a call does not apply: its first bad event or its EOF record, whichever comes first
ADDER_HD uint64_t wire_limit(unsigned long long bad, unsigned long long eof) { return bad < eof ? bad : eof; }

}  // namespace adder
