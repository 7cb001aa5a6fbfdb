// adder_api_util.hpp -- what every tool's *_api.cpp does around its own work: the error string, the device check, the
// buffers that grow with the calls, the host forms' upload, and the 25-byte header of a raw .adder stream.
// Header-only free functions: a context stays the plain struct its file declares.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>

#include "../../include/adder_hip.h"  // ADDER_OK, ADDER_E_*
#include "adder_sort_util.hpp"        // the rules without HIP: key_bits_for, scratch_capacity, kCrf

namespace adder {

// the body of a file's `Xfail(ctx, code, fmt, ...)`, which picks ctx->err or its thread-local create-error string
inline int api_fail(std::string &dst, int code, const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    dst = buf;
    return code;
}

// Returns fail_fn(ctx, ADDER_E_HIP, ...) from the enclosing function when the HIP call `expr` fails.  The message names
// the call as it is written, so a file's shorthand passes the text along: the preprocessor would hand this macro the
// call with its constants already expanded.
//     #define XHIPCHK(v, expr) ADDER_HIPCHK(xfail, v, expr, #expr)
#define ADDER_HIPCHK(fail_fn, ctx, expr, text)                                                                       \
    do {                                                                                                             \
        hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess)                                                                                        \
            return fail_fn(ctx, ADDER_E_HIP, "%s failed: %s (%s:%d)", text, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// a visible gfx950 device of that index, or the code and the message a create call fails with
inline int api_check_device(int device_id, std::string &msg) {
    char buf[128];
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        msg = "no HIP device visible (this library has no CPU fallback)";
        return ADDER_E_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) {
        snprintf(buf, sizeof buf, "device_id %d of %d", device_id, ndev);
        msg = buf;
        return ADDER_E_BAD_PARAMS;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(buf, sizeof buf, "device %d is not gfx950; this library is built for gfx950 only", device_id);
        msg = buf;
        return ADDER_E_NO_DEVICE;
    }
    return ADDER_OK;
}

// *buf holds at least `bytes`; its contents are not kept when it has to be replaced
inline hipError_t api_grow(void **buf, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return hipSuccess;
    hipError_t e = *buf ? hipFree(*buf) : hipSuccess;
    if (e != hipSuccess) return e;
    *buf = nullptr;
    *cap = 0;
    e = hipMalloc(buf, bytes);
    if (e == hipSuccess) *cap = bytes;
    return e;
}

inline void api_free_all(std::initializer_list<void *> bufs) {
    for (void *b : bufs)
        if (b) (void)hipFree(b);
}

// a host form's input on the device; one byte more than asked, so that a call of no records has a non-null buffer
inline hipError_t api_stage_input(void **d_in, size_t *cap, const void *src, size_t bytes, hipStream_t stream) {
    const hipError_t e = api_grow(d_in, cap, bytes + 1u);
    if (e != hipSuccess || bytes == 0u) return e;
    return hipMemcpyAsync(*d_in, src, bytes, hipMemcpyHostToDevice, stream);
}

// The header of a raw .adder stream (header.rs:14-25 + encoder.rs:170-229): "adder", version, endianness 'b', u16 w, h,
// u32 tps, ref, delta_t_max, u8 event size, channels; then u32 source camera (v >= 1), time mode (v >= 2), adu
// interval (v >= 3), all big-endian.  A field its version does not have is 0.
struct RawHeader {
    uint32_t version, width, height, tps, ref_interval, delta_t_max, event_size, channels;
    uint32_t source_camera, time_mode, adu_interval;
    uint32_t header_bytes;  // 25 + 4 * version
};

// false: not such a header, of a version above 3, or cut short.  What the fields may hold is the caller's to judge.
inline bool raw_header_parse(const uint8_t *b, size_t len, RawHeader *h) {
    if (!b || len < 25 || memcmp(b, "adder", 5) != 0 || b[6] != 'b' || b[5] > 3) return false;
    const uint32_t version = b[5];
    if (len < 25u + 4u * version) return false;
    auto be16 = [&](size_t o) { return (uint32_t)((b[o] << 8) | b[o + 1]); };
    auto be32 = [&](size_t o) {
        return ((uint32_t)b[o] << 24) | ((uint32_t)b[o + 1] << 16) | ((uint32_t)b[o + 2] << 8) | b[o + 3];
    };
    h->version = version;
    h->width = be16(7);
    h->height = be16(9);
    h->tps = be32(11);
    h->ref_interval = be32(15);
    h->delta_t_max = be32(19);
    h->event_size = b[23];
    h->channels = b[24];
    h->source_camera = version >= 1 ? be32(25) : 0u;
    h->time_mode = version >= 2 ? be32(29) : 0u;
    h->adu_interval = version >= 3 ? be32(33) : 0u;
    h->header_bytes = 25u + 4u * version;
    return true;
}

// what all three tools ask of the event size: 9 bytes for one channel, 11 for more, and at least one channel
inline bool raw_header_events_ok(const RawHeader &h) {
    return h.channels != 0u && h.event_size == (h.channels == 1u ? 9u : 11u);
}

}  // namespace adder
