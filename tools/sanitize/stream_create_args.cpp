// Stand-alone check of adder_stream_create's parameter checks (include/adder_stream.h), for a build with
// -fsanitize=address,undefined (see the comment at the end for the command).  Every refusal here returns before a
// device is looked for, so the program needs none: the plane whose units and sentinel key do not fit 32 bits
// (65535 x 65535 x 3 wraps to a plausible unit count in 32-bit arithmetic), and the older checks beside it.
#include <stdio.h>
#include <string.h>

#include "../../include/adder_stream.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static AdderStreamParams params(uint16_t w, uint16_t h, uint8_t ch) {
    AdderStreamParams p;
    memset(&p, 0, sizeof p);
    p.abi_version = ADDER_STREAM_ABI_VERSION;
    p.width = w;
    p.height = h;
    p.channels = ch;
    p.codec_version = 2;
    p.out_time_mode = ADDER_TIME_ABSOLUTE_T;
    p.ref_interval = 255;
    return p;
}

static void refused(AdderStreamParams p, const char *text) {
    AdderStream *s = (AdderStream *)&p;  // must come back null
    CHECK(adder_stream_create(&p, &s) == ADDER_E_BAD_PARAMS);
    CHECK(s == nullptr);
    CHECK(strstr(adder_stream_last_error(nullptr), text) != nullptr);
}

int main() {
    AdderStream *s = nullptr;
    CHECK(adder_stream_create(nullptr, &s) == ADDER_E_BAD_PARAMS);
    const AdderStreamParams ok = params(4, 4, 1);
    CHECK(adder_stream_create(&ok, nullptr) == ADDER_E_BAD_PARAMS);
    // width * height * channels + 1 in 64 bits
    refused(params(65535, 65535, 3), "plane 65535x65535x3");
    refused(params(37838, 37838, 3), "plane 37838x37838x3");  // 175 436 units in 32-bit arithmetic
    refused(params(65535, 21846, 3), "plane 65535x21846x3");  // 2^32 + 65 534
    refused(params(0, 4, 1), "plane 0x4x1");
    refused(params(4, 4, 2), "plane 4x4x2");
    AdderStreamParams p = params(4, 4, 1);
    p.ref_interval = 0;
    refused(p, "ref_interval");
    p = params(4, 4, 1);
    p.out_time_mode = 3;
    refused(p, "time modes");
    p = params(4, 4, 1);
    p.abi_version = 2;
    refused(p, "abi_version");
    printf(failures ? "FAILED: %d checks\n" : "stream create argument checks ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
// Build and run from adder-codec-rs_amd/ after `make` (the other objects stay as they are):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -x hip csrc/adder_stream_api.cpp -x c++ ../tools/sanitize/stream_create_args.cpp \
//       -x none $(ls obj/*.o | grep -v adder_stream_api) -fsanitize=address,undefined -o /tmp/stream_create_args && \
//       /tmp/stream_create_args
