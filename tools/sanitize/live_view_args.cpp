// Stand-alone check of the host-side code of the live view, for a build with -fsanitize=address,undefined (see the
// comment at the end for the command): the C exports' argument checking (include/adder_hip.h: adder_hip_set_view_mode,
// adder_hip_set_show_features, adder_hip_display_frame[_device]) and the C++ mirror's bookkeeping (Video::
// instantaneous_view_mode / practical_d_max / update_detect_features before a device context exists, and the test
// facade's argument checks).  Needs no device: with one, a context is created and the enum checks run on it too.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../adder-codec-rs_amd/host/adder_host.hpp"
#include "../../include/adder_hip.h"

extern "C" long long adder_host_live_view(const uint8_t *frames, uint32_t num_frames, uint16_t width, uint16_t height,
                                          uint8_t channels, uint32_t ref_time, uint32_t delta_t_max, int time_mode,
                                          uint32_t chunk_rows, int view_mode, float practical_d_max, int detect_features,
                                          int show_features, uint8_t *running_out, uint8_t *display_out);
extern "C" const char *adder_host_last_error();

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    using namespace adder_host;
    // null contexts / null destinations
    uint8_t byte = 0;
    CHECK(adder_hip_set_view_mode(nullptr, 0, 0.0f) == ADDER_E_BAD_PARAMS);
    CHECK(adder_hip_set_show_features(nullptr, 0) == ADDER_E_BAD_PARAMS);
    CHECK(adder_hip_display_frame(nullptr, &byte) == ADDER_E_BAD_PARAMS);
    CHECK(adder_hip_display_frame_device(nullptr, &byte, nullptr) == ADDER_E_BAD_PARAMS);
    // with a device: the enum checks and the "never enabled" refusal on a real context
    AdderHipParams p;
    adder_hip_default_params(&p, 16, 8, 1);
    AdderHipCtx *ctx = nullptr;
    const int rc = adder_hip_create(&p, &ctx);
    if (rc == ADDER_OK) {
        CHECK(adder_hip_set_view_mode(ctx, 4, 0.0f) == ADDER_E_BAD_PARAMS);
        CHECK(adder_hip_set_view_mode(ctx, 3, -1.0f) == ADDER_OK);
        CHECK(adder_hip_set_show_features(ctx, 3) == ADDER_E_BAD_PARAMS);
        CHECK(adder_hip_set_show_features(ctx, 2) == ADDER_OK);
        CHECK(adder_hip_display_frame(ctx, nullptr) == ADDER_E_BAD_PARAMS);
        CHECK(adder_hip_display_frame(ctx, &byte) == ADDER_E_BAD_PARAMS);  // the plane was never enabled
        adder_hip_destroy(ctx);
    } else {
        CHECK(rc == ADDER_E_NO_DEVICE || rc == ADDER_E_HIP);
        CHECK(ctx == nullptr && adder_hip_last_error(nullptr) != nullptr);
    }
    // the mirror before a context exists: only bookkeeping
    {
        Video video(PlaneSize(16, 8, 3), nullptr);
        video.instantaneous_view_mode(FramedViewMode::SAE).practical_d_max(12.0f).practical_d_max(std::nullopt);
        video.update_detect_features(true, ShowFeatureMode::Hold, false, true);
        video.update_detect_features(false, ShowFeatureMode::Off, false, false);
        video.instantaneous_view_mode(FramedViewMode::Intensity);
    }
    // the facade's argument checks come before any device call
    std::vector<uint8_t> frame(16 * 8, 7), out(16 * 8);
    CHECK(adder_host_live_view(frame.data(), 1, 16, 8, 1, 255, 7650, 1, 1, 4, 0.0f, 0, 0, out.data(), out.data()) == -1);
    CHECK(strstr(adder_host_last_error(), "bad view mode") != nullptr);
    CHECK(adder_host_live_view(frame.data(), 1, 16, 8, 1, 255, 7650, 1, 1, 0, 0.0f, 0, 3, out.data(), out.data()) == -1);
    CHECK(adder_host_live_view(nullptr, 1, 16, 8, 1, 255, 7650, 1, 1, 0, 0.0f, 0, 0, out.data(), out.data()) == -1);
    CHECK(adder_host_live_view(frame.data(), 1, 0, 8, 1, 255, 7650, 1, 1, 0, 0.0f, 0, 0, nullptr, nullptr) == -1);  // PlaneSize::new
    // valid arguments: runs on a device, fails cleanly without one
    const long long n = adder_host_live_view(frame.data(), 1, 16, 8, 1, 255, 7650, 1, 1, 1, 0.0f, 1, 2, out.data(), out.data());
    CHECK(rc == ADDER_OK ? n >= 0 : n == -1);
    printf(failures ? "FAILED: %d checks\n" : "live view argument checks ok (%d failures)\n", failures);
    return failures ? 1 : 0;
}
// Build and run from adder-codec-rs_amd/ after `make` (the other objects stay as they are):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -x hip csrc/adder_hip_api.cpp csrc/adder_hip_batch.cpp csrc/adder_hip_graphs.cpp csrc/adder_hip_ring_api.cpp \
//       csrc/adder_hip_records_api.cpp csrc/adder_hip_features_api.cpp csrc/adder_hip_sparse_api.cpp \
//       -x c++ host/adder_host.cpp host/adder_host_c.cpp ../tools/sanitize/live_view_args.cpp \
//       -x none $(ls obj/*.o | grep -v 'obj/adder_hip_') -fsanitize=address,undefined -o /tmp/live_view_args && /tmp/live_view_args
