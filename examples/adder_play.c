/* examples/adder_play.c -- the reference's adder_video_player from plain C: a raw `.adder` file -> the frames the
 * player would show, written one after the other as raw [height][width][channels] planes of float64 (default) or
 * uint8 (--u8).  The file is streamed through the device in batches of wire records (adder_player_play_wire_device);
 * a batch that would show more frames than the frame buffer holds changes nothing (ADDER_E_OUT_CAPACITY) and is
 * played again in halves.  A batch of one record shows at most one frame.
 *
 *   make -C adder-codec-rs_amd && gcc -O2 -Iinclude -I$ROCM_PATH/include -D__HIP_PLATFORM_AMD__ \
 *       examples/adder_play.c -Ladder-codec-rs_amd -ladder_hip -L$ROCM_PATH/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/adder-codec-rs_amd -o adder_play
 *   ./adder_play in.adder out.raw [--fps 60] [--u8] [--frames K]     (K: frames the device buffer holds)
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "adder_player.h"

#define BATCH_RECORDS (1u << 20)
#define FRAME_BUDGET_BYTES (256u << 20) /* the device frame buffer: as many frames as fit, at least one */

static int usage(void) {
    fprintf(stderr, "usage: adder_play IN.adder OUT.raw [--fps F] [--u8] [--frames K]\n");
    return 2;
}

int main(int argc, char **argv) {
    const char *in_path = NULL, *out_path = NULL;
    double fps = 60.0;
    int u8 = 0;
    uint64_t frame_cap = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--u8"))
            u8 = 1;
        else if (!strcmp(argv[i], "--fps") && i + 1 < argc)
            fps = atof(argv[++i]);
        else if (!strcmp(argv[i], "--frames") && i + 1 < argc)
            frame_cap = strtoull(argv[++i], NULL, 10);
        else if (!in_path)
            in_path = argv[i];
        else if (!out_path)
            out_path = argv[i];
        else
            return usage();
    }
    if (!in_path || !out_path) return usage();

    FILE *f = fopen(in_path, "rb");
    if (!f) return perror(in_path), 1;
    uint8_t hdr[64];
    const size_t hl = fread(hdr, 1, sizeof hdr, f);
    AdderPlayerParams p;
    uint32_t header_bytes = 0, eb = 0;
    if (adder_player_parse_header(hdr, hl, &p, &header_bytes, &eb) != ADDER_OK) {
        fprintf(stderr, "%s: not a raw .adder file\n", in_path);
        return 1;
    }
    p.playback_fps = fps;
    p.out_type = u8 ? ADDER_PLAYER_U8 : ADDER_PLAYER_F64;
    fseek(f, (long)header_bytes, SEEK_SET);
    AdderPlayer *pl = NULL;
    int rc = adder_player_create(&p, &pl);
    if (rc != ADDER_OK) {
        fprintf(stderr, "adder_player_create -> %d: %s\n", rc, adder_player_last_error(NULL));
        return 1;
    }
    FILE *g = fopen(out_path, "wb");
    if (!g) return perror(out_path), 1;

    const size_t fb = (size_t)p.width * p.height * p.channels * (u8 ? 1u : 8u);
    if (frame_cap == 0) frame_cap = FRAME_BUDGET_BYTES / fb;
    if (frame_cap == 0) frame_cap = 1;
    uint8_t *h_in = malloc((size_t)BATCH_RECORDS * eb), *d_in = NULL;
    uint8_t *h_frames = malloc(frame_cap * fb), *d_frames = NULL;
    if (!h_in || !h_frames || hipMalloc((void **)&d_in, (size_t)BATCH_RECORDS * eb) != hipSuccess ||
        hipMalloc((void **)&d_frames, frame_cap * fb) != hipSuccess) {
        fprintf(stderr, "allocation failed\n");
        return 1;
    }
    uint64_t n_in = 0, n_shown = 0;
    int status = 0, ended = 0;
    while (!ended && status == 0) {
        const size_t n = fread(h_in, eb, BATCH_RECORDS, f);
        if (n == 0) { /* no EOF record: the short read ends the stream, its check is still made */
            uint64_t got = 0;
            rc = adder_player_finish(pl, d_frames, frame_cap, &got, NULL);
            if (rc != ADDER_OK) {
                fprintf(stderr, "finish -> %d: %s\n", rc, adder_player_last_error(pl));
                return 1;
            }
            if (got) {
                hipMemcpy(h_frames, d_frames, got * fb, hipMemcpyDeviceToHost);
                fwrite(h_frames, fb, got, g);
            }
            n_shown += got;
            break;
        }
        if (hipMemcpy(d_in, h_in, n * eb, hipMemcpyHostToDevice) != hipSuccess) return 1;
        size_t at = 0, take = n;
        while (at < n) {
            if (take > n - at) take = n - at;
            uint64_t got = 0, bad = ADDER_PLAYER_NO_BAD_EVENT, consumed = 0;
            rc = adder_player_play_wire_device(pl, d_in + at * eb, take, d_frames, frame_cap, &got, &bad, &consumed,
                                               NULL);
            if (rc == ADDER_E_OUT_CAPACITY && take > 1) {
                take = (take + 1) / 2; /* nothing changed: the same records again, half as many */
                continue;
            }
            if (rc != ADDER_OK && rc != ADDER_PLAYER_E_BAD_EVENT) {
                fprintf(stderr, "play -> %d: %s\n", rc, adder_player_last_error(pl));
                return 1;
            }
            if (got) {
                hipMemcpy(h_frames, d_frames, got * fb, hipMemcpyDeviceToHost);
                fwrite(h_frames, fb, got, g);
            }
            n_shown += got;
            if (rc == ADDER_PLAYER_E_BAD_EVENT) {
                fprintf(stderr, "event %llu: %s\n", (unsigned long long)(n_in + bad), adder_player_last_error(pl));
                n_in += bad;
                status = 1;
                break;
            }
            n_in += consumed;
            if (consumed < take) { /* the EOF record: the call has made the stream's last check */
                ended = 1;
                break;
            }
            at += take;
        }
    }
    fclose(g);
    fclose(f);
    uint32_t current_t = 0;
    uint64_t frame_count = 0;
    adder_player_clock(pl, &current_t, &frame_count);
    printf("%llu ADDER events -> %llu frames (current_t %u)\n", (unsigned long long)n_in, (unsigned long long)n_shown,
           current_t);
    hipFree(d_in);
    hipFree(d_frames);
    free(h_in);
    free(h_frames);
    adder_player_destroy(pl);
    return status;
}
