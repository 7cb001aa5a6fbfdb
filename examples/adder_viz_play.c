/* examples/adder_viz_play.c -- the adder-viz player from plain C: a raw `.adder` file -> the frames the interactive
 * player would show (its running_frame after every popped frame), written one after the other as raw
 * [height][width][channels] uint8 planes; --popped writes the popped frames themselves (None as 0).  The file is
 * streamed through the device in batches of wire records (adder_viz_player_ingest_wire, the host-pointer form); a batch
 * that pops more frames than the buffer holds changes nothing (ADDER_E_OUT_CAPACITY) and is run again with the room it
 * asked for; one whose units run past the pending ring is fed in halves.  The end of the file (or --records K) is the
 * end of the stream: adder_viz_player_finish.
 *
 *   make -C adder-codec-rs_amd && gcc -O2 -Iinclude examples/adder_viz_play.c -Ladder-codec-rs_amd -ladder_hip \
 *       -Wl,-rpath,$PWD/adder-codec-rs_amd -o adder_viz_play
 *   ./adder_viz_play in.adder out.raw [--limit N | --no-limit] [--speed S] [--popped] [--records K] [--features]
 * --features switches the player's feature detection on (adder.rs:282): the running frames carry the overlay crosses,
 * and one line per frame goes to stdout: `frame J: end_ts T, F features`.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "adder_player.h" /* adder_player_parse_header */
#include "adder_viz_player.h"

#define BATCH_RECORDS (1u << 20)

static int usage(void) {
    fprintf(stderr, "usage: adder_viz_play IN.adder OUT.raw [--limit N | --no-limit] [--speed S] [--popped] [--records K] [--features]\n");
    return 2;
}

static uint32_t be32(const uint8_t *b) {
    return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
}

int main(int argc, char **argv) {
    const char *in_path = NULL, *out_path = NULL;
    int has_limit = 1, form = ADDER_VIZ_FRAME_RUNNING, features = 0;
    uint32_t limit = 60;
    float speed = 1.0f;
    uint64_t max_records = UINT64_MAX;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--popped"))
            form = ADDER_VIZ_FRAME_POPPED;
        else if (!strcmp(argv[i], "--features"))
            features = 1;
        else if (!strcmp(argv[i], "--no-limit"))
            has_limit = 0;
        else if (!strcmp(argv[i], "--limit") && i + 1 < argc)
            limit = (uint32_t)strtoul(argv[++i], NULL, 10);
        else if (!strcmp(argv[i], "--speed") && i + 1 < argc)
            speed = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--records") && i + 1 < argc)
            max_records = strtoull(argv[++i], NULL, 10);
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
    AdderPlayerParams hp;
    uint32_t header_bytes = 0, eb = 0;
    if (adder_player_parse_header(hdr, hl, &hp, &header_bytes, &eb) != ADDER_OK) {
        fprintf(stderr, "%s: not a raw .adder file\n", in_path);
        return 1;
    }
    fseek(f, (long)header_bytes, SEEK_SET);
    AdderVizPlayerParams p;
    memset(&p, 0, sizeof p);
    p.abi_version = ADDER_VIZ_PLAYER_ABI_VERSION;
    p.width = hp.width;
    p.height = hp.height;
    p.channels = hp.channels;
    p.codec_version = hdr[5];
    p.time_mode = hp.time_mode;
    p.has_buffer_limit = (uint8_t)has_limit;
    p.buffer_limit = limit;
    p.tps = hp.tps;
    p.ref_interval = hp.ref_interval;
    p.delta_t_max = be32(hdr + 19);
    /* adder.rs:263-269: tps / ref_interval for framed cameras, else 60; divided by the playback speed (f32) */
    p.output_fps = (hp.source_camera <= 5u ? (float)hp.tps / (float)hp.ref_interval : 60.0f) / speed;
    p.source_camera = hp.source_camera;
    AdderVizPlayer *pl = NULL;
    int rc = adder_viz_player_create(&p, &pl);
    if (rc != ADDER_OK) {
        fprintf(stderr, "adder_viz_player_create -> %d: %s\n", rc, adder_viz_player_last_error(NULL));
        return 1;
    }
    if (features && (rc = adder_viz_player_detect_features(pl, 1)) != ADDER_OK) {
        fprintf(stderr, "adder_viz_player_detect_features -> %d: %s\n", rc, adder_viz_player_last_error(pl));
        return 1;
    }
    FILE *g = fopen(out_path, "wb");
    if (!g) return perror(out_path), 1;

    const size_t fb = (size_t)p.width * p.height * p.channels;
    uint64_t frame_cap = 16;
    uint8_t *in = malloc((size_t)BATCH_RECORDS * eb), *frames = malloc(frame_cap * fb);
    if (!in || !frames) return fprintf(stderr, "allocation failed\n"), 1;
    uint64_t n_in = 0, n_read = 0, n_shown = 0, xy_cap = 0;
    uint64_t *end_ts = NULL, *offsets = NULL;
    uint16_t *xy = NULL;
    int status = 0, at_end = 0;
    while (status == 0) {
        size_t n = 0;
        if (!at_end) {
            size_t want = BATCH_RECORDS;
            if (max_records - n_read < want) want = (size_t)(max_records - n_read);
            n = want ? fread(in, eb, want, f) : 0;
            n_read += n;
            if (n == 0) at_end = 1;
        }
        size_t at = 0, take = n;
        for (;;) { /* the batch, in pieces when its units run past the pending ring; or the end of the stream */
            if (take > n - at) take = n - at;
            uint64_t got = 0, bad = ADDER_VIZ_PLAYER_NO_BAD_EVENT, consumed = 0;
            rc = at_end ? adder_viz_player_finish(pl, form, frames, frame_cap, &got, NULL)
                        : adder_viz_player_ingest_wire(pl, in + at * eb, take, form, frames, frame_cap, &got, NULL, &bad,
                                                       &consumed);
            if (rc == ADDER_E_OUT_CAPACITY && got > frame_cap) { /* nothing changed: again, with the room it asks for */
                frame_cap = got;
                free(frames);
                frames = malloc(frame_cap * fb);
                if (!frames) return fprintf(stderr, "allocation failed\n"), 1;
                continue;
            }
            if (rc == ADDER_E_OUT_CAPACITY && !at_end && take > 1) { /* the ring: nothing changed, half as many */
                take = (take + 1) / 2;
                continue;
            }
            if (rc != ADDER_OK && rc != ADDER_VIZ_PLAYER_E_BAD_EVENT) {
                fprintf(stderr, "-> %d: %s\n", rc, adder_viz_player_last_error(pl));
                return 1;
            }
            fwrite(frames, fb, got, g);
            if (features && got) { /* the FeatureInterval popped with each of these frames */
                uint64_t pairs = 0;
                end_ts = realloc(end_ts, got * sizeof *end_ts);
                offsets = realloc(offsets, (got + 1) * sizeof *offsets);
                if (!end_ts || !offsets) return fprintf(stderr, "allocation failed\n"), 1;
                int rf = adder_viz_player_frame_features(pl, end_ts, offsets, xy, xy_cap, &pairs);
                if (rf == ADDER_E_OUT_CAPACITY) {
                    xy_cap = pairs;
                    xy = realloc(xy, xy_cap * 2 * sizeof *xy);
                    if (!xy) return fprintf(stderr, "allocation failed\n"), 1;
                    rf = adder_viz_player_frame_features(pl, end_ts, offsets, xy, xy_cap, &pairs);
                }
                if (rf != ADDER_OK) {
                    fprintf(stderr, "-> %d: %s\n", rf, adder_viz_player_last_error(pl));
                    return 1;
                }
                for (uint64_t j = 0; j < got; ++j)
                    printf("frame %llu: end_ts %llu, %llu features\n", (unsigned long long)(n_shown + j),
                           (unsigned long long)end_ts[j], (unsigned long long)(offsets[j + 1] - offsets[j]));
            }
            n_shown += got;
            if (at_end) break;
            if (rc == ADDER_VIZ_PLAYER_E_BAD_EVENT) {
                fprintf(stderr, "event %llu: %s\n", (unsigned long long)(n_in + bad), adder_viz_player_last_error(pl));
                n_in += bad;
                status = 1;
                break;
            }
            n_in += consumed;
            if (consumed < take) { /* the EOF record */
                at_end = 1;
                break;
            }
            at += take;
            if (at >= n) break;
        }
        if (at_end && n == 0) break;
    }
    fclose(g);
    fclose(f);
    printf("%llu ADDER events -> %llu frames (frames_written %lld)\n", (unsigned long long)n_in,
           (unsigned long long)n_shown, (long long)adder_viz_player_frames_written(pl));
    free(in);
    free(frames);
    free(end_ts);
    free(offsets);
    free(xy);
    adder_viz_player_destroy(pl);
    return status;
}
