/* examples/prophesee_to_adder.c -- the reference's prophesee_to_adder tool from plain C: a Prophesee `.dat` recording
 * -> an ADDER stream (source camera Dvs, AbsoluteT), compressed like the reference tool writes it, or raw with --raw.
 * The records are streamed through the device in chunks (adder_prophesee_push_device); the start-up frames, every
 * complete group and end_events go to the sink in order.  The compressed sink is the CPU one of adder_compressed.h
 * with the tool's metadata: adu_interval = (tps as f32 / ref_time as f32) as usize, c_thresh_max of the crf row.
 *
 *   make -C adder-codec-rs_amd && gcc -O2 -Iinclude -I$ROCM_PATH/include -D__HIP_PLATFORM_AMD__ \
 *       examples/prophesee_to_adder.c -Ladder-codec-rs_amd -ladder_hip -L$ROCM_PATH/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/adder-codec-rs_amd -o prophesee_to_adder
 *   ./prophesee_to_adder in.dat out.adder [--ref-time 1] [--crf 3] [--raw]
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "adder_compressed.h"
#include "adder_prophesee.h"

#define CHUNK_RECORDS (1u << 22)
#define SOURCE_CAMERA_DVS 6u

/* c_thresh_max of the Crf rows 0..9 (rate_controller.rs) */
static const uint8_t CRF_C_THRESH_MAX[10] = {0, 1, 3, 7, 9, 10, 13, 16, 20, 25};

static int usage(void) {
    fprintf(stderr, "usage: prophesee_to_adder IN.dat OUT.adder [--ref-time N] [--crf 0..9] [--raw]\n");
    return 2;
}

/* where the events go: raw records to the file, or the compressed encoder */
typedef struct Sink {
    FILE *g;
    AdderCompressedEncoder *enc;
    uint8_t *buf;
} Sink;

static int sink_events(Sink *s, const AdderEvent *ev, uint64_t n) {
    if (s->enc) return adder_compressed_encoder_ingest(s->enc, ev, n) == ADDER_OK ? 0 : -1;
    for (uint64_t i = 0; i < n; i += 1u << 16) {
        const uint64_t k = n - i < (1u << 16) ? n - i : (1u << 16);
        const size_t b = adder_raw_events(s->buf, ev + i, k, 1);
        if (fwrite(s->buf, 1, b, s->g) != b) return -1;
    }
    return 0;
}

static int grow_host(AdderEvent **ev, uint64_t *cap, uint64_t need) {
    if (need <= *cap) return 0;
    free(*ev);
    *ev = malloc(need * sizeof(AdderEvent));
    *cap = *ev ? need : 0;
    return *ev ? 0 : -1;
}

int main(int argc, char **argv) {
    const char *in_path = NULL, *out_path = NULL;
    uint32_t ref_time = 1;
    int crf = 3, raw = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--ref-time") && i + 1 < argc)
            ref_time = (uint32_t)strtoul(argv[++i], NULL, 10);
        else if (!strcmp(argv[i], "--crf") && i + 1 < argc)
            crf = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--raw"))
            raw = 1;
        else if (!strcmp(argv[i], "--features")) {
            fprintf(stderr, "--features: feature detection on event-camera sources is not built\n");
            return 2;
        } else if (!in_path)
            in_path = argv[i];
        else if (!out_path)
            out_path = argv[i];
        else
            return usage();
    }
    if (!in_path || !out_path || crf < 0 || crf > 9 || ref_time == 0) return usage();
    FILE *f = fopen(in_path, "rb");
    if (!f) return perror(in_path), 1;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    size_t hlen = size < (1 << 20) ? (size_t)size : (1u << 20);
    uint8_t *head = malloc(hlen + 1);
    if (fread(head, 1, hlen, f) != hlen) return fprintf(stderr, "read error\n"), 1;
    AdderPropheseeHeader h;
    int rc = adder_prophesee_parse_header(head, hlen, (uint64_t)size, &h);
    free(head);
    if (rc != ADDER_OK) return fprintf(stderr, "%s: not a .dat header this tool accepts (%d)\n", in_path, rc), 1;

    AdderPropheseeParams p = {ADDER_PROPHESEE_ABI_VERSION, h.width, h.height, ref_time, crf, 0};
    AdderProphesee *pr = NULL;
    if ((rc = adder_prophesee_create(&p, &pr)) != ADDER_OK)
        return fprintf(stderr, "create: %s\n", adder_prophesee_last_error(NULL)), 1;
    const uint64_t eps = adder_prophesee_events_per_step(pr);
    const uint32_t tps = ref_time * 1000000u;  // u32, as the reference computes it
    Sink sink = {fopen(out_path, "wb"), NULL, malloc((size_t)11 << 16)};
    if (!sink.g) return perror(out_path), 1;
    if (raw) {
        uint8_t hdr[64];
        const size_t hb = adder_raw_header(hdr, 3, h.width, h.height, 1, tps, ref_time, ref_time * 2u,
                                           SOURCE_CAMERA_DVS, ADDER_TIME_ABSOLUTE_T, 0);
        fwrite(hdr, 1, hb, sink.g);
    } else {
        AdderCompressedParams cp;
        adder_compressed_default_params(&cp, h.width, h.height, 1);
        cp.codec_version = 3;
        cp.time_mode = ADDER_TIME_ABSOLUTE_T;
        cp.write_header = 1;
        cp.tps = tps;
        cp.ref_interval = ref_time;
        cp.delta_t_max = ref_time * 2u;
        cp.adu_interval = (uint32_t)((float)tps / (float)ref_time);
        cp.source_camera = SOURCE_CAMERA_DVS;
        cp.c_thresh_max = CRF_C_THRESH_MAX[crf];
        if (adder_compressed_encoder_create(&cp, &sink.enc) != ADDER_OK)
            return fprintf(stderr, "compressed sink: %s\n", adder_compressed_last_error(NULL)), 1;
    }

    AdderEvent *ev = NULL;
    uint64_t ev_cap = 0, n = 0, cap = 0;
    adder_prophesee_start(pr, NULL, 0, &cap);
    if (grow_host(&ev, &ev_cap, cap)) return fprintf(stderr, "out of memory\n"), 1;
    if ((rc = adder_prophesee_start(pr, ev, ev_cap, &n)) != ADDER_OK || sink_events(&sink, ev, n))
        return fprintf(stderr, "start: %s\n", adder_prophesee_last_error(pr)), 1;

    // the records on the device, a chunk at a time; the open group's carry is part of the output bound
    uint8_t *h_rec = malloc((size_t)CHUNK_RECORDS * 8u);
    void *d_rec = NULL, *d_ev = NULL;
    uint64_t d_ev_cap = 0;
    if (!h_rec || hipMalloc(&d_rec, (size_t)CHUNK_RECORDS * 8u) != hipSuccess) return fprintf(stderr, "alloc\n"), 1;
    fseek(f, (long)h.header_bytes, SEEK_SET);
    uint64_t total = 0;
    for (;;) {
        const size_t got = fread(h_rec, 8, CHUNK_RECORDS, f);
        if (got == 0) break;
        if (hipMemcpy(d_rec, h_rec, got * 8u, hipMemcpyHostToDevice) != hipSuccess) return 1;
        uint64_t open = 0, bad = 0;
        adder_prophesee_state(pr, NULL, NULL, &open, NULL);
        const uint64_t need = 2u * (open + got) * eps;
        if (need > d_ev_cap) {
            if (d_ev) hipFree(d_ev);
            if (hipMalloc(&d_ev, need * sizeof(AdderEvent)) != hipSuccess) return fprintf(stderr, "hipMalloc\n"), 1;
            d_ev_cap = need;
        }
        rc = adder_prophesee_push_device(pr, d_rec, got, d_ev, d_ev_cap, &n, &bad, NULL);
        if (rc != ADDER_OK) return fprintf(stderr, "push: %s\n", adder_prophesee_last_error(pr)), 1;
        if (grow_host(&ev, &ev_cap, n)) return fprintf(stderr, "out of memory\n"), 1;
        if (n && hipMemcpy(ev, d_ev, n * sizeof(AdderEvent), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        if (sink_events(&sink, ev, n)) return fprintf(stderr, "sink failed\n"), 1;
        total += got;
        if (got < CHUNK_RECORDS) break;
    }
    const uint64_t end_cap = (uint64_t)h.width * h.height * eps;
    if (grow_host(&ev, &ev_cap, end_cap)) return fprintf(stderr, "out of memory\n"), 1;
    if ((rc = adder_prophesee_finish_host(pr, ev, end_cap, &n)) != ADDER_OK || sink_events(&sink, ev, n))
        return fprintf(stderr, "finish: %s\n", adder_prophesee_last_error(pr)), 1;
    if (sink.enc) {
        const uint8_t *bytes = NULL;
        size_t nb = 0;
        if (adder_compressed_encoder_close(sink.enc, &bytes, &nb) != ADDER_OK ||
            fwrite(bytes, 1, nb, sink.g) != nb)
            return fprintf(stderr, "compressed sink: %s\n", adder_compressed_last_error(sink.enc)), 1;
        adder_compressed_encoder_destroy(sink.enc);
    } else {
        uint8_t eof[16];
        const size_t eb = adder_raw_eof(eof);
        fwrite(eof, 1, eb, sink.g);
    }
    fclose(sink.g);
    fclose(f);
    fprintf(stderr, "%llu records, %ux%u\n", (unsigned long long)total, h.width, h.height);
    hipFree(d_rec);
    if (d_ev) hipFree(d_ev);
    free(h_rec);
    free(ev);
    free(sink.buf);
    adder_prophesee_destroy(pr);
    return 0;
}
