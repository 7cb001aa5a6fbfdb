/* examples/adder_migrate.c -- the reference's migrate_raw_v0_v1_to_v2 tool from plain C: a raw `.adder` file
 * rewritten in another time mode.  The body is streamed through the device in batches of wire records
 * (adder_stream_migrate_wire_host); the output carries the rewritten header and ends with the 11-byte EOF record.
 *
 *   make -C adder-codec-rs_amd && gcc -O2 -Iinclude examples/adder_migrate.c -Ladder-codec-rs_amd -ladder_hip \
 *       -Wl,-rpath,$PWD/adder-codec-rs_amd -o adder_migrate
 *   ./adder_migrate IN.adder OUT.adder delta_t|absolute|mixed
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <strings.h>

#include "adder_stream.h"

#define BATCH_RECORDS (1u << 22)

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: adder_migrate IN.adder OUT.adder delta_t|absolute|mixed\n");
        return 2;
    }
    uint32_t time_mode;
    if (!strcasecmp(argv[3], "delta_t"))
        time_mode = ADDER_TIME_DELTA_T;
    else if (!strcasecmp(argv[3], "absolute"))
        time_mode = ADDER_TIME_ABSOLUTE_T;
    else if (!strcasecmp(argv[3], "mixed"))
        time_mode = ADDER_TIME_MIXED;
    else {
        fprintf(stderr, "Invalid time mode\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 1;
    uint8_t hdr[64], out_hdr[64], eof[16];
    const size_t hl = fread(hdr, 1, sizeof hdr, f);
    AdderStreamParams p;
    uint32_t header_bytes = 0, eb = 0;
    if (adder_stream_parse_header(hdr, hl, &p, &header_bytes, &eb) != ADDER_OK) {
        fprintf(stderr, "%s: not a raw .adder file\n", argv[1]);
        return 1;
    }
    p.out_time_mode = (uint8_t)time_mode;
    fseek(f, (long)header_bytes, SEEK_SET);
    AdderStream *s = NULL;
    int rc = adder_stream_create(&p, &s);
    if (rc != ADDER_OK) {
        fprintf(stderr, "adder_stream_create -> %d: %s\n", rc, adder_stream_last_error(NULL));
        return 1;
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) return perror(argv[2]), 1;
    fwrite(out_hdr, 1, adder_stream_migrated_header(hdr, hl, time_mode, out_hdr, sizeof out_hdr), g);

    uint8_t *in = malloc((size_t)BATCH_RECORDS * eb), *out = malloc((size_t)BATCH_RECORDS * eb);
    if (!in || !out) return 1;
    uint64_t total = 0;
    int status = 0;
    for (;;) {
        const size_t n = fread(in, eb, BATCH_RECORDS, f);
        if (n == 0) break;
        uint64_t bad = ADDER_STREAM_NO_BAD_EVENT, consumed = 0;
        rc = adder_stream_migrate_wire_host(s, in, n, out, &bad, &consumed);
        if (rc != ADDER_OK && rc != ADDER_STREAM_E_BAD_EVENT) {
            fprintf(stderr, "migrate -> %d: %s\n", rc, adder_stream_last_error(s));
            return 1;
        }
        const uint64_t done = bad < consumed ? bad : consumed;
        fwrite(out, eb, done, g);
        total += done;
        if (rc == ADDER_STREAM_E_BAD_EVENT) {
            fprintf(stderr, "event %llu cannot be migrated: %s\n", (unsigned long long)total, adder_stream_last_error(s));
            status = 1;
            break;
        }
        if (consumed < n || n < BATCH_RECORDS) break; /* EOF record, or the end of the file */
    }
    fwrite(eof, 1, adder_raw_eof(eof), g);
    fclose(g);
    fclose(f);
    if (status == 0) printf("Done!\n");
    free(in);
    free(out);
    adder_stream_destroy(s);
    return status;
}
