/* adder_compressed_model.h -- C-ABI of the compressed codec's source model on the device.
 *
 * The compressed sink of include/adder_compressed.h does four things on the host: it buckets events into 16x16
 * cubes, sorts them back into per-pixel lists, runs the source model (intra / inter residuals, the lossy bit shift
 * with its f64 intensity test) and range-codes the result.  Only the last is serial.  This object does the first
 * three over AdderEvents that already are in HBM and hands out, per finished ADU,
 *   - the coder's input: 16-bit symbol words, context << 10 | fenwick index (contexts 0 d, 1 t, 2 bitshift, 3 eof),
 *     in the coder's order, for adder_compressed_encoder_ingest_symbols (the bytes it then writes are those the
 *     host sink writes for the same events);
 *   - the decoder-exact reconstructed events: the kept events with the t the lossy bit shift leaves, in the
 *     decoder's order -- element for element what adder_compressed_decode returns for that ADU -- so that the
 *     codec's loss can be framed and measured on the device without coding anything.
 * Events are taken in stream order (AbsoluteT, as the sink requires); those of the still-open ADU stay in HBM inside
 * the object between calls.  No CPU fallback. */
#ifndef ADDER_COMPRESSED_MODEL_H
#define ADDER_COMPRESSED_MODEL_H

#include <stddef.h>
#include <stdint.h>

#include "adder_compressed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AdderCompressedModel AdderCompressedModel;

typedef struct AdderCompressedModelCounters {
    uint64_t events_in;       /* events of the ADUs modelled so far */
    uint64_t events_dropped;  /* of them, dropped by the ingest rule (a pixel's third or later event that is not later
                                 than its last kept one) */
    uint64_t bitshift[16];    /* kept events per bit shift symbol (intra events: 0 or 15) */
} AdderCompressedModelCounters;

/* The same checks as adder_compressed_encoder_create (write_header, threads, tps and source_camera are not used). */
int adder_compressed_model_create(const AdderCompressedParams *p, int device_id, AdderCompressedModel **out);
void adder_compressed_model_destroy(AdderCompressedModel *m);
const char *adder_compressed_model_last_error(const AdderCompressedModel *m);

/* Room for a call's symbol words.  0 (the default): the buffer grows to what a call needs.  Otherwise a call whose
 * ADUs need more returns ADDER_E_OUT_CAPACITY, writes nothing past the buffer and changes nothing:
 * adder_compressed_model_needed tells the words it needs, and the same call succeeds once there is room. */
int adder_compressed_model_set_symbol_capacity(AdderCompressedModel *m, uint64_t words);
int adder_compressed_model_needed(const AdderCompressedModel *m, uint64_t *words);

/* Appends n events in stream order (a device pointer, read on `stream`) and models every ADU the call closes.  Waits
 * for its results.  An event outside the plane or channel: ADDER_E_BAD_PARAMS, nothing changes. */
int adder_compressed_model_ingest_device(AdderCompressedModel *m, const AdderEvent *d_events, size_t n, void *stream);
/* Models the partial last ADU if it holds an event (as adder_compressed_encoder_close submits it); no more events
 * after it. */
int adder_compressed_model_close(AdderCompressedModel *m);

/* --- the results of the last ingest / close, valid until the next --- */
int adder_compressed_model_adus(const AdderCompressedModel *m, uint32_t *n_adus);
/* start_t: n_adus entries; symbol_offsets, event_offsets: n_adus + 1 entries into the two buffers (the last: the
 * total).  Any may be NULL.  cap: the ADUs the arrays hold room for. */
int adder_compressed_model_adu_info(const AdderCompressedModel *m, uint32_t cap, uint32_t *start_t,
                                    uint64_t *symbol_offsets, uint64_t *event_offsets);
int adder_compressed_model_symbols_device(const AdderCompressedModel *m, const uint16_t **d_symbols, uint64_t *n);
/* the copy-out forms: out is a host or a device pointer with room for cap elements */
int adder_compressed_model_symbols(AdderCompressedModel *m, uint16_t *out, uint64_t cap);
int adder_compressed_model_events_device(const AdderCompressedModel *m, const AdderEvent **d_events, uint64_t *n);
int adder_compressed_model_events(AdderCompressedModel *m, AdderEvent *out, uint64_t cap);
/* sums over every ADU modelled so far */
int adder_compressed_model_counters(const AdderCompressedModel *m, AdderCompressedModelCounters *out);
/* The device's share of the last ingest / close, in ms: the sum of the stretches of device work between the call's
 * host waits (the copies, kernels, sort and scans queued on its stream), taken with events; the waits are not in it. */
int adder_compressed_model_last_device_ms(const AdderCompressedModel *m, float *ms);
/* events of the still-open ADU (in HBM) and its start_t */
int adder_compressed_model_open_adu(const AdderCompressedModel *m, uint64_t *n_events, uint32_t *start_t);

#ifdef __cplusplus
}
#endif
#endif /* ADDER_COMPRESSED_MODEL_H */
