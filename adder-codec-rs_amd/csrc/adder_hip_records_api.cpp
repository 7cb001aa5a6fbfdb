// adder_hip_records_api.cpp -- what leaves a context other than as its own AdderEvents (include/adder_hip.h): a band's
// records over the wire and their expansion at the root, wire serialisation, the sink layout, the merge of the bands.
#include <string.h>

#include "adder_hip_ctx.hpp"

// ---- records over the wire ----
extern "C" uint32_t adder_hip_band_segments(const AdderHipCtx *c) { return c ? c->num_waves : 0u; }

extern "C" int adder_hip_integrate_records_device(AdderHipCtx *c, const uint8_t *d_frames, uint32_t num_frames,
                                                  float time_spanned, uint64_t *d_frame_offsets, void *stream,
                                                  AdderBandRecords *out) {
    if (!c || !out) return ADDER_E_BAD_PARAMS;
    if (c->poisoned) return refuse_poisoned(c);
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "previous device batch not finished (call adder_hip_finish)");
    if (c->f_submitted != c->f_collected || c->submitted != c->collected)
        return fail(c, ADDER_E_BAD_PARAMS, "frames are in flight (collect them first)");
    if (!d_frames || !d_frame_offsets || num_frames == 0) return fail(c, ADDER_E_BAD_PARAMS, "null pointer / no frames");
    if (!(time_spanned >= 0.0f)) return fail(c, ADDER_E_BAD_PARAMS, "time_spanned must be >= 0");
    // The lean regime is a precondition the CALLER can miss (include/adder_gather.h: "gather events instead"): it is
    // checked before anything is touched -- no scratch re-laid out, no graph retired, no poisoned context.
    if (c->generic_sticky || c->perpx || c->continuous || c->sparse_mode || feature_path(c) || feature_needs_perpx(c) ||
        !(c->p.multi_mode == ADDER_MULTI_COLLAPSE && (float)c->p.delta_t_max <= time_spanned))
        return fail(c, ADDER_E_BAD_PARAMS, "records can be handed out in the lean regime only (Collapse, delta_t_max <= "
                    "time_spanned, no feature mode, no generic batch before): gather events instead");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!stream) ADDER_TRY(join_null_stream(c));
    // the scratch must exist before the chunk size is known
    ADDER_TRY(alloc_scratch(c, c->p.time_mode == ADDER_TIME_ABSOLUTE_T ? kScratchLean : kScratchLean8));
    static_assert(AdderHipCtx::ring_chunks >= 2, "a records batch is packed into the ring's second chunk");
    if (num_frames > c->chunk)
        return fail(c, ADDER_E_BAD_PARAMS, "a records batch holds at most adder_hip_chunk_frames() = %u frames", c->chunk);
    BatchRequest rq;
    rq.d_frames = d_frames;
    rq.num_frames = num_frames;
    rq.time_spanned = time_spanned;
    rq.out_cap = (size_t)1 << 62;
    rq.d_offsets = d_frame_offsets;
    rq.stream = s;
    rq.records_only = true;
    rq.allow_undo = false;  // (nothing can overflow: no event buffer)
    rq.desc = &c->own;
    BatchQueued queued;
    int rc = enqueue_frames(c, rq, &queued);
    if (rc != ADDER_OK) {
        c->poisoned = true;
        return rc;
    }
    // the batch started at slot 0: the first num_frames rows of the rings are its tables, chunk 0 of the ring its logs (or
    // its fixed slots: lean-runs records); the used prefixes are packed into chunk 1's (idle) region, the runs re-based
    // onto the packed buffer
    const uint32_t rb = lean_rec_bytes(c->p.time_mode == ADDER_TIME_ABSOLUTE_T);
    const uint32_t cap = kWaveUnits * c->chunk;
    const size_t chunk_bytes = (size_t)c->num_waves * cap * rb;
    uint8_t *const packed = c->park_ring + chunk_bytes;
    const bool runs = (queued.variant & kVarLeanRuns) != 0u;  // adder_lr_kernel ran: {rho, word} records, frame-major packing
    if (runs) {
        HIPCHK(c, adder_launch_slot_pack(c->own.d_batch, num_frames, c->num_waves, rb, packed, chunk_bytes, c->status, s));
    } else {
        uint32_t *const pbase = c->wcur + c->num_waves;
        uint64_t *const d_total = c->d_side_words;  // (its own word: wcur holds ring_chunks >= 2 rows and two are in use)
        HIPCHK(c, adder_launch_log_pack(c->park_ring, cap, rb, c->wcur, pbase, c->num_waves, num_frames, c->wofs_ring, packed,
                                        chunk_bytes, d_total, c->status, s));
    }
    HIPCHK(c, hipEventRecord(c->ev_stop, s));
    out->num_frames = num_frames;
    out->num_segments = c->num_waves;
    out->record_bytes = rb | (runs ? (uint32_t)ADDER_RECORDS_RUNS : 0u);
    out->row_begin = c->p.row_begin;
    out->rows = c->rows;
    out->d_counts = c->wtot_ring;
    out->d_prefix = c->wpref_ring;
    out->d_runs = c->wofs_ring;
    out->d_records = packed;
    out->d_frame_offsets = d_frame_offsets;
    out->d_frame_table = c->own.d_ftab;
    c->pending = true;
    c->pending_stream = s;
    c->pending_offsets = d_frame_offsets;
    c->pending_frames = num_frames;
    c->pending_cap = (size_t)1 << 62;
    return ADDER_OK;
}

// wire: d_merged receives the raw sink's 9 / 11-byte records (merged_cap / merged_base still count events)
static int expand_records_impl(AdderHipCtx *c, const AdderBandRecords *bands, uint32_t n_bands, AdderEvent *d_merged,
                               size_t merged_cap, uint64_t merged_base, uint64_t *d_merged_offsets, void *stream, bool wire) {
    if (!c || !bands || n_bands == 0 || !d_merged_offsets || (!d_merged && merged_cap)) return ADDER_E_BAD_PARAMS;
    if (c->poisoned) return refuse_poisoned(c);
    const uint32_t nf = bands[0].num_frames;
    const bool abs_t = c->p.time_mode == ADDER_TIME_ABSOLUTE_T;
    // root's share of an expansion is the time step's constants and the frames' running_t: those of its last batch.  A
    // root that has integrated nothing since adder_hip_create / adder_hip_reset has neither (own.ftab_cap does not tell:
    // the table is allocated with the context, and nothing has written it)
    if (nf == 0 || nf > kMaxChunk || nf > c->own.ftab_cap || c->frames_done == 0)
        return fail(c, ADDER_E_BAD_PARAMS, "bad num_frames (root integrates the same frames first)");
    const bool runs = (bands[0].record_bytes & (uint32_t)ADDER_RECORDS_RUNS) != 0u;  // lean-runs records (expansion format 6)
    for (uint32_t r = 0; r < n_bands; ++r)
        if (bands[r].num_frames != nf || bands[r].record_bytes != (lean_rec_bytes(abs_t) | (runs ? (uint32_t)ADDER_RECORDS_RUNS : 0u)) || !bands[r].d_counts ||
            !bands[r].d_prefix || !bands[r].d_runs || !bands[r].d_records || !bands[r].d_frame_offsets ||
            bands[r].num_segments % (uint32_t)ADDER_EXPAND_SEGS != 0u || bands[r].rows == 0)
            return fail(c, ADDER_E_BAD_PARAMS, "band %u: bad description", r);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // event C's table (root's own lean-runs batches build it too; a root that only expands needs it all the same)
    if (runs) ADDER_TRY(ensure_lr_tab(c, c->last_time_spanned, s));
    // device block: n_bands BatchArgs, then the bands' offsets pointers, then the destination table [n_bands][nf]
    const size_t ptrs_at = (size_t)n_bands * kBatchDescBytes;
    const size_t dest_at = ptrs_at + (((size_t)n_bands * sizeof(uint64_t *) + 255) & ~(size_t)255);
    const size_t bytes = dest_at + (size_t)n_bands * nf * sizeof(uint64_t);
    constexpr uint32_t kSlots = AdderHipCtx::kBandDescSlots;
    if (c->band_desc_cap < bytes) {
        HIPCHK(c, hipStreamSynchronize(s));  // (the kernels queued from the old block have to be through: rare, it only grows)
        if (c->d_band_desc) HIPCHK(c, hipFree(c->d_band_desc));
        if (c->h_band_desc) HIPCHK(c, hipHostFree(c->h_band_desc));
        c->d_band_desc = c->h_band_desc = nullptr;
        c->band_desc_cap = 0;
        const size_t slot_bytes = (bytes + 4095) & ~(size_t)4095;
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_band_desc), slot_bytes * kSlots));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_band_desc), slot_bytes * kSlots, hipHostMallocDefault));
        c->band_desc_cap = slot_bytes;
        for (hipEvent_t &e : c->band_desc_e) {
            if (e) HIPCHK(c, hipEventDestroy(e));
            e = nullptr;
        }
    }
    const uint32_t slot = c->band_desc_next++ % kSlots;
    if (c->band_desc_e[slot]) HIPCHK(c, hipEventSynchronize(c->band_desc_e[slot]));  // the call four calls ago is through
    else HIPCHK(c, hipEventCreateWithFlags(&c->band_desc_e[slot], hipEventDisableTiming));
    uint8_t *const d_blk = c->d_band_desc + (size_t)slot * c->band_desc_cap;
    uint8_t *const h_blk = c->h_band_desc + (size_t)slot * c->band_desc_cap;
    uint64_t *const d_dest = reinterpret_cast<uint64_t *>(d_blk + dest_at);
    const uint64_t **h_ptrs = reinterpret_cast<const uint64_t **>(h_blk + ptrs_at);
    for (uint32_t r = 0; r < n_bands; ++r) {
        BatchArgs &b = *reinterpret_cast<BatchArgs *>(h_blk + (size_t)r * kBatchDescBytes);
        memset(&b, 0, sizeof b);
        base_args(c, &b.base);
        b.base.status = reinterpret_cast<uint32_t *>(c->d_side_words + 1);  // (the expansions' own word: d_side_words)
        b.base.n_units = bands[r].rows * c->p.width * c->p.channels;
        b.base.num_waves = bands[r].num_segments;
        b.base.row_begin = bands[r].row_begin;
        b.base.out = reinterpret_cast<AdderEventPod *>(d_merged);
        b.base.out_cap = merged_cap;
        b.base.frame_offsets = d_dest + (size_t)r * nf;  // (the expansion reads [f] only: where the band's frame starts)
        b.base.lean = runs ? 2u : 1u;
        b.base.abs_t = abs_t ? 1u : 0u;
        b.base.wire_rec = wire ? wire_record_bytes(c) : 0u;
        b.lr_tab = c->d_lr_tab;
        b.base.sc = make_consts(c, c->last_time_spanned);
        // the frames' running_t (D_EMPTY fillers): root's own batch of the same frames, or the copy the caller kept of it
        b.ftab = bands[r].d_frame_table ? const_cast<FrameTab *>(reinterpret_cast<const FrameTab *>(bands[r].d_frame_table)) : c->own.d_ftab;
        b.park_ring = const_cast<uint8_t *>(bands[r].d_records);
        b.park_bytes = 0;
        b.log_cap = 0;  // (expansion format 3 with a zero region stride: the runs index ONE packed buffer)
        b.wofs_ring = const_cast<uint32_t *>(bands[r].d_runs);
        b.wtot_ring = const_cast<uint32_t *>(bands[r].d_counts);
        b.wpref_ring = const_cast<uint32_t *>(bands[r].d_prefix);
        b.park_layout = ParkLayout{0u, 0u, 0u, 0u, 31u, 0xffffffffu};
        b.slots = kMaxChunk;  // slot of frame f = f: the tables' rows
        b.chunk = kMaxChunk;
        h_ptrs[r] = bands[r].d_frame_offsets;
    }
    HIPCHK(c, hipMemcpyAsync(d_blk, h_blk, dest_at, hipMemcpyHostToDevice, s));
    HIPCHK(c, adder_launch_band_layout(reinterpret_cast<const uint64_t *const *>(d_blk + ptrs_at), n_bands, nf,
                                       merged_base, d_merged_offsets, d_dest, s));
    if (n_bands <= kMaxBands) {  // every band in ONE launch, frame-major across the bands
        uint32_t nw[kMaxBands];
        for (uint32_t r = 0; r < n_bands; ++r) nw[r] = bands[r].num_segments;
        HIPCHK(c, adder_launch_expand_bands(d_blk, (uint32_t)kBatchDescBytes, n_bands, nw, nf, abs_t ? 1u : 0u, s, runs ? 1u : 0u,
                                            wire ? 1u : 0u));
    } else {
        const uint32_t variant = kVarCollapse | (abs_t ? kVarAbsT : 0u) | kVarLeanLog | (runs ? kVarLeanRuns : 0u) | (wire ? kVarWire : 0u);
        for (uint32_t r = 0; r < n_bands; ++r)
            HIPCHK(c, adder_launch_expand(reinterpret_cast<const BatchArgs *>(d_blk + (size_t)r * kBatchDescBytes), 0u, nf,
                                          bands[r].num_segments, variant, 0u, s));
    }
    HIPCHK(c, hipEventRecord(c->band_desc_e[slot], s));  // (the device block is read by the kernels: free after them)
    return ADDER_OK;
}
extern "C" int adder_hip_expand_records_device(AdderHipCtx *c, const AdderBandRecords *bands, uint32_t n_bands,
                                               AdderEvent *d_merged, size_t merged_cap, uint64_t merged_base,
                                               uint64_t *d_merged_offsets, void *stream) {
    return expand_records_impl(c, bands, n_bands, d_merged, merged_cap, merged_base, d_merged_offsets, stream, false);
}
extern "C" int adder_hip_expand_records_wire_device(AdderHipCtx *c, const AdderBandRecords *bands, uint32_t n_bands,
                                                    uint8_t *d_wire, size_t wire_cap_bytes, uint64_t merged_base,
                                                    uint64_t *d_merged_offsets, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    return expand_records_impl(c, bands, n_bands, reinterpret_cast<AdderEvent *>(d_wire), wire_cap_bytes / wire_record_bytes(c),
                               merged_base, d_merged_offsets, stream, true);
}

static size_t wire_align(size_t x) { return (x + 255) & ~(size_t)255; }
extern "C" void adder_hip_records_wire_sections(uint32_t nf, uint32_t nseg, uint32_t rb, size_t sec[6]) {
    (void)rb;
    const size_t tab = wire_align((size_t)nf * nseg * sizeof(uint32_t));
    sec[0] = 0;                                                    // frame offsets
    sec[1] = sec[0] + wire_align(((size_t)nf + 1) * sizeof(uint64_t));  // frame table
    sec[2] = sec[1] + wire_align((size_t)nf * sizeof(FrameTab));   // counts
    sec[3] = sec[2] + tab;                                         // prefix
    sec[4] = sec[3] + tab;                                         // runs
    sec[5] = sec[4] + tab;                                         // records
}
extern "C" size_t adder_hip_records_wire_bytes(uint32_t nf, uint32_t nseg, uint32_t rb, uint64_t n_records) {
    size_t sec[6];
    adder_hip_records_wire_sections(nf, nseg, rb, sec);
    return sec[5] + wire_align((size_t)n_records * (rb & 0xffu));  // (record_bytes may carry ADDER_RECORDS_RUNS)
}
extern "C" int adder_hip_records_to_wire(AdderHipCtx *c, const AdderBandRecords *rec, uint64_t n_records, void *d_dst,
                                         size_t dst_bytes, void *stream) {
    if (!c || !rec || !d_dst) return ADDER_E_BAD_PARAMS;
    static_assert(sizeof(FrameTab) == 8, "the wire image's frame table rows");
    const uint32_t nf = rec->num_frames, nseg = rec->num_segments, rb = rec->record_bytes;
    if (adder_hip_records_wire_bytes(nf, nseg, rb, n_records) > dst_bytes) return fail(c, ADDER_E_BAD_PARAMS, "wire buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    // (null: the stream the context's last batch ran on -- the copies are then ordered before its next batch)
    hipStream_t s = stream ? (hipStream_t)stream : (c->pending_stream ? c->pending_stream : c->stream);
    size_t sec[6];
    adder_hip_records_wire_sections(nf, nseg, rb, sec);
    uint8_t *dst = static_cast<uint8_t *>(d_dst);
    const size_t tab = (size_t)nf * nseg * sizeof(uint32_t);
    HIPCHK(c, hipMemcpyAsync(dst + sec[0], rec->d_frame_offsets, ((size_t)nf + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dst + sec[1], rec->d_frame_table ? rec->d_frame_table : c->own.d_ftab, (size_t)nf * sizeof(FrameTab),
                             hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dst + sec[2], rec->d_counts, tab, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dst + sec[3], rec->d_prefix, tab, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dst + sec[4], rec->d_runs, tab, hipMemcpyDeviceToDevice, s));
    if (n_records) HIPCHK(c, hipMemcpyAsync(dst + sec[5], rec->d_records, (size_t)n_records * (rb & 0xffu), hipMemcpyDeviceToDevice, s));
    return ADDER_OK;
}

extern "C" int adder_hip_expand_status(AdderHipCtx *c, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    uint32_t st = 0;
    uint32_t *const word = reinterpret_cast<uint32_t *>(c->d_side_words + 1);
    HIPCHK(c, hipMemcpyAsync(&st, word, sizeof st, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (st) HIPCHK(c, hipMemsetAsync(word, 0, sizeof(uint32_t), s));
    if (st & kStatusCapacity)
        return fail(c, ADDER_E_OUT_CAPACITY, "the merged event buffer was too small: events were dropped");
    return status_to_code(c, st);
}

extern "C" int adder_hip_chunk_offsets_device(AdderHipCtx *c, const AdderEvent *d_events, size_t n_events,
                                              uint32_t *d_chunk_offsets, void *stream) {
    if (!c || !d_chunk_offsets) return ADDER_E_BAD_PARAMS;
    if (n_events > 0xffffffffull) return fail(c, ADDER_E_BAD_PARAMS, "too many events for one frame");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, adder_launch_chunk_offsets(reinterpret_cast<const AdderEventPod *>(d_events), (uint32_t)n_events,
                                         c->p.row_begin, c->p.chunk_rows, c->num_chunks, d_chunk_offsets, s));
    return ADDER_OK;
}

extern "C" int adder_hip_wire_events_device(AdderHipCtx *c, const AdderEvent *d_events, size_t n_events,
                                            uint8_t *d_out, size_t out_cap_bytes, size_t *n_bytes, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (n_bytes) *n_bytes = 0;
    if ((!d_events || !d_out) && n_events) return fail(c, ADDER_E_BAD_PARAMS, "null device buffer");
    if (((uintptr_t)d_events & 3u) != 0u) return fail(c, ADDER_E_BAD_PARAMS, "d_events must be 4-byte aligned (AdderEvent alignment)");
    const size_t need = n_events * wire_record_bytes(c);
    if (n_bytes) *n_bytes = need;
    if (need > out_cap_bytes) return fail(c, ADDER_E_OUT_CAPACITY, "wire buffer too small: need %zu bytes", need);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, adder_launch_wire(reinterpret_cast<const AdderEventPod *>(d_events), n_events, wire_record_bytes(c), d_out,
                                c->status, (hipStream_t)stream));
    return ADDER_OK;
}

// ---- sink per rank (include/adder_hip.h; SURVEY 8(e): every GPU delivers its own segments) ----
extern "C" int adder_hip_sink_layout_device(AdderHipCtx *c, const uint64_t *d_all_offsets, uint32_t world, uint32_t rank,
                                            uint32_t num_frames, uint64_t *d_file_pos, uint64_t *d_dest,
                                            uint64_t *d_merged_offsets, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!d_all_offsets || !d_file_pos || !d_dest || world == 0 || rank >= world || num_frames == 0)
        return fail(c, ADDER_E_BAD_PARAMS, "sink layout: null pointer / bad rank / no frames");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, adder_launch_sink_layout(d_all_offsets, world, rank, num_frames, d_file_pos, d_dest, d_merged_offsets,
                                       (hipStream_t)stream));
    return ADDER_OK;
}
extern "C" int adder_hip_wire_scatter_device(AdderHipCtx *c, const AdderEvent *d_events, const uint64_t *d_frame_offsets,
                                             uint32_t num_frames, const uint64_t *d_dest, uint8_t *out, uint64_t out_cap_bytes,
                                             uint64_t header_bytes, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!d_events || !d_frame_offsets || !d_dest || !out) return fail(c, ADDER_E_BAD_PARAMS, "wire scatter: null pointer");
    // (the kernel takes a segment's dword phase from its byte OFFSET in the image: the image itself must start on a dword)
    if ((((uintptr_t)d_events | (uintptr_t)out) & 3u) != 0u)
        return fail(c, ADDER_E_BAD_PARAMS, "wire scatter: d_events and out must be 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    // (the events per frame are known on the device only: a fixed grid of workgroups walks every frame's blocks)
    HIPCHK(c, adder_launch_wire_scatter(reinterpret_cast<const AdderEventPod *>(d_events), d_frame_offsets, num_frames, d_dest,
                                        wire_record_bytes(c), out, out_cap_bytes, header_bytes,
                                        reinterpret_cast<uint32_t *>(c->d_side_words + 1), c->num_cus * kScatterGroupsPerCu, (hipStream_t)stream));
    return ADDER_OK;
}

// ---- multi-GPU: merge of the row bands' streams (include/adder_hip.h) ----
extern "C" size_t adder_hip_merge_work_bytes(uint32_t world, uint32_t num_frames) {
    return ((size_t)num_frames + 1 + (size_t)world * num_frames) * sizeof(uint64_t);
}

// merged_base: events of the merged stream that precede this batch (a chunk of a longer stream: d_out is then the place
// of the chunk's first event, d_merged_offsets the entry of its first frame, and the offsets written continue from there)
extern "C" int adder_hip_merge_streams_device_at(AdderHipCtx *c, const AdderEvent *d_stage, const uint64_t *d_rank_offsets,
                                                 uint32_t world, uint32_t num_frames, void *d_work, AdderEvent *d_out,
                                                 size_t out_cap, uint64_t *d_merged_offsets, uint64_t merged_base, void *stream) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!d_rank_offsets || !d_work || world == 0 || (!d_out && out_cap))
        return fail(c, ADDER_E_BAD_PARAMS, "merge: null pointer or empty world");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (num_frames == 0) {
        if (d_merged_offsets) HIPCHK(c, hipMemcpyAsync(d_merged_offsets, &merged_base, sizeof(uint64_t), hipMemcpyHostToDevice, s));
        return ADDER_OK;
    }
    HIPCHK(c, adder_launch_merge(reinterpret_cast<const AdderEventPod *>(d_stage), d_rank_offsets, world, num_frames,
                                 reinterpret_cast<uint64_t *>(d_work), reinterpret_cast<AdderEventPod *>(d_out), out_cap,
                                 d_merged_offsets, merged_base, c->status, s));
    return ADDER_OK;
}

extern "C" int adder_hip_merge_streams_device(AdderHipCtx *c, const AdderEvent *d_stage, const uint64_t *d_rank_offsets,
                                              uint32_t world, uint32_t num_frames, void *d_work, AdderEvent *d_out,
                                              size_t out_cap, uint64_t *d_merged_offsets, void *stream) {
    return adder_hip_merge_streams_device_at(c, d_stage, d_rank_offsets, world, num_frames, d_work, d_out, out_cap,
                                             d_merged_offsets, 0ull, stream);
}
