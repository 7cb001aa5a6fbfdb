// adder_hip_ring_api.cpp -- the two pipelined forms of include/adder_hip.h: adder_hip_stream_* (raw batches, two in
// flight) and the per-frame ring (adder_hip_frame_submit / _collect).
#include <stdio.h>
#include <string.h>

#include "adder_color_kernels.h"
#include "adder_hip_ctx.hpp"

static int ensure_pinned(AdderHipCtx *c, void **p, size_t *cap, size_t need) {
    if (*cap >= need && *p) return ADDER_OK;
    if (*p) HIPCHK(c, hipHostFree(*p));
    *p = nullptr;
    *cap = 0;
    HIPCHK(c, hipHostMalloc(p, std::max<size_t>(need, 16), hipHostMallocDefault));
    *cap = need;
    return ADDER_OK;
}

// Pipelined raw transcode.  submit(k) uploads and integrates batch k (blocking for exactly
// that), then queues its serialisation and download on a second stream and returns; the
// download of batch k therefore overlaps the upload + integration of batch k+1 when the
// caller submits k+1 before collecting k.  At most two batches are in flight.
extern "C" int adder_hip_stream_submit(AdderHipCtx *c, const uint8_t *frames, uint32_t num_frames,
                                       size_t frame_stride, size_t row_stride, float time_spanned,
                                       size_t out_cap_events) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->submitted - c->collected >= 2)
        return fail(c, ADDER_E_BAD_PARAMS, "two batches are in flight: call adder_hip_stream_collect first");
    HIPCHK(c, hipSetDevice(c->device));
    AdderHipCtx::StreamSlot &sl = c->slot[c->submitted & 1u];
    AdderHipCtx::StreamSlot &prev = c->slot[(c->submitted & 1u) ^ 1u];
    if (!c->out_s) HIPCHK(c, hipStreamCreateWithFlags(&c->out_s, hipStreamNonBlocking));
    if (!sl.done) {
        HIPCHK(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&sl.wired, hipEventDisableTiming));
    }
    // the previous batch's serialisation still reads c->d_events
    if (prev.busy && prev.wired) HIPCHK(c, hipStreamWaitEvent(c->stream, prev.wired, 0));
    size_t total = 0;
    int rc = batch_to_device(c, frames, num_frames, frame_stride, row_stride, time_spanned, out_cap_events, &total);
    if (rc != ADDER_OK) return rc;
    const uint32_t rec = wire_record_bytes(c);
    void *vp = sl.d_wire;
    if ((rc = ensure(c, &vp, &sl.d_wire_cap, total * rec)) != ADDER_OK) return rc;
    sl.d_wire = (uint8_t *)vp;
    vp = sl.h_wire;
    if ((rc = ensure_pinned(c, &vp, &sl.h_wire_cap, total * rec)) != ADDER_OK) return rc;
    sl.h_wire = (uint8_t *)vp;
    vp = sl.h_offsets;
    if ((rc = ensure_pinned(c, &vp, &sl.h_offsets_cap, ((size_t)num_frames + 1) * sizeof(uint64_t))) != ADDER_OK) return rc;
    sl.h_offsets = (uint64_t *)vp;
    sl.n_events = total;
    sl.n_bytes = total * rec;
    // batch_to_device has synchronised c->stream: the events are complete
    HIPCHK(c, adder_launch_wire(reinterpret_cast<const AdderEventPod *>(c->d_events), total, rec, sl.d_wire, c->status,
                                c->out_s));
    HIPCHK(c, hipMemcpyAsync(sl.h_offsets, c->d_offsets, ((size_t)num_frames + 1) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, c->out_s));
    HIPCHK(c, hipEventRecord(sl.wired, c->out_s));
    if (total) HIPCHK(c, hipMemcpyAsync(sl.h_wire, sl.d_wire, total * rec, hipMemcpyDeviceToHost, c->out_s));
    HIPCHK(c, hipMemcpyAsync(&sl.status, c->status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->out_s));
    HIPCHK(c, hipEventRecord(sl.done, c->out_s));
    sl.busy = true;
    c->submitted += 1;
    return ADDER_OK;
}

extern "C" int adder_hip_stream_collect(AdderHipCtx *c, const uint8_t **bytes, size_t *n_bytes, size_t *n_events,
                                        const uint64_t **frame_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->collected == c->submitted) return fail(c, ADDER_E_BAD_PARAMS, "no batch in flight");
    AdderHipCtx::StreamSlot &sl = c->slot[c->collected & 1u];
    HIPCHK(c, hipEventSynchronize(sl.done));
    sl.busy = false;
    c->collected += 1;
    if (bytes) *bytes = sl.h_wire;
    if (n_bytes) *n_bytes = sl.n_bytes;
    if (n_events) *n_events = sl.n_events;
    if (frame_offsets) *frame_offsets = sl.h_offsets;
    return status_to_code(c, sl.status);
}

// ------------------------------------------------------------------------------------------
// Per-frame `consume` contract without a blocking round trip (framed.rs:127-157 calls integrate_matrix once per
// decoded frame).  submit(k) queues upload, integration and hand-over of frame k and returns; collect() waits for
// the oldest frame in flight and returns pointers into its slot of page-locked host memory.  The hand-over
// (adder_frame_out_kernel: events + row-chunk offsets + result header) runs on a second stream, so frame k's
// PCIe transfer overlaps frame k+1's integration.
// ------------------------------------------------------------------------------------------

static size_t frame_slot_events(const AdderHipCtx *c, float time_spanned) {
    if (c->f_events_per_slot) return c->f_events_per_slot;
    const size_t budget = ((size_t)2 << 30) / sizeof(AdderEvent);
    return std::min(worst_case_events_per_frame(c, time_spanned), budget);
}

static int frame_slot_prepare(AdderHipCtx *c, AdderHipCtx::FrameSlot &fs, size_t need, bool need_host_events) {
    if (!fs.d_frame) {
        HIPCHK(c, dalloc(&fs.d_frame, c->n_units + 16));
        HIPCHK(c, dalloc(&fs.d_offsets, 2));
        // the slot's own description (the ring queues one frame per batch: 64 table entries are plenty) and counters
        ADDER_TRY(alloc_batch_desc(c, &fs.desc, 64));
        fs.desc.ring_slot = 1u + (uint32_t)(&fs - c->fslot);
        HIPCHK(c, dalloc(&fs.desc.feat_counters, 4));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&fs.h_hdr),
                                sizeof(FrameResult) + ((size_t)c->num_chunks + 1) * sizeof(uint32_t), hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&fs.done, hipEventDisableTiming));
    }
    if (fs.cap < need) {
        if (fs.d_events) HIPCHK(c, hipFree(fs.d_events));
        if (fs.h_events) HIPCHK(c, hipHostFree(fs.h_events));
        fs.d_events = nullptr;
        fs.h_events = nullptr;
        fs.cap = 0;
        HIPCHK(c, dalloc(&fs.d_events, need));
        fs.cap = need;
    }
    if (need_host_events && !fs.h_events)
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&fs.h_events), std::max<size_t>(fs.cap, 1) * sizeof(AdderEvent),
                                hipHostMallocDefault));
    return ADDER_OK;
}

// direct_out: page-locked memory of the caller that takes the events instead of the slot's own (device view), or null
// workgroups of the ring's wire hand-over: enough to keep the link busy, few enough to leave the next frame's kernels
// their CUs (the stores are posted writes over PCIe: a workgroup spends most of its life waiting on them)
static uint32_t wire_scatter_blocks(const AdderHipCtx *c) {
    static const uint32_t env = [] { const char *e = getenv("ADDER_HIP_WIRE_BLOCKS"); return e ? (uint32_t)atoi(e) : 0u; }();
    return env ? env : c->num_cus * 2u;  // (sweep, 1080p e = 0.3: 64-128: 203, 256: 197, 512: 185, 1024: 189 us per frame)
}

// rgb: `frame` is [rows][width][3] for a one-channel context.  It is uploaded into the slot's colour staging frame and
// converted into the slot's gray frame (adder_color.hip) on the upload stream, in front of the event the frame kernel waits for.
int frame_submit_impl(AdderHipCtx *c, const uint8_t *frame, size_t row_stride, float time_spanned, AdderEvent *direct_out,
                      size_t direct_cap, bool rgb) {
    if (c->poisoned) return refuse_poisoned(c);
    if (c->pending) return fail(c, ADDER_E_BAD_PARAMS, "a device batch is pending (call adder_hip_finish)");
    if (c->submitted != c->collected) return fail(c, ADDER_E_BAD_PARAMS, "a raw stream batch is in flight");
    if (!frame) return fail(c, ADDER_E_BAD_PARAMS, "frame is null");
    if (!(time_spanned >= 0.0f)) return fail(c, ADDER_E_BAD_PARAMS, "time_spanned must be >= 0");
    if (c->f_submitted - c->f_collected >= c->f_slots)
        return fail(c, ADDER_E_BAD_PARAMS, "%u frames are in flight: call adder_hip_frame_collect first", c->f_slots);
    if (band_features(c))
        return fail(c, ADDER_E_BAD_PARAMS, "a row band in feature / ROI mode uses the blocking calls (its feature step "
                    "needs the neighbours' halo between the frames)");
    const size_t rowlen = (size_t)c->p.width * (rgb ? 3u : c->p.channels);
    if (row_stride == 0) row_stride = rowlen;
    if (row_stride < rowlen) return fail(c, ADDER_E_BAD_PARAMS, "row_stride_bytes smaller than a row");
    HIPCHK(c, hipSetDevice(c->device));
    AdderHipCtx::FrameSlot &fs = c->fslot[c->f_submitted % c->f_slots];
    const size_t need = direct_out ? std::min(direct_cap, worst_case_events_per_frame(c, time_spanned))
                                   : frame_slot_events(c, time_spanned);
    int rc = frame_slot_prepare(c, fs, need, direct_out == nullptr);
    if (rc != ADDER_OK) return rc;
    if (!c->out_s) HIPCHK(c, hipStreamCreateWithFlags(&c->out_s, hipStreamNonBlocking));
    if (!c->frame_e) HIPCHK(c, hipEventCreateWithFlags(&c->frame_e, hipEventDisableTiming));
    // The ring's uploads go on a stream of their own, so that the next frame's 2 MB cross the link beside this frame's
    // kernels instead of behind them: 220 -> 84 us per 1080p frame at the default quality (sparse frames: real video).
    // Frames dense with events are bound by their events' way to the host and lose 3 % to the contention (194 -> 200 us
    // at crf 0).  Always, not by the frames' density: a context whose uploads change their HIP stream back and forth stays
    // slow for life (194 -> 238-330 us per dense frame after four uploads on the other stream; `profiles/r04_ring_ab.txt`).
    // ADDER_HIP_RING_DIRECT_WIRE=1 (wire format): the expansion itself stores the records into the slot's page-locked
    // buffer (adder_hip_integrate_wire_device's path, no hand-over pass) -- measured no better for sparse frames and
    // 5 % worse for dense ones (the byte stores at its waves' edges are single PCIe writes): off by default.
    static const bool direct_wire_on = env_flag("ADDER_HIP_RING_DIRECT_WIRE");
    const bool wire_direct = direct_wire_on && c->f_wire && !direct_out && !c->continuous && !feature_path(c);
    const bool own_upload = !direct_out;
    hipStream_t up = c->stream, ring_out = c->out_s;
    bool post_on_main = false;
    if (own_upload) {
        if (!c->in_s) HIPCHK(c, hipStreamCreateWithFlags(&c->in_s, hipStreamNonBlocking));
        if (!c->in_e) HIPCHK(c, hipEventCreateWithFlags(&c->in_e, hipEventDisableTiming));
        if (c->ring_cands.empty()) {
            // the context's own pair, post-processing on the context's stream, and three more pairs -- a spare stream between
            // two pairs, so that the pairs sit at every offset of the runtime's round robin over its (four) hardware queues
            const int n_cands = 5;
            c->ring_cands.resize(n_cands);
            c->ring_cands[0].out_s = c->out_s; c->ring_cands[0].in_s = c->in_s;
            c->ring_cands[1].out_s = c->out_s; c->ring_cands[1].in_s = c->in_s; c->ring_cands[1].post_on_main = true;
            for (int k = 2; k < n_cands; ++k) {
                hipStream_t t[3] = {nullptr, nullptr, nullptr};
                for (hipStream_t &x : t) {
                    HIPCHK(c, hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
                    c->ring_streams.push_back(x);
                }
                c->ring_cands[k].out_s = t[1];  // (t[0]: the spare)
                c->ring_cands[k].in_s = t[2];
            }
            c->ring_cur = 0;
            c->ring_win_frames = c->ring_win_waits = 0;
            c->ring_win_skip = 6;
        }
        // the ring's stream arrangement for this frame (AdderHipCtx::RingCand): the chosen one, or the candidate being measured
        const AdderHipCtx::RingCand &rc_ = c->ring_cands[c->ring_chosen >= 0 ? c->ring_chosen : c->ring_cur];
        up = rc_.in_s;
        ring_out = rc_.out_s;
        post_on_main = rc_.post_on_main;
    }
    if (rgb && !fs.d_rgb) HIPCHK(c, dalloc(&fs.d_rgb, rowlen * c->rows + 16));
    uint8_t *const d_in = rgb ? fs.d_rgb : fs.d_frame;
    if (row_stride == rowlen)
        HIPCHK(c, hipMemcpyAsync(d_in, frame, rowlen * c->rows, hipMemcpyHostToDevice, up));
    else
        HIPCHK(c, hipMemcpy2DAsync(d_in, rowlen, frame, row_stride, rowlen, c->rows, hipMemcpyHostToDevice, up));
    if (rgb)
        HIPCHK(c, color_to_gray_launch(fs.d_rgb, rowlen, rowlen * c->rows, fs.d_frame, c->p.width, c->n_units, c->p.width, c->rows,
                                       1u, up));
    if (own_upload) {
        HIPCHK(c, hipEventRecord(c->in_e, up));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->in_e, 0));
    }
    // The batch goes with the slot's own description (the context's may still be read by the copy engine for the frame
    // before), so it is launched eagerly: the cached batch graphs hold the context's description (get_graph).
    // Only the frame kernel runs on the context's stream; scan, expansion and hand-over of this frame go to the ring's
    // second stream as ONE captured launch per slot and kernel choice (the graph holds the slot's own description), beside
    // the next frame's kernel -- which needs this frame's pixel state and nothing else of it.  The per-frame path is bound
    // by the frames' GPU time in a row at the reference's default quality (kernel 29 us + scan / expansion / hand-over
    // 40 us per 1080p frame: 82 us sustained); side by side the period is the longer of the two.
    const bool ring_graph = c->use_graph;
    // (a ring chunk of scratch per frame slot -- its share of the frame totals must also hold the scan's tile sums, 2 words per
    // tile: planes beyond 16 384 segments with a chunk shortened by the memory budget keep the one-stream form)
    const uint32_t scan_tiles = (c->num_waves + kScanTileWaves - 1u) / kScanTileWaves;
    fs.out = direct_out ? direct_out : fs.h_events;
    fs.out_cap = need;
    BatchRequest rq;
    rq.d_frames = fs.d_frame;
    rq.num_frames = 1;
    rq.time_spanned = time_spanned;
    rq.d_out = wire_direct ? fs.out : fs.d_events;
    rq.out_cap = need;
    rq.d_offsets = fs.d_offsets;
    rq.stream = c->stream;
    rq.wire = wire_direct;
    rq.allow_undo = false;  // frames behind this one are submitted before its outcome is known: no rollback
    rq.frame_only = c->f_slots <= c->ring_chunks && c->chunk >= 2u && c->chunk >= 2u * scan_tiles;
    rq.desc = &fs.desc;
    BatchQueued queued;
    rc = enqueue_frames(c, rq, &queued);
    if (rc != ADDER_OK) {
        c->poisoned = true;
        return rc;
    }
    // (the HIPCHKs from here on return without poisoning the context, unlike the rc paths beside them: as it has been)
    // where the frame's scan / expansion / hand-over go: the ring's second stream (behind an event), or -- post_on_main -- the
    // context's own stream behind the frame kernel (no cross-stream dependency at all)
    hipStream_t post_s = post_on_main ? c->stream : ring_out;
    if (!post_on_main) {
        HIPCHK(c, hipEventRecord(c->frame_e, c->stream));
        HIPCHK(c, hipStreamWaitEvent(ring_out, c->frame_e, 0));
    }
    const bool wire = c->f_wire && !direct_out;
    fs.wire = wire;
    // the hand-over: wire scatter (9 / 11-byte records straight into the slot: 25 % fewer bytes over PCIe, and what the raw
    // sink writes) + frame_out (result header, chunk offsets, the AdderEvents copy)
    const bool split = queued.frame_only_done;  // (feature mode and timed launches queued the whole pipeline themselves)
    const uint32_t post_variant = queued.variant;
    auto hand_over = [&](hipStream_t hs) -> int {
        if (split) {  // the frame's scan (a batch of one frame: it writes the offsets too) and expansion
            HIPCHK(c, adder_launch_scan(fs.desc.d_batch, 0u, 1u, c->num_waves, hs, 1u));
            HIPCHK(c, adder_launch_expand(fs.desc.d_batch, 0u, 1u, c->num_waves, post_variant, 0u, hs));
        }
        if (wire && !wire_direct)
            HIPCHK(c, adder_launch_wire_scatter(reinterpret_cast<const AdderEventPod *>(fs.d_events), fs.d_offsets, 1u,
                                                c->d_side_words + 2, wire_record_bytes(c), reinterpret_cast<uint8_t *>(fs.out),
                                                (uint64_t)fs.out_cap * sizeof(AdderEvent), 0ull, c->status, wire_scatter_blocks(c), hs,
                                                (uint64_t)need));  // (a frame that overflowed its slot: only what the expansion kept is read)
        HIPCHK(c, adder_launch_frame_out(reinterpret_cast<const AdderEventPod *>(wire_direct ? fs.out : fs.d_events), fs.d_offsets, fs.out_cap,
                                         wire ? nullptr : reinterpret_cast<AdderEventPod *>(fs.out), reinterpret_cast<FrameResult *>(fs.h_hdr),
                                         reinterpret_cast<uint32_t *>(fs.h_hdr + sizeof(FrameResult)), c->status,
                                         feature_path(c) ? fs.desc.feat_counters : nullptr, c->p.row_begin, c->p.chunk_rows, c->num_chunks, hs,
                                         wire_direct ? wire_record_bytes(c) : 0u));
        return ADDER_OK;
    };
    if (ring_graph && !direct_out) {  // ... as one launch too: captured per slot, again whenever something it baked in has changed
                                      // (the blocking call's destination is the caller's: not worth a capture per buffer)
        const uint64_t key[6] = {(uint64_t)(uintptr_t)fs.out, (uint64_t)fs.out_cap, (uint64_t)need,
                                 (uint64_t)(wire ? 1u : 0u) | (wire_direct ? 2u : 0u) | (feature_path(c) ? 4u : 0u) | (split ? 8u : 0u) |
                                     ((uint64_t)c->p.chunk_rows << 8) | ((uint64_t)post_variant << 32),
                                 (uint64_t)(uintptr_t)fs.d_events, (uint64_t)wire_scatter_blocks(c)};
        if (!fs.out_graph || memcmp(key, fs.out_key, sizeof key) != 0) {
            if (fs.out_graph) c->retired_execs.push_back(fs.out_graph);
            fs.out_graph = nullptr;
            hipGraph_t graph = nullptr;
            HIPCHK(c, hipStreamBeginCapture(c->cap_s, hipStreamCaptureModeThreadLocal));
            const int rc_h = hand_over(c->cap_s);
            hipError_t e = hipStreamEndCapture(c->cap_s, &graph);
            if (rc_h != ADDER_OK) {
                if (graph) (void)hipGraphDestroy(graph);
                c->poisoned = true;
                return rc_h;
            }
            HIPCHK(c, e);
            e = hipGraphInstantiate(&fs.out_graph, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            HIPCHK(c, e);
            memcpy(fs.out_key, key, sizeof key);
        }
        HIPCHK(c, hipGraphLaunch(fs.out_graph, post_s));
    } else {
        rc = hand_over(post_s);
        if (rc != ADDER_OK) {
            c->poisoned = true;
            return rc;
        }
    }
    HIPCHK(c, hipEventRecord(fs.done, post_s));
    c->f_submitted += 1;
    return ADDER_OK;
}

// Waiting for a frame slot's `done` event: polled for a while before the thread is parked -- an event wait that parks wakes
// up tens of microseconds late (adder_hip_finish spins on its result flag for the same reason), and at one frame per 60 us
// that is a third of the period.
static hipError_t wait_done_event(hipEvent_t e) {
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
    uint32_t polls = 0;
    for (;;) {
        const hipError_t q = hipEventQuery(e);
        if (q == hipSuccess) return hipSuccess;
        if (q != hipErrorNotReady) return q;
        if ((++polls & 15u) == 0u && std::chrono::steady_clock::now() >= t_end) break;
    }
    return hipEventSynchronize(e);
}

int frame_collect_impl(AdderHipCtx *c, const AdderEvent **events, size_t *n_events, const uint32_t **chunk_offsets) {
    if (c->f_collected == c->f_submitted) return fail(c, ADDER_E_BAD_PARAMS, "no frame in flight");
    HIPCHK(c, hipSetDevice(c->device));
    AdderHipCtx::FrameSlot &fs = c->fslot[c->f_collected % c->f_slots];
    if (c->ring_chosen < 0 && !c->ring_cands.empty()) {
        // the candidate's window: frames per wall-clock second while the caller keeps the ring full (a collect that has to
        // wait means the GPU side is the bound; a caller paced by its source never measures, and needs no choice)
        constexpr uint32_t kWindow = 24;
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(c, wait_done_event(fs.done));
        const auto t1 = std::chrono::steady_clock::now();
        if (c->ring_win_skip) {  // (frames queued under the candidate before are still draining)
            if (--c->ring_win_skip == 0u) {
                c->ring_win_t0 = t1;
                c->ring_win_frames = c->ring_win_waits = 0;
            }
        } else {
            c->ring_win_frames += 1;
            if (std::chrono::duration<double, std::micro>(t1 - t0).count() > 3.0) c->ring_win_waits += 1;
            if (c->ring_win_frames == kWindow) {
                if (c->ring_win_waits * 2u >= kWindow) {
                    c->ring_cands[c->ring_cur].us = std::chrono::duration<double, std::micro>(t1 - c->ring_win_t0).count() / kWindow;
                    if (++c->ring_cur == (int)c->ring_cands.size()) {
                        int best = 0;
                        for (int k = 1; k < (int)c->ring_cands.size(); ++k)
                            if (c->ring_cands[k].us < c->ring_cands[best].us) best = k;
                        c->ring_chosen = best;
                        if (getenv("ADDER_HIP_DEBUG_TUNE")) {
                            fprintf(stderr, "[adder_hip] ring stream arrangements (us per frame):");
                            for (const auto &rc_ : c->ring_cands) fprintf(stderr, " %.1f", rc_.us);
                            fprintf(stderr, " -> %d\n", best);
                        }
                    }
                }
                c->ring_win_skip = 6;  // (next candidate, or the same one again when the caller was the bound)
            }
        }
    } else {
        HIPCHK(c, wait_done_event(fs.done));
    }
    c->f_collected += 1;
    const FrameResult *res = reinterpret_cast<const FrameResult *>(fs.h_hdr);
    c->last_new_features = res->new_features;
    c->f_last_produced = res->produced;
    if (events) *events = fs.out;
    if (n_events) *n_events = (size_t)res->produced;
    if (chunk_offsets) *chunk_offsets = reinterpret_cast<const uint32_t *>(fs.h_hdr + sizeof(FrameResult));
    if (res->status == kStatusCapacity) {
        c->poisoned = true;  // later frames were stepped on top of this one: there is nothing to roll back to
        return fail(c, ADDER_E_OUT_CAPACITY, "frame slot too small: the frame produced %llu events, the slot holds %zu "
                    "(adder_hip_frames_configure)", (unsigned long long)res->produced, fs.out_cap);
    }
    return status_to_code(c, res->status);
}

extern "C" int adder_hip_frames_configure(AdderHipCtx *c, uint32_t slots, size_t events_per_slot) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->f_submitted != c->f_collected) return fail(c, ADDER_E_BAD_PARAMS, "frames are in flight");
    if (slots > 4) return fail(c, ADDER_E_BAD_PARAMS, "at most 4 frame slots");
    c->f_slots = slots ? slots : 3u;
    c->f_events_per_slot = events_per_slot;
    return ADDER_OK;
}

extern "C" int adder_hip_frame_submit(AdderHipCtx *c, const uint8_t *frame, size_t row_stride, float time_spanned) {
    if (!c) return ADDER_E_BAD_PARAMS;
    return frame_submit_impl(c, frame, row_stride, time_spanned, nullptr, 0);
}

extern "C" int adder_hip_frame_submit_rgb(AdderHipCtx *c, const uint8_t *frame_hwc3, size_t row_stride, float time_spanned) {
    if (!c) return ADDER_E_BAD_PARAMS;
    ADDER_TRY(rgb_precheck(c));
    return frame_submit_impl(c, frame_hwc3, row_stride, time_spanned, nullptr, 0, true);
}

extern "C" int adder_hip_frame_collect(AdderHipCtx *c, const AdderEvent **events, size_t *n_events,
                                       const uint32_t **chunk_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    // (the slot's own format, as it was submitted: reading packed 9 / 11-byte records as 12-byte events would run past them)
    if (c->f_collected != c->f_submitted && c->fslot[c->f_collected % c->f_slots].wire)
        return fail(c, ADDER_E_BAD_PARAMS, "the oldest frame in flight holds wire records: adder_hip_frame_collect_wire");
    return frame_collect_impl(c, events, n_events, chunk_offsets);
}

extern "C" int adder_hip_frames_set_format(AdderHipCtx *c, int wire_records) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (c->f_submitted != c->f_collected) return fail(c, ADDER_E_BAD_PARAMS, "frames are in flight");
    c->f_wire = wire_records != 0;
    return ADDER_OK;
}
extern "C" int adder_hip_frame_collect_wire(AdderHipCtx *c, const uint8_t **bytes, size_t *n_bytes, size_t *n_events,
                                            const uint32_t **chunk_offsets) {
    if (!c) return ADDER_E_BAD_PARAMS;
    if (!c->f_wire) return fail(c, ADDER_E_BAD_PARAMS, "the ring hands out AdderEvents (adder_hip_frames_set_format)");
    if (c->f_collected != c->f_submitted && !c->fslot[c->f_collected % c->f_slots].wire)
        return fail(c, ADDER_E_BAD_PARAMS, "the oldest frame in flight holds AdderEvents: adder_hip_frame_collect");
    const AdderEvent *ev = nullptr;
    size_t n = 0;
    int rc = frame_collect_impl(c, &ev, &n, chunk_offsets);
    if (bytes) *bytes = reinterpret_cast<const uint8_t *>(ev);
    if (n_events) *n_events = n;
    if (n_bytes) *n_bytes = n * wire_record_bytes(c);
    return rc;
}

extern "C" uint32_t adder_hip_frames_in_flight(const AdderHipCtx *c) {
    return c ? (uint32_t)(c->f_submitted - c->f_collected) : 0u;
}
