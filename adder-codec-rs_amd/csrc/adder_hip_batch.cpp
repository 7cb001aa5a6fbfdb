// adder_hip_batch.cpp -- one batch from its request to its launches (adder_hip_ctx.hpp): what the plan reads of the
// context, the scratch ring, the launch loops, the undo copy, and enqueue_frames, which every entry point queues through.
#include <string.h>

#include <cmath>

#include "adder_hip_ctx.hpp"

StepConsts make_consts(const AdderHipCtx *c, float time_spanned) {
    StepConsts sc;
    sc.time_spanned = time_spanned;
    sc.running_t = 0.0f;  // per frame: BatchArgs::ftab
    sc.running_t_u32 = 0u;
    sc.dtm_f = (float)c->p.delta_t_max;
    sc.ref_time = c->p.ref_time;
    sc.cth = 0u;          // per frame: BatchArgs::ftab
    sc.collapse = c->p.multi_mode == ADDER_MULTI_COLLAPSE ? 1u : 0u;
    sc.abs_t = c->p.time_mode == ADDER_TIME_ABSOLUTE_T ? 1u : 0u;
    sc.max_depth = c->max_depth;
    sc.ref_magic = c->p.ref_time >= 2 ? (uint32_t)(0x100000000ull / c->p.ref_time) : 0u;
    return sc;
}

// D view's divisor when the caller has not pinned one: the reference's argument (an integer division, video.rs) with
// the logarithm taken exactly (its fast_math::log2_raw is an approximation: include/adder_framer.h)
static float practical_d_max_exact(uint32_t delta_t_max, uint32_t ref_time) {
    return (float)std::log2((double)(255.0f * (float)(delta_t_max / ref_time)));
}
ViewConsts make_view(const AdderHipCtx *c) {
    ViewConsts v;
    v.view_mode = c->view_mode;
    v.ref_time = c->p.ref_time;
    v.delta_t_max = c->p.delta_t_max;
    v.practical_d_max = c->practical_d_max > 0.0f ? c->practical_d_max : practical_d_max_exact(c->p.delta_t_max, c->p.ref_time);
    return v;
}

void base_args(const AdderHipCtx *c, FrameArgs *a) {
    memset(a, 0, sizeof *a);
    a->hdr = c->hdr;
    a->integ0 = c->integ0;
    a->dt0 = c->dt0;
    a->bdt0 = c->bdt0;
    a->lastf = c->lastf;
    a->dv_integ = c->dv_integ;
    a->dv_dt = c->dv_dt;
    a->dv_bdt = c->dv_bdt;
    a->dv_bd = c->dv_bd;
    a->cn_integ = c->cn_integ;
    a->cn_dt = c->cn_dt;
    a->cn_bdt = c->cn_bdt;
    a->cn_meta = c->cn_meta;
    a->max_nodes = c->max_depth + 1u;
    a->stage_events = c->max_depth + 3u;
    a->running = c->running_enabled ? c->running : nullptr;
    a->cth_px = c->perpx ? c->cth_px : nullptr;
    a->cctr_px = c->perpx ? c->cctr_px : nullptr;
    a->c_max = c->p.c_thresh_max;
    a->c_vel = c->p.c_increase_velocity;
    a->plane_stride = c->n_pad;
    a->status = c->status;
    a->n_units = c->n_units;
    a->num_waves = c->num_waves;
    a->width = c->p.width;
    a->channels = c->p.channels;
    a->rowlen = (uint32_t)c->p.width * c->p.channels;
    a->row_begin = c->p.row_begin;
}

// (Re)allocates a description's two blocks for `frames` table entries (its counters and ring_slot stay)
int alloc_batch_desc(AdderHipCtx *c, BatchDesc *d, size_t frames) {
    uint8_t *od = reinterpret_cast<uint8_t *>(d->d_batch), *oh = reinterpret_cast<uint8_t *>(d->h_batch);
    d->d_batch = d->h_batch = nullptr;
    d->d_ftab = d->h_ftab = nullptr;
    d->ftab_cap = 0;
    if (od) HIPCHK(c, hipFree(od));
    if (oh) HIPCHK(c, hipHostFree(oh));
    const size_t bytes = kBatchDescBytes + frames * sizeof(FrameTab);
    uint8_t *nd = nullptr, *nh = nullptr;
    HIPCHK(c, dalloc(&nd, bytes));
    d->d_batch = reinterpret_cast<BatchArgs *>(nd);
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&nh), bytes, hipHostMallocDefault));
    d->h_batch = reinterpret_cast<BatchArgs *>(nh);
    d->d_ftab = reinterpret_cast<FrameTab *>(nd + kBatchDescBytes);
    d->h_ftab = reinterpret_cast<FrameTab *>(nh + kBatchDescBytes);
    d->ftab_cap = frames;
    return ADDER_OK;
}

// planes of the feature path, on first use; the batch's counters live with its description (a frame slot's are
// allocated with the slot, the context's own here)
static int prepare_feature_set(AdderHipCtx *c, BatchDesc *desc, hipStream_t s) {
    if (!c->fset) {
        HIPCHK(c, dalloc(&c->fset, (size_t)c->rows * c->p.width));
        HIPCHK(c, hipMemsetAsync(c->fset, 0, (size_t)c->rows * c->p.width, s));
    }
    if (!c->fstamp && !is_band(c)) {
        HIPCHK(c, dalloc(&c->fstamp, (size_t)c->rows * c->p.width));
        HIPCHK(c, hipMemsetAsync(c->fstamp, 0, (size_t)c->rows * c->p.width * sizeof(uint32_t), s));
    }
    if (!desc->feat_counters) HIPCHK(c, dalloc(&desc->feat_counters, 4));
    HIPCHK(c, hipMemsetAsync(desc->feat_counters, 0, 4 * sizeof(uint32_t), s));
    return ADDER_OK;
}
// the per-unit (c_thresh, c_increase_counter) pair starts from the uniform one
static int prepare_per_unit_c_thresh(AdderHipCtx *c, hipStream_t s) {
    if (feature_needs_perpx(c) && !c->perpx) {
        if (!c->cth_px) {
            HIPCHK(c, dalloc(&c->cth_px, c->n_pad));
            HIPCHK(c, dalloc(&c->cctr_px, c->n_pad));
        }
        HIPCHK(c, hipMemsetAsync(c->cth_px, c->c_thresh, c->n_pad, s));
        HIPCHK(c, hipMemsetAsync(c->cctr_px, c->c_counter, c->n_pad, s));
        c->perpx = true;
    }
    return ADDER_OK;
}

// what the batch plan (adder_batch_plan.hpp) reads of the context, for a batch of num_frames frames of time_spanned
static BatchPlanIn plan_input(const AdderHipCtx *c, uint32_t num_frames, float time_spanned, bool wire, bool records_only) {
    BatchPlanIn in{};
    in.multi_mode = c->p.multi_mode; in.time_mode = c->p.time_mode; in.channels = c->p.channels;
    in.delta_t_max = c->p.delta_t_max; in.dtm_max_seen = c->dtm_max_seen; in.ref_time = c->p.ref_time;
    in.c_thresh = c->c_thresh; in.c_thresh_max = c->p.c_thresh_max;
    in.n_units = c->n_units; in.max_depth = c->max_depth; in.launch_depth = launch_depth(c);
    in.continuous = c->continuous; in.generic_sticky = c->generic_sticky; in.perpx = c->perpx;
    in.needs_perpx = feature_needs_perpx(c); in.feature_path = feature_path(c);
    in.cr_valid = c->cr_valid; in.frac_time_seen = c->frac_time_seen; in.cr_time = c->cr_time;
    in.frames_done = c->frames_done; in.run_bound = c->run_bound;
    in.records_only = records_only; in.wire_batch = wire;
    in.side_view = c->running_enabled ? (uint8_t)c->view_mode : 0u;
    in.num_frames = num_frames; in.time_spanned = time_spanned;
    return in;
}
size_t worst_case_events_per_frame(const AdderHipCtx *c, float time_spanned) {
    return worst_case_events_per_frame(plan_input(c, 1u, time_spanned, false, false));
}

// (Re)allocates the compaction scratch ring for one kind of record.  Fixed-slot kinds: the lean step parks at most
// one 12-byte record per unit and frame (kLeanParkBytes per segment), a Continuous context stages max_depth + 3 events
// per unit.  Log kinds (per-event records): one region per segment and CHUNK holding the hard bound of what the
// segment can emit over the chunk (log_capacity: 2 or 3 events per unit and frame + one arena), instead of a slot per
// frame that would have to hold a whole arena per unit -- 18 instead of 144 bytes per unit and frame at 64 frames.
// Chunk = frames per scan launch: as many as the budget allows (ring_chunks chunks are in flight), at most kMaxChunk.
// The budget is a third of what the device has free, at most 96 GiB (a 1080p plane takes 3 - 5 GiB at 64-frame
// chunks; a 4K RGB one -- 12 times the units -- needs 88 GiB for 64-frame chunks of per-event logs and fell to 48-frame
// chunks under round 4's 64 GiB: a 64-frame batch then paid the state's round trip twice).
static size_t scratch_bytes_per_chunk(const AdderHipCtx *c, ScratchKind kind, uint32_t chunk) {
    switch (kind) {
        case kScratchLean: return (size_t)c->num_waves * chunk * kLeanParkBytes;
        case kScratchLean8: return (size_t)c->num_waves * chunk * kLeanPark8Bytes;
        case kScratchCont:
            return (size_t)c->num_waves * chunk * (kWaveUnits + kWaveUnits * (c->max_depth + 3u) * kGenRecBytes);
        case kScratchLog2: return (size_t)c->num_waves * log_capacity(chunk, c->max_depth, true) * kGenRecBytes;
        case kScratchLog3: return (size_t)c->num_waves * log_capacity(chunk, c->max_depth, false) * kGenRecBytes;
        default: return 0;
    }
}
// The scratch ring holds ring_chunks chunks of frames: chunk k is stepped while chunk k-1 is scanned and expanded
// (launch_frame_loop makes the step of chunk k wait for the expansion of chunk k - ring_chunks).
int alloc_scratch(AdderHipCtx *c, ScratchKind kind) {
    // (a Collapse context that has the general log can run the bounded step on it: no thrash between the two)
    if (c->park_ring && (c->scratch_kind == kind || (c->scratch_kind == kScratchLog3 && kind == kScratchLog2)))
        return ADDER_OK;
    retire_graphs(c);  // they bake the chunking
    void *old[] = {c->park_ring, c->wtot_ring, c->wpref_ring, c->ftot_ring, c->wofs_ring, c->wcur};
    c->park_ring = nullptr;
    c->wtot_ring = c->wpref_ring = c->ftot_ring = c->wofs_ring = c->wcur = nullptr;
    c->park_bytes = 0;
    c->log_cap = 0;
    c->scratch_kind = kScratchNone;
    for (void *p : old)
        if (p) HIPCHK(c, hipFree(p));
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t budget = std::min<size_t>((size_t)96 << 30, free_b / 3);
    uint32_t ch = kMaxChunk;
    while (ch > 1u && c->ring_chunks * (scratch_bytes_per_chunk(c, kind, ch) + (size_t)c->num_waves * ch * 12u) > budget) --ch;
    c->chunk = ch;
    if (const char *e = getenv("ADDER_HIP_CHUNK")) c->chunk = std::max(1, std::min<int>(atoi(e), kMaxChunk));
    c->slots = c->ring_chunks * c->chunk;
    HIPCHK(c, dalloc(&c->park_ring, (size_t)c->ring_chunks * scratch_bytes_per_chunk(c, kind, c->chunk)));
    HIPCHK(c, dalloc(&c->wtot_ring, (size_t)c->slots * c->num_waves));
    HIPCHK(c, dalloc(&c->wpref_ring, (size_t)c->slots * c->num_waves));
    // events, then parked records per frame, then the scan's tile sums [slot][tile][2] (planes scanned in tiles)
    HIPCHK(c, dalloc(&c->ftot_ring, 2 * (size_t)c->slots + (size_t)c->slots * ((c->num_waves + kScanTileWaves - 1) / kScanTileWaves) * 2));
    if (kind != kScratchCont) {  // (the lean records of blocked batches go to logs too: lean_log_cap)
        HIPCHK(c, dalloc(&c->wofs_ring, (size_t)c->slots * c->num_waves));
        HIPCHK(c, dalloc(&c->wcur, (size_t)c->ring_chunks * c->num_waves));
    }
    if (kind == kScratchLog2 || kind == kScratchLog3) {
        c->log_cap = log_capacity(c->chunk, c->max_depth, kind == kScratchLog2);
    } else {
        c->park_bytes = (uint32_t)(scratch_bytes_per_chunk(c, kind, 1u) / c->num_waves);
    }
    c->scratch_kind = kind;
    return ADDER_OK;
}

// Levels >= 1 of the arena: only the generic kernels use them.
static int alloc_deep_planes(AdderHipCtx *c) {
    if (c->dv_integ) return ADDER_OK;
    const size_t deep = std::max<uint32_t>(c->max_depth, 2u) - 1u;
    HIPCHK(c, dalloc(&c->dv_integ, c->n_pad * deep));
    HIPCHK(c, dalloc(&c->dv_dt, c->n_pad * deep));
    HIPCHK(c, dalloc(&c->dv_bdt, c->n_pad * deep));
    HIPCHK(c, dalloc(&c->dv_bd, c->n_pad * deep));
    return ADDER_OK;
}

// The launch sequence of a batch.  Frames are handled in chunks of c->chunk; per chunk
//   * K1 launches back to back, each stepping up to frames_per_launch consecutive frames
//     (frame f+1 only needs frame f's pixel state),
//   * one scan launch (a block per frame) + the frame_offsets chain,
//   * the expansion of the chunk's parked records.
// With a second stream (graph capture), scan/offsets/expand of chunk k go to s2 behind the chunk's last
// K1, and the K1s of chunk k+2 wait for them (the scratch ring holds two chunks).  Running the
// expansion inside K1's grid (round 1) no longer pays: with the lean step both kernels are bound by the
// memory system, and a resident K1 grid leaves no wave slots for a concurrent kernel anyway.
static Lean1wArgs lean1w_args(const AdderHipCtx *c) {
    return Lean1wArgs{c->hdr, c->integ0, c->dt0, c->bdt0, c->lastf, c->n_units, c->num_waves};
}

// Feature path: frame f+1's contrast thresholds depend on the features frame f's EVENTS reveal, so the whole
// pipeline runs frame by frame: step, scan, offsets, expansion, features.
static int launch_feature_loop(AdderHipCtx *c, const BatchRequest &rq, uint32_t variant, hipStream_t s) {
    const BatchArgs *const d_batch = rq.desc->d_batch;
    const Lean1wArgs wide = lean1w_args(c);
    const FeatureArgs fa = feature_args(c, *rq.desc);
    const bool band = band_features(c);  // the feature step waits for the halo exchange: adder_hip_feature_detect
    for (uint32_t f = 0; f < rq.num_frames; ++f) {
        HIPCHK(c, adder_launch_frame(d_batch, f, 1u, variant, c->num_waves, 0u, s, &wide));
        HIPCHK(c, adder_launch_scan(d_batch, f, 1u, c->num_waves, s));
        HIPCHK(c, adder_launch_offsets(d_batch, f, 1u, s));
        HIPCHK(c, adder_launch_expand(d_batch, f, 1u, c->num_waves, variant, 0u, s));
        if (!band) HIPCHK(c, adder_launch_features(d_batch, f, &fa, s));
    }
    HIPCHK(c, adder_launch_publish(d_batch, rq.num_frames, c->h_result, s));
    return ADDER_OK;
}

// (s / s2: where the launches go -- the request's stream, or the capture streams of a graph being instantiated)
int launch_frame_loop(AdderHipCtx *c, const BatchRequest &rq, uint32_t variant, hipStream_t s, hipStream_t s2, bool timing) {
    const uint32_t num_frames = rq.num_frames;
    const BatchArgs *const d_batch = rq.desc->d_batch;
    // temporal blocking is off while the running-intensities side plane is wanted (per-frame
    // semantics).  Generic batches block too: levels >= 1 stay in HBM, but they are private
    // to their unit, so the lane's own program order keeps them consistent across frames.
    const uint32_t depth = launch_depth(c);
    const Lean1wArgs wide = lean1w_args(c);
    const bool keep_undo = c->snap.valid && c->snap.lean2;  // the first launch keeps the batch's undo copy (get_graph keys on it)
    // With a second stream the expansion of chunk k runs beside the frame kernel of chunk k+1.  The frame kernel is
    // bound by instruction issue, the expansion by memory, and two grids that each fill the chip would simply run one
    // after the other (measured: the scan queued behind the resident frame kernel for a whole kernel time): both are
    // launched with a few workgroups per CU that walk their work, so that both are resident on every CU.
    const bool share = s2 != nullptr && num_frames > c->chunk;
    const bool walk = share && !(variant & kVarGeneric);  // (generic batches: full grids)
    const uint32_t lean_cap = walk ? c->lean_blocks_per_cu * c->num_cus : 0u;
    const uint32_t expand_cap = walk ? c->expand_blocks_per_cu * c->num_cus : 0u;
    uint32_t k = 0;
    for (uint32_t f0 = 0; f0 < num_frames; f0 += c->chunk, ++k) {
        const uint32_t nf = std::min(c->chunk, num_frames - f0);
        if (s2 && k >= c->ring_chunks)  // scratch reuse: the expansion of the chunk that held these slots
            HIPCHK(c, hipStreamWaitEvent(s, c->cap_e2[(k - c->ring_chunks) % 5u], 0));
        const bool per_chunk = timing && c->launch_timing == 2;
        if (per_chunk) HIPCHK(c, hipEventRecord(c->launch_events[2 * c->timed_pairs], s));
        for (uint32_t f = f0; f < f0 + nf; f += depth) {
            const uint32_t nb = std::min(depth, f0 + nf - f);
            if (timing && !per_chunk) HIPCHK(c, hipEventRecord(c->launch_events[2 * c->timed_pairs], s));
            HIPCHK(c, adder_launch_frame(d_batch, f, nb, variant | variant_lazy_state_bit(variant, f + nb < num_frames, c->running_enabled) | variant_keep_undo_bit(variant, f == 0u, keep_undo),
                                         c->num_waves, lean_cap, s, &wide));
            if (timing) {  // the pair brackets the frame kernel (K1) only
                if (!per_chunk) {
                    HIPCHK(c, hipEventRecord(c->launch_events[2 * c->timed_pairs + 1], s));
                    c->timed_pairs += 1;
                }
                c->timed_launches += 1;
                c->timed_frames += nb;
            }
        }
        if (per_chunk) {  // ... or the chunk's whole run of them (no event packets between the launches)
            HIPCHK(c, hipEventRecord(c->launch_events[2 * c->timed_pairs + 1], s));
            c->timed_pairs += 1;
        }
        // (scan + offsets on a third stream of their own -- they depend on the chunk's frame kernels only -- was
        // tried: they then run at once instead of behind the previous expansion, and the expansions, now back to
        // back, take as much longer as was gained: the two big kernels compete for the same thing; in-kernel
        // timestamps, adder_hip_debug_timeline)
        hipStream_t t = s;
        if (s2) {
            HIPCHK(c, hipEventRecord(c->cap_e1, s));
            HIPCHK(c, hipStreamWaitEvent(s2, c->cap_e1, 0));
            t = s2;
        }
        if (timing) HIPCHK(c, hipEventRecord(c->post_events[2 * c->timed_posts], t));
        // (a lean-runs batch that hands its records out: the scan also leaves the segments' record prefix, for the packing)
        // (the integer-state kernels' and the bounded Collapse kernel's batches: the scan's blocks chain the frame offsets
        // themselves, adder_scan_kernel CHAIN -- a launch less per chunk; those frame kernels zero the entries, chain_zero)
        const bool chain = variant_scan_chains(variant) && num_frames != 1u && !rq.records_only;
        HIPCHK(c, adder_launch_scan(d_batch, f0, nf, c->num_waves, t, num_frames == 1u ? 1u : 0u,
                                    (rq.records_only && (variant & kVarLeanRuns)) ? 1u : 0u, chain ? 1u : 0u));
        if (num_frames != 1u && !chain) HIPCHK(c, adder_launch_offsets(d_batch, f0, nf, t));  // (one frame: done by the scan)
        if (!rq.records_only) HIPCHK(c, adder_launch_expand(d_batch, f0, nf, c->num_waves, variant, expand_cap, t, rq.desc->h_batch));
        if (timing) {
            HIPCHK(c, hipEventRecord(c->post_events[2 * c->timed_posts + 1], t));
            c->timed_posts += 1;
        }
        if (s2) HIPCHK(c, hipEventRecord(c->cap_e2[k % 5u], s2));
    }
    if (s2 && k) HIPCHK(c, hipStreamWaitEvent(s, c->cap_e2[(k - 1) % 5u], 0));  // join (s2 is in-order)
    HIPCHK(c, adder_launch_publish(d_batch, num_frames, c->h_result, s));
    return ADDER_OK;
}

// ---- undo copy of the state (see AdderHipCtx::Snapshot) ----
template <class T>
static hipError_t snap_copy(T **dst, const T *src, size_t count, hipStream_t s) {
    if (!*dst) {
        hipError_t e = dalloc(dst, count);
        if (e != hipSuccess) return e;
    }
    return hipMemcpyAsync(*dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, s);
}
// the host's side of the undo copy
static void snapshot_scalars(AdderHipCtx *c) {
    AdderHipCtx::Snapshot &n = c->snap;
    n.running_t = c->running_t;
    n.c_thresh = c->c_thresh;
    n.c_counter = c->c_counter;
    n.frames_done = c->frames_done;
    n.run_bound = c->run_bound;
    n.generic_sticky = c->generic_sticky;
    n.valid = true;
}
static int take_snapshot(AdderHipCtx *c, bool deep, hipStream_t s) {
    AdderHipCtx::Snapshot &n = c->snap;
    n.lean2 = false;
    HIPCHK(c, snap_copy(&n.slab, c->state_slab, c->slab_bytes, s));  // the five level-0 planes + status, one copy
    if (c->continuous) {
        const size_t cnt = c->n_pad * (c->max_depth + 1u);
        HIPCHK(c, snap_copy(&n.cn_integ, c->cn_integ, cnt, s));
        HIPCHK(c, snap_copy(&n.cn_dt, c->cn_dt, cnt, s));
        HIPCHK(c, snap_copy(&n.cn_bdt, c->cn_bdt, cnt, s));
        HIPCHK(c, snap_copy(&n.cn_meta, c->cn_meta, cnt, s));
    }
    // levels >= 1: the batch's first launch stores every unit's LIVE levels into the copy (BatchArgs::snap_dv_*);
    // the buffers only have to exist
    n.deep = deep && c->dv_integ;
    if (n.deep && !n.dv_integ) {
        const size_t cnt = c->n_pad * (std::max<uint32_t>(c->max_depth, 2u) - 1u);
        HIPCHK(c, dalloc(&n.dv_integ, cnt));
        HIPCHK(c, dalloc(&n.dv_dt, cnt));
        HIPCHK(c, dalloc(&n.dv_bdt, cnt));
        HIPCHK(c, dalloc(&n.dv_bd, cnt));
    }
    n.perpx = c->perpx;
    if (c->perpx) {
        HIPCHK(c, snap_copy(&n.cth_px, c->cth_px, c->n_pad, s));
        HIPCHK(c, snap_copy(&n.cctr_px, c->cctr_px, c->n_pad, s));
    }
    if (c->fset) HIPCHK(c, snap_copy(&n.fset, c->fset, (size_t)c->rows * c->p.width, s));
    if (c->fstamp) HIPCHK(c, snap_copy(&n.fstamp, c->fstamp, (size_t)c->rows * c->p.width, s));
    n.has_running = c->running != nullptr;
    if (c->running) HIPCHK(c, snap_copy(&n.running, c->running, c->n_pad, s));
    snapshot_scalars(c);
    return ADDER_OK;
}
// Can the batch keep its own undo copy (Snapshot::lean2)?  Its plan starts with adder_lp_kernel, and the context holds none
// of the planes take_snapshot copies besides the slab: no per-unit c_thresh, no feature set, no running intensities, no
// Continuous arena (the packed kernel's regime has no deep level to keep).
static bool lean2_possible(const AdderHipCtx *c, uint32_t variant) {
    return variant_frame_kernel(variant) == ADDER_KERNEL_LEAN_RUNS_PACKED && !c->continuous && !c->perpx && !c->fset && !c->running;
}
// ... then nothing is queued: the copy's planes only have to exist (laid out like state_slab; its header and delta_t
// planes are the ones written, snap_plane)
static int take_snapshot_lean2(AdderHipCtx *c, float time_spanned) {
    AdderHipCtx::Snapshot &n = c->snap;
    if (!n.slab) HIPCHK(c, dalloc(&n.slab, c->slab_bytes));
    n.lean2 = true;
    n.time_spanned = time_spanned;
    n.deep = n.perpx = n.has_running = false;
    snapshot_scalars(c);
    return ADDER_OK;
}
// the undo copy's counterpart of a plane of state_slab
template <class T>
static T *snap_plane(const AdderHipCtx *c, const T *plane) {
    return reinterpret_cast<T *>(c->snap.slab + (reinterpret_cast<const uint8_t *>(plane) - c->state_slab));
}
// Rolls a lean2 copy back: the two planes the batch's first launch kept -> the four resident planes (adder_lp_restore_kernel).
// last_fired_t is as it was (adder_lp_kernel does not touch it in DeltaT); the run report was cleared behind the batch.
// (A batch whose first launch raises kStatusLeanRuns never gets here -- only a pure capacity status is rolled back; the
// planes it refused are the very planes it copied, untouched.)
static int restore_snapshot_lean2(AdderHipCtx *c, hipStream_t s) {
    HIPCHK(c, adder_launch_lp_restore(snap_plane(c, c->hdr), snap_plane(c, c->dt0), c->hdr, c->integ0, c->dt0, c->bdt0,
                                      (uint32_t)c->n_pad, c->snap.time_spanned, s));
    return ADDER_OK;
}
int restore_snapshot(AdderHipCtx *c, hipStream_t s) {
    AdderHipCtx::Snapshot &n = c->snap;
    if (n.lean2) {
        ADDER_TRY(restore_snapshot_lean2(c, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->state_slab, n.slab, c->slab_bytes, hipMemcpyDeviceToDevice, s));
    }
    if (!n.lean2 && c->continuous) {
        const size_t cnt = c->n_pad * (c->max_depth + 1u);
        HIPCHK(c, hipMemcpyAsync(c->cn_integ, n.cn_integ, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->cn_dt, n.cn_dt, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->cn_bdt, n.cn_bdt, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->cn_meta, n.cn_meta, cnt * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    }
    if (n.deep) {
        const size_t cnt = c->n_pad * (std::max<uint32_t>(c->max_depth, 2u) - 1u);
        HIPCHK(c, hipMemcpyAsync(c->dv_integ, n.dv_integ, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->dv_dt, n.dv_dt, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->dv_bdt, n.dv_bdt, cnt * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->dv_bd, n.dv_bd, cnt, hipMemcpyDeviceToDevice, s));
    }
    if (n.perpx) {
        HIPCHK(c, hipMemcpyAsync(c->cth_px, n.cth_px, c->n_pad, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->cctr_px, n.cctr_px, c->n_pad, hipMemcpyDeviceToDevice, s));
    }
    if (!n.lean2 && c->fset && n.fset) HIPCHK(c, hipMemcpyAsync(c->fset, n.fset, (size_t)c->rows * c->p.width, hipMemcpyDeviceToDevice, s));
    // (the display's Instant mode reads the stamps alone: none may stay above the restored frames_done)
    if (!n.lean2 && c->fstamp && n.fstamp)
        HIPCHK(c, hipMemcpyAsync(c->fstamp, n.fstamp, (size_t)c->rows * c->p.width * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    c->perpx = n.perpx;
    if (c->running && n.has_running) HIPCHK(c, hipMemcpyAsync(c->running, n.running, c->n_pad, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->status, 0, sizeof(uint32_t), s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->running_t = n.running_t;
    c->c_thresh = n.c_thresh;
    c->c_counter = n.c_counter;
    c->frames_done = n.frames_done;
    c->run_bound = n.run_bound;
    c->pending_reports = false;
    c->generic_sticky = n.generic_sticky;
    n.valid = false;
    return ADDER_OK;
}

// the lean-runs expansion's tables for this time step (cr_valid: one time step per reset, so once per stream)
int ensure_lr_tab(AdderHipCtx *c, float time_spanned, hipStream_t stream) {
    if (c->d_lr_tab && c->lr_tab_time == time_spanned) return ADDER_OK;
    std::vector<uint32_t> tab(kLrTabWords);
    lr_build_tab(tab.data(), time_spanned);
    if (!c->d_lr_tab) HIPCHK(c, dalloc(&c->d_lr_tab, tab.size()));
    HIPCHK(c, hipStreamSynchronize(stream));  // (an expansion of the batch before may still read the old one)
    HIPCHK(c, hipMemcpy(c->d_lr_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->lr_tab_time = time_spanned;
    return ADDER_OK;
}

// Queues the request's frames on its stream.  What it reads of the context is the pixel state's bookkeeping and the
// context's settings; the batch's mode and its description come with the request.  A failure leaves the context as far
// as it got (the caller poisons it): a refused plan has already updated cr_valid, cr_time and frac_time_seen.
int enqueue_frames(AdderHipCtx *c, const BatchRequest &rq, BatchQueued *done) {
    const uint32_t num_frames = rq.num_frames;
    const float time_spanned = rq.time_spanned;
    const size_t out_cap = rq.out_cap;
    hipStream_t const stream = rq.stream;
    BatchDesc &desc = *rq.desc;
    // Only the context's own description can reach the cached graphs (they hold its address): a frame slot's never does.
    const bool own = rq.desc == &c->own;
    *done = BatchQueued{};
    if (c->reset_pending) {  // adder_hip_reset queued its memsets on the context's stream
        HIPCHK(c, hipStreamWaitEvent(stream, c->reset_e, 0));
        c->reset_pending = false;
    }
    ADDER_TRY(join_ri_copy(c, stream));
    if (c->sparse_mode)
        return fail(c, ADDER_E_BAD_PARAMS, "dense frames after sparse steps: the pixels' c_thresh and running_t have "
                    "diverged (pass every pixel as a sparse step, or adder_hip_reset)");
    const bool sticky_before = c->generic_sticky;
    const bool fpath = feature_path(c);
    if (fpath) {  // the corner test reads the running intensities (video.rs:736-744)
        c->running_enabled = true;
        ADDER_TRY(prepare_feature_set(c, &desc, stream));
    }
    BatchPlanIn in = plan_input(c, num_frames, time_spanned, rq.wire, rq.records_only);
    // (read per batch: the tests switch kernels inside one process)
    in.no_lp = env_flag("ADDER_HIP_NO_LP"); in.no_lr = env_flag("ADDER_HIP_NO_LR");
    in.no_rr = env_flag("ADDER_HIP_NO_RR"); in.no_cr = env_flag("ADDER_HIP_NO_CR");
    const BatchPlan plan = plan_batch(in);
    const uint32_t variant = plan.variant;
    const bool generic = variant & kVarGeneric, lr = variant & kVarLeanRuns, rr = variant & kVarRunRecords;
    c->frac_time_seen = plan.frac_time_seen; c->cr_valid = plan.cr_valid; c->cr_time = plan.cr_time;
    c->last_variant = done->variant = variant;
    if (plan.refused) return fail(c, ADDER_E_BAD_PARAMS, "%s", plan.refused);
    if (lr) ADDER_TRY(ensure_lr_tab(c, time_spanned, stream));
    if (rr && !c->d_rr_tab) {  // (does not depend on the time step: a node's last firing is ceil(2^e / I))
        std::vector<uint8_t> tab(256u * kRrTabRows);
        rr_build_tab(tab.data(), 255.0f);
        HIPCHK(c, dalloc(&c->d_rr_tab, tab.size()));
        HIPCHK(c, hipMemcpy(c->d_rr_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    }
    if (plan.scratch != kScratchNone) {
        ADDER_TRY(alloc_scratch(c, plan.scratch));
        if (generic) ADDER_TRY(alloc_deep_planes(c));
    }
    c->generic_sticky = plan.generic_sticky;
    if (c->running_enabled && !c->running) {
        ADDER_TRY(alloc_running(c, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    // an event buffer below the batch's worst case can overflow: keep an undo copy of the state so that the
    // overflow is recoverable (adder_hip_finish rolls back and reports the size needed)
    c->snap.valid = false;
    if (out_cap < worst_case_events_per_frame(in) * num_frames && rq.allow_undo) {
        ADDER_TRY(lean2_possible(c, variant) ? take_snapshot_lean2(c, time_spanned) : take_snapshot(c, generic, stream));
        c->snap.generic_sticky = sticky_before;
    }
    if (fpath) ADDER_TRY(prepare_per_unit_c_thresh(c, stream));

    // ---- batch description -> device ----
    if (desc.ftab_cap < num_frames) {
        // A frame slot's table has its fixed entries (the ring queues one frame at a time); the context's own grows, and
        // the captured graphs, which hold the description's address, go
        if (!own)
            return fail(c, ADDER_E_HIP, "internal error: %u frames for a frame slot's table of %zu entries", num_frames, desc.ftab_cap);
        retire_graphs(c);
        ADDER_TRY(alloc_batch_desc(c, &desc, std::max<size_t>(num_frames, 2 * desc.ftab_cap)));
    }
    float rt = c->running_t;
    uint8_t cth = c->c_thresh, cctr = c->c_counter;
    for (uint32_t f = 0; f < num_frames; ++f) {
        desc.h_ftab[f].running_t = rt;
        desc.h_ftab[f].cth = cth;  // the contrast test of frame f sees the value before its integrate
        rt += time_spanned;        // `self.running_t += time` (event_pixel_tree.rs:336), f32
        c_thresh_advance(cth, cctr, c->p.c_thresh_max, c->p.c_increase_velocity, time_spanned, c->p.ref_time);
    }
    BatchArgs &b = *desc.h_batch;
    base_args(c, &b.base);
    b.base.out = reinterpret_cast<AdderEventPod *>(rq.d_out);
    b.base.out_cap = out_cap;
    b.base.frame_offsets = rq.d_offsets;
    b.base.lean = plan.lean;
    b.base.abs_t = c->p.time_mode == ADDER_TIME_ABSOLUTE_T ? 1u : 0u;
    b.base.wire_rec = rq.wire ? wire_record_bytes(c) : 0u;
    b.base.sc = make_consts(c, time_spanned);
    b.frames = rq.d_frames;
    b.ftab = desc.d_ftab;
    b.park_ring = c->park_ring;
    // run records: a fixed slot per (segment, frame) like the lean records' (at most one 8 / 12-byte record per unit and
    // frame), laid out by park_offset inside the log ring (2 KB per segment and frame there: enough) -- the expansion
    // reads the sixteen segments of a wave out of one contiguous stretch instead of sixteen logs 64 KB apart
    const uint32_t pb = rr ? kWaveUnits * (c->p.time_mode == ADDER_TIME_ABSOLUTE_T ? 12u : 8u) : c->park_bytes;
    b.park_bytes = pb;
    // (a lean batch's region holds one record per unit and frame of the chunk: the same bytes as its fixed slots)
    b.log_cap = rr ? 0u : (variant & kVarLeanLog) ? kWaveUnits * c->chunk : c->log_cap;
    b.rr_tab = c->d_rr_tab;
    b.lr_tab = c->d_lr_tab;
    {
        const bool sd = c->snap.valid && c->snap.deep;  // this batch keeps an undo copy of the levels >= 1
        b.snap_dv_integ = sd ? c->snap.dv_integ : nullptr;
        b.snap_dv_dt = sd ? c->snap.dv_dt : nullptr;
        b.snap_dv_bdt = sd ? c->snap.dv_bdt : nullptr;
        b.snap_dv_bd = sd ? c->snap.dv_bd : nullptr;
        const bool s2 = c->snap.valid && c->snap.lean2;  // ... of the two planes the packed kernel's state lives in
        b.snap_hdr = s2 ? snap_plane(c, c->hdr) : nullptr;
        b.snap_dt = s2 ? snap_plane(c, c->dt0) : nullptr;
    }
    b.run_max = (lr || rr) ? c->d_run_max : nullptr;
    b.view = make_view(c);
    b.wofs_ring = c->wofs_ring;
    b.wcur = c->wcur;
    static_assert((1u << kParkGroupShift) % kExpandSegs == 0, "a group of segments must hold whole expansion waves");
    if (!batch_park_layout(b.log_cap, launch_depth(c), c->num_waves, c->chunk, pb, &b.park_layout))
        return fail(c, ADDER_E_HIP, "internal error: %u segments, %u frames of %u bytes: no group layout", c->num_waves, c->chunk, pb);
    b.wtot_ring = c->wtot_ring;
    b.wpref_ring = c->wpref_ring;
    b.ftot_ring = c->ftot_ring;
    if (rq.frame_only && desc.ring_slot != 0u) {
        // the per-frame ring: a one-frame batch always sits in scratch slot 0 -- each frame slot of the ring gets a ring
        // CHUNK of its own as "its" scratch (views of the rings shifted by whole chunks), so that the scan and expansion of
        // frame k may run beside the frame kernel of frame k + 1
        const uint32_t rk = (desc.ring_slot - 1u) % c->ring_chunks;
        b.park_ring += (size_t)rk * scratch_bytes_per_chunk(c, c->scratch_kind, c->chunk);
        const size_t rows = (size_t)rk * c->chunk * c->num_waves;
        b.wtot_ring += rows;
        b.wpref_ring += rows;
        if (b.wofs_ring) b.wofs_ring += rows;
        if (b.wcur) b.wcur += (size_t)rk * c->num_waves;
        b.ftot_ring += (size_t)rk * c->chunk;  // (its second half and the tile sums move along: still inside the allocation)
    }
    b.slots = c->slots;
    b.chunk = c->chunk;
    b.rec_total = c->d_rec_total;
    b.timeline = nullptr;
    if (getenv("ADDER_HIP_TIMELINE")) {  // diagnostics (adder_hip_debug_timeline)
        if (!c->d_timeline) HIPCHK(c, dalloc(&c->d_timeline, 4 * kTimelineChunks * 2));
        std::vector<unsigned long long> init(4 * kTimelineChunks * 2);
        for (size_t i = 0; i < init.size(); ++i) init[i] = (i & 1) ? 0ull : ~0ull;
        HIPCHK(c, hipMemcpy(c->d_timeline, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
        b.timeline = c->d_timeline;
    }
    // (frame_offsets[0] and the record count are started by the first chunk's offsets kernel: nothing to clear here)
    // (description and table are one block on either side, the context's and a slot's alike: alloc_batch_desc)
    HIPCHK(c, hipMemcpyAsync(desc.d_batch, desc.h_batch, kBatchDescBytes + num_frames * sizeof(FrameTab), hipMemcpyHostToDevice,
                             stream));

    c->timed_launches = 0;
    c->timed_pairs = 0;
    c->timed_frames = 0;
    c->timed_posts = 0;
    const bool timing = c->launch_timing != 0;
    if (timing) {
        while (c->launch_events.size() < 2 * (size_t)num_frames) {
            hipEvent_t e;
            HIPCHK(c, hipEventCreate(&e));
            c->launch_events.push_back(e);
        }
        while (c->post_events.size() < 2 * (size_t)num_frames) {
            hipEvent_t e;
            HIPCHK(c, hipEventCreate(&e));
            c->post_events.push_back(e);
        }
    }
    c->h_result->valid = 0u;
    HIPCHK(c, hipEventRecord(c->ev_start, stream));
    int rc = ADDER_OK;
    if (rq.frame_only && num_frames == 1u && !fpath && !timing && !rq.records_only) {
        // the per-frame ring: only the frame kernel goes on this stream -- the NEXT frame's kernel needs nothing else of
        // this frame, so the ring puts scan, expansion and hand-over on its second stream, beside that kernel
        const Lean1wArgs wide = lean1w_args(c);
        HIPCHK(c, adder_launch_frame(desc.d_batch, 0u, 1u, variant, c->num_waves, 0u, stream, &wide));
        done->frame_only_done = true;
    } else if (rq.records_only) {
        rc = launch_frame_loop(c, rq, variant, stream, nullptr, false);  // (stops after scan + offsets)
    } else if (fpath) {
        rc = launch_feature_loop(c, rq, variant, stream);
    } else if (own && c->use_graph && !timing) {
        hipGraphExec_t exec = nullptr;
        rc = get_graph(c, rq, variant, &exec);
        if (rc == ADDER_OK) HIPCHK(c, hipGraphLaunch(exec, stream));
    } else if (c->eager_two_streams && !timing) {
        // the graph's two-stream structure, submitted eagerly (diagnostics)
        HIPCHK(c, hipEventRecord(c->cap_e1, stream));
        HIPCHK(c, hipStreamWaitEvent(c->cap_s, c->cap_e1, 0));
        rc = launch_frame_loop(c, rq, variant, c->cap_s, c->cap_s2, false);
        if (rc == ADDER_OK) {
            HIPCHK(c, hipEventRecord(c->cap_e1, c->cap_s));
            HIPCHK(c, hipStreamWaitEvent(stream, c->cap_e1, 0));
        }
    } else {
        rc = launch_frame_loop(c, rq, variant, stream, nullptr, timing);
    }
    if (rc != ADDER_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev_stop, stream));
    c->running_t = rt;
    c->c_thresh = cth;
    c->c_counter = cctr;
    c->last_time_spanned = time_spanned;
    c->frames_done += num_frames;
    c->run_bound += num_frames;  // (every unit may have gone on accumulating; adder_hip_finish takes the kernels' report)
    c->pending_end_frames = c->frames_done;
    c->pending_reports = b.run_max != nullptr;
    c->band_frame_pending = band_features(c);
    return ADDER_OK;
}
