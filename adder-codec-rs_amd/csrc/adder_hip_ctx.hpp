// adder_hip_ctx.hpp -- the context behind include/adder_hip.h and what the adder_hip_*.cpp files share of it.
//
//   adder_hip_api.cpp           create / destroy / reset / setters and getters, the integrate_* entry points, finish,
//                               the host-buffer calls
//   adder_hip_batch.cpp         one batch from its request to its launches: plan input, scratch, the launch loops, the undo
//                               copy, enqueue_frames
//   adder_hip_graphs.cpp        the cache of captured batches: capture, instantiate, launch (the tuner's decisions are
//                               adder_graph_tune.hpp, without HIP)
//   adder_hip_ring_api.cpp      adder_hip_stream_* and the per-frame ring
//   adder_hip_records_api.cpp   records over the wire, wire serialisation, sink layout, merge
//   adder_hip_features_api.cpp  feature mode / ROI / halos, running intensities, the live view
//   adder_hip_sparse_api.cpp    sparse steps
//
// A batch's mode travels as an argument (BatchRequest -> enqueue_frames -> BatchQueued), never as a field set on the
// context around a call: what a helper reads of the context is the context's, whoever called it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/adder_hip.h"
#include "adder_batch_plan.hpp"
#include "adder_graph_tune.hpp"
#include "adder_kernels.h"

using namespace adder;

// A device-resident batch description (kernels take {BatchArgs*, f}) with its page-locked host mirror: BatchArgs, then
// (kBatchDescBytes on) the per-frame uniforms, in ONE device block and ONE host block -- one upload per batch
// (alloc_batch_desc).  The context has one; every frame slot of the per-frame ring has its own, because the copy engine
// may still be reading the host side of the frame before.
struct BatchDesc {
    BatchArgs *d_batch = nullptr, *h_batch = nullptr;  // (the blocks' base addresses)
    FrameTab *d_ftab = nullptr, *h_ftab = nullptr;     // (running_t, c_thresh) per frame
    size_t ftab_cap = 0;                               // entries
    uint32_t *feat_counters = nullptr;                 // feature path: the batch's counters (cleared per enqueue)
    uint32_t ring_slot = 0;                            // 1 + the frame slot that owns it (0: the context's own)
};

struct AdderHipCtx {
    AdderHipParams p{};
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t rows = 0, n_units = 0, num_tiles = 0, num_chunks = 0, grid = 0, num_cus = 0;
    size_t n_pad = 0;
    uint32_t max_depth = 0;
    // state planes: level 0 = {hdr, integ0, dt0, bdt0}; levels >= 1 in the deep planes (allocated by the
    // first generic batch: the lean variants never touch them)
    uint32_t *hdr = nullptr;
    float *integ0 = nullptr, *dt0 = nullptr, *bdt0 = nullptr;
    float *lastf = nullptr;
    float *dv_integ = nullptr, *dv_dt = nullptr, *dv_bdt = nullptr;
    uint8_t *dv_bd = nullptr;
    // Mode::Continuous contexts: node planes of the general arena ([max_depth + 1][n_pad]); hdr holds the arena header
    bool continuous = false;
    float *cn_integ = nullptr, *cn_dt = nullptr, *cn_bdt = nullptr;
    uint32_t *cn_meta = nullptr;
    uint8_t *state_slab = nullptr;  // hdr, lastf, status + d_run_max, integ0, dt0, bdt0 live in here
    size_t reset_bytes = 0;         // hdr .. the status block: one memset per reset
    size_t slab_bytes = 0;
    uint8_t *running = nullptr;       // the context's own rows, inside running_base
    uint8_t *running_base = nullptr;  // kFeatureHalo rows of the band above + the own rows (n_pad) + kFeatureHalo rows below
    bool running_enabled = false;
    uint32_t *d_new_xy = nullptr;     // row-band feature mode: this frame's new features (x | plane y << 16)
    uint32_t new_xy_cap = 0;
    bool band_frame_pending = false;  // a frame's events await adder_hip_feature_detect
    // undo copy of the pixel state, taken before a batch whose event buffer is smaller than the batch's worst
    // case: an overflow then rolls the state back and the caller retries with the size reported
    struct Snapshot {
        uint8_t *slab = nullptr;  // copy of state_slab
        float *dv_integ = nullptr, *dv_dt = nullptr, *dv_bdt = nullptr;
        uint8_t *dv_bd = nullptr;
        float *cn_integ = nullptr, *cn_dt = nullptr, *cn_bdt = nullptr;
        uint32_t *cn_meta = nullptr;
        bool valid = false, deep = false;
        // "lean2": only the header and delta_t planes of `slab` are valid, and the batch's first adder_lp_kernel launch
        // writes them (BatchArgs::snap_hdr / snap_dt) -- no copy is queued in front of the batch.  In the lean-runs regime
        // the other two level-0 planes follow from those two (lr_pack of lr_unpack: adder_lp_restore_kernel), and the
        // packed kernel writes nothing else: not last_fired_t, not a deep level, no per-unit c_thresh or feature plane.
        bool lean2 = false;
        float time_spanned = 0.0f;  // of the batch (lean2: the restore kernel's time step)
        float running_t = 0.0f;
        uint8_t c_thresh = 0, c_counter = 0;
        uint64_t frames_done = 0, run_bound = 0;
        bool generic_sticky = false;
        uint8_t *cth_px = nullptr, *cctr_px = nullptr, *fset = nullptr, *running = nullptr;
        uint32_t *fstamp = nullptr;  // beside fset: a refused batch's stamps lie above the restored frames_done
        bool perpx = false, has_running = false;
    } snap;
    // feature-driven rate control + ROI (video.rs:825-837, 865-1112, 1291-1293)
    bool feat_detect = false, feat_adjust = false;
    uint8_t c_thresh_baseline = 2;   // Crf::new(None): CRF[3][0] (rate_controller.rs:21,62)
    uint16_t feature_c_radius = 0;   // CRF[3][3] * min_resolution, set in create
    bool roi_on = false;
    uint16_t roi[4] = {0, 0, 0, 0};  // start.x, start.y, end.x, end.y (inclusive)
    uint8_t *cth_px = nullptr, *cctr_px = nullptr;  // per-unit pair once it stops being uniform (perpx)
    uint8_t *fset = nullptr;         // [rows][width] VideoState::features membership
    uint32_t last_new_features = 0;
    // the live view (Video::instantaneous_view_mode, video.rs:331; display_frame_features, :328)
    uint32_t view_mode = 0;          // ADDER_VIEW_*: what the running-intensities plane shows
    float practical_d_max = 0.0f;    // D view: the caller's value; <= 0: exact log2 of 255 * (delta_t_max / ref_time)
    uint32_t show_features = 0;      // ShowFeatureMode: 0 Off, 1 Instant, 2 Hold
    uint8_t *d_display = nullptr;    // staging of adder_hip_display_frame
    size_t d_display_cap = 0;
    uint32_t *fstamp = nullptr;      // [rows][width] frame (frames_done + 1 of its batch) in which the pixel last became a feature
    bool perpx = false;              // sticky until adder_hip_reset / reset_c_thresh
    // c_thresh / c_increase_counter: identical in every pixel (adder_pixel.hpp header comment)
    uint8_t c_thresh = 10, c_counter = 1;
    // a generic batch has run since create / reset: pixels may hold more than one fired level, which only
    // the generic kernels understand -- the lean variant is not chosen again until adder_hip_reset
    bool generic_sticky = false;
    // ordered-compaction scratch: a ring of two chunks of frames (a chunk is stepped while the one before
    // it is scanned and expanded)
    uint8_t *park_ring = nullptr;    // [slots][num_waves][park_bytes]
    // graph instances no longer wanted (tuning losers, evicted batch lengths): destroyed with the context.  This HIP
    // runtime (ROCm 7.0) crashed in hip::Graph::UpdateStreams at a later hipGraphLaunch of ANOTHER instance once a
    // few dozen instances had been destroyed mid-life (rocgdb backtrace; tests: 22 batch lengths on one context).
    std::vector<GraphHandle> retired_execs;  // (hipGraphExec_t)
    uint32_t park_bytes = 0;         // scratch of one segment of one frame (fixed-slot kinds)
    ScratchKind scratch_kind = kScratchNone;  // what the scratch ring is laid out for (adder_batch_plan.hpp)
    uint32_t log_cap = 0;            // records per (segment, chunk) region (log kinds)
    uint32_t *wofs_ring = nullptr;   // [slots][num_waves] log kinds: where a segment's run of a frame starts
    uint32_t *wcur = nullptr;        // [ring_chunks][num_waves] log cursors between the launches of a chunk
    // the bounded Collapse step needs exact integer sums (adder_pixel.hpp): a fractional time_spanned or a huge
    // delta_t_max since the last reset rules it out
    bool frac_time_seen = false;
    uint32_t dtm_max_seen = 0;
    // constant runs (adder_cr_kernel): every dense frame since the last reset was tested with c_thresh 0 at ONE integer
    // time_spanned, so every arena is a function of (its run's intensity, the run's length) -- adder_pixel.hpp
    bool cr_valid = true;
    float cr_time = 0.0f;
    // The integer-state kernels need rho * max(255, time_spanned) < 2^24 for every run length rho.  run_bound = an upper bound
    // of any unit's run: it grows by every frame queued and comes down to what the kernels REPORT at the end of a batch
    // (BatchResult::max_run) -- so a stream whose pixels keep changing stays on the integer kernels for good, where "frames
    // since the reset" sent every stream to the float kernels after 65 793 frames (18 minutes of video)
    uint64_t run_bound = 0, pending_end_frames = 0;
    bool pending_reports = false;
    hipEvent_t null_join = nullptr;  // stream == NULL: the batch is ordered behind the legacy default stream (join_null_stream)
    uint32_t *d_run_max = nullptr;   // (in the status block of state_slab, a cache line behind the status word: cleared by the reset's one fill)
    uint32_t *wtot_ring = nullptr;   // [slots][num_waves]
    uint32_t *wpref_ring = nullptr;  // [slots][num_waves]
    uint32_t *ftot_ring = nullptr;   // [slots]
    uint32_t chunk = 1, slots = 2;
    static constexpr uint32_t ring_chunks = 3;  // a chunk being stepped, one being scanned / expanded, one of slack between the two streams
    uint32_t lean_blocks_per_cu = 0, expand_blocks_per_cu = 0;  // walking grids of the lean path when > 0 (0 = full grids)
    uint32_t frames_per_launch = kMaxFramesPerLaunch;  // temporal blocking depth of the frame kernels
    uint32_t num_waves = 0;
    BatchDesc own;                    // the context's own batch description: every batch but the per-frame ring's
    BatchResult *h_result = nullptr;  // pinned: adder_publish_kernel writes it, finish() reads it
    hipEvent_t reset_e = nullptr;     // adder_hip_reset's memsets (queued on the context's stream, not waited for)
    bool reset_pending = false;
    // adder_hip_running_intensities_device's copy of the plane, on the caller's stream: what writes the plane next waits
    hipEvent_t ri_copy_e = nullptr, ri_src_e = nullptr;
    bool ri_copy_pending = false;
    // capture streams/events and the cache of instantiated frame-loop graphs
    hipStream_t cap_s = nullptr, cap_s2 = nullptr;
    hipEvent_t cap_e1 = nullptr, cap_e2[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    GraphCache graphs;  // hipGraphExec_t per key (get_graph) and candidate; which one runs: adder_graph_tune.hpp
    uint32_t graph_candidates = 6;
    bool use_graph = true;
    bool eager_two_streams = false;
    uint32_t *status = nullptr;   // device status word
    uint64_t *d_rec_total = nullptr;  // parked records of the last batch (diagnostics)
    // [0]: adder_log_pack_kernel's total (written, never read back); [1] (as u32): the status word of
    // adder_hip_expand_records_device's kernels -- they run on a side stream beside root's own batches, so they must not
    // share the batches' word (a capacity flag of theirs would be charged to an unrelated batch, and clearing theirs
    // could erase a flag a batch in flight raised)
    uint64_t *d_side_words = nullptr;
    uint8_t *d_rr_tab = nullptr;  // [256][kRrTabRows] chain lengths of the run-records step (built at its first batch)
    uint32_t *d_lr_tab = nullptr; // [kLrTabWords] the lean-runs expansion's events by (base_val, rho) / input, for lr_tab_time
    float lr_tab_time = 0.0f;
    // records over the wire (adder_hip_integrate_records_device / adder_hip_expand_records_device)
    uint32_t last_variant = 0;        // kernel choice of the batch queued last (enqueue_frames)
    float last_time_spanned = 0.0f;   // of the last batch (root's expansion uses its consts and frame table)
    // root: n_bands BatchArgs + pointer / destination tables per call, kBandDescSlots calls' worth in turn (a slot's
    // host block is reused once the upload queued from it has gone through: no wait for the stream's other work)
    static constexpr uint32_t kBandDescSlots = 4;
    uint8_t *d_band_desc = nullptr, *h_band_desc = nullptr;
    size_t band_desc_cap = 0;  // bytes of ONE slot
    uint32_t band_desc_next = 0;
    hipEvent_t band_desc_e[kBandDescSlots] = {nullptr, nullptr, nullptr, nullptr};
    unsigned long long *d_timeline = nullptr;  // ADDER_HIP_TIMELINE diagnostics
    // sparse steps (adder_hip_integrate_sparse): running_t per unit, and the work buffers of a call
    bool sparse_mode = false;  // c_thresh / counter / running_t live per unit from the first sparse call on
    float *rt_px = nullptr;
    struct SparseWork {
        SparseStep *steps = nullptr;
        uint32_t *keys0 = nullptr, *keys1 = nullptr, *idx0 = nullptr, *idx1 = nullptr, *count = nullptr, *offs = nullptr;
        uint2 *stage = nullptr;
        void *temp = nullptr;
        unsigned long long *total = nullptr;
        size_t cap = 0, temp_bytes = 0;  // steps
    } sw;
    uint64_t last_records = 0;
    std::vector<hipEvent_t> post_events;  // launch timing: pairs around scan + offsets + expand of every chunk
    uint32_t timed_posts = 0;
    float last_post_avg_us = 0.0f;
    uint64_t *d_offsets = nullptr;  // internal frame offsets (host-buffer API)
    size_t d_offsets_cap = 0;       // all *_cap below are in BYTES
    // staging for the host-buffer API
    uint8_t *d_frames = nullptr;    // ... and the gray form of a colour batch (the *_rgb entry points, device and host)
    size_t d_frames_cap = 0;
    uint8_t *d_rgb = nullptr;       // adder_hip_integrate_batch_rgb: the colour frames as they were uploaded
    size_t d_rgb_cap = 0;
    AdderEvent *d_events = nullptr;
    size_t d_events_cap = 0;
    uint8_t *d_wire = nullptr;      // wire-format bytes of the last raw batch
    size_t d_wire_cap = 0;
    // pipelined raw transcode (adder_hip_stream_*): two slots, each one batch in flight
    struct StreamSlot {
        uint8_t *d_wire = nullptr;
        size_t d_wire_cap = 0;
        uint8_t *h_wire = nullptr;   // pinned
        size_t h_wire_cap = 0;
        uint64_t *h_offsets = nullptr;  // pinned, [T+1]
        size_t h_offsets_cap = 0;
        hipEvent_t done = nullptr;   // wire kernel + D2H of this slot
        hipEvent_t wired = nullptr;  // wire kernel only (d_events may be overwritten after it)
        size_t n_events = 0, n_bytes = 0;
        uint32_t status = 0;
        bool busy = false;
    } slot[2];
    hipStream_t out_s = nullptr;     // wire + D2H stream of the pipeline
    uint64_t submitted = 0, collected = 0;
    // per-frame `consume` ring (adder_hip_frame_submit / _collect): every slot owns its frame, its events on
    // the device and in page-locked host memory, and its own batch description (the host-side copies are read
    // by the DMA engine after submit has returned)
    struct FrameSlot {
        uint8_t *d_frame = nullptr;
        uint8_t *d_rgb = nullptr;       // adder_hip_frame_submit_rgb: the colour frame, converted into d_frame on the upload stream
        AdderEvent *d_events = nullptr, *h_events = nullptr;
        size_t cap = 0;                 // events
        uint8_t *h_hdr = nullptr;       // pinned: FrameResult, then chunk offsets [num_chunks + 1]
        uint64_t *d_offsets = nullptr;  // [2]
        BatchDesc desc;                 // 64 table entries; feature path: this frame's counters (the context's are reset per enqueue)
        hipEvent_t done = nullptr;
        AdderEvent *out = nullptr;      // where the events were sent (h_events, or the caller's pinned buffer)
        size_t out_cap = 0;
        bool wire = false;              // the slot holds 9 / 11-byte wire records (the ring's format when it was submitted)
        hipGraphExec_t out_graph = nullptr;  // the slot's hand-over (wire scatter + frame_out) as ONE launch
        uint64_t out_key[6] = {0, 0, 0, 0, 0, 0};  // what that graph baked in
    } fslot[4];
    // The per-frame ring's stream arrangement is MEASURED, like the graph instances: where the HIP runtime puts a stream among
    // its hardware queues decides whether a dependency between two streams is cheap or costs tens of microseconds, and nothing
    // in the API tells (one process ran the default-quality ring at 60 us per frame, the next at 115; profiles/r05_ring_queues.txt).
    // Candidates: {second stream A, upload stream A}, {post-processing on the context's own stream, upload A}, and three more
    // pairs of streams; each gets a window of 24 frames, the fastest stays for the context's life.
    struct RingCand {
        hipStream_t out_s = nullptr, in_s = nullptr;  // (borrowed from ring_streams)
        bool post_on_main = false;
        double us = 1e30;  // measured period per frame
    };
    std::vector<RingCand> ring_cands;
    std::vector<hipStream_t> ring_streams;  // owned
    int ring_cur = 0, ring_chosen = -1;
    uint32_t ring_win_frames = 0, ring_win_waits = 0, ring_win_skip = 0;
    std::chrono::steady_clock::time_point ring_win_t0;
    uint32_t f_slots = 3;
    bool f_wire = false;             // the ring hands out 9 / 11-byte wire records instead of AdderEvents (adder_hip_frames_set_format)
    size_t f_events_per_slot = 0;    // 0: the mode's worst case, at most 2 GiB of events
    uint64_t f_submitted = 0, f_collected = 0;
    hipEvent_t frame_e = nullptr;
    hipStream_t in_s = nullptr;      // the ring's upload stream (wire format: the next frame's H2D beside this frame's kernels)
    uint64_t f_last_produced = 0;    // events of the frame collected last
    hipEvent_t in_e = nullptr;
    uint32_t *d_chunks = nullptr;
    // running state
    float running_t = 0.0f;  // PixelArena::running_t (identical for all pixels)
    uint64_t frames_done = 0;
    bool poisoned = false;
    std::string err;
    // pending device batch
    bool pending = false;
    hipStream_t pending_stream = nullptr;
    uint64_t *pending_offsets = nullptr;
    uint32_t pending_frames = 0;
    size_t pending_cap = 0;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    float last_ms = 0.0f;
    // optional per-launch timing (one HIP event pair around every frame launch)
    int launch_timing = 0;  // 1: a pair around every frame-kernel launch; 2: a pair around a chunk's run of them
    std::vector<hipEvent_t> launch_events;
    uint32_t timed_launches = 0, timed_frames = 0, timed_pairs = 0;
    float last_launch_avg_us = 0.0f;
};

// One batch, as its entry point asks for it: enqueue_frames reads the mode here and nowhere else.
struct BatchRequest {
    const uint8_t *d_frames = nullptr;
    uint32_t num_frames = 0;
    float time_spanned = 0.0f;
    AdderEvent *d_out = nullptr;     // (wire: the records' bytes)
    size_t out_cap = 0;              // events / records
    uint64_t *d_offsets = nullptr;
    hipStream_t stream = nullptr;
    bool wire = false;               // the expansion writes the raw sink's 9 / 11-byte records instead of AdderEvents
    bool records_only = false;       // the batch stops after its scan (adder_hip_integrate_records_device)
    bool allow_undo = true;          // an event buffer below the worst case gets an undo copy (false: nothing can overflow,
                                     // or -- the ring -- later frames are queued before the outcome is known)
    bool frame_only = false;         // a one-frame batch of the per-frame ring may stop after its frame kernel: the ring
                                     // queues scan and expansion itself, on another stream
    BatchDesc *desc = nullptr;       // the context's own, or a frame slot's
};
// ... and what enqueue_frames made of it
struct BatchQueued {
    uint32_t variant = 0;            // the kernel choice (also left in AdderHipCtx::last_variant)
    bool frame_only_done = false;    // only the frame kernel was queued (false: the whole pipeline -- feature mode, timing)
};

#pragma GCC visibility push(hidden)  // (what crosses the adder_hip_*.cpp files is not part of libadder_hip.so's ABI)
// adder_hip_api.cpp
int fail(AdderHipCtx *ctx, int code, const char *fmt, ...);
int refuse_poisoned(AdderHipCtx *c);  // ADDER_E_POISONED with the earlier failure's message
int status_to_code(AdderHipCtx *c, uint32_t st);
int join_null_stream(AdderHipCtx *c);
int rgb_precheck(AdderHipCtx *c);  // ADDER_E_BAD_PARAMS unless the context has one channel (the *_rgb entry points)
int ensure(AdderHipCtx *c, void **p, size_t *cap, size_t need);
int batch_to_device(AdderHipCtx *c, const uint8_t *frames, uint32_t num_frames, size_t frame_stride, size_t row_stride,
                    float time_spanned, size_t out_cap, size_t *total, bool rgb = false);
// adder_hip_batch.cpp
StepConsts make_consts(const AdderHipCtx *c, float time_spanned);
ViewConsts make_view(const AdderHipCtx *c);
void base_args(const AdderHipCtx *c, FrameArgs *a);
int alloc_batch_desc(AdderHipCtx *c, BatchDesc *d, size_t frames);
int alloc_scratch(AdderHipCtx *c, ScratchKind kind);
size_t worst_case_events_per_frame(const AdderHipCtx *c, float time_spanned);
int launch_frame_loop(AdderHipCtx *c, const BatchRequest &rq, uint32_t variant, hipStream_t s, hipStream_t s2, bool timing);
int ensure_lr_tab(AdderHipCtx *c, float time_spanned, hipStream_t stream);
int restore_snapshot(AdderHipCtx *c, hipStream_t s);
int enqueue_frames(AdderHipCtx *c, const BatchRequest &rq, BatchQueued *done);
// adder_hip_graphs.cpp
void retire_graphs(AdderHipCtx *c);
int get_graph(AdderHipCtx *c, const BatchRequest &rq, uint32_t variant, hipGraphExec_t *out);
void graph_tune_report(AdderHipCtx *c, float ms);
// adder_hip_features_api.cpp
int alloc_running(AdderHipCtx *c, hipStream_t s);
int join_ri_copy(AdderHipCtx *c, hipStream_t s);
FeatureArgs feature_args(const AdderHipCtx *c, const BatchDesc &desc);
// adder_hip_ring_api.cpp
int frame_submit_impl(AdderHipCtx *c, const uint8_t *frame, size_t row_stride, float time_spanned, AdderEvent *direct_out,
                      size_t direct_cap, bool rgb = false);
int frame_collect_impl(AdderHipCtx *c, const AdderEvent **events, size_t *n_events, const uint32_t **chunk_offsets);
#pragma GCC visibility pop

#define HIPCHK(ctx, expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, ADDER_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// returns a helper's code from the enclosing function unless it is ADDER_OK (the helper has set the message)
#define ADDER_TRY(expr)                  \
    do {                                 \
        const int rc_ = (expr);          \
        if (rc_ != ADDER_OK) return rc_; \
    } while (0)

template <class T>
static hipError_t dalloc(T **p, size_t count) {
    return hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T));
}

constexpr size_t kStatusBlockBytes = 256;  // the status word (+0) and d_run_max (+128) between the planes of state_slab
static size_t halo_bytes(const AdderHipCtx *c) { return (size_t)kFeatureHalo * c->p.width * c->p.channels; }

static bool env_flag(const char *name) {
    const char *e = getenv(name);
    return e && atoi(e) != 0;
}

// BatchArgs followed (256-byte aligned) by the frame table, on the device and in page-locked host memory
constexpr size_t kBatchDescBytes = (sizeof(BatchArgs) + 255) & ~(size_t)255;

static bool feature_path(const AdderHipCtx *c) { return c->feat_detect || c->roi_on; }
static bool feature_needs_perpx(const AdderHipCtx *c) {
    return c->roi_on || (c->feat_detect && c->feat_adjust && c->feature_c_radius > 0);
}
static bool is_band(const AdderHipCtx *c) { return c->p.row_begin != 0 || c->p.row_end != c->p.height; }
// A row-band context (multi-GPU) in feature mode cannot finish a frame on its own: the corner test reads the three
// rows beyond its band and the reset squares of its neighbours' new features reach into its rows.  It integrates ONE
// frame per call and leaves the feature step to adder_hip_feature_detect, between the halo exchanges (include/adder_hip.h).
static bool band_features(const AdderHipCtx *c) { return is_band(c) && (c->feat_detect || c->roi_on); }

static uint32_t launch_depth(const AdderHipCtx *c) { return c->running_enabled ? 1u : c->frames_per_launch; }

static uint32_t wire_record_bytes(const AdderHipCtx *c) { return c->p.channels == 1 ? 9u : 11u; }
