// adder_hip_graphs.cpp -- the cache of captured batches (AdderHipCtx::graphs): capture, instantiation and the key.  Which
// instance runs a batch, who is chosen and who is retired is decided in adder_graph_tune.hpp.
//
// Retired instances (tuning losers, evicted batch lengths) are destroyed with the context, never mid-life: this HIP
// runtime (ROCm 7.0) crashed in hip::Graph::UpdateStreams at a later hipGraphLaunch of ANOTHER instance once a few dozen
// instances had been destroyed mid-life (AdderHipCtx::retired_execs).
#include <stdio.h>

#include "adder_hip_ctx.hpp"

// every cached graph goes: something all of them bake in has changed (the chunking, the description's address)
void retire_graphs(AdderHipCtx *c) { tune_retire_all(c->graphs, &c->retired_execs); }

static int instantiate_graph(AdderHipCtx *c, const BatchRequest &rq, uint32_t variant, bool one_stream, hipGraphExec_t *out) {
    hipGraph_t graph = nullptr;
    HIPCHK(c, hipStreamBeginCapture(c->cap_s, hipStreamCaptureModeThreadLocal));
    // per-event-record batches (generic / bounded Collapse kernels) are captured on ONE stream: their frame kernel is
    // bound by instruction issue at full occupancy and leaves the expansion no room to run beside it -- two branches
    // measured 10.5 us per 1080p frame against 10.0 in sequence (walking grids 11.6 - 14.2)
    hipStream_t s2 = (one_stream || (variant & kVarGeneric)) ? nullptr : c->cap_s2;
    int rc = launch_frame_loop(c, rq, variant, c->cap_s, s2, false);
    hipError_t e = hipStreamEndCapture(c->cap_s, &graph);
    if (rc != ADDER_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    HIPCHK(c, e);
    e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    HIPCHK(c, e);
    return ADDER_OK;
}

// The captured launch sequence of the request, for the context's OWN description: a graph holds the address of the
// description it was captured with, and enqueue_frames comes here for no other (a frame slot's batch is launched
// eagerly).  So the description is no part of the key, and two descriptions cannot share one: there is only the one, and
// when its blocks are reallocated every graph is retired (retire_graphs).
int get_graph(AdderHipCtx *c, const BatchRequest &rq, uint32_t variant, hipGraphExec_t *out) {
    const uint32_t num_frames = rq.num_frames;
    if (rq.desc != &c->own) return fail(c, ADDER_E_HIP, "internal error: a captured batch with a frame slot's description");
    // everything else the captured launch sequence depends on
    // (running_enabled decides the launches' lazy bits, variant_lazy_state_bit)
    // (the first launch's kVarKeepUndo: a batch that keeps a two-plane undo copy and one that needs none are two sequences)
    // (bits: frames 0-23, variant 24-39, launch depth 40-47, running 48)
    const uint32_t key_variant = variant | variant_keep_undo_bit(variant, true, c->snap.valid && c->snap.lean2);
    const uint64_t key = (uint64_t)(num_frames & 0xffffffu) | ((uint64_t)(key_variant & kVarKeyMask) << 24) | ((uint64_t)(launch_depth(c) & 0xffu) << 40) |
                         ((uint64_t)(c->running_enabled ? 1u : 0u) << 48);
    bool one_stream = false;
    int use = tune_pick(c->graphs, key, variant_graph_candidates(variant, num_frames, c->chunk, c->graph_candidates), &one_stream,
                        &c->retired_execs);
    if (use < 0) {
        // the first candidate runs the chunks' kernels one after the other, the others on two branches (the frame
        // kernel of chunk k + 1 beside the scan / expansion of chunk k): with both big kernels bound by instruction
        // issue the branches only get in each other's way on a full 1080p plane (1.335 against 1.284 ms per step,
        // medians of six processes each), on small or quiet planes they hide the short kernels' launch gaps -- the
        // measured batch times decide
        hipGraphExec_t exec = nullptr;
        ADDER_TRY(instantiate_graph(c, rq, variant, one_stream, &exec));
        use = tune_add(c->graphs, key, exec);
    }
    *out = static_cast<hipGraphExec_t>(c->graphs.keys[key].cand[use]);
    return ADDER_OK;
}

// the batch queued last has finished in `ms` (of interest while its graph is still being chosen)
void graph_tune_report(AdderHipCtx *c, float ms) {
    const GraphTune *g = tune_report(c->graphs, ms, &c->retired_execs);
    if (g && getenv("ADDER_HIP_DEBUG_TUNE")) {
        fprintf(stderr, "[adder_hip] graph candidates (ms):");
        for (float v : g->ms) fprintf(stderr, " %.3f", v);
        fprintf(stderr, " -> %d\n", g->chosen);
    }
}

extern "C" int adder_hip_launch_plan_settled(const AdderHipCtx *c) { return !c || tune_settled(c->graphs) ? 1 : 0; }
