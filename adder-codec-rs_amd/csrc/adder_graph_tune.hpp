// adder_graph_tune.hpp -- which instance of a captured batch runs next: the decisions of the graph cache and its tuner,
// without HIP (tests/test_graph_tune.py drives them on the CPU through tests/cpu_sim/graph_tune.cpp).  Capture,
// instantiation and launch stay in adder_hip_graphs.cpp; an instance is an opaque handle here.
//
// How well the two branches of an instantiated graph overlap is decided when it is instantiated (the runtime binds the
// branches to hardware queues then; measured: the same graph comes out at 1.86 or 2.08 ms per 300-frame step from one
// instantiation to the next, stable for the life of the instance), so a key keeps a few candidates, runs each on real
// batches while it is new, and settles on the fastest.  The schedule for `want` candidates: candidate 0 twice, 1 twice,
// ..., want-1 twice, then candidate 0 twice more (it ran first, on a cold chip); a candidate's first run also uploads
// the instance and never counts.  2 * want + 2 batches pass before the choice (want == 1: two).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#pragma GCC visibility push(hidden)  // (internal to libadder_hip.so: none of this is part of its ABI)
namespace adder {

typedef void *GraphHandle;  // (a hipGraphExec_t to adder_hip_graphs.cpp)

constexpr int kTuneRunsPerCandidate = 2;  // the first run of an instance also uploads it
constexpr int kTuneRecheckRuns = 2;
// the one-stream instance keeps the batch unless a two-branch one beats it by more than the runs' own scatter
constexpr float kTuneTwoBranchGain = 0.985f;
constexpr size_t kGraphCacheKeys = 24;  // keep the cache small

struct GraphTune {
    std::vector<GraphHandle> cand;  // (null: retired after the choice)
    std::vector<float> ms;          // best batch time seen per candidate
    std::vector<int> runs;
    int chosen = -1;                // settled
    int last = -1;                  // candidate of the batch in flight
    int recheck = 0;                // extra runs of candidate 0 after the others
    uint32_t want = 1;              // candidates to try (variant_graph_candidates)
};

struct GraphCache {
    std::map<uint64_t, GraphTune> keys;
    uint64_t tune_key = 0;      // the key whose batch is in flight ...
    bool tune_pending = false;  // ... while it is still being chosen: its time is wanted (tune_report)
};

inline void tune_retire(const GraphTune &g, std::vector<GraphHandle> *retired) {
    for (GraphHandle e : g.cand)
        if (e) retired->push_back(e);
}

// every cached instance goes: something all of them bake in has changed
inline void tune_retire_all(GraphCache &gc, std::vector<GraphHandle> *retired) {
    for (auto &kv : gc.keys) tune_retire(kv.second, retired);
    gc.keys.clear();
    gc.tune_pending = false;
}

// The candidate that runs the batch of `key` now, or -1: the caller instantiates one more (*one_stream: the first
// candidate runs the chunks' kernels one after the other, every later one on two branches) and hands it to tune_add.
// A key not seen before is entered with `want` candidates to try; with the cache full the smallest key goes first,
// its live instances to `retired`.
inline int tune_pick(GraphCache &gc, uint64_t key, uint32_t want, bool *one_stream, std::vector<GraphHandle> *retired) {
    auto it = gc.keys.find(key);
    if (it == gc.keys.end()) {
        if (gc.keys.size() >= kGraphCacheKeys) {
            tune_retire(gc.keys.begin()->second, retired);
            gc.keys.erase(gc.keys.begin());
        }
        it = gc.keys.emplace(key, GraphTune{}).first;
        it->second.want = want;
    }
    GraphTune &g = it->second;
    gc.tune_pending = false;
    *one_stream = g.cand.empty();
    if (g.chosen >= 0) return g.chosen;
    // still choosing: the newest candidate until it has had its runs, then one more candidate
    int use = (int)g.cand.size() - 1;
    if (use > 0 && g.cand.size() >= g.want && g.runs[use] >= kTuneRunsPerCandidate && g.recheck < kTuneRecheckRuns)
        use = 0;  // every candidate has had its runs: the first one ran on a cold chip -- it gets two more now
    else if ((use < 0 || g.runs[use] >= kTuneRunsPerCandidate) && g.cand.size() < g.want)
        return -1;
    g.last = use;
    gc.tune_key = key;
    gc.tune_pending = true;
    return use;
}

// the instance tune_pick asked for: it runs the batch
inline int tune_add(GraphCache &gc, uint64_t key, GraphHandle h) {
    GraphTune &g = gc.keys[key];
    g.cand.push_back(h);
    g.ms.push_back(1e30f);
    g.runs.push_back(0);
    g.last = (int)g.cand.size() - 1;
    gc.tune_key = key;
    gc.tune_pending = true;
    return g.last;
}

// The batch of a key that is still being chosen has finished in `ms`.  Returns the key's entry when that settled the
// choice (the losers are in `retired`, their slots null), else null; a report with no batch pending, or for a key that
// has been evicted since, changes nothing.
inline const GraphTune *tune_report(GraphCache &gc, float ms, std::vector<GraphHandle> *retired) {
    if (!gc.tune_pending) return nullptr;
    gc.tune_pending = false;
    auto it = gc.keys.find(gc.tune_key);
    if (it == gc.keys.end()) return nullptr;
    GraphTune &g = it->second;
    if (g.last < 0 || g.chosen >= 0) return nullptr;
    g.runs[g.last] += 1;
    if (g.runs[g.last] > 1 || kTuneRunsPerCandidate == 1) g.ms[g.last] = std::min(g.ms[g.last], ms);
    const bool all_ran = g.cand.size() >= g.want && g.runs.back() >= kTuneRunsPerCandidate;
    if (all_ran && g.cand.size() > 1 && g.last == 0 && g.runs[0] > kTuneRunsPerCandidate) g.recheck += 1;
    if (!(all_ran && (g.cand.size() == 1 || g.recheck >= kTuneRecheckRuns))) return nullptr;
    int best = 0;
    for (int k = 1; k < (int)g.cand.size(); ++k)
        if (g.ms[k] < g.ms[best] * (best == 0 ? kTuneTwoBranchGain : 1.0f)) best = k;
    for (int k = 0; k < (int)g.cand.size(); ++k)
        if (k != best) {
            retired->push_back(g.cand[k]);
            g.cand[k] = nullptr;
        }
    g.chosen = best;
    return &g;
}

// no batch of a key still being chosen is in flight (adder_hip_launch_plan_settled)
inline bool tune_settled(const GraphCache &gc) {
    auto it = gc.keys.find(gc.tune_key);
    return it == gc.keys.end() || it->second.chosen >= 0;
}

}  // namespace adder
#pragma GCC visibility pop
