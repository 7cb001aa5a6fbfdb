// C entry points of the graph tuner's decisions (adder-codec-rs_amd/csrc/adder_graph_tune.hpp, the header
// adder_hip_graphs.cpp includes) for tests/test_graph_tune.py.  A handle is a number the test makes up.
#include "adder_graph_tune.hpp"
#include "adder_variant.hpp"

using namespace adder;

extern "C" {
void *tune_new() { return new GraphCache(); }
void tune_delete(void *gc) { delete static_cast<GraphCache *>(gc); }
// tune_pick; the instances it retired are appended to retired[] (*n_retired counts them)
int tune_pick_c(void *gc, uint64_t key, uint32_t want, int *one_stream, uintptr_t *retired, int *n_retired) {
    std::vector<GraphHandle> r;
    bool one = false;
    const int use = tune_pick(*static_cast<GraphCache *>(gc), key, want, &one, &r);
    *one_stream = one ? 1 : 0;
    for (GraphHandle h : r) retired[(*n_retired)++] = reinterpret_cast<uintptr_t>(h);
    return use;
}
int tune_add_c(void *gc, uint64_t key, uintptr_t handle) {
    return tune_add(*static_cast<GraphCache *>(gc), key, reinterpret_cast<GraphHandle>(handle));
}
// tune_report: the chosen candidate when the report settled the choice, else -1
int tune_report_c(void *gc, float ms, uintptr_t *retired, int *n_retired) {
    std::vector<GraphHandle> r;
    const GraphTune *g = tune_report(*static_cast<GraphCache *>(gc), ms, &r);
    for (GraphHandle h : r) retired[(*n_retired)++] = reinterpret_cast<uintptr_t>(h);
    return g ? g->chosen : -1;
}
int tune_retire_all_c(void *gc, uintptr_t *retired) {
    std::vector<GraphHandle> r;
    tune_retire_all(*static_cast<GraphCache *>(gc), &r);
    for (size_t i = 0; i < r.size(); ++i) retired[i] = reinterpret_cast<uintptr_t>(r[i]);
    return (int)r.size();
}
int tune_settled_c(void *gc) { return tune_settled(*static_cast<GraphCache *>(gc)) ? 1 : 0; }
int tune_pending_c(void *gc) { return static_cast<GraphCache *>(gc)->tune_pending ? 1 : 0; }
int tune_keys_c(void *gc) { return (int)static_cast<GraphCache *>(gc)->keys.size(); }
// best time of a candidate of a key (1e30: none counted yet), -1 for a key or candidate that is not there
float tune_best_ms_c(void *gc, uint64_t key, int cand) {
    const GraphCache &c = *static_cast<GraphCache *>(gc);
    auto it = c.keys.find(key);
    if (it == c.keys.end() || cand < 0 || cand >= (int)it->second.ms.size()) return -1.0f;
    return it->second.ms[cand];
}
uint32_t tune_graph_candidates(uint32_t variant, uint32_t num_frames, uint32_t chunk, uint32_t candidates) {
    return variant_graph_candidates(variant, num_frames, chunk, candidates);
}
}
