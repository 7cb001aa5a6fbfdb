// C entry points of the batch plan (adder-codec-rs_amd/csrc/adder_batch_plan.hpp, the header libadder_hip.so's
// enqueue_frames includes) for tests/test_batch_plan.py.
#include "adder_batch_plan.hpp"

using namespace adder;

extern "C" {
size_t plan_in_size() { return sizeof(BatchPlanIn); }
size_t plan_out_size() { return sizeof(BatchPlan); }
void plan_batch_c(const BatchPlanIn *in, BatchPlan *out) { *out = plan_batch(*in); }
size_t plan_worst_case_events_per_frame(const BatchPlanIn *in) { return worst_case_events_per_frame(*in); }
unsigned plan_frame_kernel(uint32_t variant) { return variant_frame_kernel(variant); }
int plan_scan_chains(uint32_t variant) { return variant_scan_chains(variant) ? 1 : 0; }
int plan_park_layout(uint32_t log_cap, uint32_t launch_depth, uint32_t num_waves, uint32_t chunk, uint32_t park_bytes,
                     ParkLayout *out) {
    return batch_park_layout(log_cap, launch_depth, num_waves, chunk, park_bytes, out) ? 1 : 0;
}
}
