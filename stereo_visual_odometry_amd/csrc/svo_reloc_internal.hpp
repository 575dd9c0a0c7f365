// svo_reloc_internal.hpp — what follows the search in a relocalising call: k_reloc_select's arguments and launcher
// (svo_kernels_reloc.hip) and the PnP stage context it feeds (svo_api.hip), both for reloc_run (svo_match_api.hip).
#pragma once
#include "svo_internal.hpp"
#include "svo_match_internal.hpp"
#include "svo_reloc.hpp"

// The arguments of k_reloc_select.  In: the n result rows of the search, the index's point rows, the queries' pixels, rules 1 and 4.
// Out: the stage context's PnP inputs (out_xy = tl1, out_xyz = world, candidate c at element c), its state row, and the candidate
// lists with their count.
struct RelocArgs {
    const svo_desc_match* match; const RelocPoint* points; const float2* xy; int n;
    RelocRule rule; int min_candidates;
    float2* out_xy; float* out_xyz; SeqState* st;
    int32_t* cand_query; int32_t* cand_row; int32_t* n_cand;
};
// one block behind k_desc_match_merge on the index's stream; a.n <= SVO_RELOC_MAX_QUERIES (the caller checks)
void launch_reloc_select(const RelocArgs& a, hipStream_t s);

// This thread's cached stage context (svo_api.hip, stage_ctx) configured as svo_camera_to_world configures it, with room for cap
// points: its buffers are idle when this returns, and stay this thread's until its next stage call.
int svo_reloc_stage_ctx(int device, int cap, int ransac_iterations, float reproj_error, float confidence, const DevBuffers** d);
