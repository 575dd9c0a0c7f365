// svo_reloc_batch_internal.hpp — the batched relocalisation as its translation units share it: the arguments and launchers of the
// kernels (svo_kernels_reloc_batch.hip) and the PnP stage context of B sequences (svo_api.hip), for svo_desc_index_localize_batch
// (svo_match_api.hip).  The plan and the staging's layout are svo_reloc_batch.hpp's.
#pragma once
#include "svo_guide_internal.hpp"
#include "svo_reloc_batch.hpp"

// one camera of a guided batch as the kernels read it
struct RelocBatchCam { GuidePose pose; float radius; int32_t pad; };
static_assert(sizeof(RelocBatchCam) == RB_CAMERA_BYTES, "svo_reloc_batch.hpp lays the cameras out");

// The guided search of one group of cameras (RbGroup): the index's rows, the cameras of the whole call with their offsets, the
// concatenated queries and pixels, the lane order (global query numbers; null: the queries as they come), the rows' plan, the
// group's first camera and first query, and the partial states of the group: part[(q - q0) * r.n_chunks + chunk].
struct RelocBatchSearch {
    const uint32_t* desc; const uint64_t* ids; const RelocPoint* points;
    const RelocBatchCam* cams; const int32_t* begin;
    const uint32_t* query; const float2* qxy; const int32_t* order;
    RbRange r; int cam0, q0;
    MatchPartial* part;
};
void launch_desc_match_guided_batch(const RelocBatchSearch& a, const RbGrid& g, hipStream_t s);

// order[begin[b] .. begin[b + 1]) = camera b's queries, as global numbers, sorted by (rb_cell_key, j): one block per camera
void launch_reloc_batch_order(const float2* qxy, const int32_t* begin, const RelocBatchCam* cams, int n_cameras, int32_t* order, hipStream_t s);

// k_reloc_select's arguments for every camera at once.  match, xy, cand_query, cand_row: the concatenated arrays, camera b's slice at
// begin[b]; out_xy, out_xyz: the stage context's PnP inputs, camera b's rows at b * cap; st, n_cand: one entry per camera.
struct RelocBatchSelect {
    const svo_desc_match* match; const RelocPoint* points; const float2* xy; const int32_t* begin;
    RelocRule rule; int min_candidates;
    float2* out_xy; float* out_xyz; SeqState* st; int cap;
    int32_t* cand_query; int32_t* cand_row; int32_t* n_cand;
};
void launch_reloc_select_batch(const RelocBatchSelect& a, int n_cameras, hipStream_t s);

// out[begin[b] + c] = inlier[b * cap + c] for c < n_cand[b]: the PnP's flags into the cameras' slices
void launch_reloc_batch_inliers(const uint8_t* inlier, int cap, const int32_t* begin, const int32_t* n_cand, int n_cameras, int max_slice,
                                uint8_t* out, hipStream_t s);

// The PnP stage context of a batch (svo_api.hip): *held, the caller's own context, configured as svo_reloc_stage_ctx configures this
// thread's, with room for n_seq sequences of cap points.  It is kept when it fits; otherwise a new one is made — sequences and points
// at least doubled where they were outgrown — and the old one is handed back in *outgrown for the caller to keep until it goes
// (freeing device memory waits for the device).  *d: a copy of its buffers with B = n_seq, so that a launch runs over n_seq sequences.
int svo_reloc_batch_ctx(int device, int n_seq, int cap, int ransac_iterations, float reproj_error, float confidence, svo_context** held,
                        svo_context** outgrown, DevBuffers* d);
