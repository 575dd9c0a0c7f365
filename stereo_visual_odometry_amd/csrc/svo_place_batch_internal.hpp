// svo_place_batch_internal.hpp — the batched place candidates as their translation units share them: the arguments and launchers of
// the kernels (svo_kernels_place_batch.hip) for svo_desc_index_tag_votes_batch, places_batch and places_from_ids_batch
// (svo_match_api.hip).  The rules and the layouts are svo_place_batch.hpp's.  Every launcher enqueues on s and returns.
#pragma once
#include "svo_place_internal.hpp"
#include "svo_place_batch.hpp"

static_assert(sizeof(PbCam) == 16, "a camera's record is 16 bytes");
static_assert(PB_MAX_CAMERAS == SVO_PLACE_BATCH_MAX_CAMERAS && PB_MAX_IDS == SVO_PLACE_BATCH_MAX_IDS && PB_MAX_BINS == SVO_PLACE_BATCH_MAX_BINS, "include/svo.h's limits");

// The table of one call: camera b's entries are list[begin[b] .. begin[b] + n) with n = its slice's length, or n_dev[b] where n_dev
// is given (k_reloc_select_batch's counts; no more than the slice).  m_rows (k_reloc_select_batch's cand_row, laid out like the
// list): the list is gathered as ids[m_rows[p]]; null: the list is there already.  table: mask + 1 slots, all PLACE_EMPTY going in.
struct PbTableArgs {
    const int32_t* begin; const int32_t* n_dev; const int32_t* m_rows; const uint64_t* ids;
    uint64_t* list; int32_t* cam; int32_t* table; uint32_t mask;
    PbCam* cams;
};
// Two launches, a block per camera each: the list and cam[] complete, then the inserts; cams[b].n_landmarks = |M_b|
void launch_place_batch_table(const PbTableArgs& a, int n_cameras, hipStream_t s);

// Rule 2 for every camera: the shared bins {rows, first_inv, end} (votes unused; all zero going in) and votes[cam * n_bins + bin]
// (zero going in) of the rows [row_lo, row_hi).  Every row is read once, whatever the number of cameras.
struct PbSweepArgs {
    const int32_t* table; uint32_t mask; const uint64_t* list; const int32_t* cam;
    const uint64_t* ids; const RelocPoint* points; int row_lo, row_hi; int32_t tag_lo, tag_hi;
    int n_bins; PlaceBin* bins; int32_t* votes;
};
void launch_place_batch_sweep(const PbSweepArgs& a, hipStream_t s);

// Rule 3, a block per camera over its row of votes: places[cam * max_places ..], cams[cam].n_places and n_tags_voted
void launch_place_batch_pick(const int32_t* votes, const PlaceBin* bins, int n_bins, int32_t tag_lo, int32_t min_votes, int32_t separation,
                             int32_t max_places, PlaceOut* places, PbCam* cams, int n_cameras, hipStream_t s);
