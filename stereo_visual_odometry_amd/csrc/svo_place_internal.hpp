// svo_place_internal.hpp — the place candidates as their translation units share them: the launchers of the kernels
// (svo_kernels_place.hip) for svo_desc_index_tag_votes, places and places_from_ids (svo_match_api.hip).  The rules and the scratch's
// layout are svo_place.hpp's.  Every launcher enqueues on s and returns.
#pragma once
#include "svo_reloc_internal.hpp"
#include "svo_place.hpp"

static_assert(sizeof(PlaceBin) == 16 && sizeof(PlaceOut) == 32 && sizeof(svo_place) == sizeof(PlaceOut), "a bin is 16 bytes, a place 32");
static_assert(sizeof(PlaceCtl) == 32 + 32 * PLACE_MAX_PLACES, "the counts, then the places");
static_assert(PLACE_MAX_IDS == SVO_RELOC_MAX_QUERIES && PLACE_MAX_IDS == SVO_PLACE_MAX_IDS, "M is one selection's candidates at most");
static_assert(PLACE_MAX_TAGS == SVO_PLACE_MAX_TAGS && PLACE_MAX_PLACES == SVO_PLACE_MAX_PLACES && PLACE_MAX_ROWS == SVO_MATCH_MAX_ROWS, "include/svo.h's limits");

// What rule 2's sweep reads.  M is the ids of `list` (m_rows null) or the ids of the index's rows m_rows[c] (k_reloc_select's
// cand_row); its entries are *n_dev where n_dev is given (at most n), else n; n <= PLACE_MAX_IDS.
struct PlaceSweepArgs {
    const uint64_t* list; const int32_t* m_rows; const int32_t* n_dev; int n;
    const uint64_t* ids; const RelocPoint* points; int row_lo, row_hi; int32_t tag_lo, tag_hi;
    PlaceBin* bins; PlaceCtl* ctl;
};
// Rule 2: the bins (all zero going in) of the rows [row_lo, row_hi), and ctl->n_landmarks = |M| (zero going in).  combine: the
// lanes of a wave that share a tag issue one set of atomics; without, every qualifying row issues its own four.  Same bits either way.
void launch_place_sweep(const PlaceSweepArgs& a, bool combine, hipStream_t s);
// Rule 3 behind the sweep: the bins with votes >= min_votes as a list of keys (ctl->n_list, ctl->n_tags_voted; zero going in), then
// one block that emits ctl->places and ctl->n_places.  Two launches: no kernel waits for another workgroup.
void launch_place_pick(PlaceBin* bins, int n_bins, int32_t tag_lo, int32_t min_votes, int32_t separation, int32_t max_places, uint64_t* keys,
                       PlaceCtl* ctl, hipStream_t s);
