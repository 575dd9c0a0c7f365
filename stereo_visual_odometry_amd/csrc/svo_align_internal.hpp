// svo_align_internal.hpp — the map alignment as its translation units share it: the arguments and launchers of the kernels
// (svo_kernels_align.hip) for svo_desc_index_pair_rows and svo_desc_index_align (svo_match_api.hip).  The rules and the staging's
// layout are svo_align.hpp's.
#pragma once
#include "svo_reloc_internal.hpp"
#include "svo_align.hpp"

static_assert(ALIGN_MAX_ROWS == SVO_RELOC_MAX_QUERIES, "the pair kernel's LDS lists are k_reloc_select's");
static_assert(sizeof(AlignModel) == 96 && sizeof(AlignOut) == 136, "svo_align.hpp lays the staging out");

// Rules 2 - 5 on the n result rows of the search of rows [src_lo, src_lo + n) (n <= ALIGN_MAX_ROWS; the caller checks): the pairs in
// increasing source row into pair_src, pair_dst and, six floats each, pairs; pair_inlier cleared; *out zeroed but for n_pairs.
struct AlignPairsArgs {
    const svo_desc_match* match; const RelocPoint* points; const uint64_t* ids; int src_lo, n;
    RelocRule rule;
    int32_t* pair_src; int32_t* pair_dst; uint8_t* pair_inlier; float* pairs; AlignOut* out;
};
void launch_align_pairs(const AlignPairsArgs& a, hipStream_t s);

// Rules 6 - 10 behind it.  Both kernels read out->n_pairs and do nothing below min_pairs.  score: counts[h] and models[h] for
// h < hypotheses.  fit: the best hypothesis, the refit rounds, pair_inlier and the rest of *out.
struct AlignFitArgs {
    const float* pairs; int hypotheses, min_pairs, refit_rounds; double dist2;
    int32_t* counts; AlignModel* models; uint8_t* pair_inlier; AlignOut* out;
};
void launch_align_score(const AlignFitArgs& a, hipStream_t s);
void launch_align_fit(const AlignFitArgs& a, hipStream_t s);
