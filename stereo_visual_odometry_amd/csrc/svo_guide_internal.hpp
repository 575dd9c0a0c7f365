// svo_guide_internal.hpp — the two launchers a search with a guide puts where an unguided one puts launch_desc_match: the projection
// and the gated search (svo_kernels_guide.hip), for search_enqueue (svo_match_api.hip).  The merge behind them is the unguided one.
#pragma once
#include "svo_reloc_internal.hpp"
#include "svo_guide.hpp"

// uv[row] = the projection of points[row] for every row of [row_lo, row_hi); an empty range launches nothing
void launch_guide_project(const RelocPoint* points, const GuidePose& g, int row_lo, int row_hi, float2* uv, hipStream_t s);

// launch_desc_match over the admissible rows only.  Lane `slot` of the launch serves query order[slot] (order: a permutation of
// 0 .. n - 1 on the device) — its descriptor query[order[slot]], its pixel qxy[order[slot]] — and writes
// part[order[slot] * r.n_chunks + j], so that k_desc_match_merge behind it sees the queries under their own numbers.
void launch_desc_match_guided(const uint32_t* desc, const uint64_t* ids, const float2* uv, const uint32_t* query, const float2* qxy,
                              const int32_t* order, int n, float radius, const MatchRange& r, MatchPartial* part, hipStream_t s);
