// svo_match_internal.hpp — what the descriptor index's two translation units share (svo_kernels_match.hip: the kernels and their
// launchers; svo_match_api.hip: the index object and the C-ABI of include/svo.h, "Descriptor index").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svo.h"
#include "svo_match.hpp"

// the (k1, k2) of one (query, chunk): MatchState without id1, which ids[row of k1] gives back
struct MatchPartial { match_key k1, k2; };
static_assert(sizeof(MatchPartial) == 16, "a partial state leaves as one 16-byte store");

// The geometry of one search: rows [row_lo, row_hi) cut at the multiples of chunk_rows.  Chunk j of the search is the index's chunk
// chunk0 + j, clipped to the range: the first one skips to row_lo, the last one stops at row_hi.
struct MatchRange { int row_lo, row_hi, chunk_rows, chunk0, n_chunks; };
static inline MatchRange match_range(int row_lo, int row_hi, int chunk_rows) {
    MatchRange r{row_lo, row_hi, chunk_rows, row_lo / chunk_rows, 0};
    if (row_hi > row_lo) r.n_chunks = (row_hi - 1) / chunk_rows - r.chunk0 + 1;
    return r;
}

// n queries (device, 8 dwords each) against the rows of r: part[q * r.n_chunks + j] for every query q and chunk j.  n <= 0 or an
// empty range launches nothing.
void launch_desc_match(const uint32_t* desc, const uint64_t* ids, const uint32_t* query, int n, const MatchRange& r, MatchPartial* part, hipStream_t s);
// the partial states of each query folded into its result row; an empty range (r.n_chunks == 0) gives rows of SVO_MATCH_NONE
void launch_desc_match_merge(const MatchPartial* part, const uint64_t* ids, int n, const MatchRange& r, svo_desc_match* out, hipStream_t s);

// the text svo_last_error() returns on this thread (svo_api.hip owns it)
void svo_set_error(const char* msg);
