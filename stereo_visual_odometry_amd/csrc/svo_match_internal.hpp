// svo_match_internal.hpp — the search of the descriptor index as its translation units share it: the geometry of a search and the
// launchers of k_desc_match and k_desc_match_merge (svo_kernels_match.hip) for the host side (svo_match_api.hip), and the device
// code that k_desc_match and k_desc_match_guided (svo_kernels_guide.hip) have in common.
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

#if defined(__HIPCC__)
// query q's eight dwords, which a lane keeps in VGPRs for its whole walk
static __device__ __forceinline__ void match_load_query(const uint32_t* __restrict__ query, int q, uint32_t (&qd)[8]) {
    const uint4* qp = reinterpret_cast<const uint4*>(query + (size_t)q * 8);
    const uint4 a = qp[0], b = qp[1];
    qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
}

// the Hamming distance of a query and a row read as two 16-byte halves
static __device__ __forceinline__ uint32_t match_dist(const uint32_t (&q)[8], const uint4 a, const uint4 b) {
    uint32_t d = __popc(q[0] ^ a.x);
    d += __popc(q[1] ^ a.y); d += __popc(q[2] ^ a.z); d += __popc(q[3] ^ a.w);
    d += __popc(q[4] ^ b.x); d += __popc(q[5] ^ b.y); d += __popc(q[6] ^ b.z); d += __popc(q[7] ^ b.w);
    return d;
}

// the rows chunk j of the search walks: [r0, r1), inside [row_lo, row_hi)
static __device__ __forceinline__ void match_chunk_rows(const MatchRange& r, int j, int& r0, int& r1) {
    r0 = (r.chunk0 + j) * r.chunk_rows;               // <= row_hi < 2^24, chunk_rows <= 2^24: no overflow
    r1 = r0 + r.chunk_rows;
    r0 = r0 > r.row_lo ? r0 : r.row_lo;
    r1 = r1 < r.row_hi ? r1 : r.row_hi;
}
#endif
