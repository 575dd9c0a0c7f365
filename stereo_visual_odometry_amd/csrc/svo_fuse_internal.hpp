// svo_fuse_internal.hpp — the landmark fusion as its translation units share it: the launchers of the kernels
// (svo_kernels_fuse.hip) for svo_desc_index_match_near, pair_near, relabel and fuse (svo_match_api.hip).  The rules and the scratch's
// layout are svo_fuse.hpp's.  Every launcher enqueues on s and returns.
#pragma once
#include "svo_reloc_internal.hpp"
#include "svo_fuse.hpp"

static_assert(sizeof(FuseCount) == 64 && sizeof(FuseCtl) == 64 + 64 * FUSE_COUNT_SLOTS, "one cache line per count");
static_assert(FUSE_MAX_ROWS == SVO_RELOC_MAX_QUERIES, "the pairing behind the search is k_align_pairs: 4096 rows");

// Rules 1 - 2: the n source rows [src_row, src_row + n) of the index as the queries against the rows of r, each against the rows its
// point admits: part[q * r.n_chunks + j] for source row src_row + q and chunk j, k_desc_match's layout, so that
// launch_desc_match_merge follows unchanged.  n <= 0 or an empty range launches nothing.
void launch_desc_match_near(const uint32_t* desc, const uint64_t* ids, const RelocPoint* points, int src_row, int n, float radius,
                            const MatchRange& r, MatchPartial* part, hipStream_t s);

// Rule 4 on the pairs k_align_pairs left (*n_pairs of them, at most cap): from[c] = ids[pair_src[c]], to[c] = ids[pair_dst[c]], and
// ctl->n_same, ctl->n_fused (zero going in).
void launch_fuse_map(const int32_t* n_pairs, int cap, const int32_t* pair_src, const int32_t* pair_dst, const uint64_t* ids, uint64_t* from,
                     uint64_t* to, FuseCtl* ctl, hipStream_t s);
// Rule 5.  The table (slots, all FUSE_EMPTY going in) takes the entries of the (from, to) list that map something — *n_dev of them
// where n_dev is given (at most n), else n — and then every row of [row_lo, row_hi) whose id the table maps gets its new id;
// ctl->counts (zero going in) count them, summed over the slots.  Two launches: no kernel waits for another workgroup.
void launch_fuse_relabel(const uint64_t* from, const uint64_t* to, const int32_t* n_dev, int n, int32_t* table, uint32_t slots, uint64_t* ids,
                         int row_lo, int row_hi, FuseCtl* ctl, hipStream_t s);
