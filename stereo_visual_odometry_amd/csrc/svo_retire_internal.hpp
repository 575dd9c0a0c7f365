// svo_retire_internal.hpp — the launchers of the index-maintenance kernels (svo_kernels_retire.hip) for the host side
// (svo_match_api.hip).  Every launcher enqueues on s and returns; an empty range launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svo_retire.hpp"

// the arrays of an index as the kernels see them; points null: an index without points
struct RetireRows { uint4* desc; uint64_t* ids; uint4* points; };
// What a maintenance call keeps on the device beside its scratch: the table's overflow flag, and a transform's two counts.  The
// counts are spread over RETIRE_COUNT_SLOTS cache lines — block b adds to slot b % RETIRE_COUNT_SLOTS, the host sums — since atomics
// on one address take their turns in the L2: with one pair of counters the kernel took 0.193 ms for 2^20 rows on an MI355X, with
// the slots 0.011 ms (tools/desc_retire_bench.py).
#define RETIRE_COUNT_SLOTS 128
struct RetireCounts { int32_t n_moved, n_skipped, pad[14]; };
struct RetireCtl { int32_t table_full, pad[15]; RetireCounts counts[RETIRE_COUNT_SLOTS]; };
static_assert(sizeof(RetireCounts) == 64 && sizeof(RetireCtl) == 64 + 64 * RETIRE_COUNT_SLOTS, "one cache line per pair of counts");
// the transform's matrix, by value
struct RetireT { double m[16]; };

// keep[i] = alive1(row_lo + i) for the scope's n rows; sorted: the id list on the device, ascending without duplicates
void launch_retire_flags(const RetireRows& x, int row_lo, int n, uint32_t flags, int32_t tag_lo, int32_t tag_hi, const uint64_t* sorted,
                         int32_t n_sorted, uint8_t* keep, hipStream_t s);
// LATEST_PER_ID: the table (slots, all RETIRE_EMPTY going in) takes every alive row, then keep[i] stays set only where the row is
// its id's slot; ctl->table_full is raised where a probe runs out (it cannot at load <= 1/2)
void launch_retire_latest(const RetireRows& x, int row_lo, int n, uint8_t* keep, int32_t* table, uint32_t slots, RetireCtl* ctl, hipStream_t s);
// rank[i] = #{i' < i : keep[i']} for i = 0 .. n: the block counts (counts: blocks + RETIRE_BLOCK + 1 entries), their scan, the ranks
void launch_retire_ranks(const uint8_t* keep, int n, int32_t* counts, int32_t* rank, hipStream_t s);
// One slab: rows [row, row + n) of the index into the bounce buffer (slab_rows rows: descriptors, then points, then ids), the row
// with keep[i] set at place rank[i] - rank[0]; then the rows of the bounce buffer down to dst + rank[0] and on.  keep and rank null:
// every row, in place order.
void launch_retire_slab(const RetireRows& x, int row, int n, const uint8_t* keep, const int32_t* rank, int dst, void* bounce, int slab_rows,
                        hipStream_t s);
// every selected row of [row_lo, row_hi) through T; ctl->counts (zero going in) count them, summed over the slots
void launch_transform_points(uint4* points, const RetireT& T, int row_lo, int row_hi, int32_t tag_lo, int32_t tag_hi, RetireCtl* ctl, hipStream_t s);
