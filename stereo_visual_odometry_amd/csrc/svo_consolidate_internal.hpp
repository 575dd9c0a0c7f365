// svo_consolidate_internal.hpp — the launchers of the consolidation kernels (svo_kernels_consolidate.hip) for the host side
// (svo_match_api.hip).  Every launcher enqueues on s and returns; an empty scope launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svo_consolidate.hpp"
#include "svo_retire_internal.hpp"

// What a call keeps on the device beside its scratch, in the room of retire's RetireCtl: the table's overflow flag and the counts of
// the result, spread over CONS_COUNT_SLOTS cache lines as the transform's are (svo_retire_internal.hpp) — block b adds to slot
// b % CONS_COUNT_SLOTS, the host sums.
#define CONS_COUNT_SLOTS RETIRE_COUNT_SLOTS
struct ConsCounts { int32_t n_members, n_groups, n_far_views, n_capped_groups, pad[12]; };
struct ConsCtl { int32_t table_full, pad[15]; ConsCounts counts[CONS_COUNT_SLOTS]; };
static_assert(sizeof(ConsCounts) == 64 && sizeof(ConsCtl) == sizeof(RetireCtl), "the consolidation's counts live where retire's do");

// the parts of the scratch the kernels see (cons_layout cuts them), and the scope
struct ConsWork {
    int row_lo, n;                                    // the scope [row_lo, row_lo + n)
    int32_t tag_lo, tag_hi;
    uint8_t* keep;                                    // [n]
    int32_t* offset;                                  // [n + 1] the ranks' room
    int32_t* sums;                                    // the block counts' room
    int32_t* table; int32_t* count; uint32_t slots;   // [slots] each; table RETIRE_EMPTY and count 0 going in
    int32_t* list;                                    // [n]
    ConsCtl* ctl;                                     // zero going in
};

// Rules 1 - 5 up to the keep flags: keep[i] = 0 exactly for the members that are not their group's latest row, and the latest row
// of every group of two or more holds the medoid's descriptor and rule 4's point.  Nothing of the index is written when
// ctl->table_full was raised (it cannot be at load <= 1/2).
void launch_consolidate(const RetireRows& x, const ConsWork& w, float radius, hipStream_t s);
