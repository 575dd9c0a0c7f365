// svo_insert_internal.hpp — the launcher of the insertion kernels (svo_kernels_insert.hip) for the host side (svo_match_api.hip).
// It enqueues on s and returns; a call without tiles launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "svo_insert.hpp"

// the index's rows as the kernels write them: points null on an index without points
struct InsertRows { uint8_t* desc; uint64_t* ids; uint4* points; };

// One launch sequence: the observation and descriptor rows it reads (device addresses: a slot of the host-mapped rings, or a staged
// group in the scratch), the parts of the working memory (insert_layout cuts them), and the call.
struct InsertWork {
    const uint8_t* obs;                               // rows of INSERT_OBS_BYTES
    const uint8_t* desc;                              // rows of INSERT_DESC_BYTES
    const InsertEntry* entry; const double* T;        // [n], [n][12] or null: the points as they are
    int32_t n, tiles;
    uint64_t* mask;                                   // [tiles][INSERT_TILE_WAVES]
    int32_t* offset;                                  // [tiles + 1]
    InsertCtl* ctl; int32_t* n_added;                 // what the call reads back
    uint32_t need;                                    // insert_need
    int32_t with_points;
    int32_t at, room;                                 // the first row written, and how many may be: capacity - at
};

// Rules 1 - 5: the kept rows of the n entries at rows at + 0 .. of x, ctl and n_added as InsertCtl says.  Nothing is written when
// the kept rows exceed w.room.
void launch_insert(const InsertRows& x, const InsertWork& w, hipStream_t s);
