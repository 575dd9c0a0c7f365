// svo_insert.hpp — the rules of the descriptor index's batched insertion (include/svo.h, "Batched insertion"): which observation
// rows of an entry are kept, the id and the point of a kept row, the plan that cuts the entries into tiles, where a tile's rows land,
// and the layout of the working memory.  Plain C++ that a host compiler takes as it is, like svo_consolidate.hpp, so that a
// stand-alone host program (tests/cpp/insert_host.cpp) runs exactly the text the kernels (svo_kernels_insert.hip) and
// svo_match_api.hip run.  Integers only but for the point, which is reloc_map_point (svo_reloc.hpp): f64, every operation rounded on
// its own (the translation units that include this are built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "svo_reloc.hpp"

#if defined(__HIPCC__)
#define SVO_INSERT_HD __host__ __device__
#else
#define SVO_INSERT_HD
#endif

#define INSERT_MAX_ENTRIES 1024                       // include/svo.h: SVO_INSERT_MAX_ENTRIES
#define INSERT_MAX_OBS_ROWS (1 << 18)                 // the rows of one staged group, and of one svo_desc_index_add_obs
#define INSERT_TILE 256                               // rows of one tile: a block of four waves, a lane per row
#define INSERT_TILE_WAVES (INSERT_TILE / 64)
#define INSERT_SCAN_BLOCK 1024                        // lanes of the one block that scans the tile counts
#define INSERT_OBS_BYTES 64                           // svo_track_obs, and where the kernels read in it
#define INSERT_OBS_ID 0
#define INSERT_OBS_XYZ 40
#define INSERT_OBS_FLAGS 56
#define INSERT_DESC_BYTES 32
#define INSERT_HAS_XYZ 2u                             // include/svo.h: SVO_OBS_HAS_XYZ

// ---- rule 2: a row is kept when its flags carry every needed bit; the points call always needs SVO_OBS_HAS_XYZ
SVO_INSERT_HD static inline uint32_t insert_need(uint32_t need_flags, bool with_points) { return with_points ? need_flags | INSERT_HAS_XYZ : need_flags; }
SVO_INSERT_HD static inline bool insert_keep(int32_t flags, uint32_t need) { return ((uint32_t)flags & need) == need; }

// ---- rule 4: the id of a kept row, modulo 2^64
SVO_INSERT_HD static inline uint64_t insert_id(int64_t obs_id, uint64_t id_base) { return (uint64_t)obs_id + id_base; }

// ---- rule 5: the point of a kept row (T null: as it is), and whether the call must refuse it
SVO_INSERT_HD static inline void insert_point(const double* T, const float p[3], float out[3]) {
    if (T) reloc_map_point(T, p, out);
    else { out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; }
}
SVO_INSERT_HD static inline bool insert_point_ok(const float p[3]) { return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]); }

// ---- the plan.  One entry as the kernels read it, 32 bytes: its rows [begin, begin + rows) of the observation and descriptor rows
// the launch is given, the number of its first tile, its tag and its id offset.  An entry of r rows has insert_tiles(r) tiles; tile
// t of the call belongs to the last entry whose tile0 is at most t (an entry without rows has no tile and shares its tile0 with the
// entry after it, which comes later in that order).
struct InsertEntry { int32_t begin, rows, tile0, tag; uint64_t id_base; uint64_t reserved; };
SVO_INSERT_HD static inline int32_t insert_tiles(int32_t rows) { return (rows + INSERT_TILE - 1) / INSERT_TILE; }
// fills tile0 from rows, entry after entry -> the call's tiles
static inline int32_t insert_plan(int32_t n, InsertEntry* e) {
    int32_t t = 0;
    for (int32_t b = 0; b < n; b++) { e[b].tile0 = t; t += insert_tiles(e[b].rows); }
    return t;
}
// the entry of tile t, 0 <= t < the call's tiles: a bisection over tile0
SVO_INSERT_HD static inline int32_t insert_tile_entry(const InsertEntry* e, int32_t n, int32_t t) {
    int32_t lo = 0, hi = n - 1;                       // the answer is in [lo, hi]; e[0].tile0 == 0 <= t
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) / 2;
        if (e[mid].tile0 <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- rule 3: where a kept row lands.  A tile's keep bits are four 64-bit masks, a wave each (bit l: lane l's row is kept).  The rank
// of row (wave w, lane l) among its tile's kept rows, and the tile's count; the row's place is size + offset[tile] + rank, offset
// being the exclusive scan of the counts over the call's tiles in order.
SVO_INSERT_HD static inline int32_t insert_popc(uint64_t m) { return (int32_t)__builtin_popcountll(m); }
SVO_INSERT_HD static inline int32_t insert_tile_count(const uint64_t* mask) {
    int32_t c = 0;
    for (int w = 0; w < INSERT_TILE_WAVES; w++) c += insert_popc(mask[w]);
    return c;
}
SVO_INSERT_HD static inline int32_t insert_rank(const uint64_t* mask, int32_t wave, int32_t lane) {
    int32_t r = 0;
    uint64_t own = 0;
    for (int w = 0; w < INSERT_TILE_WAVES; w++) {     // a fixed trip count: the masks stay in registers
        if (w < wave) r += insert_popc(mask[w]);
        if (w == wave) own = mask[w];
    }
    return r + insert_popc(own & (((uint64_t)1 << lane) - 1));
}
SVO_INSERT_HD static inline bool insert_kept(const uint64_t* mask, int32_t wave, int32_t lane) {
    uint64_t own = 0;
    for (int w = 0; w < INSERT_TILE_WAVES; w++) if (w == wave) own = mask[w];
    return (own >> lane) & 1;
}

// What a call reads back: the kept rows of all entries, whether they exceed the room it was given (nothing was written then), and
// whether a kept row's point was not finite.  64 bytes, in front of the entries' counts.
struct InsertCtl { int32_t total, over, nonfinite, pad[13]; };

// ---- the working memory of one call in the index's maintenance scratch, every part rounded up to 256 bytes: going up in one copy
// the entries and their transforms (12 doubles each: the rows of cam_to_map that reloc_map_point reads); the masks, the offsets (one
// more than the tiles); coming down in one copy the control block and the entries' counts; and, for a staged group, its observation
// and descriptor rows.  The pinned staging mirrors [0, up_end) and [down, down_end).
struct InsertLayout { size_t entry, T, up_end, mask, offset, down, n_added, down_end, obs, desc, total; };
static inline size_t insert_round(size_t b) { return (b + 255) / 256 * 256; }
static inline InsertLayout insert_layout(int32_t n, int32_t tiles, int32_t staged_rows) {
    InsertLayout l;
    const size_t e = (size_t)n, t = (size_t)tiles, r = (size_t)staged_rows;
    l.entry = 0;
    l.T = insert_round(sizeof(InsertEntry) * e);
    l.up_end = l.T + insert_round(12 * sizeof(double) * e);
    l.mask = l.up_end;
    l.offset = l.mask + insert_round(8 * INSERT_TILE_WAVES * t);
    l.down = l.offset + insert_round(4 * (t + 1));
    l.n_added = l.down + sizeof(InsertCtl);
    l.down_end = l.down + insert_round(sizeof(InsertCtl) + 4 * e);
    l.obs = l.down_end;
    l.desc = l.obs + insert_round((size_t)INSERT_OBS_BYTES * r);
    l.total = l.desc + insert_round((size_t)INSERT_DESC_BYTES * r);
    return l;
}

// ---- the whole of rules 1 - 5 for one call as a sequential program runs them, over rows where the kernels read them: obs rows of
// 64 bytes, desc rows of 32.  Kept rows go to out_* from row 0 on (out_xyz, out_tag only with_points); n_added[b] per entry.
// -> the kept rows, or -1 when a kept row's point is not finite.  T: 12 doubles an entry, or null.
static inline int32_t insert_plain(int32_t n, const InsertEntry* e, const uint8_t* obs, const uint8_t* desc, uint32_t need, bool with_points,
                                   const double* T, uint8_t* out_desc, uint64_t* out_ids, float* out_xyz, int32_t* out_tag, int32_t* n_added) {
    int32_t at = 0;
    bool bad = false;
    for (int32_t b = 0; b < n; b++) {
        n_added[b] = 0;
        for (int32_t i = 0; i < e[b].rows; i++) {
            const uint8_t* row = obs + (size_t)(e[b].begin + i) * INSERT_OBS_BYTES;
            int32_t flags; int64_t id; float p[3], q[3];
            __builtin_memcpy(&flags, row + INSERT_OBS_FLAGS, 4);
            if (!insert_keep(flags, need)) continue;
            __builtin_memcpy(&id, row + INSERT_OBS_ID, 8);
            __builtin_memcpy(p, row + INSERT_OBS_XYZ, 12);
            __builtin_memcpy(out_desc + (size_t)at * INSERT_DESC_BYTES, desc + (size_t)(e[b].begin + i) * INSERT_DESC_BYTES, INSERT_DESC_BYTES);
            out_ids[at] = insert_id(id, e[b].id_base);
            if (with_points) {
                insert_point(T ? T + 12 * b : nullptr, p, q);
                if (!insert_point_ok(q)) bad = true;
                out_xyz[3 * at] = q[0]; out_xyz[3 * at + 1] = q[1]; out_xyz[3 * at + 2] = q[2];
                out_tag[at] = e[b].tag;
            }
            at++; n_added[b]++;
        }
    }
    return bad ? -1 : at;
}
