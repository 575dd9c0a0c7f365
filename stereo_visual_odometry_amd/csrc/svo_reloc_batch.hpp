// svo_reloc_batch.hpp — the arithmetic of the batched relocalisation (include/svo.h, "Batched relocalisation"): the check of a call's
// offsets, the plan of its search — the rows of a chunk, the groups of cameras one launch serves, the grid of each launch — the cell
// key that orders a camera's lanes, and the layout of the batch's staging.  Plain C++ that a host compiler takes as it is, like
// svo_retire.hpp, so that a stand-alone host program (tests/cpp/reloc_batch_host.cpp) runs exactly the text svo_match_api.hip and the
// kernels (svo_kernels_reloc_batch.hip) run.  Integers, and one f64 quotient per pixel coordinate for the key.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_RB_HD __host__ __device__
#else
#define SVO_RB_HD
#endif

#define RB_MAX_CAMERAS 1024                           // include/svo.h: SVO_RELOC_BATCH_MAX_CAMERAS
#define RB_MAX_QUERIES (1 << 20)                      // include/svo.h: SVO_RELOC_BATCH_MAX_QUERIES, all cameras together
#define RB_MAX_SLICE 4096                             // queries of one camera: SVO_RELOC_MAX_QUERIES
#define RB_MAX_ROWS (1 << 24)                         // rows of an index
#define RB_BLOCK_SLOTS 1024                           // query slots of one block of the guided search: 16 waves
#define RB_TILE_ROWS 1024                             // rows whose projections one block holds in LDS at a time: 8 KiB
#define RB_GRID_LIMIT 65535                           // blocks along y and z of one launch
#define RB_PART_BUDGET ((size_t)1 << 22)              // partial states of one launch (64 MiB), as the single calls'

// ---- a call's offsets: n_cameras + 1 entries, [0] = 0, non-decreasing, a slice at most RB_MAX_SLICE, the total at most RB_MAX_QUERIES
enum RbOffsets { RB_OFFSETS_OK = 0, RB_OFFSETS_COUNT, RB_OFFSETS_NULL, RB_OFFSETS_FIRST, RB_OFFSETS_ORDER, RB_OFFSETS_SLICE, RB_OFFSETS_TOTAL };
static inline RbOffsets rb_check_offsets(int n_cameras, const int32_t* begin) {
    if (n_cameras < 0 || n_cameras > RB_MAX_CAMERAS) return RB_OFFSETS_COUNT;
    if (n_cameras == 0) return RB_OFFSETS_OK;
    if (!begin) return RB_OFFSETS_NULL;
    if (begin[0] != 0) return RB_OFFSETS_FIRST;
    for (int b = 0; b < n_cameras; b++) {
        if (begin[b + 1] < begin[b]) return RB_OFFSETS_ORDER;
        if (begin[b + 1] - begin[b] > RB_MAX_SLICE) return RB_OFFSETS_SLICE;     // both in 0 .. total so far: no overflow
        if (begin[b + 1] > RB_MAX_QUERIES) return RB_OFFSETS_TOTAL;
    }
    return RB_OFFSETS_OK;
}
static inline int rb_max_slice(int n_cameras, const int32_t* begin) {
    int m = 0;
    for (int b = 0; b < n_cameras; b++) m = begin[b + 1] - begin[b] > m ? begin[b + 1] - begin[b] : m;
    return m;
}

// ---- the rows of a search: [row_lo, row_hi) cut at the multiples of chunk_rows, svo_match_internal.hpp's MatchRange field by field
struct RbRange { int row_lo, row_hi, chunk_rows, chunk0, n_chunks; };
static inline RbRange rb_range(int row_lo, int row_hi, int chunk_rows) {
    RbRange r{row_lo, row_hi, chunk_rows, row_lo / chunk_rows, 0};
    if (row_hi > row_lo) r.n_chunks = (row_hi - 1) / chunk_rows - r.chunk0 + 1;
    return r;
}
// the rows chunk j walks: [r0, r1), inside [row_lo, row_hi)
SVO_RB_HD static inline void rb_chunk_rows(const RbRange& r, int j, int& r0, int& r1) {
    r0 = (r.chunk0 + j) * r.chunk_rows;               // <= row_hi <= 2^24, chunk_rows <= 2^24: no overflow
    r1 = r0 + r.chunk_rows;
    r0 = r0 > r.row_lo ? r0 : r.row_lo;
    r1 = r1 < r.row_hi ? r1 : r.row_hi;
}

// The plan.  Partial states are stored per (query, chunk), so a launch serves a GROUP of consecutive cameras whose queries times the
// chunks fit the budget.  The rows of a chunk double from the index's setting until the largest slice — 64 queries at least, a
// wave — fits alone, so every group holds one camera at least (4096 queries and 2^24 rows: 16 384 rows a chunk at most).  Groups
// are then filled greedily in camera order.  The results depend on none of it.
static inline RbRange rb_plan_range(int row_lo, int row_hi, int chunk_rows, int max_slice) {
    const size_t widest = (size_t)(max_slice > 64 ? max_slice : 64);
    RbRange r = rb_range(row_lo, row_hi, chunk_rows);
    while (widest * (size_t)r.n_chunks > RB_PART_BUDGET) r = rb_range(row_lo, row_hi, chunk_rows *= 2);
    return r;
}
// One launch of the search: cameras [cam0, cam1), their queries [q0, q1), the widest slice among them.
struct RbGroup { int cam0, cam1, q0, q1, max_n; };
// the group that starts at camera cam0 < n_cameras
static inline RbGroup rb_next_group(int n_cameras, const int32_t* begin, int cam0, int n_chunks) {
    RbGroup g{cam0, cam0, begin[cam0], begin[cam0], 0};
    const size_t chunks = (size_t)(n_chunks > 0 ? n_chunks : 0);
    while (g.cam1 < n_cameras && g.cam1 - g.cam0 < RB_GRID_LIMIT) {
        const int n = begin[g.cam1 + 1] - begin[g.cam1];
        if (g.cam1 > g.cam0 && (size_t)(begin[g.cam1 + 1] - g.q0) * chunks > RB_PART_BUDGET) break;
        g.cam1++; g.q1 = begin[g.cam1];
        g.max_n = n > g.max_n ? n : g.max_n;
    }
    return g;
}
// The grid of the guided launch of a group: x the chunks, y the cameras, z the tile groups — a block serves `threads` slots of one
// camera, a multiple of 64 that covers the widest slice up to RB_BLOCK_SLOTS.  max_n == 0 or no chunks: nothing to launch (x = 0).
struct RbGrid { int x, y, z, threads; };
static inline RbGrid rb_guided_grid(const RbGroup& g, int n_chunks) {
    if (g.max_n <= 0 || n_chunks <= 0) return RbGrid{0, 0, 0, 0};
    int threads = (g.max_n + 63) / 64 * 64;
    threads = threads < RB_BLOCK_SLOTS ? threads : RB_BLOCK_SLOTS;
    return RbGrid{n_chunks, g.cam1 - g.cam0, (g.max_n + threads - 1) / threads, threads};
}
// the unguided launch of a group: k_desc_match over its concatenated queries, one wave per block, y the waves
static inline RbGrid rb_unguided_grid(const RbGroup& g, int n_chunks) {
    if (g.q1 <= g.q0 || n_chunks <= 0) return RbGrid{0, 0, 0, 0};
    return RbGrid{n_chunks, (g.q1 - g.q0 + 63) / 64, 1, 64};
}
// the partial states a group's launch writes
static inline size_t rb_group_states(const RbGroup& g, int n_chunks) { return (size_t)(g.q1 - g.q0) * (size_t)(n_chunks > 0 ? n_chunks : 0); }

// ---- the lane order's key: the image cell of a pixel (side 2 x radius, 1 px at least), cells in raster order, a non-finite pixel
// last.  52 bits: 26 per axis, the cell numbers clamped to +-2^25 (less two at the top, so that no pixel shares the last key).
#define RB_KEY_BITS 52
#define RB_KEY_LAST (((uint64_t)1 << RB_KEY_BITS) - 1)
SVO_RB_HD static inline uint64_t rb_cell_axis(double c) {
    const double lim = 33554432.;                     // 2^25
    const double v = c < -lim ? -lim : c > lim - 2. ? lim - 2. : c;
    return (uint64_t)((int64_t)v + (int64_t)33554432);
}
SVO_RB_HD static inline uint64_t rb_cell_key(float x, float y, float radius) {
    const double side = 2. * (double)radius > 1. ? 2. * (double)radius : 1.;
    const double cx = __builtin_floor((double)x / side), cy = __builtin_floor((double)y / side);
    if (!(cx - cx == 0.) || !(cy - cy == 0.)) return RB_KEY_LAST;                  // v - v is 0 for a finite v and NaN otherwise
    return rb_cell_axis(cy) << 26 | rb_cell_axis(cx);
}
// (key, j) as one 64-bit entry of the sort: j < 4096 takes the low 12 bits
SVO_RB_HD static inline uint64_t rb_order_entry(uint64_t key, int j) { return key << 12 | (uint64_t)j; }
SVO_RB_HD static inline int rb_entry_query(uint64_t e) { return (int)(e & 4095u); }

// ---- the staging.  One device block and one pinned block, cut alike, each part rounded up to 256 bytes (include/svo.h states the
// sums): what goes up in one copy — the queries, their pixels, the offsets, the cameras' priors — then what comes down in one copy —
// the candidate counts, the two candidate lists, the inlier flags — then, on the device only, the lane order and the search's result
// rows.  The state rows have pinned room of their own (two rows a camera: up and down); on the device they are the stage context's.
#define RB_CAMERA_BYTES 136                           // RelocBatchCam: the prior as GuidePose (128) + radius + padding
struct RbLayout { size_t query, xy, begin, cams, up_end, n_cand, cand_query, cand_row, inlier, down_end, order, match, total; };
static inline size_t rb_round(size_t bytes) { return (bytes + 255) / 256 * 256; }
static inline RbLayout rb_layout(size_t cameras, size_t queries) {
    RbLayout l;
    l.query = 0; l.xy = rb_round(32 * queries);
    l.begin = l.xy + rb_round(8 * queries);
    l.cams = l.begin + rb_round(4 * (cameras + 1));
    l.up_end = l.cams + rb_round(RB_CAMERA_BYTES * cameras);
    l.n_cand = l.up_end; l.cand_query = l.n_cand + rb_round(4 * cameras);
    l.cand_row = l.cand_query + rb_round(4 * queries);
    l.inlier = l.cand_row + rb_round(4 * queries);
    l.down_end = l.inlier + rb_round(queries);
    l.order = l.down_end; l.match = l.order + rb_round(4 * queries);
    l.total = l.match + rb_round(32 * queries);
    return l;
}
// a capacity that at least doubles when it grows: the first `need` as it is (`first` at least)
static inline size_t rb_grow(size_t cap, size_t need, size_t first) {
    if (need <= cap) return cap;
    size_t c = cap ? 2 * cap : first;
    return c < need ? need : c;
}
