// svo_retire.hpp — the rules of the descriptor index's maintenance calls (include/svo.h, "Index maintenance"): which rows of a scope
// a retire rule keeps alive, the sorted id list's search, the hash and the probe order of the latest-per-id table, the size of that
// table and of the scratch, and the arithmetic that moves a point.  Plain C++ that a host compiler takes as it is, like svo_match.hpp
// and svo_reloc.hpp, so that a stand-alone host program (tests/cpp/desc_retire_host.cpp) runs exactly the text the kernels
// (svo_kernels_retire.hip) and svo_match_api.hip run.  The retire rule is integers only; the transform is f64 with every operation
// rounded on its own (the translation units that include this are built with -ffp-contract=off).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_RETIRE_HD __host__ __device__
#else
#define SVO_RETIRE_HD
#endif

// include/svo.h: SVO_RETIRE_*, SVO_POINT_NONE
#define RETIRE_BY_TAG 1u
#define RETIRE_BY_IDS 2u
#define RETIRE_LATEST_PER_ID 4u
#define RETIRE_SCOPE 8u
#define RETIRE_ALL_FLAGS 15u
#define RETIRE_POINT_NONE (-1)
#define RETIRE_MAX_IDS (1 << 24)
#define RETIRE_MAX_ROWS (1 << 24)
#define RETIRE_DEFAULT_SLAB (1 << 18)                 // rows of one slab of the compaction unless svo_desc_index_set_retire_slab_rows says otherwise
#define RETIRE_ROW_BYTES 56                           // descriptor 32 + id 8 + point 16: what a row of the bounce buffer takes
#define RETIRE_BLOCK 256                              // lanes of every block of the retire kernels; the scan has two levels of it
#define RETIRE_EMPTY (-1)                             // a slot of the latest-per-id table that holds no row

// alive1 of a row of the scope: tag is read only with BY_TAG, listed (is the row's id in the list?) only with BY_IDS
SVO_RETIRE_HD static inline bool retire_alive1(uint32_t flags, int32_t tag, int32_t tag_lo, int32_t tag_hi, bool listed) {
    if (flags & RETIRE_SCOPE) return false;
    if ((flags & RETIRE_BY_TAG) && !(tag_lo <= tag && tag <= tag_hi)) return false;
    if ((flags & RETIRE_BY_IDS) && listed) return false;
    return true;
}

// is id in sorted[0 .. n), ascending without duplicates?
SVO_RETIRE_HD static inline bool retire_id_listed(const uint64_t* sorted, int32_t n, uint64_t id) {
    int32_t lo = 0, hi = n;                           // the first entry >= id lies in [lo, hi]
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && sorted[lo] == id;
}

// The latest-per-id table: a power of two of slots, at least 2 x the scope's rows (load <= 1/2), each RETIRE_EMPTY or a row number.
// The key of a slot is ids[its row]: a slot changes between rows of one id only, so no id value is a sentinel.
SVO_RETIRE_HD static inline uint32_t retire_table_slots(int32_t scope_rows) {
    uint32_t t = 2;
    while (t < 2u * (uint32_t)scope_rows) t *= 2;     // scope_rows <= 2^24: t <= 2^25
    return t;
}
// where the probe of an id starts (the finaliser of splitmix64, every bit of the id reaches the low bits), and where it goes next
SVO_RETIRE_HD static inline uint32_t retire_slot_first(uint64_t id, uint32_t mask) {
    uint64_t z = id + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)z & mask;
}
SVO_RETIRE_HD static inline uint32_t retire_slot_next(uint32_t slot, uint32_t mask) { return (slot + 1) & mask; }

// The transform of svo_desc_index_transform_points, coordinate c of the point (x, y, z) through T (4 x 4, row-major): the formula of
// svo_desc_index_add_frame_points (svo_reloc.hpp, reloc_map_point), restated here for the device.
SVO_RETIRE_HD static inline float retire_map_coord(const double* T, int c, float x, float y, float z) {
    double v = T[4 * c] * (double)x;
    v = v + T[4 * c + 1] * (double)y;
    v = v + T[4 * c + 2] * (double)z;
    v = v + T[4 * c + 3];
    return (float)v;
}
// is the row selected: a point, and its tag inside the window?
SVO_RETIRE_HD static inline bool retire_tag_selected(int32_t tag, int32_t tag_lo, int32_t tag_hi) {
    return tag != RETIRE_POINT_NONE && tag_lo <= tag && tag <= tag_hi;
}
// finite without <math.h>: the exponent bits of an f32 are not all ones
SVO_RETIRE_HD static inline bool retire_finite_bits(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

// Where the parts of the scratch of one retire call start, in bytes, each part rounded up to 256 (include/svo.h states `total` as the
// bound): the keep flags, the scope's ranks (one more than its rows), the two levels of block counts, the table (LATEST_PER_ID
// only), the sorted id list (BY_IDS only) and the bounce buffer of one slab (no longer than the rows that may move).
struct RetireLayout { size_t keep, rank, counts, table, ids, bounce, total; };
static inline size_t retire_round(size_t bytes) { return (bytes + 255) / 256 * 256; }
static inline RetireLayout retire_layout(int32_t scope_rows, int32_t moving_rows, int32_t n_ids, int32_t slab_rows, uint32_t flags) {
    RetireLayout l;
    const size_t m = (size_t)scope_rows, blocks = (m + RETIRE_BLOCK - 1) / RETIRE_BLOCK;
    const size_t slab = (size_t)(moving_rows < slab_rows ? moving_rows : slab_rows);
    l.keep = 0; l.rank = retire_round(m);
    l.counts = l.rank + retire_round(4 * (m + 1));
    l.table = l.counts + retire_round(4 * (blocks + RETIRE_BLOCK + 1));
    l.ids = l.table + ((flags & RETIRE_LATEST_PER_ID) ? retire_round(4 * (size_t)retire_table_slots(scope_rows)) : 0);
    l.bounce = l.ids + ((flags & RETIRE_BY_IDS) ? retire_round(8 * (size_t)n_ids) : 0);
    l.total = l.bounce + retire_round(RETIRE_ROW_BYTES * slab);
    return l;
}
