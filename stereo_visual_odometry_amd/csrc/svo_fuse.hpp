// svo_fuse.hpp — the rules of the descriptor index's landmark fusion (include/svo.h, "Landmark fusion"): a call's refusals, the 3-D
// gate of rule 1, the map step of rule 4, the table over the `from` values that rule 5's sweep probes, and the layout of the
// scratch.  Plain C++ that a host compiler takes as it is, like svo_align.hpp and svo_retire.hpp, so that a stand-alone host program
// (tests/cpp/fuse_host.cpp) runs exactly the text svo_match_api.hip and the kernels (svo_kernels_fuse.hip) run.  The gate is f32
// (the translation units that include this are built with -ffp-contract=off; it has no product to contract anyway); everything else
// is integers: host and device agree in every bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_FUSE_HD __host__ __device__
#else
#define SVO_FUSE_HD
#endif

#define FUSE_MAX_ROWS 4096                            // include/svo.h: SVO_FUSE_MAX_ROWS, the rows of a source span
#define FUSE_MAX_LIST (1 << 20)                       // include/svo.h: SVO_FUSE_MAX_LIST, the entries of svo_desc_index_relabel's lists
#define FUSE_MAX_RATIO (1 << 20)                      // ratio_num, ratio_den: svo_reloc.hpp's SVO_RELOC_MAX_RATIO
#define FUSE_POINT_NONE (-1)                          // include/svo.h: SVO_POINT_NONE, the tag of a row without a point
#define FUSE_EMPTY (-1)                               // a slot of the table that holds no list position

// ---- a call's refusals.  The request is svo_fuse_params field by field; row_hi = -1 is the index's size, as everywhere
struct FuseRequest {
    int32_t src_lo, src_hi, dst_lo, dst_hi, relabel_lo, relabel_hi, max_dist, ratio_num, ratio_den;
    float radius;
};
enum FuseRefusal { FUSE_OK = 0, FUSE_SRC_RANGE, FUSE_DST_RANGE, FUSE_RELABEL_RANGE, FUSE_ROWS, FUSE_OVERLAP, FUSE_RADIUS, FUSE_MAX_DIST, FUSE_RATIO };

// do [a_lo, a_hi) and [b_lo, b_hi) share a row?  An empty span shares none; spans that touch (a_hi == b_lo) share none.
static inline bool fuse_spans_overlap(int a_lo, int a_hi, int b_lo, int b_hi) {
    return a_lo < a_hi && b_lo < b_hi && a_lo < b_hi && b_lo < a_hi;
}
// one span, resolved in place (-1 becomes size): svo_desc_index_match's row-range rule
static inline bool fuse_span_ok(int32_t& lo, int32_t& hi, int size) {
    if (hi == -1) hi = size;
    return lo >= 0 && hi <= size && lo <= hi;
}

// What svo_desc_index_match_near refuses: the two spans, resolved in place, and the radius.
static inline FuseRefusal fuse_check_search(FuseRequest& q, int size) {
    if (!fuse_span_ok(q.src_lo, q.src_hi, size)) return FUSE_SRC_RANGE;
    if (!fuse_span_ok(q.dst_lo, q.dst_hi, size)) return FUSE_DST_RANGE;
    if (q.src_hi - q.src_lo > FUSE_MAX_ROWS) return FUSE_ROWS;
    if (fuse_spans_overlap(q.src_lo, q.src_hi, q.dst_lo, q.dst_hi)) return FUSE_OVERLAP;
    if (!isfinite(q.radius) || q.radius < 0.f) return FUSE_RADIUS;
    return FUSE_OK;
}
// everything svo_desc_index_pair_near and svo_desc_index_fuse refuse
static inline FuseRefusal fuse_check(FuseRequest& q, int size) {
    if (const FuseRefusal e = fuse_check_search(q, size); e != FUSE_OK) return e;
    if (!fuse_span_ok(q.relabel_lo, q.relabel_hi, size)) return FUSE_RELABEL_RANGE;
    if (q.max_dist < 0 || q.max_dist > 256) return FUSE_MAX_DIST;
    if (q.ratio_num < 1 || q.ratio_num > FUSE_MAX_RATIO || q.ratio_den < 1 || q.ratio_den > FUSE_MAX_RATIO) return FUSE_RATIO;
    return FUSE_OK;
}

// ---- rule 1: the gate.  f32 throughout, every limit inclusive; a row without a point on either side admits nothing.
SVO_FUSE_HD static inline bool fuse_admits_axis(float p, float q, float radius) { return __builtin_fabsf(p - q) <= radius; }
SVO_FUSE_HD static inline bool fuse_admits(float px, float py, float pz, int32_t ptag, float qx, float qy, float qz, int32_t qtag, float radius) {
    return ptag != FUSE_POINT_NONE && qtag != FUSE_POINT_NONE && fuse_admits_axis(px, qx, radius) && fuse_admits_axis(py, qy, radius) &&
           fuse_admits_axis(pz, qz, radius);
}

// ---- rule 4: does the pair (from, to) map anything?  One with from == to is counted in n_same; a list entry like it is ignored.
SVO_FUSE_HD static inline bool fuse_maps(uint64_t from, uint64_t to) { return from != to; }

// ---- rule 5: the table.  A power of two of slots, at least 2 x the list's entries (load <= 1/2), each FUSE_EMPTY or a position of
// the (from, to) list.  The key of a slot is from[its position]: the list never changes while the table lives, and a slot changes
// between positions of one `from` value only, so no id value is a sentinel and the ids the sweep overwrites are never a key.
SVO_FUSE_HD static inline uint32_t fuse_table_slots(int32_t entries) {
    uint32_t t = 2;
    while (t < 2u * (uint32_t)entries) t *= 2;        // entries <= 2^20: t <= 2^21
    return t;
}
// where the probe of an id starts (splitmix64's finaliser: every bit of the id reaches the low bits), and where it goes next
SVO_FUSE_HD static inline uint32_t fuse_slot_first(uint64_t id, uint32_t mask) {
    uint64_t z = id + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)z & mask;
}
SVO_FUSE_HD static inline uint32_t fuse_slot_next(uint32_t slot, uint32_t mask) { return (slot + 1) & mask; }

// The two read-modify-writes of an insert as a sequential program does them; the kernel passes atomicCAS and atomicMin instead.
struct FusePlainSlot {
    int32_t cas(int32_t* p, int32_t expect, int32_t v) const { const int32_t old = *p; if (old == expect) *p = v; return old; }
    void min(int32_t* p, int32_t v) const { if (v < *p) *p = v; }
};

// Entry `pos` of the list into the table: an entry that maps nothing is ignored; an empty slot takes the position; a slot whose
// position has the same `from` value keeps the smaller position ("the smallest list position wins", whatever order the lanes
// arrive in); any other slot sends the probe on, wrapping.  -> false when the probe ran out of slots, which the table's size rules out.
template <class Slot>
SVO_FUSE_HD static inline bool fuse_table_insert(int32_t* table, uint32_t mask, const uint64_t* from, const uint64_t* to, int32_t pos, const Slot& slot_op) {
    const uint64_t id = from[pos];
    if (!fuse_maps(id, to[pos])) return true;
    uint32_t slot = fuse_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = fuse_slot_next(slot, mask)) {
        const int32_t old = slot_op.cas(&table[slot], FUSE_EMPTY, pos);
        if (old == FUSE_EMPTY) return true;           // the slot was empty and is this entry's now
        if (from[old] == id) { slot_op.min(&table[slot], pos); return true; }
    }
    return false;
}

// The list position that maps `id`, or -1.  An inserted value's probe never meets an empty slot before its own.
SVO_FUSE_HD static inline int32_t fuse_table_find(const int32_t* table, uint32_t mask, const uint64_t* from, uint64_t id) {
    uint32_t slot = fuse_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = fuse_slot_next(slot, mask)) {
        const int32_t at = table[slot];
        if (at == FUSE_EMPTY) return -1;
        if (from[at] == id) return at;
    }
    return -1;
}

// ---- the scratch of one call, in the index's maintenance scratch, every part rounded up to 256 bytes: what the kernels report, the
// (from, to) list of `entries` entries, and the table.  include/svo.h states `total`.
// The changed rows are counted over FUSE_COUNT_SLOTS cache lines — block b adds to slot b % FUSE_COUNT_SLOTS, the host sums — as the
// transform's counts are (svo_retire_internal.hpp): atomics on one address take their turns in the L2.
#define FUSE_COUNT_SLOTS 128
struct FuseCount { int32_t n_rows_relabelled, pad[15]; };
struct FuseCtl { int32_t n_same, n_fused, table_full, pad[13]; FuseCount counts[FUSE_COUNT_SLOTS]; };
static inline size_t fuse_round(size_t b) { return (b + 255) / 256 * 256; }
struct FuseLayout { size_t ctl, from, to, table, total; };
static inline FuseLayout fuse_layout(int32_t entries) {
    FuseLayout l;
    const size_t n = (size_t)entries;
    l.ctl = 0; l.from = fuse_round(sizeof(FuseCtl));
    l.to = l.from + fuse_round(8 * n);
    l.table = l.to + fuse_round(8 * n);
    l.total = l.table + fuse_round(4 * (size_t)fuse_table_slots(entries));
    return l;
}
