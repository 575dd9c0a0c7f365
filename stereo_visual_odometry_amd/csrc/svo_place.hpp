// svo_place.hpp — the rules of the descriptor index's place candidates (include/svo.h, "Place candidates"): a call's refusals, the set
// M of recognised landmark ids that rule 2's sweep probes, a tag's bin as the sweep accumulates it, the order and the suppression of
// rule 3, and the layout of the scratch.  Plain C++ that a host compiler takes as it is, like svo_fuse.hpp, so that a stand-alone
// host program (tests/cpp/place_host.cpp) runs exactly the text svo_match_api.hip and the kernels (svo_kernels_place.hip) run.
// Integers only: host and device agree in every bit.  The hash is svo_fuse.hpp's; there is no second one.
#pragma once
#include "svo_fuse.hpp"

#define SVO_PLACE_HD SVO_FUSE_HD

#define PLACE_MAX_TAGS (1 << 20)                      // include/svo.h: SVO_PLACE_MAX_TAGS, the bins of one call
#define PLACE_MAX_PLACES 64                           // include/svo.h: SVO_PLACE_MAX_PLACES
#define PLACE_MAX_IDS 4096                            // include/svo.h: SVO_PLACE_MAX_IDS, the entries of an id list (M has no more ids)
#define PLACE_MAX_RATIO (1 << 20)                     // ratio_num, ratio_den: svo_reloc.hpp's SVO_RELOC_MAX_RATIO
#define PLACE_MAX_ROWS (1 << 24)                      // include/svo.h: SVO_MATCH_MAX_ROWS, the rows of an index
#define PLACE_EMPTY (-1)                              // a slot of the set that holds no list position

// ---- a call's refusals.  The request is svo_place_params field by field; row_hi = -1 is the index's size, as everywhere
struct PlaceRequest { int32_t row_lo, row_hi, max_dist, ratio_num, ratio_den, tag_lo, tag_hi, min_votes, separation, max_places; };
enum PlaceRefusal { PLACE_OK = 0, PLACE_ROW_RANGE, PLACE_TAG_LO, PLACE_TAG_HI, PLACE_TAG_SPAN, PLACE_MIN_VOTES, PLACE_SEPARATION, PLACE_MAX_PLACES_RANGE,
                    PLACE_MAX_DIST, PLACE_RATIO };

// What svo_desc_index_tag_votes refuses: the row range, resolved in place, and the tag span (at most PLACE_MAX_TAGS bins; the
// difference is taken in 64 bits, tag_hi may be INT32_MAX).
static inline PlaceRefusal place_check_votes(PlaceRequest& q, int size) {
    if (!fuse_span_ok(q.row_lo, q.row_hi, size)) return PLACE_ROW_RANGE;
    if (q.tag_lo < 0) return PLACE_TAG_LO;
    if (q.tag_hi < q.tag_lo) return PLACE_TAG_HI;
    if ((int64_t)q.tag_hi - (int64_t)q.tag_lo + 1 > PLACE_MAX_TAGS) return PLACE_TAG_SPAN;
    return PLACE_OK;
}
// everything svo_desc_index_places_from_ids refuses (rules 2 - 3) ...
static inline PlaceRefusal place_check_pick(PlaceRequest& q, int size) {
    if (const PlaceRefusal e = place_check_votes(q, size); e != PLACE_OK) return e;
    if (q.min_votes < 1) return PLACE_MIN_VOTES;
    if (q.separation < 0) return PLACE_SEPARATION;
    if (q.max_places < 1 || q.max_places > PLACE_MAX_PLACES) return PLACE_MAX_PLACES_RANGE;
    return PLACE_OK;
}
// ... and svo_desc_index_places (rules 1 - 3): with the selection's own
static inline PlaceRefusal place_check(PlaceRequest& q, int size) {
    if (const PlaceRefusal e = place_check_pick(q, size); e != PLACE_OK) return e;
    if (q.max_dist < 0 || q.max_dist > 256) return PLACE_MAX_DIST;
    if (q.ratio_num < 1 || q.ratio_num > PLACE_MAX_RATIO || q.ratio_den < 1 || q.ratio_den > PLACE_MAX_RATIO) return PLACE_RATIO;
    return PLACE_OK;
}

// ---- rule 1's set M.  fuse_table_slots(n) slots, each PLACE_EMPTY or a position of the id list; the key of a slot is ids[its
// position], so no id value is a sentinel (0 and 2^64 - 1 are ids like any other).  A duplicate of an id already in the set is
// found and dropped: M is a set.
enum PlaceInsert { PLACE_SET_FULL = 0, PLACE_SET_NEW = 1, PLACE_SET_DUPLICATE = 2 };
struct PlacePlainSlot {
    int32_t cas(int32_t* p, int32_t expect, int32_t v) const { const int32_t old = *p; if (old == expect) *p = v; return old; }
};
// Entry `pos` of the list into the set; the kernel passes an atomicCAS on LDS.  ids[] is complete before the first insert.
template <class Slot>
SVO_PLACE_HD static inline PlaceInsert place_set_insert(int32_t* table, uint32_t mask, const uint64_t* ids, int32_t pos, const Slot& slot_op) {
    const uint64_t id = ids[pos];
    uint32_t slot = fuse_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = fuse_slot_next(slot, mask)) {
        const int32_t old = slot_op.cas(&table[slot], PLACE_EMPTY, pos);
        if (old == PLACE_EMPTY) return PLACE_SET_NEW;
        if (ids[old] == id) return PLACE_SET_DUPLICATE;
    }
    return PLACE_SET_FULL;                            // the table's size (load <= 1/2) rules it out
}
// is `id` in M?  An inserted value's probe never meets an empty slot before its own.
SVO_PLACE_HD static inline bool place_set_has(const int32_t* table, uint32_t mask, const uint64_t* ids, uint64_t id) {
    uint32_t slot = fuse_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = fuse_slot_next(slot, mask)) {
        const int32_t at = table[slot];
        if (at == PLACE_EMPTY) return false;
        if (ids[at] == id) return true;
    }
    return false;
}

// ---- rule 2: one bin per tag of [tag_lo, tag_hi], 16 bytes, all zero going in.  Every field is a sum or a maximum, so integer
// atomics in any order give the same bits.  The smallest row is kept as the LARGEST of PLACE_MAX_ROWS - r (r < 2^24: 1 at least),
// so that zero means "no row" and one memset clears a bin.
struct PlaceBin { int32_t votes, rows, first_inv, end; };
SVO_PLACE_HD static inline bool place_tag_qualifies(int32_t tag, int32_t tag_lo, int32_t tag_hi) { return tag >= tag_lo && tag <= tag_hi; }
SVO_PLACE_HD static inline int32_t place_first_inv(int32_t row) { return PLACE_MAX_ROWS - row; }
// a bin's row_first and row_end as the caller sees them; a bin without rows: 0 and 0
SVO_PLACE_HD static inline int32_t place_row_first(const PlaceBin& b) { return b.first_inv ? PLACE_MAX_ROWS - b.first_inv : 0; }
SVO_PLACE_HD static inline int32_t place_row_end(const PlaceBin& b) { return b.end; }
// one row into its bin as a sequential program does it
static inline void place_bin_add(PlaceBin& b, int32_t row, bool in_m) {
    b.rows += 1; b.votes += in_m ? 1 : 0;
    if (place_first_inv(row) > b.first_inv) b.first_inv = place_first_inv(row);
    if (row + 1 > b.end) b.end = row + 1;
}

// ---- rule 3.  The order as one key: the larger votes first, at equal votes the smaller bin.  votes >= 1, so no key of a bin in P
// is 0, and 0 marks an entry that has been removed.
SVO_PLACE_HD static inline uint64_t place_key(int32_t votes, int32_t bin) { return (uint64_t)(uint32_t)votes << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)bin); }
SVO_PLACE_HD static inline int32_t place_key_bin(uint64_t key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)key); }
SVO_PLACE_HD static inline int32_t place_key_votes(uint64_t key) { return (int32_t)(key >> 32); }
// does the place emitted at bin `chosen` remove bin t from P?  Both in 0 .. 2^20: the difference is exact
SVO_PLACE_HD static inline bool place_suppresses(int32_t t, int32_t chosen, int32_t separation) {
    const int32_t d = t > chosen ? t - chosen : chosen - t;
    return d <= separation;
}
// One place of the result, 32 bytes: include/svo.h's svo_place
struct PlaceOut { int32_t tag, votes, rows, row_first, row_end, reserved[3]; };
SVO_PLACE_HD static inline PlaceOut place_out(int32_t bin, int32_t tag_lo, const PlaceBin& b) {
    return PlaceOut{tag_lo + bin, b.votes, b.rows, place_row_first(b), place_row_end(b), {0, 0, 0}};
}
// Rule 3 as a sequential program: keys[0 .. n) are place_key of the bins of P in any order and are consumed (removed entries become
// 0); out receives at most max_places places -> their number.  The kernel runs the same rounds with a block-wide maximum.
static inline int place_pick(uint64_t* keys, int32_t n, const PlaceBin* bins, int32_t tag_lo, int32_t separation, int32_t max_places, PlaceOut* out) {
    int n_places = 0;
    int32_t last = -1;
    while (n_places < max_places) {
        uint64_t best = 0;
        for (int32_t e = 0; e < n; e++) {
            if (keys[e] == 0) continue;
            if (last >= 0 && place_suppresses(place_key_bin(keys[e]), last, separation)) { keys[e] = 0; continue; }
            if (keys[e] > best) best = keys[e];
        }
        if (best == 0) break;
        last = place_key_bin(best);
        out[n_places++] = place_out(last, tag_lo, bins[last]);
    }
    return n_places;
}

// ---- the scratch of one call, in the index's maintenance scratch, every part rounded up to 256 bytes: what the kernels report (the
// counts and the places), the id list (or the candidates' rows) of at most PLACE_MAX_IDS entries, the bins, and rule 3's list of keys.
// include/svo.h states `total`.
struct PlaceCtl { int32_t n_landmarks, n_tags_voted, n_list, n_places, set_full, pad[3]; PlaceOut places[PLACE_MAX_PLACES]; };
struct PlaceLayout { size_t ctl, ids, bins, keys, total; };
static inline PlaceLayout place_layout(int32_t n_ids, int32_t n_bins, bool pick) {
    PlaceLayout l;
    l.ctl = 0; l.ids = fuse_round(sizeof(PlaceCtl));
    l.bins = l.ids + fuse_round(8 * (size_t)n_ids);
    l.keys = l.bins + fuse_round(sizeof(PlaceBin) * (size_t)n_bins);
    l.total = l.keys + (pick ? fuse_round(8 * (size_t)n_bins) : 0);
    return l;
}
// the LDS of one sweep block: the id list, then the set's slots
static inline size_t place_lds_bytes(int32_t n_ids) { return 8 * (size_t)(n_ids > 0 ? n_ids : 1) + 4 * (size_t)fuse_table_slots(n_ids); }
