// svo_place_batch.hpp — the rules of the batched place candidates (include/svo.h, "Batched place candidates"): a call's own refusal,
// the table of (id, camera) pairs that one sweep probes for every camera at once, rule 3 over a camera's row of votes, and the
// layouts of the scratch and of the pinned staging.  Plain C++ that a host compiler takes as it is, like svo_place.hpp, so that a
// stand-alone host program (tests/cpp/place_batch_host.cpp) runs exactly the text svo_match_api.hip and the kernels
// (svo_kernels_place_batch.hip) run.  Integers only.  The offsets' rules are svo_reloc_batch.hpp's (rb_check_offsets), a slice's and
// the window's svo_place.hpp's, the hash svo_fuse.hpp's; there is no second copy of any.
#pragma once
#include "svo_place.hpp"
#include "svo_reloc_batch.hpp"

#define PB_MAX_CAMERAS 1024                           // include/svo.h: SVO_PLACE_BATCH_MAX_CAMERAS
#define PB_MAX_IDS (1 << 20)                          // include/svo.h: SVO_PLACE_BATCH_MAX_IDS, ids or queries of all cameras together
#define PB_MAX_BINS (1 << 24)                         // include/svo.h: SVO_PLACE_BATCH_MAX_BINS, cameras x bins of the tag window
#define PB_CAM_NONE (-1)                              // a list position beyond its camera's entries: in no set
static_assert(PB_MAX_CAMERAS == RB_MAX_CAMERAS && PB_MAX_IDS == RB_MAX_QUERIES && PLACE_MAX_IDS == RB_MAX_SLICE, "rb_check_offsets checks a place batch's offsets");

// ---- the call's own refusal, behind rb_check_offsets and place_check_*: the votes of all cameras are one array
enum PlaceBatchRefusal { PB_OK = 0, PB_BINS };
static inline int64_t pb_bins(int32_t tag_lo, int32_t tag_hi) { return (int64_t)tag_hi - (int64_t)tag_lo + 1; }
static inline PlaceBatchRefusal pb_check_bins(int n_cameras, int32_t tag_lo, int32_t tag_hi) {
    return (int64_t)n_cameras * pb_bins(tag_lo, tag_hi) > PB_MAX_BINS ? PB_BINS : PB_OK;     // 1024 x 2^20 at most: no overflow
}

// ---- the table.  fuse_table_slots(total) slots over the concatenated list, each PLACE_EMPTY or a list position.  The key of a
// position is the pair (ids[pos], camera of pos), read through the list, which is complete before the first insert and never
// changes, and the offsets (a camera's positions are consecutive): no id value is a sentinel.  The hash takes the id alone, so
// every camera's entry for one id lies on that id's probe sequence, and one walk from hash(id) to the first empty slot meets them
// all.  An insert that finds its own pair counts nothing: M is a set per camera.
// The two accesses of an insert as a sequential program does them; the kernel passes a plain load and an atomicCAS instead.
struct PbPlainSlot {
    int32_t peek(const int32_t* p) const { return *p; }
    int32_t cas(int32_t* p, int32_t expect, int32_t v) const { const int32_t old = *p; if (old == expect) *p = v; return old; }
};
// Entry `pos` of camera [lo, hi)'s positions into the table.  A slot is written once and never emptied, so a look that finds it
// taken needs no atomic (a stale look that finds it empty costs one compare-and-swap, which tells the truth); and a taken slot is
// the same camera's exactly when its position lies in [lo, hi), so only such a slot's id is read: walking over the other cameras'
// entries of one id, the bulk of the probe when many cameras share it, costs one sequential load a slot.
template <class Slot>
SVO_PLACE_HD static inline PlaceInsert pb_insert(int32_t* table, uint32_t mask, const uint64_t* ids, int32_t lo, int32_t hi, int32_t pos, const Slot& slot_op) {
    const uint64_t id = ids[pos];
    uint32_t slot = fuse_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = fuse_slot_next(slot, mask)) {
        int32_t old = slot_op.peek(&table[slot]);
        if (old == PLACE_EMPTY) old = slot_op.cas(&table[slot], PLACE_EMPTY, pos);
        if (old == PLACE_EMPTY) return PLACE_SET_NEW;
        if (old >= lo && old < hi && ids[old] == id) return PLACE_SET_DUPLICATE;
    }
    return PLACE_SET_FULL;                            // the table's size (load <= 1/2) rules it out
}
// hit(pos) for every position of the table whose id is `id`: one per camera that holds it.  An inserted pair's probe never meets an
// empty slot before its own, so the walk ends at the first empty slot.  Four slots a step: their loads, and then their ids', do not
// wait for one another; slots behind the first empty one are read and not used (the table has an empty slot in any mask + 1
// consecutive ones, so the walk ends before it meets a slot twice).
#define PB_VISIT_STEP 4
template <class Hit>
SVO_PLACE_HD static inline void pb_visit(const int32_t* table, uint32_t mask, const uint64_t* ids, uint64_t id, const Hit& hit) {
    uint32_t slot = fuse_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step += PB_VISIT_STEP, slot = (slot + PB_VISIT_STEP) & mask) {
        int32_t at[PB_VISIT_STEP];
        uint64_t key[PB_VISIT_STEP];
        for (int i = 0; i < PB_VISIT_STEP; i++) at[i] = table[(slot + (uint32_t)i) & mask];
        for (int i = 0; i < PB_VISIT_STEP; i++) key[i] = at[i] != PLACE_EMPTY ? ids[at[i]] : 0;
        for (int i = 0; i < PB_VISIT_STEP; i++) {
            if (at[i] == PLACE_EMPTY) return;
            if (key[i] == id) hit(at[i]);
        }
    }
}

// ---- rule 3 over one camera's row of votes, without a key list.  The keys emitted decrease strictly, so a bin whose key is not
// below the last emitted one has been emitted or suppressed; any other bin is in P exactly when no emitted place suppresses it
// (a place suppresses itself: separation >= 0).  That is place_pick's P round by round.
SVO_PLACE_HD static inline bool pb_in_p(uint64_t key, uint64_t last_key, const int32_t* chosen, int n_chosen, int32_t separation) {
    if (n_chosen > 0 && key >= last_key) return false;
    const int32_t bin = place_key_bin(key);
    for (int i = 0; i < n_chosen; i++)
        if (place_suppresses(bin, chosen[i], separation)) return false;
    return true;
}
// a camera's bin: its own votes and the three fields every camera shares
SVO_PLACE_HD static inline PlaceBin pb_bin(int32_t votes, const PlaceBin& shared) { return PlaceBin{votes, shared.rows, shared.first_inv, shared.end}; }
// Rule 3 as a sequential program; the kernel runs the same rounds with a block-wide maximum.  -> the places' number
static inline int pb_pick(const int32_t* votes, const PlaceBin* shared, int32_t n_bins, int32_t tag_lo, int32_t min_votes, int32_t separation,
                          int32_t max_places, PlaceOut* out, int32_t* n_tags_voted) {
    int32_t voted = 0;
    for (int32_t b = 0; b < n_bins; b++) voted += votes[b] >= 1;
    *n_tags_voted = voted;
    int32_t chosen[PLACE_MAX_PLACES];
    int n_places = 0;
    uint64_t last_key = 0;
    while (n_places < max_places) {
        uint64_t best = 0;
        for (int32_t b = 0; b < n_bins; b++) {
            if (votes[b] < min_votes || votes[b] < 1) continue;
            const uint64_t key = place_key(votes[b], b);
            if (key > best && pb_in_p(key, last_key, chosen, n_places, separation)) best = key;
        }
        if (best == 0) break;
        last_key = best;
        chosen[n_places] = place_key_bin(best);
        out[n_places] = place_out(chosen[n_places], tag_lo, pb_bin(votes[chosen[n_places]], shared[chosen[n_places]]));
        n_places++;
    }
    return n_places;
}

// ---- the scratch of one call, in the index's maintenance scratch, every part rounded up to 256 bytes (include/svo.h states
// `total`): what comes down in one copy — a record per camera, then the places (max_places a camera; tag_votes_batch: none), or the
// shared bins and the votes — then the offsets, the concatenated id list, the camera of every list position, and the table.
struct PbCam { int32_t n_landmarks, n_tags_voted, n_places, set_full; };
struct PbLayout { size_t cams, places, bins, votes, down_end, begin, list, cam, table, total; };
static inline PbLayout pb_layout(size_t cameras, size_t entries, size_t n_bins, size_t max_places) {
    PbLayout l;
    l.cams = 0; l.places = fuse_round(sizeof(PbCam) * cameras);
    l.bins = l.places + fuse_round(sizeof(PlaceOut) * max_places * cameras);
    l.votes = l.bins + fuse_round(sizeof(PlaceBin) * n_bins);
    l.down_end = l.votes + fuse_round(4 * cameras * n_bins);
    l.begin = l.down_end; l.list = l.begin + fuse_round(4 * (cameras + 1));
    l.cam = l.list + fuse_round(8 * entries);
    l.table = l.cam + fuse_round(4 * entries);
    l.total = l.table + fuse_round(4 * (size_t)fuse_table_slots((int32_t)entries));
    return l;
}
// The pinned staging of one call: what goes up in one copy — the offsets, then the ids (places_batch sends its queries through the
// batched relocalisation's staging instead) — and room for what comes down: the records and the places, or all of [cams, down_end).
struct PbStage { size_t begin, ids, up_end, down, total; };
static inline PbStage pb_stage(const PbLayout& l, size_t cameras, size_t entries, bool pick) {
    PbStage s;
    s.begin = 0; s.ids = fuse_round(4 * (cameras + 1));
    s.up_end = s.ids + fuse_round(8 * entries);
    s.down = s.up_end;
    s.total = s.down + (pick ? l.bins : l.down_end);
    return s;
}
