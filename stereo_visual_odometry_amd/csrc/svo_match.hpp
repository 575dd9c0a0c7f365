// svo_match.hpp — the integer rules of the descriptor index's 2-nearest-neighbour search (include/svo.h, "Descriptor index"): the
// packed key, the streaming update of one lane's state and the merge of two partial states.  Plain C++ that a host compiler takes as
// it is, like svo_desc.hpp, so that a stand-alone host program (tests/cpp/desc_match_host.cpp) runs exactly the text k_desc_match and
// k_desc_match_merge (svo_kernels_match.hip) run.  Integers only: host and device agree in every bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_MATCH_HD __host__ __device__
#else
#define SVO_MATCH_HD
#endif

#define SVO_MATCH_ROW_BITS 24                         // a row number fits 24 bits: an index holds at most 1 << 24 rows
#define SVO_MATCH_MAX_ROWS (1 << SVO_MATCH_ROW_BITS)
#define SVO_MATCH_DIST_NONE 257                       // include/svo.h: SVO_MATCH_NO_DIST, one past the largest distance (256)

// The packed key of (distance, row): dist << 24 | row.  Keys compare as the definition's (dist, row) pairs compare — the smaller
// distance first, at equal distances the smaller row — and keys of different rows differ.  A distance runs 0 .. 256, nine bits,
// so a key needs 33 bits and is carried in 64.
typedef uint64_t match_key;
// "no row": above every key of a row, and its distance field reads SVO_MATCH_DIST_NONE
#define SVO_MATCH_KEY_NONE ((match_key)SVO_MATCH_DIST_NONE << SVO_MATCH_ROW_BITS)

SVO_MATCH_HD static inline match_key match_make_key(uint32_t dist, uint32_t row) { return (match_key)dist << SVO_MATCH_ROW_BITS | row; }
SVO_MATCH_HD static inline uint32_t match_key_dist(match_key k) { return (uint32_t)(k >> SVO_MATCH_ROW_BITS); }
SVO_MATCH_HD static inline bool match_key_none(match_key k) { return k >= SVO_MATCH_KEY_NONE; }
// the row of a key, -1 for "no row"
SVO_MATCH_HD static inline int32_t match_key_row(match_key k) { return match_key_none(k) ? -1 : (int32_t)(k & (SVO_MATCH_MAX_ROWS - 1)); }

// What is known of a set of rows S already seen.  The invariant both rules below keep:
//   k1  = the smallest key of S (SVO_MATCH_KEY_NONE for the empty set), id1 = the id of its row (0 for the empty set),
//   k2  = the smallest key of S among rows whose id differs from id1 (SVO_MATCH_KEY_NONE if there is none).
struct MatchState {
    match_key k1, k2;
    uint64_t id1;
};
SVO_MATCH_HD static inline MatchState match_empty() { return MatchState{SVO_MATCH_KEY_NONE, SVO_MATCH_KEY_NONE, 0}; }

// Streaming update: S gains one row (k, id), k not in S.
//  k < k1, another id: the old best is now the smallest key with an id other than the best's (every other key of S is larger).
//  k < k1, the same id: the rows with another id are the same set as before, k2 stands.
//  otherwise the best stands, and the row competes for k2 if its id differs from the best's.
SVO_MATCH_HD static inline void match_update(MatchState& s, match_key k, uint64_t id) {
    if (k < s.k1) {
        if (id != s.id1) s.k2 = s.k1;
        s.k1 = k; s.id1 = id;
    } else if (id != s.id1 && k < s.k2) {
        s.k2 = k;
    }
}

// Merge of the states of two DISJOINT row sets.  The best is the smaller k1 (w, the other side is l).  The second is the smallest of
// the other three keys whose row's id differs from w.id1:
//  w.k2 qualifies by w's invariant;
//  l.id1 != w.id1: l.k1 qualifies, and it is below l.k2, which drops out;
//  l.id1 == w.id1: l.k1 does not, and l.k2 is by l's invariant the smallest key of l's set with an id other than w.id1.
// So only the id of each side's best is needed.  Symmetric in its arguments; an empty side changes nothing.
SVO_MATCH_HD static inline MatchState match_merge(const MatchState& a, const MatchState& b) {
    const bool a_wins = a.k1 <= b.k1;                 // equal only when both are empty
    const match_key w_k1 = a_wins ? a.k1 : b.k1, w_k2 = a_wins ? a.k2 : b.k2, l_k1 = a_wins ? b.k1 : a.k1, l_k2 = a_wins ? b.k2 : a.k2;
    const uint64_t w_id1 = a_wins ? a.id1 : b.id1;    // field by field: values to select, no address of a state taken
    const match_key other = a.id1 != b.id1 ? l_k1 : l_k2;
    return MatchState{w_k1, other < w_k2 ? other : w_k2, w_id1};
}

// ---- the capacity rule of the index's growable buffers (svo_match_api.hip: grow), host only.  A buffer of `cap` units that must
// hold `need`: it never shrinks; when it grows it doubles from `first` (from twice its size, once it has one) until the need fits, so
// a buffer allocates O(log) times and the ones it has outgrown sum to less than the one in use; up to `clamp` (0: none) the
// doubling stops at the clamp.  So need <= capacity < max(2 * need, first + 1) for the largest need so far.
#include <stddef.h>
static inline size_t match_grow_capacity(size_t cap, size_t need, size_t first, size_t clamp) {
    if (need <= cap) return cap;
    size_t c = cap ? 2 * cap : first;
    while (c < need) c *= 2;
    return clamp && need <= clamp && c > clamp ? clamp : c;
}
