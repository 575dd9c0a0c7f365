// svo_reloc.hpp — the rules of the descriptor index's relocaliser (include/svo.h, "Relocalisation"): the point row of an index, the
// acceptance test of a search result, the order among accepted queries of one landmark, and the transform of an observation's point
// into the map.  Plain C++ that a host compiler takes as it is, like svo_match.hpp, so that a stand-alone host program
// (tests/cpp/reloc_select_host.cpp) runs exactly the text k_reloc_select (svo_kernels_reloc.hip) and svo_match_api.hip run.  The
// selection is integers only: host and device agree in every bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_RELOC_HD __host__ __device__
#else
#define SVO_RELOC_HD
#endif

#define SVO_RELOC_MAX_QUERIES 4096                    // queries of one call: one staged search, one block of k_reloc_select
#define SVO_RELOC_POINT_NONE (-1)                     // include/svo.h: SVO_POINT_NONE, the tag of a row without a point
#define SVO_RELOC_MAX_RATIO (1 << 20)                 // ratio_num, ratio_den: 1 .. 2^20, so that 257 * either stays far inside an int32

// One row of an index's points, 16 bytes: the landmark in the map frame and the caller's tag (>= 0), or SVO_RELOC_POINT_NONE
struct RelocPoint { float x, y, z; int32_t tag; };

// what rule 1 compares a search result with
struct RelocRule { int32_t max_dist, ratio_num, ratio_den; };

// Rule 1: a query is accepted when it has a best row, that row carries a point, the distance is at most max_dist, and
// dist * ratio_den < dist2 * ratio_num — strictly.  dist2 is SVO_MATCH_NO_DIST (257) where no other landmark is in the range.
SVO_RELOC_HD static inline bool reloc_accept(int32_t row, int32_t tag, int32_t dist, int32_t dist2, const RelocRule& r) {
    return row >= 0 && tag != SVO_RELOC_POINT_NONE && dist <= r.max_dist && dist * r.ratio_den < dist2 * r.ratio_num;
}

// Rule 2: among accepted queries of one id the smallest (dist, j) survives.  The pair as one key: j < 4096 takes 12 bits of the 16.
SVO_RELOC_HD static inline uint32_t reloc_key(int32_t dist, int32_t j) { return (uint32_t)dist << 16 | (uint32_t)j; }
SVO_RELOC_HD static inline int32_t reloc_key_query(uint32_t key) { return (int32_t)(key & 0xFFFFu); }
// does accepted query a lose to accepted query b?  (keys of different queries differ, so a never loses to itself)
SVO_RELOC_HD static inline bool reloc_loses(uint64_t id_a, uint32_t key_a, uint64_t id_b, uint32_t key_b) { return id_a == id_b && key_b < key_a; }

// The transform of svo_desc_index_add_frame_points: a point p of the T0 left camera frame into the map through T (4 x 4, row-major,
// the pose of that camera in the map).  Per coordinate f32(T[4r] x + T[4r+1] y + T[4r+2] z + T[4r+3]) in f64, left to right; the
// translation units that include this are built without contraction (-ffp-contract=off), so no product fuses with a sum.
SVO_RELOC_HD static inline void reloc_map_point(const double T[16], const float p[3], float out[3]) {
    for (int r = 0; r < 3; r++) {
        double v = T[4 * r] * (double)p[0];
        v = v + T[4 * r + 1] * (double)p[1];
        v = v + T[4 * r + 2] * (double)p[2];
        v = v + T[4 * r + 3];
        out[r] = (float)v;
    }
}
