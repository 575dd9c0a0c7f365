// svo_desc.hpp — the integer rules of the steered BRIEF descriptor (include/svo.h, "Binary descriptors"): the direction tables, the
// test pattern, the bin rule and the rotation of a pattern point.  Plain C++ that a host compiler takes as it is, like svo_prior.hpp,
// so that a stand-alone host program (tests/cpp/desc_host.cpp) runs exactly the text k_track_desc and k_describe_points
// (svo_kernels_desc.hip) run.  Integers only: host and device agree in every bit.
#pragma once
#include <stdint.h>
#include "svo_brief_pattern.hpp"

#if defined(__HIPCC__)
#define SVO_DESC_HD __host__ __device__
#else
#define SVO_DESC_HD
#endif
// A table is ordinary constant data to the host, and device-resident constant data to the device code that indexes it with a lane.
#if defined(__HIP_DEVICE_COMPILE__)
#define SVO_DESC_TABLE static __device__ const
#else
#define SVO_DESC_TABLE static const
#endif

#define SVO_DESC_BINS 30          // 12 degrees each
#ifndef SVO_DESC_BYTES
#define SVO_DESC_BYTES 32         // 256 bits (include/svo.h defines it for callers)
#endif
#define SVO_DESC_HALF 15          // the patch is (2 * 15 + 1)^2
#define SVO_DESC_DISC 240         // the moments run over dx^2 + dy^2 <= 240
#define SVO_DESC_REACH 13         // |coordinate| of a pattern point, before and after rotation

// round(2^14 cos(12 k deg)), round(2^14 sin(12 k deg)), k = 0 .. 29: literals, so no libm decides a bit
SVO_DESC_TABLE int32_t SVO_DESC_COS[SVO_DESC_BINS] = {16384, 16026, 14968, 13255, 10963, 8192, 5063, 1713, -1713, -5063, -8192, -10963, -13255, -14968, -16026,
                                                      -16384, -16026, -14968, -13255, -10963, -8192, -5063, -1713, 1713, 5063, 8192, 10963, 13255, 14968, 16026};
SVO_DESC_TABLE int32_t SVO_DESC_SIN[SVO_DESC_BINS] = {0, 3406, 6664, 9630, 12176, 14189, 15582, 16294, 16294, 15582, 14189, 12176, 9630, 6664, 3406,
                                                      0, -3406, -6664, -9630, -12176, -14189, -15582, -16294, -16294, -15582, -14189, -12176, -9630, -6664, -3406};
// test i = (ax, ay, bx, by) at [4 i .. 4 i + 3]
SVO_DESC_TABLE int8_t SVO_BRIEF_PATTERN[4 * SVO_BRIEF_TESTS] = {SVO_BRIEF_PATTERN_VALUES};

// the centre rule: mask_keeps' rounding (truncation toward zero of v + 0.5f), clamped into [0, n - 1].  v must be finite.
SVO_DESC_HD static inline int desc_centre(float v, int n) {
    int i = (int)(v + 0.5f);
    i = i < n - 1 ? i : n - 1;
    return i > 0 ? i : 0;
}
// REFLECT_101 of a coordinate within 15 of [0, n), n >= 16: one reflection
SVO_DESC_HD static inline int desc_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// what bin k scores for the moments (|m| < 2^21, so the products need 36 bits)
SVO_DESC_HD static inline int64_t desc_score(int32_t m10, int32_t m01, int k) {
    return (int64_t)m10 * (int64_t)SVO_DESC_COS[k] + (int64_t)m01 * (int64_t)SVO_DESC_SIN[k];
}
// does (score b, bin kb) beat (score a, bin ka)?  The larger score; at equal scores the smaller bin.
SVO_DESC_HD static inline bool desc_beats(int64_t b, int kb, int64_t a, int ka) { return b > a || (b == a && kb < ka); }
// the bin rule: the smallest k that maximises the score
SVO_DESC_HD static inline int desc_bin(int32_t m10, int32_t m01) {
    int best = 0;
    int64_t top = desc_score(m10, m01, 0);
    for (int k = 1; k < SVO_DESC_BINS; k++) {
        const int64_t s = desc_score(m10, m01, k);
        if (desc_beats(s, k, top, best)) { top = s; best = k; }
    }
    return best;
}
// a pattern point rotated by the bin: rounding shift (arithmetic) of the Q14 products
SVO_DESC_HD static inline void desc_rotate(int px, int py, int bin, int& rx, int& ry) {
    const int32_t c = SVO_DESC_COS[bin], s = SVO_DESC_SIN[bin];
    rx = (px * c - py * s + 8192) >> 14;
    ry = (px * s + py * c + 8192) >> 14;
}
