// svo_guide.hpp — the rules of the guided search (include/svo.h, "Guided search"): the projection of an index row's point with a
// pose prior, and the pixel gate between a row's projection and a query.  Plain C++ that a host compiler takes as it is, like
// svo_prior.hpp and svo_reloc.hpp, so that a stand-alone host program (tests/cpp/guide_host.cpp) runs exactly the text
// k_guide_project and k_desc_match_guided (svo_kernels_guide.hip) and the index's host code run.  The projection is f64 with every
// product, quotient and sum rounded on its own — the translation units that include this are built without contraction
// (-ffp-contract=off) — and the gate is f32, so host and device agree in every bit.
#pragma once
#include <stdint.h>

#ifndef SVO_HD
#if defined(__HIPCC__)
#define SVO_HD __host__ __device__
#else
#define SVO_HD
#endif
#endif

#define SVO_GUIDE_POINT_NONE (-1)                     // include/svo.h: SVO_POINT_NONE, the tag of a row without a point

// The prior as the projection reads it: x_cam = R X_map + t, and the four entries of the camera matrix it uses (K[0], K[2], K[4],
// K[5]) widened to f64.
struct GuidePose { double R[9], t[3], fx, cx, fy, cy; };

static inline GuidePose guide_pose(const double R[9], const double t[3], const float K[9]) {
    GuidePose g;
    for (int i = 0; i < 9; i++) g.R[i] = R[i];
    for (int i = 0; i < 3; i++) g.t[i] = t[i];
    g.fx = (double)K[0]; g.cx = (double)K[2]; g.fy = (double)K[4]; g.cy = (double)K[5];
    return g;
}

SVO_HD static inline bool guide_finite_f32(float v) { return v - v == 0.f; }       // x - x is 0 for every finite x and NaN otherwise

// Rule 1: the projection (u, v) of the point (x, y, z) with tag `tag`.  Left to right: Xc = ((R0 x + R1 y) + R2 z) + t0, likewise Yc
// and Zc; u = f32(fx (Xc / Zc) + cx), v = f32(fy (Yc / Zc) + cy).  The row is visible when it has a point, Zc > 0 strictly and both
// u and v are finite after the rounding to f32; an invisible row projects to (+inf, +inf).  -> visible
SVO_HD static inline bool guide_project(const GuidePose& g, float x, float y, float z, int32_t tag, float& u, float& v) {
    const float inf = __builtin_inff();
    u = inf; v = inf;
    if (tag == SVO_GUIDE_POINT_NONE) return false;
    const double X = (double)x, Y = (double)y, Z = (double)z;
    double c[3];
    for (int r = 0; r < 3; r++) {
        double s = g.R[3 * r] * X;
        s = s + g.R[3 * r + 1] * Y;
        s = s + g.R[3 * r + 2] * Z;
        c[r] = s + g.t[r];
    }
    if (!(c[2] > 0.)) return false;
    double pu = g.fx * (c[0] / c[2]);
    pu = pu + g.cx;
    double pv = g.fy * (c[1] / c[2]);
    pv = pv + g.cy;
    const float fu = (float)pu, fv = (float)pv;
    if (!guide_finite_f32(fu) || !guide_finite_f32(fv)) return false;
    u = fu; v = fv;
    return true;
}

// Rule 2: is the row whose projection is (u, v) admissible for the query at pixel (qx, qy)?  f32 throughout, both limits inclusive.
// An invisible row (+inf) fails against every finite pixel, and against a non-finite one inf - inf is NaN, which fails too.
SVO_HD static inline bool guide_admits_axis(float p, float q, float radius) { return __builtin_fabsf(p - q) <= radius; }
SVO_HD static inline bool guide_admits(float u, float v, float qx, float qy, float radius) {
    return guide_admits_axis(u, qx, radius) && guide_admits_axis(v, qy, radius);
}
