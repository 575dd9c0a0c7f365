// svo_prior.hpp — the arithmetic of the motion prior (include/svo.h, "Motion prior"): plain C++ that a host compiler takes as it is,
// so that a stand-alone host program (tests/cpp/motion_prior_host.cpp, tests/cpp/auto_prior_host.cpp) runs exactly the code the
// library runs.  The functions marked SVO_HD are also compiled for the device: k_prior_predict (svo_kernels_prior.hip) runs
// prior_predict_row, the host runs the same text behind svo_motion_prior_from_rotation — f64, nothing fused (-ffp-contract=off), so
// both give the same bits.  The host functions return null, or the text of the SVO_ERR_ARG they stand for.
#pragma once
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define SVO_HD __host__ __device__
#else
#define SVO_HD
#endif

// One sequence's row of a frame's priors — the homography T0 -> T1, its inverse, and whether the sequence has one in this frame.  The
// frame's rows ([B], indexed by sequence) are a kernel argument of k_lk_chain_prior and k_prior_predict alone, like MaskArgs:
// DevBuffers and every other kernel's argument block stay as they are.  source: where the row came from (svo_get_last_motion_prior)
// — 0 with has = 1 is a caller's explicit prior, PRIOR_SOURCE_PREDICTED one that k_prior_predict wrote.
struct PriorRow { float H[9], Hi[9]; int has, source; };
#define PRIOR_SOURCE_PREDICTED 2

SVO_HD static inline bool prior_finite_f64(double v) { return v - v == 0.; }      // x - x is 0 for every finite x and NaN otherwise
static inline bool prior_all_finite(const float* m, int n) { for (int k = 0; k < n; k++) if (!isfinite(m[k])) return false; return true; }

// inv = adj(m) / det in f64: each cofactor a d - b c, det = m0 C00 + m1 C01 + m2 C02.  false: det is 0 or not finite.
SVO_HD static inline bool prior_invert3x3(const double m[9], double inv[9]) {
    const double C00 = m[4] * m[8] - m[5] * m[7], C01 = m[5] * m[6] - m[3] * m[8], C02 = m[3] * m[7] - m[4] * m[6];
    const double C10 = m[2] * m[7] - m[1] * m[8], C11 = m[0] * m[8] - m[2] * m[6], C12 = m[1] * m[6] - m[0] * m[7];
    const double C20 = m[1] * m[5] - m[2] * m[4], C21 = m[2] * m[3] - m[0] * m[5], C22 = m[0] * m[4] - m[1] * m[3];
    const double det = m[0] * C00 + m[1] * C01 + m[2] * C02;
    if (det == 0. || !prior_finite_f64(det)) return false;
    const double adj[9] = {C00, C10, C20, C01, C11, C21, C02, C12, C22};        // the transposed cofactors
    for (int k = 0; k < 9; k++) inv[k] = adj[k] / det;
    return true;
}

// One prior as the kernels take it: H checked and copied; Hi the caller's (checked) or, when null, H's inverse rounded to f32.
static inline const char* prior_make(const float* H, const float* Hi, float outH[9], float outHi[9]) {
    if (!prior_all_finite(H, 9) || (Hi && !prior_all_finite(Hi, 9))) return "motion prior: a non-finite entry";
    if (!Hi) {
        double m[9], inv[9];
        for (int k = 0; k < 9; k++) m[k] = (double)H[k];
        if (!prior_invert3x3(m, inv)) return "motion prior: H is singular (pass Hi, or an invertible H)";
        for (int k = 0; k < 9; k++) outHi[k] = (float)inv[k];
    } else memcpy(outHi, Hi, sizeof(float) * 9);
    memcpy(outH, H, sizeof(float) * 9);
    return nullptr;
}

// H = f32(K R K^-1), Hi = f32(K Rt K^-1) with K = Pl[:, :3], in f64 (K^-1 by the adjugate; a product's three terms summed left to
// right), each entry rounded to f32 once.  Either output may be null.  0, or PRIOR_NOT_FINITE / PRIOR_SINGULAR_K.
#define PRIOR_NOT_FINITE 1
#define PRIOR_SINGULAR_K 2
SVO_HD static inline void prior_mul3x3(const double* a, const double* b, double* o) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
SVO_HD static inline int prior_rotation_homography(const float Pl[12], const double R[9], float H[9], float Hi[9]) {
    double K[9], Ki[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) K[3 * i + j] = (double)Pl[4 * i + j];
    int finite = 1;                                                              // (no early exit: the loops unroll into registers on the device)
    for (int k = 0; k < 9; k++) finite &= (int)prior_finite_f64(K[k]) & (int)prior_finite_f64(R[k]);
    if (!finite) return PRIOR_NOT_FINITE;
    if (!prior_invert3x3(K, Ki)) return PRIOR_SINGULAR_K;
    for (int t = 0; t < 2; t++) {
        float* out = t ? Hi : H;
        if (!out) continue;
        double Rt[9], KR[9], M[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rt[3 * i + j] = t ? R[3 * j + i] : R[3 * i + j];
        prior_mul3x3(K, Rt, KR); prior_mul3x3(KR, Ki, M);
        for (int k = 0; k < 9; k++) out[k] = (float)M[k];
    }
    return 0;
}
static inline const char* prior_from_rotation(const float Pl[12], const double R[9], float H[9], float Hi[9]) {
    const int e = prior_rotation_homography(Pl, R, H, Hi);
    return e == PRIOR_NOT_FINITE ? "motion prior: a non-finite entry in K or R" : e == PRIOR_SINGULAR_K ? "motion prior: K = Pl[:, :3] is singular" : nullptr;
}

// The predicted prior of SVO_PRIOR_LAST_ROTATION (svo.h has the rule) for one sequence that takes a frame: `row` is the frame's row
// as the host left it (explicit = its `has` may be trusted: the rows were uploaded; otherwise the row is stale memory and counts as
// empty).  An explicit prior stays untouched.  Otherwise the row is rewritten whole: the rotation homography of the sequence's last
// pose when that pose stands (ok == 1 as the last frame it took left it, frame_id > 0: not reset since) and K R K^-1 / K Rt K^-1 are
// what svo_motion_prior_from_rotation + svo_set_motion_prior would accept (K regular, every entry finite, also after the rounding to
// f32), else an empty row.  Returns whether it wrote the row.
SVO_HD static inline bool prior_predict_row(PriorRow* row, bool explicit_rows, int ok, int frame_id, const double R[9], const float Pl[12]) {
    if (explicit_rows && row->has) return false;
    PriorRow p = {};
    int good = ok == 1 && frame_id > 0 && prior_rotation_homography(Pl, R, p.H, p.Hi) == 0;
    for (int k = 0; k < 9; k++) good &= (int)prior_finite_f64((double)p.H[k]) & (int)prior_finite_f64((double)p.Hi[k]);
    if (!good) for (int k = 0; k < 9; k++) p.H[k] = p.Hi[k] = 0.f;
    p.has = good ? 1 : 0; p.source = good ? PRIOR_SOURCE_PREDICTED : 0;
    *row = p;
    return true;
}
