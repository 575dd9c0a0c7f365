// svo_prior.hpp — the host arithmetic of the motion prior (include/svo.h, "Motion prior"): plain C++, no HIP, so that a stand-alone
// host program (tests/cpp/motion_prior_host.cpp) runs exactly the code the library runs.  Each function returns null, or the text of
// the SVO_ERR_ARG it stands for.
#pragma once
#include <math.h>
#include <string.h>

static inline bool prior_all_finite(const float* m, int n) { for (int k = 0; k < n; k++) if (!isfinite(m[k])) return false; return true; }

// inv = adj(m) / det in f64: each cofactor a d - b c, det = m0 C00 + m1 C01 + m2 C02.  false: det is 0 or not finite.
static inline bool prior_invert3x3(const double m[9], double inv[9]) {
    const double C00 = m[4] * m[8] - m[5] * m[7], C01 = m[5] * m[6] - m[3] * m[8], C02 = m[3] * m[7] - m[4] * m[6];
    const double C10 = m[2] * m[7] - m[1] * m[8], C11 = m[0] * m[8] - m[2] * m[6], C12 = m[1] * m[6] - m[0] * m[7];
    const double C20 = m[1] * m[5] - m[2] * m[4], C21 = m[2] * m[3] - m[0] * m[5], C22 = m[0] * m[4] - m[1] * m[3];
    const double det = m[0] * C00 + m[1] * C01 + m[2] * C02;
    if (det == 0. || !isfinite(det)) return false;
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
// right).  Either output may be null.
static inline const char* prior_from_rotation(const float Pl[12], const double R[9], float H[9], float Hi[9]) {
    double K[9], Ki[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) K[3 * i + j] = (double)Pl[4 * i + j];
    for (int k = 0; k < 9; k++) if (!isfinite(K[k]) || !isfinite(R[k])) return "motion prior: a non-finite entry in K or R";
    if (!prior_invert3x3(K, Ki)) return "motion prior: K = Pl[:, :3] is singular";
    const auto mul = [](const double* a, const double* b, double* o) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
    };
    for (int t = 0; t < 2; t++) {
        float* out = t ? Hi : H;
        if (!out) continue;
        double Rt[9], KR[9], M[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rt[3 * i + j] = t ? R[3 * j + i] : R[3 * i + j];
        mul(K, Rt, KR); mul(KR, Ki, M);
        for (int k = 0; k < 9; k++) out[k] = (float)M[k];
    }
    return nullptr;
}
