// The host arithmetic of the motion prior (stereo_visual_odometry_amd/csrc/svo_prior.hpp — the very functions libsvo_hip.so runs
// behind svo_set_motion_prior and svo_motion_prior_from_rotation) in a stand-alone program: no GPU, no library, so it can be built
// with -fsanitize=address,undefined and run anywhere (tests/test_motion_prior_host.py).
//   * the adjugate inverse: H Hi = I to rounding on a rotation homography, the exact inverse of a power-of-two scaling, refusal of
//     a singular and of a non-finite matrix;
//   * prior_from_rotation: H = K R K^-1 and Hi = K Rt K^-1 against a long-double evaluation, Hi the inverse of H, H(R = I) = I in bits,
//     either output omitted, a singular K and a non-finite R refused;
//   * prior_make: a caller's Hi is taken as given, a missing one is the adjugate inverse, non-finite entries are refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include "../../stereo_visual_odometry_amd/csrc/svo_prior.hpp"

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); fails++; } } while (0)

static void mul(const long double* a, const long double* b, long double* o) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

int main() {
    const float Pl[12] = {718.856f, 0.f, 160.f, 0.f, 0.f, 718.856f, 120.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    const double a = 7.65 * 3.14159265358979323846 / 180.0, b = 0.02, c = -0.013;
    // R = Ry(a) Rx(b) Rz(c)
    const double ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b), cc = std::cos(c), sc = std::sin(c);
    const long double Ry[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca}, Rx[9] = {1, 0, 0, 0, cb, -sb, 0, sb, cb}, Rz[9] = {cc, -sc, 0, sc, cc, 0, 0, 0, 1};
    long double t[9], Rl[9];
    mul(Ry, Rx, t); mul(t, Rz, Rl);
    double R[9];
    for (int k = 0; k < 9; k++) R[k] = (double)Rl[k];

    float H[9], Hi[9];
    CHECK(prior_from_rotation(Pl, R, H, Hi) == nullptr);
    {   // against K R K^-1 in long double, K^-1 written out for this K
        const long double fx = Pl[0], cx = Pl[2], fy = Pl[5], cy = Pl[6];
        const long double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1}, Ki[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
        long double Rt[9], KR[9], M[9], Mi[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rt[3 * i + j] = Rl[3 * j + i];
        mul(K, Rl, KR); mul(KR, Ki, M);
        mul(K, Rt, KR); mul(KR, Ki, Mi);
        long double scale = 0;
        for (int k = 0; k < 9; k++) scale = std::fmax(scale, std::fabs(M[k]));
        for (int k = 0; k < 9; k++) { CHECK(std::fabs(H[k] - M[k]) <= 1e-6L * scale); CHECK(std::fabs(Hi[k] - Mi[k]) <= 1e-6L * scale); }
    }
    {   // Hi is H's inverse, also through the adjugate of the rounded H
        double m[9], inv[9];
        for (int k = 0; k < 9; k++) m[k] = H[k];
        CHECK(prior_invert3x3(m, inv));
        double scale = 0;
        for (int k = 0; k < 9; k++) scale = std::fmax(scale, std::fabs((double)Hi[k]));
        for (int k = 0; k < 9; k++) CHECK(std::fabs(inv[k] - Hi[k]) <= 1e-6 * scale);
        float oH[9], oHi[9];
        CHECK(prior_make(H, nullptr, oH, oHi) == nullptr);
        CHECK(!std::memcmp(oH, H, sizeof(H)));
        for (int k = 0; k < 9; k++) CHECK(oHi[k] == (float)inv[k]);
        const float given[9] = {9, 8, 7, 6, 5, 4, 3, 2, 1};                       // a caller's Hi is not second-guessed
        CHECK(prior_make(H, given, oH, oHi) == nullptr && !std::memcmp(oHi, given, sizeof(given)));
    }
    {   // the identity rotation is the identity homography, in bits, whatever K is
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        float h[9];
        CHECK(prior_from_rotation(Pl, I, h, nullptr) == nullptr);
        for (int k = 0; k < 9; k++) CHECK(h[k] == (k % 4 == 0 ? 1.f : 0.f));
        float hi[9];
        CHECK(prior_from_rotation(Pl, I, nullptr, hi) == nullptr);
        for (int k = 0; k < 9; k++) CHECK(hi[k] == (k % 4 == 0 ? 1.f : 0.f));
    }
    {   // exact cases and refusals of the inverse
        const double s[9] = {4, 0, 0, 0, 0.5, 0, 0, 0, 2}, want[9] = {0.25, 0, 0, 0, 2, 0, 0, 0, 0.5};
        double inv[9];
        CHECK(prior_invert3x3(s, inv));
        for (int k = 0; k < 9; k++) CHECK(inv[k] == want[k]);
        const double sing[9] = {1, 2, 3, 2, 4, 6, 0, 0, 1};
        CHECK(!prior_invert3x3(sing, inv));
        const double huge[9] = {1e200, 0, 0, 0, 1e200, 0, 0, 0, 1e200};        // det overflows: not finite
        CHECK(!prior_invert3x3(huge, inv));
        const float fsing[9] = {1, 2, 3, 2, 4, 6, 0, 0, 1};
        float oH[9], oHi[9];
        CHECK(prior_make(fsing, nullptr, oH, oHi) != nullptr);
        float nf[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        nf[4] = std::numeric_limits<float>::infinity();
        CHECK(prior_make(nf, nullptr, oH, oHi) != nullptr);
        nf[4] = std::numeric_limits<float>::quiet_NaN();
        CHECK(prior_make(nf, nullptr, oH, oHi) != nullptr);
        const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        CHECK(prior_make(eye, nf, oH, oHi) != nullptr);                          // a non-finite Hi is refused too
    }
    {   // refusals of the rotation helper
        float badP[12];
        std::memcpy(badP, Pl, sizeof(badP));
        badP[0] = 0.f;                                                            // fx = 0: K singular
        CHECK(prior_from_rotation(badP, R, H, Hi) != nullptr);
        double badR[9];
        std::memcpy(badR, R, sizeof(badR));
        badR[3] = std::numeric_limits<double>::quiet_NaN();
        CHECK(prior_from_rotation(Pl, badR, H, Hi) != nullptr);
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("MOTION PRIOR HOST OK\n");
    return 0;
}
