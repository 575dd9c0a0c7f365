// align_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_align.hpp, the rules of the map alignment compiled
// for the host from the text svo_match_api.hip and the kernels run (tests/test_align_host.py builds it with AddressSanitizer and
// UBSan and runs it): every refusal of a call; the spans' overlap where they touch and where they share one row; the sampler for
// every n_pairs 3 .. 4096 at a spread of h, and its fallback forced at n_pairs = 3; Horn's closed form on three pairs and the
// residual; the staging's sizes at n = 4096, H = 1024.
#include "../../stereo_visual_odometry_amd/csrc/svo_align.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include <limits>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static AlignRequest good() { return AlignRequest{100, 200, 0, 100, 40, 7, 10, 6, 256, 4, 0.05f}; }
template <typename F> static AlignRefusal with(F change, int size = 1000) {
    AlignRequest q = good();
    change(q);
    return align_check(q, size);
}

static void test_refusals() {
    AlignRequest q = good();
    CHECK(align_check(q, 1000) == ALIGN_OK && q.src_hi == 200);
    q = good(); q.src_hi = -1; q.dst_lo = 0; q.dst_hi = 100;                // -1 is the size
    CHECK(align_check(q, 300) == ALIGN_OK && q.src_hi == 300);
    q = good(); q.dst_hi = -1;                                              // D = [0, size) swallows S
    CHECK(align_check(q, 1000) == ALIGN_OVERLAP && q.dst_hi == 1000);
    CHECK(with([](AlignRequest& r) { r.src_lo = -1; }) == ALIGN_SRC_RANGE);
    CHECK(with([](AlignRequest& r) { r.src_hi = 1001; }) == ALIGN_SRC_RANGE);
    CHECK(with([](AlignRequest& r) { r.src_lo = 201; }) == ALIGN_SRC_RANGE);
    CHECK(with([](AlignRequest& r) { r.src_hi = -2; }) == ALIGN_SRC_RANGE);
    CHECK(with([](AlignRequest& r) { r.dst_lo = -1; }) == ALIGN_DST_RANGE);
    CHECK(with([](AlignRequest& r) { r.dst_hi = 1001; }) == ALIGN_DST_RANGE);
    CHECK(with([](AlignRequest& r) { r.dst_lo = 101; }) == ALIGN_DST_RANGE);
    CHECK(with([](AlignRequest& r) { r.src_lo = 1000; r.src_hi = 1000 + ALIGN_MAX_ROWS; }, 10000) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.src_lo = 1000; r.src_hi = 1001 + ALIGN_MAX_ROWS; }, 10000) == ALIGN_ROWS);
    CHECK(with([](AlignRequest& r) { r.src_lo = 0; r.src_hi = std::numeric_limits<int32_t>::max(); }, std::numeric_limits<int32_t>::max()) == ALIGN_ROWS);
    CHECK(with([](AlignRequest& r) { r.max_dist = -1; }) == ALIGN_MAX_DIST && with([](AlignRequest& r) { r.max_dist = 257; }) == ALIGN_MAX_DIST);
    CHECK(with([](AlignRequest& r) { r.max_dist = 0; }) == ALIGN_OK && with([](AlignRequest& r) { r.max_dist = 256; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.ratio_num = 0; }) == ALIGN_RATIO && with([](AlignRequest& r) { r.ratio_den = 0; }) == ALIGN_RATIO);
    CHECK(with([](AlignRequest& r) { r.ratio_num = ALIGN_MAX_RATIO + 1; }) == ALIGN_RATIO && with([](AlignRequest& r) { r.ratio_den = ALIGN_MAX_RATIO + 1; }) == ALIGN_RATIO);
    CHECK(with([](AlignRequest& r) { r.ratio_num = ALIGN_MAX_RATIO; r.ratio_den = 1; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.min_pairs = 2; }) == ALIGN_MIN_PAIRS && with([](AlignRequest& r) { r.min_pairs = 3; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.min_pairs = ALIGN_MAX_ROWS + 1; }) == ALIGN_MIN_PAIRS && with([](AlignRequest& r) { r.min_pairs = ALIGN_MAX_ROWS; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.hypotheses = 0; }) == ALIGN_HYPOTHESES && with([](AlignRequest& r) { r.hypotheses = ALIGN_MAX_HYPOTHESES + 1; }) == ALIGN_HYPOTHESES);
    CHECK(with([](AlignRequest& r) { r.hypotheses = 1; }) == ALIGN_OK && with([](AlignRequest& r) { r.hypotheses = ALIGN_MAX_HYPOTHESES; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.refit_rounds = -1; }) == ALIGN_REFIT && with([](AlignRequest& r) { r.refit_rounds = ALIGN_MAX_REFIT + 1; }) == ALIGN_REFIT);
    CHECK(with([](AlignRequest& r) { r.refit_rounds = 0; }) == ALIGN_OK && with([](AlignRequest& r) { r.refit_rounds = ALIGN_MAX_REFIT; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.inlier_dist = 0.f; }) == ALIGN_INLIER_DIST && with([](AlignRequest& r) { r.inlier_dist = -1.f; }) == ALIGN_INLIER_DIST);
    CHECK(with([](AlignRequest& r) { r.inlier_dist = std::numeric_limits<float>::infinity(); }) == ALIGN_INLIER_DIST);
    CHECK(with([](AlignRequest& r) { r.inlier_dist = std::numeric_limits<float>::quiet_NaN(); }) == ALIGN_INLIER_DIST);
    CHECK(with([](AlignRequest& r) { r.inlier_dist = std::numeric_limits<float>::denorm_min(); }) == ALIGN_OK);
    // the spans come first, the parameters in the header's order
    CHECK(with([](AlignRequest& r) { r.src_lo = -1; r.max_dist = -1; }) == ALIGN_SRC_RANGE && with([](AlignRequest& r) { r.max_dist = -1; r.inlier_dist = 0.f; }) == ALIGN_MAX_DIST);
}

static void test_overlap() {
    CHECK(!align_spans_overlap(100, 200, 0, 100) && !align_spans_overlap(0, 100, 100, 200));        // touching, either order
    CHECK(align_spans_overlap(100, 200, 0, 101) && align_spans_overlap(0, 101, 100, 200));          // one row shared
    CHECK(align_spans_overlap(100, 200, 199, 300) && !align_spans_overlap(100, 200, 200, 300));
    CHECK(align_spans_overlap(0, 10, 0, 10) && align_spans_overlap(0, 10, 3, 4) && align_spans_overlap(3, 4, 0, 10));
    CHECK(!align_spans_overlap(5, 5, 0, 10) && !align_spans_overlap(0, 10, 5, 5) && !align_spans_overlap(5, 5, 5, 5));   // an empty span shares nothing
    CHECK(with([](AlignRequest& r) { r.dst_hi = 101; }) == ALIGN_OVERLAP && with([](AlignRequest& r) { r.dst_hi = 100; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.dst_lo = 199; r.dst_hi = 300; }) == ALIGN_OVERLAP && with([](AlignRequest& r) { r.dst_lo = 200; r.dst_hi = 300; }) == ALIGN_OK);
    CHECK(with([](AlignRequest& r) { r.src_lo = r.src_hi = 50; }) == ALIGN_OK);                      // an empty source inside D
}

static void test_sampler() {
    const uint32_t hs[] = {0u, 1u, 2u, 7u, 63u, 64u, 255u, 1023u, 65535u, 0x80000000u, 0xFFFFFFFFu};
    int most = 0;
    for (int32_t n = 3; n <= ALIGN_MAX_ROWS; n++) {
        for (const uint32_t h : hs) {
            int32_t s[3];
            const int draws = align_sample_draws(h, n, ALIGN_MAX_DRAWS, s);
            most = draws > most ? draws : most;
            CHECK(s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && s[0] < n && s[1] < n && s[2] < n);
            CHECK(s[0] != s[1] && s[0] != s[2] && s[1] != s[2]);
            CHECK(draws >= 3 && draws <= ALIGN_MAX_DRAWS);
            int32_t again[3];
            align_sample(h, n, again);
            CHECK(again[0] == s[0] && again[1] == s[1] && again[2] == s[2]);
        }
    }
    printf("most draws: %d\n", most);
    CHECK(align_mix64(0) == 0xE220A8397B1DCDAFull);                          // splitmix64's first output from state 0
    // the fallback, forced: no draw, one draw, two draws' worth
    for (uint32_t h = 0; h < 64; h++) {
        int32_t s[3], full[3];
        CHECK(align_sample_draws(h, 3, 0, s) == 0 && s[0] == 0 && s[1] == 1 && s[2] == 2);
        align_sample(h, 3, full);
        CHECK(align_sample_draws(h, 3, 1, s) == 1 && s[0] == full[0]);
        CHECK(s[1] == (s[0] == 0 ? 1 : 0) && s[2] == (s[0] == 2 ? 1 : 2));    // the two smallest numbers not used, in order
        for (int k = 2; k < 6; k++) {
            align_sample_draws(h, 3, k, s);
            CHECK(s[0] != s[1] && s[0] != s[2] && s[1] != s[2] && s[0] >= 0 && s[0] < 3 && s[1] >= 0 && s[1] < 3 && s[2] >= 0 && s[2] < 3);
        }
        align_sample_draws(h, 4096, 1, s);                                    // the fallback at a large n: the smallest two besides the draw
        CHECK(s[0] >= 0 && s[0] < 4096 && s[1] == (s[0] == 0 ? 1 : 0) && s[2] == (s[0] <= 1 ? 2 : 1));
    }
}

static void test_model() {
    // a rotation of 0.7 rad about (1, 2, 3) / sqrt(14) and a shift, as the GPU tests' scenes
    const double a[3] = {1 / sqrt(14.), 2 / sqrt(14.), 3 / sqrt(14.)}, c = cos(0.7), s = sin(0.7);
    double R[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (i == j ? c : 0.) + (1 - c) * a[i] * a[j];
    R[1] -= s * a[2]; R[2] += s * a[1]; R[3] += s * a[2]; R[5] -= s * a[0]; R[6] -= s * a[1]; R[7] += s * a[0];
    const double t[3] = {12., -3., 40.};
    const float P[4][3] = {{1.f, 2.f, 3.f}, {-20.f, 5.f, 7.f}, {4.f, -25.f, 11.f}, {9.f, 9.f, -14.f}};
    float pq[4][6];
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < 3; i++) {
            pq[k][i] = P[k][i];
            pq[k][3 + i] = (float)(R[3 * i] * P[k][0] + R[3 * i + 1] * P[k][1] + R[3 * i + 2] * P[k][2] + t[i]);
        }
    AlignModel m;
    align_model3(pq[0], pq[1], pq[2], m);
    CHECK(align_model_finite(m));
    for (int i = 0; i < 9; i++) CHECK(fabs(m.R[i] - R[i]) < 1e-6);            // the points are rounded to f32 at up to 60 m
    for (int i = 0; i < 3; i++) CHECK(fabs(m.t[i] - t[i]) < 1e-4);
    const double d2 = align_dist2(0.05f);
    CHECK(d2 == (double)0.05f * (double)0.05f);
    for (int k = 0; k < 4; k++) CHECK(align_residual2(m, pq[k]) < 1e-8 && align_is_inlier(m, pq[k], d2));
    float far[6] = {pq[3][0], pq[3][1], pq[3][2], pq[3][3] + 1.f, pq[3][4], pq[3][5]};
    CHECK(fabs(align_residual2(m, far) - 1.) < 1e-3 && !align_is_inlier(m, far, d2));
    // three pairs that are one point: a zero matrix, the Jacobi returns at once, the model is the identity about the centroid
    align_model3(pq[0], pq[0], pq[0], m);
    CHECK(align_model_finite(m) && m.R[0] == 1. && m.R[4] == 1. && m.R[8] == 1. && align_residual2(m, pq[0]) < 1e-8);
    // a non-finite point gives a non-finite model, which scores nothing
    float bad[6] = {std::numeric_limits<float>::infinity(), 0.f, 0.f, 0.f, 0.f, 0.f};
    align_model3(pq[0], pq[1], bad, m);
    CHECK(!align_model_finite(m) && !align_is_inlier(m, pq[0], d2));
}

// ---- Horn's closed form where the eigenvector pick, the Jacobi's early returns and the centroid subtraction do the work
// The column of the Jacobi's U that align_horn takes, by align_horn's own rule (the first of the largest eigenvalues), from the
// text of the header: the same 4 x 4 matrix through the same align_jacobi4.  -> the index, and the quaternion
static int horn_index(const double (&s)[9], double (&q)[4]) {
    double Qs[16] = {0}, evs[4], U[16];
    Qs[0] = s[0] + s[4] + s[8]; Qs[5] = s[0] - s[4] - s[8]; Qs[10] = s[4] - s[8] - s[0]; Qs[15] = s[8] - s[0] - s[4];
    Qs[4] = Qs[1] = s[5] - s[7]; Qs[8] = Qs[2] = s[6] - s[2]; Qs[12] = Qs[3] = s[1] - s[3];
    Qs[9] = Qs[6] = s[3] + s[1]; Qs[13] = Qs[7] = s[6] + s[2]; Qs[14] = Qs[11] = s[7] + s[5];
    align_jacobi4(Qs, evs, U);
    int i_ev = 0;
    for (int i = 1; i < 4; i++) if (evs[i] > evs[i_ev]) i_ev = i;
    for (int i = 0; i < 4; i++) q[i] = U[4 * i + i_ev];
    return i_ev;
}

enum Cloud { CLOUD_GENERIC, CLOUD_PLANE, CLOUD_LINE, CLOUD_TWO };
struct HornCase { const char* name; double angle, axis[3]; Cloud cloud; float offset; bool shift; };

// n <= 8 pairs of a case: source points that are exact in f32, their images rounded to f32.  -> the largest coordinate
static double horn_case_pairs(const HornCase& hc, int n, float (&pq)[8][6]) {
    static const float P[8][3] = {{1.f, 2.f, 3.f}, {-20.f, 5.f, 7.f}, {4.f, -25.f, 11.f}, {9.f, 9.f, -14.f},
                                  {-7.5f, 13.25f, 21.f}, {16.f, -3.5f, -9.f}, {-12.f, -18.f, 5.5f}, {27.f, 22.f, -1.25f}};
    const double na = sqrt(hc.axis[0] * hc.axis[0] + hc.axis[1] * hc.axis[1] + hc.axis[2] * hc.axis[2]);
    const double a[3] = {hc.axis[0] / na, hc.axis[1] / na, hc.axis[2] / na}, c = cos(hc.angle), s = sin(hc.angle);
    double R[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (i == j ? c : 0.) + (1 - c) * a[i] * a[j];
    R[1] -= s * a[2]; R[2] += s * a[1]; R[3] += s * a[2]; R[5] -= s * a[0]; R[6] -= s * a[1]; R[7] += s * a[0];
    const double t[3] = {hc.shift ? 12. : 0., hc.shift ? -3. : 0., hc.shift ? 40. : 0.};
    double most = 0.;
    for (int k = 0; k < n; k++) {
        const float* p = P[hc.cloud == CLOUD_TWO ? (k == n - 1 ? 1 : 0) : k];       // two points: all but the last pair are one point
        float x = p[0], y = p[1], z = p[2];
        if (hc.cloud == CLOUD_PLANE) z = (float)(0.3 * x - 0.2 * y + 1.);
        if (hc.cloud == CLOUD_LINE) { y = 2.f * x + 1.f; z = -x + 3.f; }
        pq[k][0] = x + hc.offset; pq[k][1] = y + hc.offset; pq[k][2] = z + hc.offset;
        for (int i = 0; i < 3; i++) {
            pq[k][3 + i] = (float)(R[3 * i] * (double)pq[k][0] + R[3 * i + 1] * (double)pq[k][1] + R[3 * i + 2] * (double)pq[k][2] + t[i]);
            most = fmax(most, fmax(fabs((double)pq[k][i]), fabs((double)pq[k][3 + i])));
        }
    }
    return most;
}

// One case at n pairs: rule 7's sums in the pairs' order, align_horn, and at n = 3 align_model3, which must give the same bits.
// The result is finite, orthonormal with det +1 to 1e-12, and fits its pairs to the f32 rounding of their coordinates.  Horn's
// optimum has no larger a sum of squared residuals than the true motion, whose residuals are the rounding of the images: at most
// half an ulp of the largest coordinate on each of 3 n coordinates, so every residual is within sqrt(3 n) half ulps — also where the
// optimum is not unique (a line, two points).  1e-12 of the largest coordinate is added for the f64 arithmetic itself.
static int horn_case_run(const HornCase& hc, int n) {
    float pq[8][6];
    const double most = horn_case_pairs(hc, n, pq);
    double cp[3] = {0, 0, 0}, cq[3] = {0, 0, 0}, s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < n; k++) { cp[i] += (double)pq[k][i]; cq[i] += (double)pq[k][3 + i]; }
        cp[i] /= (double)n; cq[i] /= (double)n;
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < n; k++) s[3 * i + j] += ((double)pq[k][i] - cp[i]) * ((double)pq[k][3 + j] - cq[j]);
    AlignModel m;
    align_horn(cp, cq, s, m);
    if (n == 3) {
        AlignModel m3;
        align_model3(pq[0], pq[1], pq[2], m3);
        for (int i = 0; i < 9; i++) CHECK(m3.R[i] == m.R[i]);
        for (int i = 0; i < 3; i++) CHECK(m3.t[i] == m.t[i]);
    }
    CHECK(align_model_finite(m));
    const double* R = m.R;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) CHECK(fabs(R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1. : 0.)) <= 1e-12);
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    CHECK(fabs(det - 1.) <= 1e-12);
    const double half_ulp = 0.5 * ((double)nextafterf((float)most, std::numeric_limits<float>::infinity()) - (double)(float)most);
    const double bound = sqrt(3. * n) * half_ulp + 1e-12 * most;
    double worst = 0.;
    for (int k = 0; k < n; k++) worst = fmax(worst, sqrt(align_residual2(m, pq[k])));
    CHECK(worst <= bound);
    double q[4];
    const int i_ev = horn_index(s, q);
    CHECK(m.R[0] == ((q[0] * q[0] + q[1] * q[1]) - q[2] * q[2]) - q[3] * q[3]);   // the quaternion align_horn took
    printf("  %-28s n %d: eigenvector %d, q0 %+.3e, worst residual %.3g m (bound %.3g m)\n", hc.name, n, i_ev, q[0], worst, bound);
    return i_ev;
}

static void test_model_geometry() {
    const double pi = 3.14159265358979323846;
    const HornCase cases[] = {
        {"pi about x", pi, {1, 0, 0}, CLOUD_GENERIC, 0.f, true}, {"pi about y", pi, {0, 1, 0}, CLOUD_GENERIC, 0.f, true},
        {"pi about z", pi, {0, 0, 1}, CLOUD_GENERIC, 0.f, true}, {"pi about (1, 2, 3)", pi, {1, 2, 3}, CLOUD_GENERIC, 0.f, true},
        {"2 pi / 3 about (1, 1, 1)", 2 * pi / 3, {1, 1, 1}, CLOUD_GENERIC, 0.f, true}, {"identity", 0., {1, 2, 3}, CLOUD_GENERIC, 0.f, false},
        {"planar", 0.7, {1, 2, 3}, CLOUD_PLANE, 0.f, true}, {"collinear", 0.7, {1, 2, 3}, CLOUD_LINE, 0.f, true},
        {"two points", 0.7, {1, 2, 3}, CLOUD_TWO, 0.f, true}, {"at +5000 m", 0.7, {1, 2, 3}, CLOUD_GENERIC, 5000.f, true},
        {"planar, pi about (3, -1, 2)", pi, {3, -1, 2}, CLOUD_PLANE, 0.f, true},
    };
    int seen[4] = {0, 0, 0, 0};
    printf("Horn's closed form, case by case:\n");
    for (const HornCase& hc : cases)
        for (const int n : {3, 8}) seen[horn_case_run(hc, n)]++;
    printf("eigenvector index taken: 0 x %d, 1 x %d, 2 x %d, 3 x %d\n", seen[0], seen[1], seen[2], seen[3]);
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && seen[3] > 0);
}

static void test_layout() {
    const AlignLayout l = align_layout(ALIGN_MAX_ROWS, ALIGN_MAX_HYPOTHESES);
    CHECK(sizeof(AlignOut) == 136 && sizeof(AlignModel) == 96);
    CHECK(l.out == 0 && l.pair_src == 256 && l.pair_dst == 256 + 16384 && l.pair_inlier == 256 + 32768 && l.down_end == 37120);
    CHECK(l.pairs == l.down_end && l.counts == l.pairs + 98304 && l.models == l.counts + 4096 && l.total == 237824);
    CHECK(l.total + (size_t)ALIGN_MAX_ROWS * 32 < 400 * 1024);                // with the search's result rows: below 400 KiB
    for (const size_t o : {l.out, l.pair_src, l.pair_dst, l.pair_inlier, l.pairs, l.counts, l.models, l.total}) CHECK(o % 256 == 0);
    const AlignLayout s = align_layout(1, 1);                                 // every part has room for one entry at least
    CHECK(s.pair_src - s.out >= sizeof(AlignOut) && s.pairs - s.pair_inlier >= 1 && s.counts - s.pairs >= 24 && s.total - s.models >= sizeof(AlignModel));
}

int main() {
    test_refusals();
    test_overlap();
    test_sampler();
    test_model();
    test_model_geometry();
    test_layout();
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ALIGN HOST OK\n");
    return 0;
}
