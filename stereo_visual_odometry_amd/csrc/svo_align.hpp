// svo_align.hpp — the rules of the descriptor index's map alignment (include/svo.h, "Map alignment"): a call's refusals, the
// counter-based sampler of rule 6, Horn's closed form of rule 7, the residual of rule 8, and the layout of the staging.  Plain C++
// that a host compiler takes as it is, like svo_reloc_batch.hpp, so that a stand-alone host program (tests/cpp/align_host.cpp) runs
// exactly the text svo_match_api.hip and the kernels (svo_kernels_align.hip) run.  The refusals, the sampler and the layout are
// integers; the model and the residual are f64, every operation rounded on its own (the translation units that include this are
// built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SVO_ALIGN_HD __host__ __device__
#define SVO_ALIGN_UNROLL _Pragma("unroll")
#else
#define SVO_ALIGN_HD
#define SVO_ALIGN_UNROLL
#endif

#define ALIGN_MAX_ROWS 4096                           // include/svo.h: SVO_ALIGN_MAX_ROWS, the rows of a source span
#define ALIGN_MAX_HYPOTHESES 1024                     // include/svo.h: SVO_ALIGN_MAX_HYPOTHESES
#define ALIGN_MAX_REFIT 8                             // refit_rounds: 0 .. 8
#define ALIGN_MAX_DRAWS 64                            // draws of one hypothesis before the fallback fills in
#define ALIGN_MAX_RATIO (1 << 20)                     // ratio_num, ratio_den: svo_reloc.hpp's SVO_RELOC_MAX_RATIO

// ---- a call's refusals.  The request is svo_align_params field by field; row_hi = -1 is the index's size, as everywhere
struct AlignRequest {
    int32_t src_lo, src_hi, dst_lo, dst_hi, max_dist, ratio_num, ratio_den, min_pairs, hypotheses, refit_rounds;
    float inlier_dist;
};
enum AlignRefusal {
    ALIGN_OK = 0, ALIGN_SRC_RANGE, ALIGN_DST_RANGE, ALIGN_ROWS, ALIGN_OVERLAP, ALIGN_MAX_DIST, ALIGN_RATIO, ALIGN_MIN_PAIRS, ALIGN_HYPOTHESES,
    ALIGN_REFIT, ALIGN_INLIER_DIST
};

// do [a_lo, a_hi) and [b_lo, b_hi) share a row?  An empty span shares none; spans that touch (a_hi == b_lo) share none.
static inline bool align_spans_overlap(int a_lo, int a_hi, int b_lo, int b_hi) {
    return a_lo < a_hi && b_lo < b_hi && a_lo < b_hi && b_lo < a_hi;
}

// The spans of a call, resolved in place (-1 becomes size): what svo_desc_index_match_rows refuses.
static inline AlignRefusal align_check_spans(AlignRequest& q, int size) {
    if (q.src_hi == -1) q.src_hi = size;
    if (q.dst_hi == -1) q.dst_hi = size;
    if (q.src_lo < 0 || q.src_hi > size || q.src_lo > q.src_hi) return ALIGN_SRC_RANGE;
    if (q.dst_lo < 0 || q.dst_hi > size || q.dst_lo > q.dst_hi) return ALIGN_DST_RANGE;
    if (q.src_hi - q.src_lo > ALIGN_MAX_ROWS) return ALIGN_ROWS;
    if (align_spans_overlap(q.src_lo, q.src_hi, q.dst_lo, q.dst_hi)) return ALIGN_OVERLAP;
    return ALIGN_OK;
}

// everything svo_desc_index_pair_rows and svo_desc_index_align refuse: the spans, then the parameters in the header's order
static inline AlignRefusal align_check(AlignRequest& q, int size) {
    if (const AlignRefusal e = align_check_spans(q, size); e != ALIGN_OK) return e;
    if (q.max_dist < 0 || q.max_dist > 256) return ALIGN_MAX_DIST;
    if (q.ratio_num < 1 || q.ratio_num > ALIGN_MAX_RATIO || q.ratio_den < 1 || q.ratio_den > ALIGN_MAX_RATIO) return ALIGN_RATIO;
    if (q.min_pairs < 3 || q.min_pairs > ALIGN_MAX_ROWS) return ALIGN_MIN_PAIRS;
    if (q.hypotheses < 1 || q.hypotheses > ALIGN_MAX_HYPOTHESES) return ALIGN_HYPOTHESES;
    if (q.refit_rounds < 0 || q.refit_rounds > ALIGN_MAX_REFIT) return ALIGN_REFIT;
    if (!isfinite(q.inlier_dist) || !(q.inlier_dist > 0.f)) return ALIGN_INLIER_DIST;
    return ALIGN_OK;
}

// ---- rule 6: the sampler.  splitmix64's finaliser on the counter (h << 32 | k)
SVO_ALIGN_HD static inline uint64_t align_mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Three distinct pair numbers below n_pairs (>= 3) for hypothesis h.  Draw k = 0, 1, .. is (mix64(h << 32 | k) >> 32) % n_pairs; a
// draw equal to an earlier one of this hypothesis is skipped.  After max_draws draws (ALIGN_MAX_DRAWS in the library; a test passes
// fewer to reach the fallback) every missing position takes the smallest pair number not yet used, so the loop ends whatever the
// generator gives.  Returns the draws made.
SVO_ALIGN_HD static inline int align_sample_draws(uint32_t h, int32_t n_pairs, int max_draws, int32_t (&out)[3]) {
    int got = 0, k = 0;
    out[0] = out[1] = out[2] = -1;
    for (; k < max_draws && got < 3; k++) {
        const int32_t d = (int32_t)((uint32_t)(align_mix64((uint64_t)h << 32 | (uint64_t)(uint32_t)k) >> 32) % (uint32_t)n_pairs);
        const bool seen = (got > 0 && d == out[0]) || (got > 1 && d == out[1]);
        if (seen) continue;
        if (got == 0) out[0] = d; else if (got == 1) out[1] = d; else out[2] = d;
        got++;
    }
    for (int32_t c = 0; got < 3; c++) {               // c < 3 + got <= 5: at most two numbers are taken
        const bool seen = (got > 0 && c == out[0]) || (got > 1 && c == out[1]);
        if (seen) continue;
        if (got == 0) out[0] = c; else if (got == 1) out[1] = c; else out[2] = c;
        got++;
    }
    return k;
}
SVO_ALIGN_HD static inline void align_sample(uint32_t h, int32_t n_pairs, int32_t (&out)[3]) { (void)align_sample_draws(h, n_pairs, ALIGN_MAX_DRAWS, out); }

// ---- rules 7 and 8: the model x_dst = R x_src + t
struct AlignModel { double R[9], t[3]; };

// one rotation of the cyclic Jacobi on the pair (I, J) of a symmetric 4 x 4 (upper triangle of A), p3p_jacobi4's step
template <int I, int J>
SVO_ALIGN_HD static inline void align_jacobi_rot(double (&A)[16], double (&D)[4], double (&Z)[4], double (&U)[16], int iter, double tresh) {
    const double Aij = A[4 * I + J], eps_machine = 100.0 * fabs(Aij);
    if (iter > 3 && fabs(D[I]) + eps_machine == fabs(D[I]) && fabs(D[J]) + eps_machine == fabs(D[J])) { A[4 * I + J] = 0.0; return; }
    if (!(fabs(Aij) > tresh)) return;
    double hh = D[J] - D[I], t;
    if (fabs(hh) + eps_machine == fabs(hh)) t = Aij / hh;
    else {
        const double theta = 0.5 * hh / Aij;
        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
        if (theta < 0.0) t = -t;
    }
    hh = t * Aij;
    Z[I] -= hh; Z[J] += hh; D[I] -= hh; D[J] += hh;
    A[4 * I + J] = 0.0;
    const double c = 1.0 / sqrt(1 + t * t), s = t * c, tau = s / (1.0 + c);
    SVO_ALIGN_UNROLL
    for (int k = 0; k < I; k++) { const double g = A[k * 4 + I], h = A[k * 4 + J]; A[k * 4 + I] = g - s * (h + g * tau); A[k * 4 + J] = h + s * (g - h * tau); }
    SVO_ALIGN_UNROLL
    for (int k = I + 1; k < J; k++) { const double g = A[I * 4 + k], h = A[k * 4 + J]; A[I * 4 + k] = g - s * (h + g * tau); A[k * 4 + J] = h + s * (g - h * tau); }
    SVO_ALIGN_UNROLL
    for (int k = J + 1; k < 4; k++) { const double g = A[I * 4 + k], h = A[J * 4 + k]; A[I * 4 + k] = g - s * (h + g * tau); A[J * 4 + k] = h + s * (g - h * tau); }
    SVO_ALIGN_UNROLL
    for (int k = 0; k < 4; k++) { const double g = U[k * 4 + I], h = U[k * 4 + J]; U[k * 4 + I] = g - s * (h + g * tau); U[k * 4 + J] = h + s * (g - h * tau); }
}

// symmetric 4 x 4 eigen decomposition, cyclic Jacobi: p3p_jacobi4 (svo_kernels_pnp.hip) restated with every index a constant
SVO_ALIGN_HD static inline void align_jacobi4(double (&A)[16], double (&D)[4], double (&U)[16]) {
    double B[4], Z[4] = {0, 0, 0, 0};
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 16; i++) U[i] = (i % 5 == 0);
    B[0] = A[0]; B[1] = A[5]; B[2] = A[10]; B[3] = A[15];
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 4; i++) D[i] = B[i];
    for (int iter = 0; iter < 50; iter++) {
        const double sum = fabs(A[1]) + fabs(A[2]) + fabs(A[3]) + fabs(A[6]) + fabs(A[7]) + fabs(A[11]);
        if (sum == 0.0) return;
        const double tresh = (iter < 3) ? 0.2 * sum / 16. : 0.0;
        align_jacobi_rot<0, 1>(A, D, Z, U, iter, tresh); align_jacobi_rot<0, 2>(A, D, Z, U, iter, tresh); align_jacobi_rot<0, 3>(A, D, Z, U, iter, tresh);
        align_jacobi_rot<1, 2>(A, D, Z, U, iter, tresh); align_jacobi_rot<1, 3>(A, D, Z, U, iter, tresh); align_jacobi_rot<2, 3>(A, D, Z, U, iter, tresh);
        SVO_ALIGN_UNROLL
        for (int i = 0; i < 4; i++) { B[i] += Z[i]; D[i] = B[i]; Z[i] = 0; }
    }
}

// Horn's closed form from the centroids cp, cq and the centred cross-covariance S[3 i + j] = sum (p_i - cp_i) (q_j - cq_j): the
// symmetric 4 x 4 matrix, the eigenvector of its largest eigenvalue (the first of equal ones) as a quaternion, R, and t = cq - R cp.
SVO_ALIGN_HD static inline void align_horn(const double (&cp)[3], const double (&cq)[3], const double (&s)[9], AlignModel& m) {
    double Qs[16], evs[4], U[16], q[4];
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 16; i++) Qs[i] = 0;
    Qs[0] = s[0] + s[4] + s[8]; Qs[5] = s[0] - s[4] - s[8]; Qs[10] = s[4] - s[8] - s[0]; Qs[15] = s[8] - s[0] - s[4];
    Qs[4] = Qs[1] = s[5] - s[7]; Qs[8] = Qs[2] = s[6] - s[2]; Qs[12] = Qs[3] = s[1] - s[3];
    Qs[9] = Qs[6] = s[3] + s[1]; Qs[13] = Qs[7] = s[6] + s[2]; Qs[14] = Qs[11] = s[7] + s[5];
    align_jacobi4(Qs, evs, U);
    int i_ev = 0;
    double ev_max = evs[0];
    SVO_ALIGN_UNROLL
    for (int i = 1; i < 4; i++) if (evs[i] > ev_max) { ev_max = evs[i]; i_ev = i; }
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 4; i++) q[i] = i_ev == 0 ? U[i * 4] : i_ev == 1 ? U[i * 4 + 1] : i_ev == 2 ? U[i * 4 + 2] : U[i * 4 + 3];
    const double q02 = q[0] * q[0], q12 = q[1] * q[1], q22 = q[2] * q[2], q32 = q[3] * q[3];
    const double q0_1 = q[0] * q[1], q0_2 = q[0] * q[2], q0_3 = q[0] * q[3], q1_2 = q[1] * q[2], q1_3 = q[1] * q[3], q2_3 = q[2] * q[3];
    m.R[0] = q02 + q12 - q22 - q32; m.R[1] = 2. * (q1_2 - q0_3); m.R[2] = 2. * (q1_3 + q0_2);
    m.R[3] = 2. * (q1_2 + q0_3); m.R[4] = q02 + q22 - q12 - q32; m.R[5] = 2. * (q2_3 - q0_1);
    m.R[6] = 2. * (q1_3 - q0_2); m.R[7] = 2. * (q2_3 + q0_1); m.R[8] = q02 + q32 - q12 - q22;
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 3; i++) m.t[i] = cq[i] - (m.R[3 * i] * cp[0] + m.R[3 * i + 1] * cp[1] + m.R[3 * i + 2] * cp[2]);
}

// The model of three pairs.  A pair is six floats (p, q), widened to f64.  Centroids ((a + b) + c) / 3, then the centred products
// summed in the pairs' order.
SVO_ALIGN_HD static inline void align_model3(const float* a, const float* b, const float* c, AlignModel& m) {
    double cp[3], cq[3], s[9];
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 3; i++) {
        cp[i] = (((double)a[i] + (double)b[i]) + (double)c[i]) / 3.;
        cq[i] = (((double)a[3 + i] + (double)b[3 + i]) + (double)c[3 + i]) / 3.;
    }
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 3; i++) {
        SVO_ALIGN_UNROLL
        for (int j = 0; j < 3; j++)
            s[3 * i + j] = (((double)a[i] - cp[i]) * ((double)a[3 + j] - cq[j]) + ((double)b[i] - cp[i]) * ((double)b[3 + j] - cq[j])) +
                           ((double)c[i] - cp[i]) * ((double)c[3 + j] - cq[j]);
    }
    align_horn(cp, cq, s, m);
}

SVO_ALIGN_HD static inline bool align_model_finite(const AlignModel& m) {
    bool ok = true;
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 9; i++) ok = ok && isfinite(m.R[i]);
    SVO_ALIGN_UNROLL
    for (int i = 0; i < 3; i++) ok = ok && isfinite(m.t[i]);
    return ok;
}

// |R p + t - q|^2 of one pair: per coordinate (((R0 x + R1 y) + R2 z) + t) - q, then (rx^2 + ry^2) + rz^2
SVO_ALIGN_HD static inline double align_residual2(const AlignModel& m, const float* pq) {
    const double x = (double)pq[0], y = (double)pq[1], z = (double)pq[2];
    const double rx = (((m.R[0] * x + m.R[1] * y) + m.R[2] * z) + m.t[0]) - (double)pq[3];
    const double ry = (((m.R[3] * x + m.R[4] * y) + m.R[5] * z) + m.t[1]) - (double)pq[4];
    const double rz = (((m.R[6] * x + m.R[7] * y) + m.R[8] * z) + m.t[2]) - (double)pq[5];
    return (rx * rx + ry * ry) + rz * rz;
}
// rule 8's compare: inclusive, against the squared distance; a non-finite residual is no inlier
SVO_ALIGN_HD static inline bool align_is_inlier(const AlignModel& m, const float* pq, double dist2) { return align_residual2(m, pq) <= dist2; }
static inline double align_dist2(float inlier_dist) { return (double)inlier_dist * (double)inlier_dist; }

// ---- the staging.  What a call leaves on the device, and in the pinned block its first down_end bytes: the result row, the two row
// lists and the inlier flags (one copy down); then the packed pairs, the hypotheses' counts and their models.
struct AlignOut {                                     // what the kernels report
    int32_t success, n_pairs, n_inliers, best_hypothesis, best_count, refit_rounds_run, pad[2];
    double R[9], t[3], rms;
};
#define ALIGN_PAIR_FLOATS 6                           // a packed pair: p then q
static inline size_t align_round(size_t b) { return (b + 255) / 256 * 256; }
struct AlignLayout { size_t out, pair_src, pair_dst, pair_inlier, down_end, pairs, counts, models, total; };
static inline AlignLayout align_layout(size_t n, size_t hypotheses) {
    AlignLayout l;
    size_t at = 0;
    l.out = at; at += align_round(sizeof(AlignOut));
    l.pair_src = at; at += align_round(n * sizeof(int32_t));
    l.pair_dst = at; at += align_round(n * sizeof(int32_t));
    l.pair_inlier = at; at += align_round(n);
    l.down_end = at;
    l.pairs = at; at += align_round(n * ALIGN_PAIR_FLOATS * sizeof(float));
    l.counts = at; at += align_round(hypotheses * sizeof(int32_t));
    l.models = at; at += align_round(hypotheses * sizeof(AlignModel));
    l.total = at;
    return l;
}
