// The C++ facade's map alignment (include/svo/visual_odometry.hpp: DescriptorIndex::match_rows, pair_rows, align, align_params) on a
// real GPU: match_rows against match with a host copy of the source descriptors, byte for byte; pair_rows and align against the
// caller's reference (written into the input); then the round trip — transform_points with the result's T, and align again gives the
// identity with the same inliers; overlapping spans throw and leave the outputs as they were.
// argv[1]: int32 {m, src_lo, src_hi, dst_lo, dst_hi, k, hypotheses, min_pairs}, float inlier_dist, m descriptors of 32 bytes, m ids
// (uint64), m points (3 floats), m tags (int32), then the k expected pairs — source rows, destination rows (int32), inlier flags
// (uint8) — and the expected R (9 doubles) and t (3 doubles) (tests/test_gpu_align_facade.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "svo/visual_odometry.hpp"

using namespace visual_odometry;
using Descriptor = DescriptorIndex::Descriptor;

template <typename T> static bool get(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || (bool)f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)));
}

// the angle of A B^T, from its skew part
static double angle(const double A[9], const double B[9]) {
    double D[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) D[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
    const double s = 0.5 * std::sqrt((D[7] - D[5]) * (D[7] - D[5]) + (D[2] - D[6]) * (D[2] - D[6]) + (D[3] - D[1]) * (D[3] - D[1]));
    return std::atan2(s, 0.5 * (D[0] + D[4] + D[8] - 1.));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[8];
    float inlier_dist;
    if (!f.read((char*)hdr, sizeof(hdr)) || !f.read((char*)&inlier_dist, sizeof(inlier_dist))) return 2;
    const int m = hdr[0], k = hdr[5];
    std::vector<Descriptor> desc;
    std::vector<float> xyz;
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags, want_src, want_dst;
    std::vector<uint8_t> want_inlier;
    std::vector<double> want_R, want_t;
    if (!get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) || !get(f, tags, (size_t)m) || !get(f, want_src, (size_t)k) ||
        !get(f, want_dst, (size_t)k) || !get(f, want_inlier, (size_t)k) || !get(f, want_R, 9) || !get(f, want_t, 3)) return 2;
    try {
        DescriptorIndex index(m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        svo_align_params prm = DescriptorIndex::align_params(inlier_dist);
        prm.src_lo = hdr[1]; prm.src_hi = hdr[2]; prm.dst_lo = hdr[3]; prm.dst_hi = hdr[4]; prm.hypotheses = hdr[6]; prm.min_pairs = hdr[7];
        // rule 1: the same rows as a search with a host copy of the source's descriptors
        const std::vector<Descriptor> copy(desc.begin() + prm.src_lo, desc.begin() + prm.src_hi);
        const std::vector<svo_desc_match> rows = index.match_rows({prm.src_lo, prm.src_hi}, {prm.dst_lo, prm.dst_hi}), plain = index.match(copy, prm.dst_lo, prm.dst_hi);
        if (rows.size() != plain.size() || memcmp(rows.data(), plain.data(), rows.size() * sizeof(svo_desc_match))) { std::printf("match_rows differs from match\n"); return 1; }
        const DescriptorIndex::Pairs pr = index.pair_rows(prm);
        if (pr.src != want_src || pr.dst != want_dst || !pr.inlier.empty()) { std::printf("pair_rows: %zu pairs, %d expected\n", pr.src.size(), k); return 1; }
        DescriptorIndex::Pairs pairs;
        const svo_align_result r = index.align(prm, &pairs);
        if (!r.success || r.n_pairs != k || pairs.src != want_src || pairs.dst != want_dst || pairs.inlier != want_inlier) { std::printf("align: the pairs or the inliers differ\n"); return 1; }
        double dt = 0;
        for (int i = 0; i < 3; i++) dt = std::fmax(dt, std::fabs(r.t[i] - want_t[(size_t)i]));
        std::printf("t differs by %.3g m, R by %.3g rad, rms %.3g\n", dt, angle(r.R, want_R.data()), r.rms);
        if (dt > 1e-6 || angle(r.R, want_R.data()) > 1e-6) { std::printf("align: the transform differs from the reference\n"); return 1; }
        for (int i = 0; i < 3; i++)
            if (r.T[4 * i + 3] != r.t[i] || r.T[4 * i] != r.R[3 * i] || r.T[4 * i + 2] != r.R[3 * i + 2] || r.T[12 + i] != 0. || r.T[15] != 1.) { std::printf("T is not (R, t)\n"); return 1; }
        // the round trip
        const std::pair<int, int> moved = index.transform_points(r.T, {prm.src_lo, prm.src_hi});
        if (moved.first != prm.src_hi - prm.src_lo || moved.second != 0) { std::printf("transform_points moved %d rows\n", moved.first); return 1; }
        const svo_align_result again = index.align(prm);
        const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        double t2 = 0;
        for (int i = 0; i < 3; i++) t2 = std::fmax(t2, std::fabs(again.t[i]));
        std::printf("after the transform: t %.3g m, R %.3g rad\n", t2, angle(again.R, eye));
        // the moved points were rounded to f32 at up to 80 m (half an ulp: 4e-6 m a coordinate), which the fit averages over its
        // hundreds of inliers: the least-squares fit of the moved points is the identity but for that
        if (!again.success || again.n_inliers != r.n_inliers || t2 > 1e-6 || angle(again.R, eye) > 1e-6) { std::printf("the second alignment is not the identity\n"); return 1; }
        // a refusal: spans that share a row
        svo_align_params bad = prm;
        bad.dst_hi = prm.src_lo + 1; bad.dst_lo = 0;
        DescriptorIndex::Pairs kept = pairs;
        bool threw = false;
        try { index.align(bad, &kept); } catch (const std::runtime_error&) { threw = true; }
        if (!threw || kept.src != pairs.src || kept.inlier != pairs.inlier) { std::printf("overlapping spans were accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("ALIGN FACADE OK\n");
    return 0;
}
