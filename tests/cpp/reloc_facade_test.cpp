// The C++ facade's relocaliser (include/svo/visual_odometry.hpp: DescriptorIndex::enable_points, add_points, select, localize) against
// the C-ABI and the caller's reference: the candidates select returns are the reference's; localize's pose, inlier flags and
// iteration count are svo_camera_to_world's on the candidate arrays svo_desc_index_select returns, byte for byte; enabling points on
// a filled index, add_points without points and min_candidates < 6 throw.
// argv[1]: int32 {n, m, k}, float K[9], n queries of 32 bytes, n pixels (2 floats), m descriptors of 32 bytes, m ids (uint64),
// m points (3 floats), m tags (int32), k expected queries, k expected rows (tests/test_gpu_reloc_facade.py).
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
template <typename F> static bool throws(F f) {
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[3];
    float K[9];
    if (!f.read((char*)hdr, sizeof(hdr)) || !f.read((char*)K, sizeof(K))) return 2;
    const int n = hdr[0], m = hdr[1], k = hdr[2];
    std::vector<Descriptor> query, desc;
    std::vector<float> xy, xyz;
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags, want_q, want_r;
    if (!get(f, query, (size_t)n) || !get(f, xy, 2 * (size_t)n) || !get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) ||
        !get(f, tags, (size_t)m) || !get(f, want_q, (size_t)k) || !get(f, want_r, (size_t)k)) return 2;
    try {
        DescriptorIndex plain(m), index(m);
        if (!throws([&] { plain.add_points(desc, ids, xyz, tags); })) { std::printf("add_points on an index without points\n"); return 1; }
        plain.add(desc, ids);
        if (!throws([&] { plain.enable_points(); }) || plain.size() != m) { std::printf("points enabled on a filled index\n"); return 1; }
        index.enable_points();
        const int cut = m / 2;
        const std::vector<Descriptor> d0(desc.begin(), desc.begin() + cut), d1(desc.begin() + cut, desc.end());
        const std::vector<uint64_t> i0(ids.begin(), ids.begin() + cut), i1(ids.begin() + cut, ids.end());
        const std::vector<float> p0(xyz.begin(), xyz.begin() + 3 * cut), p1(xyz.begin() + 3 * cut, xyz.end());
        const std::vector<int32_t> t0(tags.begin(), tags.begin() + cut), t1(tags.begin() + cut, tags.end());
        if (index.add_points(d0, i0, p0, t0) != 0 || index.add_points(d1, i1, p1, t1) != cut || index.size() != m) { std::printf("add_points: first rows / size\n"); return 1; }
        svo_reloc_params prm = DescriptorIndex::default_params();
        if (prm.max_dist != 40 || prm.ratio_num != 7 || prm.ratio_den != 10 || prm.min_candidates != 6 || prm.row_lo != 0 || prm.row_hi != -1) { std::printf("default parameters\n"); return 1; }
        const DescriptorIndex::Candidates sel = index.select(query, xy, prm);
        if (sel.query != want_q || sel.row != want_r) { std::printf("select: %zu candidates, %d expected\n", sel.query.size(), k); return 1; }
        // the arrays the PnP reads, from the C entry, and svo_camera_to_world on them
        std::vector<float> cxy(2 * (size_t)n), cxyz(3 * (size_t)n);
        int kc = 0;
        svo_throw(svo_desc_index_select(index.handle(), n, query[0].data(), xy.data(), &prm, &kc, nullptr, nullptr, cxy.data(), cxyz.data()));
        if (kc != k) { std::printf("the C entry's count\n"); return 1; }
        svo_reloc_result guess;
        memset(&guess, 0, sizeof(guess));
        guess.R[0] = guess.R[4] = guess.R[8] = 1;
        double R[9], t[3];
        memcpy(R, guess.R, sizeof(R)); memcpy(t, guess.t, sizeof(t));
        std::vector<int> inl((size_t)k);
        int n_inl = 0, ok = 0, iters = 0;
        svo_throw(svo_camera_to_world(0, K, k, cxy.data(), cxyz.data(), R, t, inl.data(), &n_inl, &ok, prm.ransac_iterations, prm.reproj_error, prm.confidence, &iters));
        DescriptorIndex::Candidates cand;
        DescriptorIndex moved(std::move(index));
        const svo_reloc_result got = moved.localize(K, query, xy, prm, guess, &cand);
        if (!ok || !got.success || got.n_candidates != k || cand.query != want_q || cand.row != want_r) { std::printf("localize: success / candidates\n"); return 1; }
        if (memcmp(got.R, R, sizeof(R)) || memcmp(got.t, t, sizeof(t)) || got.iters_run != iters || got.n_inliers != n_inl) { std::printf("localize differs from svo_camera_to_world\n"); return 1; }
        std::vector<uint8_t> flags((size_t)k, 0);
        for (int i = 0; i < n_inl; i++) flags[(size_t)inl[(size_t)i]] = 1;
        if (flags != cand.inlier || n_inl < k / 2) { std::printf("the inlier sets differ (%d inliers)\n", n_inl); return 1; }
        double T[16];
        svo_throw(svo_inverse_transform(0, got.R, got.t, T));
        if (memcmp(T, got.T, sizeof(T))) { std::printf("T is not the inverse of (R, t)\n"); return 1; }
        prm.min_candidates = 5;
        if (!throws([&] { moved.select(query, xy, prm); })) { std::printf("min_candidates = 5 was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("RELOC FACADE OK\n");
    return 0;
}
