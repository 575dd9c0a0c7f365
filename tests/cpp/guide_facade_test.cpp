// The C++ facade's guided search (include/svo/visual_odometry.hpp: DescriptorIndex::project, match_guided, select_guided,
// localize_guided) against the C-ABI on the same index: each of the four returns what its C entry returns, byte for byte; the
// candidates are the caller's reference (written into the input); a negative radius throws.
// argv[1]: int32 {n, m, k}, float K[9], double R[9], double t[3], float radius, n queries of 32 bytes, n pixels (2 floats),
// m descriptors of 32 bytes, m ids (uint64), m points (3 floats), m tags (int32), k expected queries, k expected rows
// (tests/test_gpu_guide_facade.py).
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
    float K[9], radius;
    double R[9], t[3];
    if (!f.read((char*)hdr, sizeof(hdr)) || !f.read((char*)K, sizeof(K)) || !f.read((char*)R, sizeof(R)) || !f.read((char*)t, sizeof(t)) ||
        !f.read((char*)&radius, sizeof(radius))) return 2;
    const int n = hdr[0], m = hdr[1], k = hdr[2];
    std::vector<Descriptor> query, desc;
    std::vector<float> xy, xyz;
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags, want_q, want_r;
    if (!get(f, query, (size_t)n) || !get(f, xy, 2 * (size_t)n) || !get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) ||
        !get(f, tags, (size_t)m) || !get(f, want_q, (size_t)k) || !get(f, want_r, (size_t)k)) return 2;
    try {
        DescriptorIndex index(m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        const svo_reloc_guide g = DescriptorIndex::guide(R, t, radius);
        if (memcmp(g.R, R, sizeof(R)) || memcmp(g.t, t, sizeof(t)) || g.radius != radius || g.reserved != 0) { std::printf("guide()\n"); return 1; }
        const svo_reloc_params prm = DescriptorIndex::default_params();
        // project: the whole index and a sub-range
        std::vector<float> uv_c(2 * (size_t)m);
        svo_throw(svo_desc_index_project(index.handle(), K, &g, 0, -1, uv_c.data()));
        const std::vector<float> uv = index.project(K, g), part = index.project(K, g, 3, m - 2);
        if (uv.size() != uv_c.size() || memcmp(uv.data(), uv_c.data(), uv.size() * sizeof(float))) { std::printf("project differs from the C entry\n"); return 1; }
        if (part.size() != 2 * (size_t)(m - 5) || memcmp(part.data(), uv_c.data() + 6, part.size() * sizeof(float))) { std::printf("project: the sub-range\n"); return 1; }
        // match_guided
        std::vector<svo_desc_match> rows_c((size_t)n);
        svo_throw(svo_desc_index_match_guided(index.handle(), K, &g, n, query[0].data(), xy.data(), 0, -1, rows_c.data()));
        const std::vector<svo_desc_match> rows = index.match_guided(K, g, query, xy);
        if (rows.size() != rows_c.size() || memcmp(rows.data(), rows_c.data(), rows.size() * sizeof(svo_desc_match))) { std::printf("match_guided differs from the C entry\n"); return 1; }
        // select_guided: the reference's candidates, and the C entry's arrays for the PnP
        const DescriptorIndex::Candidates sel = index.select_guided(K, g, query, xy, prm);
        if (sel.query != want_q || sel.row != want_r) { std::printf("select_guided: %zu candidates, %d expected\n", sel.query.size(), k); return 1; }
        std::vector<float> cxy(2 * (size_t)n), cxyz(3 * (size_t)n);
        int kc = 0;
        svo_throw(svo_desc_index_select_guided(index.handle(), K, &g, n, query[0].data(), xy.data(), &prm, &kc, nullptr, nullptr, cxy.data(), cxyz.data()));
        if (kc != k) { std::printf("the C entry's count\n"); return 1; }
        // localize_guided: the C entry's result, and svo_camera_to_world on select's arrays
        svo_reloc_result guess;
        memset(&guess, 0, sizeof(guess));
        memcpy(guess.R, R, sizeof(R)); memcpy(guess.t, t, sizeof(t));
        svo_reloc_result res_c = guess;
        std::vector<int32_t> cq((size_t)n), cr((size_t)n);
        std::vector<uint8_t> ci((size_t)n);
        svo_throw(svo_desc_index_localize_guided(index.handle(), K, &g, n, query[0].data(), xy.data(), &prm, &res_c, cq.data(), cr.data(), ci.data()));
        DescriptorIndex::Candidates cand;
        index.set_guided_sort(false);
        const svo_reloc_result got = index.localize_guided(K, g, query, xy, prm, guess, &cand);
        index.set_guided_sort(true);
        if (memcmp(&got, &res_c, sizeof(got)) || !got.success || got.n_candidates != k) { std::printf("localize_guided differs from the C entry\n"); return 1; }
        cq.resize((size_t)k); cr.resize((size_t)k); ci.resize((size_t)k);
        if (cand.query != cq || cand.row != cr || cand.inlier != ci || cand.query != want_q) { std::printf("localize_guided: the candidate lists\n"); return 1; }
        double R2[9], t2[3];
        memcpy(R2, R, sizeof(R2)); memcpy(t2, t, sizeof(t2));
        std::vector<int> inl((size_t)k);
        int n_inl = 0, ok = 0, iters = 0;
        svo_throw(svo_camera_to_world(0, K, k, cxy.data(), cxyz.data(), R2, t2, inl.data(), &n_inl, &ok, prm.ransac_iterations, prm.reproj_error, prm.confidence, &iters));
        if (!ok || memcmp(got.R, R2, sizeof(R2)) || memcmp(got.t, t2, sizeof(t2)) || got.iters_run != iters || got.n_inliers != n_inl) { std::printf("localize_guided differs from svo_camera_to_world\n"); return 1; }
        const svo_reloc_guide bad = DescriptorIndex::guide(R, t, -1.f);
        if (!throws([&] { index.project(K, bad); }) || !throws([&] { index.match_guided(K, bad, query, xy); }) ||
            !throws([&] { index.select_guided(K, bad, query, xy, prm); })) { std::printf("a negative radius was accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("GUIDE FACADE OK\n");
    return 0;
}
