// The C++ facade's index maintenance (include/svo/visual_odometry.hpp: DescriptorIndex::retire, transform_points, retire_slab_rows)
// against the C-ABI on the same rows and against the caller's reference: kept_before entry for entry, every kept row found again at
// its new number with its id, the transform's two counts, and the projections of both indexes byte for byte afterwards; a rule
// with unknown flag bits throws and changes nothing.
// argv[1]: int32 {m, n_drop, tag_lo, tag_hi}, m descriptors of 32 bytes, m ids (uint64), m x 3 floats, m tags (int32), n_drop ids,
// m + 1 expected kept_before (int32) for the scope [2, m - 3) with BY_TAG | BY_IDS | LATEST_PER_ID, 16 doubles T, int32 {moved,
// skipped} expected of transform_points(T, every row, tags [tag_lo, tag_hi]) after the retire (tests/test_gpu_desc_retire_facade.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "svo/visual_odometry.hpp"

using namespace visual_odometry;
using Descriptor = DescriptorIndex::Descriptor;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int32_t hdr[4];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int m = hdr[0], n_drop = hdr[1];
    std::vector<Descriptor> desc((size_t)m);
    std::vector<uint64_t> ids((size_t)m), drop((size_t)n_drop);
    std::vector<float> xyz(3 * (size_t)m);
    std::vector<int32_t> tags((size_t)m), want((size_t)m + 1);
    double T[16];
    int32_t counts[2];
    if (!f.read((char*)desc.data(), (std::streamsize)m * 32) || !f.read((char*)ids.data(), (std::streamsize)m * 8) ||
        !f.read((char*)xyz.data(), (std::streamsize)m * 12) || !f.read((char*)tags.data(), (std::streamsize)m * 4) ||
        !f.read((char*)drop.data(), (std::streamsize)n_drop * 8) || !f.read((char*)want.data(), (std::streamsize)(m + 1) * 4) ||
        !f.read((char*)T, sizeof(T)) || !f.read((char*)counts, sizeof(counts))) return 2;
    svo_desc_index* c_index = nullptr;
    try {
        DescriptorIndex index(m);
        index.enable_points();
        svo_throw(svo_desc_index_create(0, m, &c_index));
        svo_throw(svo_desc_index_enable_points(c_index));
        index.retire_slab_rows(8);
        svo_throw(svo_desc_index_set_retire_slab_rows(c_index, 8));
        if (index.retire_slab_rows() != 8) { std::printf("retire_slab_rows\n"); return 1; }
        index.add_points(desc, ids, xyz, tags);
        svo_throw(svo_desc_index_add_points(c_index, m, desc[0].data(), ids.data(), xyz.data(), tags.data(), nullptr));

        svo_retire_rule bad = DescriptorIndex::retire_rule();
        bad.flags = 16;
        bool threw = false;
        try { index.retire(bad); } catch (const std::runtime_error&) { threw = true; }
        if (!threw || index.size() != m) { std::printf("unknown flag bits were accepted\n"); return 1; }

        svo_retire_rule rule = DescriptorIndex::retire_rule(2, m - 3);
        rule.flags = SVO_RETIRE_BY_TAG | SVO_RETIRE_BY_IDS | SVO_RETIRE_LATEST_PER_ID;
        rule.tag_lo = hdr[2]; rule.tag_hi = hdr[3]; rule.n_ids = n_drop; rule.ids = drop.data();
        const std::vector<int32_t> kept_before = index.retire(rule);
        std::vector<int32_t> c_kept((size_t)m + 1);
        int n_kept = -1;
        svo_throw(svo_desc_index_retire(c_index, &rule, c_kept.data(), &n_kept));
        if (kept_before != want) { std::printf("kept_before differs from the reference's\n"); return 1; }
        if (c_kept != want || n_kept != want.back() || index.size() != n_kept) { std::printf("the C entry's kept_before / size\n"); return 1; }
        if (n_kept == m || n_kept < 4) { std::printf("the case drops nothing or nearly everything (%d of %d)\n", n_kept, m); return 1; }
        const auto rows = index.match(desc);
        for (int r = 0; r < m; r++)
            if (kept_before[(size_t)r + 1] > kept_before[(size_t)r] &&
                (rows[(size_t)r].row != kept_before[(size_t)r] || rows[(size_t)r].dist != 0 || rows[(size_t)r].id != ids[(size_t)r])) {
                std::printf("kept row %d is not at %d\n", r, kept_before[(size_t)r]);
                return 1;
            }
        // a rule without flags keeps everything: the identity
        const std::vector<int32_t> again = index.retire(DescriptorIndex::retire_rule());
        for (int r = 0; r <= n_kept; r++) if (again[(size_t)r] != r) { std::printf("flags == 0 moved a row\n"); return 1; }

        const auto moved = index.transform_points(T, {0, -1}, {hdr[2], hdr[3]});
        int c_moved = -1, c_skipped = -1;
        svo_throw(svo_desc_index_transform_points(c_index, T, 0, -1, hdr[2], hdr[3], &c_moved, &c_skipped));
        if (moved.first != counts[0] || moved.second != counts[1] || c_moved != counts[0] || c_skipped != counts[1]) {
            std::printf("transform_points: %d moved, %d skipped (C entry %d, %d), expected %d, %d\n", moved.first, moved.second, c_moved, c_skipped, counts[0], counts[1]);
            return 1;
        }
        if (counts[0] < 1) { std::printf("the case moves nothing\n"); return 1; }
        const float K[9] = {500, 0, 320, 0, 500, 180, 0, 0, 1};
        const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 30};
        const svo_reloc_guide g = DescriptorIndex::guide(R, t, 1.f);
        const std::vector<float> uv = index.project(K, g);
        std::vector<float> c_uv(uv.size());
        svo_throw(svo_desc_index_project(c_index, K, &g, 0, -1, c_uv.data()));
        if (uv.size() != 2 * (size_t)n_kept || memcmp(uv.data(), c_uv.data(), uv.size() * sizeof(float))) { std::printf("the projections differ\n"); return 1; }
        index.retire_slab_rows(0);
        if (index.retire_slab_rows() != 262144) { std::printf("the default slab\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_desc_index_destroy(c_index);
        return 1;
    }
    svo_desc_index_destroy(c_index);
    std::printf("DESC RETIRE OK\n");
    return 0;
}
