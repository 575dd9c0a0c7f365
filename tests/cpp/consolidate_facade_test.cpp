// The C++ facade's landmark consolidation (include/svo/visual_odometry.hpp: DescriptorIndex::consolidate_params, consolidate,
// read_rows) on a real GPU, against the caller's reference (written into the input): read_rows gives back what add_points took;
// consolidate's record and kept_before; read_rows of the whole index byte for byte afterwards; the same call twice; and refusals
// that throw.
// argv[1]: int32 {m, row_lo, row_hi, tag_lo, tag_hi, k, 6 int32 of the expected record}, the radius (float), m descriptors of 32
// bytes, m ids (uint64), m points (3 floats), m tags (int32), m + 1 int32 of kept_before, then the k rows expected afterwards in the
// same four arrays (tests/test_gpu_consolidate_facade.py).
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

static bool same(const DescriptorIndex::Rows& r, const std::vector<Descriptor>& desc, const std::vector<uint64_t>& ids, const std::vector<float>& xyz,
                 const std::vector<int32_t>& tags) {
    return r.desc == desc && r.ids == ids && r.tags == tags && r.xyz.size() == xyz.size() &&
           (xyz.empty() || memcmp(r.xyz.data(), xyz.data(), xyz.size() * sizeof(float)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[12];
    float radius;
    if (!f.read((char*)hdr, sizeof(hdr)) || !f.read((char*)&radius, sizeof(radius))) return 2;
    const size_t m = (size_t)hdr[0], k = (size_t)hdr[5];
    std::vector<Descriptor> desc, desc2;
    std::vector<float> xyz, xyz2;
    std::vector<uint64_t> ids, ids2;
    std::vector<int32_t> tags, tags2, want_map;
    if (!get(f, desc, m) || !get(f, ids, m) || !get(f, xyz, 3 * m) || !get(f, tags, m) || !get(f, want_map, m + 1) || !get(f, desc2, k) || !get(f, ids2, k) ||
        !get(f, xyz2, 3 * k) || !get(f, tags2, k)) return 2;
    try {
        DescriptorIndex index((int)m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        if (!same(index.read_rows(), desc, ids, xyz, tags)) { std::printf("read_rows differs from what add_points took\n"); return 1; }
        const DescriptorIndex::Rows part = index.read_rows(3, 10, false);
        if (part.desc.size() != 7 || part.ids[0] != ids[3] || !part.xyz.empty() || !part.tags.empty()) { std::printf("read_rows(3, 10) differs\n"); return 1; }
        svo_consolidate_params prm = DescriptorIndex::consolidate_params(radius);
        if (prm.row_lo != 0 || prm.row_hi != -1 || prm.tag_lo != 0 || prm.tag_hi != INT32_MAX || prm.radius != radius || prm.reserved != 0) {
            std::printf("the defaults differ from svo.h\n"); return 1;
        }
        prm.row_lo = hdr[1]; prm.row_hi = hdr[2]; prm.tag_lo = hdr[3]; prm.tag_hi = hdr[4];
        std::vector<int32_t> kept_before;
        const svo_consolidate_result r = index.consolidate(prm, &kept_before);
        std::printf("members %d, groups %d, dropped %d, far views %d, capped %d, kept %d\n", r.n_members, r.n_groups, r.n_dropped, r.n_far_views,
                    r.n_capped_groups, r.n_kept);
        if (memcmp(&r, hdr + 6, 6 * sizeof(int32_t)) != 0 || r.reserved[0] != 0 || r.reserved[1] != 0) { std::printf("the record differs from the reference\n"); return 1; }
        if (kept_before != want_map || index.size() != (int)k) { std::printf("kept_before differs from the reference\n"); return 1; }
        if (!same(index.read_rows(), desc2, ids2, xyz2, tags2)) { std::printf("the rows differ from the reference\n"); return 1; }
        prm.row_hi = hdr[2] == -1 ? -1 : want_map[(size_t)hdr[2]];
        const svo_consolidate_result again = index.consolidate(prm);
        if (again.n_dropped != 0 || again.n_kept != (int)k || !same(index.read_rows(), desc2, ids2, xyz2, tags2)) { std::printf("the second call changed something\n"); return 1; }
        // refusals: each throws
        int threw = 0;
        svo_consolidate_params bad = prm;
        bad.radius = -1.f;
        try { index.consolidate(bad); } catch (const std::runtime_error&) { threw++; }
        bad = prm; bad.row_lo = 5; bad.row_hi = 3;
        try { index.consolidate(bad); } catch (const std::runtime_error&) { threw++; }
        try { index.read_rows(0, (int)k + 1); } catch (const std::runtime_error&) { threw++; }
        DescriptorIndex plain(16);                     // no points
        plain.add({desc[0], desc[1], desc[2]}, {ids[0], ids[1], ids[2]});
        try { plain.consolidate(DescriptorIndex::consolidate_params(radius)); } catch (const std::runtime_error&) { threw++; }
        try { plain.read_rows(); } catch (const std::runtime_error&) { threw++; }
        const DescriptorIndex::Rows three = plain.read_rows(0, -1, false);
        if (threw != 5 || three.desc.size() != 3 || three.desc[2] != desc[2] || three.ids[1] != ids[1]) { std::printf("%d of 5 refusals threw\n", threw); return 1; }
        if (!same(index.read_rows(), desc2, ids2, xyz2, tags2)) { std::printf("a refused call changed something\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("CONSOLIDATE FACADE OK\n");
    return 0;
}
