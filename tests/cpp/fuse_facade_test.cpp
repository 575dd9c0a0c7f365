// The C++ facade's landmark fusion (include/svo/visual_odometry.hpp: DescriptorIndex::fuse_params, match_near, pair_near, relabel,
// fuse) on a real GPU, against the caller's reference (written into the input): match_near's rows byte for byte, the dry run's pairs,
// the four counts of fuse and its pairs, the ids afterwards as a search sees them, a second call that finds everything fused, a
// relabel that undoes one landmark, and a refusal that throws and leaves the outputs as they were.
// argv[1]: int32 {m, src_lo, src_hi, dst_lo, dst_hi, k, n_same, n_fused, n_rows}, float radius, m descriptors of 32 bytes, m ids
// (uint64), m points (3 floats), m tags (int32), the src_hi - src_lo expected result rows of match_near (32 bytes each), the k
// expected pairs — source rows, destination rows (int32) — and the m ids expected afterwards (tests/test_gpu_fuse_facade.py).  Every
// row's descriptor is its own, so a search for it over the whole index returns the row with its id.
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

// the ids of the index's rows, read through a search for every row's own descriptor
static bool ids_are(DescriptorIndex& index, const std::vector<Descriptor>& desc, const std::vector<uint64_t>& want) {
    const std::vector<svo_desc_match> rows = index.match(desc, 0, -1);
    for (size_t r = 0; r < rows.size(); r++)
        if (rows[r].row != (int32_t)r || rows[r].dist != 0 || rows[r].id != want[r]) return false;
    return rows.size() == want.size();
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[9];
    float radius;
    if (!f.read((char*)hdr, sizeof(hdr)) || !f.read((char*)&radius, sizeof(radius))) return 2;
    const int m = hdr[0], k = hdr[5];
    std::vector<Descriptor> desc;
    std::vector<float> xyz;
    std::vector<uint64_t> ids, want_ids;
    std::vector<int32_t> tags, want_src, want_dst;
    std::vector<svo_desc_match> want_rows;
    if (!get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) || !get(f, tags, (size_t)m) ||
        !get(f, want_rows, (size_t)(hdr[2] - hdr[1])) || !get(f, want_src, (size_t)k) || !get(f, want_dst, (size_t)k) || !get(f, want_ids, (size_t)m)) return 2;
    try {
        DescriptorIndex index(m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        svo_fuse_params prm = DescriptorIndex::fuse_params(radius);
        prm.src_lo = hdr[1]; prm.src_hi = hdr[2]; prm.dst_lo = hdr[3]; prm.dst_hi = hdr[4];
        const std::vector<svo_desc_match> rows = index.match_near({prm.src_lo, prm.src_hi}, {prm.dst_lo, prm.dst_hi}, radius);
        if (rows.size() != want_rows.size() || memcmp(rows.data(), want_rows.data(), rows.size() * sizeof(svo_desc_match))) { std::printf("match_near differs from the reference\n"); return 1; }
        const DescriptorIndex::Pairs dry = index.pair_near(prm);
        if (dry.src != want_src || dry.dst != want_dst) { std::printf("pair_near: %zu pairs, %d expected\n", dry.src.size(), k); return 1; }
        if (!ids_are(index, desc, ids)) { std::printf("the dry run changed an id\n"); return 1; }
        DescriptorIndex::Pairs pairs;
        const svo_fuse_result r = index.fuse(prm, &pairs);
        std::printf("pairs %d, same %d, fused %d, rows %d\n", r.n_pairs, r.n_same, r.n_fused, r.n_rows_relabelled);
        if (r.n_pairs != k || r.n_same != hdr[6] || r.n_fused != hdr[7] || r.n_rows_relabelled != hdr[8] || pairs.src != want_src || pairs.dst != want_dst) {
            std::printf("fuse: the counts or the pairs differ\n"); return 1;
        }
        if (!ids_are(index, desc, want_ids)) { std::printf("fuse: the ids differ from the reference\n"); return 1; }
        const svo_fuse_result again = index.fuse(prm);
        if (again.n_pairs != k || again.n_same != k || again.n_fused != 0 || again.n_rows_relabelled != 0 || !ids_are(index, desc, want_ids)) {
            std::printf("the second call changed something\n"); return 1;
        }
        // relabel: the first fused landmark of the source span back under its old id, in the source span only
        size_t c = 0;
        while (c < (size_t)k && ids[(size_t)want_src[c]] == ids[(size_t)want_dst[c]]) c++;
        if (c < (size_t)k) {
            const uint64_t old_id = ids[(size_t)want_src[c]], new_id = ids[(size_t)want_dst[c]];
            int expect = 0;
            std::vector<uint64_t> back = want_ids;
            for (int row = prm.src_lo; row < prm.src_hi; row++)
                if (want_ids[(size_t)row] == new_id) { back[(size_t)row] = old_id; expect++; }
            const int changed = index.relabel({new_id, new_id, old_id}, {old_id, 7, old_id}, {prm.src_lo, prm.src_hi});
            if (changed != expect || expect == 0 || !ids_are(index, desc, back)) { std::printf("relabel changed %d rows, %d expected\n", changed, expect); return 1; }
        }
        // a refusal: spans that share a row
        svo_fuse_params bad = prm;
        bad.dst_lo = 0; bad.dst_hi = prm.src_lo + 1;
        DescriptorIndex::Pairs kept = pairs;
        bool threw = false;
        try { index.fuse(bad, &kept); } catch (const std::runtime_error&) { threw = true; }
        if (!threw || kept.src != pairs.src || kept.dst != pairs.dst) { std::printf("overlapping spans were accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("FUSE FACADE OK\n");
    return 0;
}
