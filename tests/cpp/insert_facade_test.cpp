// The C++ facade's batched insertion (include/svo/visual_odometry.hpp: DescriptorIndex::add_obs, add_frames, insert_stats) on a
// real GPU, against the caller's reference (written into the input): add_obs with points onto a non-empty index, the rows read back
// byte for byte, first_row and n_added, the statistics; the plain call on the same index; and refusals that throw and add nothing.
// argv[1]: int32 {n, need_flags, total_rows, want_total}, n + 1 int32 row_begin, total_rows observation rows (64 bytes) and
// descriptors (32 bytes), n uint64 id_base, n int32 tags, n x 16 doubles, then the want_total rows expected — descriptors, ids
// (uint64), points (3 floats), tags (int32) — and n int32 first_row (for an index that held 3 rows) and n int32 n_added
// (tests/test_gpu_insert_facade.py).
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[4];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const size_t n = (size_t)hdr[0], rows = (size_t)hdr[2], k = (size_t)hdr[3];
    const uint32_t need = (uint32_t)hdr[1];
    std::vector<int32_t> row_begin, want_tags, want_first, want_added;
    std::vector<svo_track_obs> obs;
    std::vector<Descriptor> desc, want_desc;
    std::vector<uint64_t> want_ids;
    std::vector<float> want_xyz;
    DescriptorIndex::InsertArgs a;
    if (!get(f, row_begin, n + 1) || !get(f, obs, rows) || !get(f, desc, rows) || !get(f, a.id_base, n) || !get(f, a.tags, n) || !get(f, a.cam_to_map, 16 * n) ||
        !get(f, want_desc, k) || !get(f, want_ids, k) || !get(f, want_xyz, 3 * k) || !get(f, want_tags, k) || !get(f, want_first, n) || !get(f, want_added, n)) return 2;
    try {
        DescriptorIndex index((int)k + 3 + (int)rows);
        index.enable_points();
        const std::vector<Descriptor> three(3, desc[0]);
        index.add_points(three, {7, 8, 9}, std::vector<float>(9, 1.f), {0, 0, 0});
        const DescriptorIndex::Inserted r = index.add_obs(row_begin, obs, desc, true, a, need);
        if (r.first_row != want_first || r.n_added != want_added || index.size() != (int)k + 3) { std::printf("first_row / n_added / size differ from the reference\n"); return 1; }
        const DescriptorIndex::Rows got = index.read_rows(3, -1);
        if (got.desc != want_desc || got.ids != want_ids || got.tags != want_tags || memcmp(got.xyz.data(), want_xyz.data(), 12 * k) != 0) {
            std::printf("the rows differ from the reference\n"); return 1;
        }
        const svo_desc_insert_stats st = index.insert_stats();
        std::printf("path %d, scanned %llu, added %llu\n", st.last_path, (unsigned long long)st.rows_scanned, (unsigned long long)st.rows_added);
        if (st.last_path != SVO_INSERT_PATH_STAGED || st.rows_scanned != rows || st.rows_added != k) { std::printf("the statistics differ\n"); return 1; }
        // the plain call on the index with points: need_flags 0 keeps every row, the points are SVO_POINT_NONE
        DescriptorIndex::InsertArgs plain_args; plain_args.id_base = a.id_base;
        index.truncate(3);
        const DescriptorIndex::Inserted p = index.add_obs(row_begin, obs, desc, false, plain_args, 0);
        const DescriptorIndex::Rows all = index.read_rows(3, -1);
        if (index.size() != 3 + (int)rows || p.first_row[0] != 3 || all.tags.size() != rows) { std::printf("the plain call differs\n"); return 1; }
        for (size_t i = 0; i < rows; i++) if (all.tags[i] != SVO_POINT_NONE || all.desc[i] != desc[i]) { std::printf("the plain call's row %zu differs\n", i); return 1; }
        // refusals: each throws and adds nothing
        int threw = 0;
        const int before = index.size();
        DescriptorIndex::InsertArgs bad = a;
        bad.tags[0] = -1;
        try { index.add_obs(row_begin, obs, desc, true, bad, need); } catch (const std::runtime_error&) { threw++; }
        bad = a; bad.cam_to_map.pop_back();
        try { index.add_obs(row_begin, obs, desc, true, bad, need); } catch (const std::runtime_error&) { threw++; }
        try { index.add_frames(nullptr, 1); } catch (const std::runtime_error&) { threw++; }
        DescriptorIndex no_points(8);
        try { no_points.add_obs(row_begin, obs, desc, true, a, need); } catch (const std::runtime_error&) { threw++; }
        DescriptorIndex small(1);
        try { small.add_obs(row_begin, obs, desc, false, plain_args, 0); } catch (const std::runtime_error&) { threw++; }
        if (threw != 5 || index.size() != before || small.size() != 0) { std::printf("%d of 5 refusals threw\n", threw); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("INSERT FACADE OK\n");
    return 0;
}
