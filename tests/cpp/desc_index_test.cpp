// The C++ facade's descriptor index (include/svo/visual_odometry.hpp: DescriptorIndex) against the C-ABI on the same rows: add in two
// parts, match over the whole index and over a sub-range, truncate and add again — every result row byte for byte the C entry's, and
// the whole-index rows the ones the caller's reference computed; a full index and a bad range throw; the index moves.
// argv[1]: int32 {n, m}, n queries of 32 bytes, m descriptors of 32 bytes, m ids (uint64), n expected svo_desc_match rows
// (tests/test_gpu_desc_index_facade.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "svo/visual_odometry.hpp"

using namespace visual_odometry;
using Descriptor = DescriptorIndex::Descriptor;

static bool same_rows(const std::vector<svo_desc_match>& a, const std::vector<svo_desc_match>& b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(svo_desc_match)));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[2];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int n = hdr[0], m = hdr[1];
    std::vector<Descriptor> query((size_t)n), desc((size_t)m);
    std::vector<uint64_t> ids((size_t)m);
    std::vector<svo_desc_match> want((size_t)n);
    if (!f.read((char*)query.data(), (std::streamsize)n * 32) || !f.read((char*)desc.data(), (std::streamsize)m * 32) ||
        !f.read((char*)ids.data(), (std::streamsize)m * 8) || !f.read((char*)want.data(), (std::streamsize)n * 32)) return 2;
    static_assert(sizeof(svo_desc_match) == 32 && sizeof(Descriptor) == 32, "row sizes");
    svo_desc_index* c_index = nullptr;
    try {
        DescriptorIndex index(m);
        svo_throw(svo_desc_index_create(0, m, &c_index));
        svo_throw(svo_desc_index_set_chunk_rows(index.handle(), 8));          // 27 rows: four pieces
        svo_throw(svo_desc_index_set_chunk_rows(c_index, 8));
        const int cut = m / 3;
        const std::vector<Descriptor> d0(desc.begin(), desc.begin() + cut), d1(desc.begin() + cut, desc.end());
        const std::vector<uint64_t> i0(ids.begin(), ids.begin() + cut), i1(ids.begin() + cut, ids.end());
        if (index.add(d0, i0) != 0 || index.add(d1, i1) != cut || index.size() != m) { std::printf("add: first rows / size\n"); return 1; }
        svo_throw(svo_desc_index_add(c_index, m, desc[0].data(), ids.data(), nullptr));
        std::vector<svo_desc_match> c_rows((size_t)n);
        svo_throw(svo_desc_index_match(c_index, n, query[0].data(), 0, -1, c_rows.data()));
        const auto rows = index.match(query);
        if (!same_rows(rows, c_rows)) { std::printf("the facade and the C entry differ on the whole index\n"); return 1; }
        if (!same_rows(rows, want)) { std::printf("the rows differ from the reference's\n"); return 1; }
        svo_throw(svo_desc_index_match(c_index, n, query[0].data(), 5, m - 3, c_rows.data()));
        if (!same_rows(index.match(query, 5, m - 3), c_rows)) { std::printf("the facade and the C entry differ on a sub-range\n"); return 1; }
        int second_ids = 0;
        for (const auto& r : rows) second_ids += r.row2 >= 0 && r.id2 != r.id;
        if (second_ids < n / 2) { std::printf("too few second neighbours (%d)\n", second_ids); return 1; }
        bool threw = false;
        try { index.add(d0, i0); } catch (const std::runtime_error&) { threw = true; }
        if (!threw || index.size() != m) { std::printf("a full index took rows\n"); return 1; }
        threw = false;
        try { index.match(query, 3, m + 1); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a range beyond the size was accepted\n"); return 1; }
        index.truncate(cut); svo_throw(svo_desc_index_truncate(c_index, cut));
        if (index.add(d0, i0) != cut) { std::printf("add after truncate\n"); return 1; }
        svo_throw(svo_desc_index_add(c_index, cut, d0[0].data(), i0.data(), nullptr));
        svo_throw(svo_desc_index_match(c_index, n, query[0].data(), 0, -1, c_rows.data()));
        DescriptorIndex moved(std::move(index));
        if (moved.size() != 2 * cut || !same_rows(moved.match(query), c_rows)) { std::printf("after truncate + add, moved\n"); return 1; }
        if (!moved.match({}).empty()) { std::printf("no queries gave rows\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_desc_index_destroy(c_index);
        return 1;
    }
    svo_desc_index_destroy(c_index);
    std::printf("DESC INDEX OK\n");
    return 0;
}
