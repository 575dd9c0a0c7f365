// A stand-alone host program over stereo_visual_odometry_amd/csrc/svo_reloc.hpp — the text k_reloc_select and the index's host code
// run — built with AddressSanitizer and UBSan by tests/test_reloc_host.py and compared with tables tests/reloc_ref.py wrote.
// The selection is walked the way the kernel walks it (the accepted list in increasing j, every entry against the whole list, the
// survivors in list order), serially, through the header's own predicates.
// argv[1]: a sequence of cases until the end of the file, each
//   int32 {n, m, max_dist, ratio_num, ratio_den, k}, n result rows of 32 bytes {u64 id, id2; i32 row, row2; u16 dist, dist2; u32 0},
//   m tags (int32), k expected queries, k expected rows (int32),
// then a case with n = -1: int32 {-1, count}, 16 doubles T, count x 3 floats in, count x 3 floats expected.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "../../stereo_visual_odometry_amd/csrc/svo_reloc.hpp"

struct Row { uint64_t id, id2; int32_t row, row2; uint16_t dist, dist2; uint32_t reserved; };
static_assert(sizeof(Row) == 32 && sizeof(RelocPoint) == 16, "row sizes");

static void select(const std::vector<Row>& m, const std::vector<int32_t>& tags, const RelocRule& rule, std::vector<int32_t>& cq, std::vector<int32_t>& cr) {
    std::vector<uint64_t> id;
    std::vector<uint32_t> key;
    for (int j = 0; j < (int)m.size(); j++) {
        const int32_t tag = m[j].row >= 0 ? tags[(size_t)m[j].row] : SVO_RELOC_POINT_NONE;
        if (!reloc_accept(m[j].row, tag, m[j].dist, m[j].dist2, rule)) continue;
        id.push_back(m[j].id); key.push_back(reloc_key(m[j].dist, j));
    }
    for (size_t e = 0; e < id.size(); e++) {
        bool lost = false;
        for (size_t b = 0; b < id.size(); b++) lost = lost || reloc_loses(id[e], key[e], id[b], key[b]);
        if (lost) continue;
        const int32_t j = reloc_key_query(key[e]);
        cq.push_back(j); cr.push_back(m[(size_t)j].row);
    }
}

template <typename T> static bool get(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || (bool)f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int cases = 0, points = 0;
    int32_t hdr[6];
    while (f.read((char*)hdr, 2 * sizeof(int32_t))) {
        if (hdr[0] == -1) {                                       // the transform
            std::vector<double> T; std::vector<float> in, want;
            if (!get(f, T, 16) || !get(f, in, 3 * (size_t)hdr[1]) || !get(f, want, 3 * (size_t)hdr[1])) return 2;
            for (int i = 0; i < hdr[1]; i++) {
                float out[3];
                reloc_map_point(T.data(), &in[3 * (size_t)i], out);
                if (memcmp(out, &want[3 * (size_t)i], sizeof(out))) { std::printf("FAILED: point %d of a transform\n", i); return 1; }
                points++;
            }
            continue;
        }
        if (!f.read((char*)(hdr + 2), 4 * sizeof(int32_t))) return 2;
        const int n = hdr[0], m = hdr[1], k = hdr[5];
        if (n < 0 || n > SVO_RELOC_MAX_QUERIES || m < 0 || k < 0 || k > n) return 2;
        std::vector<Row> rows; std::vector<int32_t> tags, want_q, want_r, cq, cr;
        if (!get(f, rows, (size_t)n) || !get(f, tags, (size_t)m) || !get(f, want_q, (size_t)k) || !get(f, want_r, (size_t)k)) return 2;
        for (const Row& r : rows) if (r.row >= m) return 2;
        select(rows, tags, RelocRule{hdr[2], hdr[3], hdr[4]}, cq, cr);
        if (cq != want_q || cr != want_r) { std::printf("FAILED: case %d (n = %d): %zu candidates, %d expected\n", cases, n, cq.size(), k); return 1; }
        cases++;
    }
    // the key: (dist, j) order, and the query back out of it at both ends
    if (!(reloc_key(3, 4095) < reloc_key(4, 0)) || !(reloc_key(3, 5) < reloc_key(3, 6)) || reloc_key_query(reloc_key(256, 4095)) != 4095 ||
        reloc_key_query(reloc_key(0, 0)) != 0 || reloc_loses(7, reloc_key(1, 1), 7, reloc_key(1, 1))) { std::printf("FAILED: the key\n"); return 1; }
    if (cases < 1 || points < 1) { std::printf("FAILED: %d cases, %d points read\n", cases, points); return 1; }
    std::printf("RELOC HOST OK (%d cases, %d points)\n", cases, points);
    return 0;
}
