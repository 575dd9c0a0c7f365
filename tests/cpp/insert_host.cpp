// insert_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_insert.hpp, the rules of the descriptor index's
// batched insertion compiled for the host from the text svo_match_api.hip and the kernels run (tests/test_insert_host.py builds it
// with AddressSanitizer and UBSan and runs it): the keep predicate, the id rule, the point rule, the plan of tiles and the entry of a
// tile, the rank and the count of a tile's masks, the layout of the working memory; and, against the vectors of the numpy reference
// in argv[1], the whole call twice — as the sequential program (insert_plain) and as the kernels run it, tile by tile and lane by
// lane: masks, the scan of the counts, and each kept lane's place.
// argv[1]: int32 n_cases; per case int32 {n, need_flags, with_points, has_T, total_rows, want_total (-1: a non-finite point)}, then
// n x int32 rows, total_rows x 64 bytes obs, total_rows x 32 bytes desc, n x uint64 id_base, n x int32 tags, n x 16 doubles, n x
// int32 want_added, and for want_total >= 0: want_total x 32 bytes desc, x uint64 ids, x 3 floats, x int32 tags (the last two only
// with_points).
#include "../../stereo_visual_odometry_amd/csrc/svo_insert.hpp"
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static void test_rules() {
    CHECK(insert_need(1, false) == 1 && insert_need(1, true) == 3 && insert_need(0, true) == 2 && insert_need(0, false) == 0);
    CHECK(insert_keep(0, 0) && insert_keep(7, 0) && insert_keep(1, 1) && !insert_keep(2, 1) && insert_keep(3, 3) && !insert_keep(1, 3) && !insert_keep(0, 2));
    CHECK(insert_keep(-1, 0x80000001u) && !insert_keep(0x7FFFFFFF, 0x80000000u));
    CHECK(insert_id(5, 7) == 12 && insert_id(-1, 0) == ~(uint64_t)0 && insert_id(-1, 1) == 0 && insert_id(3, ~(uint64_t)0) == 2);
    CHECK(insert_id(std::numeric_limits<int64_t>::min(), (uint64_t)1 << 63) == 0);
    CHECK(insert_tiles(0) == 0 && insert_tiles(1) == 1 && insert_tiles(256) == 1 && insert_tiles(257) == 2 && insert_tiles(513) == 3 && insert_tiles(1 << 18) == 1024);
    const float p[3] = {1.5f, -2.25f, 1e30f};
    float q[3], r[3];
    insert_point(nullptr, p, q);
    CHECK(memcmp(p, q, 12) == 0 && insert_point_ok(q));
    const double T[16] = {0.25, 1e-3, 3.0, -7.5, 1.0 / 3.0, 2.0, 1e-20, 0.1, 1e10, -1e10, 1e-9, 4.0, 0, 0, 0, 1};
    insert_point(T, p, q); reloc_map_point(T, p, r);
    CHECK(memcmp(q, r, 12) == 0);
    CHECK(q[0] == (float)(((0.25 * (double)p[0] + 1e-3 * (double)p[1]) + 3.0 * (double)p[2]) + -7.5));
    const double big[16] = {1e39, 0, 0, 0, 0, 1e39, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    insert_point(big, p, q);
    CHECK(!insert_point_ok(q) && insert_point_ok(p));
    const float nan3[3] = {0.f, std::numeric_limits<float>::quiet_NaN(), 0.f};
    CHECK(!insert_point_ok(nan3));
}

static void test_masks() {
    uint64_t m[4] = {~(uint64_t)0, 0, (uint64_t)1 << 63 | 1, 0x00FF00FF00FF00FFull};
    CHECK(insert_tile_count(m) == 64 + 0 + 2 + 32);
    CHECK(insert_rank(m, 0, 0) == 0 && insert_rank(m, 0, 63) == 63 && insert_rank(m, 2, 0) == 64 && insert_rank(m, 2, 63) == 65 && insert_rank(m, 3, 0) == 66 && insert_rank(m, 3, 16) == 74);
    CHECK(insert_kept(m, 0, 17) && !insert_kept(m, 1, 0) && insert_kept(m, 2, 63) && !insert_kept(m, 2, 62) && insert_kept(m, 3, 7) && !insert_kept(m, 3, 8));
}

static void test_plan() {
    const int32_t rows[9] = {0, 0, 300, 0, 1, 256, 0, 513, 0};
    InsertEntry e[9];
    for (int b = 0; b < 9; b++) e[b] = InsertEntry{b * 1000, rows[b], -1, 0, 0, 0};
    const int32_t tiles = insert_plan(9, e);
    CHECK(tiles == 2 + 1 + 1 + 3);
    const int32_t want[7] = {2, 2, 4, 5, 7, 7, 7};
    for (int t = 0; t < tiles; t++) {
        const int32_t b = insert_tile_entry(e, 9, t);
        CHECK(b == want[t] && e[b].tile0 <= t && t < e[b].tile0 + insert_tiles(e[b].rows));
    }
    InsertEntry one{0, 5, -1, 0, 0, 0};
    CHECK(insert_plan(1, &one) == 1 && insert_tile_entry(&one, 1, 0) == 0);
    std::vector<InsertEntry> many(INSERT_MAX_ENTRIES);
    for (int b = 0; b < INSERT_MAX_ENTRIES; b++) many[(size_t)b] = InsertEntry{0, 1 + b % 3, -1, 0, 0, 0};
    CHECK(insert_plan(INSERT_MAX_ENTRIES, many.data()) == INSERT_MAX_ENTRIES);
    for (int t = 0; t < INSERT_MAX_ENTRIES; t++) CHECK(insert_tile_entry(many.data(), INSERT_MAX_ENTRIES, t) == t);
}

static void test_layout() {
    CHECK(sizeof(InsertEntry) == 32 && sizeof(InsertCtl) == 64);
    const InsertLayout l = insert_layout(INSERT_MAX_ENTRIES, INSERT_MAX_ENTRIES + INSERT_MAX_OBS_ROWS / INSERT_TILE, INSERT_MAX_OBS_ROWS);
    CHECK(l.entry == 0 && l.T == 32 * 1024 && l.up_end == l.T + 96 * 1024 && l.mask == l.up_end);
    CHECK(l.offset == l.mask + 32 * 2048 && l.down == l.offset + insert_round(4 * 2049) && l.n_added == l.down + 64 && l.down_end == l.down + 64 + 4096 + 192);
    CHECK(l.desc - l.obs == (size_t)64 << 18 && l.total - l.desc == (size_t)32 << 18);
    CHECK(l.total - l.obs == (size_t)24 << 20);                            // the staged rows: 24 MiB at the most
    for (size_t v : {l.T, l.up_end, l.mask, l.offset, l.down, l.down_end, l.obs, l.desc, l.total}) CHECK(v % 256 == 0);
    const InsertLayout s = insert_layout(1, 1, 0);
    CHECK(s.T == 256 && s.up_end == 512 && s.offset == 768 && s.down == 1024 && s.n_added == 1088 && s.down_end == 1280 && s.total == 1280);
    CHECK(insert_layout(3, 0, 0).T == insert_layout(3, 77, 5).T);           // where the transforms go depends on the entries alone
}

struct Reader {
    FILE* f;
    template <typename T> std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("FAIL: short vector file\n"); g_fail++; }
        return v;
    }
};

// the call as the three kernels run it: -> the kept rows, each written at offset[tile] + rank; -2 where two lanes took one place
static int32_t as_the_kernels(int32_t n, std::vector<InsertEntry>& e, const uint8_t* obs, const uint8_t* desc, uint32_t need, bool with_points, const double* T,
                              uint8_t* out_desc, uint64_t* out_ids, float* out_xyz, int32_t* out_tag, int32_t* n_added) {
    const int32_t tiles = insert_plan(n, e.data());
    std::vector<uint64_t> mask((size_t)tiles * INSERT_TILE_WAVES, 0);
    for (int32_t t = 0; t < tiles; t++)                                     // k_insert_count
        for (int32_t lane = 0; lane < INSERT_TILE; lane++) {
            const InsertEntry& en = e[(size_t)insert_tile_entry(e.data(), n, t)];
            const int32_t r = (t - en.tile0) * INSERT_TILE + lane;
            if (r >= en.rows) continue;
            int32_t flags;
            memcpy(&flags, obs + (size_t)(en.begin + r) * INSERT_OBS_BYTES + INSERT_OBS_FLAGS, 4);
            if (insert_keep(flags, need)) mask[(size_t)t * INSERT_TILE_WAVES + lane / 64] |= (uint64_t)1 << (lane % 64);
        }
    std::vector<int32_t> offset((size_t)tiles + 1, 0);                      // k_insert_scan
    for (int32_t t = 0; t < tiles; t++) offset[(size_t)t + 1] = offset[(size_t)t] + insert_tile_count(&mask[(size_t)t * INSERT_TILE_WAVES]);
    for (int32_t b = 0; b < n; b++) n_added[b] = offset[(size_t)(e[(size_t)b].tile0 + insert_tiles(e[(size_t)b].rows))] - offset[(size_t)e[(size_t)b].tile0];
    const int32_t total = offset[(size_t)tiles];
    std::vector<uint8_t> written((size_t)total, 0);
    bool bad = false, clash = false;
    for (int32_t t = tiles - 1; t >= 0; t--)                                // k_insert_put, in an order of its own: the places do not depend on it
        for (int32_t lane = INSERT_TILE - 1; lane >= 0; lane--) {
            const uint64_t* m = &mask[(size_t)t * INSERT_TILE_WAVES];
            if (!insert_kept(m, lane / 64, lane % 64)) continue;
            const int32_t b = insert_tile_entry(e.data(), n, t);
            const InsertEntry& en = e[(size_t)b];
            const int32_t row = en.begin + (t - en.tile0) * INSERT_TILE + lane, to = offset[(size_t)t] + insert_rank(m, lane / 64, lane % 64);
            if (to < 0 || to >= total || written[(size_t)to]) { clash = true; continue; }
            written[(size_t)to] = 1;
            memcpy(out_desc + (size_t)to * INSERT_DESC_BYTES, desc + (size_t)row * INSERT_DESC_BYTES, INSERT_DESC_BYTES);
            int64_t id; float p[3], q[3];
            memcpy(&id, obs + (size_t)row * INSERT_OBS_BYTES + INSERT_OBS_ID, 8);
            memcpy(p, obs + (size_t)row * INSERT_OBS_BYTES + INSERT_OBS_XYZ, 12);
            out_ids[to] = insert_id(id, en.id_base);
            if (!with_points) continue;
            insert_point(T ? T + 12 * (size_t)b : nullptr, p, q);
            if (!insert_point_ok(q)) bad = true;
            memcpy(out_xyz + 3 * (size_t)to, q, 12); out_tag[to] = en.tag;
        }
    return clash ? -2 : bad ? -1 : total;
}

static void test_vectors(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { printf("FAIL: cannot open %s\n", path); g_fail++; return; }
    Reader rd{f};
    const int32_t n_cases = rd.take<int32_t>(1)[0];
    int rows_seen = 0;
    for (int32_t c = 0; c < n_cases && !g_fail; c++) {
        const std::vector<int32_t> h = rd.take<int32_t>(6);
        const int32_t n = h[0], total_rows = h[4], want_total = h[5];
        const bool with_points = h[2] != 0, has_T = h[3] != 0;
        const uint32_t need = insert_need((uint32_t)h[1], with_points);
        const std::vector<int32_t> rows = rd.take<int32_t>((size_t)n);
        const std::vector<uint8_t> obs = rd.take<uint8_t>((size_t)total_rows * 64), desc = rd.take<uint8_t>((size_t)total_rows * 32);
        const std::vector<uint64_t> id_base = rd.take<uint64_t>((size_t)n);
        const std::vector<int32_t> tags = rd.take<int32_t>((size_t)n);
        const std::vector<double> T16 = rd.take<double>((size_t)n * 16);
        const std::vector<int32_t> want_added = rd.take<int32_t>((size_t)n);
        const size_t wt = want_total > 0 ? (size_t)want_total : 0;
        const std::vector<uint8_t> want_desc = rd.take<uint8_t>(wt * 32);
        const std::vector<uint64_t> want_ids = rd.take<uint64_t>(wt);
        const std::vector<float> want_xyz = rd.take<float>(with_points ? wt * 3 : 0);
        const std::vector<int32_t> want_tag = rd.take<int32_t>(with_points ? wt : 0);
        std::vector<InsertEntry> e((size_t)n);
        std::vector<double> T12((size_t)n * 12);
        int32_t at = 0;
        for (int32_t b = 0; b < n; b++) {
            e[(size_t)b] = InsertEntry{at, rows[(size_t)b], 0, tags[(size_t)b], id_base[(size_t)b], 0};
            at += rows[(size_t)b];
            memcpy(&T12[(size_t)b * 12], &T16[(size_t)b * 16], 96);
        }
        CHECK(at == total_rows);
        for (int pass = 0; pass < 2; pass++) {
            std::vector<uint8_t> out_desc((size_t)total_rows * 32 + 1);
            std::vector<uint64_t> out_ids((size_t)total_rows + 1);
            std::vector<float> out_xyz((size_t)total_rows * 3 + 1);
            std::vector<int32_t> out_tag((size_t)total_rows + 1), n_added((size_t)n + 1);
            const int32_t got = pass == 0
                ? (insert_plan(n, e.data()), insert_plain(n, e.data(), obs.data(), desc.data(), need, with_points, has_T ? T12.data() : nullptr, out_desc.data(), out_ids.data(), out_xyz.data(), out_tag.data(), n_added.data()))
                : as_the_kernels(n, e, obs.data(), desc.data(), need, with_points, has_T ? T12.data() : nullptr, out_desc.data(), out_ids.data(), out_xyz.data(), out_tag.data(), n_added.data());
            CHECK(got == want_total);
            if (got != want_total) printf("  case %d pass %d: got %d want %d\n", c, pass, got, want_total);
            CHECK(memcmp(n_added.data(), want_added.data(), 4 * (size_t)n) == 0);
            if (want_total <= 0) continue;                                  // nothing kept: nothing to compare (and no null for memcmp)
            CHECK(memcmp(out_desc.data(), want_desc.data(), wt * 32) == 0 && memcmp(out_ids.data(), want_ids.data(), wt * 8) == 0);
            if (with_points) CHECK(memcmp(out_xyz.data(), want_xyz.data(), wt * 12) == 0 && memcmp(out_tag.data(), want_tag.data(), wt * 4) == 0);
        }
        rows_seen += total_rows;
    }
    fclose(f);
    printf("%d cases, %d rows\n", n_cases, rows_seen);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: insert_host vectors.bin\n"); return 2; }
    test_rules(); test_masks(); test_plan(); test_layout(); test_vectors(argv[1]);
    if (g_fail) { printf("INSERT HOST FAILED: %d\n", g_fail); return 1; }
    printf("INSERT HOST OK\n");
    return 0;
}
