// reloc_batch_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_reloc_batch.hpp, the arithmetic of the batched
// relocalisation compiled for the host from the text svo_match_api.hip and the kernels run (tests/test_reloc_batch_host.py builds it
// with AddressSanitizer and UBSan and runs it): every refusal of a call's offsets; the plan at the maximal shape — 1024 cameras of
// 1024 queries, 1 << 24 rows, chunk rows 1 .. 1 << 24 — and at small ones: every launch's grid within 65 535 along y and z, the
// partial states of every launch within the budget, and every (query, row) covered exactly once; the cell key; the staging's layout.
#include "../../stereo_visual_odometry_amd/csrc/svo_reloc_batch.hpp"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static void test_offsets() {
    std::vector<int32_t> ok{0, 5, 5, 4101};
    CHECK(rb_check_offsets(3, ok.data()) == RB_OFFSETS_OK);
    CHECK(rb_check_offsets(0, nullptr) == RB_OFFSETS_OK);
    CHECK(rb_check_offsets(-1, ok.data()) == RB_OFFSETS_COUNT && rb_check_offsets(RB_MAX_CAMERAS + 1, ok.data()) == RB_OFFSETS_COUNT);
    CHECK(rb_check_offsets(3, nullptr) == RB_OFFSETS_NULL);
    std::vector<int32_t> first{1, 5, 5, 9}, order{0, 5, 4, 9}, slice{0, 5, 4102, 4103}, neg{0, -1, 3, 4};
    CHECK(rb_check_offsets(3, first.data()) == RB_OFFSETS_FIRST);
    CHECK(rb_check_offsets(3, order.data()) == RB_OFFSETS_ORDER);
    CHECK(rb_check_offsets(3, neg.data()) == RB_OFFSETS_ORDER);
    CHECK(rb_check_offsets(3, slice.data()) == RB_OFFSETS_SLICE);
    std::vector<int32_t> full((size_t)RB_MAX_CAMERAS + 1);                // 1024 x 1024: exactly the limit
    for (int b = 0; b <= RB_MAX_CAMERAS; b++) full[(size_t)b] = b * 1024;
    CHECK(rb_check_offsets(RB_MAX_CAMERAS, full.data()) == RB_OFFSETS_OK && full.back() == RB_MAX_QUERIES);
    full.back() += 1;
    CHECK(rb_check_offsets(RB_MAX_CAMERAS, full.data()) == RB_OFFSETS_TOTAL);
    std::vector<int32_t> wide(258);                                       // 256 slices of 4096 and one query more
    for (int b = 0; b < 258; b++) wide[(size_t)b] = b <= 256 ? b * 4096 : RB_MAX_QUERIES + 1;
    CHECK(rb_check_offsets(257, wide.data()) == RB_OFFSETS_TOTAL);
    CHECK(rb_max_slice(3, ok.data()) == 4096 && rb_max_slice(0, nullptr) == 0);
}

// One plan, checked launch by launch.  Coverage is arithmetic: the groups tile the cameras and the queries in order; inside a group
// the guided grid's slots (z x threads) cover every slice once and the unguided grid's waves the concatenated queries; the chunks
// tile [row_lo, row_hi) in order.
static void check_plan(int n_cameras, const std::vector<int32_t>& begin, int row_lo, int row_hi, int chunk_rows) {
    const int max_slice = rb_max_slice(n_cameras, begin.data());
    const RbRange r = rb_plan_range(row_lo, row_hi, chunk_rows, max_slice);
    CHECK(r.chunk_rows >= chunk_rows && r.chunk_rows % chunk_rows == 0 && r.chunk_rows <= (1 << 24));
    int at = row_lo;                                                      // the chunks, in order, without gap or overlap
    for (int j = 0; j < r.n_chunks; j++) {
        int r0, r1;
        rb_chunk_rows(r, j, r0, r1);
        CHECK(r0 == at && r1 > r0 && r1 - r0 <= r.chunk_rows);
        at = r1;
    }
    CHECK(r.n_chunks == 0 ? row_hi <= row_lo : at == row_hi);
    int cam = 0, q = 0, launches = 0;
    while (cam < n_cameras) {
        const RbGroup g = rb_next_group(n_cameras, begin.data(), cam, r.n_chunks);
        CHECK(g.cam0 == cam && g.cam1 > cam && g.cam1 <= n_cameras && g.q0 == q && g.q1 == begin[(size_t)g.cam1]);
        CHECK(rb_group_states(g, r.n_chunks) <= RB_PART_BUDGET);
        int widest = 0;
        for (int b = g.cam0; b < g.cam1; b++) widest = begin[(size_t)b + 1] - begin[(size_t)b] > widest ? begin[(size_t)b + 1] - begin[(size_t)b] : widest;
        CHECK(g.max_n == widest);
        const RbGrid gg = rb_guided_grid(g, r.n_chunks), gu = rb_unguided_grid(g, r.n_chunks);
        if (widest > 0 && r.n_chunks > 0) {
            CHECK(gg.x == r.n_chunks && gg.y == g.cam1 - g.cam0 && gg.y <= RB_GRID_LIMIT && gg.z >= 1 && gg.z <= RB_GRID_LIMIT);
            CHECK(gg.threads % 64 == 0 && gg.threads >= 64 && gg.threads <= RB_BLOCK_SLOTS);
            CHECK((size_t)gg.z * gg.threads >= (size_t)widest && (size_t)(gg.z - 1) * gg.threads < (size_t)widest);   // every slot once, no idle tile group
            CHECK(gu.x == r.n_chunks && gu.y <= RB_GRID_LIMIT && gu.z == 1 && gu.threads == 64);
            CHECK((size_t)gu.y * 64 >= (size_t)(g.q1 - g.q0) && (size_t)(gu.y - 1) * 64 < (size_t)(g.q1 - g.q0));
        } else {
            CHECK(gg.x == 0 && gu.x == 0);
        }
        cam = g.cam1; q = g.q1; launches++;
    }
    CHECK(q == (n_cameras ? begin[(size_t)n_cameras] : 0) && launches <= (n_cameras > 0 ? n_cameras : 0));
}

static void test_plans() {
    std::vector<int32_t> full((size_t)RB_MAX_CAMERAS + 1);
    for (int b = 0; b <= RB_MAX_CAMERAS; b++) full[(size_t)b] = b * 1024;
    for (int chunk = 1; chunk <= (1 << 24); chunk *= 2) check_plan(RB_MAX_CAMERAS, full, 0, 1 << 24, chunk);
    check_plan(RB_MAX_CAMERAS, full, 12345, (1 << 24) - 7, 1000);
    std::vector<int32_t> widest(257);                                     // 256 cameras of 4096
    for (int b = 0; b <= 256; b++) widest[(size_t)b] = b * 4096;
    for (int chunk : {1, 64, 1024, 1 << 20}) check_plan(256, widest, 0, 1 << 24, chunk);
    std::vector<int32_t> ragged{0, 0, 1, 64, 128, 193, 1217, 2242, 6338, 6338, 6343};
    for (int chunk : {1, 7, 64, 1024, 4096})
        for (int lo : {0, 3, 1030})
            for (int hi : {0, 1030, 2621, 2624}) if (lo <= hi) check_plan(10, ragged, lo, hi, chunk);
    std::vector<int32_t> none{0, 0, 0};
    check_plan(2, none, 0, 5000, 64);
    check_plan(0, none, 0, 5000, 64);
    // the budget binds: 1 << 20 queries against 65 536 rows at 1024 rows a chunk are 64 chunks, 16 groups of 64 cameras
    const RbRange r = rb_plan_range(0, 65536, 1024, 1024);
    CHECK(r.n_chunks == 64 && r.chunk_rows == 1024);
    const RbGroup g = rb_next_group(RB_MAX_CAMERAS, full.data(), 0, r.n_chunks);
    CHECK(g.cam1 == 64 && rb_group_states(g, r.n_chunks) == RB_PART_BUDGET);
    // the widest slice decides the rows of a chunk: 4096 queries and 1 << 24 rows at one row a chunk end at 16 384 rows
    CHECK(rb_plan_range(0, 1 << 24, 1, 4096).chunk_rows == 16384 && rb_plan_range(0, 1 << 24, 1, 1).chunk_rows == 256);
}

static void test_keys() {
    CHECK(rb_cell_key(5.f, 5.f, 12.f) < rb_cell_key(30.f, 5.f, 12.f) && rb_cell_key(30.f, 5.f, 12.f) < rb_cell_key(5.f, 30.f, 12.f));
    CHECK(rb_cell_key(5.f, 5.f, 12.f) == rb_cell_key(23.9f, 0.f, 12.f));
    CHECK(rb_cell_key(-1.f, -1.f, 12.f) < rb_cell_key(0.f, 0.f, 12.f));
    CHECK(rb_cell_key(2.5f, 0.2f, 0.f) == rb_cell_key(2.9f, 0.9f, 0.25f));               // a side of 1 px at least
    const float inf = INFINITY, nan = NAN;
    for (float bad : {inf, -inf, nan}) CHECK(rb_cell_key(bad, 1.f, 12.f) == RB_KEY_LAST && rb_cell_key(1.f, bad, 12.f) == RB_KEY_LAST);
    CHECK(rb_cell_key(3e38f, 3e38f, 0.f) < RB_KEY_LAST && rb_cell_key(-3e38f, -3e38f, 0.f) == 0);   // clamped, below the non-finite key
    CHECK(rb_cell_key(1.f, 1.f, 3e38f) < RB_KEY_LAST);
    const uint64_t e = rb_order_entry(RB_KEY_LAST, 4095);
    CHECK(rb_entry_query(e) == 4095 && (e >> 12) == RB_KEY_LAST && rb_order_entry(7, 5) < rb_order_entry(7, 6) && rb_order_entry(7, 4095) < rb_order_entry(8, 0));
}

static void test_layout() {
    for (size_t c : {(size_t)1, (size_t)9, (size_t)1024})
        for (size_t q : {(size_t)0, (size_t)1, (size_t)4097, (size_t)RB_MAX_QUERIES}) {
            const RbLayout l = rb_layout(c, q);
            const size_t parts[] = {l.query, l.xy, l.begin, l.cams, l.up_end, l.cand_query, l.cand_row, l.inlier, l.down_end, l.match, l.total};
            for (size_t i = 0; i + 1 < sizeof(parts) / sizeof(parts[0]); i++) CHECK(parts[i] <= parts[i + 1] && parts[i] % 256 == 0);
            CHECK(l.xy - l.query >= 32 * q && l.begin - l.xy >= 8 * q && l.cams - l.begin >= 4 * (c + 1) && l.up_end - l.cams >= RB_CAMERA_BYTES * c);
            CHECK(l.n_cand == l.up_end && l.cand_query - l.n_cand >= 4 * c && l.cand_row - l.cand_query >= 4 * q && l.inlier - l.cand_row >= 4 * q);
            CHECK(l.down_end - l.inlier >= q && l.order == l.down_end && l.match - l.order >= 4 * q && l.total - l.match >= 32 * q);
            const RbLayout big = rb_layout(2 * c, 2 * q + 1);             // a call's cut fits a block with more room
            CHECK(l.total <= big.total && l.down_end <= big.down_end);
        }
    CHECK(rb_grow(0, 5, 16) == 16 && rb_grow(16, 17, 16) == 32 && rb_grow(16, 100, 16) == 100 && rb_grow(16, 16, 16) == 16 && rb_grow(0, 99, 16) == 99);
}

int main() {
    test_offsets();
    test_plans();
    test_keys();
    test_layout();
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("RELOC BATCH HOST OK\n");
    return 0;
}
