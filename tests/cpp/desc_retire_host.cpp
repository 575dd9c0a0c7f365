// desc_retire_host.cpp — stereo_visual_odometry_amd/csrc/svo_retire.hpp compiled for the host: the text the index-maintenance kernels
// and svo_match_api.hip run.  Built with -fsanitize=address,undefined by tests/test_desc_retire_host.py.
//  - alive1 on both sides of every clause, and the sorted list's search at its ends, in its gaps and on an empty list;
//  - the table's size, the hash's range, and a serial model of the insert (the kernel's loop with the atomics as plain statements)
//    in a small table whose probes wrap around at the last slot: per id the largest alive row, whatever the order of the rows;
//  - the transform's arithmetic against long double where long double is exact (64-bit significands: products of an f64 and an f32
//    widened, and sums of two such values of similar size, fit), and the finite test on the edge values;
//  - the scratch layout: parts in order, aligned, sized as include/svo.h states.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../stereo_visual_odometry_amd/csrc/svo_retire.hpp"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static uint64_t rng_state = 0x1234567ull;
static uint64_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return rng_state >> 11; }

// the kernel's insert, serially: CAS on an empty slot, max on a slot of the same id, else the next slot; false: the probe ran out
static bool insert(std::vector<int32_t>& table, const std::vector<uint64_t>& ids, int32_t row) {
    const uint32_t mask = (uint32_t)table.size() - 1;
    uint32_t slot = retire_slot_first(ids[(size_t)row], mask);
    for (uint32_t step = 0; step <= mask; step++, slot = retire_slot_next(slot, mask)) {
        const int32_t old = table[slot];
        if (old == RETIRE_EMPTY) { table[slot] = row; return true; }
        if (ids[(size_t)old] == ids[(size_t)row]) { table[slot] = std::max(old, row); return true; }
    }
    return false;
}
// the kernel's lookup: the row the id's slot holds, -1 where the probe meets an empty slot or runs out
static int32_t lookup(const std::vector<int32_t>& table, const std::vector<uint64_t>& ids, uint64_t id) {
    const uint32_t mask = (uint32_t)table.size() - 1;
    uint32_t slot = retire_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = retire_slot_next(slot, mask)) {
        const int32_t at = table[slot];
        if (at == RETIRE_EMPTY) return -1;
        if (ids[(size_t)at] == id) return at;
    }
    return -1;
}

static void test_predicate() {
    CHECK(retire_alive1(0, -1, 5, 2, true));                            // no flag: everything lives
    CHECK(!retire_alive1(RETIRE_SCOPE, 0, 0, 0, false));
    CHECK(!retire_alive1(RETIRE_SCOPE | RETIRE_BY_TAG, 3, 0, 9, false));
    for (int32_t tag = -2; tag <= 8; tag++) CHECK(retire_alive1(RETIRE_BY_TAG, tag, 2, 5, true) == (tag >= 2 && tag <= 5));
    CHECK(!retire_alive1(RETIRE_BY_TAG, 3, 5, 2, false));               // an empty window
    CHECK(retire_alive1(RETIRE_BY_TAG, -1, -1, 3, false));              // a row without a point is inside a window that holds -1
    CHECK(retire_alive1(RETIRE_BY_TAG, INT32_MIN, INT32_MIN, INT32_MAX, false) && retire_alive1(RETIRE_BY_TAG, INT32_MAX, INT32_MIN, INT32_MAX, false));
    CHECK(!retire_alive1(RETIRE_BY_IDS, 0, 0, 0, true) && retire_alive1(RETIRE_BY_IDS, 0, 0, 0, false));
    CHECK(retire_alive1(RETIRE_LATEST_PER_ID, 0, 0, 0, true));          // latest is not part of alive1
    CHECK(!retire_alive1(RETIRE_BY_TAG | RETIRE_BY_IDS, 3, 2, 5, true) && !retire_alive1(RETIRE_BY_TAG | RETIRE_BY_IDS, 6, 2, 5, false) &&
          retire_alive1(RETIRE_BY_TAG | RETIRE_BY_IDS, 5, 2, 5, false));
    for (int32_t tag = -2; tag <= 8; tag++) CHECK(retire_tag_selected(tag, -5, 5) == (tag != -1 && tag <= 5));
}

static void test_list() {
    CHECK(!retire_id_listed(nullptr, 0, 7));
    const uint64_t one[1] = {7};
    CHECK(retire_id_listed(one, 1, 7) && !retire_id_listed(one, 1, 6) && !retire_id_listed(one, 1, 8));
    std::vector<uint64_t> v = {0, 3, 4, 1000, 1ull << 40, UINT64_MAX - 1, UINT64_MAX};
    for (uint64_t id : v) CHECK(retire_id_listed(v.data(), (int32_t)v.size(), id));
    const uint64_t absent[] = {1, 2, 5, 999, 1001, (1ull << 40) + 1, UINT64_MAX - 2};
    for (uint64_t id : absent) CHECK(!retire_id_listed(v.data(), (int32_t)v.size(), id));
    CHECK(!retire_id_listed(v.data() + 1, (int32_t)v.size() - 2, 0) && !retire_id_listed(v.data() + 1, (int32_t)v.size() - 2, UINT64_MAX));
    std::vector<uint64_t> big;
    for (int i = 0; i < 1000; i++) big.push_back(rnd() | 1);           // odd values
    std::sort(big.begin(), big.end());
    big.erase(std::unique(big.begin(), big.end()), big.end());
    for (uint64_t id : big) CHECK(retire_id_listed(big.data(), (int32_t)big.size(), id) && !retire_id_listed(big.data(), (int32_t)big.size(), id + 1));
}

static void test_table() {
    CHECK(retire_table_slots(0) == 2 && retire_table_slots(1) == 2 && retire_table_slots(2) == 4 && retire_table_slots(3) == 8);
    CHECK(retire_table_slots(4) == 8 && retire_table_slots(5) == 16 && retire_table_slots(4000) == 8192 && retire_table_slots(1 << 24) == (1u << 25));
    for (int i = 0; i < 2000; i++) {
        const uint64_t id = i < 2 ? (i ? UINT64_MAX : 0) : rnd() * (rnd() | 1);
        for (uint32_t mask : {1u, 7u, 8191u, (1u << 25) - 1}) CHECK(retire_slot_first(id, mask) <= mask);
    }
    CHECK(retire_slot_next(7, 7) == 0 && retire_slot_next(6, 7) == 7 && retire_slot_next(0, 1) == 1 && retire_slot_next(1, 1) == 0);
    // 8 slots, 4 ids chosen to start at the last slot: the probes wrap, and every id still ends at its largest row
    std::vector<uint64_t> at_last;
    for (uint64_t id = 0; at_last.size() < 4; id++) if (retire_slot_first(id, 7) == 7) at_last.push_back(id);
    std::vector<uint64_t> ids;
    for (int rep = 0; rep < 3; rep++) for (uint64_t id : at_last) ids.push_back(id);        // 12 rows, 4 ids, 3 rows each
    for (int order = 0; order < 50; order++) {
        std::vector<int32_t> rows(ids.size());
        for (size_t i = 0; i < rows.size(); i++) rows[i] = (int32_t)i;
        for (size_t i = rows.size() - 1; i > 0; i--) std::swap(rows[i], rows[(size_t)(rnd() % (i + 1))]);   // the order the lanes arrive in
        std::vector<int32_t> table(8, RETIRE_EMPTY);
        for (int32_t r : rows) CHECK(insert(table, ids, r));
        CHECK(table[7] != RETIRE_EMPTY && table[0] != RETIRE_EMPTY && table[1] != RETIRE_EMPTY && table[2] != RETIRE_EMPTY && table[3] == RETIRE_EMPTY);
        for (size_t k = 0; k < at_last.size(); k++) CHECK(lookup(table, ids, at_last[k]) == (int32_t)(8 + k));
    }
    // a full table: the probe of one more id runs out after `slots` steps instead of spinning
    {
        std::vector<uint64_t> many;
        for (uint64_t id = 100; many.size() < 9; id++) many.push_back(id);
        std::vector<int32_t> table(8, RETIRE_EMPTY);
        for (int32_t r = 0; r < 8; r++) CHECK(insert(table, many, r));
        CHECK(!insert(table, many, 8) && lookup(table, many, many[8]) == -1);
    }
    // design load: 2000 ids in 4000 rows in the table retire gives 4000 rows, ids 0 and 2^64 - 1 among them
    {
        std::vector<uint64_t> two(4000);
        for (int i = 0; i < 2000; i++) two[(size_t)i] = two[(size_t)(3999 - i)] = i == 0 ? 0 : i == 1 ? UINT64_MAX : rnd() * 2654435761ull + (uint64_t)i;
        std::vector<int32_t> table(retire_table_slots(4000), RETIRE_EMPTY);
        for (int32_t r = 3999; r >= 0; r--) CHECK(insert(table, two, r));
        int kept = 0;
        for (int32_t r = 0; r < 4000; r++) kept += lookup(table, two, two[(size_t)r]) == r;
        CHECK(kept == 2000);
        for (int32_t r = 2000; r < 4000; r++) CHECK(lookup(table, two, two[(size_t)r]) == r);
    }
}

static void test_transform() {
    // exact in long double: entries of T and coordinates with few significant bits, so that each product and each sum fits 64 bits
    for (int i = 0; i < 5000; i++) {
        double T[16];
        for (double& t : T) t = (double)((int64_t)(rnd() % 2000001) - 1000000) / 1024.0;
        const float p[3] = {(float)((int)(rnd() % 20001) - 10000) / 16.f, (float)((int)(rnd() % 20001) - 10000) / 16.f, (float)((int)(rnd() % 20001) - 10000) / 16.f};
        for (int c = 0; c < 3; c++) {
            const long double v = (long double)T[4 * c] * p[0] + (long double)T[4 * c + 1] * p[1] + (long double)T[4 * c + 2] * p[2] + (long double)T[4 * c + 3];
            CHECK(retire_map_coord(T, c, p[0], p[1], p[2]) == (float)(double)v);     // v is exact and fits an f64: one rounding, to f32
        }
    }
    // one operation at a time: 1 + 2^-53 * 1 rounds to 1 in f64 before 2^-53 more arrives (a fused or wider sum would see 2^-52)
    {
        double T[16] = {1, 0x1p-53, 0x1p-53, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
        CHECK(retire_map_coord(T, 0, 1.f, 1.f, 1.f) == 0.f);
        const long double wide = ((long double)1 + (long double)0x1p-53) + (long double)0x1p-53 - 1;
        CHECK(sizeof(long double) <= 8 || wide != 0);
    }
    // the identity changes no bit of a value that is not -0 (the rule's sums turn -0 into +0)
    {
        double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const float vals[5] = {1.5f, -3.25e-30f, 3.4e38f, 1e-45f, 0.f};
        for (float a : vals) for (int c = 0; c < 3; c++) {
            const float out = retire_map_coord(I, c, c == 0 ? a : 2.f, c == 1 ? a : 2.f, c == 2 ? a : 2.f);
            CHECK(memcmp(&out, &a, 4) == 0);
        }
    }
    // overflow and the finite test
    {
        double S[16] = {1e38, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const float over = retire_map_coord(S, 0, 4.f, 0.f, 0.f), fits = retire_map_coord(S, 0, 3.f, 0.f, 0.f);
        uint32_t b;
        memcpy(&b, &over, 4); CHECK(isinf(over) && !retire_finite_bits(b));
        memcpy(&b, &fits, 4); CHECK(isfinite(fits) && retire_finite_bits(b));
        const float bad = retire_map_coord(S, 1, 0.f, INFINITY, 0.f) - INFINITY;
        memcpy(&b, &bad, 4); CHECK(!retire_finite_bits(b));
        CHECK(retire_finite_bits(0x7F7FFFFFu) && retire_finite_bits(0xFF7FFFFFu) && !retire_finite_bits(0x7F800000u) && !retire_finite_bits(0xFF800000u) &&
              !retire_finite_bits(0x7FC00000u) && retire_finite_bits(0) && retire_finite_bits(0x80000000u) && retire_finite_bits(1));
    }
}

static void test_layout() {
    const uint32_t all = RETIRE_ALL_FLAGS;
    for (int m : {1, 63, 255, 256, 257, 4000, 300000, 1 << 24}) {
        for (int slab : {64, RETIRE_DEFAULT_SLAB}) {
            const int moving = m + 100 < (1 << 24) ? m + 100 : m, n_ids = 77;
            const RetireLayout l = retire_layout(m, moving, n_ids, slab, all);
            CHECK(l.keep == 0 && l.rank >= (size_t)m && l.counts - l.rank >= 4 * ((size_t)m + 1));
            CHECK(l.table - l.counts >= 4 * (((size_t)m + 255) / 256 + 257));
            CHECK(l.ids - l.table >= 4 * (size_t)retire_table_slots(m) && l.bounce - l.ids >= 8 * (size_t)n_ids);
            CHECK(l.total - l.bounce >= (size_t)RETIRE_ROW_BYTES * (size_t)std::min(slab, moving));
            for (size_t off : {l.rank, l.counts, l.table, l.ids, l.bounce, l.total}) CHECK(off % 256 == 0);
            const size_t R = 255, stated = ((size_t)m + R) / 256 * 256 + (4 * ((size_t)m + 1) + R) / 256 * 256 + (4 * (((size_t)m + 255) / 256 + 257) + R) / 256 * 256 +
                                          (4 * (size_t)retire_table_slots(m) + R) / 256 * 256 + (8 * (size_t)n_ids + R) / 256 * 256 +
                                          (56 * (size_t)std::min(slab, moving) + R) / 256 * 256;
            CHECK(l.total == stated);
            const RetireLayout bare = retire_layout(m, moving, n_ids, slab, RETIRE_BY_TAG);
            CHECK(bare.ids == bare.table && bare.bounce == bare.ids && bare.total < l.total);
        }
    }
}

int main() {
    test_predicate();
    test_list();
    test_table();
    test_transform();
    test_layout();
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("DESC RETIRE HOST OK\n");
    return 0;
}
