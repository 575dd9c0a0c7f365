// fuse_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_fuse.hpp, the rules of the landmark fusion compiled
// for the host from the text svo_match_api.hip and the kernels run (tests/test_fuse_host.py builds it with AddressSanitizer and UBSan
// and runs it): every refusal of a call and the spans where they touch; the scratch's sizes; and, against the vectors of the numpy
// reference in argv[1], the gate, the hash, and the table — insert in list order, in reverse and interleaved, then the sweep of
// rule 5 over a copy of the ids — with the map step in front of it.
// argv[1]: int32 {n_gate, n_hash, n_list, n_ids, row_lo, row_hi, want_changed, slots}; n_gate records of 7 floats (p, q, radius) and 3
// int32 (p's tag, q's tag, expected); n_hash ids (uint64) and their expected first slots (uint32) under mask slots - 1; the from and
// the to list (uint64 each); the ids (uint64) and the ids expected afterwards.
#include "../../stereo_visual_odometry_amd/csrc/svo_fuse.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include <limits>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static FuseRequest good() { return FuseRequest{100, 200, 0, 100, 0, -1, 40, 7, 10, 0.5f}; }
template <typename F> static FuseRefusal with(F change, int size = 1000) {
    FuseRequest q = good();
    change(q);
    return fuse_check(q, size);
}

static void test_refusals() {
    FuseRequest q = good();
    CHECK(fuse_check(q, 1000) == FUSE_OK && q.src_hi == 200 && q.relabel_hi == 1000);
    q = good(); q.src_hi = -1;
    CHECK(fuse_check(q, 300) == FUSE_OK && q.src_hi == 300);
    q = good(); q.dst_hi = -1;                                              // D = [0, size) swallows S
    CHECK(fuse_check(q, 1000) == FUSE_OVERLAP && q.dst_hi == 1000);
    CHECK(with([](FuseRequest& r) { r.src_lo = -1; }) == FUSE_SRC_RANGE && with([](FuseRequest& r) { r.src_hi = 1001; }) == FUSE_SRC_RANGE);
    CHECK(with([](FuseRequest& r) { r.src_lo = 201; }) == FUSE_SRC_RANGE && with([](FuseRequest& r) { r.src_hi = -2; }) == FUSE_SRC_RANGE);
    CHECK(with([](FuseRequest& r) { r.dst_lo = -1; }) == FUSE_DST_RANGE && with([](FuseRequest& r) { r.dst_hi = 1001; }) == FUSE_DST_RANGE);
    CHECK(with([](FuseRequest& r) { r.dst_lo = 101; }) == FUSE_DST_RANGE);
    CHECK(with([](FuseRequest& r) { r.relabel_lo = -1; }) == FUSE_RELABEL_RANGE && with([](FuseRequest& r) { r.relabel_hi = 1001; }) == FUSE_RELABEL_RANGE);
    CHECK(with([](FuseRequest& r) { r.relabel_lo = 5; r.relabel_hi = 4; }) == FUSE_RELABEL_RANGE && with([](FuseRequest& r) { r.relabel_lo = 7; r.relabel_hi = 7; }) == FUSE_OK);
    CHECK(with([](FuseRequest& r) { r.src_lo = 1000; r.src_hi = 1000 + FUSE_MAX_ROWS; }, 10000) == FUSE_OK);
    CHECK(with([](FuseRequest& r) { r.src_lo = 1000; r.src_hi = 1001 + FUSE_MAX_ROWS; }, 10000) == FUSE_ROWS);
    CHECK(with([](FuseRequest& r) { r.src_lo = 0; r.src_hi = std::numeric_limits<int32_t>::max(); }, std::numeric_limits<int32_t>::max()) == FUSE_ROWS);
    CHECK(with([](FuseRequest& r) { r.dst_hi = 101; }) == FUSE_OVERLAP && with([](FuseRequest& r) { r.src_lo = 99; }) == FUSE_OVERLAP);
    CHECK(with([](FuseRequest& r) { r.src_lo = r.src_hi = 50; }) == FUSE_OK);                                  // an empty span shares nothing
    CHECK(with([](FuseRequest& r) { r.radius = -0.5f; }) == FUSE_RADIUS && with([](FuseRequest& r) { r.radius = 0.f; }) == FUSE_OK);
    CHECK(with([](FuseRequest& r) { r.radius = std::numeric_limits<float>::infinity(); }) == FUSE_RADIUS);
    CHECK(with([](FuseRequest& r) { r.radius = std::numeric_limits<float>::quiet_NaN(); }) == FUSE_RADIUS);
    CHECK(with([](FuseRequest& r) { r.max_dist = -1; }) == FUSE_MAX_DIST && with([](FuseRequest& r) { r.max_dist = 257; }) == FUSE_MAX_DIST);
    CHECK(with([](FuseRequest& r) { r.max_dist = 0; }) == FUSE_OK && with([](FuseRequest& r) { r.max_dist = 256; }) == FUSE_OK);
    CHECK(with([](FuseRequest& r) { r.ratio_num = 0; }) == FUSE_RATIO && with([](FuseRequest& r) { r.ratio_den = 0; }) == FUSE_RATIO);
    CHECK(with([](FuseRequest& r) { r.ratio_num = FUSE_MAX_RATIO + 1; }) == FUSE_RATIO && with([](FuseRequest& r) { r.ratio_den = FUSE_MAX_RATIO + 1; }) == FUSE_RATIO);
    CHECK(with([](FuseRequest& r) { r.ratio_num = FUSE_MAX_RATIO; r.ratio_den = 1; }) == FUSE_OK);
    q = good(); q.max_dist = 999; q.relabel_lo = -5;                        // the search's check looks at neither
    CHECK(fuse_check_search(q, 1000) == FUSE_OK);
    CHECK(!fuse_spans_overlap(0, 100, 100, 200) && fuse_spans_overlap(0, 101, 100, 200) && !fuse_spans_overlap(5, 5, 0, 10));
}

static void test_layout() {
    CHECK(sizeof(FuseCtl) == 8256);
    CHECK(fuse_table_slots(0) == 2 && fuse_table_slots(1) == 2 && fuse_table_slots(2) == 4 && fuse_table_slots(3) == 8);
    CHECK(fuse_table_slots(4096) == 8192 && fuse_table_slots(4097) == 16384 && fuse_table_slots(FUSE_MAX_LIST) == (1u << 21));
    const FuseLayout a = fuse_layout(4096), b = fuse_layout(FUSE_MAX_LIST), c = fuse_layout(1);
    CHECK(a.total == 106752 && a.from == 8448 && a.to == 8448 + 32768 && a.table == 8448 + 65536);            // include/svo.h, "Memory"
    CHECK(b.total == 8448 + ((size_t)24 << 20));
    CHECK(c.total == 8448 + 256 + 256 + 256);
}

template <typename T> static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// the table built by inserting the list's positions in `order`, then rule 5 over ids[row_lo .. row_hi) -> the rows changed
static int relabel(const std::vector<uint64_t>& from, const std::vector<uint64_t>& to, const std::vector<int32_t>& order, uint32_t slots,
                   std::vector<uint64_t>& ids, int row_lo, int row_hi) {
    std::vector<int32_t> table(slots, FUSE_EMPTY);
    for (int32_t pos : order) CHECK(fuse_table_insert(table.data(), slots - 1, from.data(), to.data(), pos, FusePlainSlot{}));
    size_t used = 0;
    for (int32_t s : table) used += s != FUSE_EMPTY;
    CHECK(2 * used <= slots);
    const std::vector<uint64_t> before = ids;         // the sweep reads a row's id before it writes it; keys come from `from` alone
    int changed = 0;
    for (int r = row_lo; r < row_hi; r++) {
        const int32_t at = fuse_table_find(table.data(), slots - 1, from.data(), ids[(size_t)r]);
        if (at < 0) continue;
        CHECK(from[(size_t)at] == before[(size_t)r] && fuse_maps(from[(size_t)at], to[(size_t)at]));
        ids[(size_t)r] = to[(size_t)at];
        changed++;
    }
    return changed;
}

static int test_vectors(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    int32_t hdr[8];
    if (fread(hdr, sizeof(hdr), 1, f) != 1) return 2;
    const int n_gate = hdr[0], n_hash = hdr[1], n_list = hdr[2], n_ids = hdr[3], row_lo = hdr[4], row_hi = hdr[5], want_changed = hdr[6];
    const uint32_t slots = (uint32_t)hdr[7];
    CHECK(slots == fuse_table_slots(n_list));
    for (int i = 0; i < n_gate; i++) {
        float v[7];
        int32_t t[3];
        if (fread(v, sizeof(v), 1, f) != 1 || fread(t, sizeof(t), 1, f) != 1) return 2;
        CHECK((int32_t)fuse_admits(v[0], v[1], v[2], t[0], v[3], v[4], v[5], t[1], v[6]) == t[2]);
        CHECK(fuse_admits(v[3], v[4], v[5], t[1], v[0], v[1], v[2], t[0], v[6]) == fuse_admits(v[0], v[1], v[2], t[0], v[3], v[4], v[5], t[1], v[6]));
    }
    std::vector<uint64_t> hash_id, from, to, ids, want;
    std::vector<uint32_t> hash_slot;
    if (!get(f, hash_id, (size_t)n_hash) || !get(f, hash_slot, (size_t)n_hash) || !get(f, from, (size_t)n_list) || !get(f, to, (size_t)n_list) ||
        !get(f, ids, (size_t)n_ids) || !get(f, want, (size_t)n_ids)) return 2;
    fclose(f);
    for (int i = 0; i < n_hash; i++) CHECK(fuse_slot_first(hash_id[(size_t)i], slots - 1) == hash_slot[(size_t)i]);
    CHECK(fuse_slot_next(slots - 1, slots - 1) == 0 && fuse_slot_next(0, slots - 1) == 1);
    std::vector<int32_t> fwd, rev, mix;
    for (int i = 0; i < n_list; i++) { fwd.push_back(i); rev.push_back(n_list - 1 - i); }
    for (int i = 0; i < n_list; i++) mix.push_back((int32_t)(((int64_t)i * 7919) % n_list));       // 7919 is prime and n_list no multiple of it
    for (const std::vector<int32_t>* order : {&fwd, &rev, &mix}) {                                  // whatever order the lanes arrive in
        std::vector<uint64_t> got = ids;
        const int changed = relabel(from, to, *order, slots, got, row_lo, row_hi);
        CHECK(changed == want_changed);
        CHECK(got == want);
    }
    printf("gate %d, hash %d, list %d, ids %d, changed %d\n", n_gate, n_hash, n_list, n_ids, want_changed);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    test_refusals();
    test_layout();
    if (const int rc = test_vectors(argv[1]); rc != 0) { printf("cannot read %s\n", argv[1]); return rc; }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("FUSE HOST OK\n");
    return 0;
}
