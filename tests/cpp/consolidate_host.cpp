// consolidate_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_consolidate.hpp, the rules of the landmark
// consolidation compiled for the host from the text svo_match_api.hip and the kernels run (tests/test_consolidate_host.py builds it
// with AddressSanitizer and UBSan and runs it): every refusal of a call; the members' rule, the views' cap, the order of two views;
// the scratch layout's sizes; and, against the vectors of the numpy reference in argv[1], the medoid, the gated mean point and the
// far views of planted groups.
// argv[1]: int32 n_groups; per group int32 {n, want_medoid, want_far}, the radius (float), n rows (int32, ascending), n descriptors
// of 8 uint32, n points of 3 floats, and the 3 floats expected.
#include "../../stereo_visual_odometry_amd/csrc/svo_consolidate.hpp"
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static ConsRefusal check(int lo, int hi, float radius, int size = 1000, int* hi_out = nullptr) {
    ConsRequest q{lo, hi, 0, 5, radius};
    const ConsRefusal e = cons_check(q, size);
    if (hi_out) *hi_out = q.row_hi;
    return e;
}

static void test_refusals() {
    int hi = 0;
    CHECK(check(0, -1, 0.5f, 1000, &hi) == CONS_OK && hi == 1000);
    CHECK(check(0, 0, 0.f, 0) == CONS_OK && check(1000, -1, 0.f) == CONS_OK && check(40, 40, 0.f) == CONS_OK && check(0, 1000, 0.f) == CONS_OK);
    CHECK(check(-1, 5, 0.5f) == CONS_RANGE && check(5, 3, 0.5f) == CONS_RANGE && check(0, 1001, 0.5f) == CONS_RANGE);
    CHECK(check(1001, -1, 0.5f) == CONS_RANGE && check(0, -2, 0.5f) == CONS_RANGE);
    CHECK(check(0, -1, -0.5f) == CONS_RADIUS && check(0, -1, -1e-30f) == CONS_RADIUS);
    CHECK(check(0, -1, std::numeric_limits<float>::infinity()) == CONS_RADIUS && check(0, -1, -std::numeric_limits<float>::infinity()) == CONS_RADIUS);
    CHECK(check(0, -1, std::numeric_limits<float>::quiet_NaN()) == CONS_RADIUS);
    CHECK(check(5, 3, -1.f) == CONS_RANGE);                                 // the range is looked at first
}

static void test_rules() {
    CHECK(!cons_member(-1, 0, 5) && !cons_member(-1, -1, 5) && cons_member(0, 0, 5) && cons_member(5, 0, 5) && !cons_member(6, 0, 5));
    CHECK(!cons_member(3, 5, 2) && cons_member(std::numeric_limits<int32_t>::max(), 0, std::numeric_limits<int32_t>::max()));
    CHECK(cons_views(1) == 1 && cons_views(63) == 63 && cons_views(64) == 64 && cons_views(65) == 64 && cons_views(1 << 24) == 64);
    CHECK(cons_better(3, 10, 4, 99) && !cons_better(4, 99, 3, 10) && cons_better(3, 11, 3, 10) && !cons_better(3, 10, 3, 11) && !cons_better(3, 10, 3, 10));
    uint32_t a[8], b[8];
    for (int w = 0; w < 8; w++) { a[w] = 0; b[w] = 0xFFFFFFFFu; }
    CHECK(cons_hamming(a, a) == 0 && cons_hamming(a, b) == 256);
    b[7] = 0x80000001u;
    CHECK(cons_hamming(a, b) == 226 && cons_hamming(b, a) == 226);
    CHECK(cons_near(1.f, 2.f, 3.f, 1.5f, 2.f, 2.5f, 0.5f) && !cons_near(1.f, 2.f, 3.f, 1.5f, 2.f, 2.4375f, 0.5f) && cons_near(1.f, 2.f, 3.f, 1.f, 2.f, 3.f, 0.f));
    CHECK(cons_mean(3.0, 2) == 1.5f && cons_mean(5.0, 3) == (float)(5.0 / 3.0));
    // the order of the sum binds: 4, 2^-22, 2^-51, 2^-51 ascending gives 1, descending 1 + 2^-23 (tests/test_consolidate_ref.py)
    const float v[4] = {4.f, 0x1p-22f, 0x1p-51f, 0x1p-51f};
    double up = 0.0, down = 0.0;
    for (int j = 0; j < 4; j++) { up = up + (double)v[j]; down = down + (double)v[3 - j]; }
    CHECK(cons_mean(up, 4) == 1.f && cons_mean(down, 4) == 1.f + 0x1p-23f);
}

static void test_layout() {
    const ConsLayout a = cons_layout(1, 1, 64);
    CHECK(a.keep == 0 && a.rank == 256 && a.counts == 512 && a.table == 512 + 1280 && a.count == a.table + 256 && a.list == a.count + 256);
    CHECK(a.bounce == a.list + 256 && a.total == a.bounce + 256);
    const int m = 70000;
    const ConsLayout l = cons_layout(m, 80000, 1 << 18);
    const size_t slots = 262144, R = 256;
    CHECK(retire_table_slots(m) == slots);
    CHECK(l.rank == (m + R - 1) / R * R && l.counts - l.rank == (4 * (size_t)(m + 1) + R - 1) / R * R);
    CHECK(l.table - l.counts == (4 * (size_t)(274 + 257) + R - 1) / R * R && l.count - l.table == 4 * slots && l.list - l.count == 4 * slots);
    CHECK(l.bounce - l.list == (4 * (size_t)m + R - 1) / R * R && l.total - l.bounce == 56 * (size_t)80000);
    CHECK(cons_layout(m, 80000, 64).total - cons_layout(m, 80000, 64).bounce == 56 * 64);
    // retire's parts lie where retire's layout puts them: the ranks and the block counts serve both
    const RetireLayout r = retire_layout(m, 80000, 0, 1 << 18, RETIRE_LATEST_PER_ID);
    CHECK(r.keep == l.keep && r.rank == l.rank && r.counts == l.counts && r.table == l.table);
    const ConsLayout big = cons_layout(RETIRE_MAX_ROWS, RETIRE_MAX_ROWS, RETIRE_DEFAULT_SLAB);
    CHECK(big.total > big.bounce && big.count - big.table == 4 * (size_t)(1u << 25));
}

template <typename T> static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int test_vectors(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    int32_t n_groups = 0;
    if (fread(&n_groups, 4, 1, f) != 1) { fclose(f); return 2; }
    int singles = 0, capped = 0, ties = 0;
    for (int g = 0; g < n_groups; g++) {
        int32_t hdr[3];
        float radius;
        std::vector<int32_t> rows;
        std::vector<uint32_t> desc;
        std::vector<float> xyz, want;
        if (fread(hdr, 4, 3, f) != 3 || fread(&radius, 4, 1, f) != 1 || !get(f, rows, (size_t)hdr[0]) || !get(f, desc, 8 * (size_t)hdr[0]) ||
            !get(f, xyz, 3 * (size_t)hdr[0]) || !get(f, want, 3)) { fclose(f); return 2; }
        float got[3];
        int32_t far = -1;
        const int32_t m = cons_group_plain(hdr[0], rows.data(), desc.data(), xyz.data(), radius, got, &far);
        CHECK(m == hdr[1] && far == hdr[2] && memcmp(got, want.data(), 12) == 0);
        singles += hdr[0] == 1; capped += hdr[0] == CONS_MAX_VIEWS; ties += m == hdr[0] - 1;
    }
    fclose(f);
    CHECK(n_groups >= 20 && singles >= 1 && capped >= 1 && ties >= 1);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    test_refusals();
    test_rules();
    test_layout();
    if (const int rc = test_vectors(argv[1]); rc != 0) return rc;
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("CONSOLIDATE HOST OK\n");
    return 0;
}
