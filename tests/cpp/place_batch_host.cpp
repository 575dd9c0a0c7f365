// place_batch_host.cpp — a stand-alone program over stereo_visual_odometry_amd/csrc/svo_place_batch.hpp, the rules of the batched
// place candidates compiled for the host from the text svo_match_api.hip and the kernels run (tests/test_place_batch_host.py builds
// it with AddressSanitizer and UBSan and runs it): every refusal of a call — the offsets', a slice's, the window's and the product of
// cameras and bins, with 2^24 accepted and 2^24 + 1 refused —; the layouts' sizes at the limits; and, against the vectors of the
// numpy reference in argv[1], the table of (id, camera) pairs — every case's list inserted in order, in reverse and interleaved, with
// a sequential stand-in for the compare-and-swap — with the one sweep over the rows behind it, colliding ids among the cases; and
// rule 3 over a row of votes against the reference's places and against the single call's pick over a key list.
// argv[1]: int32 {n_rows, row_lo, row_hi, tag_lo, tag_hi, n_cases, n_pick}; the rows' ids (uint64) and tags (int32); the expected
// rows, row_first, row_end (tag_hi - tag_lo + 1 int32 each); per case int32 {cameras, total}, the offsets (cameras + 1 int32), the list
// (total uint64), the expected n_landmarks (cameras int32) and votes (cameras x bins int32); then n_pick records as place_host.cpp
// reads them: int32 {n_bins, tag_lo, min_votes, separation, max_places, n_places}, the bins' votes, rows, row_first, row_end and the
// expected places (8 int32 each).
#include "../../stereo_visual_odometry_amd/csrc/svo_place_batch.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static void test_refusals() {
    // the offsets: svo_reloc_batch.hpp's rules, on a place batch's limits
    const int32_t ok[4] = {0, 0, 4096, 4100}, first[2] = {1, 2}, order[3] = {0, 5, 4}, slice[2] = {0, 4097};
    CHECK(rb_check_offsets(3, ok) == RB_OFFSETS_OK && rb_check_offsets(0, nullptr) == RB_OFFSETS_OK);
    CHECK(rb_check_offsets(-1, ok) == RB_OFFSETS_COUNT && rb_check_offsets(PB_MAX_CAMERAS + 1, ok) == RB_OFFSETS_COUNT);
    CHECK(rb_check_offsets(1, nullptr) == RB_OFFSETS_NULL && rb_check_offsets(1, first) == RB_OFFSETS_FIRST);
    CHECK(rb_check_offsets(2, order) == RB_OFFSETS_ORDER && rb_check_offsets(1, slice) == RB_OFFSETS_SLICE);
    std::vector<int32_t> full(PB_MAX_CAMERAS + 1);
    for (int b = 0; b <= PB_MAX_CAMERAS; b++) full[(size_t)b] = b * 1024;                  // 1024 cameras of 1024: 2^20 in all
    CHECK(rb_check_offsets(PB_MAX_CAMERAS, full.data()) == RB_OFFSETS_OK);
    full[PB_MAX_CAMERAS] += 1;
    CHECK(rb_check_offsets(PB_MAX_CAMERAS, full.data()) == RB_OFFSETS_TOTAL);
    // a slice's and the window's own: svo_place.hpp's, as the single calls'
    PlaceRequest q{0, -1, 40, 7, 10, 0, 255, 1, 0, 8};
    CHECK(place_check(q, 1000) == PLACE_OK && q.row_hi == 1000);
    q.tag_hi = PLACE_MAX_TAGS;
    CHECK(place_check_votes(q, 1000) == PLACE_TAG_SPAN);
    // the product of cameras and bins
    CHECK(pb_check_bins(16, 0, PLACE_MAX_TAGS - 1) == PB_OK && pb_check_bins(17, 0, PLACE_MAX_TAGS - 1) == PB_BINS);          // 2^24, and above
    CHECK(pb_check_bins(PB_MAX_CAMERAS, 5, 5 + 16383) == PB_OK && pb_check_bins(PB_MAX_CAMERAS, 5, 5 + 16384) == PB_BINS);
    CHECK(pb_check_bins(673, 0, 24928) == PB_BINS && pb_check_bins(673, 0, 24927) == PB_OK);   // 673 x 24 929 = 2^24 + 1
    CHECK(pb_check_bins(0, 0, PLACE_MAX_TAGS - 1) == PB_OK && pb_check_bins(1, 0, PLACE_MAX_TAGS - 1) == PB_OK);
    CHECK(pb_check_bins(PB_MAX_CAMERAS, 2147483647 - PLACE_MAX_TAGS + 1, 2147483647) == PB_BINS && pb_bins(2147483647, 2147483647) == 1);
}

static void test_layout() {
    CHECK(sizeof(PbCam) == 16);
    const PbLayout a = pb_layout(512, (size_t)1 << 20, 256, 8);                            // include/svo.h, "Memory"
    CHECK(a.places == 8192 && a.bins == a.places + 131072 && a.votes == a.bins + 4096 && a.down_end == a.votes + 524288);
    CHECK(a.list == a.begin + 2304 && a.cam == a.list + ((size_t)8 << 20) && a.table == a.cam + ((size_t)4 << 20));
    CHECK(a.total == ((size_t)20 << 20) + 669952);
    const PbLayout m = pb_layout(16, (size_t)1 << 20, (size_t)1 << 20, 0);                 // the limits of tag_votes_batch: 2^24 bins
    CHECK(m.places == 256 && m.bins == 256 && m.votes == 256 + ((size_t)16 << 20) && m.down_end == m.votes + ((size_t)64 << 20));
    CHECK(m.total == m.down_end + 256 + ((size_t)8 << 20) + ((size_t)4 << 20) + ((size_t)8 << 20));
    const PbLayout w = pb_layout(PB_MAX_CAMERAS, PB_MAX_IDS, 16384, PLACE_MAX_PLACES);      // 1024 cameras x 16 384 bins, 64 places each
    CHECK(w.bins == 16384 + ((size_t)2 << 20) && w.down_end - w.votes == ((size_t)64 << 20) && w.total < ((size_t)100 << 20));
    const PbLayout z = pb_layout(1, 0, 1, 1);
    CHECK(z.total == 256 + 256 + 256 + 256 + 256 + 0 + 0 + 256);
    const PbStage s = pb_stage(a, 512, (size_t)1 << 20, true), v = pb_stage(m, 16, (size_t)1 << 20, false);
    CHECK(s.ids == 2304 && s.up_end == 2304 + ((size_t)8 << 20) && s.total == s.up_end + 8192 + 131072);
    CHECK(a.list - a.begin == s.ids - s.begin);                                            // one copy takes the offsets and the ids up
    CHECK(v.total == v.up_end + m.down_end);
    CHECK(fuse_table_slots(PB_MAX_IDS) == 2u << 20 && fuse_table_slots(0) == 2);
}

template <typename T> static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int test_vectors(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    int32_t hdr[7];
    if (fread(hdr, sizeof(hdr), 1, f) != 1) return 2;
    const int n_rows = hdr[0], row_lo = hdr[1], row_hi = hdr[2], tag_lo = hdr[3], tag_hi = hdr[4], n_cases = hdr[5], n_pick = hdr[6];
    const size_t nb = (size_t)(tag_hi - tag_lo + 1);
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags, want_shared[3];
    if (!get(f, ids, (size_t)n_rows) || !get(f, tags, (size_t)n_rows) || !get(f, want_shared[0], nb) || !get(f, want_shared[1], nb) || !get(f, want_shared[2], nb)) return 2;
    for (int k = 0; k < n_cases; k++) {
        int32_t ch[2];
        if (fread(ch, sizeof(ch), 1, f) != 1) return 2;
        const int C = ch[0], T = ch[1];
        std::vector<int32_t> begin, want_lm, want_votes;
        std::vector<uint64_t> list;
        if (!get(f, begin, (size_t)C + 1) || !get(f, list, (size_t)T) || !get(f, want_lm, (size_t)C) || !get(f, want_votes, (size_t)C * nb)) return 2;
        CHECK(rb_check_offsets(C, begin.data()) == RB_OFFSETS_OK && begin[(size_t)C] == T);
        std::vector<int32_t> cam((size_t)T, PB_CAM_NONE);
        for (int b = 0; b < C; b++) for (int p = begin[(size_t)b]; p < begin[(size_t)b + 1]; p++) cam[(size_t)p] = b;
        const uint32_t slots = fuse_table_slots(T);
        std::vector<int32_t> fwd, rev, mix;
        for (int i = 0; i < T; i++) { fwd.push_back(i); rev.push_back(T - 1 - i); }
        int stride = 7919;                                                                 // a prime that does not divide T: a permutation
        while (T > 0 && T % stride == 0) stride += 2;
        for (int i = 0; i < T; i++) mix.push_back((int32_t)(((int64_t)i * stride) % T));
        if (T > 1 && T % 7919 != 0) { std::vector<char> seen((size_t)T, 0); for (int32_t p : mix) seen[(size_t)p] = 1; for (char s : seen) CHECK(s); }
        for (const std::vector<int32_t>* order : {&fwd, &rev, &mix}) {                     // whatever order the lanes arrive in
            std::vector<int32_t> table(slots, PLACE_EMPTY), fresh((size_t)C, 0);
            for (int32_t pos : *order) {
                const int32_t b = cam[(size_t)pos];
                const PlaceInsert r = pb_insert(table.data(), slots - 1, list.data(), begin[(size_t)b], begin[(size_t)b + 1], pos, PbPlainSlot{});
                CHECK(r != PLACE_SET_FULL);
                fresh[(size_t)b] += r == PLACE_SET_NEW;
            }
            CHECK(fresh == want_lm);
            std::vector<PlaceBin> bins(nb, PlaceBin{0, 0, 0, 0});
            std::vector<int32_t> votes((size_t)C * nb, 0);
            for (int r = row_lo; r < row_hi; r++) {
                if (!place_tag_qualifies(tags[(size_t)r], tag_lo, tag_hi)) continue;
                const size_t bin = (size_t)(tags[(size_t)r] - tag_lo);
                place_bin_add(bins[bin], r, false);
                pb_visit(table.data(), slots - 1, list.data(), ids[(size_t)r], [&](int32_t at) { votes[(size_t)cam[(size_t)at] * nb + bin] += 1; });
            }
            CHECK(votes == want_votes);
            int bad = 0;
            for (size_t b = 0; b < nb; b++)
                bad += bins[b].rows != want_shared[0][b] || place_row_first(bins[b]) != want_shared[1][b] || place_row_end(bins[b]) != want_shared[2][b];
            CHECK(bad == 0);
        }
        printf("case %d: %d cameras, %d entries, %u slots\n", k, C, T, slots);
    }
    for (int c = 0; c < n_pick; c++) {
        int32_t h[6];
        if (fread(h, sizeof(h), 1, f) != 1) return 2;
        std::vector<int32_t> v[4], want_places;
        for (auto& a : v) if (!get(f, a, (size_t)h[0])) return 2;
        if (!get(f, want_places, 8 * (size_t)h[5])) return 2;
        std::vector<PlaceBin> shared((size_t)h[0]), own((size_t)h[0]);
        for (int b = 0; b < h[0]; b++) {
            shared[(size_t)b] = PlaceBin{-12345, v[1][(size_t)b], v[1][(size_t)b] ? place_first_inv(v[2][(size_t)b]) : 0, v[3][(size_t)b]};   // the shared votes field is not read
            own[(size_t)b] = pb_bin(v[0][(size_t)b], shared[(size_t)b]);
        }
        PlaceOut out[PLACE_MAX_PLACES], single[PLACE_MAX_PLACES];
        int32_t voted = -1, want_voted = 0;
        for (int b = 0; b < h[0]; b++) want_voted += v[0][(size_t)b] >= 1;
        const int k = pb_pick(v[0].data(), shared.data(), h[0], h[1], h[2], h[3], h[4], out, &voted);
        CHECK(k == h[5] && voted == want_voted);
        CHECK(k == h[5] && (k == 0 || memcmp(out, want_places.data(), (size_t)k * sizeof(PlaceOut)) == 0));
        std::vector<uint64_t> keys;                                                        // the single call's pick
        for (int b = 0; b < h[0]; b++) if (own[(size_t)b].votes >= h[2] && own[(size_t)b].votes >= 1) keys.push_back(place_key(own[(size_t)b].votes, b));
        const int ks = place_pick(keys.data(), (int32_t)keys.size(), own.data(), h[1], h[3], h[4], single);
        CHECK(ks == k && (k == 0 || memcmp(out, single, (size_t)k * sizeof(PlaceOut)) == 0));
    }
    fclose(f);
    printf("rows %d, bins %zu, cases %d, pick cases %d\n", n_rows, nb, n_cases, n_pick);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    test_refusals();
    test_layout();
    if (const int rc = test_vectors(argv[1]); rc != 0) { printf("cannot read %s\n", argv[1]); return rc; }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("PLACE BATCH HOST OK\n");
    return 0;
}
