// The C++ facade's batched place candidates (include/svo/visual_odometry.hpp: DescriptorIndex::places_batch, places_from_ids_batch,
// tag_votes_batch) on a real GPU: every camera of every call against the caller's reference (written into the input) and against
// the facade's single calls on the same index — the three counts, the places byte for byte, the recognised landmarks, the votes
// row by row and the three shared arrays; an empty camera among the others; no camera at all; a second call; and refusals that throw.
// argv[1]: int32 {m, n_cameras, row_lo, row_hi, tag_lo, tag_hi, min_votes, separation, max_places}, m descriptors of 32 bytes, m ids
// (uint64), m points (3 floats), m tags (int32); then per camera int32 {n_q, n_landmarks, n_tags_voted, n_places}, n_q query
// descriptors and the n_places expected places (32 bytes each) (tests/test_gpu_place_batch_facade.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "svo/visual_odometry.hpp"

using namespace visual_odometry;
using Descriptor = DescriptorIndex::Descriptor;
using Places = DescriptorIndex::Places;

template <typename T> static bool get(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || (bool)f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)));
}

static bool same(const Places& a, const Places& b) {
    return a.result.n_landmarks == b.result.n_landmarks && a.result.n_tags_voted == b.result.n_tags_voted && a.result.n_places == b.result.n_places &&
           a.places.size() == b.places.size() && (a.places.empty() || memcmp(a.places.data(), b.places.data(), a.places.size() * sizeof(svo_place)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[9];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int m = hdr[0], B = hdr[1];
    std::vector<Descriptor> desc;
    std::vector<float> xyz;
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags;
    if (!get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) || !get(f, tags, (size_t)m)) return 2;
    std::vector<std::vector<Descriptor>> query((size_t)B);
    std::vector<Places> want((size_t)B);
    for (int b = 0; b < B; b++) {
        int h[4];
        if (!f.read((char*)h, sizeof(h)) || !get(f, query[(size_t)b], (size_t)h[0]) || !get(f, want[(size_t)b].places, (size_t)h[3])) return 2;
        want[(size_t)b].result = svo_place_result{h[1], h[2], h[3]};
    }
    try {
        DescriptorIndex index(m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        svo_place_params prm = DescriptorIndex::place_params();
        prm.row_lo = hdr[2]; prm.row_hi = hdr[3]; prm.tag_lo = hdr[4]; prm.tag_hi = hdr[5]; prm.min_votes = hdr[6]; prm.separation = hdr[7]; prm.max_places = hdr[8];
        std::vector<DescriptorIndex::Candidates> cands;
        const std::vector<Places> got = index.places_batch(query, prm, &cands);
        if (got.size() != (size_t)B || cands.size() != (size_t)B) { std::printf("places_batch: %zu cameras\n", got.size()); return 1; }
        std::vector<std::vector<uint64_t>> lists((size_t)B);
        for (int b = 0; b < B; b++) {
            const size_t i = (size_t)b;
            std::printf("camera %d: %zu queries, landmarks %d, tags voted %d, places %d\n", b, query[i].size(), got[i].result.n_landmarks, got[i].result.n_tags_voted,
                        got[i].result.n_places);
            if (!same(got[i], want[i])) { std::printf("camera %d differs from the reference\n", b); return 1; }
            DescriptorIndex::Candidates one;
            if (!same(got[i], index.places(query[i], prm, &one))) { std::printf("camera %d differs from the single call\n", b); return 1; }
            if (cands[i].query != one.query || cands[i].row != one.row) { std::printf("camera %d: the recognised landmarks differ\n", b); return 1; }
            for (int32_t r : one.row) lists[i].push_back(ids[(size_t)r]);
            if (!lists[i].empty()) lists[i].push_back(lists[i][0]);                         // duplicates are legal
        }
        const std::vector<Places> again = index.places_batch(query, prm);
        const std::vector<Places> by_id = index.places_from_ids_batch(lists, prm);
        const DescriptorIndex::TagVotesBatch v = index.tag_votes_batch(lists, {prm.row_lo, prm.row_hi}, {prm.tag_lo, prm.tag_hi});
        if (v.n_bins != (size_t)(prm.tag_hi - prm.tag_lo + 1) || v.votes.size() != (size_t)B * v.n_bins) { std::printf("tag_votes_batch: the sizes\n"); return 1; }
        for (int b = 0; b < B; b++) {
            const size_t i = (size_t)b;
            if (!same(again[i], got[i])) { std::printf("camera %d: the second call differs\n", b); return 1; }
            if (!same(by_id[i], got[i]) || !same(by_id[i], index.places_from_ids(lists[i], prm))) { std::printf("camera %d: places_from_ids_batch differs\n", b); return 1; }
            const DescriptorIndex::TagVotes one = index.tag_votes(lists[i], {prm.row_lo, prm.row_hi}, {prm.tag_lo, prm.tag_hi});
            if (!std::equal(one.votes.begin(), one.votes.end(), v.votes.begin() + (long)(i * v.n_bins)) || one.rows != v.rows || one.row_first != v.row_first ||
                one.row_end != v.row_end) { std::printf("camera %d: tag_votes_batch differs\n", b); return 1; }
        }
        if (!index.places_batch({}, prm).empty() || !index.places_from_ids_batch({}, prm).empty()) { std::printf("no camera, but a result\n"); return 1; }
        // refusals: each throws
        int threw = 0;
        svo_place_params bad = prm;
        bad.min_votes = 0;
        try { index.places_batch(query, bad); } catch (const std::runtime_error&) { threw++; }
        bad = prm; bad.tag_hi = bad.tag_lo - 1;
        try { index.places_from_ids_batch(lists, bad); } catch (const std::runtime_error&) { threw++; }
        try { index.tag_votes_batch(std::vector<std::vector<uint64_t>>(17), {0, -1}, {0, SVO_PLACE_MAX_TAGS - 1}); } catch (const std::runtime_error&) { threw++; }   // 17 x 2^20 bins
        try { index.tag_votes_batch({std::vector<uint64_t>(SVO_PLACE_MAX_IDS + 1, 1)}, {0, -1}, {0, 0}); } catch (const std::runtime_error&) { threw++; }
        try { index.places_from_ids_batch(std::vector<std::vector<uint64_t>>(SVO_PLACE_BATCH_MAX_CAMERAS + 1), prm); } catch (const std::runtime_error&) { threw++; }
        DescriptorIndex plain(16);                     // no points: tags live there
        try { plain.tag_votes_batch(lists); } catch (const std::runtime_error&) { threw++; }
        if (threw != 6) { std::printf("%d of 6 refusals threw\n", threw); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("PLACE BATCH FACADE OK\n");
    return 0;
}
