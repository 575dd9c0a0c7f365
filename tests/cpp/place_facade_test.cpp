// The C++ facade's place candidates (include/svo/visual_odometry.hpp: DescriptorIndex::place_params, places, places_from_ids,
// tag_votes) on a real GPU, against the caller's reference (written into the input): the three counts, the places byte for byte and
// the recognised landmarks of places; tag_votes' four arrays; places_from_ids with the same landmarks by id; the same call twice; and
// refusals that throw.
// argv[1]: int32 {m, n_q, row_lo, row_hi, tag_lo, tag_hi, min_votes, separation, max_places, n_landmarks, n_tags_voted, n_places},
// m descriptors of 32 bytes, m ids (uint64), m points (3 floats), m tags (int32), n_q query descriptors, the n_places expected places
// (32 bytes each), the expected cand_query and cand_row (n_landmarks int32 each), and the expected votes, rows, row_first, row_end of
// the recognised landmarks' ids (tag_hi - tag_lo + 1 int32 each) (tests/test_gpu_place_facade.py).
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

static bool same(const DescriptorIndex::Places& p, const int* hdr, const std::vector<svo_place>& want) {
    return p.result.n_landmarks == hdr[9] && p.result.n_tags_voted == hdr[10] && p.result.n_places == hdr[11] && p.places.size() == want.size() &&
           (want.empty() || memcmp(p.places.data(), want.data(), want.size() * sizeof(svo_place)) == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[12];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int m = hdr[0], n_q = hdr[1];
    const size_t nb = (size_t)(hdr[5] - hdr[4] + 1);
    std::vector<Descriptor> desc, query;
    std::vector<float> xyz;
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags, want_query, want_row, want_votes[4];
    std::vector<svo_place> want_places;
    if (!get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) || !get(f, tags, (size_t)m) || !get(f, query, (size_t)n_q) ||
        !get(f, want_places, (size_t)hdr[11]) || !get(f, want_query, (size_t)hdr[9]) || !get(f, want_row, (size_t)hdr[9])) return 2;
    for (auto& v : want_votes) if (!get(f, v, nb)) return 2;
    try {
        DescriptorIndex index(m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        svo_place_params prm = DescriptorIndex::place_params();
        if (prm.max_dist != 40 || prm.ratio_num != 7 || prm.ratio_den != 10 || prm.tag_lo != 0 || prm.tag_hi != SVO_PLACE_MAX_TAGS - 1 || prm.min_votes != 1 ||
            prm.separation != 0 || prm.max_places != 8 || prm.row_lo != 0 || prm.row_hi != -1) { std::printf("the defaults differ from svo.h\n"); return 1; }
        prm.row_lo = hdr[2]; prm.row_hi = hdr[3]; prm.tag_lo = hdr[4]; prm.tag_hi = hdr[5]; prm.min_votes = hdr[6]; prm.separation = hdr[7]; prm.max_places = hdr[8];
        DescriptorIndex::Candidates cand;
        const DescriptorIndex::Places p = index.places(query, prm, &cand);
        std::printf("landmarks %d, tags voted %d, places %d\n", p.result.n_landmarks, p.result.n_tags_voted, p.result.n_places);
        if (!same(p, hdr, want_places)) { std::printf("places differs from the reference\n"); return 1; }
        if (cand.query != want_query || cand.row != want_row) { std::printf("the recognised landmarks differ from the reference\n"); return 1; }
        if (!same(index.places(query, prm), hdr, want_places)) { std::printf("the second call differs\n"); return 1; }
        std::vector<uint64_t> m_ids;
        for (int32_t r : cand.row) m_ids.push_back(ids[(size_t)r]);
        m_ids.insert(m_ids.end(), m_ids.begin(), m_ids.begin() + (std::ptrdiff_t)(m_ids.size() / 2));              // duplicates are legal
        if (m_ids.size() <= (size_t)SVO_PLACE_MAX_IDS && !same(index.places_from_ids(m_ids, prm), hdr, want_places)) { std::printf("places_from_ids differs from places\n"); return 1; }
        const DescriptorIndex::TagVotes v = index.tag_votes(m_ids, {prm.row_lo, prm.row_hi}, {prm.tag_lo, prm.tag_hi});
        if (v.votes != want_votes[0] || v.rows != want_votes[1] || v.row_first != want_votes[2] || v.row_end != want_votes[3]) { std::printf("tag_votes differs from the reference\n"); return 1; }
        if (!index.places({}, prm).places.empty() || !index.places_from_ids({}, prm).places.empty()) { std::printf("no query, but a place\n"); return 1; }
        // refusals: each throws
        int threw = 0;
        svo_place_params bad = prm;
        bad.min_votes = 0;
        try { index.places(query, bad); } catch (const std::runtime_error&) { threw++; }
        bad = prm; bad.tag_hi = bad.tag_lo - 1;
        try { index.places_from_ids(m_ids, bad); } catch (const std::runtime_error&) { threw++; }
        try { index.tag_votes(m_ids, {0, -1}, {0, SVO_PLACE_MAX_TAGS}); } catch (const std::runtime_error&) { threw++; }
        try { index.tag_votes(std::vector<uint64_t>(SVO_PLACE_MAX_IDS + 1, 1), {0, -1}, {0, 0}); } catch (const std::runtime_error&) { threw++; }
        DescriptorIndex plain(16);                     // no points: tags live there
        try { plain.tag_votes(m_ids); } catch (const std::runtime_error&) { threw++; }
        if (threw != 5) { std::printf("%d of 5 refusals threw\n", threw); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("PLACE FACADE OK\n");
    return 0;
}
