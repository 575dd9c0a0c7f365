// The C++ facade's batched relocalisation (include/svo/visual_odometry.hpp: DescriptorIndex::localize_batch, batch_order) against
// the facade's single calls on the same index: per camera the result record byte for byte and the candidate lists, guided and
// unguided; the first camera's candidates are the caller's reference (written into the input); the order is a permutation of every
// slice; a camera with 4097 queries throws and leaves the cameras as they were.
// argv[1]: int32 {B, m, k}, m descriptors of 32 bytes, m ids (uint64), m points (3 floats), m tags (int32), then per camera int32 n,
// float K[9], double R[9], double t[3], float radius, n queries of 32 bytes, n pixels (2 floats); then k expected queries and k
// expected rows of camera 0, guided (tests/test_gpu_reloc_batch_facade.py).
#include <algorithm>
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[3];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int B = hdr[0], m = hdr[1], k = hdr[2];
    std::vector<Descriptor> desc;
    std::vector<float> xyz;
    std::vector<uint64_t> ids;
    std::vector<int32_t> tags, want_q, want_r;
    if (!get(f, desc, (size_t)m) || !get(f, ids, (size_t)m) || !get(f, xyz, 3 * (size_t)m) || !get(f, tags, (size_t)m)) return 2;
    std::vector<DescriptorIndex::BatchCamera> cams((size_t)B);
    for (auto& c : cams) {
        int n;
        double R[9], t[3];
        float radius;
        if (!f.read((char*)&n, sizeof(n)) || !f.read((char*)c.K, sizeof(c.K)) || !f.read((char*)R, sizeof(R)) || !f.read((char*)t, sizeof(t)) ||
            !f.read((char*)&radius, sizeof(radius)) || !get(f, c.query, (size_t)n) || !get(f, c.xy, 2 * (size_t)n)) return 2;
        c.guide = DescriptorIndex::guide(R, t, radius);
        memset(&c.result, 0, sizeof(c.result));
        memcpy(c.result.R, R, sizeof(R)); memcpy(c.result.t, t, sizeof(t));
    }
    if (!get(f, want_q, (size_t)k) || !get(f, want_r, (size_t)k)) return 2;
    try {
        DescriptorIndex index(m);
        index.enable_points();
        index.add_points(desc, ids, xyz, tags);
        const svo_reloc_params prm = DescriptorIndex::default_params();
        for (const bool guided : {true, false}) {
            std::vector<DescriptorIndex::BatchCamera> got = cams;
            index.localize_batch(got.data(), got.size(), guided, prm);
            int located = 0;
            for (size_t b = 0; b < cams.size(); b++) {
                DescriptorIndex::Candidates cand;
                const svo_reloc_result one = guided ? index.localize_guided(cams[b].K, cams[b].guide, cams[b].query, cams[b].xy, prm, cams[b].result, &cand)
                                                    : index.localize(cams[b].K, cams[b].query, cams[b].xy, prm, cams[b].result, &cand);
                if (memcmp(&one, &got[b].result, sizeof(one))) { std::printf("camera %zu (guided %d): the result differs from the single call\n", b, (int)guided); return 1; }
                if (cand.query != got[b].candidates.query || cand.row != got[b].candidates.row || cand.inlier != got[b].candidates.inlier) {
                    std::printf("camera %zu (guided %d): the candidate lists\n", b, (int)guided); return 1;
                }
                located += one.success;
            }
            if (guided && (got[0].candidates.query != want_q || got[0].candidates.row != want_r)) { std::printf("camera 0: %zu candidates, %d expected\n", got[0].candidates.query.size(), k); return 1; }
            if (guided && located < 2) { std::printf("fewer than two cameras were located\n"); return 1; }
            std::vector<int32_t> order = index.batch_order();
            size_t lo = 0;
            for (const auto& c : cams) {                                  // a permutation of every slice
                std::sort(order.begin() + (long)lo, order.begin() + (long)(lo + c.query.size()));
                for (size_t j = 0; j < c.query.size(); j++) if (order[lo + j] != (int32_t)(lo + j)) { std::printf("the order is no permutation\n"); return 1; }
                lo += c.query.size();
            }
            if (order.size() != lo) { std::printf("the order's length\n"); return 1; }
        }
        std::vector<DescriptorIndex::BatchCamera> bad = cams;
        bad[0].query.resize(4097); bad[0].xy.resize(2 * 4097);
        bad[0].result.n_candidates = 77;
        bool threw = false;
        try { index.localize_batch(bad.data(), bad.size(), true, prm); } catch (const std::runtime_error&) { threw = true; }
        if (!threw || bad[0].result.n_candidates != 77 || !bad[0].candidates.query.empty()) { std::printf("4097 queries were accepted\n"); return 1; }
        index.localize_batch(nullptr, 0, true, prm);                      // no cameras: legal
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("RELOC BATCH FACADE OK\n");
    return 0;
}
