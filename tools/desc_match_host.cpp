// The host loop the descriptor index replaces, as a baseline for tools/desc_match_bench.py: the `popcountll` Hamming distance
// INTEGRATION.md gave before the index existed, extended to the index's rule (include/svo.h, "Descriptor index": the best row by
// (distance, row), and the best row whose id differs from the best's), over queries split among threads.
//
//   g++ -O3 -march=native -std=c++17 -pthread tools/desc_match_host.cpp -o tools/desc_match_host
//   tools/desc_match_host check FILE               FILE: int32 {n, m}, n queries, m descriptors (32 bytes each), m ids (uint64),
//                                                  n expected 32-byte result rows (tools/desc_match_bench.py writes it from
//                                                  tests/desc_match_ref.py) -> "HOST MATCH CHECK OK" when every row equals
//   tools/desc_match_host bench N SIZE THREADS REPS  random rows, ids in runs of 4 -> one JSON line with the median milliseconds
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <thread>
#include <vector>

struct Match { uint64_t id, id2; int32_t row, row2; uint16_t dist, dist2; uint32_t reserved; };
static_assert(sizeof(Match) == 32, "the index's result row");

static inline int hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; k += 8) { uint64_t x, y; memcpy(&x, a + k, 8); memcpy(&y, b + k, 8); d += __builtin_popcountll(x ^ y); }
    return d;
}

// queries [q0, q1): rows in order, so at equal distances the first (lower) row stays
static void match_some(const uint8_t* query, int q0, int q1, const uint8_t* desc, const uint64_t* ids, int m, Match* out) {
    for (int q = q0; q < q1; q++) {
        const uint8_t* qd = query + (size_t)q * 32;
        int d1 = 257, d2 = 257, r1 = -1, r2 = -1;
        uint64_t id1 = 0;
        for (int r = 0; r < m; r++) {
            const int d = hamming(qd, desc + (size_t)r * 32);
            if (d < d1) {
                if (ids[r] != id1 && r1 >= 0) { d2 = d1; r2 = r1; }
                d1 = d; r1 = r; id1 = ids[r];
            } else if (ids[r] != id1 && d < d2) { d2 = d; r2 = r; }
        }
        out[q] = Match{id1, r2 >= 0 ? ids[r2] : 0, r1, r2, (uint16_t)d1, (uint16_t)d2, 0};
    }
}

static void match_all(const uint8_t* query, int n, const uint8_t* desc, const uint64_t* ids, int m, Match* out, int threads) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back(match_some, query, (int)((int64_t)n * t / threads), (int)((int64_t)n * (t + 1) / threads), desc, ids, m, out);
    for (auto& t : pool) t.join();
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "check")) {
        std::ifstream f(argv[2], std::ios::binary);
        int hdr[2];
        if (!f.read((char*)hdr, sizeof(hdr))) return 2;
        const int n = hdr[0], m = hdr[1];
        std::vector<uint8_t> query((size_t)n * 32), desc((size_t)m * 32);
        std::vector<uint64_t> ids((size_t)m);
        std::vector<Match> want((size_t)n), got((size_t)n);
        if (!f.read((char*)query.data(), (std::streamsize)query.size()) || !f.read((char*)desc.data(), (std::streamsize)desc.size()) ||
            !f.read((char*)ids.data(), (std::streamsize)m * 8) || !f.read((char*)want.data(), (std::streamsize)n * 32)) return 2;
        match_all(query.data(), n, desc.data(), ids.data(), m, got.data(), 3);
        for (int q = 0; q < n; q++)
            if (memcmp(&got[q], &want[q], sizeof(Match))) { std::printf("query %d differs from the reference\n", q); return 1; }
        std::printf("HOST MATCH CHECK OK (%d queries, %d rows)\n", n, m);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "bench")) {
        const int n = atoi(argv[2]), m = atoi(argv[3]), threads = atoi(argv[4]), reps = atoi(argv[5]);
        if (n < 1 || m < 1 || threads < 1 || threads > 16 || reps < 1) return 2;
        std::vector<uint8_t> query((size_t)n * 32), desc((size_t)m * 32);
        std::vector<uint64_t> ids((size_t)m);
        uint64_t s = 0x9E3779B97F4A7C15ull;
        auto next = [&s]() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint8_t)((s * 0x2545F4914F6CDD1Dull) >> 56); };
        for (auto& b : query) b = next();
        for (auto& b : desc) b = next();
        for (int r = 0; r < m; r++) ids[(size_t)r] = 7 + (uint64_t)r / 4;
        std::vector<Match> out((size_t)n);
        std::vector<double> ms;
        for (int k = 0; k < reps + 1; k++) {                          // the first call warms the caches and is dropped
            const auto t0 = std::chrono::steady_clock::now();
            match_all(query.data(), n, desc.data(), ids.data(), m, out.data(), threads);
            if (k) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        uint64_t sum = 0;
        for (const auto& r : out) sum += (uint64_t)r.row + r.dist;
        std::printf("{\"n\": %d, \"size\": %d, \"threads\": %d, \"reps\": %d, \"median_ms\": %.3f, \"min_ms\": %.3f, \"checksum\": %llu}\n", n, m, threads, reps,
                    ms[ms.size() / 2], ms[0], (unsigned long long)sum);
        return 0;
    }
    std::fprintf(stderr, "usage: desc_match_host check FILE | bench N SIZE THREADS REPS\n");
    return 2;
}
