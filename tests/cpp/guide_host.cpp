// A stand-alone host program over stereo_visual_odometry_amd/csrc/svo_guide.hpp — the text k_guide_project, k_desc_match_guided and
// the index's host code run — built with AddressSanitizer and UBSan by tests/test_guide_host.py and compared byte for byte with
// tables tests/guide_ref.py wrote.
// argv[1]: a sequence of tables until the end of the file, each
//   int32 {1, m}: a projection table — float K[9], double R[9], double t[3], m points {float x, y, z; int32 tag}, m x 2 floats expected;
//   int32 {2, m}: a gate table — int32 k, float radius, m x 2 floats uv, k x 2 floats xy, k x m bytes expected (query-major).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "../../stereo_visual_odometry_amd/csrc/svo_guide.hpp"

struct Point { float x, y, z; int32_t tag; };
static_assert(sizeof(Point) == 16, "a point row is 16 bytes");

template <typename T> static bool get(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || (bool)f.read((char*)v.data(), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int tables = 0;
    long points = 0, invisible = 0, gates = 0, admitted = 0;
    int32_t hdr[2];
    while (f.read((char*)hdr, sizeof(hdr))) {
        const int m = hdr[1];
        if (m < 0 || m > (1 << 20)) return 2;
        if (hdr[0] == 1) {
            std::vector<float> K, want; std::vector<double> R, t; std::vector<Point> p;
            if (!get(f, K, 9) || !get(f, R, 9) || !get(f, t, 3) || !get(f, p, (size_t)m) || !get(f, want, 2 * (size_t)m)) return 2;
            const GuidePose g = guide_pose(R.data(), t.data(), K.data());
            for (int i = 0; i < m; i++) {
                float uv[2];
                const bool vis = guide_project(g, p[(size_t)i].x, p[(size_t)i].y, p[(size_t)i].z, p[(size_t)i].tag, uv[0], uv[1]);
                if (memcmp(uv, &want[2 * (size_t)i], sizeof(uv))) { std::printf("FAILED: table %d, point %d: (%a, %a) against (%a, %a)\n", tables, i, uv[0], uv[1], want[2 * (size_t)i], want[2 * (size_t)i + 1]); return 1; }
                if (vis != (uv[0] - uv[0] == 0.f)) { std::printf("FAILED: table %d, point %d: the visibility flag\n", tables, i); return 1; }
                points++; invisible += !vis;
            }
        } else if (hdr[0] == 2) {
            int32_t k; float radius;
            if (!f.read((char*)&k, sizeof(k)) || !f.read((char*)&radius, sizeof(radius)) || k < 0 || k > (1 << 20)) return 2;
            std::vector<float> uv, xy; std::vector<uint8_t> want;
            if (!get(f, uv, 2 * (size_t)m) || !get(f, xy, 2 * (size_t)k) || !get(f, want, (size_t)k * (size_t)m)) return 2;
            for (int j = 0; j < k; j++)
                for (int i = 0; i < m; i++) {
                    const bool a = guide_admits(uv[2 * (size_t)i], uv[2 * (size_t)i + 1], xy[2 * (size_t)j], xy[2 * (size_t)j + 1], radius);
                    if (a != (want[(size_t)j * (size_t)m + (size_t)i] != 0)) { std::printf("FAILED: table %d, query %d, row %d: the gate\n", tables, j, i); return 1; }
                    gates++; admitted += a;
                }
        } else {
            return 2;
        }
        tables++;
    }
    if (tables < 1 || points < 1 || invisible < 1 || invisible == points || admitted < 1 || admitted == gates) {
        std::printf("FAILED: %d tables, %ld points (%ld invisible), %ld gates (%ld admitted)\n", tables, points, invisible, gates, admitted);
        return 1;
    }
    std::printf("GUIDE HOST OK (%d tables, %ld points, %ld gates)\n", tables, points, gates);
    return 0;
}
