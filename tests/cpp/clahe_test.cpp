// The C++ facade with CLAHE (include/svo/visual_odometry.hpp, set_clahe): a VisualOdometry with set_clahe(3.0, 6, 4) fed the frames
// gives the poses and counters of a plain one fed the equalised frames, bit for bit; clear_clahe returns it to the plain launches.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], then per frame left, right, left equalised, right equalised
// (tests/test_gpu_clahe_facade.py; the equalised frames come from tests/clahe_ref.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <vector>
#include "svo/visual_odometry.hpp"

using namespace visual_odometry;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[3];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int n = hdr[0], rows = hdr[1], cols = hdr[2];
    const size_t px = (size_t)rows * cols;
    Mat34f Pl, Pr;
    if (!f.read((char*)Pl.data(), sizeof(float) * 12) || !f.read((char*)Pr.data(), sizeof(float) * 12)) return 2;
    std::vector<std::vector<uint8_t>> img(4 * (size_t)n);
    for (auto& i : img) {
        i.resize(px);
        if (!f.read((char*)i.data(), (std::streamsize)px)) return 2;
    }
    svo_config cfg; svo_config_default(&cfg); cfg.max_translation_norm = 2.0;
    try {
        VisualOdometry plain(cfg), eq(cfg);
        plain.initalize_projection_matricies(Pl, Pr); eq.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { eq.set_clahe(2.0, 17, 8); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("17 tiles accepted\n"); return 1; }
        threw = false;
        try { eq.set_clahe(std::numeric_limits<double>::quiet_NaN()); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a NaN clip limit accepted\n"); return 1; }
        eq.set_clahe(3.0, 6, 4);                                      // before the first frame: applied when the context is created
        int poses = 0;
        for (int k = 0; k < n; k++) {
            const bool last = k == n - 1;                             // the last frame runs with CLAHE cleared, on the equalised frame
            if (last) eq.clear_clahe();
            const auto a = plain.stereo_callback(Image(img[4 * k + 2].data(), rows, cols), Image(img[4 * k + 3].data(), rows, cols));
            const auto b = eq.stereo_callback(Image(img[4 * k + (last ? 2 : 0)].data(), rows, cols), Image(img[4 * k + (last ? 3 : 1)].data(), rows, cols));
            if (a.first != b.first || memcmp(a.second.data(), b.second.data(), sizeof(double) * 16) || memcmp(&plain.stats, &eq.stats, sizeof(svo_frame_stats))) {
                std::printf("frame %d differs: ok %d vs %d, inliers %d vs %d\n", k, (int)a.first, (int)b.first, plain.stats.n_inliers, eq.stats.n_inliers);
                return 1;
            }
            if (!!(svo_get_last_frame_path(eq.handle()) & SVO_PATH_CLAHE) == last || (svo_get_last_frame_path(plain.handle()) & SVO_PATH_CLAHE)) {
                std::printf("frame %d: path bits\n", k);
                return 1;
            }
            poses += a.first;
        }
        if (poses < 1) { std::printf("no pose\n"); return 1; }
        threw = false;
        try { eq.set_clahe(2.0, 0, 8); } catch (const std::runtime_error&) { threw = true; }   // with a context: the library's own check
        if (!threw) { std::printf("0 tiles accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("CLAHE FACADE OK\n");
    return 0;
}
