// The C++ facade with an input encoding (include/svo/visual_odometry.hpp, set_input_encoding): a VisualOdometry fed bgra8 frames
// gives the poses and counters of one fed the grey frames, bit for bit, and rejects frames whose channel count is not the
// encoding's.  argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], then per frame left grey, right grey, left bgra, right bgra (tests/test_gpu_input_format.py).
#include <cstdio>
#include <cstring>
#include <fstream>
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
    for (size_t i = 0; i < img.size(); i++) {
        img[i].resize(px * (i % 4 < 2 ? 1 : 4));
        if (!f.read((char*)img[i].data(), (std::streamsize)img[i].size())) return 2;
    }
    svo_config cfg; svo_config_default(&cfg); cfg.max_translation_norm = 2.0;
    try {
        VisualOdometry grey(cfg), colour(cfg);
        grey.initalize_projection_matricies(Pl, Pr); colour.initalize_projection_matricies(Pl, Pr);
        colour.set_input_encoding("bgra8");                           // before the first frame: applied when the context is created
        bool threw = false;
        try { colour.set_input_encoding("bayer_rggb8"); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("unknown encoding accepted\n"); return 1; }
        int poses = 0;
        for (int k = 0; k < n; k++) {
            const auto a = grey.stereo_callback(Image(img[4 * k].data(), rows, cols), Image(img[4 * k + 1].data(), rows, cols));
            const auto b = colour.stereo_callback(Image(img[4 * k + 2].data(), rows, cols, 0, 4), Image(img[4 * k + 3].data(), rows, cols, 0, 4));
            if (a.first != b.first || memcmp(a.second.data(), b.second.data(), sizeof(double) * 16) || memcmp(&grey.stats, &colour.stats, sizeof(svo_frame_stats))) {
                std::printf("frame %d differs: ok %d vs %d, inliers %d vs %d\n", k, (int)a.first, (int)b.first, grey.stats.n_inliers, colour.stats.n_inliers);
                return 1;
            }
            if (!(svo_get_last_frame_path(colour.handle()) & SVO_PATH_INPUT_CONVERTED) || (svo_get_last_frame_path(grey.handle()) & SVO_PATH_INPUT_CONVERTED)) {
                std::printf("frame %d: path bits\n", k);
                return 1;
            }
            poses += a.first;
        }
        if (poses < 1) { std::printf("no pose\n"); return 1; }
        threw = false;
        try { colour.stereo_callback(Image(img[0].data(), rows, cols), Image(img[1].data(), rows, cols)); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a mono8 frame was accepted as bgra8\n"); return 1; }
        threw = false;
        try { colour.stereo_callback(Image(img[2].data(), rows, cols, 0, 3), Image(img[3].data(), rows, cols, 0, 3)); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a 3-channel frame was accepted as bgra8\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    std::printf("INPUT FORMAT OK\n");
    return 0;
}
