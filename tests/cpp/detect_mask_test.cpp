// The C++ facade's detection mask (include/svo/visual_odometry.hpp: set_detection_mask, clear_detection_mask, the masked
// featureDetectionFast) against the C-ABI on the same frames: a VisualOdometry with the mask set before its first frame and a
// one-sequence svo_context with svo_set_detection_mask give the same poses, statistics and feature sets, bit for bit; every feature
// the masked detector returns lies on a non-zero mask byte; after clear_detection_mask the path bit goes away one call later.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], then per frame left, right; then the mask (tests/test_gpu_detect_mask_facade.py).
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
    Mat34f Pl, Pr;
    if (!f.read((char*)Pl.data(), sizeof(float) * 12) || !f.read((char*)Pr.data(), sizeof(float) * 12)) return 2;
    std::vector<std::vector<uint8_t>> img(2 * (size_t)n, std::vector<uint8_t>((size_t)rows * cols));
    for (auto& im : img) if (!f.read((char*)im.data(), (std::streamsize)im.size())) return 2;
    std::vector<uint8_t> mask((size_t)rows * cols);
    if (!f.read((char*)mask.data(), (std::streamsize)mask.size())) return 2;
    svo_config cfg; svo_config_default(&cfg); cfg.max_translation_norm = 2.0;
    svo_context* ctx = nullptr;
    try {
        VisualOdometry vo(cfg);
        vo.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { vo.set_detection_mask(mask.data(), cols); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a mask without a size accepted before the first frame\n"); return 1; }
        // rows further apart than they are long, before the first frame: the object keeps a packed copy
        std::vector<uint8_t> wide((size_t)rows * (cols + 5), 0);
        for (int y = 0; y < rows; y++) memcpy(wide.data() + (size_t)y * (cols + 5), mask.data() + (size_t)y * cols, (size_t)cols);
        vo.set_detection_mask(wide.data(), cols + 5, cols, rows);
        svo_throw(svo_create(&cfg, 0, 1, cols, rows, &ctx));
        svo_throw(svo_set_projection(ctx, -1, Pl.data(), Pr.data()));
        svo_throw(svo_set_detection_mask(ctx, -1, mask.data(), cols, 0));
        const int clear_at = n - 2;                                   // call clear_at still scans a masked image, the next does not
        for (int k = 0; k < n; k++) {
            if (k == clear_at) { vo.clear_detection_mask(); svo_throw(svo_set_detection_mask(ctx, -1, nullptr, 0, 0)); }
            const Image L(img[2 * k].data(), rows, cols), R(img[2 * k + 1].data(), rows, cols);
            const auto a = vo.stereo_callback(L, R);
            double T[16]; svo_frame_stats st;
            const int rc = svo_process(ctx, L.data, R.data, L.step, T, &st);
            svo_throw(rc);
            if (a.first != (rc == 1) || memcmp(a.second.data(), T, sizeof(T)) || memcmp(&vo.stats, &st, sizeof(st))) {
                std::printf("frame %d: facade and C-ABI differ (ok %d / %d)\n", k, (int)a.first, rc);
                return 1;
            }
            const bool want = k >= 1 && k <= clear_at;
            for (svo_context* c : {vo.handle(), ctx})
                if (((svo_get_last_frame_path(c) & SVO_PATH_DETECT_MASKED) != 0) != want) { std::printf("frame %d: path bit\n", k); return 1; }
            std::vector<float> xy(2 * 32768);
            const int nf = svo_get_features(ctx, 0, 32768, xy.data(), nullptr, nullptr);
            std::vector<float> fxy(2 * 32768);
            if (nf < 0 || svo_get_features(vo.handle(), 0, 32768, fxy.data(), nullptr, nullptr) != nf || memcmp(xy.data(), fxy.data(), sizeof(float) * 2 * nf)) {
                std::printf("frame %d: feature sets differ\n", k);
                return 1;
            }
        }
        if (!vo.stats.n_inliers) { std::printf("last frame has no pose\n"); return 1; }
        const Image I(img[0].data(), rows, cols), M(mask.data(), rows, cols);
        std::vector<float> resp, resp_all;
        const std::vector<Point2f> kept = featureDetectionFast(I, M, 20, resp), all = featureDetectionFast(I, 20, resp_all);
        if (kept.empty() || kept.size() >= all.size() || resp.size() != kept.size()) { std::printf("masked detector: %zu of %zu\n", kept.size(), all.size()); return 1; }
        for (const Point2f& p : kept)
            if (!mask[(size_t)p.y * cols + (size_t)p.x]) { std::printf("a keypoint on a masked-out pixel\n"); return 1; }
        threw = false;
        try { featureDetectionFast(I, Image(mask.data(), rows - 1, cols), 20, resp); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a mask of another size accepted\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_destroy(ctx);
        return 1;
    }
    svo_destroy(ctx);
    std::printf("DETECT MASK OK\n");
    return 0;
}
