// The C++ facade's pose covariance (include/svo/visual_odometry.hpp: set_pose_covariance, last_pose_covariance) against the C-ABI
// on the same frames: a VisualOdometry with the mode set before its first frame and a one-sequence svo_context give the same 72
// numbers and flag per frame, bit for bit; the mode off throws, a bad mode throws.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], then per frame left, right (tests/test_gpu_pose_cov_facade.py).
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
    svo_config cfg; svo_config_default(&cfg); cfg.max_translation_norm = 2.0;
    svo_context* ctx = nullptr;
    try {
        VisualOdometry vo(cfg), off(cfg);
        vo.initalize_projection_matricies(Pl, Pr); off.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { vo.set_pose_covariance(7); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("bad mode accepted\n"); return 1; }
        threw = false;
        try { vo.set_pose_covariance(SVO_COV_FIXED_SIGMA, 0.0); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("zero sigma accepted\n"); return 1; }
        vo.set_pose_covariance(SVO_COV_FIXED_SIGMA, 0.75);            // before the first frame: applied when the context is created
        svo_throw(svo_create(&cfg, 0, 1, cols, rows, &ctx));
        svo_throw(svo_set_projection(ctx, -1, Pl.data(), Pr.data()));
        svo_throw(svo_set_pose_covariance(ctx, SVO_COV_FIXED_SIGMA, 0.75));
        int valid_frames = 0;
        for (int k = 0; k < n; k++) {
            const Image L(img[2 * k].data(), rows, cols), R(img[2 * k + 1].data(), rows, cols);
            const auto a = vo.stereo_callback(L, R);
            double T[16]; svo_frame_stats st;
            const int rc = svo_process(ctx, L.data, R.data, L.step, T, &st);
            svo_throw(rc);
            const VisualOdometry::PoseCovariance c = vo.last_pose_covariance();
            double cov_T[36], cov_p[36]; int valid = -1;
            svo_throw(svo_get_last_pose_covariance(ctx, cov_T, cov_p, &valid));
            if (a.first != (rc == 1) || memcmp(a.second.data(), T, sizeof(T)) || c.valid != (valid == 1) || c.valid != a.first ||
                memcmp(c.cov_T.data(), cov_T, sizeof(cov_T)) || memcmp(c.cov_p.data(), cov_p, sizeof(cov_p))) {
                std::printf("frame %d: facade and C-ABI differ (ok %d / %d, valid %d / %d)\n", k, (int)a.first, rc, (int)c.valid, valid);
                return 1;
            }
            if (c.valid && !(c.cov_T[0] > 0 && c.cov_T[35] > 0 && c.cov_p[0] > 0)) { std::printf("frame %d: non-positive variances\n", k); return 1; }
            if (!(svo_get_last_frame_path(vo.handle()) & SVO_PATH_POSE_COV)) { std::printf("frame %d: path bit\n", k); return 1; }
            valid_frames += c.valid;
        }
        if (valid_frames < 1) { std::printf("no valid covariance\n"); return 1; }
        off.stereo_callback(Image(img[0].data(), rows, cols), Image(img[1].data(), rows, cols));
        threw = false;
        try { off.last_pose_covariance(); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("mode off gave a covariance\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_destroy(ctx);
        return 1;
    }
    svo_destroy(ctx);
    std::printf("POSE COV OK\n");
    return 0;
}
