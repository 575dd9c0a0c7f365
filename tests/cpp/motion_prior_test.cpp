// The C++ facade's motion prior (include/svo/visual_odometry.hpp: set_rotation_prior, set_motion_prior) against the C-ABI on one
// turning pair: a VisualOdometry and a one-sequence svo_context, both given the rotation before the second frame, return the same
// transform, statistics and tracks, byte for byte; the frame keeps its pose (fail_reason 0) where the same pair without the prior
// loses it (fail_reason 2); the frame reports SVO_PATH_MOTION_PRIOR; a prior before the first frame throws.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], double R[9], then per frame left, right (tests/test_gpu_motion_prior_facade.py).
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
    double R[9];
    if (!f.read((char*)Pl.data(), sizeof(float) * 12) || !f.read((char*)Pr.data(), sizeof(float) * 12) || !f.read((char*)R, sizeof(R))) return 2;
    if (n != 2) return 2;
    std::vector<std::vector<uint8_t>> img(2 * (size_t)n, std::vector<uint8_t>((size_t)rows * cols));
    for (auto& im : img) if (!f.read((char*)im.data(), (std::streamsize)im.size())) return 2;
    svo_config cfg; svo_config_default(&cfg); cfg.win_w = cfg.win_h = 21;
    svo_context* ctx = nullptr;
    try {
        VisualOdometry vo(cfg), plain(cfg);
        vo.initalize_projection_matricies(Pl, Pr); plain.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { vo.set_rotation_prior(R); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("a prior before the first frame was accepted\n"); return 1; }
        svo_throw(svo_create(&cfg, 0, 1, cols, rows, &ctx));
        svo_throw(svo_set_projection(ctx, -1, Pl.data(), Pr.data()));
        for (int k = 0; k < n; k++) {
            const Image L(img[2 * k].data(), rows, cols), Rt(img[2 * k + 1].data(), rows, cols);
            if (k == 1) {
                vo.set_rotation_prior(R);
                float H[9], Hi[9];
                svo_throw(svo_motion_prior_from_rotation(Pl.data(), R, H, Hi));
                svo_throw(svo_set_motion_prior(ctx, 0, H, Hi));
            }
            const auto a = vo.stereo_callback(L, Rt);
            const auto p = plain.stereo_callback(L, Rt);
            double T[16]; svo_frame_stats st;
            const int rc = svo_process(ctx, L.data, Rt.data, L.step, T, &st);
            svo_throw(rc);
            if (a.first != (rc == 1) || std::memcmp(a.second.data(), T, sizeof(T)) || std::memcmp(&vo.stats, &st, sizeof(st))) {
                std::printf("frame %d: facade and C-ABI differ (ok %d / %d, tracks %d / %d)\n", k, (int)a.first, rc, vo.stats.n_after_bounds, st.n_after_bounds);
                return 1;
            }
            const int cap = 1 << 15;
            std::vector<float> ta((size_t)cap * 2), tb((size_t)cap * 2);
            const int na = svo_get_last_tracks(vo.handle(), 0, cap, nullptr, nullptr, ta.data(), nullptr, nullptr, nullptr);
            const int nb = svo_get_last_tracks(ctx, 0, cap, nullptr, nullptr, tb.data(), nullptr, nullptr, nullptr);
            if (na != nb || (na > 0 && std::memcmp(ta.data(), tb.data(), sizeof(float) * 2 * (size_t)na))) { std::printf("frame %d: tracks differ\n", k); return 1; }
            const bool bit = (svo_get_last_frame_path(vo.handle()) & SVO_PATH_MOTION_PRIOR) != 0;
            if (bit != (k == 1) || (svo_get_last_frame_path(plain.handle()) & SVO_PATH_MOTION_PRIOR)) { std::printf("frame %d: path bit\n", k); return 1; }
            if (k == 1) {
                if (!a.first || vo.stats.fail_reason != 0) { std::printf("the prior did not save the frame: fail_reason %d\n", vo.stats.fail_reason); return 1; }
                if (p.first || plain.stats.fail_reason != 2) { std::printf("without the prior the frame was not lost: fail_reason %d\n", plain.stats.fail_reason); return 1; }
                int pending = -1;
                svo_throw(svo_get_motion_prior(vo.handle(), 0, nullptr, nullptr, &pending));
                if (pending != 0) { std::printf("the prior was not consumed\n"); return 1; }
            }
        }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_destroy(ctx);
        return 1;
    }
    svo_destroy(ctx);
    std::printf("MOTION PRIOR FACADE OK\n");
    return 0;
}
