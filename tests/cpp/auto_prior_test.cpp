// The C++ facade's predicted prior (include/svo/visual_odometry.hpp: set_motion_prior_mode, last_motion_prior) against the C-ABI on the
// three frames of the turning scene: a VisualOdometry in SVO_PRIOR_LAST_ROTATION — the mode set before the first frame, so it is kept
// and applied when the context is created — and a one-sequence svo_context in the default mode that is handed, before frame 2, the
// transposed rotation of the transform frame 1 returned (the host restatement of svo.h).  Both get the ground-truth rotation before
// frame 1.  They return the same transform and statistics, byte for byte; frame 2 keeps its pose; the facade reports source 0, 1, 2
// and, at frame 2, the 18 floats the C-ABI context had pending; an unknown mode throws.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], double R[9], then per frame left, right (tests/test_gpu_auto_prior_facade.py).
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
    double R1[9];
    if (!f.read((char*)Pl.data(), sizeof(float) * 12) || !f.read((char*)Pr.data(), sizeof(float) * 12) || !f.read((char*)R1, sizeof(R1))) return 2;
    if (n != 3) return 2;
    std::vector<std::vector<uint8_t>> img(2 * (size_t)n, std::vector<uint8_t>((size_t)rows * cols));
    for (auto& im : img) if (!f.read((char*)im.data(), (std::streamsize)im.size())) return 2;
    svo_config cfg; svo_config_default(&cfg); cfg.win_w = cfg.win_h = 21;
    svo_context* ctx = nullptr;
    try {
        VisualOdometry vo(cfg);
        vo.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { vo.set_motion_prior_mode(7); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("an unknown mode was accepted\n"); return 1; }
        vo.set_motion_prior_mode(SVO_PRIOR_LAST_ROTATION);                       // before the first frame: kept for the context
        svo_throw(svo_create(&cfg, 0, 1, cols, rows, &ctx));
        svo_throw(svo_set_projection(ctx, -1, Pl.data(), Pr.data()));
        double T[16] = {0}; int rc = 0;
        for (int k = 0; k < n; k++) {
            const Image L(img[2 * k].data(), rows, cols), Rt(img[2 * k + 1].data(), rows, cols);
            float wantH[9] = {0}, wantHi[9] = {0};
            if (k == 1) {
                vo.set_rotation_prior(R1);
                svo_throw(svo_motion_prior_from_rotation(Pl.data(), R1, wantH, wantHi));
                svo_throw(svo_set_motion_prior(ctx, 0, wantH, wantHi));
            }
            if (k == 2 && rc == 1) {                                              // the rule, restated: R = T[:3, :3] transposed
                double R[9];
                for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = T[4 * j + i];
                svo_throw(svo_motion_prior_from_rotation(Pl.data(), R, wantH, wantHi));
                svo_throw(svo_set_motion_prior(ctx, 0, wantH, wantHi));
            }
            const auto a = vo.stereo_callback(L, Rt);
            svo_frame_stats st;
            rc = svo_process(ctx, L.data, Rt.data, L.step, T, &st);
            svo_throw(rc);
            if (a.first != (rc == 1) || std::memcmp(a.second.data(), T, sizeof(T)) || std::memcmp(&vo.stats, &st, sizeof(st))) {
                std::printf("frame %d: facade and C-ABI differ (ok %d / %d, tracks %d / %d)\n", k, (int)a.first, rc, vo.stats.n_after_bounds, st.n_after_bounds);
                return 1;
            }
            const VisualOdometry::MotionPrior p = vo.last_motion_prior();
            if (p.source != k) { std::printf("frame %d: source %d\n", k, p.source); return 1; }
            if (k > 0 && (std::memcmp(p.H.data(), wantH, sizeof(wantH)) || std::memcmp(p.Hi.data(), wantHi, sizeof(wantHi)))) { std::printf("frame %d: the prior's bits differ\n", k); return 1; }
            const int want_path = SVO_PATH_MOTION_PRIOR | SVO_PATH_PRIOR_PREDICTED;
            if ((svo_get_last_frame_path(vo.handle()) & want_path) != want_path) { std::printf("frame %d: path bits\n", k); return 1; }
            if ((svo_get_last_frame_path(ctx) & SVO_PATH_PRIOR_PREDICTED) != 0) { std::printf("frame %d: the plain context predicted\n", k); return 1; }
            if (k >= 1 && (!a.first || vo.stats.fail_reason != 0)) { std::printf("frame %d lost: fail_reason %d\n", k, vo.stats.fail_reason); return 1; }
        }
        int mode = -1;
        svo_throw(svo_get_motion_prior_mode(vo.handle(), &mode));
        if (mode != SVO_PRIOR_LAST_ROTATION) { std::printf("mode %d\n", mode); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_destroy(ctx);
        return 1;
    }
    svo_destroy(ctx);
    std::printf("AUTO PRIOR FACADE OK\n");
    return 0;
}
