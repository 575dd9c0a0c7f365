// The C++ facade's track output (include/svo/visual_odometry.hpp: set_track_output, last_track_observations) against the C-ABI on
// the same frames: a VisualOdometry with the output set before its first frame and a one-sequence svo_context give the same rows
// per frame, byte for byte; ids persist from frame to frame; the output off throws, a bad max_rows throws.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], then per frame left, right (tests/test_gpu_track_obs_facade.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
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
    static_assert(sizeof(svo_track_obs) == 64, "svo_track_obs is 64 bytes");
    svo_config cfg; svo_config_default(&cfg); cfg.max_translation_norm = 2.0;
    svo_context* ctx = nullptr;
    const int MAX_ROWS = 4096;
    try {
        VisualOdometry vo(cfg), off(cfg);
        vo.initalize_projection_matricies(Pl, Pr); off.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { vo.set_track_output(0); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("max_rows 0 accepted\n"); return 1; }
        vo.set_track_output(MAX_ROWS);                                // before the first frame: applied when the context is created
        svo_throw(svo_create(&cfg, 0, 1, cols, rows, &ctx));
        svo_throw(svo_set_projection(ctx, -1, Pl.data(), Pr.data()));
        svo_throw(svo_set_track_output(ctx, 1, MAX_ROWS));
        std::set<long long> before;
        int persisted = 0, total = 0;
        for (int k = 0; k < n; k++) {
            const Image L(img[2 * k].data(), rows, cols), R(img[2 * k + 1].data(), rows, cols);
            const auto a = vo.stereo_callback(L, R);
            double T[16]; svo_frame_stats st;
            const int rc = svo_process(ctx, L.data, R.data, L.step, T, &st);
            svo_throw(rc);
            const std::vector<svo_track_obs> obs = vo.last_track_observations();
            std::vector<svo_track_obs> want(MAX_ROWS);
            int n_tracks = -1;
            const int got = svo_get_last_track_obs(ctx, 0, MAX_ROWS, want.data(), &n_tracks);
            svo_throw(got);
            if (a.first != (rc == 1) || memcmp(a.second.data(), T, sizeof(T)) || (int)obs.size() != got || n_tracks != st.n_after_bounds ||
                (got > 0 && memcmp(obs.data(), want.data(), sizeof(svo_track_obs) * (size_t)got))) {
                std::printf("frame %d: facade and C-ABI differ (ok %d / %d, rows %d / %d, tracks %d / %d)\n", k, (int)a.first, rc, (int)obs.size(), got, n_tracks, st.n_after_bounds);
                return 1;
            }
            if (!(svo_get_last_frame_path(vo.handle()) & SVO_PATH_TRACK_IDS)) { std::printf("frame %d: path bit\n", k); return 1; }
            std::set<long long> now;
            for (const svo_track_obs& t : obs) { now.insert((long long)t.id); persisted += before.count((long long)t.id) ? 1 : 0; }
            if (now.size() != obs.size()) { std::printf("frame %d: ids repeat\n", k); return 1; }
            total += (int)obs.size();
            before = now;
        }
        if (total < 100 || persisted < 50) { std::printf("too few rows (%d) or persisting ids (%d)\n", total, persisted); return 1; }
        off.stereo_callback(Image(img[0].data(), rows, cols), Image(img[1].data(), rows, cols));
        threw = false;
        try { off.last_track_observations(); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("output off gave rows\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_destroy(ctx);
        return 1;
    }
    svo_destroy(ctx);
    std::printf("TRACK OBS OK\n");
    return 0;
}
