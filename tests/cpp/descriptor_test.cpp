// The C++ facade's descriptor output (include/svo/visual_odometry.hpp: set_descriptor_output, last_track_descriptors) against the
// C-ABI on the same frames: a VisualOdometry with both outputs set before its first frame and a one-sequence svo_context give the same
// descriptor rows per frame, byte for byte, one per observation row; the rows equal svo_describe_points at the rows' l1 on the frame's
// left image; descriptors without the track output, and the getter on a frame that ran without them, throw.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], then per frame left, right (tests/test_gpu_track_descriptors.py).
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
    const int MAX_ROWS = 4096;
    try {
        VisualOdometry vo(cfg), plain(cfg);
        vo.initalize_projection_matricies(Pl, Pr); plain.initalize_projection_matricies(Pl, Pr);
        bool threw = false;
        try { vo.set_descriptor_output(true); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("descriptors accepted without the track output\n"); return 1; }
        vo.set_track_output(MAX_ROWS); vo.set_descriptor_output(true);   // before the first frame: applied when the context is created
        plain.set_track_output(MAX_ROWS);
        svo_throw(svo_create(&cfg, 0, 1, cols, rows, &ctx));
        svo_throw(svo_set_projection(ctx, -1, Pl.data(), Pr.data()));
        if (svo_set_descriptor_output(ctx, 1) != SVO_ERR_STATE) { std::printf("C-ABI: descriptors accepted without the track output\n"); return 1; }
        svo_throw(svo_set_track_output(ctx, 1, MAX_ROWS));
        svo_throw(svo_set_descriptor_output(ctx, 1));
        int total = 0;
        for (int k = 0; k < n; k++) {
            const Image L(img[2 * k].data(), rows, cols), R(img[2 * k + 1].data(), rows, cols);
            vo.stereo_callback(L, R);
            double T[16]; svo_frame_stats st;
            svo_throw(svo_process(ctx, L.data, R.data, L.step, T, &st));
            const auto obs = vo.last_track_observations();
            const auto desc = vo.last_track_descriptors();
            std::vector<uint8_t> want((size_t)MAX_ROWS * SVO_DESC_BYTES);
            int n_tracks = -1;
            const int got = svo_get_last_track_descriptors(ctx, 0, MAX_ROWS, want.data(), &n_tracks);
            svo_throw(got);
            if (desc.size() != obs.size() || (int)desc.size() != got || n_tracks != st.n_after_bounds ||
                (got > 0 && memcmp(desc[0].data(), want.data(), (size_t)SVO_DESC_BYTES * (size_t)got))) {
                std::printf("frame %d: facade and C-ABI differ (rows %d / %d / %d, tracks %d / %d)\n", k, (int)desc.size(), (int)obs.size(), got, n_tracks, st.n_after_bounds);
                return 1;
            }
            if (!(svo_get_last_frame_path(vo.handle()) & SVO_PATH_DESCRIPTORS)) { std::printf("frame %d: path bit\n", k); return 1; }
            if (got > 0) {                                            // the stage call at the rows' own points gives the rows
                std::vector<float> xy(2 * (size_t)got);
                for (int i = 0; i < got; i++) { xy[2 * i] = obs[i].l1[0]; xy[2 * i + 1] = obs[i].l1[1]; }
                std::vector<uint8_t> stage((size_t)got * SVO_DESC_BYTES);
                svo_throw(svo_describe_points(0, L.data, cols, rows, L.step, got, xy.data(), stage.data(), nullptr));
                if (memcmp(stage.data(), want.data(), stage.size())) { std::printf("frame %d: the stage call and the frame's rows differ\n", k); return 1; }
            }
            total += got;
        }
        if (total < 100) { std::printf("too few rows (%d)\n", total); return 1; }
        plain.stereo_callback(Image(img[0].data(), rows, cols), Image(img[1].data(), rows, cols));
        if (svo_get_last_frame_path(plain.handle()) & SVO_PATH_DESCRIPTORS) { std::printf("path bit without descriptors\n"); return 1; }
        threw = false;
        try { plain.last_track_descriptors(); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("descriptors off gave rows\n"); return 1; }
        int8_t pat[1024]; int32_t cs[60];
        svo_throw(svo_descriptor_pattern(pat, cs));
        if (cs[0] != 16384 || cs[30] != 0 || cs[37] != cs[38]) { std::printf("tables\n"); return 1; }
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        svo_destroy(ctx);
        return 1;
    }
    svo_destroy(ctx);
    std::printf("DESCRIPTORS OK\n");
    return 0;
}
