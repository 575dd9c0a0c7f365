// The C++ facade's settings before the first frame (include/svo/visual_odometry.hpp; DESIGN.md, "Facades: settings before the
// first frame").  Held equals live: a VisualOdometry given every setting it can hold before its first frame gives, frame by frame
// and bit for bit, what a raw C-ABI context gives that got the same setters after svo_create.  All or nothing: a held setting the
// new context refuses leaves the object before its first frame with everything still held.
// argv[1]: int32 {n, rows, cols}, float Pl[12], Pr[12], double D[5], then per frame left, right as interleaved BGR
// (tests/test_gpu_facade_deferred.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "svo/visual_odometry.hpp"

using namespace visual_odometry;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)
#define C_OK(call) CHECK((call) >= 0, "%s: %s", #call, svo_last_error())

template <class F>
static bool throws(F f) {
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[3];
    if (!f.read((char*)hdr, sizeof(hdr))) return 2;
    const int n = hdr[0], rows = hdr[1], cols = hdr[2];
    const size_t bytes = (size_t)rows * cols * 3;
    Mat34f Pl, Pr;
    double D[5];
    if (!f.read((char*)Pl.data(), sizeof(float) * 12) || !f.read((char*)Pr.data(), sizeof(float) * 12) || !f.read((char*)D, sizeof(D))) return 2;
    std::vector<std::vector<uint8_t>> img(2 * (size_t)n);
    for (auto& i : img) {
        i.resize(bytes);
        if (!f.read((char*)i.data(), (std::streamsize)bytes)) return 2;
    }
    auto frame = [&](int k, int cam) { return Image(img[2 * (size_t)k + cam].data(), rows, cols, 0, 3); };
    // a mild lens on both cameras: K = Pl[:, :3], R = identity, P = the projection matrices
    svo_camera_info info[2] = {};
    for (int cam = 0; cam < 2; cam++) {
        const Mat34f& P = cam ? Pr : Pl;
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { info[cam].K[3 * i + j] = Pl[4 * i + j]; info[cam].R[3 * i + j] = i == j; }
        for (int i = 0; i < 12; i++) info[cam].P[i] = P[i];
        for (int i = 0; i < 5; i++) info[cam].D[i] = D[i];
        info[cam].n_d = 5; info[cam].width = cols; info[cam].height = rows;
    }
    std::vector<uint8_t> mask((size_t)rows * cols, 1);
    for (int y = rows / 4; y < rows / 2; y++) for (int x = cols / 8; x < cols / 2; x++) mask[(size_t)y * cols + x] = 0;
    svo_config cfg; svo_config_default(&cfg); cfg.max_translation_norm = 2.0;
    svo_context* live = nullptr;
    try {
        // ---- held equals live
        VisualOdometry held(cfg);
        CHECK(throws([&] { const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; held.set_motion_prior(eye); }), "set_motion_prior before the first frame accepted");
        CHECK(throws([&] { held.set_detection_mask(mask.data(), 0); }), "set_detection_mask without a size before the first frame accepted");
        held.set_rectification(info[0], info[1]);
        held.initalize_projection_matricies(Pl, Pr);
        held.set_input_encoding("bgr8");
        held.set_pose_covariance(SVO_COV_FIXED_SIGMA, 0.75);
        held.set_detection_mask(mask.data(), 0, cols, rows);
        held.set_clahe(3.0, 6, 4);
        held.set_track_output(64);
        held.set_descriptor_output(true);
        held.set_motion_prior_mode(SVO_PRIOR_LAST_ROTATION);
        CHECK(!held.handle(), "a context before the first frame");
        C_OK(svo_create(&cfg, default_device(), 1, cols, rows, &live));
        C_OK(svo_set_rectification(live, -1, &info[0], &info[1]));
        C_OK(svo_set_projection(live, -1, Pl.data(), Pr.data()));
        C_OK(svo_set_input_format(live, SVO_INPUT_BGR8));
        C_OK(svo_set_pose_covariance(live, SVO_COV_FIXED_SIGMA, 0.75));
        C_OK(svo_set_detection_mask(live, -1, mask.data(), cols, 0));
        C_OK(svo_set_clahe(live, 1, 3.0, 6, 4));
        C_OK(svo_set_track_output(live, 1, 64));
        C_OK(svo_set_descriptor_output(live, 1));
        C_OK(svo_set_motion_prior_mode(live, SVO_PRIOR_LAST_ROTATION));
        const int always = SVO_PATH_INPUT_CONVERTED | SVO_PATH_POSE_COV | SVO_PATH_CLAHE | SVO_PATH_TRACK_IDS | SVO_PATH_DESCRIPTORS;
        int poses = 0, predicted = 0;
        for (int k = 0; k < n; k++) {
            const auto a = held.stereo_callback(frame(k, 0), frame(k, 1));
            Mat44 T; svo_frame_stats st;
            const int rc = svo_process(live, frame(k, 0).data, frame(k, 1).data, cols * 3, T.data(), &st);
            C_OK(rc);
            CHECK(a.first == (rc == 1) && !memcmp(a.second.data(), T.data(), sizeof(double) * 16), "frame %d: the transforms differ", k);
            CHECK(!memcmp(&held.stats, &st, sizeof(st)), "frame %d: the counters differ", k);
            const int path = svo_get_last_frame_path(live);
            CHECK(svo_get_last_frame_path(held.handle()) == path, "frame %d: paths %#x vs %#x", k, svo_get_last_frame_path(held.handle()), path);
            CHECK((path & always) == always && (k < 1 || (path & SVO_PATH_DETECT_MASKED)), "frame %d: path %#x lacks a setting's bit", k, path);
            std::vector<svo_track_obs> obs(64);
            std::vector<DescriptorIndex::Descriptor> desc(64);
            const int n_obs = svo_get_last_track_obs(live, 0, 64, obs.data(), nullptr), n_desc = svo_get_last_track_descriptors(live, 0, 64, desc[0].data(), nullptr);
            C_OK(n_obs); C_OK(n_desc);
            const auto held_obs = held.last_track_observations();
            const auto held_desc = held.last_track_descriptors();
            CHECK((int)held_obs.size() == n_obs && (int)held_desc.size() == n_desc && n_obs == n_desc, "frame %d: row counts", k);
            CHECK(!n_obs || (!memcmp(held_obs.data(), obs.data(), sizeof(svo_track_obs) * n_obs) && !memcmp(held_desc.data(), desc.data(), sizeof(desc[0]) * n_desc)),
                  "frame %d: the rows differ", k);
            std::printf("frame %d: ok %d path %#x inliers %d rows %d\n", k, rc, path, st.n_inliers, n_obs);
            poses += rc == 1 && st.n_inliers > 0;
            predicted += k >= 2 && (path & SVO_PATH_PRIOR_PREDICTED);
        }
        CHECK(poses >= 1 && predicted >= 1, "no pose (%d) or no predicted prior (%d): the comparison shows too little", poses, predicted);

        // ---- all or nothing: more rows than the context's feature capacity pass the facade's check and are refused at creation
        VisualOdometry vo(cfg);
        vo.initalize_projection_matricies(Pl, Pr);
        vo.set_input_encoding("bgr8");
        vo.set_detection_mask(mask.data(), 0, cols, rows);
        vo.set_track_output(1 << 30);
        vo.set_motion_prior_mode(SVO_PRIOR_LAST_ROTATION);
        for (int attempt = 0; attempt < 2; attempt++) {
            CHECK(throws([&] { vo.stereo_callback(frame(0, 0), frame(0, 1)); }), "a track output of 1 << 30 rows accepted");
            CHECK(!vo.handle(), "a context after a refused first frame");
            CHECK(throws([&] { vo.last_track_observations(); }) && throws([&] { vo.last_motion_prior(); }), "a getter before the first frame");
        }
        vo.set_track_output(32);                                      // corrected: the same frame again, everything else still held
        vo.stereo_callback(frame(0, 0), frame(0, 1));
        int present = 0, mode = -1;
        std::vector<uint8_t> got(mask.size());
        C_OK(svo_get_detection_mask(vo.handle(), -1, got.data(), &present));
        C_OK(svo_get_motion_prior_mode(vo.handle(), &mode));
        CHECK(present == 1 && got == mask, "the held mask was not installed");
        CHECK(mode == SVO_PRIOR_LAST_ROTATION, "the held prior mode was not applied");
        CHECK(svo_get_last_frame_path(vo.handle()) & SVO_PATH_TRACK_IDS, "the corrected track output was not applied");
        vo.last_track_observations();
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    svo_destroy(live);
    std::printf("DEFERRED FACADE OK\n");
    return 0;
}
