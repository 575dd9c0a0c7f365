// svo_latency — single-stream latency of the synchronous callback as a C / C++ host sees it (no Python in the loop): the
// reference's own call pattern, one robot, one stream, stereo_callback(left, right) per camera frame (src/stereo_vo.cpp:61-62,
// src/main.cpp:394).  Reads stereo pairs from a raw file (int32 n, h, w; then n x (left, right) gray images), plays them
// ping-pong through svo_process and prints the mean / median / p95 wall time per call, with ordinary heap buffers and with
// page-locked ones (svo_alloc_pinned).
//   svo_latency frames.bin [win=21] [calls=200] [max_translation=2.0] [--covariance | --mask | --clahe | --tracks [--descriptors] | --prior | --prior-auto]   (KITTI-00 intrinsics: the file comes from tools/latency_cpp.py)
// --covariance: every leg is run twice, without and with the pose covariance (svo_set_pose_covariance, SVO_COV_RESIDUAL).
// --mask: every leg is run twice, without and with a static detection mask (svo_set_detection_mask: the lower quarter of the image
// closed, a bonnet) — a masked lone-stream frame issues the unfused front, one launch more.
// --clahe: every leg is run twice, without and with CLAHE (svo_set_clahe, clip 2.0, 8 x 8 tiles): two launches more per frame.
// --tracks: every leg is run twice, without and with the track output (svo_set_track_output, max_rows 2048): the unfused front, the
// ids builds of the emit, and two launches more per frame (k_ids_compact, k_track_obs).
// --tracks --descriptors: a third run of every leg with the descriptor output on top of the track output (svo_set_descriptor_output):
// one launch more per frame (k_track_desc) and 32 bytes more per row over PCIe.
// --prior: every leg is run twice, without and with a motion prior before every call (svo_set_motion_prior): the identity homography —
// the frame file holds no poses — so the tracks are the same and the difference is the mechanism's cost: the setter, one small copy
// on the frame's stream, k_lk_chain_prior in k_lk_chain's place.
// --prior-auto: every leg is run twice, without and with svo_set_motion_prior_mode(SVO_PRIOR_LAST_ROTATION): one launch more per frame
// (k_prior_predict) and k_lk_chain_prior, seeded with the rotation of the frame before.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>
#include "svo.h"

static double run(const std::vector<const uint8_t*>& L, const std::vector<const uint8_t*>& R, int w, int h, int win, int calls, double max_t, const char* label, bool covariance = false, bool mask = false, bool clahe = false, bool tracks = false, int prior = 0 /* 1: the identity before every call, 2: SVO_PRIOR_LAST_ROTATION */, bool descriptors = false) {
    svo_config cfg; svo_config_default(&cfg);
    cfg.win_w = cfg.win_h = win; cfg.max_translation_norm = max_t;
    svo_context* ctx = nullptr;
    if (svo_create(&cfg, 0, 1, w, h, &ctx) != SVO_OK) { std::fprintf(stderr, "svo_create: %s\n", svo_last_error()); std::exit(1); }
    const float Pl[12] = {718.856f, 0, 607.1928f, 0, 0, 718.856f, 185.2157f, 0, 0, 0, 1, 0};
    float Pr[12]; std::memcpy(Pr, Pl, sizeof(Pl)); Pr[3] = -386.1448f;
    svo_set_projection(ctx, -1, Pl, Pr);
    if (covariance && svo_set_pose_covariance(ctx, SVO_COV_RESIDUAL, 1.0) != SVO_OK) { std::fprintf(stderr, "svo_set_pose_covariance: %s\n", svo_last_error()); std::exit(1); }
    if (mask) {
        std::vector<uint8_t> m((size_t)w * h, 255);
        std::fill(m.begin() + (size_t)(h - h / 4) * w, m.end(), (uint8_t)0);
        if (svo_set_detection_mask(ctx, -1, m.data(), w, 0) != SVO_OK) { std::fprintf(stderr, "svo_set_detection_mask: %s\n", svo_last_error()); std::exit(1); }
    }
    if (clahe && svo_set_clahe(ctx, 1, 2.0, 8, 8) != SVO_OK) { std::fprintf(stderr, "svo_set_clahe: %s\n", svo_last_error()); std::exit(1); }
    if (tracks && svo_set_track_output(ctx, 1, 2048) != SVO_OK) { std::fprintf(stderr, "svo_set_track_output: %s\n", svo_last_error()); std::exit(1); }
    if (descriptors && svo_set_descriptor_output(ctx, 1) != SVO_OK) { std::fprintf(stderr, "svo_set_descriptor_output: %s\n", svo_last_error()); std::exit(1); }
    if (prior == 2 && svo_set_motion_prior_mode(ctx, SVO_PRIOR_LAST_ROTATION) != SVO_OK) { std::fprintf(stderr, "svo_set_motion_prior_mode: %s\n", svo_last_error()); std::exit(1); }
    const int n = (int)L.size();
    auto pp = [&](int i) { const int p = i % (2 * n - 2); return p < n ? p : 2 * n - 2 - p; };
    double T[16]; svo_frame_stats st; int n_ok = 0;
    const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 8; i++) svo_process(ctx, L[pp(i)], R[pp(i)], w, T, &st);
    std::vector<double> us(calls);
    for (int i = 0; i < calls; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (prior == 1 && svo_set_motion_prior(ctx, 0, eye, eye) != SVO_OK) { std::fprintf(stderr, "svo_set_motion_prior: %s\n", svo_last_error()); std::exit(1); }
        const int rc = svo_process(ctx, L[pp(8 + i)], R[pp(8 + i)], w, T, &st);
        us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (rc < 0) { std::fprintf(stderr, "svo_process: %s\n", svo_last_error()); std::exit(1); }
        n_ok += rc == 1;
    }
    svo_destroy(ctx);
    double mean = 0; for (double v : us) mean += v; mean /= calls;
    std::sort(us.begin(), us.end());
    std::printf("%-28s mean %.1f us   median %.1f   p95 %.1f   min %.1f   (%d calls, %d poses ok, %d features into LK)\n", label, mean, us[calls / 2], us[calls * 95 / 100], us[0], calls, n_ok, st.n_into_lk);
    return us[calls / 2];
}

int main(int argc, char** argv) {
    bool covariance = false, mask = false, clahe = false, tracks = false, descriptors = false; int prior = 0;
    if (argc > 3 && !std::strcmp(argv[argc - 1], "--descriptors") && !std::strcmp(argv[argc - 2], "--tracks")) { descriptors = true; argc--; }
    if (argc > 2 && !std::strcmp(argv[argc - 1], "--covariance")) { covariance = true; argc--; }
    else if (argc > 2 && !std::strcmp(argv[argc - 1], "--mask")) { mask = true; argc--; }
    else if (argc > 2 && !std::strcmp(argv[argc - 1], "--clahe")) { clahe = true; argc--; }
    else if (argc > 2 && !std::strcmp(argv[argc - 1], "--tracks")) { tracks = true; argc--; }
    else if (argc > 2 && !std::strcmp(argv[argc - 1], "--prior")) { prior = 1; argc--; }
    else if (argc > 2 && !std::strcmp(argv[argc - 1], "--prior-auto")) { prior = 2; argc--; }
    if (argc < 2) { std::fprintf(stderr, "usage: svo_latency frames.bin [win] [calls] [max_translation] [--covariance | --mask | --clahe | --tracks [--descriptors] | --prior | --prior-auto]\n"); return 2; }
    const int win = argc > 2 ? std::atoi(argv[2]) : 21, calls = argc > 3 ? std::atoi(argv[3]) : 200;
    const double max_t = argc > 4 ? std::atof(argv[4]) : 2.0;
    std::ifstream f(argv[1], std::ios::binary);
    int hdr[3];
    f.read((char*)hdr, sizeof(hdr));
    const int n = hdr[0], h = hdr[1], w = hdr[2];
    const size_t img = (size_t)w * h;
    std::vector<uint8_t> heap(img * 2 * n);
    f.read((char*)heap.data(), (std::streamsize)heap.size());
    if (!f || n < 2) { std::fprintf(stderr, "bad frame file\n"); return 2; }
    std::vector<const uint8_t*> L(n), R(n);
    for (int k = 0; k < n; k++) { L[k] = heap.data() + img * (2 * k); R[k] = heap.data() + img * (2 * k + 1); }
    run(L, R, w, h, win, calls, max_t, "heap buffers:");
    if (covariance) run(L, R, w, h, win, calls, max_t, "heap buffers, covariance:", true);
    if (mask) run(L, R, w, h, win, calls, max_t, "heap buffers, mask:", false, true);
    if (clahe) run(L, R, w, h, win, calls, max_t, "heap buffers, CLAHE:", false, false, true);
    if (tracks) run(L, R, w, h, win, calls, max_t, "heap buffers, tracks:", false, false, false, true);
    if (descriptors) run(L, R, w, h, win, calls, max_t, "heap buffers, descriptors:", false, false, false, true, 0, true);
    if (prior) run(L, R, w, h, win, calls, max_t, prior == 2 ? "heap buffers, prior auto:" : "heap buffers, prior:", false, false, false, false, prior);
    uint8_t* pin = (uint8_t*)svo_alloc_pinned(heap.size());
    if (pin) {
        std::memcpy(pin, heap.data(), heap.size());
        for (int k = 0; k < n; k++) { L[k] = pin + img * (2 * k); R[k] = pin + img * (2 * k + 1); }
        run(L, R, w, h, win, calls, max_t, "page-locked buffers:");
        if (covariance) run(L, R, w, h, win, calls, max_t, "page-locked, covariance:", true);
        if (mask) run(L, R, w, h, win, calls, max_t, "page-locked, mask:", false, true);
        if (clahe) run(L, R, w, h, win, calls, max_t, "page-locked, CLAHE:", false, false, true);
        if (tracks) run(L, R, w, h, win, calls, max_t, "page-locked, tracks:", false, false, false, true);
        if (descriptors) run(L, R, w, h, win, calls, max_t, "page-locked, descriptors:", false, false, false, true, 0, true);
        if (prior) run(L, R, w, h, win, calls, max_t, prior == 2 ? "page-locked, prior auto:" : "page-locked, prior:", false, false, false, false, prior);
        svo_free_pinned(pin);
    }
    return 0;
}
