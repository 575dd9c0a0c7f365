/*
 * svo.h — C-ABI of the MI355X-native stereo-VO per-frame front end (libsvo_hip.so).
 *
 * This is the drop-in boundary for the hot path of Alex7Li/stereo_visual_odometry:
 *   VisualOdometry::stereo_callback  (reference src/vo.cpp:41-137, decl include/vo.h:333-334)
 * and the stage functions its own tests call directly (src/main.cpp:110,125,168,196,243).
 * The reference has no FFI today (plain C++ class API, include/vo.h:46-472); every entry point
 * below names the reference interface it replaces.  Plain pointers and sizes only — no C++ types,
 * no torch types.  All functions return SVO_OK (0) or a negative svo_status; nothing throws.
 *
 * Everything behind this header runs on the GPU (hand-written HIP kernels for gfx950).  There is
 * no CPU fallback: if no HIP device is usable the calls fail with SVO_ERR_HIP.
 *
 * Pointer convention: unless a parameter is documented as "device", pointers are HOST memory and
 * the call synchronises before returning.
 */
#ifndef SVO_H
#define SVO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SVO_OK = 0,
    SVO_ERR_ARG = -1,      /* bad argument (null pointer, size mismatch, unsupported window ...) */
    SVO_ERR_HIP = -2,      /* HIP runtime error / no device; svo_last_error() has the text */
    SVO_ERR_CAPACITY = -3, /* input exceeds the capacity the context was created with */
    SVO_ERR_STATE = -4,    /* call order violated (e.g. projection not set) */
    SVO_ERR_INTERNAL = -5  /* the library found a state it rules out ("Index maintenance": the latest-per-id table overflowed) */
} svo_status;

/* The reference's compile-time constants (include/vo.h:53-127, 251-252; src/vo.cpp:183-184, 295)
 * as a run-time struct.  svo_config_default() fills the reference values. */
typedef struct {
    int bucket_start_row;                 /* vo.h:53   4   */
    int buckets_along_height;             /* vo.h:60   92  */
    int buckets_along_width;              /* vo.h:61   160 */
    int features_per_bucket;              /* vo.h:65   1   (1 .. 64; 1 takes the fused argmax path, larger capacities the general Bucket::add_feature walk) */
    int features_threshold;               /* vo.h:71   15  */
    int pre_matching_feature_threshold;   /* vo.h:78   100 */
    int age_threshold;                    /* vo.h:84   20  */
    int fast_threshold;                   /* vo.h:90   20  */
    float ransac_reprojection_error;      /* vo.h:97   8   */
    int ransac_iterations;                /* vo.h:102  100 */
    double optical_flow_min_eig_threshold;/* vo.h:108  1e-3 */
    double circular_matching_success_threshold; /* vo.h:115 0.15 */
    double max_translation_norm;          /* vo.h:121  0.1 */
    double max_rotation_norm;             /* vo.h:127  0.5 */
    int win_w, win_h;                     /* vo.h:251  10x10 (square, 5 .. 31; 3-channel contexts 5 .. 21) */
    int max_level;                        /* vo.h:252  3 */
    int lk_max_count;                     /* vo.cpp:183 30 */
    double lk_epsilon;                    /* vo.cpp:184 1e-4 */
    float ransac_confidence;              /* vo.cpp:295 0.98f */
    int max_features;                     /* build preset (not in the reference): 0 = unlimited */
    int channels;                         /* 1 (default): 8-bit single-channel images, what the ROS path delivers (stereo_vo.cpp:9).
                                           * 3: interleaved 8-bit BGR, what the reference CLI really feeds (main.cpp:38-46 returns the
                                           * colour Mats): cv::FAST then walks the first `width` BYTES of every row (it has no channel
                                           * check), pyramids and LK are 3-channel.  Frame pipeline only (svo_process*, svo_submit_batch);
                                           * strides are in bytes.  Reproduces the trajectory the reference recorded for run1/. */
    int lk_float_sums;                    /* 0 (default): the LK normal equations are summed as exact integers (order-independent, fastest).
                                           * 1: they are summed in FLOAT in the lane order of OpenCV 4.x's SIMD128 code (lkpyramid.cpp,
                                           * `#if CV_SIMD128 && !CV_NEON`), i.e. with OpenCV's own rounding.  Measured on the reference's
                                           * recording: mode 1 reproduces run1/result.csv digit for digit (with channels = 3), mode 0 flips
                                           * borderline tracks at 4 of its first 24 frames (1e-5 .. 1e-3 m).  2.4 times the default's LK
                                           * time at the 21x21 window (the float chains are serial); frame pipeline and svo_circular_matching only. */
} svo_config;

/* Per-frame counters — the numbers the reference prints at vo.cpp:226,239,326,331,365,108-110,128-130. */
typedef struct {
    int n_after_detect;     /* vo.cpp:326 / :331 */
    int second_pass;        /* vo.cpp:327-332 ran */
    int n_into_lk;
    int n_after_circular;   /* vo.cpp:239 */
    int n_after_bounds;     /* vo.cpp:365 */
    int n_inliers;          /* vo.cpp:103 */
    int ransac_iters;       /* iterations the adaptive RANSAC loop would have run */
    int fail_reason;        /* 0 ok, 1 first frame, 2 too few tracks (vo.cpp:82), 3 RANSAC fail / few inliers (:106), 4 motion gate (:129),
                             * 5 idle: the sequence did not take this frame (svo_process_batch_masked / svo_submit_batch_masked; every
                             * other field is 0, T is its last good transform, ok is 0) */
    int n_features_out;     /* size of currentVOFeatures on return */
    int lk_level_visits;    /* (feature, pass, level) visits of the LK passes that reached the Newton loop.  A feature runs its passes
                             * up to and including the first one that returns status 0: vo.cpp:227-238 deletes it whatever the later
                             * passes return, so the frame pipeline does not run them */
    int lk_newton_steps;    /* Newton iterations of those passes (the work term of the LK flop model) */
    int lk_dead_after_pass[3]; /* features whose status first became 0 in pass 0 (L0->L1), 1 (L1->R1), 2 (R1->R0) */
} svo_frame_stats;

typedef struct svo_context svo_context;

const char* svo_last_error(void);
int  svo_device_count(void);
void svo_config_default(svo_config* cfg);

/* ------------------------------------------------------------------------------------------------
 * Frame pipeline.  One context = n_seq independent VisualOdometry instances (reference: one object
 * per stream, include/vo.h:231) on one GPU, sharing image size and config; they advance in lock-step
 * through svo_process_batch.  n_seq = 1 is the reference's single-instance use.
 * ---------------------------------------------------------------------------------------------- */

/* replaces: VisualOdometry::VisualOdometry()  (vo.h:277, vo.cpp:5) */
int svo_create(const svo_config* cfg, int device, int n_seq, int width, int height, svo_context** out);
void svo_destroy(svo_context* ctx);

/* replaces: VisualOdometry::initalize_projection_matricies(Pl, Pr)  (vo.h:307-309, vo.cpp:8-26).
 * Pl, Pr: 3x4 float32 row-major.  seq = -1 sets every sequence. */
int svo_set_projection(svo_context* ctx, int seq, const float Pl[12], const float Pr[12]);

/* replaces: VisualOdometry::stereo_callback(left, right) -> pair<bool, Mat_<double>>  (vo.h:333-334, vo.cpp:41-137)
 * for all n_seq sequences at once.  left/right: n_seq pointers to 8-bit single-channel images
 * (width x height, row stride `stride` bytes); images_on_device != 0 means they are device pointers.
 * T_out: n_seq x 16 doubles (4x4 row-major): the pair's .second (last good transform on failure).
 * ok_out: n_seq ints: the pair's .first.  stats: n_seq entries or NULL. */
int svo_process_batch(svo_context* ctx, const uint8_t* const* left, const uint8_t* const* right, int stride,
                      int images_on_device, double* T_out, int* ok_out, svo_frame_stats* stats);

/* Page-locked host memory for the caller's image buffers (hipHostMalloc underneath; any hipHostMalloc'ed / hipHostRegister'ed
 * memory works the same).  svo_process / svo_process_batch given host images COPY them first (SURVEY.md 8b "Ownership": inputs
 * are borrowed for the call only); images that lie in page-locked memory with packed rows (stride == width * channels) are read
 * by the DMA engines in place, which saves the staging memcpy — ~40 us per 1241x376 pair, 0.54 -> 0.50 ms per synchronous call.
 * The reference has no counterpart (cv::Mat data is ordinary heap memory). */
void* svo_alloc_pinned(size_t bytes);
void  svo_free_pinned(void* p);

/* n_seq == 1 convenience with the reference's callback shape (also the ROS-callback shape, src/stereo_vo.cpp:61-62).
 * Returns 1 (pose produced), 0 (no pose this frame; T_out = last good transform) or a negative svo_status. */
int svo_process(svo_context* ctx, const uint8_t* left, const uint8_t* right, int stride, double T_out[16], svo_frame_stats* stats);

/* replaces: VisualOdometry::circularMatching(imgLeftT1, imgRightT1, pointsLeftT0, pointsRightT0, pointsLeftT1, pointsRightT1, features)
 * (vo.h:374-379, vo.cpp:169-240) as the MEMBER call it is in the reference: the T0 side is the pyramid pair this context
 * cached in its last svo_process / svo_circular_matching (vo.h:257-258; prime it with svo_process, as main.cpp:191 does), the
 * pyramids of the given T1 images become the cached pair (vo.cpp:231-232) — the next svo_process tracks against them.
 * Without the compaction: n points in, n points out per list, ok[n] = all four LK statuses && loop closure (vo.cpp:217-230).
 * n == 0 returns before anything is cached (vo.cpp:179-181).  n_seq == 1 contexts; images in the context's format. */
int svo_circular_matching(svo_context* ctx, const uint8_t* left_t1, const uint8_t* right_t1, int stride, int n,
                          const float* pl0, float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok);

/* Asynchronous form for throughput: enqueue one frame for every sequence and return immediately
 * (device pointers only; the images must stay valid until the matching svo_collect).
 * Results are queued in order; svo_collect blocks for the oldest outstanding frame. At most 8 in flight. */
/* Diagnostics: VGPRs one SIMD has left beside a full complement of this context's LK waves (-1 unknown).  Several many-sequence
 * contexts on one device overlap their f64 kernels with each other's LK kernel only when this is >= 96.  At the metric's window
 * (w = 21, single channel) it is 32 since round 3 — six waves of 80 registers: the faster LK build wins over the overlap, DESIGN.md
 * section 2 — so such contexts simply take turns.  Builds that leave >= 96 keep the overlap scheme; by the compiler's register
 * counts (profiles/r04_lk_vgprs.md) those are w = 22 single channel, and with lk_float_sums = 1 w = 17, 19, 23, 28-31 single
 * channel and w = 10, 12 three-channel.  A test pins the w = 21 figure, so that a change to the LK kernel that alters the
 * regime fails loudly; another probes which builds reach the overlap scheme and runs them against the oracle.
 * NOTE on locality: creating or destroying ANOTHER context with more than 8 sequences on the same device changes which builds of
 * the PnP / triangulation kernels this context launches from its next frame on (full-register alone; 96-register when the
 * device is shared and the figure above is >= 96) and chains its LK launches behind the other's.  Results are bit-identical
 * either way: the 96-register refine sums its terms in the order of the full build.  svo_get_last_frame_path tells which
 * builds a frame took. */
int svo_get_lk_registers_left(svo_context* ctx);

/* Diagnostics: the decisions the library made for the most recently ISSUED frame of ctx (svo_process*, svo_submit*), as a
 * bitmask of SVO_PATH_*; 0 before the first frame and for a frame on which every sequence was idle.  ctx == NULL: those of this
 * thread's last stage call that runs the f64 kernels (svo_triangulate, svo_camera_to_world).  Host-side bookkeeping only. */
#define SVO_PATH_LEAN            1   /* the 96-register builds of triangulation / EPnP / refine (shared device, or SVO_FORCE_LEAN=1) */
#define SVO_PATH_LK_CHAINED      2   /* the LK launch waited for / armed the device's chaining event (several many-sequence contexts) */
#define SVO_PATH_INGEST_AHEAD    4   /* the pyramids were built ahead on the context's image stream (many sequences) */
#define SVO_PATH_FRONT_FUSED     8   /* the fused lone-stream front (ingest + pyramid beside detection) */
#define SVO_PATH_TRI_EPNP_FUSED 16   /* triangulation and the first EPnP chunk in one launch (lone stream) */
#define SVO_PATH_GRAPH          32   /* the frame replayed a captured hipGraph (SVO_GRAPH=1); the other bits are the capture's */
#define SVO_PATH_INPUT_CONVERTED 64  /* the frame's ingest converted the caller's pixels to grey (svo_set_input_format) */
#define SVO_PATH_POSE_COV       128  /* the frame ran k_pose_cov after its refine (svo_set_pose_covariance; also set by svo_pose_covariance) */
#define SVO_PATH_CLAHE          512  /* the frame's images were equalised (two launches) in front of its ingest (svo_set_clahe; also set by svo_clahe) */
#define SVO_PATH_DETECT_MASKED  256  /* the frame's detection applied a detection mask (svo_set_detection_mask; also set by svo_append_features_from_image_masked) */
#define SVO_PATH_TRACK_IDS    1024   /* the frame carried track ids and wrote its observation rows (svo_set_track_output) */
#define SVO_PATH_MOTION_PRIOR 2048   /* some active sequence of the frame used a motion prior: k_lk_chain_prior ran in k_lk_chain's place (svo_set_motion_prior) */
int svo_get_last_frame_path(svo_context* ctx);

int svo_submit_batch(svo_context* ctx, const uint8_t* const* left_dev, const uint8_t* const* right_dev, int stride);
int svo_collect(svo_context* ctx, double* T_out, int* ok_out, svo_frame_stats* stats);

/* Ragged / continuous batching (the reference has no counterpart: it is one object per stream).  active: host array of n_seq
 * bytes, nonzero = the sequence takes this frame; NULL = all active (then identical to the unmasked call).  The image pointers of
 * idle sequences are not read and may be NULL (the arrays too, when no sequence is active); an active sequence with a NULL
 * pointer is SVO_ERR_ARG.  An idle sequence's state is not touched — its active frames give the same results whether idle frames
 * are interleaved or not — and its result row is its last good T, ok 0, all stats 0 but fail_reason 5; frame_id does not advance.
 * An all-idle frame is legal, takes a results-ring slot like any other and launches only the result write.  The kernels' grids
 * cover the active sequences only. */
int svo_process_batch_masked(svo_context* ctx, const uint8_t* const* left, const uint8_t* const* right, int stride,
                             int images_on_device, const uint8_t* active, double* T_out, int* ok_out, svo_frame_stats* stats);
int svo_submit_batch_masked(svo_context* ctx, const uint8_t* const* left_dev, const uint8_t* const* right_dev, int stride,
                            const uint8_t* active);
/* Return one sequence (seq = -1: all) to the state of a freshly created context, so its next active frame is a first frame
 * (fail_reason 1).  Pl / Pr: new projection matrices for it (K = Pl[:, :3], as svo_set_projection), or both NULL to keep them;
 * exactly one NULL is SVO_ERR_ARG.  Stream-ordered: takes effect after every frame already submitted and before every frame
 * submitted later.  Does not synchronise, and is legal with frames in flight. */
int svo_reset_sequence(svo_context* ctx, int seq, const float Pl[12], const float Pr[12]);

/* ------------------------------------------------------------------------------------------------
 * Rectification of raw frames — replaces what feeds the reference's left/image_rect and right/image_rect topics
 * (src/stereo_vo.cpp:53-54): image_geometry::PinholeCameraModel::rectifyImage in stereo_image_proc, i.e.
 * cv::initUndistortRectifyMap once per calibration + cv::remap per frame.  A rectifying context takes RAW frames (raw_w x raw_h
 * pixels, rows `stride` bytes, channels as configured) in every frame entry point (svo_process, svo_process_batch[_masked],
 * svo_submit_batch[_masked], svo_circular_matching); level 0 of every pyramid and the FAST image are the rectified frame
 * (width x height of svo_create), so everything downstream sees exactly the bytes it would have seen had the caller passed
 * the rectified images.  Without maps a context is plain and launches exactly what it always did.
 *
 * Map (per camera): for every rectified pixel (u, v), a source position in the raw image in fixed point with 5 fractional
 * bits, ix = round_half_even(src_x * 32) (likewise iy) — OpenCV's CV_16SC2 + CV_16UC1 pair:
 *   map1[v][u] = (ix >> 5, iy >> 5) as int16 x 2,   map2[v][u] = (iy & 31) * 32 + (ix & 31) as uint16 (masked to 10 bits).
 * Interpolation (bilinear, 8-bit, per channel), x0 = ix >> 5, fx = ix & 31 (likewise y):
 *   out = ((32-fx)(32-fy) p(x0,y0) + fx(32-fy) p(x0+1,y0) + (32-fx)fy p(x0,y0+1) + fx fy p(x0+1,y0+1) + 512) >> 10,
 * a tap outside the raw image reads 0 (BORDER_CONSTANT, value 0).  This is cv::remap's INTER_LINEAR with INTER_BITS = 5 and
 * 15-bit weights: each weight * 32768 is an exact multiple of 32, so the forms agree and no weight correction ever applies.
 * PARITY UNPINNED: equality with cv::remap is believed, not measured (no OpenCV on the machines this was built on); the tests
 * pin the kernels to a numpy restatement of the formula above, bit for bit.
 * ---------------------------------------------------------------------------------------------- */

/* A ROS sensor_msgs/CameraInfo, as far as rectification needs it.  D: plumb_bob (n_d = 5: k1 k2 p1 p2 k3) or
 * rational_polynomial (n_d = 8: k1 k2 p1 p2 k3 k4 k5 k6); n_d = 0 or 4 are accepted too.  R, P row-major.  width x height is
 * the RAW image size.  Thin-prism / tilt coefficients and the fisheye model are not covered: pass your own maps for those. */
typedef struct {
    double K[9];
    double D[8];
    int n_d;
    double R[9];
    double P[12];
    int width, height;
} svo_camera_info;

/* Install maps for one sequence, or (seq = -1) the shared maps used by every sequence without maps of its own — stored once,
 * not per sequence.  map1_*: width*height*2 int16, map2_*: width*height uint16 (the context's rectified size).  raw_w / raw_h are
 * fixed per context: the first call sets them, later calls must match (SVO_ERR_ARG).  Stream-ordered like svo_reset_sequence:
 * legal with frames in flight, takes effect from the next frame submitted — every frame carries its own map pointers, a
 * replaced map is freed once no frame in flight names it.  The slot handover of a continuous pool is svo_reset_sequence(seq,
 * Pl, Pr) + svo_set_rectification(seq, ...) before the next submit.  A frame in which an active sequence has no map (neither
 * its own nor shared) fails with SVO_ERR_STATE.  Host images given to svo_process / svo_process_batch are read in place by the
 * DMA engines when pinned with stride == raw_w * channels. */
int svo_set_rectification_maps(svo_context* ctx, int seq, int raw_w, int raw_h, const int16_t* map1_l, const uint16_t* map2_l,
                               const int16_t* map1_r, const uint16_t* map2_r);
/* Convenience: builds both maps with svo_init_rectify_map (raw size = left->width x left->height; both must agree) and installs
 * them as svo_set_rectification_maps does.  It does NOT call svo_set_projection: pass left->P / right->P there (as float).  ROS's
 * P_right[0][3] = -fx * baseline is exactly the reference's negative bf term (stereo_vo.cpp:47). */
int svo_set_rectification(svo_context* ctx, int seq, const svo_camera_info* left, const svo_camera_info* right);
/* Back to a plain context (frames at the rectified size, no remap) from the next frame submitted; results are then bit-identical
 * to a context that never had maps.  The raw size may be set afresh afterwards. */
int svo_clear_rectification(svo_context* ctx);

/* ------------------------------------------------------------------------------------------------
 * Input formats — replaces cv_bridge::toCvCopy(img, MONO8) in the reference's ROS node (src/stereo_vo.cpp:6-14), i.e. the
 * cv::cvtColor(.., ..2GRAY) a colour or YUV camera costs per frame and per camera on the CPU.  A channels == 1 context has an
 * input format: it describes the BYTES OF THE FRAMES THE CALLER PASSES; the context's own pixel format stays mono8, and the
 * conversion happens inside frame ingest, while the source tile is staged — no extra pass over memory, nothing downstream
 * changes.  (channels = 3 is something else: the CLI's BGR quirk, which keeps three planes.)
 *
 *   constant                             value   bytes per pixel   grey value of pixel x of a row
 *   SVO_INPUT_MONO8 (default)            0       1                 the byte
 *   SVO_INPUT_BGR8 / SVO_INPUT_RGB8      1 / 2   3                 the formula below
 *   SVO_INPUT_BGRA8 / SVO_INPUT_RGBA8    3 / 4   4                 the formula below, alpha ignored
 *   SVO_INPUT_UYVY                       5       2                 byte 2x + 1 of the row (COLOR_YUV2GRAY_UYVY: Y extracted)
 *   SVO_INPUT_YUY2                       6       2                 byte 2x of the row
 *
 *   grey = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14
 * — cv::cvtColor BGR2GRAY for 8-bit images as SURVEY.md Appendix A.7, tools/svo_cli.cpp --gray 1 and
 * tests/golden/make_run1_fixture.py restate it.
 * PARITY UNPINNED: equality with cv::cvtColor is believed, not measured (no OpenCV on the machines this was built on).  Newer
 * OpenCV releases may use 15-bit weights (3735, 19235, 9798, >> 15); on the committed run1 frames the two formulas differ at
 * 2e-5 of the pixels, by one grey level.  Which one a given cv_bridge build runs has not been verified.  The tests pin the kernels
 * to a numpy restatement of the table above, bit for bit.
 *
 * With rectification the conversion comes first, as image_proc does it (image_mono -> image_rect): each of the four raw taps is
 * converted to grey, a tap outside the raw image is 0, and the bilinear formula of the rectification section runs on the grey
 * taps — remap(grey(raw), map1, map2).
 *
 * Every frame entry point (svo_process, svo_process_batch[_masked], svo_submit_batch[_masked], svo_circular_matching) then takes
 * frames of in_width x in_height pixels (the raw size when rectifying) whose rows are `stride` bytes apart and hold
 * in_width * bytes_per_pixel bytes; stride < in_width * bytes_per_pixel is SVO_ERR_ARG.  The kernels never read a byte outside
 * [0, in_width * bytes_per_pixel) of a row: the caller's buffers need no slack.  Host images are staged, or read in place when
 * pinned with packed rows, at in_width * bytes_per_pixel bytes per row.
 * ---------------------------------------------------------------------------------------------- */
#define SVO_INPUT_MONO8 0
#define SVO_INPUT_BGR8  1
#define SVO_INPUT_RGB8  2
#define SVO_INPUT_BGRA8 3
#define SVO_INPUT_RGBA8 4
#define SVO_INPUT_UYVY  5
#define SVO_INPUT_YUY2  6
/* Set the format of the frames submitted from now on.  A channels == 3 context or an unknown format: SVO_ERR_ARG.  Stream-ordered
 * like svo_clear_rectification: legal with frames in flight, takes effect from the next frame submitted — the kernels are chosen
 * on the host when a frame is issued, so every frame carries its own format.  SVO_INPUT_MONO8 returns the context to launching
 * exactly the kernels of a context that never called this.  svo_get_last_frame_path reports SVO_PATH_INPUT_CONVERTED for a frame
 * whose ingest converted.  Under SVO_GRAPH=1 a converting frame replays a graph captured for its format (the format is part of
 * what a slot's graph is keyed on, so a format switch re-captures); results are identical to the launch list's. */
int svo_set_input_format(svo_context* ctx, int format);

/* ---- CLAHE: contrast-limited adaptive histogram equalisation in frame ingest ------------------------------------------------
 * Replaces cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply() on both images of a frame (VINS-Fusion's `equalize`,
 * ORB-SLAM3's preprocessing): FAST's threshold and LK's minimum-eigenvalue cut are absolute grey-level quantities, so shadow,
 * tunnels and over-exposed scenes lose features without it.  A channels == 1 context only.  The input is the caller's frame in
 * grey, in_width x in_height pixels (the raw size when rectifying), after the input-format conversion and before rectification
 * — remap(clahe(grey(raw))) — each camera from its own histograms.  Detection masks live in the rectified geometry and are
 * unaffected.
 *
 * Definition (w x h image, tiles_x x tiles_y tiles, each 1 .. 16):
 *  1. Padding.  w % tiles_x == 0 && h % tiles_y == 0: the extended image is the image.  Otherwise it is the image extended on the
 *     right by tiles_x - (w % tiles_x) columns and at the bottom by tiles_y - (h % tiles_y) rows with REFLECT_101 — a dimension
 *     that IS divisible is then extended by a whole tiles_* (OpenCV's quirk).  tw = ext_w / tiles_x, th = ext_h / tiles_y,
 *     area = tw th.  An extension beyond w - 1 / h - 1 (REFLECT_101 undefined) or tw / th == 0 is rejected.
 *  2. Per tile: the 256-bin histogram of its tw x th pixels of the extended image.  clip_limit > 0:
 *     clip = max((int)(clip_limit * area / 256), 1) (product and quotient in double); every bin above clip is cut to clip,
 *     clipped = the sum of the excess; batch = clipped / 256, residual = clipped - 256 batch; every bin += batch; if residual > 0,
 *     step = max(256 / residual, 1) and for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++.
 *     clip_limit <= 0: no clipping.
 *  3. LUT: scale = 255.0f / (float)area; with the running integer sum s over the bins,
 *     lut[i] = clamp(rint_half_even((float)s * scale), 0, 255).
 *  4. Interpolation, all f32, every operation rounded on its own (no FMA), in this order; inv_tw = 1.0f / tw, inv_th = 1.0f / th.
 *     Pixel (x, y) of the original image with value v: txf = (float)x * inv_tw - 0.5f; tx1 = floor(txf), tx2 = tx1 + 1;
 *     xa = txf - (float)tx1, xa1 = 1.0f - xa; then tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1); the same in y;
 *     res = (L[ty1][tx1][v] xa1 + L[ty1][tx2][v] xa) ya1 + (L[ty2][tx1][v] xa1 + L[ty2][tx2][v] xa) ya;
 *     out = clamp(rint_half_even(res), 0, 255).
 * PARITY UNPINNED: this restates cv::CLAHE::apply for 8-bit images from memory of OpenCV 4.x clahe.cpp; equality with OpenCV is
 * believed, not measured (no OpenCV on the machines this was built on).  The tests pin the kernels to a numpy restatement of
 * exactly the text above, bit for bit.
 *
 * svo_set_clahe: on = 0 switches it off (the other arguments are not looked at).  Host state like svo_set_input_format: legal with
 * frames in flight, every frame carries the setting it was issued with, from the next frame submitted.  SVO_ERR_ARG: a
 * channels == 3 context, tiles outside 1 .. 16, a non-finite clip_limit, a geometry rule 1 rejects for the context's input size
 * (checked when the setter runs; if svo_set_rectification* later changes the raw size to one rule 1 rejects, the frame submit
 * fails with SVO_ERR_STATE).  With CLAHE off a context launches exactly what it always did and no new path bit shows; with it on a
 * frame runs two launches (per-tile LUTs, then interpolation into a library-owned mono8 staging frame) in front of its unchanged
 * mono8 ingest, on the stream the ingest runs on, and reports SVO_PATH_CLAHE (and SVO_PATH_INPUT_CONVERTED when its format
 * converts).  Idle sequences of a ragged frame are not touched.  Under SVO_GRAPH=1 CLAHE frames run from the launch list. */
int svo_set_clahe(svo_context* ctx, int on, double clip_limit, int tiles_x, int tiles_y);

/* ---- Pose covariance ------------------------------------------------------------------------------------------------------
 * A 6x6 covariance with every pose, computed on the device right after the refine and written into the results ring beside the
 * pose: no extra copy, no extra synchronisation, valid with frames in flight.  Off by default; mode 0 launches exactly what a
 * context that never called the setter launches, and no other result of a frame changes by a bit in any mode.
 *
 * Definition, for a frame with ok = 1.  p^ = (r^, t^): the rotation vector and translation of the refined solvePnP result (the
 * cameraToWorld parameters; the returned T = [R^ t^; 0 1]^-1).  The inliers are the m tracks with inlier[i] = 1 of
 * svo_get_last_tracks; X_i = world[i], u_i = pl1[i], both f32 widened to f64.
 *   residuals   e_i(p) = pi(R(r) X_i + t) - u_i,   pi(x, y, z) = (fx x / z + cx, fy y / z + cy), fx fy cx cy of K = Pl[:, :3]
 *   J           the 2m x 6 Jacobian of e with respect to (r, t) at p^ (what the refine's own iterations form);  H = Jt J
 *   sigma^2     SVO_COV_RESIDUAL: |e(p^)|^2 / (2m - 6);   SVO_COV_FIXED_SIGMA: pixel_sigma^2
 *   cov_p       sigma^2 H^-1: 6x6 row-major in the order (r0 r1 r2 t0 t1 t2), the covariance of the cameraToWorld parameters
 *   cov_T       G cov_p Gt: the covariance of the returned T in the order (c0 c1 c2 phi0 phi1 phi2) — position first, as ROS orders
 *               a pose covariance.  c = -R(r)t t is T's translation column, phi the LEFT perturbation of its rotation block,
 *               R_out = Exp(phi) R^t.  With c^ = -R^t t^ and the right Jacobian of SO(3)
 *               Jr(r) = I - (1 - cos th) / th^2 [r]x + (th - sin th) / th^3 [r]x^2   (I - [r]x / 2 for th < 1e-9):
 *                   G = [ [c^]x Jr(r^)   -R^t ]
 *                       [    -Jr(r^)       0  ]
 *   valid = 1   iff ok = 1, m >= 3 (H has rank <= 2m), 2m - 6 > 0 in mode SVO_COV_RESIDUAL, and every Cholesky pivot of H is
 *               positive — more than 2^-40 of the diagonal entry it is what is left of, so that the rounding noise of a singular H
 *               does not pass for a pivot.  Otherwise valid = 0 and all 72 numbers are 0.0: failed frames (fail_reason 1-4) and
 *               idle sequences (fail_reason 5) included.
 * All arithmetic is f64.  The 96-register build sums in the order of the full one: identical bits either way. */
#define SVO_COV_OFF 0
#define SVO_COV_RESIDUAL 1      /* sigma^2 = |e|^2 / (2m - 6) */
#define SVO_COV_FIXED_SIGMA 2   /* sigma = pixel_sigma */
/* Set the mode of the frames submitted from now on (legal with frames in flight: every frame carries the mode it was issued with,
 * as it carries its input format; under SVO_GRAPH=1 a switch re-captures the slot's graph).  A bad mode, or SVO_COV_FIXED_SIGMA
 * with pixel_sigma <= 0 or not finite: SVO_ERR_ARG (pixel_sigma is not looked at in the other modes). */
int svo_set_pose_covariance(svo_context* ctx, int mode, double pixel_sigma);
/* The covariances of the last COLLECTED frame (svo_collect, svo_process*): cov_T and cov_p B x 36 doubles, valid B ints; each may
 * be NULL.  SVO_ERR_STATE if that frame was issued with SVO_COV_OFF or none was collected yet.  Host memory only: no device
 * access, no synchronisation.  A frame on which every sequence was idle launches nothing: its rows are zero with valid = 0 as
 * for any idle sequence, and svo_get_last_frame_path reports 0 for it — without SVO_PATH_POSE_COV — whatever the mode. */
int svo_get_last_pose_covariance(svo_context* ctx, double* cov_T, double* cov_p, int* valid);

/* Introspection (parity tests): currentVOFeatures (vo.h:245) of one sequence, and the last frame's
 * compacted tracks.  Arrays may be NULL.  Returns the count or a negative status.  inlier[] is the is_ok vector of vo.cpp:115-119:
 * all zero when the frame failed before it was built (RANSAC failure or fewer inliers than features_threshold, vo.cpp:106-113). */
int svo_get_features(svo_context* ctx, int seq, int cap, float* xy, int* ages, int* strengths);
int svo_get_last_tracks(svo_context* ctx, int seq, int cap, float* pl0, float* pr0, float* pl1, float* pr1,
                        float* world, uint8_t* inlier);
/* ---- Track ids and per-frame stereo observations ---------------------------------------------------------------------------
 * What a landmark back end consumes (a sliding-window bundle adjuster, a smart-factor graph, an MSCKF): per frame, a list of
 * (landmark id, stereo observation).  Off by default; off, a context launches exactly what a context that never called the
 * setter launches.  On, every feature carries a 64-bit id through the frame and the frame's tracks are written, as rows of
 * svo_track_obs, into a pinned ring beside the pose: no extra copy, no extra synchronisation, valid with frames in flight.
 * Nothing a frame already returned (pose, stats, svo_get_features, svo_get_last_tracks) changes by a bit.
 *
 * The identity rule.  Per (context, sequence) there is a counter next_id (int64): 0 at creation and after svo_reset_sequence
 * (stream-ordered like the rest of the reset).
 *  1. Detection pass (each of the two, feature_set.cpp:75-89).  The pass publishes a feature set of n_out entries in bucket-raster
 *     order.  An entry that came from the existing list (rank < n_old in the pass's input list — a track that ties with a fresh
 *     FAST hit at the same pixel wins as first-come) keeps its id.  A fresh FAST hit at output position p gets next_id + p.  After
 *     the pass next_id += n_out.  Ids are unique and increasing, not dense.  The second pass applies the same rule to the first
 *     pass's output: a first-pass newcomer displaced in the second pass burns its id.
 *  2. Circular + bounds compaction (stable).  The id of feature i goes to track and feature position pos, with the age.  Features
 *     beyond max_features drop out with their ids.
 *  3. Inlier compaction (only on the path that replaces the feature set by the inliers: fail_reason 0 or 4).  New feature pos takes
 *     the id of the track it was (the pos-th inlier).  On fail_reason 2 and 3 the feature set, and so its ids, is step 2's output.
 *  4. Observation row i of a frame is track i of svo_get_last_tracks (RANSAC's row order): its id, the four points, world[i],
 *     inlier[i], and the age step 2 wrote (the feature's age after this frame's increment, vo.cpp:70-72).  On fail_reason 2 the
 *     frame did not triangulate: xyz is 0 0 0 and SVO_OBS_HAS_XYZ is clear.  SVO_OBS_INLIER is set only where the frame built
 *     its inlier vector (fail_reason 0 or 4).
 * A row whose id appeared in no earlier frame is a first sighting; l0 of a row whose id was in the previous frame's feature set is
 * that feature's position, bit for bit. */
typedef struct {            /* 64 bytes */
    int64_t id;             /* persistent within (context, sequence) since creation / the last svo_reset_sequence */
    float l0[2], r0[2];     /* the track at T0: left, right */
    float l1[2], r1[2];     /* the track at T1: left, right — this frame's stereo observation */
    float xyz[3];           /* world[i] of svo_get_last_tracks: triangulated from (l0, r0), in the T0 left camera frame; 0 0 0 when SVO_OBS_HAS_XYZ is clear */
    int32_t age;            /* the feature's age after this frame's increment */
    int32_t flags;          /* SVO_OBS_* */
    int32_t pad;
} svo_track_obs;
#define SVO_OBS_INLIER  1   /* inlier[i] of svo_get_last_tracks */
#define SVO_OBS_HAS_XYZ 2   /* the frame triangulated (fail_reason 0, 3 or 4) */
/* on != 0: switch the output on with room for max_rows rows per sequence and frame (1 .. the context's feature capacity: rows of
 * the default grid x columns, 14 080); the pinned ring [8][n_seq][max_rows] rows plus a {n_tracks, n_rows} header per (slot,
 * sequence) is allocated at first use and freed with the context.  The features a sequence holds at that moment get the ids
 * next_id + index and next_id advances by their count (stream-ordered).  on == 0: off again (max_rows is not looked at).
 * A setup action: SVO_ERR_STATE with frames in flight.  SVO_ERR_ARG: features_per_bucket > 1 (the general bucket walk carries no
 * ids), a bad max_rows.  While on, svo_get_last_frame_path reports SVO_PATH_TRACK_IDS, a lone stream issues the unfused front (as
 * a masked frame does), frames run from the launch list under SVO_GRAPH=1, and svo_circular_matching — which overwrites the
 * feature set behind the ids' back — returns SVO_ERR_STATE. */
int svo_set_track_output(svo_context* ctx, int on, int max_rows);
/* The rows of sequence seq in the last COLLECTED frame (svo_collect, svo_process*), from host memory: no device access, no
 * synchronisation.  *n_tracks (may be NULL) = the frame's full track count; returns min(n_tracks, max_rows, cap) = the rows
 * written, the first ones in track order.  An idle sequence, a first frame and an all-idle frame have n_tracks = 0.
 * SVO_ERR_STATE if that frame was issued with the output off or none was collected yet. */
int svo_get_last_track_obs(svo_context* ctx, int seq, int cap, svo_track_obs* rows, int* n_tracks);
/* Introspection: the ids of svo_get_features' entries, in its order; returns the count.  Synchronises like svo_get_features.
 * SVO_ERR_STATE with the output off. */
int svo_get_feature_ids(svo_context* ctx, int seq, int cap, int64_t* ids);

/* ---- Binary descriptors for the observation rows ------------------------------------------------------------------------------
 * What a landmark back end needs to recognise a place again (loop closure, relocalisation, map merging): an appearance descriptor
 * per landmark.  Off by default; off, a context launches exactly what it launched before.  On, every frame writes one 32-byte
 * descriptor per observation row into a second pinned ring: row i describes l1 of observation row i on that frame's LEFT image as
 * ingest left it (after format conversion, CLAHE and rectification: level 0 of the frame's pyramid).  Compare with the Hamming
 * distance.
 *
 * The descriptor is a steered BRIEF-256 in ORB's construction (intensity-centroid orientation, a rotated test pattern, comparisons
 * of smoothed pixels) with every step defined on integers: the rules below ARE the contract, and the kernel agrees with them in
 * every bit.  Parity with OpenCV's cv::ORB is UNPINNED and NOT CLAIMED: OpenCV was not available where this was written, and its
 * learned pattern table is not ours — a descriptor from here does not match one from cv::ORB, nor a vocabulary trained on them.
 *
 *  Centre.   cx = clamp((int)(x + 0.5f), 0, W - 1), cy likewise with H: the rounding of a detection mask's look-up (truncation
 *            toward zero, then the clamp).
 *  Patch.    P(dx, dy), dx, dy in [-15, 15] = the grey byte of the image at (cx + dx, cy + dy); a coordinate outside the image is
 *            reflected (REFLECT_101: -i for i < 0, 2 n - 2 - i for i >= n).  W, H >= 16 is required, so one reflection suffices.
 *  Orientation.  m10 = sum dx P, m01 = sum dy P over the disc dx^2 + dy^2 <= 240 (749 pixels): exact integers, |m| < 2^21.
 *            bin = the SMALLEST k in 0 .. 29 that maximises m10 C[k] + m01 S[k] (int64), with C = round(2^14 cos(12 k deg)),
 *            S = round(2^14 sin(12 k deg)) as literals:
 *              C[0..14] = 16384 16026 14968 13255 10963 8192 5063 1713 -1713 -5063 -8192 -10963 -13255 -14968 -16026, C[k+15] = -C[k]
 *              S[0..14] = 0 3406 6664 9630 12176 14189 15582 16294 16294 15582 14189 12176 9630 6664 3406,           S[k+15] = -S[k]
 *            The first maximum wins: m10 = 0, m01 > 0 ties bins 7 and 8 and gives 7; m10 = 0, m01 < 0 gives 22; a flat patch gives 0.
 *  Smoothing.  B(u, v) = sum of P over the 5 x 5 box centred at (u, v), |u|, |v| <= 13: an integer in 0 .. 6375.
 *  Pattern.  256 tests (ax, ay, bx, by), int8, ax^2 + ay^2 <= 169, bx^2 + by^2 <= 169, a != b: the library's own table
 *            (svo_descriptor_pattern), Gaussian point pairs with sigma = 31 / 5 written by tools/make_brief_pattern.py.
 *  Rotation of a point (px, py) by the bin:  rx = (px C[bin] - py S[bin] + 8192) >> 14,  ry = (px S[bin] + py C[bin] + 8192) >> 14
 *            (arithmetic shift).  For every integer point of norm <= 13 and every bin |rx|, |ry| <= 13: every box lies in the patch.
 *  Bits.     bit i = B(rot a_i) < B(rot b_i); bit i is bit i % 8 (LSB first) of byte i / 8.  A row is SVO_DESC_BYTES = 32 bytes.
 *
 * The bin is a 12-degree quantisation of the patch's intensity-centroid direction: it makes the descriptor follow in-plane rotation
 * in steps, it is not a scale or viewpoint normalisation, and two views whose direction falls on either side of a bin boundary
 * differ by one bin's rotation of the pattern. */
#define SVO_DESC_BYTES 32
#define SVO_PATH_DESCRIPTORS 8192 /* svo_get_last_frame_path: the frame wrote descriptor rows (k_track_desc); also set by svo_describe_points */
/* on != 0: frames submitted from now on write descriptor rows; the pinned ring [8][n_seq][max_rows][32] bytes (max_rows: the track
 * output's) is allocated at first use, re-allocated when svo_set_track_output changes max_rows, freed with the context.  A setup
 * action: SVO_ERR_STATE with frames in flight, or with the track output off — a descriptor row describes an observation row, and
 * svo_set_track_output(ctx, 0, ...) switches the descriptors off too.  SVO_ERR_ARG: a channels = 3 context, an image smaller than
 * 16 in either dimension.  While on, svo_get_last_frame_path reports SVO_PATH_DESCRIPTORS. */
int svo_set_descriptor_output(svo_context* ctx, int on);
/* The descriptor rows of sequence seq in the last COLLECTED frame, from host memory: no device access, no synchronisation.  desc:
 * cap rows of 32 bytes.  Returns the rows written = what svo_get_last_track_obs returns for that frame and cap; *n_tracks (may be
 * NULL) = the frame's full track count.  SVO_ERR_STATE if that frame was issued with descriptors off or none was collected yet. */
int svo_get_last_track_descriptors(svo_context* ctx, int seq, int cap, uint8_t* desc, int* n_tracks);
/* The library's tables: pattern[4 i .. 4 i + 3] = (ax, ay, bx, by) of test i; cs[0..29] = C, cs[30..59] = S.  Either may be NULL
 * (both NULL: SVO_ERR_ARG).  Needs no device. */
int svo_descriptor_pattern(int8_t pattern[1024], int32_t cs[60]);

/* ---- Descriptor index: exact 2-nearest-neighbour Hamming matching on the device -------------------------------------------------
 * What the descriptors are for: recognising a place again.  An index is an append-only array of rows (descriptor[32], id) in device
 * memory, 40 bytes per row, numbered from 0 in the order they were added.  A search is brute force and exact; it is defined on
 * integers, and the kernels agree with the definition below in every bit.
 *
 *  Distance.   d(q, r) = the popcount of the 256-bit XOR of query q and the descriptor of row r: 0 .. 256.
 *  Order.      key(q, r) = (d(q, r), r), compared lexicographically: the smaller distance wins, at equal distances the smaller row.
 *  Row range.  A search runs over the rows [row_lo, row_hi).  Rows arrive in time order, so a loop closer keeps the recent past out
 *              with row_hi.
 *  Best.       row = the row of the smallest key in the range.
 *  Second.     row2 = the row of the smallest key among the rows of the range whose id DIFFERS from id[row].  A landmark seen in k
 *              frames has k rows, all close to each other: a plain second-nearest row would nearly always be the same landmark
 *              again, and a ratio test (dist / dist2) would then reject every good match.
 *
 * What cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) is to an OpenCV user, except for the second neighbour's id rule.  PARITY
 * UNPINNED: which of several rows at one distance cv::BFMatcher returns was not measured (no OpenCV on the machines this was built
 * on); no equality with it is claimed, the order above is the contract.
 *
 * An index owns one non-blocking stream and its own pinned staging.  svo_desc_index_add and svo_desc_index_match are synchronous to
 * the caller and wait for that stream only — no device-wide synchronisation, nothing on a context's streams — so both are legal
 * while any context has frames in flight, and change no bit of what those frames return.  One index is used by one thread at a
 * time. */
typedef struct svo_desc_index svo_desc_index;
#define SVO_MATCH_NONE (-1)      /* row / row2: an empty range / no row with another id */
#define SVO_MATCH_NO_DIST 257    /* dist / dist2 where the row is SVO_MATCH_NONE: above every distance, so `dist * 10 < dist2 * 7` passes for a lone candidate */
typedef struct {                 /* 32 bytes */
    uint64_t id, id2;            /* id[row], id[row2]; 0 where the row is SVO_MATCH_NONE */
    int32_t  row, row2;          /* SVO_MATCH_NONE: an empty range / no row with another id */
    uint16_t dist, dist2;        /* 0 .. 256; SVO_MATCH_NO_DIST with SVO_MATCH_NONE */
    uint32_t reserved;           /* 0 */
} svo_desc_match;
/* An empty index with room for capacity rows on `device`: 1 <= capacity <= 1 << 24 (a row number takes 24 bits of a search's packed
 * key), else SVO_ERR_ARG.  40 bytes of device memory per row, allocated here. */
int svo_desc_index_create(int device, int capacity, svo_desc_index** out);
void svo_desc_index_destroy(svo_desc_index* index);
/* Append n rows from host memory: desc n x 32 bytes, ids n values.  All n or none: size + n > capacity is SVO_ERR_ARG and adds
 * nothing.  *first_row (may be NULL) = the row number of the first one.  n = 0 is legal. */
int svo_desc_index_add(svo_desc_index* index, int n, const uint8_t* desc, const uint64_t* ids, int* first_row);
/* Append, in row order, the observation + descriptor rows of sequence seq of ctx's last COLLECTED frame whose flags contain every
 * bit of need_flags (SVO_OBS_INLIER: the frame's inliers; 0: every row), read from the two pinned rings; the id of a row is its
 * svo_track_obs id.  *first_row, *n_added may be NULL.  SVO_ERR_STATE exactly where svo_get_last_track_descriptors gives it;
 * SVO_ERR_ARG as svo_desc_index_add's (nothing added) and for a bad ctx / seq. */
int svo_desc_index_add_frame(svo_desc_index* index, svo_context* ctx, int seq, uint32_t need_flags, int* first_row, int* n_added);
int svo_desc_index_size(const svo_desc_index* index);
/* Keep the first n_rows rows (0 clears the index); rows added afterwards take their numbers.  n_rows > size or < 0: SVO_ERR_ARG. */
int svo_desc_index_truncate(svo_desc_index* index, int n_rows);
/* The best and second-best row of [row_lo, row_hi) for each of n queries (host, n x 32 bytes) into out (host, n rows).
 * row_hi = -1: the index's size.  n = 0 and row_lo == row_hi (every row of out is then SVO_MATCH_NONE) are legal.
 * SVO_ERR_ARG: row_lo < 0, row_hi > size, row_lo > row_hi. */
int svo_desc_index_match(svo_desc_index* index, int n, const uint8_t* query, int row_lo, int row_hi, svo_desc_match* out);
/* Tuning: the rows of the index one block of the search walks (0 = the default, 1024).  The search cuts the range at the multiples
 * of this number and keeps a 16-byte partial result per (query, piece) in a device scratch owned by the index.  The scratch starts
 * at 64 KiB and at least doubles whenever a search needs more, so an index that grows frame by frame re-allocates O(log size)
 * times; a search of up to 65 536 pieces needs 64 MiB of it at most (more pieces mean fewer queries per launch, 64 at least).
 * Outgrown buffers are freed with the index — freeing device memory waits for the whole device — and sum to less than the buffer
 * in use: below 128 MiB in all up to 65 536 pieces.  The results do not depend on this number.  SVO_ERR_ARG: rows < 0 or > 1 << 24. */
int svo_desc_index_set_chunk_rows(svo_desc_index* index, int rows);
int svo_desc_index_get_chunk_rows(const svo_desc_index* index);
/* Diagnostics, for tools/desc_match_bench.py and the tests; nothing a search returns depends on them.  svo_desc_index_set_timing:
 * on != 0 records two HIP events around the kernels of every later svo_desc_index_match and reads their time after the call's
 * synchronisation; off (the default) a search records nothing.  svo_desc_index_get_stats: the device time of the last search's
 * kernels in milliseconds (summed over its launches, the copies not in it; 0 with timing off or when nothing was launched), how
 * often the scratch was allocated, its size, and the bytes of the buffers it has outgrown.  After svo_desc_index_select or
 * svo_desc_index_localize with timing on, last_kernels_ms is the device time of the selection kernel alone.  After a guided call
 * ("Guided search") with timing on it is the device time of the projection kernel plus the guided search kernels (after
 * svo_desc_index_project: the projection kernel alone).  After svo_desc_index_tag_votes, svo_desc_index_places or
 * svo_desc_index_places_from_ids ("Place candidates") with timing on it is the device span of the new kernels alone — the clearing
 * of the bins, the sweep and, for the two places calls, the compaction and the pick — not the search and the selection in front. */
typedef struct {
    float    last_kernels_ms;
    int32_t  scratch_allocations;
    uint64_t scratch_bytes, scratch_bytes_outgrown;
} svo_desc_index_stats;
int svo_desc_index_set_timing(svo_desc_index* index, int on);
int svo_desc_index_get_stats(const svo_desc_index* index, svo_desc_index_stats* stats);

/* ---- Relocalisation: where is this camera in the map? ----------------------------------------------------------------------------
 * An index may carry a 3-D point per row: the landmark in the caller's map frame.  One call then takes a frame's (descriptor, pixel)
 * pairs, searches, selects a consistent candidate set on the device and runs the RANSAC-PnP of svo_camera_to_world on it: one host
 * synchronisation, no host round trip between the search and the pose.  Like add and match, every call here waits for the index's
 * own stream only and is legal with frames in flight.
 *
 * The selection is defined on integers.  Per query j (0 .. n - 1) let m_j be its search result over [row_lo, row_hi)
 * (svo_desc_index_match's row j), and tag[r] the tag of row r's point:
 *  1. Accept.      j is accepted when m_j.row != SVO_MATCH_NONE, tag[m_j.row] != SVO_POINT_NONE, m_j.dist <= max_dist and
 *                  m_j.dist * ratio_den < m_j.dist2 * ratio_num — strictly; dist2 = SVO_MATCH_NO_DIST (257) of a lone candidate passes.
 *  2. One pixel per landmark.  Among the accepted queries with the same m_j.id only the smallest (m_j.dist, j) survives.
 *  3. Candidates.  The survivors in increasing j: candidate c carries (query j, row m_j.row, pixel xy[j], point xyz[m_j.row]).
 *  4. Gate.        n_candidates < min_candidates: success = 0, the PnP does nothing and iters_run = 0. */
#define SVO_POINT_NONE (-1)      /* the tag of an index row without a point */
#define SVO_RELOC_MAX_QUERIES 4096
typedef struct {
    int32_t row_lo, row_hi;      /* the rows searched, as svo_desc_index_match's (row_hi = -1: the index's size) */
    int32_t max_dist;            /* rule 1: 0 .. 256 */
    int32_t ratio_num, ratio_den; /* rule 1: 1 .. 1 << 20 each */
    int32_t min_candidates;      /* rule 4: >= 6 (with 4 or 5 points svo_camera_to_world takes direct routes chosen on the host) */
    int32_t ransac_iterations;   /* these three as svo_camera_to_world's */
    float   reproj_error, confidence;
} svo_reloc_params;
typedef struct {
    int32_t success, n_candidates, n_inliers, iters_run;
    double  R[9], t[3];          /* in: the extrinsic guess; out: the pose on success (untouched otherwise): x_cam = R X_map + t */
    double  T[16];               /* out, on success: the inverse, the camera in the map (row-major 4 x 4); zeros otherwise */
} svo_reloc_result;
/* max_dist = 40, ratio 7 / 10, min_candidates = 6, the whole index; iterations, error and confidence from svo_config_default */
void svo_reloc_params_default(svo_reloc_params* params);
/* Give the index's rows points: capacity x 16 bytes of device memory, a row being {float x, y, z; int32_t tag}.  Legal only while
 * the index is empty (SVO_ERR_STATE otherwise); enabling twice is legal.  svo_desc_index_add on such an index writes SVO_POINT_NONE
 * rows; svo_desc_index_truncate drops the points with their rows. */
int svo_desc_index_enable_points(svo_desc_index* index);
/* svo_desc_index_add with a point per row: xyz n x 3 floats in the map frame, tags n values >= 0 (NULL: all 0; a frame number is
 * the intended use).  All n rows or none.  SVO_ERR_STATE: an index without points.  SVO_ERR_ARG: a negative tag, a non-finite
 * coordinate, and svo_desc_index_add's. */
int svo_desc_index_add_points(svo_desc_index* index, int n, const uint8_t* desc, const uint64_t* ids, const float* xyz,
                              const int32_t* tags, int* first_row);
/* svo_desc_index_add_frame with SVO_OBS_HAS_XYZ always required, and each row's point moved into the map.  An observation row's xyz
 * is in the T0 left camera frame — the frame BEFORE the one just collected (svo_track_obs) — so cam_to_map (16 doubles, row-major
 * 4 x 4; NULL: the identity) is the pose of the PREVIOUS frame's left camera in the map, not the pose svo_collect has just returned.
 * Per coordinate r the stored value is f32(T[4r] x + T[4r+1] y + T[4r+2] z + T[4r+3]), evaluated in f64 from left to right
 * without contraction.  SVO_ERR_STATE: an index without points; SVO_ERR_ARG: a negative tag, a non-finite entry of cam_to_map or
 * result. */
int svo_desc_index_add_frame_points(svo_desc_index* index, svo_context* ctx, int seq, uint32_t need_flags, const double* cam_to_map,
                                    int32_t tag, int* first_row, int* n_added);
/* The selection alone: rules 1 - 3 for n <= SVO_RELOC_MAX_QUERIES queries (host: query n x 32 bytes, xy n x 2 floats; xy may be NULL
 * when cand_xy is) -> *n_candidates and, where non-NULL, per candidate its query, its row, its pixel (2 floats) and its point
 * (3 floats), each with room for n entries — the arrays the PnP of svo_desc_index_localize reads.  ransac_* and min_candidates > n
 * play no part.  SVO_ERR_STATE: an index without points.  SVO_ERR_ARG: n > 4096, a bad row range, max_dist outside 0 .. 256, a ratio
 * term outside 1 .. 1 << 20, min_candidates < 6. */
int svo_desc_index_select(svo_desc_index* index, int n, const uint8_t* query, const float* xy, const svo_reloc_params* params,
                          int* n_candidates, int32_t* cand_query, int32_t* cand_row, float* cand_xy, float* cand_xyz);
/* Search, select, RANSAC-PnP.  K: the 3 x 3 camera matrix; result->R, t: the guess going in.  cand_query, cand_row, cand_inlier
 * (each n entries, each may be NULL): per candidate its query, its row and whether the PnP kept it (1 / 0).  For the candidate
 * arrays svo_desc_index_select returns, success, R, t, the inlier set and iters_run equal svo_camera_to_world's on those arrays
 * with the same guess and parameters in every bit: the same kernels on the same inputs.  Errors as svo_desc_index_select's. */
int svo_desc_index_localize(svo_desc_index* index, const float K[9], int n, const uint8_t* query, const float* xy,
                            const svo_reloc_params* params, svo_reloc_result* result, int32_t* cand_query, int32_t* cand_row,
                            uint8_t* cand_inlier);

/* ---- Guided search: search only where a pose prior projects ---------------------------------------------------------------------
 * A camera that tracks in a map knows roughly where it is: the last map pose composed with the frame's odometry, or a loop closer's
 * hypothesis.  The calls below project the index's points with that prior and match each query only against the rows that land near
 * its pixel (what ORB-SLAM's SearchByProjection does).  The search is cheaper, and in repeated structure — two landmarks that look
 * alike — dist2 becomes the nearest OTHER landmark that could be at this pixel, so the ratio test of "Relocalisation" works where the
 * unguided one rejects every correct match.  A second family beside the unguided calls, which are unchanged.
 *
 * A guide is a pose prior x_cam = R X_map + t (the convention of svo_reloc_result) and a radius in pixels.  K is the call's 3 x 3
 * camera matrix; the projection uses K[0], K[2], K[4] and K[5] only (fx, cx, fy, cy), widened to f64.  The PnP still gets all of K.
 *  1. Projection of row r with point (x, y, z) and tag, in f64, every product, quotient and sum rounded on its own (no contraction),
 *     left to right as in svo_desc_index_add_frame_points:
 *       Xc = ((R0 x + R1 y) + R2 z) + t0,   Yc likewise with R3, R4, R5, t1,   Zc with R6, R7, R8, t2;
 *       u = f32(fx (Xc / Zc) + cx),   v = f32(fy (Yc / Zc) + cy).
 *     The row is VISIBLE when its tag is not SVO_POINT_NONE, Zc > 0 strictly, and u and v are both finite after the rounding to f32.
 *     An invisible row's projection is (+inf, +inf).
 *  2. Gate.  Row r is ADMISSIBLE for query j with pixel (x_j, y_j) when |u_r - x_j| <= radius and |v_r - y_j| <= radius; the
 *     subtractions, absolute values and comparisons are f32 and both limits are inclusive.  An invisible row is admissible for
 *     nobody; a query with a non-finite pixel admits nothing (inf - inf is NaN and the comparison fails).
 *  3. Search.  svo_desc_index_match's definition over the admissible rows of [row_lo, row_hi) only: best by (dist, row), second =
 *     the best admissible row of another id.  No admissible row: SVO_MATCH_NONE and SVO_MATCH_NO_DIST, as for an empty range.
 *  4. Selection and PnP.  Rules 1 - 4 of "Relocalisation", unchanged, on those result rows.
 * The results do not depend on the chunk size, on the order in which the library visits the queries, or on anything else internal.
 *
 * Every call is synchronous, waits for the index's own stream only, is legal with frames in flight and synchronises once.  The
 * projection runs on every call — nothing is cached between calls — into a device array of capacity x 8 bytes that the index
 * allocates at its first guided call and frees with the index (with 32 KiB for the queries' order, below).  A guided search is one
 * launch over all its queries: where queries x pieces would exceed the scratch's 64 MiB budget (svo_desc_index_set_chunk_rows) the
 * rows of a piece double until it fits.
 * SVO_ERR_ARG: radius negative or not finite; a non-finite entry of R, t or K; n > SVO_RELOC_MAX_QUERIES (the guided match too: it
 * shares the 4096-row pixel staging); a NULL K or guide; and the refusals of the unguided call of the same name.  SVO_ERR_STATE: an
 * index without points. */
typedef struct {
    double  R[9], t[3];          /* the prior: x_cam = R X_map + t */
    float   radius;              /* rule 2, in pixels: finite, >= 0 */
    int32_t reserved;            /* 0 */
} svo_reloc_guide;
/* Rule 1 alone, the stage on its own (as svo_describe_points is for the descriptors): uv (host) receives (row_hi - row_lo) x 2
 * floats, the projections of rows [row_lo, row_hi); row_hi = -1: the index's size.  The radius is checked and not used. */
int svo_desc_index_project(svo_desc_index* index, const float K[9], const svo_reloc_guide* guide, int row_lo, int row_hi, float* uv);
/* Rules 1 - 3: svo_desc_index_match with a pixel per query (xy: n x 2 floats) and the gate.  n <= SVO_RELOC_MAX_QUERIES. */
int svo_desc_index_match_guided(svo_desc_index* index, const float K[9], const svo_reloc_guide* guide, int n, const uint8_t* query,
                                const float* xy, int row_lo, int row_hi, svo_desc_match* out);
/* svo_desc_index_select and svo_desc_index_localize over the guided search; xy is required.  result->R, t going in remain the PnP's
 * extrinsic guess and are not tied to the guide — passing the guide's R, t is the usual choice.  For the arrays
 * svo_desc_index_select_guided returns, svo_desc_index_localize_guided equals svo_camera_to_world in every bit, as
 * svo_desc_index_localize does for svo_desc_index_select's. */
int svo_desc_index_select_guided(svo_desc_index* index, const float K[9], const svo_reloc_guide* guide, int n, const uint8_t* query,
                                 const float* xy, const svo_reloc_params* params, int* n_candidates, int32_t* cand_query,
                                 int32_t* cand_row, float* cand_xy, float* cand_xyz);
int svo_desc_index_localize_guided(svo_desc_index* index, const float K[9], const svo_reloc_guide* guide, int n, const uint8_t* query,
                                   const float* xy, const svo_reloc_params* params, svo_reloc_result* result, int32_t* cand_query,
                                   int32_t* cand_row, uint8_t* cand_inlier);
/* Tuning and diagnostics.  A wave of the guided search serves 64 queries and skips a row that none of them admits, which pays when
 * the 64 sit close together in the image: the library sorts a call's queries by image cell (side 2 x radius, cells in raster order,
 * ties by j) and lets lane `slot` serve the slot-th query of that order; everything it returns is under the queries' own numbers.
 * on = 0 serves the queries in the caller's order instead (default: on).  The results do not depend on it. */
int svo_desc_index_set_guided_sort(svo_desc_index* index, int on);

/* ---- Index maintenance: retire rows and move points on the device ---------------------------------------------------------------
 * A map forgets and is corrected.  svo_desc_index_retire drops rows anywhere in the index and closes the gaps in place;
 * svo_desc_index_transform_points moves the points of a span of rows through a 4 x 4 transform (a loop closure's correction, a
 * merged map's alignment).  Both run on the device, are synchronous, wait for the index's own stream only and are legal with frames
 * in flight; a refused call changes nothing.
 *
 * The retire rule.  Let n0 be the size before the call and S = [row_lo, row_hi) the scope (row_hi = -1: n0).
 *   alive1(r):  r in S, SVO_RETIRE_SCOPE is clear, with SVO_RETIRE_BY_TAG tag_lo <= tag[r] <= tag_hi (plain int32 compares; a row
 *               without a point has the tag SVO_POINT_NONE = -1), and with SVO_RETIRE_BY_IDS id[r] is not among ids[0 .. n_ids).
 *   keep(r):    r is not in S; or alive1(r) and — with SVO_RETIRE_LATEST_PER_ID — there is no r' > r with alive1(r') and
 *               id[r'] == id[r].  "Latest" is decided among the scope's survivors of the other rules only.
 *   kept_before[r] = #{r' < r : keep(r')} for r = 0 .. n0; the new size is kept_before[n0].
 * A kept row r becomes row kept_before[r]: its descriptor, its id and (where the index has points) its point are carried bit for
 * bit, and the order of the rows is preserved.  kept_before is the whole remapping: a stored row number or frame boundary f becomes
 * kept_before[f], and row r was kept iff kept_before[r + 1] > kept_before[r].  flags == 0 keeps everything and is legal; a window
 * with tag_lo > tag_hi drops the scope, as SVO_RETIRE_SCOPE does (one frame's rows: [first_row[k], first_row[k + 1])).
 * SVO_ERR_STATE: SVO_RETIRE_BY_TAG on an index without points.  SVO_ERR_ARG: unknown flag bits; a scope that svo_desc_index_match
 * refuses as a row range; n_ids < 0 or > 1 << 24; SVO_RETIRE_BY_IDS with ids == NULL and n_ids > 0.  SVO_ERR_INTERNAL: the
 * latest-per-id table overflowed, which its size rules out; nothing was changed.
 *
 * The transform rule.  Row r is selected when r is in [row_lo, row_hi) and tag_lo <= tag[r] <= tag_hi with tag[r] != SVO_POINT_NONE.
 * Coordinate c (0, 1, 2) of a selected row's point (x, y, z) becomes f32(((T[4c] x + T[4c+1] y) + T[4c+2] z) + T[4c+3]), evaluated
 * in f64, every operation rounded on its own, left to right, without contraction: svo_desc_index_add_frame_points' formula.  A
 * selected row whose result has a non-finite coordinate is left as it is and counted in *n_skipped — the index never holds a
 * non-finite point; the other selected rows are counted in *n_moved (either may be NULL).  Tags, ids and descriptors are untouched.
 * SVO_ERR_ARG: a non-finite entry of T, a bad row range.  SVO_ERR_STATE: an index without points.
 *
 * Memory.  There is no second copy of the index.  A retire call works in a scratch the index owns; with m the scope's rows,
 * R(b) = b rounded up to a multiple of 256 and slots(m) the smallest power of two >= max(2, 2 m), a call needs
 *   need = R(m) + R(4 (m + 1)) + R(4 (ceil(m / 256) + 257)) + [LATEST_PER_ID: R(4 slots(m))] + [BY_IDS: R(8 n_ids)]
 *          + R(56 min(retire_slab_rows, n0 - row_lo))
 * bytes: the keep flags, the ranks, the block counts, the latest-per-id table, the sorted id list and the bounce buffer through
 * which one slab of rows moves (rows are compacted slab after slab in row order, so nothing is read after it could have been
 * overwritten).  The scratch is 64 KiB times a power of two, the smallest that holds the largest call so far: at most
 * max(65 536, 2 need - 1) bytes.  It at least doubles when it grows, so an index retired again and again as it grows allocates
 * O(log size) times; outgrown buffers are freed with the index and sum to less than the one in use.  flags == 0 and an empty scope
 * need nothing.  kept_before reaches the host in pieces through the index's pinned staging, and only when it is asked for. */
#define SVO_RETIRE_BY_TAG        1   /* drop rows of the scope whose tag is outside [tag_lo, tag_hi] */
#define SVO_RETIRE_BY_IDS        2   /* drop rows of the scope whose id is in ids[0 .. n_ids) */
#define SVO_RETIRE_LATEST_PER_ID 4   /* of the rows of the scope that survive the two rules above, keep per id only the newest */
#define SVO_RETIRE_SCOPE         8   /* drop every row of the scope */
typedef struct {
    uint32_t flags;                  /* SVO_RETIRE_* bits */
    int32_t  row_lo, row_hi;         /* the scope [row_lo, row_hi), row_hi = -1: the size; rows outside it are kept */
    int32_t  tag_lo, tag_hi;         /* SVO_RETIRE_BY_TAG: inclusive */
    int32_t  n_ids;                  /* 0 .. 1 << 24 */
    const uint64_t* ids;             /* SVO_RETIRE_BY_IDS: host memory, any order, duplicates allowed */
} svo_retire_rule;
typedef struct {
    float    last_kernels_ms;        /* the device time of the last retire's or transform's kernels (svo_desc_index_set_timing on; else 0) */
    int32_t  scratch_allocations;    /* how often the retire scratch was allocated */
    uint64_t scratch_bytes, scratch_bytes_outgrown;
} svo_desc_retire_stats;
/* kept_before: size-before-the-call + 1 entries, or NULL; *n_kept (may be NULL): the new size */
int svo_desc_index_retire(svo_desc_index* index, const svo_retire_rule* rule, int32_t* kept_before, int* n_kept);
/* T: 16 doubles, row-major 4 x 4; row_hi = -1: the index's size */
int svo_desc_index_transform_points(svo_desc_index* index, const double T[16], int row_lo, int row_hi, int32_t tag_lo, int32_t tag_hi,
                                    int* n_moved, int* n_skipped);
/* Tuning: the rows of one slab of retire's compaction (0 = the default, 262 144: a bounce buffer of 14 MiB at most).  The results
 * do not depend on it.  SVO_ERR_ARG: rows < 0 or > 1 << 24. */
int svo_desc_index_set_retire_slab_rows(svo_desc_index* index, int rows);
int svo_desc_index_get_retire_slab_rows(const svo_desc_index* index);
int svo_desc_index_get_retire_stats(const svo_desc_index* index, svo_desc_retire_stats* stats);

/* ---- Batched relocalisation: many cameras against one index in one call ------------------------------------------------------------
 * A many-sequence context tracks hundreds of cameras per step; the calls above serve one camera each, and most of such a call is
 * launch latency.  svo_desc_index_localize_batch serves n_cameras cameras in one call: one upload, the searches of all cameras in a
 * few launches, one selection launch with a block per camera, the RANSAC-PnP kernels over n_cameras sequences, one host
 * synchronisation.
 *
 * The contract, which is the whole definition.  Camera b has the queries [query_begin[b], query_begin[b + 1]) of query and xy, the
 * camera matrix K + 9 b, the guide guides[b], and results[b].R, t going in as its extrinsic guess.
 *  - results[b] equals, in every bit, what svo_desc_index_localize_guided returns for that slice alone with the same params; with
 *    guides == NULL, what svo_desc_index_localize returns.
 *  - The first results[b].n_candidates entries of cand_query, cand_row and cand_inlier (each may be NULL) at offset query_begin[b]
 *    equal that single call's arrays; cand_query is numbered inside the slice, 0 .. n_b - 1.  Nothing beyond those entries is written.
 *  - The results do not depend on the chunk size, on the order of the lanes, on how the library groups cameras into launches, or on
 *    the number of cameras.
 * A camera has at most SVO_RELOC_MAX_QUERIES queries, a call 0 .. SVO_RELOC_BATCH_MAX_CAMERAS cameras (0 is legal and launches
 * nothing) and at most SVO_RELOC_BATCH_MAX_QUERIES queries in all.  A camera without queries gets success = 0, n_candidates = 0.
 * params is one record for the call; guided and unguided cameras do not mix.
 * SVO_ERR_ARG / SVO_ERR_STATE: wherever the single call gives them for any camera; also query_begin[0] != 0, a decreasing offset, a
 * slice above 4096, a total above 1 << 20, n_cameras outside 0 .. 1024.  Every refusal is decided before anything is uploaded or
 * enqueued and leaves results untouched.
 * The call synchronises once, waits for the index's own stream only, and is legal with frames in flight; one index is used by one
 * thread at a time.  With svo_desc_index_set_timing on, last_kernels_ms is the device span from the first kernel the call launches
 * to the last.
 *
 * How it runs (none of it shows in the results).  The guided search projects inside the search kernel, tile by tile into LDS: no
 * array of projections exists (cameras x rows x 8 bytes would be 4 GiB at 512 cameras and 1 << 20 rows).  Partial states are kept
 * per (query, piece), so a launch serves a group of consecutive cameras whose queries x pieces fit the scratch's 64 MiB budget; the
 * rows of a piece double from svo_desc_index_set_chunk_rows' number until the widest slice (64 queries at least) fits alone.  With
 * svo_desc_index_set_guided_sort on, each camera's lanes are ordered on the device by image cell (side 2 x radius, 1 px at least,
 * raster order, a non-finite pixel last; ties by j); off, and without guides, the lanes take the queries as they come.
 * The PnP runs in a stage context of its own that the index owns: n_cameras sequences, configured as svo_camera_to_world's.  Above 8
 * cameras the PnP kernels take their many-sequence builds, which give the lone builds' bits.
 *
 * Memory, all owned by the index, allocated at the first batch call and freed with the index.  With C cameras, Q queries in all and
 * R(b) = b rounded up to a multiple of 256, a call needs a device staging of
 *   R(32 Q) + R(8 Q) + R(4 (C + 1)) + R(136 C)         the queries, their pixels, the offsets, the cameras' priors (one copy up)
 *   + R(4 C) + 2 R(4 Q) + R(Q)                         the candidate counts, the two candidate lists, the inlier flags (one copy down)
 *   + R(4 Q) + R(32 Q)                                 the lane order and the search's result rows
 * bytes, a pinned staging of the first two lines, and 2 C pinned state rows.  The staging is separate from the 4096-row staging of
 * the single calls.  Its capacities in cameras (16 at first) and queries (4096 at first) each at least double when a call outgrows
 * them; outgrown blocks, and outgrown stage contexts (sequences and points per sequence at least double likewise), are freed with
 * the index and sum to less than the ones in use. */
#define SVO_RELOC_BATCH_MAX_CAMERAS 1024
#define SVO_RELOC_BATCH_MAX_QUERIES (1 << 20)
int svo_desc_index_localize_batch(svo_desc_index* index, int n_cameras,
                                  const float* K,                  /* n_cameras x 9 */
                                  const svo_reloc_guide* guides,   /* n_cameras, or NULL: the unguided search for every camera */
                                  const int32_t* query_begin,      /* n_cameras + 1 offsets into query / xy: [0] = 0, non-decreasing */
                                  const uint8_t* query, const float* xy,   /* total x 32 bytes, total x 2 floats */
                                  const svo_reloc_params* params,  /* one for the call */
                                  svo_reloc_result* results,       /* n_cameras; R, t going in: each camera's extrinsic guess */
                                  int32_t* cand_query, int32_t* cand_row, uint8_t* cand_inlier);   /* total entries each, each may be NULL */
/* Diagnostic: the lane order of the last batch call as global query numbers — entries [query_begin[b], query_begin[b + 1]) are a
 * permutation of camera b's slice; the identity where the order kernel did not run.  *n: the call's total; order receives
 * min(cap, *n) entries.  SVO_ERR_STATE: no batch call yet, or the staging has grown since. */
int svo_desc_index_get_batch_order(const svo_desc_index* index, int cap, int32_t* order, int* n);

/* ---- Batched insertion: many sequences' frames into the index in one call -----------------------------------------------------------
 * svo_desc_index_add_frame serves one sequence per call and runs on the host: it copies the rows out of the pinned rings, packs
 * them, transforms the points, and pays three uploads and a synchronisation.  A many-sequence context that builds one map pays that
 * once per sequence and step.  svo_desc_index_add_frames appends the selected rows of n entries — sequences of ctx's last COLLECTED
 * frame — in one call: the filter, the order-preserving compaction, the f64 point transform and the id offset run on the device,
 * which reads the rows where the frame's kernels left them, in the host-mapped rings; one host synchronisation per call.
 *
 * The rules.
 *  1. Entries.  Entry b is sequence seqs[b]; seqs == NULL: entry b is sequence b.  Duplicates are legal (they are what a loop of
 *     single calls would do).  1 <= n <= SVO_INSERT_MAX_ENTRIES; svo_desc_index_add_obs also takes n = 0 and adds nothing.  An entry
 *     whose sequence has no rows in the last collected frame — a first frame, a sequence idle under the mask: n_tracks = 0, as
 *     svo_get_last_track_obs reports — contributes none.
 *  2. Keep.  Row i of entry b is kept iff (flags & need) == need; need = need_flags for the plain call, need_flags | SVO_OBS_HAS_XYZ
 *     with points.
 *  3. Order.  Kept rows are appended in entry order, and inside an entry in row order.  n_added[b] is entry b's kept count,
 *     first_row[b] the size before the call plus the counts of the entries before b.  The rows of a sequence are scanned up to the
 *     stored-row count of its header, min(n_tracks, max_rows), as the single call scans them.
 *  4. Id.  id = (uint64_t)obs.id + id_base[b] modulo 2^64; id_base == NULL: all zero.  Two sequences' track ids both start at 0:
 *     id_base (say seq << 48) keeps them apart in one index.  The single calls keep their rule, id = obs.id.
 *  5. Point and tag.  Per coordinate the arithmetic of svo_desc_index_add_frame_points — f64, left to right, no contraction,
 *     rounded to f32 — through cam_to_map + 16 b; cam_to_map == NULL stores xyz as it is.  The tag is tags[b] >= 0 (tags == NULL:
 *     all zero).  On an index with points the plain call writes SVO_POINT_NONE rows, as svo_desc_index_add does.
 *  6. All or nothing.  SVO_ERR_ARG, size unchanged and every row below size untouched when the kept rows exceed capacity - size, a
 *     cam_to_map entry is not finite, a tag is negative, or a kept row's point is not finite.  (Rows beyond size are never read; the
 *     kernels may have written there.)  size moves once, after the synchronisation.
 *  7. Refusals otherwise: the single calls', for any entry — a null index or context, a sequence outside the context, SVO_ERR_STATE
 *     where svo_get_last_track_descriptors gives it and for the points call on an index without points — all decided before anything
 *     is launched.
 *  8. The contract is the definition.  With id_base zero, the index after the call, first_row and n_added equal, in every bit, those
 *     of the loop of svo_desc_index_add_frame[_points] over the entries.
 * first_row and n_added (n entries each) may be NULL.  The calls are synchronous, wait for the index's own stream only, are legal
 * with frames in flight and change no bit of what those frames return.
 *
 * svo_desc_index_add_obs is the same stage on the caller's own rows in host memory: entry b has the rows [row_begin[b],
 * row_begin[b + 1]) of obs and desc (row_begin[0] = 0, non-decreasing, at most 1 << 18 rows in all); with_points != 0 is the points
 * call (cam_to_map, tags as above), 0 the plain call (both ignored).
 *
 * How it runs (none of it shows in the results).  SVO_INSERT_PATH_RING: the rows are still in their slot of the rings and index and
 * context are on one device: the kernels read the rings in place over the host link — 4 bytes of every row's flags, then the id, the
 * point and the descriptor of the kept rows only.  SVO_INSERT_PATH_STAGED: the rows are in the context's kept copies (eight frames
 * were submitted since the collect) or on another device, or are the caller's (add_obs): they go up through a pinned staging in
 * groups of whole entries of at most 1 << 18 rows (96 bytes a row: under 24 MiB; it starts at 64 KiB and doubles), one
 * synchronisation per group, the same kernels.  The working memory is the maintenance scratch ("Index maintenance").
 * svo_desc_index_get_insert_stats: the last call's path, the rows it scanned and added, and with svo_desc_index_set_timing on the
 * device span of its kernels (summed over a staged call's groups; the copies are not in it). */
#define SVO_INSERT_MAX_ENTRIES 1024
#define SVO_INSERT_MAX_OBS_ROWS (1 << 18)
#define SVO_INSERT_PATH_NONE   0   /* no batched insertion yet */
#define SVO_INSERT_PATH_RING   1
#define SVO_INSERT_PATH_STAGED 2
typedef struct {
    float    last_kernels_ms;
    int32_t  last_path;          /* SVO_INSERT_PATH_* */
    uint64_t rows_scanned, rows_added;
} svo_desc_insert_stats;
int svo_desc_index_add_frames(svo_desc_index* index, svo_context* ctx, int n, const int32_t* seqs, uint32_t need_flags,
                              const uint64_t* id_base, int32_t* first_row, int32_t* n_added);
int svo_desc_index_add_frames_points(svo_desc_index* index, svo_context* ctx, int n, const int32_t* seqs, uint32_t need_flags,
                                     const uint64_t* id_base, const double* cam_to_map /* n x 16 or NULL */,
                                     const int32_t* tags /* n or NULL */, int32_t* first_row, int32_t* n_added);
int svo_desc_index_add_obs(svo_desc_index* index, int n, const int32_t* row_begin /* n + 1 */, const svo_track_obs* obs,
                           const uint8_t* desc, uint32_t need_flags, const uint64_t* id_base, int with_points,
                           const double* cam_to_map, const int32_t* tags, int32_t* first_row, int32_t* n_added);
int svo_desc_index_get_insert_stats(const svo_desc_index* index, svo_desc_insert_stats* stats);

/* ---- Map alignment: the rigid transform between two row spans of the index ----------------------------------------------------------
 * Merging a second sequence's map, and closing a loop, need the transform between two sets of landmarks that are already in the
 * index: a 3-D to 3-D alignment, not a PnP from one image's pixels.  svo_desc_index_align searches the descriptors of a SOURCE span
 * S = [src_lo, src_hi) in a DESTINATION span D = [dst_lo, dst_hi), pairs rows up, and fits x_dst = R x_src + t by RANSAC and refit,
 * all on the device: no descriptor leaves it, one host synchronisation.  The result's T goes straight into
 * svo_desc_index_transform_points(index, T, src_lo, src_hi, ...).  Only SE(3): stereo maps are metric.  Sim(3) (a scale) is not offered.
 *
 * Both spans follow the row_hi = -1 convention.  S has n = src_hi - src_lo <= SVO_ALIGN_MAX_ROWS rows, and S and D share no row
 * (spans that touch are legal; an empty span shares nothing).  Rules 1 - 5 are defined on integers.  tag[r], id[r], xyz[r]: row r's.
 *  1. Search.  For j = 0 .. n - 1, m_j is svo_desc_index_match's result row for the query "descriptor of row src_lo + j" over D,
 *     equal in every bit: the same kernels read the query from the index itself.
 *  2. Accept.  j is accepted when tag[src_lo + j] != SVO_POINT_NONE and rule 1 of "Relocalisation" holds for m_j: a row with a
 *     point, dist <= max_dist, dist * ratio_den < dist2 * ratio_num strictly (257 passes).
 *  3. One source row per destination landmark.  Among the accepted j with the same m_j.id only the smallest (m_j.dist, j) survives
 *     (rule 2 of "Relocalisation").
 *  4. One destination per source landmark.  Among the survivors of rule 3 with the same id[src_lo + j] only the smallest
 *     (m_j.dist, j) survives: a landmark seen in k frames has k source rows and would otherwise vote k times.
 *  5. Pairs.  The survivors in increasing j: pair c is (src row src_lo + j, dst row m_j.row, p_c = xyz[src row], q_c = xyz[dst row]).
 *     n_pairs < min_pairs: success = 0, nothing further runs, every other field of the result is 0 and best_hypothesis is -1.
 *  6. Hypotheses.  H = hypotheses, 1 .. SVO_ALIGN_MAX_HYPOTHESES, all evaluated: there is no adaptive stop.  Hypothesis h (0 .. H - 1)
 *     draws three distinct pair numbers with a counter-based generator: draw k = 0, 1, .. is
 *         (mix64((uint64_t)h << 32 | k) >> 32) % n_pairs,
 *     mix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
 *     (splitmix64's finaliser, modulo 2^64).  A draw equal to an earlier one of the same hypothesis is skipped.  After 64 draws a
 *     position still missing takes the smallest pair number not yet used, so the loop ends whatever the generator gives.
 *     svo_align_sample is that function.
 *  7. Model.  Horn's closed form in f64 on the three pairs, the points widened from f32: the centroids, the centred 3 x 3
 *     cross-covariance, the symmetric 4 x 4 matrix, its eigenvectors by cyclic Jacobi, the one of the largest eigenvalue as a unit
 *     quaternion, R, and t = c_q - R c_p.  A model with a non-finite entry scores 0.
 *  8. Score.  count_h = #{c : |R p_c + t - q_c|^2 <= inlier_dist^2}, in f64, the compare inclusive (inlier_dist widened, then
 *     squared).  best = the largest count; at equal counts the smallest h.
 *  9. Refit.  The inlier set starts as best's.  Up to refit_rounds times, while the set has at least 3 members: fit the model of
 *     rule 7 to all members; the new set is every pair within inlier_dist of that model; the round is counted; stop when the set
 *     did not change.  Every sum is taken in a fixed order that depends on the pair numbers only: the same call gives the same bits.
 * 10. Result.  The model is the last one fitted (best's where no round ran), the inliers the last set.  success = n_inliers >=
 *     min_pairs.  On success R, t (x_dst = R x_src + t), T (the same as a row-major 4 x 4) and rms (the root of the inliers' mean
 *     squared residual); zeros otherwise.  n_pairs, n_inliers, best_hypothesis, best_count and refit_rounds_run always.
 *
 * Against an f64 reference that takes its eigenvectors and sums another way the models differ in their last bits, so a pair whose
 * residual sits within rounding of inlier_dist may fall on either side; apart from such pairs the sets are the reference's.
 *
 * Every call is synchronous, synchronises once, waits for the index's own stream only and is legal with frames in flight.  A refused
 * call changes nothing, its outputs included.  With svo_desc_index_set_timing on, last_kernels_ms is the device span from the first
 * kernel the call launches to the last.
 * SVO_ERR_STATE: an index without points.  SVO_ERR_ARG: a span svo_desc_index_match refuses as a row range; n > 4096; spans that
 * share a row; and, for svo_desc_index_pair_rows and svo_desc_index_align, max_dist outside 0 .. 256, a ratio term outside
 * 1 .. 1 << 20, min_pairs outside 3 .. 4096, hypotheses outside 1 .. 1024, refit_rounds outside 0 .. 8, inlier_dist not finite or <= 0.
 *
 * Memory.  The search's n result rows (32 n bytes) go where svo_desc_index_match's go, the index's 4096-row result buffer (128 KiB,
 * held since the index was created).  The rest is one device block the index allocates at the first pair_rows or align call and
 * frees with the index, laid out for n = 4096 and H = 1024 with every part rounded up to 256 bytes: the result row (136 bytes), the
 * two row lists (4 n each), the inlier flags (n), the packed pairs (24 n), the H counts (4 H) and the H models (96 H): 237 824
 * bytes; its first 37 120 bytes have a pinned twin.  Below 400 KiB in all. */
#define SVO_ALIGN_MAX_ROWS 4096
#define SVO_ALIGN_MAX_HYPOTHESES 1024
typedef struct {
    int32_t src_lo, src_hi;      /* S: the rows that move; at most SVO_ALIGN_MAX_ROWS */
    int32_t dst_lo, dst_hi;      /* D: the rows searched */
    int32_t max_dist;            /* rule 2: 0 .. 256 */
    int32_t ratio_num, ratio_den; /* rule 2: 1 .. 1 << 20 each */
    int32_t min_pairs;           /* rules 5 and 10: 3 .. 4096 */
    int32_t hypotheses;          /* rule 6: 1 .. SVO_ALIGN_MAX_HYPOTHESES */
    int32_t refit_rounds;        /* rule 9: 0 .. 8 */
    float   inlier_dist;         /* rules 8 and 9, in the map's unit: finite, > 0 */
    int32_t reserved;            /* 0 */
} svo_align_params;
typedef struct {
    int32_t success, n_pairs, n_inliers, best_hypothesis, best_count, refit_rounds_run;
    double  R[9], t[3];          /* x_dst = R x_src + t */
    double  T[16];               /* the same, row-major 4 x 4: svo_desc_index_transform_points' argument */
    double  rms;
} svo_align_result;
/* max_dist = 40, ratio 7 / 10 (svo_reloc_params_default's), min_pairs = 6, hypotheses = 256, refit_rounds = 4, src = dst = {0, -1}
 * (the caller sets the spans).  inlier_dist is an argument because no default in metres has been measured for any stereo rig: it
 * depends on the baseline, the depth and the triangulation's noise, and this header does not invent one. */
void svo_align_params_default(svo_align_params* params, float inlier_dist);
/* Rule 6's sampler on the host: out[0 .. 3) for hypothesis h of n_pairs pairs.  SVO_ERR_ARG: n_pairs < 3, NULL out. */
int svo_align_sample(uint32_t h, int32_t n_pairs, int32_t* out);
/* Rule 1 alone: out (host) receives n result rows.  The index needs no points for this call. */
int svo_desc_index_match_rows(svo_desc_index* index, int src_lo, int src_hi, int dst_lo, int dst_hi, svo_desc_match* out);
/* Rules 1 - 5: *n_pairs and, where non-NULL, the pairs' source and destination rows, each with room for n entries.  Every
 * parameter is checked as svo_desc_index_align checks it; min_pairs, hypotheses, refit_rounds and inlier_dist play no other part. */
int svo_desc_index_pair_rows(svo_desc_index* index, const svo_align_params* params, int* n_pairs, int32_t* pair_src, int32_t* pair_dst);
/* All of it.  pair_src, pair_dst, pair_inlier (1 / 0): n entries each, each may be NULL; the first result->n_pairs are written. */
int svo_desc_index_align(svo_desc_index* index, const svo_align_params* params, svo_align_result* result, int32_t* pair_src,
                         int32_t* pair_dst, uint8_t* pair_inlier);

/* ---- Landmark fusion: one id per landmark after a map merge or loop closure ---------------------------------------------------------
 * After svo_desc_index_align and svo_desc_index_transform_points have laid a second sequence's landmarks, or a loop's recent ones, on
 * top of the first, every landmark of the overlap exists under two ids with near-identical descriptors and near-identical points.  A
 * query from that place finds one copy as `row` and the other as `row2` with dist2 ~ dist, rule 1 of "Relocalisation" rejects it, the
 * guided search does not help (both copies project to one pixel), and SVO_RETIRE_LATEST_PER_ID cannot thin the copies, because it
 * keys on the id.  svo_desc_index_fuse gives the two copies ONE id (what ORB-SLAM's SearchAndFuse does): it searches the descriptors
 * of a SOURCE span S = [src_lo, src_hi) in a DESTINATION span D = [dst_lo, dst_hi) among the rows whose POINT lies near the source
 * row's, pairs rows up, and renames the source landmarks' ids to their partners' in a RELABEL span L = [relabel_lo, relabel_hi) (the
 * whole index by default), all on the device: no descriptor, point or id leaves it, one host synchronisation.  No point is averaged
 * or snapped: each row keeps its own triangulation.
 *
 * The three spans follow the row_hi = -1 convention.  S has n = src_hi - src_lo <= SVO_FUSE_MAX_ROWS rows; S and D share no row
 * (spans that touch are legal; an empty span shares nothing); L is any span.  Every rule is defined on integers and f32 compares.
 * tag[r], id[r], (x_r, y_r, z_r): row r's.
 *  1. Gate.  Row r of D is ADMISSIBLE for the source row s when tag[r] != SVO_POINT_NONE, tag[s] != SVO_POINT_NONE, and
 *     |x_r - x_s| <= radius, |y_r - y_s| <= radius and |z_r - z_s| <= radius; the subtractions, absolute values and comparisons are
 *     f32 and every limit is inclusive: a cube of side 2 x radius in the map's unit, the 3-D counterpart of rule 2 of "Guided
 *     search".  A source row without a point admits nothing.
 *  2. Search.  For j = 0 .. n - 1, m_j is svo_desc_index_match's definition for the query "descriptor of row src_lo + j" over the
 *     admissible rows of D only: best by (dist, row), second = the best admissible row of another id than the best row's.  Nothing
 *     admissible: SVO_MATCH_NONE and SVO_MATCH_NO_DIST, as for an empty range.  The result does not depend on the chunk size.
 *  3. Accept, one source row per destination landmark, one destination per source landmark, pairs: rules 2 - 5 of "Map alignment"
 *     unchanged on those m_j, the orderings by (m_j.dist, j) included.  Pair c, in increasing j, is (src row src_lo + j, dst row
 *     m_j.row).  There is no min_pairs gate: zero pairs is a success that changes nothing.
 *  4. Map.  from_c = id[pair_src[c]] and to_c = id[pair_dst[c]], both read before anything is written.  A pair with from_c == to_c is
 *     counted in n_same and maps nothing; the others are counted in n_fused.  By rule 3 the from_c are distinct.
 *  5. Relabel.  Every row r of L with id[r] == from_c for a mapping pair c gets id[r] = to_c: one simultaneous step on the ids as they
 *     were.  With a -> b and b -> c in one call, a's rows become b and b's rows become c; no chain is followed.  Descriptors, points,
 *     tags, the order of the rows and the size are untouched.  n_rows_relabelled counts the rows whose id changed.
 *  6. Refusals.  A refused call changes nothing, its outputs included.  SVO_ERR_STATE: an index without points (match_near, pair_near
 *     and fuse; not relabel).  SVO_ERR_ARG: a span svo_desc_index_match refuses as a row range; n > 4096; S and D sharing a row;
 *     radius negative or not finite; and, for pair_near and fuse, max_dist outside 0 .. 256 or a ratio term outside 1 .. 1 << 20.
 * A later call that meets a landmark already fused finds its own id on the other side and counts it in n_same, so a large overlap is
 * fused span after span (one keyframe of at most 4096 rows a call), and a repeated call changes nothing.
 *
 * svo_desc_index_relabel is rule 5 alone on host lists, for a back end that fused landmarks itself: entry i maps from_ids[i] to
 * to_ids[i].  An entry with from == to is ignored, as if it were not in the list; where a `from` value occurs in more than one of the
 * remaining entries, the one at the smallest list position wins.  It needs no points.  SVO_ERR_ARG: n outside 0 .. SVO_FUSE_MAX_LIST,
 * a NULL list with n > 0, a bad row range.
 *
 * Every call is synchronous, waits for the index's own stream only and is legal with frames in flight; match_near, pair_near and fuse
 * synchronise once, and so does relabel after its lists have gone up (through the index's pinned staging, in pieces of 20 480
 * entries, as svo_desc_index_retire's ids do).  With svo_desc_index_set_timing on, last_kernels_ms (svo_desc_index_get_stats) is the
 * device span from the first kernel the call launches to the last.
 *
 * Memory.  The search's n result rows go where svo_desc_index_match's go, its partial states into the search's scratch, and the
 * pairs into "Map alignment"'s device block (237 824 bytes, allocated at the first call that pairs).  The map and the table live in
 * the maintenance scratch of "Index maintenance" (the same buffer, the same growth rule): with e the entries of the list — n for
 * pair_near and fuse, the list's length for relabel — R(b) = b rounded up to a multiple of 256 and slots(e) the smallest power of two
 * >= max(2, 2 e), a call needs
 *   need = 8 448 + 2 R(8 e) + R(4 slots(e))
 * bytes: what the kernels report (64 bytes and 128 cache lines of row counts), the `from` and the `to` list, and the table of list
 * positions.  e = 4096: 106 752 bytes; e = 1 << 20: 24 MiB + 8 448.  An 8 256-byte pinned block receives the counts. */
#define SVO_FUSE_MAX_ROWS 4096
#define SVO_FUSE_MAX_LIST (1 << 20)
typedef struct {
    int32_t src_lo, src_hi;          /* S: the rows whose landmarks are renamed; at most SVO_FUSE_MAX_ROWS */
    int32_t dst_lo, dst_hi;          /* D: the rows searched */
    int32_t relabel_lo, relabel_hi;  /* L: the rows whose ids may change */
    int32_t max_dist;                /* rule 3: 0 .. 256 */
    int32_t ratio_num, ratio_den;    /* rule 3: 1 .. 1 << 20 each */
    float   radius;                  /* rule 1, in the map's unit: finite, >= 0 */
    int32_t reserved;                /* 0 */
} svo_fuse_params;
typedef struct {
    int32_t n_pairs;                 /* rule 3 */
    int32_t n_same, n_fused;         /* rule 4: n_same + n_fused == n_pairs */
    int32_t n_rows_relabelled;       /* rule 5 */
} svo_fuse_result;
/* max_dist = 40, ratio 7 / 10 (svo_reloc_params_default's), src = dst = relabel = {0, -1} (the caller sets S and D).  radius is an
 * argument for the reason svo_align_params_default's inlier_dist is one: how far two triangulations of one landmark lie apart
 * depends on the baseline, the depth and the alignment's residual, no value in metres has been measured for any stereo rig, and
 * this header does not invent one. */
void svo_fuse_params_default(svo_fuse_params* params, float radius);
/* Rules 1 - 2: out (host) receives n result rows. */
int svo_desc_index_match_near(svo_desc_index* index, int src_lo, int src_hi, int dst_lo, int dst_hi, float radius, svo_desc_match* out);
/* Rules 1 - 3, the dry run: *n_pairs and, where non-NULL, the pairs' source and destination rows, each with room for n entries.
 * Every parameter is checked as svo_desc_index_fuse checks it; the relabel span plays no other part. */
int svo_desc_index_pair_near(svo_desc_index* index, const svo_fuse_params* params, int* n_pairs, int32_t* pair_src, int32_t* pair_dst);
/* Rule 5 alone.  from_ids, to_ids: n entries each, host memory; row_hi = -1: the index's size; *n_rows_relabelled may be NULL. */
int svo_desc_index_relabel(svo_desc_index* index, int n, const uint64_t* from_ids, const uint64_t* to_ids, int row_lo, int row_hi,
                           int* n_rows_relabelled);
/* All of it.  pair_src, pair_dst: n entries each, each may be NULL; the first result->n_pairs are written.  result may be NULL. */
int svo_desc_index_fuse(svo_desc_index* index, const svo_fuse_params* params, svo_fuse_result* result, int32_t* pair_src, int32_t* pair_dst);

/* ---- Place candidates: which keyframes of the map a frame resembles ------------------------------------------------------------------
 * svo_desc_index_localize, svo_desc_index_align and svo_desc_index_fuse take the row span of a keyframe; these calls find it (what
 * ORB-SLAM's DetectLoopCandidates does, and with ids in place of descriptors its UpdateLocalKeyFrames).  A keyframe is a TAG: the
 * caller tags the rows of one keyframe alike ("Relocalisation").  The score of a tag is covisibility — how many of the rows under
 * it belong to a landmark the frame recognised — counted by a sweep over the index's ids and tags on the device: no id or tag leaves
 * it and the caller keeps no first_row table.  Voting with svo_desc_index_match's best row alone would be the wrong vote: a landmark
 * seen from k keyframes has k rows and the best one falls on any of them, which smears a place's votes over its neighbours.
 *
 * Every rule is defined on integers.  tag[r], id[r]: row r's; row_hi = -1 is the index's size.
 *  1. Recognised landmarks.  Rules 1 - 3 of "Relocalisation" unchanged over [row_lo, row_hi) with max_dist, ratio_num, ratio_den,
 *     without pixels (svo_desc_index_select with xy = NULL): candidate c is (cand_query[c], cand_row[c]).  M is the set of the
 *     candidates' ids id[cand_row[c]]: at most SVO_PLACE_MAX_IDS ids, one candidate per landmark.  n_landmarks = |M|.
 *  2. Votes.  Row r of [row_lo, row_hi) QUALIFIES when tag_lo <= tag[r] <= tag_hi; tag_lo >= 0, so a row without a point
 *     (SVO_POINT_NONE) never does.  For the qualifying rows of tag t: rows[t] is their number, row_first[t] the smallest r,
 *     row_end[t] the largest r + 1, votes[t] the number of them with id[r] in M.  Plain counts of rows: a landmark with two rows
 *     under one tag counts twice.  A tag without a qualifying row has 0 in all four.  Arrays over the span are indexed t - tag_lo.
 *     Every output is a sum, a minimum or a maximum of integers: the same bits on every run.
 *  3. Places.  P = the tags of the span with votes[t] >= min_votes.  Up to max_places times, while P is not empty: the tag of P
 *     with the largest votes, at equal votes the smallest tag (the older keyframe, the larger loop), is emitted as
 *     {tag, votes, rows, row_first, row_end}, and every t with |t - tag| <= separation leaves P.  separation keeps the consecutive
 *     keyframes of one place from filling the list.  n_tags_voted counts the tags of the span with votes[t] >= 1.
 *  4. Refusals.  A refused call changes nothing, its outputs included.  SVO_ERR_STATE: an index without points (tags live there).
 *     SVO_ERR_ARG: a row range svo_desc_index_match refuses; tag_lo < 0; tag_hi < tag_lo; tag_hi - tag_lo + 1 > SVO_PLACE_MAX_TAGS;
 *     n_ids outside 0 .. SVO_PLACE_MAX_IDS or a NULL list with n_ids > 0; for the two places calls min_votes < 1, separation < 0,
 *     max_places outside 1 .. SVO_PLACE_MAX_PLACES; for svo_desc_index_places n outside 0 .. 4096, max_dist outside 0 .. 256 and a
 *     ratio term outside 1 .. 1 << 20.
 * The rows of a tag need not be contiguous ([row_first, row_end) then holds other tags' rows too: after a fuse and a retire the
 * caller decides whether the span is still the keyframe), and row_hi keeps a loop closer's most recent keyframes out of the vote.
 *
 * Every call is synchronous, runs in the index's own stream, is legal with frames in flight, changes nothing in the index and
 * synchronises with the host once.  svo_desc_index_set_timing: see there.
 *
 * Memory.  The id list, the bins (16 bytes a tag) and rule 3's list (8 bytes a tag; not for tag_votes) live in the maintenance
 * scratch of "Index maintenance" (the same buffer, the same growth rule): with b = tag_hi - tag_lo + 1 and R as in "Landmark
 * fusion", need = 2 304 + R(8 n_ids) + R(16 b) + R(8 b) bytes; 4096 ids and 1 << 20 tags: 24 MiB + 35 072.  A pinned block of the
 * same growth rule receives 2 080 bytes (places) or 2 080 + 16 b bytes (tag_votes).  A sweep block holds M in 8 n_ids + 4 slots
 * bytes of LDS (slots as in "Landmark fusion"): 64 KiB at most. */
#define SVO_PLACE_MAX_TAGS (1 << 20)
#define SVO_PLACE_MAX_PLACES 64
#define SVO_PLACE_MAX_IDS 4096
typedef struct {
    int32_t row_lo, row_hi;          /* the rows searched (rule 1) and swept (rule 2) */
    int32_t max_dist;                /* rule 1: 0 .. 256 */
    int32_t ratio_num, ratio_den;    /* rule 1: 1 .. 1 << 20 each */
    int32_t tag_lo, tag_hi;          /* rule 2: the tags that get a bin, inclusive; at most SVO_PLACE_MAX_TAGS of them */
    int32_t min_votes;               /* rule 3: >= 1 */
    int32_t separation;              /* rule 3: >= 0 */
    int32_t max_places;              /* rule 3: 1 .. SVO_PLACE_MAX_PLACES */
} svo_place_params;
typedef struct {
    int32_t tag, votes, rows;        /* rule 2's counts of the tag */
    int32_t row_first, row_end;      /* its rows lie in [row_first, row_end): the span svo_desc_index_localize, align and fuse take */
    int32_t reserved[3];             /* 0 */
} svo_place;
typedef struct {
    int32_t n_landmarks;             /* |M| */
    int32_t n_tags_voted;            /* the tags of the span with at least one vote */
    int32_t n_places;                /* the places written */
} svo_place_result;
/* rows = {0, -1}, max_dist = 40, ratio 7 / 10 (svo_reloc_params_default's), tags = {0, SVO_PLACE_MAX_TAGS - 1}, min_votes = 1,
 * separation = 0, max_places = 8. */
void svo_place_params_default(svo_place_params* params);
/* Rule 2 alone with the caller's id list as M (host memory; duplicates are legal, M is a set): the stage the tests read, and the
 * local-map query "which keyframes saw the landmarks I am tracking".  votes, rows, row_first, row_end: tag_hi - tag_lo + 1 host
 * entries each, each may be NULL. */
int svo_desc_index_tag_votes(svo_desc_index* index, int n_ids, const uint64_t* ids, int row_lo, int row_hi, int32_t tag_lo, int32_t tag_hi,
                             int32_t* votes, int32_t* rows, int32_t* row_first, int32_t* row_end);
/* Rules 1 - 3 for n descriptors of 32 bytes.  places: room for params->max_places entries, the first result->n_places are written.
 * cand_query, cand_row: n entries each, each may be NULL; the first result->n_landmarks are written, as svo_desc_index_select's. */
int svo_desc_index_places(svo_desc_index* index, int n, const uint8_t* query, const svo_place_params* params, svo_place_result* result,
                          svo_place* places, int32_t* cand_query, int32_t* cand_row);
/* Rules 2 - 3 for a back end that knows its landmarks: M is the id list.  max_dist and the ratio play no part and are not checked. */
int svo_desc_index_places_from_ids(svo_desc_index* index, int n_ids, const uint64_t* ids, const svo_place_params* params,
                                   svo_place_result* result, svo_place* places);
/* Diagnostics, for tools/place_bench.py: on = 0 makes the sweep issue every qualifying row's four atomics on its own in place of one
 * set per run of equal tags in a wave (the default, on != 0).  The results do not depend on it. */
int svo_desc_index_set_place_combine(svo_desc_index* index, int on);

/* ---- Batched place candidates: every camera's keyframe votes in one call --------------------------------------------------------------
 * A map back end asks per step which keyframes of the map each camera resembles (loop-closure and map-merge candidates, the
 * tracker's local map); the calls above serve one camera each, with an upload, launches, a copy back and a host wait per camera.
 * These serve n_cameras cameras in one call: one upload, ONE sweep that reads every row of the index once for the whole call, one
 * pick launch with a block per camera, one host synchronisation.  Three of rule 2's four arrays — rows, row_first, row_end — depend
 * on the row range and the tag window alone, so they exist once; only votes is per camera.
 *
 * The contract, which is the whole definition.  Camera b owns the slice [begin[b], begin[b + 1]) of ids (id_begin) or of query
 * (query_begin); one params record — one row range, one tag window — holds for the call, as in "Batched relocalisation".
 *  - results[b], the first results[b].n_places entries of places + b * params->max_places and, for places_batch, the first
 *    results[b].n_landmarks entries of cand_query and cand_row at offset query_begin[b] (cand_query numbered inside the slice) equal,
 *    in every bit, what svo_desc_index_places_from_ids, or svo_desc_index_places, returns for that slice alone.
 *  - votes + b * n_bins (n_bins = tag_hi - tag_lo + 1; camera-major) equals svo_desc_index_tag_votes' votes for that slice; rows,
 *    row_first and row_end (n_bins entries each) equal any single call's.
 *  - Nothing beyond those entries is written.  Each output pointer may be NULL.
 *  - The results do not depend on the number of cameras or their order, on how the library groups cameras into launches, or on
 *    svo_desc_index_set_chunk_rows.
 *  - An id may appear in any number of cameras' lists and more than once in one camera's list: M is a set per camera.  0 and
 *    2^64 - 1 are ids like any other.
 * Refusals, each decided before anything is uploaded or enqueued; a refused call leaves every output untouched.  SVO_ERR_STATE /
 * SVO_ERR_ARG: whatever the single call refuses for any slice ("Place candidates", rule 4; a NULL list or NULL queries with a
 * total above 0); the offsets' rules of "Batched relocalisation" — begin[0] != 0, a decreasing offset, a slice above 4096, a total
 * above SVO_PLACE_BATCH_MAX_IDS, n_cameras outside 0 .. SVO_PLACE_BATCH_MAX_CAMERAS; and n_cameras x n_bins above
 * SVO_PLACE_BATCH_MAX_BINS (narrow the tag window, or split the cameras over calls).  Zero cameras is legal, launches nothing and
 * writes nothing.
 *
 * Every call is synchronous, runs in the index's own stream, synchronises with the host once, is legal with frames in flight and
 * changes nothing in the index (svo_desc_index_get_batch_order reports no batch call after places_batch: it used that staging).
 * With svo_desc_index_set_timing on, last_kernels_ms is, as after svo_desc_index_places, the device span of these kernels alone —
 * the clearing, the table, the sweep and the pick — not the search and the selection in front.
 *
 * How it runs (none of it shows in the results).  The ids of all cameras form one list; position p's key is the pair (ids[p],
 * camera of p), read through the list, which never changes while the table lives.  A global open-addressing table of list
 * positions (slots as in "Landmark fusion", on the total) is hashed by the id alone and claimed with a 32-bit compare-and-swap per
 * distinct pair; results[b].n_landmarks counts camera b's fresh inserts.  The sweep — one lane per row — accumulates the shared
 * bins with the single sweep's wave-combined runs and, for a row whose tag qualifies, walks from hash(id) to the first empty slot,
 * adding 1 to votes[camera][bin] at every slot that holds its id.  Rule 3 runs with a block per camera over its row of votes.
 * For places_batch the search and the selection in front are "Batched relocalisation"'s, unguided, without pixels and without its
 * PnP, through that section's staging and stage context; the list is gathered on the device from the selection's candidate rows.
 *
 * Memory.  The device side lives in the maintenance scratch of "Index maintenance" (the same buffer, the same growth rule).  With C
 * cameras, T ids or queries in all, b bins, P = max_places (0 for tag_votes_batch) and R, slots as in "Landmark fusion", a call needs
 *   need = R(16 C) + R(32 P C) + R(16 b) + R(4 C b)      a record per camera, the places, the shared bins, the votes (what comes down)
 *        + R(4 (C + 1)) + R(8 T) + R(4 T) + R(4 slots(T)) the offsets, the id list, the camera of every position, the table
 * bytes: 512 cameras of 2048 ids and 256 bins, P = 8: 20 MiB + 669 952; the limits (C x b = 1 << 24, T = 1 << 20): about 100 MiB.
 * The pinned block of "Place candidates" (the same growth rule) holds R(4 (C + 1)) + R(8 T) bytes going up and, coming down,
 * R(16 C) + R(32 P C) bytes (the two places calls) or R(16 C) + R(16 b) + R(4 C b) (tag_votes_batch).  places_batch also takes
 * "Batched relocalisation"'s stagings and partial states for T queries. */
#define SVO_PLACE_BATCH_MAX_CAMERAS 1024
#define SVO_PLACE_BATCH_MAX_IDS (1 << 20)
#define SVO_PLACE_BATCH_MAX_BINS (1 << 24)
/* Rule 2 for every camera.  id_begin: n_cameras + 1 offsets into ids.  votes: n_cameras x n_bins; rows, row_first, row_end: n_bins. */
int svo_desc_index_tag_votes_batch(svo_desc_index* index, int n_cameras, const int32_t* id_begin, const uint64_t* ids, int row_lo, int row_hi,
                                   int32_t tag_lo, int32_t tag_hi, int32_t* votes, int32_t* rows, int32_t* row_first, int32_t* row_end);
/* Rules 2 - 3 for every camera.  results: n_cameras; places: n_cameras x params->max_places. */
int svo_desc_index_places_from_ids_batch(svo_desc_index* index, int n_cameras, const int32_t* id_begin, const uint64_t* ids,
                                         const svo_place_params* params, svo_place_result* results, svo_place* places);
/* Rules 1 - 3 for every camera.  query_begin: n_cameras + 1 offsets into query (32 bytes a descriptor); cand_query, cand_row: total
 * entries each, camera b's at query_begin[b]. */
int svo_desc_index_places_batch(svo_desc_index* index, int n_cameras, const int32_t* query_begin, const uint8_t* query,
                                const svo_place_params* params, svo_place_result* results, svo_place* places, int32_t* cand_query,
                                int32_t* cand_row);

/* ---- Landmark consolidation: medoid descriptor and mean point per landmark --------------------------------------------------------
 * A landmark seen in k frames has k rows, each with one view's descriptor and one triangulation.  svo_desc_index_consolidate leaves
 * one row per landmark: the most central of the observed descriptors and the mean of the points that agree with it.  It runs on the
 * device, in place, is synchronous, waits for the index's own stream only and is legal with frames in flight.  The rules are the
 * whole definition; the result equals a sequential program's in every bit.  Let n0 be the size before the call and
 * S = [row_lo, row_hi) the scope (row_hi = -1: n0).
 *  1. Members.  Row r is a member when r is in S, tag[r] != SVO_POINT_NONE and tag_lo <= tag[r] <= tag_hi.  A group is the set of
 *     members with one id, in ascending rows r_0 < ... < r_(k-1).  Every non-member — a row outside S, a row without a point, a row
 *     outside the tag window — is kept and carried bit for bit.
 *  2. Views.  The views of a group are its last min(k, SVO_CONSOLIDATE_MAX_VIEWS) members.  The older members of a larger group are
 *     dropped without contributing; such a group is counted in n_capped_groups.
 *  3. Medoid.  For view i, s_i is the sum over the group's views j of d(i, j), the search's Hamming distance.  The medoid is the view
 *     with the smallest s_i, at equal sums the one with the larger row.  (ORB-SLAM's ComputeDistinctiveDescriptors takes the least
 *     median; this rule is the sum, and no parity with it is claimed.)
 *  4. Point.  View j is near when |p_j[c] - p_medoid[c]| <= radius in f32 on all three axes c ("Landmark fusion"'s gate); the
 *     medoid is always near, the other views are counted in n_far_views.  Coordinate c of the new point is
 *     f32(sum_c / (double)n_near), where sum_c is the f64 sum of the near views' coordinates in ascending row order, starting from
 *     0.0, every addition and the division rounded on its own, without contraction.
 *  5. Result.  Of a group of two or more, only r_(k-1) is kept: it takes the medoid's descriptor and rule 4's point and keeps its
 *     own id and its own tag.  A group of one row is left as it is, in every bit.  kept_before (n0 + 1 entries, or NULL), the new
 *     size, the order of the rows and the remapping of stored row numbers are exactly svo_desc_index_retire's.
 * The result record: n_members; n_groups; n_dropped = n_members - n_groups; n_far_views; n_capped_groups; n_kept, the new size.  A
 * second identical call changes nothing.  radius is in the map's unit; no default is measured for any rig.
 * Refusals, each decided before the first write to the index: a refused call changes nothing.  SVO_ERR_ARG: a row range
 * svo_desc_index_match refuses, a radius that is not finite or negative.  SVO_ERR_STATE: an index without points.
 * SVO_ERR_INTERNAL: the table of ids overflowed, which its size rules out.
 *
 * What it costs in information.  After consolidation a landmark has one row and so one tag: in "Place candidates" it votes for the
 * keyframe of its latest view only, exactly as after SVO_RETIRE_LATEST_PER_ID.  Consolidate what has left the window the place
 * search looks at (tag_hi), not the whole index.  Consolidation does not cross ids: run svo_desc_index_fuse first.
 *
 * Memory.  All working memory is the maintenance scratch of "Index maintenance" (the same buffer, the same growth rule).  With m the
 * scope's rows and R and slots as there, a call needs
 *   need = R(m) + R(4 (m + 1)) + R(4 (ceil(m / 256) + 257)) + 2 R(4 slots(m)) + R(4 m) + R(56 min(retire_slab_rows, n0 - row_lo))
 * bytes: retire's keep flags, ranks and block counts, the table of latest rows, the members counted per slot, the member list and
 * the bounce buffer.  An empty scope needs nothing.
 *
 * svo_desc_index_read_rows copies the rows [row_lo, row_hi) (row_hi = -1: the size) to the host: desc 32 bytes a row, ids, xyz three
 * floats a row, tags; each may be NULL.  A row without a point reads xyz = +inf and tag = SVO_POINT_NONE.  The data comes through the
 * index's pinned staging 4096 rows at a time on the index's stream; the call is legal with frames in flight.  With
 * svo_desc_index_add_points (and svo_desc_index_add for the runs of rows without a point) it saves and restores a map.
 * SVO_ERR_STATE: xyz or tags asked of an index without points.  SVO_ERR_ARG: a row range svo_desc_index_match refuses. */
#define SVO_CONSOLIDATE_MAX_VIEWS 64
typedef struct {
    int32_t row_lo, row_hi;          /* the scope [row_lo, row_hi), row_hi = -1: the size */
    int32_t tag_lo, tag_hi;          /* rule 1: inclusive */
    float   radius;                  /* rule 4: finite, >= 0 */
    int32_t reserved;                /* 0 */
} svo_consolidate_params;
typedef struct {
    int32_t n_members, n_groups, n_dropped, n_far_views, n_capped_groups, n_kept;
    int32_t reserved[2];             /* 0 */
} svo_consolidate_result;
/* the whole index, tags 0 .. INT32_MAX */
void svo_consolidate_params_default(svo_consolidate_params* params, float radius);
/* result may be NULL; kept_before: size-before-the-call + 1 entries, or NULL */
int svo_desc_index_consolidate(svo_desc_index* index, const svo_consolidate_params* params, svo_consolidate_result* result, int32_t* kept_before);
int svo_desc_index_read_rows(svo_desc_index* index, int row_lo, int row_hi, uint8_t* desc, uint64_t* ids, float* xyz, int32_t* tags);

/* ---- Detection masks: keep features off marked regions of the left image ----------------------------------------------------
 * What OpenCV users pass to FeatureDetector::detect(image, keypoints, mask); the reference calls cv::FAST directly and has none.
 * A mask is an 8-bit image of the context's size width x height — the rectified, grey geometry, whatever the input format and the
 * rectification are.  A non-zero byte means "features allowed here".  Without a mask a context launches exactly what it always did.
 *
 * The rule.  With a mask, the list appendFeaturesFromImage hands to the bucket grid — the existing tracks first, then the new
 * cv::FAST hits in raster order — is filtered as KeyPointsFilter::runByPixelsMask does it:
 *   an entry at (x, y) stays iff mask[min((int)(y + 0.5f), H-1)][min((int)(x + 0.5f), W-1)] != 0.
 * FAST, its threshold and its 3x3 non-max suppression run on the whole image as before; the mask is applied to the survivors,
 * AFTER NMS, as OpenCV does (a suppressed neighbour of a masked-out winner does not come back).  A filtered entry makes no offer to
 * the grid; the others keep their rank in the unfiltered list, so ties break exactly as in the filtered one.  A filtered track is
 * gone from the feature set, as if its bucket had been lost.  The second detection pass (threshold / 4) uses the same mask.
 *
 * Which image a mask belongs to.  The detection of call k scans the left image of call k - 1, and the tracks it filters are
 * positions in that image.  A mask therefore belongs to a left image, not to a call: the mask in force when a frame is submitted
 * describes THAT FRAME'S left image and is applied when that image is scanned, in the sequence's following call.  A static mask is
 * set once and holds until it is cleared; a per-frame mask (a segmentation network's output) is set before each submit.  After a
 * clear the next call still applies the mask of the image it scans; the call after that is unmasked.
 *
 * svo_set_detection_mask: seq = -1 installs the one shared mask, seq >= 0 a sequence's own, which overrides the shared one.
 * mask = NULL clears (seq = -1: all of them).  mask: height rows of width bytes, `stride` bytes apart, in host memory, or
 * (on_device != 0) in device memory — then the caller's writes to it must be complete, or ordered on svo_get_stream's stream.
 * The mask is copied into library-owned device memory on the frame stream, like svo_reset_sequence's work: legal with frames in
 * flight, no host synchronisation for a device mask, and the copy lands between the frames submitted before and after it (a host
 * mask passes through one pinned staging buffer; a second host mask waits for the first one's copy).  Every scope keeps two slots:
 * a frame records the slot of its left image and the setter writes the other, so the detection still queued for the previous
 * image reads what it was given.  (The shared pair has one record for all sequences: with ragged frames, a sequence that stays
 * idle across two shared-mask changes sees the newer mask on its old image.  A sequence's own pair has no such limit: an idle
 * sequence's record and slots are not touched.)  Buffers are allocated at first use and freed with the context.
 * Errors (SVO_ERR_ARG): a channels = 3 context (FAST walks the bytes of the interleaved row there, pixel positions mean nothing),
 * features_per_bucket > 1 (the general bucket walk takes no mask), stride < width, seq out of range.
 * svo_get_last_frame_path reports SVO_PATH_DETECT_MASKED for a frame whose detection applied a mask to some sequence.  A lone
 * stream's masked frame issues the unfused front (ingest, then the masked FAST kernel: one launch more); under SVO_GRAPH=1 masked
 * frames run from the launch list, as rectifying frames do.
 * svo_get_detection_mask: the mask in force for the frames submitted next (seq's own, else the shared one; seq = -1: the shared
 * one) to out (width * height bytes, packed; may be NULL), *present = whether there is one.  Synchronises the context's stream. */
int svo_set_detection_mask(svo_context* ctx, int seq, const uint8_t* mask, int stride, int on_device);
int svo_get_detection_mask(svo_context* ctx, int seq, uint8_t* out /* W*H, packed */, int* present);
/* ---- Motion prior: seed the temporal LK passes with a predicted flow ---------------------------------------------------------
 * What OpenCV users get from OPTFLOW_USE_INITIAL_FLOW, fed from a gyro, a wheel model or the previous pose.  The reference calls
 * calcOpticalFlowPyrLK with flags = 0 and has none, so this is off by default: a context that never sets a prior launches exactly
 * what it always did.  Both temporal passes of circularMatching (L0 -> L1 and R1 -> R0) otherwise start their search at the
 * feature's own position; in a turn every feature moves by fx tan(yaw step) pixels and the pyramid runs out of reach.
 *
 * A prior is a 3x3 homography H (f32, row-major) that maps pixel coordinates in the sequence's previous frame (T0) to predicted
 * pixel coordinates in the frame being submitted (T1).  The rectified cameras share K, so one H serves both cameras; its inverse Hi
 * serves the backward pass.
 *
 * Prediction pred(M, (x, y)), M = m0 .. m8.  Every operation is f32 and rounded once, nothing is fused, division is IEEE:
 *   X = (m0 x + m1 y) + m2,   Y = (m3 x + m4 y) + m5,   D = (m6 x + m7 y) + m8.
 *   If D > 0 and X / D, Y / D are both finite the guess is (X / D, Y / D); otherwise it is (x, y) (a NaN anywhere ends here).
 *
 * LK with a guess (OPTFLOW_USE_INITIAL_FLOW): at the top level nextPt = guess * 2^-top instead of prevPt * 2^-top.  The template
 * still comes from prevPt, and every test, rule and counter of the pass is otherwise unchanged: guess == prevPt gives the bits of
 * the pass without a guess.
 *
 * Circular matching with a prior: pass 0 (L0 -> L1) starts from pred(H, pl0), pass 2 (R1 -> R0) from pred(Hi, pr1); passes 1 and 3
 * (the stereo passes) start as always.  Masks, early-out, bounds tests, the loop-closure threshold and the work counters are unchanged.
 *
 * Hi when the caller passes none: the adjugate of H widened to f64 (each cofactor a d - b c in f64), divided by
 * det = h0 C00 + h1 C01 + h2 C02, each entry rounded to f32.  A det that is 0 or not finite is SVO_ERR_ARG.
 *
 * Scope.  A prior is one-shot and per sequence: it belongs to the next frame that sequence takes and is consumed by it.  An idle
 * frame of a masked submit does not consume it.  A frame without a prior for a sequence tracks that sequence exactly as without
 * the feature, bit for bit, also when other sequences of the same launch have one.  svo_reset_sequence drops a pending prior.
 *
 * Ordering.  The setters are host state plus, per frame, one small copy on the frame's stream from a pinned block of its
 * results-ring slot: stream-ordered, no host synchronisation, legal with frames in flight — every frame carries its own priors, as
 * it carries its input format.  A frame in which some active sequence has a prior launches k_lk_chain_prior where it would launch
 * k_lk_chain, reports SVO_PATH_MOTION_PRIOR, and under SVO_GRAPH=1 runs from the launch list, as masked frames do.
 *
 * SVO_ERR_ARG: a channels = 3 context, an lk_float_sums = 1 context (that mode exists to reproduce the reference's recording, which
 * has no prior), seq out of range, a non-finite entry, a singular H with Hi = NULL.  svo_circular_matching (the member form) returns
 * SVO_ERR_STATE while a prior is pending.
 *
 * svo_set_motion_prior: seq = -1 sets every sequence; H = NULL clears a pending prior (Hi is not looked at); Hi = NULL makes the
 * library invert H as above.
 * svo_set_motion_priors: one call per frame at batch sizes.  H (and Hi, or NULL: inverted) hold n_seq x 9 floats; has: n_seq
 * bytes, non-zero = the sequence gets its row, zero = its pending prior is cleared; NULL = every sequence gets its row.  Nothing
 * is changed when any used row is refused.
 * svo_get_motion_prior: what the next frame of seq will use — *pending (0 / 1), and with a prior pending H and Hi (each may be
 * NULL).  Host side only: no device access, no synchronisation.
 * svo_motion_prior_from_rotation: pure host helper.  H = f32(K R K^-1), Hi = f32(K Rt K^-1), K = Pl[:, :3], computed in f64 (K^-1 by
 * the adjugate).  R (3x3 row-major) rotates T0-camera coordinates into T1-camera coordinates: a gyro's integrated increment moved
 * into the camera frame.  Either output may be NULL.  SVO_ERR_ARG: a singular K, a non-finite entry. */
int svo_set_motion_prior(svo_context* ctx, int seq, const float H[9], const float Hi[9]);
int svo_set_motion_priors(svo_context* ctx, const float* H /* n_seq x 9 */, const float* Hi /* n_seq x 9 or NULL */, const uint8_t* has /* n_seq or NULL = all */);
int svo_get_motion_prior(svo_context* ctx, int seq, float H[9], float Hi[9], int* pending);
int svo_motion_prior_from_rotation(const float Pl[12], const double R[9], float H[9], float Hi[9]);
/* Predicted priors: the prior from each sequence's own last pose, computed on the device.  With frames in flight the host has not
 * seen frame k-1's pose when it submits frame k, so it cannot hand that pose over through the setters above without collecting
 * first; the rotation is on the device already, on the stream the next frame runs on.  In SVO_PRIOR_LAST_ROTATION one small launch
 * (k_prior_predict, one thread per sequence that takes the frame) at the head of every frame turns it into the frame's prior rows.
 *
 * The rule, per sequence that takes a frame:
 *  1. A pending explicit prior (svo_set_motion_prior / svo_set_motion_priors) wins: it is consumed as always, its bits untouched.
 *  2. Otherwise, in SVO_PRIOR_LAST_ROTATION, the sequence gets a predicted prior if the last frame it took returned ok = 1 and it
 *     has not been reset since (svo_reset_sequence: the first frames after a reset get none).  An idle frame writes no state, so a
 *     sequence that resumes after a pause predicts from the last frame it took, however many frames it sat out.  The prior is
 *       H = f32(K R K^-1),  Hi = f32(K Rt K^-1),
 *     K = Pl[:, :3] of the sequence's left projection matrix, R the rotation that frame's solve ended with: the transpose of the
 *     upper-left 3x3 of the transform it returned, R[i][j] = T[4 j + i] (the inverse transform stores Rt exactly).  The arithmetic is
 *     svo_motion_prior_from_rotation's: f64 throughout, K^-1 by the adjugate divided by det = k0 C00 + k1 C01 + k2 C02, a product's
 *     three terms summed left to right ((a b + c d) + e f), K R first and then (K R) K^-1, nothing fused, each entry rounded to f32
 *     once.  A singular K, or a non-finite entry in K, R, H or Hi, gives no prior.
 *  3. Otherwise the sequence has no prior in this frame and tracks exactly as without the feature, bit for bit.  A failed frame
 *     therefore seeds nothing: a bad pose cannot feed on itself, and the frame after it searches from the features' own positions.
 * Host equivalent: a context in SVO_PRIOR_EXPLICIT that collects every frame and, before the next submit, calls
 * svo_motion_prior_from_rotation(Pl, R, H, Hi) and svo_set_motion_prior(ctx, seq, H, Hi) for every sequence whose collected frame
 * returned ok = 1 (R from that frame's T as above) submits the same frames: the same 18 floats, the same results in every bit.
 *
 * svo_set_motion_prior_mode: host state carried per frame, like the input format — legal with frames in flight, in force from the
 * next submit.  SVO_PRIOR_EXPLICIT (the default) is everything above this paragraph and nothing else: a context that never sets the
 * mode launches exactly what it always did.  While SVO_PRIOR_LAST_ROTATION is set every frame some sequence takes launches
 * k_prior_predict and k_lk_chain_prior, reports SVO_PATH_MOTION_PRIOR | SVO_PATH_PRIOR_PREDICTED, and under SVO_GRAPH=1 runs from
 * the launch list; a frame on which every sequence is idle launches neither.  The frame entry points only: svo_circular_matching
 * and the stage calls are unchanged.  SVO_ERR_ARG: an unknown mode, a channels = 3 context, an lk_float_sums = 1 context.
 * svo_get_last_motion_prior: what the frame last collected used for seq — *source 0 none (H, Hi untouched), 1 an explicit prior,
 * 2 a predicted one; H and Hi (each may be NULL) are the 18 floats k_lk_chain_prior read.  An idle sequence of that frame reports
 * 0.  Host memory only, no synchronisation.  SVO_ERR_STATE before the first collect; a context that never had a prior reports 0. */
#define SVO_PRIOR_EXPLICIT      0   /* default: only what the setters give */
#define SVO_PRIOR_LAST_ROTATION 1   /* a sequence without an explicit prior for a frame gets one predicted from its last pose */
#define SVO_PATH_PRIOR_PREDICTED 4096 /* svo_get_last_frame_path: the frame was issued in SVO_PRIOR_LAST_ROTATION and ran k_prior_predict */
int svo_set_motion_prior_mode(svo_context* ctx, int mode);
int svo_get_motion_prior_mode(svo_context* ctx, int* mode);
int svo_get_last_motion_prior(svo_context* ctx, int seq, float H[9], float Hi[9], int* source);

/* Diagnostics (pyramid tests): one level of one stored pyramid of sequence seq, WITH its stored border — every level keeps a
 * REFLECT_101 border of `pad` pixels on each side (the LK kernel reads it directly), as cv::buildOpticalFlowPyramid keeps its
 * winSize border.  out gets (h + 2 pad) rows of (w + 2 pad) bytes, packed, from pixel (-pad, -pad); cap is its size in bytes.
 * which: SVO_PYR_T1 or SVO_PYR_LAST_LEFT; cam: 0 left, 1 right; plane: 0 .. channels-1 (a BGR context keeps one pyramid per
 * colour plane); level: 0 .. n_levels-1.  w, h, pad, n_levels may be NULL; they are filled before anything else is checked, and
 * out == NULL returns SVO_OK after filling them (sizes only, no device access).  SVO_ERR_STATE while frames are in flight, for a
 * sequence without a frame since its creation or its last reset (the pyramids of a reset sequence are not its own any more), and
 * for SVO_PYR_LAST_LEFT while no frame has cached that pair.  Bad indices: SVO_ERR_ARG.  Synchronises the context's stream. */
#define SVO_PYR_T1        0   /* the pyramids of the sequence's last frame (= imageLeftT0_ / imageRightT0_ of the next) */
#define SVO_PYR_LAST_LEFT 1   /* lastLeftPyramid's slot (vo.cpp:50-53, 179-181, 231-232): may be older than T1 */
int svo_get_pyramid(svo_context* ctx, int seq, int which, int cam, int plane, int level,
                    uint8_t* out, int64_t cap, int* w, int* h, int* pad, int* n_levels);
/* Diagnostics (derivative-plane tests): the Scharr planes the LK kernel loads at the levels >= 1 (many-sequence grey contexts in
 * the exact-sums mode keep them beside every pyramid), one level of one stored pyramid, WITH the stored border.  ix / iy each get
 * (h + 2 pad) rows of (w + 2 pad) int16 samples, packed, from sample (-pad, -pad): inside the level 4 x the Scharr derivative of
 * the level with its REFLECT_101 border, outside it zero (derivBorder = BORDER_CONSTANT).  cap is the size of each array in
 * samples; either may be NULL.  which, cam, the slot read, the SVO_ERR_STATE refusals (frames in flight, no frame since creation or
 * reset, no cached lastLeftPyramid) and the synchronisation are svo_get_pyramid's.  level: 1 .. n_levels-1 (level 0 has no planes:
 * SVO_ERR_ARG).  pad and n_levels are filled once seq, which and cam are valid, w and h once level is; ix == iy == NULL returns
 * SVO_OK after filling them.  A context that keeps no planes (<= 8 sequences, channels = 3, lk_float_sums = 1, a one-level
 * pyramid, SVO_LK_DERIV=0 or SVO_INGEST_AHEAD=0 in the environment) returns SVO_ERR_STATE, with a message that says so, whatever
 * level and the arrays are: that is how a caller asks whether the planes exist.  A pure read: it changes no launch. */
int svo_get_derivatives(svo_context* ctx, int seq, int which, int cam, int level,
                        int16_t* ix, int16_t* iy, int64_t cap /* samples per array */,
                        int* w, int* h, int* pad, int* n_levels);
/* Timing: HIP-event milliseconds of the dominant kernel (the fused LK chain) in the last processed frame, and of the whole frame.
 * With SVO_GRAPH=1 in the environment a context replays each frame as a captured hipGraph (one per results-ring slot; off by
 * default: measured slightly slower than the launch list on MI355X): stage events are then not recorded and lk_ms /
 * svo_get_stage_timing fail with SVO_ERR_STATE; frame_ms is always available. */
int svo_get_last_timing(svo_context* ctx, float* lk_ms, float* frame_ms);
/* The four stage-boundary events of a frame cost a lone stream ~10 us per frame (measured, one sequence), so they are recorded
 * only on request: svo_set_stage_timing(ctx, 1), or SVO_STAGE_TIMING=1 in the environment when the context is created.  While
 * off, lk_ms and svo_get_stage_timing fail with SVO_ERR_STATE; frame_ms is always available. */
int svo_set_stage_timing(svo_context* ctx, int on);
/* Per-stage HIP-event milliseconds of the last collected frame (all sequences of the context together), in pipeline order:
 * ms[0] ingest + pyramids (vo.cpp:74-75, 200-201)   ms[1] FAST + bucketing, both passes (vo.cpp:325-332)
 * ms[2] the four LK passes + masks (vo.cpp:203-230, 341-359)   ms[3] compaction + triangulation (vo.cpp:233-238, 360-364, 89-94)
 * ms[4] RANSAC-PnP, inlier update, gates, result record (vo.cpp:101-136).  The reference has no timers.
 * A lone-stream context (<= 8 sequences) runs independent stages in shared launches: ms[0] then covers ingest + pyramids AND the
 * first detection pass (ms[1]: only the second pass), ms[3] covers compaction, triangulation AND the first EPnP chunk. */
int svo_get_stage_timing(svo_context* ctx, float ms[5]);
void* svo_get_stream(svo_context* ctx);   /* hipStream_t the context launches on */

/* ------------------------------------------------------------------------------------------------
 * Stage-level entry points (host arrays in / out, one call = upload + kernel(s) + download).
 * They run the same kernels as the frame pipeline and exist so the reference's own unit tests
 * (src/main.cpp:50-264) and the parity tests can exercise each stage alone.  Their device buffers are kept per calling thread
 * and reused while device, image size and the buffer-shaping part of the configuration (bucket grid, LK window, levels, channels,
 * at most the RANSAC iteration count they were allocated for) stay the same — other parameters are taken over in place.
 * svo_stage_cache_clear() releases the calling thread's buffers.  A thread that exits hands its buffers to the next thread that
 * needs some (they are not freed at thread exit, where the HIP runtime may be gone): svo_stage_cache_clear_all() frees every
 * cached context that no live thread holds (plus the caller's) and returns how many it freed.
 * ---------------------------------------------------------------------------------------------- */

void svo_stage_cache_clear(void);
int svo_stage_cache_clear_all(void);

/* replaces: featureDetectionFast(image, fast_threshold, response_strengths)  (vo.h:393-395, feature_set.cpp:55-68)
 * i.e. cv::FAST(.., nonmaxSuppression=true).  xy: cap x 2, resp: cap.  *n_out = total found (may exceed cap). */
int svo_fast_detect(int device, const uint8_t* img, int w, int h, int stride, int threshold,
                    int cap, float* xy, float* resp, int* n_out);
/* the same behind a detection mask (the section on detection masks: applied to the NMS survivors); mask rows mask_stride apart */
int svo_fast_detect_masked(int device, const uint8_t* img, int w, int h, int stride, int threshold,
                           const uint8_t* mask, int mask_stride, int cap, float* xy, float* resp, int* n_out);
/* the NMS-surviving score map (h*w bytes, 0 where no keypoint) — test hook for the FAST kernel */
int svo_fast_score_map(int device, const uint8_t* img, int w, int h, int stride, int threshold, uint8_t* score);

/* replaces: FeatureSet::filterByBucketLocationInternal(image, bah, baw, start_row, per_bucket)
 * (vo.h:168-172, feature_set.cpp:95-147) incl. Bucket::add_feature / compute_score (feature_set.cpp:16-53).
 * In place on (xy, ages, strengths); *n_io is the count in and out. */
int svo_bucket_filter(int device, int img_w, int img_h, int* n_io, float* xy, int* ages, int* strengths,
                      int buckets_along_height, int buckets_along_width, int bucket_start_row,
                      int features_per_bucket, int age_threshold, int fast_threshold);

/* replaces: FeatureSet::appendFeaturesFromImage(image, fast_threshold) with the default grid
 * (vo.h:186-187, feature_set.cpp:75-89): FAST + append (age 0) + bucket filter, fused on the GPU
 * (bucket winners are picked with 64-bit atomicMax keys straight from the FAST kernel). cap = array capacity. */
int svo_append_features_from_image(int device, const svo_config* cfg, const uint8_t* img, int w, int h, int stride,
                                   int fast_threshold, int cap, int* n_io, float* xy, int* ages, int* strengths);

/* the same with a detection mask over the whole list (the tracks passed in, then the FAST hits); features_per_bucket must be 1 */
int svo_append_features_from_image_masked(int device, const svo_config* cfg, const uint8_t* img, int w, int h, int stride,
                                          int fast_threshold, const uint8_t* mask, int mask_stride, int cap, int* n_io,
                                          float* xy, int* ages, int* strengths);

/* replaces: cv::buildOpticalFlowPyramid(img, pyr, winSize, maxLevel)  (vo.cpp:50,52,200,201).
 * Returns the levels as tightly packed u8 images concatenated in `levels_out` (level l is
 * w_l*h_l bytes, w_l=(w_{l-1}+1)/2); n_levels_out <= max_level+1 (stops when the next level would
 * not exceed the window; win >= 7).  Derivatives are not materialised (they are fused into the LK kernel). */
int svo_build_pyramid(int device, const uint8_t* img, int w, int h, int stride, int win, int max_level,
                      uint8_t* levels_out, int64_t levels_cap, int* n_levels_out);

/* replaces: cv::calcOpticalFlowPyrLK(prevPyr, nextPyr, prevPts, nextPts, status, err, winSize, maxLevel, termcrit, 0, minEig)
 * (vo.cpp:203-215) on two images (pyramids are built internally). */
int svo_lk_track(int device, const uint8_t* prev_img, const uint8_t* next_img, int w, int h, int stride,
                 int n, const float* prev_pts, float* next_pts, uint8_t* status,
                 int win, int max_level, int max_count, double epsilon, double min_eig_threshold);

/* The same with OPTFLOW_USE_INITIAL_FLOW (the motion-prior section: LK with a guess): guess_pts (n x 2) is where the top level's
 * search of each point starts.  guess_pts == prev_pts gives svo_lk_track's bits. */
int svo_lk_track_guess(int device, const uint8_t* prev_img, const uint8_t* next_img, int w, int h, int stride,
                       int n, const float* prev_pts, const float* guess_pts, float* next_pts, uint8_t* status,
                       int win, int max_level, int max_count, double epsilon, double min_eig_threshold);

/* replaces: VisualOdometry::circularMatching  (vo.h:374-379, vo.cpp:169-240) without the compaction:
 * the four LK passes L0->L1->R1->R0->L0, fused in one kernel, plus the status / loop-closure mask
 * (vo.cpp:217-230).  Outputs n points each and ok[n]. */
int svo_circular_match(int device, const svo_config* cfg, const uint8_t* l0, const uint8_t* r0,
                       const uint8_t* l1, const uint8_t* r1, int w, int h, int stride,
                       int n, const float* pl0, float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok);

/* The same with a motion prior (the motion-prior section: circular matching with a prior) on k_lk_chain_prior, all four passes run:
 * H maps T0 pixels to T1 pixels; Hi its inverse, or NULL: the library inverts H.  cfg->channels and cfg->lk_float_sums are taken as
 * 1 and 0.  SVO_ERR_ARG as svo_set_motion_prior's.  H = identity gives svo_circular_match's bits. */
int svo_circular_match_prior(int device, const svo_config* cfg, const uint8_t* l0, const uint8_t* r0,
                             const uint8_t* l1, const uint8_t* r1, int w, int h, int stride,
                             int n, const float* pl0, const float H[9], const float Hi[9],
                             float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok);

/* replaces: findClosePoints(points_1, points_2, threshold)  (vo.h:430-432, vo.cpp:265-280) */
int svo_find_close_points(int device, int n, const float* p1, const float* p2, float threshold, uint8_t* ok);

/* replaces: cv::triangulatePoints + cv::convertPointsFromHomogeneous  (vo.cpp:89-94). xyz: n x 3 float32. */
int svo_triangulate(int device, const float Pl[12], const float Pr[12], int n, const float* pts_l, const float* pts_r, float* xyz);

/* replaces: cameraToWorld(K, cameraPoints, worldPoints, rotation, translation) -> pair<inliers, success>
 * (vo.h:452-456, vo.cpp:282-313) = cv::solvePnPRansac(.., useExtrinsicGuess, iterations, reprojErr, confidence, inliers, ITERATIVE).
 * K 3x3 f32; R (3x3 f64) and t (3 f64) in/out; inliers: int32[n]; *success = the pair's .second.
 * Small inputs follow cv::solvePnPRansac: n == 5 is one direct EPnP solve and n == 4 one direct P3P solve (every point an
 * inlier, no RANSAC, no refine); n < 4 is SVO_ERR_ARG (OpenCV asserts npoints >= 4). */
int svo_camera_to_world(int device, const float K[9], int n, const float* cam_pts, const float* world_pts,
                        double R[9], double t[3], int* inliers, int* n_inliers, int* success,
                        int ransac_iterations, float reproj_error, float confidence, int* iters_run);

/* The pose covariance of the section above for one point set and one pose, on the frame pipeline's device function: the
 * counterpart of svo_camera_to_world, taking its inputs (K, cam_pts n x 2 f32, world_pts n x 3 f32) and its outputs R and t.
 * inliers: n FLAGS (non-zero = the point counts), NULL = every point — NOT svo_camera_to_world's list of n_inliers indices:
 * set flags[index[k]] = 1 for k < n_inliers first.  mode SVO_COV_RESIDUAL or SVO_COV_FIXED_SIGMA.  cov_p, cov_T (36 doubles each) and valid may be
 * NULL.  n < 1 or a bad mode / pixel_sigma: SVO_ERR_ARG; a singular H is valid = 0 and zeros, not an error. */
int svo_pose_covariance(int device, const float K[9], int n, const float* cam_pts, const float* world_pts,
                        const int* inliers, const double R[9], const double t[3],
                        int mode, double pixel_sigma, double cov_p[36], double cov_T[36], int* valid);

/* replaces: cv::initUndistortRectifyMap(K, D, R, P[:, :3], (w, h), CV_16SC2, map1, map2) (the map half of
 * image_geometry::PinholeCameraModel::rectifyImage).  Host only, f64, no device needed.  The scalar loop restated exactly
 * (no FMA contraction): iR = (P33 R)^-1 by the 3x3 adjugate / determinant; per row i: _x = i ir[1] + ir[2], _y = i ir[4] + ir[5],
 * _w = i ir[7] + ir[8], stepped by += ir[0], ir[3], ir[6] per column; w = 1/_w, x = _x w, y = _y w; r2 = x^2 + y^2;
 * kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2); xd = x kr + p1 2xy + p2 (r2 + 2x^2),
 * yd = y kr + p1 (r2 + 2y^2) + p2 2xy; u = fx xd + cx, v = fy yd + cy; ix = round_half_even(32 u) (likewise iy; outside the
 * int32 range: INT_MIN, as cvRound).  R NULL = identity, P NULL = K.  map1: w*h*2 int16, map2: w*h uint16. */
int svo_init_rectify_map(const double K[9], const double* D, int n_d, const double R[9], const double P[12], int w, int h,
                         int16_t* map1, uint16_t* map2);

/* replaces: cv::remap(raw, out, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) (the per-frame half of rectifyImage): the remap
 * of the rectification section alone, on the kernel's device function.  out: w*h*channels bytes, packed; raw rows raw_stride
 * bytes apart; channels 1 or 3 (interleaved). */
int svo_rectify_image(int device, const int16_t* map1, const uint16_t* map2, int w, int h, const uint8_t* raw, int raw_w, int raw_h,
                      int raw_stride, int channels, uint8_t* out);

/* replaces: cv::cvtColor(src, out, COLOR_*2GRAY) / cv_bridge's MONO8 conversion: the grey conversion of the input-format section
 * alone, on the kernels' device functions.  src: h rows of w pixels in `format` (SVO_INPUT_*), `stride` bytes apart; out: w*h
 * bytes, packed. */
int svo_convert_gray(int device, int format, const uint8_t* src, int w, int h, int stride, uint8_t* out);

/* replaces: cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply(grey(src), out): the CLAHE section's stage alone, on the
 * frame pipeline's two kernels.  src: h rows of w pixels in `format` (SVO_INPUT_*), `stride` bytes apart; out: w*h grey bytes,
 * packed.  SVO_ERR_ARG as svo_set_clahe's. */
int svo_clahe(int device, int format, const uint8_t* src, int w, int h, int stride,
              double clip_limit, int tiles_x, int tiles_y, uint8_t* out);

/* The descriptor section's stage alone, on the frame pipeline's device function: the descriptors (n rows of 32 bytes) and, when bins
 * is not NULL, the orientation bins of n points xy (x, y pairs) of the w x h grey image img, rows `stride` bytes apart.  n = 0 is
 * legal.  SVO_ERR_ARG: w or h < 16, stride < w, a non-finite coordinate.  Not cv::ORB's output (see the section above). */
int svo_describe_points(int device, const uint8_t* img, int w, int h, int stride, int n, const float* xy, uint8_t* desc, int* bins);

/* replaces: getInverseTransform(rotation, translation)  (vo.h:469-470, vo.cpp:246-258): [R t; 0 1]^-1, 4x4 row-major.
 * Runs the device function the frame pipeline ends with (one tiny launch). */
int svo_inverse_transform(int device, const double R[9], const double t[3], double T[16]);

#ifdef __cplusplus
}
#endif
#endif
