/*
 * orc.h — CPU ORACLE for the stereo-VO per-frame front end.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load the library built from this directory.  The
 * product path (stereo_visual_odometry_amd/csrc) never includes, links or calls it.
 *
 * What it is: a plain-C restatement of the reference pipeline
 *   /root/reference/src/vo.cpp, /root/reference/src/feature_set.cpp, /root/reference/include/vo.h
 * and of the OpenCV 4.5.x functions that pipeline calls (cv::FAST, cv::buildOpticalFlowPyramid,
 * cv::calcOpticalFlowPyrLK, cv::triangulatePoints, cv::convertPointsFromHomogeneous,
 * cv::solvePnPRansac, cv::Rodrigues).  OpenCV is a third-party dependency that is NOT vendored
 * in the reference and NOT present in this image (the reference links libopencv_*.so.405, i.e.
 * OpenCV 4.5.x, unpinned by any manifest: Makefile:4 uses pkg-config opencv4).  Its published
 * algorithms are restated here from the OpenCV 4.5 documentation / sources as known; every
 * function cites the reference call site it stands in for.
 *
 * Parity pin status (see DESIGN.md "Oracle"):
 *   - END TO END, against output the reference itself recorded: fed the BGR frames of the reference's run1/ data set the
 *     way its CLI feeds them (orc_vo_stereo_callback_cn, cn = 3), the whole pipeline reproduces run1/result.csv to
 *     <= 1e-6 m absolute (3-4 of the 6 digits the file prints) for the first 13 frames; what happens after that, per
 *     deviation below, is MEASURED by tools/deviation_ablation.py (table in tests/golden/deviation_ablation.txt).
 *   - Bucket / FeatureSet logic, findClosePoints: pinned by the reference's own known-answer
 *     tests (src/main.cpp:50-78, 102-172), restated in tests/test_oracle_kat.py.
 *   - FAST-9/16 + NMS: pinned by test_featureset (src/main.cpp:102-127): 11 features, strength<=128.
 *   - pyramid + LK + circular mask: pinned by test_circularMatching (src/main.cpp:174-209): 121/121.
 *   - RANSAC-PnP + LM refine: pinned by test_cameraToWorld (src/main.cpp:211-264): R,t to 1e-8/1e-6.
 *   - Bit-level equality with OpenCV for LK / PnP / triangulation: PARITY UNPINNED (no OpenCV
 *     here, the reference binary cannot run, and no reference test covers triangulatePoints);
 *     the recording above bounds the accumulated difference at 1e-6 m per frame.
 *
 * Deliberate, documented deviations from OpenCV numerics (all inside the pose tolerance).  What each one does to the agreement
 * with the reference's recording is MEASURED (tools/deviation_ablation.py -> tests/golden/deviation_ablation.txt):
 *   D1 causes the disagreements at frames 14, 15, 22, 23 (and, through the changed feature sets, everything after);
 *   D2, D4 cause none; D5 in force reproduces all 128 rows, reverted it loses frames 25 and 57 (the basis of a numerically
 *   zero singular subspace is decided by rounding noise; OpenCV's own is unknowable without its exact SVD build).
 * With D1 reverted (ORC_OCV_D1_LK_FLOAT — also an opt-in mode of the HIP path, svo_config.lk_float_sums) the oracle prints
 * 127 of the 128 rows of run1/result.csv digit for digit (383 of 384 values; the last differs by one unit of the sixth digit).
 *   D1. LK accumulates A11,A12,A22,b1,b2 as exact int64 sums and converts to float once
 *       (OpenCV: float accumulation in SIMD-lane order, which is not reproducible).  This makes
 *       the validity masks bit-reproducible between this oracle and the HIP kernels.
 *   D2. The final LM refine of solvePnPRansac starts from the best RANSAC model (OpenCV 4.5:
 *       from whichever hypothesis was evaluated last, because rvec/tvec alias the callback's
 *       buffers).
 *   D3. (REMOVED in round 3.)  Rounds 1-2 took EPnP's null-space basis from the right singular vectors of the one-sided
 *       Jacobi SVD; OpenCV reads the left ones (Ut).  Measured on the recording: with D1 reverted, the right-vector form flips
 *       an inlier decision at frame 25 (1.6 mm), the left-vector form reproduces all 128 rows.  Oracle and HIP path now read
 *       the left vectors; ORC_ALT_D3_RIGHT brings the old form back for the ablation table.
 *   D4. RANSAC hypotheses are scored with the EPnP rotation matrix directly instead of the
 *       R -> rvec -> R round trip through cv::Rodrigues (identity up to 1 ulp); this keeps the
 *       inlier masks free of libm (sin/cos/acos) and therefore bit-reproducible on the GPU.
 *   D5. EPnP's 12x12 Jacobi SVD sweeps its row pairs in round-robin (Brent-Luk) order instead of OpenCV's
 *       cyclic-by-rows order: same algorithm and convergence test, different (equally valid) pair schedule,
 *       chosen because the n/2 pairs of a round are independent and the GPU rotates them in parallel.
 *   D6. PARITY UNPINNED.  A solve whose R or t holds a non-finite value is a failed solve: cameraToWorld returns success = 0,
 *       leaves R and t untouched and reports no inliers (fail_reason 3 in the frame pipeline) — the direct 5-point EPnP, the
 *       direct P3P and the refined pose of the RANSAC path alike.  Without it five exactly coplanar points come back as
 *       "success, 5 inliers, R = t = NaN": the fourth control point coincides with the centroid, every alpha_3 is 0, L keeps one
 *       non-zero column, approximation 1 solves b4 = 0 and forms betas[1] = b4[1] / sqrt(b4[0]) = 0 / 0
 *       (find_betas_approx_1; approximation 3 the same with b5[3] / sqrt(b5[0]); approximation 2 gives R = 0 and a NaN
 *       reprojection error), and no NaN error is "smaller" than another, so N stays 1.  A NaN pose passes the motion gate
 *       (tn > max || angle > max is false for NaN) and would be multiplied into the caller's trajectory.  What OpenCV returns
 *       for this input cannot be pinned here (no OpenCV); the same expressions stand in its epnp.cpp.  No finite result changes.
 */
#ifndef ORC_H
#define ORC_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORC_MAX_LEVELS 8

/* ---- configuration: the reference's compile-time constants (include/vo.h:53-127,251-252) ---- */
typedef struct {
    int bucket_start_row;        /* vo.h:53  = 4   */
    int buckets_along_height;    /* vo.h:60  = 92  */
    int buckets_along_width;     /* vo.h:61  = 160 */
    int features_per_bucket;     /* vo.h:65  = 1   */
    int features_threshold;      /* vo.h:71  = 15  */
    int pre_matching_feature_threshold; /* vo.h:78 = 100 */
    int age_threshold;           /* vo.h:84  = 20  */
    int fast_threshold;          /* vo.h:90  = 20  */
    float ransac_reprojection_error; /* vo.h:97 = 8 */
    int ransac_iterations;       /* vo.h:102 = 100 */
    double optical_flow_min_eig_threshold; /* vo.h:108 = 0.001 */
    double circular_matching_success_threshold; /* vo.h:115 = 0.15 */
    double max_translation_norm; /* vo.h:121 = 0.1 */
    double max_rotation_norm;    /* vo.h:127 = 0.5 */
    int win_w, win_h;            /* vo.h:251 = 10,10 */
    int max_level;               /* vo.h:252 = 3 */
    int lk_max_count;            /* vo.cpp:183 = 30 */
    double lk_epsilon;           /* vo.cpp:184 = 1e-4 */
    float ransac_confidence;     /* vo.cpp:295 = 0.98f (a float32 in the reference) */
    int max_features;            /* build preset, NOT in the reference: 0 = unlimited; >0 keeps the
                                    first max_features of the bucketed set */
    int channels;                /* 1 = single-channel input (default), 3 = interleaved BGR as the reference CLI feeds (B-1) */
    int lk_float_sums;           /* mirror of svo_config.lk_float_sums: 1 = this object's LK passes run with D1 reverted (ORC_OCV_D1_LK_FLOAT) */
} orc_config;

void orc_config_default(orc_config* c);
/* threads used by the data-parallel loops (points inside each LK pass, image rows) — OpenCV's parallel_for_ analogue.
   n <= 0 selects all cores; returns the count in effect.  Results do not depend on it. */
int orc_set_threads(int n);

/* ---- deviation switches (tools/deviation_ablation.py; CPU only — the product has no such switch unless DESIGN.md §3 says so) ----
 * Each bit REVERTS one documented deviation D1..D5 (see the header comment) to what OpenCV 4.5 does, so that the effect of
 * every deviation on the reference's own recording (run1/result.csv) can be measured one at a time.  0 = the oracle as the
 * HIP path is checked against.  The variants of D1 exist because the exact SIMD flavour of the reference's OpenCV build
 * (lkpyramid.cpp is compiled at the library's CPU baseline) is unknown. */
#define ORC_OCV_D1_LK_FLOAT      0x01u  /* LK sums in float, lkpyramid.cpp's CV_SIMD128 order (8 interleaved elements per step) */
#define ORC_OCV_D2_LM_FROM_LAST  0x02u  /* the final LM starts from the LAST evaluated hypothesis (rvec/tvec alias the callback's) */
#define ORC_ALT_D3_RIGHT         0x04u  /* NOT a revert: puts the FORMER deviation D3 back (EPnP basis from the right singular vectors) —
                                           rounds 1-2 behaviour, kept for the ablation table only */
#define ORC_OCV_D4_RVEC_TRIP     0x08u  /* hypotheses stored as rvec|tvec: scoring goes R -> rvec -> R through cv::Rodrigues */
#define ORC_OCV_D5_JACOBI_CYCLIC 0x10u  /* EPnP's 12x12 Jacobi SVD sweeps cyclic-by-rows (JacobiSVDImpl_) */
#define ORC_OCV_HYPOT            0x20u  /* every Jacobi rotation computes gamma = hypot(p, beta) with libm, as JacobiSVDImpl_ does (oracle: sqrt(p*p + beta*beta)) */
#define ORC_ALT_J12_HALVES       0x1000u /* experiment: the 12-term sums of EPnP's 12x12 Jacobi as two halves (lane-parallel form) */
#define ORC_ALT_J12_QUARTERS     0x2000u /* experiment: ... as four quarters of three */
#define ORC_ALT_TRI_RR           0x4000u /* experiment: the 4x4 Jacobi of the triangulation sweeps in round-robin order */
#define ORC_OCV_D1_FMA           0x100u /* with D1: v_muladd fused (an AVX2/FMA3-baseline build) */
#define ORC_OCV_D1_W4            0x200u /* with D1: the OpenCV 3.x SSE2 form (4 elements per step for A, sequential 4-lane reduce) */
#define ORC_OCV_D1_SCALAR        0x400u /* with D1: no SIMD at all (plain float accumulation in element order) */
unsigned orc_set_opencv_mode(unsigned mask);    /* returns the previous mask */
unsigned orc_get_opencv_mode(void);

/* ---- FAST-9/16 (cv::FAST, called at feature_set.cpp:61) ---- */
/* Writes NMS-surviving corner scores (0 elsewhere) into score[h*w]. nonmax=0 writes raw corner flags as score. */
void orc_fast_score_map(const uint8_t* img, int w, int h, int stride, int threshold, int nonmax, uint8_t* score);
/* Raster-ordered keypoints like cv::FAST + KeyPoint::convert (feature_set.cpp:55-68).
   xy = 2*cap floats, resp = cap floats. Returns the TOTAL count (may exceed cap; only cap are written). */
int orc_fast_detect(const uint8_t* img, int w, int h, int stride, int threshold, int nonmax,
                    int cap, float* xy, float* resp);

/* ---- Bucket / FeatureSet (feature_set.cpp:1-152) ---- */
typedef struct {
    int max_size, n;
    float* xy; int* ages; int* strengths;   /* capacity max_size */
} orc_bucket;
void orc_bucket_init(orc_bucket* b, int max_size);
void orc_bucket_free(orc_bucket* b);
int  orc_bucket_compute_score(int age, int strength, int fast_threshold);   /* feature_set.cpp:16-18 */
void orc_bucket_add_feature(orc_bucket* b, float x, float y, int age, int strength,
                            int age_threshold, int fast_threshold);        /* feature_set.cpp:20-53 */
/* FeatureSet::filterByBucketLocationInternal (feature_set.cpp:95-147). In place; returns new n. */
int orc_bucket_filter(int img_w, int img_h, int n, float* xy, int* ages, int* strengths,
                      int buckets_along_height, int buckets_along_width, int bucket_start_row,
                      int features_per_bucket, int age_threshold, int fast_threshold);

/* ---- pyramid (cv::buildOpticalFlowPyramid, vo.cpp:50,52,200,201) ---- */
typedef struct {
    int nlevels;                 /* levels actually built */
    int pad_x, pad_y;            /* = winSize */
    int w[ORC_MAX_LEVELS], h[ORC_MAX_LEVELS];
    uint8_t* img[ORC_MAX_LEVELS];   int img_stride[ORC_MAX_LEVELS];    /* pointer to pixel (0,0) of a padded buffer */
    int16_t* deriv[ORC_MAX_LEVELS]; int deriv_stride[ORC_MAX_LEVELS];  /* int16 units; interleaved (dx,dy) */
    void* owned[2 * ORC_MAX_LEVELS];
} orc_pyramid;
void orc_pyr_down(const uint8_t* src, int sw, int sh, int sstride, uint8_t* dst, int dstride); /* dst is ((sw+1)/2,(sh+1)/2) */
void orc_scharr(const uint8_t* src, int w, int h, int sstride, int16_t* dst, int dstride);       /* calcSharrDeriv */
void orc_build_pyramid(const uint8_t* img, int w, int h, int stride, int win_w, int win_h, int max_level, orc_pyramid* out);
void orc_pyramid_free(orc_pyramid* p);

/* ---- pyramidal LK (cv::calcOpticalFlowPyrLK, vo.cpp:203-215) ---- */
void orc_lk_track(const orc_pyramid* prev, const orc_pyramid* next, int n, const float* prev_pts,
                  float* next_pts, uint8_t* status, int win_w, int win_h, int max_level,
                  int max_count, double epsilon, double min_eig_threshold);

/* Multi-channel form (cv::calcOpticalFlowPyrLK with cn = image channels: the window sums run over all channels of every
 * pixel, lkpyramid.cpp LKTrackerInvoker `x < winSize.width*cn`).  prev / next: cn single-channel pyramids, one per colour
 * plane — plane k of a pyramid built from an interleaved image equals channel k of OpenCV's cn-channel pyramid, because
 * pyrDown, the Scharr derivative and the bilinear patch sampling all act per channel.  cn = 1 is orc_lk_track. */
#define ORC_MAX_CN 3
void orc_lk_track_cn(int cn, const orc_pyramid* const* prev, const orc_pyramid* const* next, int n, const float* prev_pts,
                     float* next_pts, uint8_t* status, int win_w, int win_h, int max_level,
                     int max_count, double epsilon, double min_eig_threshold);
/* channel k of an interleaved cn-channel image -> contiguous w x h plane */
void orc_extract_plane(const uint8_t* img, int w, int h, int stride, int cn, int k, uint8_t* plane);

/* ---- helpers (vo.cpp:144-168, 265-280) ---- */
void orc_find_close_points(int n, const float* p1, const float* p2, float threshold, uint8_t* ok);

/* ---- circularMatching (vo.cpp:169-240) on prebuilt pyramids; returns the mask, no compaction ---- */
void orc_circular_match(const orc_pyramid* l0, const orc_pyramid* r0, const orc_pyramid* l1, const orc_pyramid* r1,
                        int n, const float* pl0, float* pl1, float* pr1, float* pr0, float* pl0_circle,
                        uint8_t* ok, const orc_config* cfg);

void orc_circular_match_cn(int cn, const orc_pyramid* const* l0, const orc_pyramid* const* r0, const orc_pyramid* const* l1,
                           const orc_pyramid* const* r1, int n, const float* pl0, float* pl1, float* pr1, float* pr0,
                           float* pl0_circle, uint8_t* ok, const orc_config* cfg);

/* ---- triangulation (cv::triangulatePoints + convertPointsFromHomogeneous, vo.cpp:89-94) ---- */
void orc_triangulate(const float Pl[12], const float Pr[12], int n, const float* pts_l, const float* pts_r,
                     float* xyz /* 3n */, float* homog /* 4n or NULL */);

/* ---- Rodrigues (cv::Rodrigues, vo.cpp:125,289,308) ---- */
void orc_rodrigues_to_matrix(const double r[3], double R[9], double dRdr[27] /* or NULL */);
void orc_rodrigues_to_vector(const double R[9], double r[3]);

/* ---- RANSAC-PnP (cv::solvePnPRansac via cameraToWorld, vo.cpp:282-313) ---- */
typedef struct { uint64_t state; } orc_rng;
void     orc_rng_init(orc_rng* r, uint64_t seed);
uint32_t orc_rng_next(orc_rng* r);
int      orc_rng_uniform(orc_rng* r, int a, int b);
int      orc_ransac_update_num_iters(double p, double ep, int model_points, int max_iters);

/* EPnP on n>=4 points (object f64, image pixel coords f64). K = fx,fy,cx,cy. Outputs R (row-major), t. Returns mean reproj err. */
/* cv::solvePnP(SOLVEPNP_P3P) on exactly four points (orc_p3p.c): the branch solvePnPRansac takes for npoints == 4 */
int orc_p3p(const double obj[12], const double img[8], double fx, double fy, double cx, double cy, double R[9], double t[3]);
double orc_epnp(int n, const double* obj, const double* img, double fx, double fy, double cx, double cy,
                double R[9], double t[3]);
/* Levenberg–Marquardt refine as cvFindExtrinsicCameraParams2(useExtrinsicGuess=1). rvec,tvec in/out. returns iterations used */
int orc_pnp_refine_lm(int n, const double* obj, const double* img, double fx, double fy, double cx, double cy,
                      double rvec[3], double tvec[3]);
/* cameraToWorld (vo.cpp:282-313). K = 3x3 f32 row-major. world = 3n f32, cam = 2n f32.
   R (3x3 f64) and t (3 f64) are in/out (guess in, result out on success; unchanged on failure).
   inliers: int32[n] ascending indices, *n_inliers count. Returns success (1/0).
   dbg (optional, may be NULL): dbg[0]=iterations run, dbg[1]=best inlier count. */
int orc_camera_to_world(const float K[9], int n, const float* cam_pts, const float* world_pts,
                        double R[9], double t[3], int* inliers, int* n_inliers,
                        int ransac_iterations, float reproj_error, float confidence, int* dbg);

/* ---- getInverseTransform (vo.cpp:246-258) ---- */
void orc_inverse_transform(const double R[9], const double t[3], double T[16]);

/* ---- VisualOdometry (vo.cpp:41-137; state vo.h:233-269) ---- */
typedef struct orc_vo orc_vo;
typedef struct {
    int n_after_detect;     /* feature-set size after appendFeaturesFromImage (vo.cpp:326 / :331) */
    int second_pass;        /* 1 if the FAST_THRESHOLD/4 pass ran (vo.cpp:327-332) */
    int n_into_lk;          /* after max_features cap */
    int n_after_circular;   /* vo.cpp:239 */
    int n_after_bounds;     /* vo.cpp:365 */
    int n_inliers;          /* vo.cpp:103 */
    int ransac_iters;
    int fail_reason;        /* 0 ok, 1 first frame, 2 too few tracks, 3 ransac fail / few inliers, 4 motion gate */
    int n_features_out;     /* size of currentVOFeatures when the callback returns */
    int lk_level_visits;    /* (point, pass, level) visits that reached the Newton loop, over the passes a feature runs: up to and including its first pass with status 0 */
    int lk_newton_steps;    /* Newton iterations of those passes */
    int lk_dead_after_pass[3]; /* features whose status first became 0 in pass k = 0 (L0->L1), 1 (L1->R1), 2 (R1->R0): vo.cpp:227-238 deletes them whatever the later passes return */
} orc_frame_stats;
typedef struct { long long level_visits, newton_steps; int dead_after_pass[3]; } orc_lk_chain_stats;
extern orc_lk_chain_stats orc_last_chain_stats;   /* of the last orc_circular_match_cn call */
extern long long orc_lk_counters[4];   /* running totals: [0] level visits that reached the Newton loop, [1] Newton iterations, [2] all visits */

orc_vo* orc_vo_create(const orc_config* cfg);
void    orc_vo_destroy(orc_vo* vo);
void    orc_vo_set_projection(orc_vo* vo, const float Pl[12], const float Pr[12]);   /* vo.cpp:8-26 */
/* returns 1 if ok (pose produced), 0 otherwise; T_out always gets the "second" of the pair (vo.cpp:43-44,136). */
int     orc_vo_stereo_callback(orc_vo* vo, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                               double T_out[16], orc_frame_stats* stats);
/* The same callback on cn-channel interleaved images (cn = 1 or 3; stride in bytes).  cn = 3 restates what the reference CLI
 * really runs: readImages returns the BGR Mats (main.cpp:38-46), so cv::FAST — which has no channel
 * check — walks the first `w` BYTES of every row of the interleaved image (byte column = keypoint x), while the pyramids and LK
 * are genuinely 3-channel.  Pinned by the reference's own recording: run1/result.csv (tests/test_run1_color.py). */
int     orc_vo_stereo_callback_cn(orc_vo* vo, const uint8_t* left, const uint8_t* right, int w, int h, int stride, int cn,
                                  double T_out[16], orc_frame_stats* stats);
/* introspection for parity tests */
int     orc_vo_num_features(const orc_vo* vo);
void    orc_vo_get_features(const orc_vo* vo, float* xy, int* ages, int* strengths);
void    orc_vo_get_pose_guess(const orc_vo* vo, double R[9], double t[3]);
/* last frame's compacted tracks (after bounds mask): 4 point lists + world points + inlier flags. returns n */
int     orc_vo_get_last_tracks(const orc_vo* vo, float* pl0, float* pr0, float* pl1, float* pr1, float* world, uint8_t* inlier);

#ifdef __cplusplus
}
#endif
#endif
